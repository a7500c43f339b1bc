"""Scenes for the pre-pass's second stage (csrc/dog_prune.hpp, "the cell bound"), shared by tests/test_prune_refine_cpu.py (the
restatement against the response maps) and tests/test_gpu_prune_refine.py (the kernel against the restatement).  A SET is one
tracker geometry — kernel length, window, frame, sign — with a handful of windows; everything is built once and left unchanged.
Test code only."""
import numpy as np

import fp32_restatement as fr
import prune_restatement as pr
import prune_refine_restatement as rr

FILL = 128


def tw_for_kernel_len(l):
    for tw10 in range(20, 1400):
        if fr.kernel_len(fr.sigma_of(tw10 / 10)) == l:
            return tw10 / 10
    raise AssertionError(l)


def _frame(fh, fw, discs, rad, value, background=FILL, noise=0, seed=0):
    f = np.full((fh, fw), background, np.uint8)
    ii, jj = np.ogrid[:fh, :fw]
    for cy, cx in discs:
        f[(ii - cy) ** 2 + (jj - cx) ** 2 <= rad * rad] = value
    if noise:
        rng = np.random.default_rng(seed)
        f = np.clip(f.astype(np.int16) + rng.integers(-noise, noise + 1, f.shape), 0, 255).astype(np.uint8)
    return f


class Scene:
    def __init__(self, name, frame, guess, target, quiet):
        self.name, self.frame, self.guess = name, frame, guess
        self.target = target      # a target is in the window
        self.quiet = quiet        # … and the noise is at most ±3 levels: the second stage must take something away


class Set:
    """name, l, window (n1, n2), darker; scenes; per scene the tile, the first stage (pp) and the second (rf)."""

    def __init__(self, name, l, ws, darker, margin=6):
        self.name, self.l, self.ws, self.darker, self.fill = name, l, ws, darker, FILL
        self.tw = 6.0 if l == 17 else tw_for_kernel_len(l)   # (l = 17 from 5.0 on: at 6 the L pixels always meet the disc)
        assert fr.kernel_len(fr.sigma_of(self.tw)) == l
        self.radii = (ws[0] // 2, ws[1] // 2)
        n1, n2 = ws
        self.fh, self.fw = n1 + l - 1 + 2 * margin, n2 + l - 1 + 2 * margin
        self.centre = (self.fh // 2 + 1, self.fw // 2 + 1)                    # a 1-based guess whose tile lies inside the frame
        self.w0 = (self.centre[0] - n1 // 2 - 1, self.centre[1] - n2 // 2 - 1)  # 0-based frame row / column of window pixel (0, 0)
        self.rad = max(2, int(self.tw) // 2)
        self.scenes = []
        self._done = None

    def add(self, name, discs, noise=0, seed=0, guess=None, target=True, strict=True):
        """discs: window coordinates (row, column) of the centres.  strict=False: a scene of this file's own, beyond the list the
        second stage is held to, on which it need not take anything away."""
        value = 0 if self.darker else 255
        at = [(self.w0[0] + y, self.w0[1] + x) for y, x in discs]
        f = _frame(self.fh, self.fw, at, self.rad, value, noise=noise, seed=seed)
        self.scenes.append(Scene(name, f, guess or self.centre, target and bool(discs), strict and target and bool(discs) and noise <= 3))

    def stages(self):
        if self._done is None:
            self._done = []
            for sc in self.scenes:
                tile = fr.window_tile(sc.frame, self.fill, self.l, self.radii, sc.guess)
                pp = pr.prepass(tile, self.fill, self.tw, self.darker)
                self._done.append((tile, pp, rr.refine(tile, self.fill, self.tw, self.darker, pp)))
        return self._done

    def frames(self):
        return np.stack([sc.frame for sc in self.scenes])

    def guesses(self):
        return np.array([sc.guess for sc in self.scenes], np.int32)

    def nstrips(self):
        return sum(1 for _, w in pr.slots(self.ws[1]) if w > 1 or self.ws[1] == 1)

    def jobs(self, refined):
        """The sorted (window, strip, first block, one past the last) of the non-empty strip ranges."""
        out = []
        for b, (_, pp, rf) in enumerate(self.stages()):
            for s, (ba, bb) in enumerate((rf if refined else pp)["hull"][:self.nstrips()]):
                if bb > ba:
                    out.append((b, s, ba, bb))
        return sorted(out)

    def counts(self):
        """(kept, total) of the first stage, what pdog_get_prune_counts reports."""
        pairs = [pr.kept_pairs(pp, self.l) for _, pp, _ in self.stages()]
        return sum(k for k, _ in pairs), sum(t for _, t in pairs)


def _common(st, two_strips):
    n1, n2 = st.ws
    # (l = 17: rows at which the first stage's L pixels meet the 7-pixel disc — at every third row or so they miss it and the
    # first stage already keeps everything, tests/test_prune_cpu.py — and the second stage then has a block to take away)
    st.add("disc", [(21 if st.l == 17 else n1 // 2 + 3, n2 // 3)])
    st.add("disc-noise3", [(23, n2 // 3) if st.l == 17 else (n1 // 2 - 5, n2 // 3 + 4)], noise=3, seed=1)
    st.add("first-rows", [(1, n2 // 2)], noise=2, seed=2)
    # (l = 17: the disc's two blocks are the window's last, and the L pixels may miss it — nothing is left to take away)
    st.add("last-rows", [(n1 - 2, n2 // 2 + 3)], noise=2, seed=3, strict=st.l != 17)
    st.add("noise40", [(n1 // 2, n2 // 2)], noise=40, seed=4)
    st.add("flat", [])
    st.add("noise-only", [], noise=3, seed=5)
    # over the frame's corner: the guess near (1, 1), the disc inside the frame and inside the window
    st.add("corner", [], noise=2, seed=6, guess=(3, 4))
    st.scenes[-1].frame[:] = _frame(st.fh, st.fw, [(14 if st.l == 17 else st.rad + 4, st.rad + 6)], st.rad, 0 if st.darker else 255, noise=2, seed=6)
    st.scenes[-1].target = st.scenes[-1].quiet = True
    if two_strips:
        st.add("boundary", [(n1 // 2 + (3 if st.l == 17 else 0), 64)], noise=1, seed=7)                      # centred on the strips' boundary
        # equal, in different strips: both stay.  (l = 17, NS = 3: with two equal discs L reaches about two thirds of the peak and
        # the restatement takes no block away at any of the rows 16 … 31 tried: not held to `strictly fewer` there)
        st.two = [(n1 // 4, 20), (n1 - n1 // 4, n2 - 20)]
        st.add("two-discs", st.two, noise=1, seed=8, strict=st.l != 17)


_SETS = None


def sets():
    """l = 17, 65, 109 (NS = 3, 9, 15; both entry steps of roll_entry_step); one-strip windows whose height is no multiple of 8;
    101 × 129 (two strips and a remainder column); 61 × 101 (the second strip shifted to column 37); bright targets."""
    global _SETS
    if _SETS is None:
        out = []
        for name, l, ws, darker, two in (("l17-one-strip", 17, (45, 45), True, False), ("l17-strips-remainder", 17, (101, 129), True, True),
                                         ("l65-one-strip", 65, (77, 45), True, False), ("l65-strips-remainder", 65, (101, 129), True, True),
                                         ("l65-shifted-bright", 65, (61, 101), False, True), ("l109-shifted", 109, (61, 101), True, True)):
            st = Set(name, l, ws, darker)
            _common(st, two)
            out.append(st)
        _SETS = out
    return _SETS
