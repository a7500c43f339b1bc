"""Hard windows for any kernel length: the scenes of tests/test_gpu_exact_lengths.py, and the one table through which that
file and tests/test_exact_scenes_cpu.py read them.

hard_windows generalises tests/test_gpu_exact.py's _hard_windows (45 x 45 windows, l = 65, dark targets, level = fill = 128) to
any kernel length, window shape, sign, background level and fill.  Sizes follow the target: tw = tw_for_kernel_len(l),
rad = max(2, int(tw) // 2).  One frame per window, just large enough for an interior tile under a guess jitter of +-JIT:
(n1 + l - 1 + 2 JIT) x (n2 + l - 1 + 2 JIT).  Six families:
    0  noise only, +-1 ... +-3 levels about `level`
    1  a disc of even diameter (its centre between pixels) one grey level from `level`, of the target's sign, half of them
       under +-1 noise
    2  two discs mirrored about the window centre, the second 0 or 1 level fainter.  Where the window is two strips wide, half
       of the pairs lie in different 64-column strips and half in one; where the width leaves remainder columns (1 ... 6 beyond
       whole strips) a quarter of the pairs put the second disc's centre into them; `min_sep` keeps both offsets large (pairs
       across the tiled kernel's sub-window borders)
    3  an even-sized rectangle whose centre falls between pixels: 2 or 4 mathematically tied pixels
    4  the easy control: a full-contrast disc under +-3 levels
    5  the tile hangs over a border or a corner of the frame.  Even ones: the frame lies at the FILL's level and a 2 x 2 block of
       the target's colour sits on a noise-free patch that the padding continues (four tied pixels, tests/layout_frames.py's
       "empty" recipe).  Odd ones: the frame lies far from the fill, a strong edge enters the tile, V = max|pixel - dc| is large
       and many pixels fall under T V / 255
The noise of families 0 and 1 is not any draw: with the window's own V = max|pixel - dc| the flag rule T V / 255 is met by
chance only, so search_attempts draws until the emulated FP32 map's two best responses lie within it, and
tests/golden/exact_scene_attempts.json records the number of the draw per window (`python tests/exact_scenes.py` rewrites it).
Families cycle over the windows (so every one is present from n = 6 on) in a seeded order.

A Set names one (FP32 order, l, window, n, content, sign, families) combination; used_sets() lists every Set the GPU file runs,
built by the same functions the GPU file calls.  evaluate(oracle, S) holds, once per process: the scene, the dense Float64
oracle's positions, and — on request, the CPU file's — what the float32 emulation of the Set's order (tests/fp32_restatement.py)
says about every window.  Test code only."""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_restatement as fr  # noqa: E402

JIT = 3
ALL = (0, 1, 2, 3, 4, 5)
CONTENTS = {"fill": (128, 128), "local dc": (40, 200)}      # content -> (level, fill)


def tw_for_kernel_len(l):
    for tw10 in range(20, 1400):
        if fr.kernel_len(fr.sigma_of(tw10 / 10)) == l:
            return tw10 / 10
    raise AssertionError(l)


def roll_variant(l):
    return 100 if l == 65 else 100 + l


def geometry(l, ws):
    """radii, (n1, n2), (fh, fw) and the centre of the interior guesses (1-based)."""
    r1, r2 = ws[0] // 2, ws[1] // 2
    n1, n2 = 2 * r1 + 1, 2 * r2 + 1
    hw = l // 2
    return (r1, r2), (n1, n2), (n1 + l - 1 + 2 * JIT, n2 + l - 1 + 2 * JIT), (r1 + hw + 1 + JIT, r2 + hw + 1 + JIT)


def _put(frame, ci, cj, val, mask):
    """mask with its centre pixel (h // 2, w // 2) on (ci, cj), 0-based; clipped at the frame."""
    h, w = mask.shape
    i0, j0 = ci - h // 2, cj - w // 2
    sub = frame[max(i0, 0):max(i0 + h, 0), max(j0, 0):max(j0 + w, 0)]
    m = mask[max(-i0, 0):max(-i0, 0) + sub.shape[0], max(-j0, 0):max(-j0, 0) + sub.shape[1]]
    sub[m] = val


def _noisy(rng, frame, amp):
    return (frame.astype(np.int16) + rng.integers(-amp, amp + 1, frame.shape)).clip(0, 255).astype(np.uint8)


class _Builder:
    """The windows of one scene, one at a time: window(b, attempt) -> (frame, guess).  Placement comes from a generator of the
    window's own; the NOISE of families 0 and 1 from one seeded by (window, attempt) — exact_scenes.search_attempts looks for
    the first attempt whose emulated FP32 map has its two best responses within threshold_f32(F) V / 255."""

    def __init__(self, l, ws, n, darker, level, fill, seed, families=ALL, min_sep=None):
        self.l, self.ws, self.n, self.darker, self.level, self.fill, self.min_sep = l, ws, n, darker, level, fill, min_sep
        self.key = [seed, l, ws[0], ws[1], n, int(darker), level, fill]
        self.rad = max(2, int(tw_for_kernel_len(l)) // 2)
        rng = np.random.Generator(np.random.PCG64(self.key))
        fam = np.array([families[k % len(families)] for k in range(n)])
        rng.shuffle(fam)
        self.fam = fam
        self.rank = np.array([int((fam[:b] == fam[b]).sum()) for b in range(n)])      # k: the window's number within its family

    def searched(self, b):
        """Windows whose noise is chosen by search_attempts: family 0, and family 1's noisy half."""
        return self.fam[b] == 0 or (self.fam[b] == 1 and self.rank[b] % 2 == 1)

    def window(self, b, attempt=0):
        l, darker, level, fill, rad = self.l, self.darker, self.level, self.fill, self.rad
        (r1, r2), (n1, n2), (fh, fw), (c1, c2) = geometry(l, self.ws)
        hw = l // 2
        rng = np.random.Generator(np.random.PCG64(self.key + [b]))
        nrng = np.random.Generator(np.random.PCG64(self.key + [b, attempt]))
        yy, xx = np.mgrid[-rad:rad + 1, -rad:rad + 1]
        disc = (yy * yy + xx * xx) <= rad * rad
        ye, xe = np.mgrid[0:2 * rad, 0:2 * rad] - rad + 0.5
        even_disc = (ye * ye + xe * xe) <= rad * rad             # its centre falls between pixels: four tied pixels
        sgn = -1 if darker else 1

        def tv(base, depth):
            return int(np.clip(base + sgn * depth, 0, 255))

        def inside(r, shrink):
            return int(rng.integers(-max(r - shrink, 0), max(r - shrink, 0) + 1))
        D = min(128, level if darker else 255 - level)           # full contrast against `level`
        rem = n2 % 64 if n2 > 64 and 0 < n2 % 64 <= 6 else 0      # remainder columns beyond whole strips (thin / folded)
        f, k = int(self.fam[b]), int(self.rank[b])
        gi, gj = c1 + int(rng.integers(-JIT, JIT + 1)), c2 + int(rng.integers(-JIT, JIT + 1))    # interior: the whole tile inside the frame
        F = np.full((fh, fw), level, np.uint8)
        if f == 0:
            F = _noisy(nrng, F, int(rng.integers(1, 4)))
        elif f == 1:
            _put(F, gi - 1 + inside(r1, 2), gj - 1 + inside(r2, 2), tv(level, 1), even_disc)
            if k % 2:
                F = _noisy(nrng, F, 1)
        elif f == 2:
            lo1, lo2 = (min(self.min_sep[0], r1 - 1), min(self.min_sep[1], r2 - 1)) if self.min_sep else (0, 0)
            while True:
                di = int(rng.integers(lo1, r1))
                if rem and k % 4 == 3:
                    dj = r2 - int(rng.integers(0, rem))           # the second disc's centre in a remainder column
                elif n2 >= 128:                                    # even k: the discs in different 64-column strips; odd k: in one
                    dj = int(rng.choice([d for d in range(r2) if ((r2 - d) // 64 != (r2 + d) // 64) == (k % 2 == 0)]))
                else:
                    dj = int(rng.integers(lo2, r2)) * (1 if self.min_sep or rng.integers(0, 2) else -1)
                if max(di, abs(dj)) >= min(3, max(r1, r2) - 1):
                    break
            _put(F, gi - 1 - di, gj - 1 - dj, tv(level, D), disc)
            _put(F, gi - 1 + di, gj - 1 + dj, tv(level, D - int(rng.integers(0, 2))), disc)
            if (k // 2) % 2:
                F = _noisy(nrng, F, 1)
        elif f == 3:
            side = 2 * int(rng.integers(max(2, rad // 3), rad + 1))
            mask = np.ones((side + (k % 2), side), bool)          # odd rows: 2 tied pixels; even: 4
            _put(F, gi - 1 + inside(r1, 2), gj - 1 + inside(r2, 2), tv(level, int(rng.integers(min(28, D), D + 1))), mask)
        elif f == 4:
            _put(F, gi - 1 + inside(r1, 2), gj - 1 + inside(r2, 2), tv(level, D), disc)
            F = _noisy(nrng, F, 3)
        else:
            assert f == 5, f
            side = (k // 2) % 8                                    # four corners, then four borders
            top, bottom = (1, min(r1 + hw // 2, fh)), (max(fh - r1 - hw // 2 + 1, 1), fh)
            left, right = (1, min(r2 + hw // 2, fw)), (max(fw - r2 - hw // 2 + 1, 1), fw)
            ri = (top, top, bottom, bottom, top, bottom, None, None)[side]
            rj = (left, right, left, right, None, None, left, right)[side]
            if ri is not None:
                gi = int(rng.integers(ri[0], ri[1] + 1))
            if rj is not None:
                gj = int(rng.integers(rj[0], rj[1] + 1))
            if k % 2 == 0:      # the frame at the fill's level: the padding continues a noise-free patch around a 2 x 2 block
                F = _noisy(nrng, np.full((fh, fw), fill, np.uint8), 2)
                bi = int(np.clip(gi - 1 + inside(min(r1, 4), 1), 0, fh - 2))
                bj = int(np.clip(gj - 1 + inside(min(r2, 4), 1), 0, fw - 2))
                p = hw + 2
                F[max(bi - p, 0):bi + 2 + p, max(bj - p, 0):bj + 2 + p] = fill
                F[bi:bi + 2, bj:bj + 2] = tv(fill, min(128, fill if darker else 255 - fill))
            else:               # the frame far from the fill: a strong edge enters the tile
                lv = level if abs(level - fill) >= 64 else (fill + 100 if fill + 100 <= 250 else fill - 100)
                F = _noisy(nrng, np.full((fh, fw), lv, np.uint8), 2)
        return F, (gi, gj)


def hard_windows(l, ws, n, darker, level, fill, seed, families=ALL, min_sep=None, attempts=None):
    """frames u8 [n, fh, fw], 1-based guesses int32 [n, 2], family ids [n].  attempts: None, or per window the number of the
    noise draw (tests/golden/exact_scene_attempts.json holds them per Set)."""
    B = _Builder(l, ws, n, darker, level, fill, seed, families, min_sep)
    wins = [B.window(b, 0 if attempts is None else int(attempts[b])) for b in range(n)]
    return np.stack([f for f, _ in wins]), np.array([g for _, g in wins], np.int32), B.fam


# ---- the sets ----
Set = collections.namedtuple("Set", "order l ws n content darker families min_sep own_fill")

# Set -> a scene seed other than 0, should a set ever miss tests/test_exact_scenes_cpu.py's shares (none does)
SEEDS = {}


def make_set(order, l, ws, n, content="fill", darker=True, families=ALL, min_sep=None, own_fill=False):
    return Set(order, l, tuple(ws), n, content, bool(darker), tuple(families), min_sep, own_fill)


def label(S):
    return (f"{S.order} l={S.l} {S.ws[0]}x{S.ws[1]} n={S.n} {S.content} {'dark' if S.darker else 'bright'}"
            + ("" if S.families == ALL else f" families={','.join(map(str, S.families))}") + (" own-fill" if S.own_fill else ""))


ROLL_LENGTHS = (17, 29, 49, 65, 81, 101, 125, 149)
ROLL_BRIGHT = (17, 65, 101, 149)
ROLL_NO_PRUNE = (17, 65, 109)
CHAIN_LENGTHS = (17, 65, 101, 149)
P, X = (21, 45), (21, 131)
RING = ((0, 65), (1, 65), (2, 65), (10, 65), (13, 65), (20, 29))
FUSED_LENGTHS = (29, 45, 65, 85, 101)
FUSED_BRIGHT = (29, 101)
FUSED_WS = (23, 37)
TILED_LENGTHS = (29, 65, 101)
TILED_WS = (96, 81)
TWOPASS = ([(29, (45, 45)), (65, (45, 45))] + [(l, ws) for l in (101, 113, 125) for ws in ((33, 41), (61, 75))] + [(293, (21, 21))])
FUNCTOR_LENGTHS = (29, 101)


def roll_set(l, ws, content="fill", darker=True, n=None):
    if n is None:
        n = 64 if ws[1] < 128 or l <= 65 else 24
    return make_set("roll", l, ws, n, content, darker)


def roll_chain_set(l):
    return make_set("roll", l, X, 48, families=(0,))          # 8 clips x 6 frames


def ring_set(l):
    return make_set("ring", l, (45, 45), 96)


def fused_set(l, content="fill", darker=True):
    return make_set("fused", l, FUSED_WS, 48, content, darker)


def fused_chain_set(l):
    return make_set("fused", l, FUSED_WS, 24, families=(0,))


def tiled_set(l):
    return make_set("tiled", l, TILED_WS, 14, min_sep=(12, 12))


def tiled_chain_set(l):
    return make_set("tiled", l, TILED_WS, 8, families=(0,))


def twopass_set(l, ws):
    return make_set("twopass", l, ws, 40)


def functor_set(l, window):
    return make_set("fused", l, (window, window), 6, families=(0, 1), own_fill=True)


def used_sets(oracle):
    """Every Set tests/test_gpu_exact_lengths.py runs (the functor's default window is the oracle's, src/PawsomeTracker.jl:64-68)."""
    out = []
    for l in ROLL_LENGTHS:
        out += [roll_set(l, P), roll_set(l, P, "local dc"), roll_set(l, X)]
    out += [roll_set(l, P, darker=False) for l in ROLL_BRIGHT]
    out += [roll_set(l, P) for l in ROLL_NO_PRUNE]
    out += [roll_set(65, (21, 65)), roll_set(65, (21, 513), n=8)]
    out += [roll_chain_set(l) for l in CHAIN_LENGTHS]
    out += [ring_set(l) for l in sorted({l for _, l in RING})]
    for l in FUSED_LENGTHS:
        out += [fused_set(l), fused_chain_set(l)]
    out += [fused_set(l, darker=False) for l in FUSED_BRIGHT] + [fused_set(65, "local dc")]
    for l in TILED_LENGTHS:
        out += [tiled_set(l), tiled_chain_set(l)]
    out += [twopass_set(l, ws) for l, ws in TWOPASS]
    out += [functor_set(l, oracle.default_window(tw_for_kernel_len(l))) for l in FUNCTOR_LENGTHS]
    return list(dict.fromkeys(out))


# ---- the table ----
ATTEMPTS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exact_scene_attempts.json")
_ATTEMPTS = None
_SCENES = {}
_EMULATED = {}


def attempts_of(S):
    """Per window the noise draw search_attempts chose for this Set (None: none recorded, every window takes draw 0)."""
    global _ATTEMPTS
    if _ATTEMPTS is None:
        import json
        _ATTEMPTS = json.load(open(ATTEMPTS_FILE)) if os.path.exists(ATTEMPTS_FILE) else {}
    return _ATTEMPTS.get(label(S))


class _Emulation:
    """The float32 emulation of a Set's order on one window: (argmax as a 1-based position, first in column-major order;
    best - second best, the second best the largest response of any OTHER pixel; threshold_f32(F) V / 255; V; dc)."""

    def __init__(self, S):
        self.S = S
        self.tw = tw_for_kernel_len(S.l)
        self.radii, (self.n1, self.n2) = geometry(S.l, S.ws)[:2]
        gp, gm, _, _ = fr.tap_tables(self.tw, S.darker)
        self.o = fr.order(S.order, S.l, n1=self.n1, n2=self.n2)
        self.T = float(fr.threshold_f32(fr.factor(self.o, gp, gm)))

    def float64_position(self, frame, fill, guess):
        """(argmax, best - second best, threshold_f32(F) V / 255) of the separable Float64 response (numpy; the search's stand-in
        for the dense oracle, which the CPU test asks)."""
        S, (r1, r2) = self.S, self.radii
        if not hasattr(self, "_toeplitz"):
            gp, gm, _, _ = fr.tap_tables(self.tw, S.darker)
            def toep(g, n):
                M = np.zeros((n, n + S.l - 1))
                for y in range(n):
                    M[y, y:y + S.l] = g
                return M
            self._toeplitz = [(toep(g, self.n1), toep(g, self.n2)) for g in (gp, gm)]
        tile = fr.window_tile(frame, int(fill), S.l, (r1, r2), guess)
        v = tile.astype(np.float64) - fr.dc_level(tile, int(fill))
        (Ap, Bp), (Am, Bm) = self._toeplitz
        flat = ((Ap @ v @ Bp.T - Am @ v @ Bm.T) * ((-1.0 if S.darker else 1.0) / 255.0)).T.ravel()
        a = int(np.argmax(flat))
        best = flat[a]
        flat[a] = -np.inf
        return (int(guess[0]) - r1 + a % self.n1, int(guess[1]) - r2 + a // self.n1), best - flat.max(), self.T * np.abs(v).max() / 255.0

    def __call__(self, frame, fill, guess):
        S, (r1, r2) = self.S, self.radii
        tile = fr.window_tile(frame, int(fill), S.l, (r1, r2), guess)
        dc = fr.dc_level(tile, int(fill))
        flat = fr.response_of_order(tile, int(fill), self.tw, S.darker, self.o, dc=dc).T.ravel()      # column-major
        a = int(np.argmax(flat))                                 # (the first of equal maxima)
        best = float(flat[a])
        flat[a] = -np.inf
        vmax = int(np.abs(tile.astype(np.int32) - dc).max())
        return (int(guess[0]) - r1 + a % self.n1, int(guess[1]) - r2 + a // self.n1), best - float(flat.max()), self.T * vmax / 255.0, vmax, dc


def search_attempts(oracle, S, cap=50000000):
    """Per window of families 0 and 1 (noisy half) the first noise draw whose emulated FP32 map has its two best responses
    within threshold_f32(F) V / 255 — the windows that only the Float64 arithmetic can decide.  In a Set of noise alone (the
    chains') the first window's draw must also make the emulated FP32 argmax differ from a Float64 ranking: the actual FP32
    error is a small share of its bound, and without this no window of such a Set would be decided wrongly by FP32 alone.
    A condition on the inputs: nothing of the library runs.  `python tests/exact_scenes.py` records the draws of every used Set."""
    level, fill = CONTENTS[S.content]
    B = _Builder(S.l, S.ws, S.n, S.darker, level, fill, SEEDS.get(S, 0), S.families, S.min_sep)
    E = _Emulation(S)
    out = []
    for b in range(S.n):
        a = 0
        while B.searched(b):
            frame, g = B.window(b, a)
            v = oracle.mode_u8(frame) if S.own_fill else fill
            differ = b == 0 and S.families == (0,)
            if differ:      # (FP32 can only misrank where the Float64 gap is a fraction of the bound: the cheap look first)
                pos64, gap64, bound64 = E.float64_position(frame, v, g)
            if not differ or gap64 <= 0.25 * bound64:
                pos, gap, bound, _, _ = E(frame, v, g)
                if gap <= bound and not (differ and pos == pos64):
                    break
            a += 1
            assert a < cap, (label(S), b)
        out.append(a)
    return out


def evaluate(oracle, S, emulate=False):
    """dict(frames, guesses, fam, fills, tw, radii, dense) of the Set's scene — with `emulate` also, per window: emu, gap,
    bound, V and dc as _Emulation gives them, and T."""
    if S not in _SCENES:
        level, fill = CONTENTS[S.content]
        seed = SEEDS.get(S, 0)
        frames, guesses, fam = hard_windows(S.l, S.ws, S.n, S.darker, level, fill, seed, S.families, S.min_sep, attempts_of(S))
        tw = tw_for_kernel_len(S.l)
        sg = oracle.sigma(tw)
        assert oracle.kernel_len(sg) == S.l
        K = oracle.dog_kernel(sg, S.darker)
        radii = geometry(S.l, S.ws)[0]
        if S.own_fill:            # the host functor's fill: the mode of its frame
            fills = np.array([oracle.mode_u8(f) for f in frames])
            dense = np.array([oracle.detect(f, int(v), K, radii, (int(g[0]), int(g[1]))) for f, v, g in zip(frames, fills, guesses)], np.int32)
        else:
            fills = np.full(S.n, fill)
            dense = oracle.detect_batch_par(frames, fill, K, sg, S.darker, radii, guesses, separable=False)
        _SCENES[S] = dict(frames=frames, guesses=guesses, fam=fam, fills=fills, tw=tw, radii=radii, dense=dense, K=K, seed=seed)
    sc = _SCENES[S]
    if emulate and S not in _EMULATED:
        E = _Emulation(S)
        rows = [E(f, v, g) for f, v, g in zip(sc["frames"], sc["fills"], sc["guesses"])]
        _EMULATED[S] = dict(emu=np.array([r[0] for r in rows], np.int32), gap=np.array([r[1] for r in rows]), bound=np.array([r[2] for r in rows]),
                            V=np.array([r[3] for r in rows]), dc=np.array([r[4] for r in rows]), T=E.T)
    return dict(sc, **_EMULATED[S]) if emulate else sc


def oracle_chain(oracle, S, clip, nf, start):
    """The serial chain over frames clip * nf ... of the Set's scene from `start`, by the dense oracle: memoised."""
    sc = evaluate(oracle, S)
    memo = sc.setdefault("chains", {})
    key = (clip, nf, int(start[0]), int(start[1]))
    if key not in memo:
        g, out = (int(start[0]), int(start[1])), []
        for f in sc["frames"][clip * nf:(clip + 1) * nf]:
            g = tuple(oracle.detect(f, CONTENTS[S.content][1], sc["K"], sc["radii"], g))
            out.append(g)
        memo[key] = np.array(out, np.int32)
    return memo[key]


def _search_one(S):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle.dog_oracle import Oracle
    return label(S), search_attempts(Oracle(), S)


if __name__ == "__main__":      # record the noise draws of every used Set, or of those whose label holds argv[1] (minutes on eight cores; run it with OMP_NUM_THREADS=1: the products are small)
    import json
    import multiprocessing
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle.dog_oracle import Oracle
    sets = [S for S in used_sets(Oracle()) if len(sys.argv) < 2 or sys.argv[1] in label(S)]
    sets.sort(key=lambda S: S.n * S.ws[1] / S.l ** 2, reverse=True)      # the long searches first
    table = json.load(open(ATTEMPTS_FILE)) if len(sys.argv) > 1 and os.path.exists(ATTEMPTS_FILE) else {}
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        for name, draws in pool.imap_unordered(_search_one, sets):
            table[name] = draws
            print(name, max(draws), flush=True)
            with open(ATTEMPTS_FILE, "w") as f:      # (rewritten as the results arrive: a search may run long)
                f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(table[k], separators=(',', ':'))}" for k in sorted(table)) + "\n}\n")
