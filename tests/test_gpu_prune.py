"""Kept ranges on the roll batch path (csrc/dog_prune.hpp): a pre-pass bounds, per window, which 8-row blocks of which strips
can hold the peak or a near-tie, and the roll / thin kernels compute only those.  Nothing the caller sees may move.

Every case runs one batch of 64 windows (a frame of 300 × 400 each) on the pinned roll instance twice, pruning on and
`no_prune`, exact mode on, and compares
  * the positions, exactly, with each other and with the dense Float64 oracle;
  * the windows' merged FP32 maxima, bit for bit (BatchTracker.batch_maxima);
  * the number of windows exact mode re-evaluated.
Shapes: windows 129 × 129 (two strips and a remainder column) and 65 × 65 (one strip and a remainder column); l = 17 and 65
(three waves per SIMD) and, on the 129 × 129 windows, l = 109 (two).  Scenes of the disc batch: a disc in the interior, across
the strip boundary, in the window's first and last rows, hanging over the frame's edge (padding skip inside a range), two
identical discs far apart (a tie: the first in column-major order wins), a second disc a little fainter, a bright disc beside
the target, a window whose level sits off the fill.  The quiet batch holds flat windows and noise only.
Against a vacuous pass: the kept share (BatchTracker.prune_counts) must be below 1 for the disc batch and exactly 1 for the
quiet batch — a property of the inputs (tests/test_prune_cpu.py: a clean disc prunes, a window without one does not) — and
the kernel's (kept, total) counts must EQUAL the ones tests/prune_restatement.py derives from the same windows.  Each scene
also runs as a batch of its own eight windows: the restatement must find there the mechanism the scene was built for (a hull
inside the window, at its first rows, at its last rows, a skipped slot, padding-only sub-chunks inside a kept range, two
slots kept across the strip boundary, a level off the fill), and the kernel's counts must equal the restatement's per scene."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_restatement as fr  # noqa: E402
import prune_restatement as pr  # noqa: E402

pytestmark = pytest.mark.gpu

FILL, FH, FW, N = 128, 300, 400, 64
CONFIGS = [(117, 17, 129), (117, 17, 65), (100, 65, 129), (100, 65, 65), (209, 109, 129)]   # (variant id, l, window edge)


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    return m


def _tw_for_kernel_len(l):
    for tw10 in range(20, 1400):
        if fr.kernel_len(fr.sigma_of(tw10 / 10)) == l:
            return tw10 / 10
    raise AssertionError(l)


def _disc(f, centre, rad, value):
    """centre 1-based (row, col); clipped at the frame."""
    ii, jj = np.ogrid[:f.shape[0], :f.shape[1]]
    f[(ii - (centre[0] - 1)) ** 2 + (jj - (centre[1] - 1)) ** 2 <= rad * rad] = value


def _disc_batch(l, n):
    """64 frames and guesses: eight scenes, eight placements each."""
    tw = _tw_for_kernel_len(l)
    rad, r, hw = max(2, int(tw) // 2), n // 2, l // 2
    rng = np.random.default_rng([l, n])
    far = min(r - rad - 2, 36)      # offset of the paired discs from the guess, per axis: apart, and inside the window
    assert 2 * far > 2 * rad + 2 and far + rad < r, (l, n, far)
    frames, guesses = [], []
    for k in range(N):
        scene, v = k % 8, k // 8
        f = np.full((FH, FW), FILL, np.uint8)
        g = (150 + 3 * v, 200 - 5 * v)
        noise = 2
        if scene == 0:                                    # interior
            _disc(f, (g[0] + 5 - v, g[1] - 7 + 2 * v), rad, 0)
        elif scene == 1:                                  # across the boundary between strip 0 and what follows it (window column 64)
            _disc(f, (g[0] + 2 * v - 6, g[1] - r + 64 + (v % 3) - 1), rad, 0)
        elif scene == 2:                                  # the window's first rows / last rows
            _disc(f, (g[0] - r + 1 + v % 4 if v < 4 else g[0] + r - 1 - v % 4, g[1] + 3 * v - 9), rad, 0)
        elif scene == 3:                                  # over the frame's edge: top, bottom, left, right
            g = [(2 + v, 180), (FH - 1 - v, 220), (140, 3 + v), (160, FW - 2 - v)][v % 4]
            c = [(1, 184), (FH, 214), (143, 1), (156, FW)][v % 4]
            _disc(f, c, rad, 0)
        elif scene == 4:                                  # two identical discs far apart, mirror images about the guess: a tie
                                                          # (exact where the kernel reaches neither from the other, a near-tie else)
            _disc(f, (g[0] - far, g[1] - far), rad, 0)
            _disc(f, (g[0] + far, g[1] + far), rad, 0)
            noise = 0
        elif scene == 5:                                  # a second disc a little fainter
            _disc(f, (g[0] - far, g[1] + far), rad, 0)
            _disc(f, (g[0] + far, g[1] - far), rad, 2 + v)
            noise = 0 if v % 2 else 1
        elif scene == 6:                                  # a bright disc beside the dark target
            _disc(f, (g[0] + far, g[1] + far - v), rad, 255)
            _disc(f, (g[0] - far + v, g[1] - far), rad, 0)
        else:                                             # the window's level sits off the fill
            f[...] = 60 + 4 * v
            _disc(f, (g[0] - 4 + v, g[1] + 6), rad, 0)
            if v >= 6:                                    # … and hangs over the top edge: padding that is not zero
                g = (4 + v, g[1])
                _disc(f, (9, g[1] + 6), rad, 0)
        if noise:
            f = np.clip(f.astype(np.int16) + rng.integers(-noise, noise + 1, f.shape), 0, 255).astype(np.uint8)
        frames.append(f)
        guesses.append(g)
    return np.stack(frames), np.array(guesses, np.int32)


def _quiet_batch(l, n):
    """Flat windows (at the fill, some over the frame's edges, and off it) and noise only (± 1 and ± 3 levels).  The noise
    windows and the ones off the fill lie inside the frame: padding beside them is a region of its own (an edge, or blocks
    of exact zeros under noise) and may rightly be pruned."""
    rng = np.random.default_rng([l, n, 1])
    frames, guesses = [], []
    for k in range(N):
        kind, v = k % 4, k // 4
        f = np.full((FH, FW), FILL if kind != 1 else 70, np.uint8)
        if kind >= 2:
            a = 1 if kind == 2 else 3
            f = (f.astype(np.int16) + rng.integers(-a, a + 1, f.shape)).astype(np.uint8)
        frames.append(f)
        inside = (150 - 20 + 3 * v, 200 + 20 - 2 * v)
        guesses.append(inside if kind else [inside, (5 + v, 30 + 20 * v), (FH - v, 390 - 3 * v), (100 + 10 * v, 2)][v % 4])
    return np.stack(frames), np.array(guesses, np.int32)


_CACHE = {}
SCENES = ("interior", "strip boundary", "first / last rows", "over the frame's edge", "two equal discs", "fainter second disc",
          "bright disc beside", "level off the fill")


def _mechanisms(frames, guesses, l, n):
    """What the restatement (tests/prune_restatement.py) says the pre-pass does with these windows: (kept, total) pairs and
    which mechanisms of the kept ranges they exercise."""
    tw, hw, r = _tw_for_kernel_len(l), l // 2, n // 2
    kept = total = 0
    mech = set()
    several = True
    for f, g in zip(frames, guesses):
        tile = fr.window_tile(f, FILL, l, (r, r), g)
        pp = pr.prepass(tile, FILL, tw, True)
        k, t = pr.kept_pairs(pp, l)
        kept, total = kept + k, total + t
        ti0 = int(g[0]) - r - 1 - hw
        for (ba, bb) in pp["hull"]:
            if bb == ba:
                mech.add("slot skipped")
                continue
            if 0 < ba and bb < pp["nblk"]:
                mech.add("hull inside")
            if ba == 0 and bb < pp["nblk"]:
                mech.add("hull at the first rows")
            if ba > 0 and bb == pp["nblk"]:
                mech.add("hull at the last rows")
            sc_hi = min(pp["nsub"], bb + pr.tail(l))
            if pp["dc"] == FILL and (ba, sc_hi) != (0, pp["nsub"]) and any(ti0 + 8 * sc + 7 < 0 or ti0 + 8 * sc >= FH for sc in range(ba, sc_hi)):
                mech.add("padding skip inside a range")
        if pp["dc"] != FILL:
            mech.add("dc off the fill")
        several = several and sum(bb > ba for ba, bb in pp["hull"]) >= 2
    if several:
        mech.add("two slots kept in every window")
    return kept, total, mech


# what each scene is there for, as the restatement must find it in every configuration (a property of the inputs, checked
# before the kernel's counts are held to the restatement's); scene 4, the tie, is held by positions and counts alone
SCENE_MECHANISMS = (
    {"hull inside", "slot skipped"},
    {"two slots kept in every window"},
    {"hull at the first rows", "hull at the last rows"},
    {"padding skip inside a range"},
    set(),
    set(),
    set(),
    {"dc off the fill"},
)


def _case(oracle, kind, l, n):
    """Frames, guesses and the oracle's positions of one batch: built once, shared by the tests that use it."""
    key = (kind, l, n)
    if key not in _CACHE:
        frames, guesses = (_disc_batch if kind == "disc" else _quiet_batch)(l, n)
        K = oracle.dog_kernel(oracle.sigma(_tw_for_kernel_len(l)), True)
        ref = oracle.detect_batch(frames, FILL, K, (n // 2, n // 2), guesses)
        _CACHE[key] = (frames, guesses, ref)
    return _CACHE[key]


def _run(pt, frames, guesses, vid, l, n, no_prune, want_resp=False, batch=N):
    import torch
    bt = pt.BatchTracker(FH, FW, _tw_for_kernel_len(l), (n, n), True, FILL)
    try:
        assert bt.info().kernel_len == l
        bt.set_variant(vid)
        bt.set_tuning("no_prune", no_prune)
        bt.set_exact(1)
        assert bt.kernel_for_batch(batch) == vid
        d_f, d_g = torch.from_numpy(frames).cuda(), torch.from_numpy(guesses).cuda()
        if want_resp:
            pos, resp = bt.detect(d_f, d_g, want_resp=True)
            bt.sync()
            return pos.cpu().numpy(), resp.cpu().numpy(), bt.prune_counts()
        pos = bt.detect(d_f, d_g)
        bt.sync()
        return pos.cpu().numpy(), bt.batch_maxima(batch), bt.exact_stats()[2], bt.prune_counts()
    finally:
        bt.close()


def _compare(pt, oracle, kind, vid, l, n):
    frames, guesses, ref = _case(oracle, kind, l, n)
    pos_p, max_p, ref_p, (kept, total) = _run(pt, frames, guesses, vid, l, n, 0)
    pos_d, max_d, ref_d, dense_counts = _run(pt, frames, guesses, vid, l, n, 1)
    print(f"prune {kind} l={l} window={n}: kept {kept} of {total} (slot, sub-chunk) pairs; windows refined {ref_p} / {ref_d}")
    assert dense_counts == (0, 0)                        # `no_prune` ran no pre-pass
    assert total > 0                                     # … and the default did
    assert np.array_equal(pos_p, pos_d), np.argwhere(pos_p != pos_d)[:4]
    assert np.array_equal(pos_p, ref), np.argwhere(pos_p != ref)[:4]
    assert np.array_equal(max_p.view(np.int32), max_d.view(np.int32)), np.argwhere(max_p != max_d)[:4]
    assert ref_p == ref_d
    return kept, total


@pytest.mark.parametrize("vid,l,n", CONFIGS)
def test_disc_scenes_prune_and_nothing_moves(pt, oracle, vid, l, n):
    kept, total = _compare(pt, oracle, "disc", vid, l, n)
    assert kept < total
    frames, guesses, ref = _case(oracle, "disc", l, n)
    assert (kept, total) == _mechanisms(frames, guesses, l, n)[:2]       # the kernel's counts are the restatement's


@pytest.mark.parametrize("vid,l,n", CONFIGS)
def test_each_scene_exercises_its_mechanism(pt, oracle, vid, l, n):
    """The eight windows of each scene as a batch of their own: the restatement finds the mechanism the scene was built for
    (SCENE_MECHANISMS), and the kernel keeps exactly the (slot, sub-chunk) pairs the restatement keeps — L, energies, hull and
    counts all enter that number — with the oracle's positions."""
    frames, guesses, ref = _case(oracle, "disc", l, n)
    for scene, name in enumerate(SCENES):
        idx = [k for k in range(N) if k % 8 == scene]
        kept, total, mech = _mechanisms(frames[idx], guesses[idx], l, n)
        assert SCENE_MECHANISMS[scene] <= mech, (name, sorted(mech))
        if scene != 4:
            assert kept < total, name
        pos, _, _, counts = _run(pt, np.ascontiguousarray(frames[idx]), np.ascontiguousarray(guesses[idx]), vid, l, n, 0, batch=len(idx))
        print(f"prune scene l={l} window={n} {name}: kept {counts[0]} of {counts[1]}; {sorted(mech)}")
        assert counts == (kept, total), (name, counts, (kept, total))
        assert np.array_equal(pos, ref[idx]), name


@pytest.mark.parametrize("vid,l,n", CONFIGS)
def test_flat_and_noise_only_keep_everything(pt, oracle, vid, l, n):
    kept, total = _compare(pt, oracle, "quiet", vid, l, n)
    assert kept == total
    frames, guesses, _ = _case(oracle, "quiet", l, n)
    assert (kept, total) == _mechanisms(frames, guesses, l, n)[:2]


def test_a_launch_that_asks_for_the_map_stays_dense(pt, oracle):
    vid, l, n = 100, 65, 129
    frames, guesses, ref = _case(oracle, "disc", l, n)
    pos_p, resp_p, counts = _run(pt, frames, guesses, vid, l, n, 0, want_resp=True)
    pos_d, resp_d, _ = _run(pt, frames, guesses, vid, l, n, 1, want_resp=True)
    assert counts == (0, 0)
    assert np.array_equal(resp_p.view(np.int32), resp_d.view(np.int32))
    assert np.array_equal(pos_p, pos_d) and np.array_equal(pos_p, ref)
