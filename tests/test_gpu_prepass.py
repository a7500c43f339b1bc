"""The roll batch path's pre-pass (csrc/dog_prune.hpp) on window shapes whose slots do not fall on dword boundaries, and on
tiles that hang over the frame.  The pre-pass forms its energies from raw-pixel moments per column segment; a dword that
straddles a cut between two segments takes a byte-masked path, and a dword that hangs over the frame's edge is read byte by
byte.  These shapes and scenes reach both, and the window's level decides whether a masked-out byte could be mistaken for a
pixel (bright windows, V = 255).

Window shapes (h, w) and what their slots are (tests/prune_restatement.py, slots; held to the literal layout below):
  (129, 197)  three aligned strips and five remainder columns at 192 … 196
  (65, 101)   strips at 0 and 37
  (65, 131)   two strips and remainder columns at 128, 129, 130
  (45, 45)    one partial strip
Kernel lengths: l = 65 on every shape, l = 17 on (45, 45), l = 109 on (129, 197); and once the headline's own geometry,
257 × 257 at l = 65, with 8 windows.  Scenes, three windows each (two for the headline): a disc in the interior; a disc with
the guess in the bottom-right corner of the LAST frame of the stack (the tile hangs over both edges and over the last row of
the last frame); a bright level (200, disc 140: no pixel is 0 and the level lies off the fill); level 255 with a disc of 0
(the disc's pixels set V = dc; the sampled level comes out a few levels under 255, the disc pulls it).

Per batch, pruning on against `no_prune`, exact mode on, the roll variant pinned: positions equal the oracle's and the dense
run's, the merged FP32 maxima match bit for bit, the refined counts are equal.  Per window, each as a batch of its own on a
fresh tracker (the policy sleeps after a window that keeps everything): the kernel's (kept, total) equals the restatement's
— dc, V, the cell choice, L, the threshold and every hull enter that number."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_restatement as fr  # noqa: E402
import prune_restatement as pr  # noqa: E402

FILL, FH, FW = 128, 300, 400
SHAPES = {
    (129, 197): [(0, 64), (64, 64), (128, 64)] + [(192 + k, 1) for k in range(5)],
    (65, 101): [(0, 64), (37, 64)],
    (65, 131): [(0, 64), (64, 64), (128, 1), (129, 1), (130, 1)],
    (45, 45): [(0, 45)],
    (257, 257): [(0, 64), (64, 64), (128, 64), (192, 64), (256, 1)],
}
# (variant id, l, (h, w), windows per scene)
CONFIGS = [(100, 65, (129, 197), 3), (100, 65, (65, 101), 3), (100, 65, (65, 131), 3), (100, 65, (45, 45), 3),
           (117, 17, (45, 45), 3), (209, 109, (129, 197), 3), (100, 65, (257, 257), 2)]
SCENES = ("interior", "bright level", "level 255", "corner of the last frame")   # (the corner scene last: its frames end the stack)


def test_slot_layouts():
    for (h, w), want in SHAPES.items():
        assert pr.slots(w) == want, (w, pr.slots(w))


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


def _batch(l, shape, per_scene):
    """Frames and guesses, window k of scene k mod 4; the last frame of the stack belongs to the corner scene."""
    tw = _tw_for_kernel_len(l)
    rad = max(2, int(tw) // 2)
    rng = np.random.default_rng([l, shape[0], shape[1]])
    frames, guesses = [], []
    for k in range(4 * per_scene):
        scene, v = k % 4, k // 4
        g = (150 + 3 * v, 200 - 5 * v)
        if scene == 0:                                        # a disc in the interior
            f = np.full((FH, FW), FILL, np.uint8)
            _disc(f, (g[0] + 5 - 2 * v, g[1] - 7 + 3 * v), rad, 0)
            noise = 2
        elif scene == 1:                                      # a bright level off the fill, no pixel 0
            f = np.full((FH, FW), 200, np.uint8)
            _disc(f, (g[0] - 4 + v, g[1] + 6), rad, 140)
            noise = 2
        elif scene == 2:                                      # level 255, a disc of 0 inside the frame: V = 255
            f = np.full((FH, FW), 255, np.uint8)
            _disc(f, (g[0] + 3, g[1] - 5 + 2 * v), rad, 0)
            noise = 0
        else:                                                 # the guess in the frame's bottom-right corner
            f = np.full((FH, FW), FILL, np.uint8)
            g = (FH - 1 - v, FW - 2 - 2 * v)
            _disc(f, (FH - 3 - rad - v, FW - 4 - rad - v), rad, 0)
            noise = 2
        if noise:
            f = np.clip(f.astype(np.int16) + rng.integers(-noise, noise + 1, f.shape), 0, 255).astype(np.uint8)
        frames.append(f)
        guesses.append(g)
    frames = np.stack(frames)
    assert frames[1::4].min() > 0
    return frames, np.array(guesses, np.int32)


_CACHE = {}


def _case(oracle, l, shape, per_scene):
    """Frames, guesses, the oracle's positions and the restatement's pre-pass per window: built once, left unchanged."""
    key = (l, shape)
    if key not in _CACHE:
        frames, guesses = _batch(l, shape, per_scene)
        tw, radii = _tw_for_kernel_len(l), (shape[0] // 2, shape[1] // 2)
        K = oracle.dog_kernel(oracle.sigma(tw), True)
        ref = oracle.detect_batch(frames, FILL, K, radii, guesses)
        pps = [pr.prepass(fr.window_tile(f, FILL, l, radii, g), FILL, tw, True) for f, g in zip(frames, guesses)]
        _CACHE[key] = (frames, guesses, ref, pps)
    return _CACHE[key]


def _tracker(pt, vid, l, shape, no_prune, batch):
    bt = pt.BatchTracker(FH, FW, _tw_for_kernel_len(l), shape, True, FILL)
    try:
        assert bt.info().kernel_len == l
        bt.set_variant(vid)
        bt.set_tuning("no_prune", no_prune)
        bt.set_exact(1)
        assert bt.kernel_for_batch(batch) == vid
    except BaseException:
        bt.close()
        raise
    return bt


def _run(pt, d_f, d_g, vid, l, shape, no_prune):
    n = d_g.shape[0]
    bt = _tracker(pt, vid, l, shape, no_prune, n)
    try:
        pos = bt.detect(d_f, d_g)
        bt.sync()
        return pos.cpu().numpy(), bt.batch_maxima(n), bt.exact_stats()[2], bt.prune_counts()
    finally:
        bt.close()


@pytest.mark.gpu
@pytest.mark.parametrize("vid,l,shape,per_scene", CONFIGS)
def test_prepass_on_unaligned_slots(pt, oracle, vid, l, shape, per_scene):
    import torch
    frames, guesses, ref, pps = _case(oracle, l, shape, per_scene)
    n = len(frames)
    assert [tuple(s) for s in pps[0]["slots"]] == SHAPES[shape]
    counts = [pr.kept_pairs(pp, l) for pp in pps]
    for k, (kept, total) in enumerate(counts):
        print(f"prepass l={l} window={shape} {SCENES[k % 4]} #{k // 4}: restatement keeps {kept} of {total}; dc {pps[k]['dc']} V {pps[k]['V']} "
              f"origin {pps[k]['origin']} L {pps[k]['L']:.6g}")
    # what must hold for the restatement alone, before the kernel is consulted
    for k, (kept, total) in enumerate(counts):
        scene = k % 4
        if l == 65 and shape != (45, 45) and scene in (0, 3):
            assert kept < total, (shape, SCENES[scene], kept, total)
        if scene == 1:
            assert pps[k]["dc"] != FILL and pps[k]["dc"] - pps[k]["V"] > 0       # a bright level: no counted pixel is 0
        if scene == 2:                                                            # the disc's 0 sets V (it also pulls the sampled level a little off 255)
            assert pps[k]["V"] == pps[k]["dc"] >= 240
    if l == 17:
        assert (5, 8) in counts
    d_f, d_g = torch.from_numpy(frames).cuda(), torch.from_numpy(guesses).cuda()
    # ---- the batch: nothing the caller sees moves ----
    pos_p, max_p, ref_p, (kept, total) = _run(pt, d_f, d_g, vid, l, shape, 0)
    pos_d, max_d, ref_d, dense_counts = _run(pt, d_f, d_g, vid, l, shape, 1)
    print(f"prepass l={l} window={shape}: batch kept {kept} of {total}; windows refined {ref_p} / {ref_d}")
    assert dense_counts == (0, 0) and total > 0
    assert np.array_equal(pos_p, pos_d), np.argwhere(pos_p != pos_d)[:4]
    assert np.array_equal(pos_p, ref), np.argwhere(pos_p != ref)[:4]
    assert np.array_equal(max_p.view(np.int32), max_d.view(np.int32)), np.argwhere(max_p != max_d)[:4]
    assert ref_p == ref_d
    assert (kept, total) == (sum(c[0] for c in counts), sum(c[1] for c in counts))
    # ---- every window as a batch of its own, on a fresh tracker, out of the same stack (frame_index): the corner windows
    # read the stack's last rows ----
    for k in range(n):
        bt = _tracker(pt, vid, l, shape, 0, 1)
        try:
            pos = bt.detect(d_f, d_g[k:k + 1].contiguous(), frame_index=torch.tensor([k], dtype=torch.int32, device="cuda"))
            bt.sync()
            got = bt.prune_counts()
            pos = pos.cpu().numpy()
        finally:
            bt.close()
        assert got == counts[k], (k, SCENES[k % 4], got, counts[k])
        assert np.array_equal(pos[0], ref[k]), (k, SCENES[k % 4])
