"""The pre-pass's fast paths (csrc/dog_prune.hpp) where they begin and end.  The patch of the L pixels goes to LDS as loaded where
all its rows and whole dwords lie inside the frame, and through clamped loads, masks and fill otherwise; a wrong test reads outside
the frame or stages the wrong bytes.  L's row pass centres each pixel once and gives a thread four outputs of a row; the extremes
of the energy pass no longer mask odd bytes.  A mistake in any of them moves the window's V, L, hulls and job list.  Shapes with
full and partial 8 × 8 cells per side, a patch of 24 and of 72 rows, one pass and more than one pass of the energy loop and of the
patch staging:

  l = 17, window 25 × 25:   tile 41 × 41,   frame 96 × 128
  l = 65, window 33 × 33:   tile 97 × 97,   frame 112 × 128
  l = 17, window 129 × 129: tile 145 × 145, frame 176 × 192 (361 cells for 256 threads; two strips and a remainder column)

18 windows per shape, by the tile's first frame row / column (placements): the tile wholly inside the frame; its origin exactly at 0
and exactly at fh − NA / fw − TWin, the last positions still inside; one pixel further out on each of the four sides; the tile over
an edge while the target, and with it the patch, stays in the frame's interior; the target within l ÷ 2 of each edge, the patch over
it.  test_placements_are_what_they_say (no GPU) holds the list to that text with the restatement's own patch origin.

Each shape as one batch on a fresh tracker, three ways: plain; on a stack whose rows lie row_stride = fw + 13 bytes apart with 0x00
behind every row; behind a frame-index table out of a strided stack twice as long with 0xff in every byte that is no pixel (the
patch's plain loads step by the stride).  Per way: the job list, sorted, equals the restatement's refined strips entry for entry;
the counts equal the restatement's first-stage sums; positions equal the Float64 oracle's and the `no_prune` run's.
Measured on an MI355X: the file's nine GPU cases together 2.4 s."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_restatement as fr  # noqa: E402
import prune_restatement as pr  # noqa: E402
import prune_refine_restatement as rr  # noqa: E402
import prune_length_scenes as ps  # noqa: E402
import test_gpu_prepass_edges as edges  # noqa: E402

FILL, SLACK = 128, 13
# (l, window, frame height)
SHAPES = [(17, (25, 25), 96), (65, (33, 33), 112), (17, (129, 129), 176)]


def _fw(shape):
    return 128 if shape[1] < 100 else 192
WAYS = ("plain", "strided", "table")


def placements(l, shape, fh):
    """[(kind, tile origin (ti0, wj0))]"""
    NA, TWin = shape[0] + l - 1, shape[1] + l - 1
    b, r = fh - NA, _fw(shape) - TWin                # the last origins still inside
    over = min(l // 4, 6)                            # the tile over an edge by this much: the patch around the window's centre stays inside
    far = shape[0] // 2 + l // 2 - 2                 # the target two pixels from the edge
    out = [("inside", (5, 9)), ("inside", (b - 3, r - 6))]
    out += [("exact", o) for o in ((0, 0), (b, r), (0, r), (b, 0))]
    out += [("one-out", o) for o in ((-1, 5), (b + 1, 5), (5, -1), (5, r + 1))]
    out += [("tile-over", o) for o in ((-over, 7), (b + over, 7), (6, -over), (6, r + over))]
    out += [("patch-over", o) for o in ((-far, 11), (b + far, 11), (3, -far), (3, r + far))]
    return out


_CACHE = {}


def _case(oracle, l, shape, fh):
    """Frames (one per window), guesses, the oracle's positions, the restatement's prepass / refined hulls: built once, left unchanged."""
    key = (l, shape, fh)
    if key not in _CACHE:
        tw, radii, hw, FW = edges._tw_for_kernel_len(l), (shape[0] // 2, shape[1] // 2), l // 2, _fw(shape)
        rad = max(2, int(tw) // 2)
        origins = [o for _, o in placements(l, shape, fh)]
        guesses = np.array([(ti0 + radii[0] + 1 + hw, wj0 + radii[1] + 1 + hw) for ti0, wj0 in origins], np.int32)
        assert all(1 <= g1 <= fh and 1 <= g2 <= FW for g1, g2 in guesses), guesses
        rng = np.random.default_rng([l, shape[0], shape[1], fh])
        ii, jj = np.ogrid[:fh, :FW]
        frames = []
        for k, (g1, g2) in enumerate(guesses):
            f = np.full((fh, FW), FILL, np.uint8)
            ci, cj = min(max(g1 + 2 - k % 4, rad + 2), fh - rad - 1), min(max(g2 - 3 + k % 5, rad + 2), FW - rad - 1)   # a disc near the guess, inside the frame
            f[(ii - (ci - 1)) ** 2 + (jj - (cj - 1)) ** 2 <= rad * rad] = 0
            f = np.clip(f.astype(np.int16) + rng.integers(-2, 3, f.shape), 0, 255).astype(np.uint8)
            if shape[0] < 100:   # bright dots on the frame's own border (tests/test_gpu_prepass_edges.py); on the large window they would
                f[::16, 0] = f[3::16, -1] = f[0, 5::16] = f[-1, 1::16] = 251     # push the cell choice, and the patch with it, off the edge
            frames.append(f)
        frames = np.stack(frames)
        ref = oracle.detect_batch(frames, FILL, oracle.dog_kernel(oracle.sigma(tw), True), radii, guesses)
        pps, rfs = [], []
        for f, g in zip(frames, guesses):
            tile = fr.window_tile(f, FILL, l, radii, g)
            pps.append(pr.prepass(tile, FILL, tw, True))
            rfs.append(rr.refine(tile, FILL, tw, True, pps[-1]))
        _CACHE[key] = (frames, guesses, origins, ref, pps, rfs)
    return _CACHE[key]


def _strided(frames, pattern):
    """The frames in one buffer, rows FW + SLACK bytes apart, `pattern` in every byte that is no pixel."""
    import torch
    n, fh, fw = frames.shape
    rs = fw + SLACK
    flat = np.full(n * fh * rs, pattern, np.uint8)
    flat.reshape(n, fh, rs)[:, :, :fw] = frames
    view = torch.as_strided(torch.from_numpy(flat).cuda(), (n, fh, fw), (fh * rs, rs, 1))
    assert np.array_equal(view.cpu().numpy(), frames)
    return view


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    return m


def _run(pt, l, shape, fh, d_f, d_g, d_idx, no_prune):
    bt = pt.BatchTracker(fh, _fw(shape), edges._tw_for_kernel_len(l), shape, True, FILL)
    try:
        assert bt.info().kernel_len == l
        bt.set_variant(ps.variant_id(l))
        bt.set_tuning("no_prune", no_prune)
        bt.set_exact(1)
        assert bt.kernel_for_batch(len(d_g)) == ps.variant_id(l)
        pos = bt.detect(d_f, d_g, frame_index=d_idx) if d_idx is not None else bt.detect(d_f, d_g)
        bt.sync()
        jobs = None if no_prune else sorted(tuple(int(v) for v in row) for row in bt.prune_jobs())
        return pos.cpu().numpy(), bt.prune_counts(), jobs
    finally:
        bt.close()


@pytest.mark.parametrize("l,shape,fh", SHAPES)
def test_placements_are_what_they_say(oracle, l, shape, fh):
    """No GPU: full and partial cells on both sides, and each kind of placement is what the text above says."""
    frames, guesses, origins, ref, pps, rfs = _case(oracle, l, shape, fh)
    NA, TWin, FW = shape[0] + l - 1, shape[1] + l - 1, _fw(shape)
    assert NA % 8 and TWin % 8 and NA // 8 >= 5 and TWin // 8 >= 5
    kinds = [k for k, _ in placements(l, shape, fh)]
    assert 16 <= len(kinds) <= 32
    for kind, (ti0, wj0), pp in zip(kinds, origins, pps):
        tile_in = ti0 >= 0 and ti0 + NA <= fh and wj0 >= 0 and wj0 + TWin <= FW
        oy, ox = pp["origin"]
        PH, PQ4 = 8 + l - 1, (8 + l - 1 + 3) // 4 * 4
        patch_in = ti0 + oy >= 0 and ti0 + oy + PH <= fh and wj0 + ox >= 0 and wj0 + ox + PQ4 <= FW
        assert tile_in == (kind in ("inside", "exact")), (kind, ti0, wj0)
        if kind == "exact":
            assert ti0 in (0, fh - NA) and wj0 in (0, FW - TWin)
        if kind == "one-out":
            assert (ti0 in (-1, fh - NA + 1)) != (wj0 in (-1, FW - TWin + 1))
        if kind == "tile-over":
            assert patch_in, (ti0, wj0, oy, ox)
        if kind == "patch-over":
            assert not patch_in, (ti0, wj0, oy, ox)
    assert {(o[0] < 0, o[0] + NA > fh, o[1] < 0, o[1] + TWin > FW) for k, o in zip(kinds, origins) if k == "patch-over"} == \
        {(True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True)}
    # the energies decide something on these scenes: a block span covers most of so small a tile, so at l = 17 the first stage
    # excludes in a few windows only, and at l = 65 nothing, where the second stage narrows nearly every window
    assert any(pr.kept_pairs(pp, l)[0] < pr.kept_pairs(pp, l)[1] for pp in pps) or any(rf["hull"] != pp["hull"] for pp, rf in zip(pps, rfs))


@pytest.mark.gpu
@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("l,shape,fh", SHAPES)
def test_fast_paths_against_the_restatement(pt, oracle, l, shape, fh, way):
    import torch
    frames, guesses, origins, ref, pps, rfs = _case(oracle, l, shape, fh)
    nstrips = len([1 for _, w in pr.slots(shape[1]) if w > 1])
    want_jobs = sorted((b, s, ba, bb) for b, rf in enumerate(rfs) for s, (ba, bb) in enumerate(rf["hull"][:nstrips]) if bb > ba)
    want_counts = tuple(int(sum(pr.kept_pairs(pp, l)[i] for pp in pps)) for i in (0, 1))
    d_g = torch.from_numpy(guesses).cuda()
    if way == "plain":
        d_f, d_idx = torch.from_numpy(frames).cuda(), None
    elif way == "strided":
        d_f, d_idx = _strided(frames, 0), None
    else:
        d_f, d_idx = edges._stack(frames, 255)
    dense, dense_counts, _ = _run(pt, l, shape, fh, d_f, d_g, d_idx, 1)
    pos, counts, jobs = _run(pt, l, shape, fh, d_f, d_g, d_idx, 0)
    print(f"fast paths l={l} window={shape} {way}: kernel keeps {counts[0]} of {counts[1]} (restatement {want_counts}), {len(jobs)} jobs (restatement {len(want_jobs)})")
    assert dense_counts == (0, 0)
    assert jobs == want_jobs, [(a, b) for a, b in zip(jobs, want_jobs) if a != b][:4]
    assert counts == want_counts, (counts, want_counts)
    assert np.array_equal(pos, ref), [(k, origins[k], pos[k].tolist(), ref[k].tolist()) for k in np.argwhere((pos != ref).any(1)).ravel()[:4]]
    assert np.array_equal(pos, dense), np.argwhere(pos != dense)[:4]
