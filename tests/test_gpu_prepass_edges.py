"""The roll batch path's pre-pass (csrc/dog_prune.hpp) where its clamped loads can go wrong.  A word of the tile that hangs
over the frame is loaded at its row and start column clamped into the frame and rebuilt by a shift of the clamp distance; a
wrong distance, a shift in the wrong direction or a mask that does not follow the shift moves the window's moments, and a
load that leaves the frame's columns reads the row's padding.  The smallest shapes that reach every such case:

  (45, 45) at l = 17, frame 70 × 83     the tile (61 × 61) hangs over one side at a time
  (65, 101) at l = 65, frame 150 × 83   the tile (129 × 165) is wider than the frame and hangs over both sides at once

The frame is 83 wide: no multiple of 4, so the last dword of a frame row is never whole.  Guesses put the tile's first column
at frame column −1 … −8 and its first row at frame row −1 … −8 (every clamp distance of an 8-byte cell to the left, every row
count above), and the tile's last 8-byte cell 1 … 7 bytes over the right edge with its last rows 1 … 7 over the bottom; on
the wide tile the eight left offsets put the cell that crosses the right edge at every alignment too.  Every window has a
frame of its own, chosen through a frame_index table out of a stack twice as long, rows row_stride = 83 + 13 bytes apart;
the last window reads the last frame of the stack.

Per window, each as a batch of its own on a fresh tracker (the policy sleeps after a window that keeps everything): the
kernel's (kept, total) equals the restatement's — dc, V, the cell choice, L, the threshold and every hull enter that number
— and the position equals the oracle's and the `no_prune` run's.  Every case runs twice, with the bytes of the row padding,
the gaps and the frames the table does not select all 0 and all 255: everything must be identical, so a load that strays
outside the frame's columns or rows shows up without any fault."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_restatement as fr  # noqa: E402
import prune_restatement as pr  # noqa: E402

FILL, FW, SLACK, GAP, BASE = 128, 83, 13, 5, 3
# (variant id, l, (h, w), frame height)
CONFIGS = [(117, 17, (45, 45), 70), (100, 65, (65, 101), 150)]
PATTERNS = (0, 255)


def _tw_for_kernel_len(l):
    for tw10 in range(20, 1400):
        if fr.kernel_len(fr.sigma_of(tw10 / 10)) == l:
            return tw10 / 10
    raise AssertionError(l)


def _guesses(l, shape, fh):
    """1-based guesses from the tile's first frame row / column (ti0, wj0): left with top, right with bottom."""
    hw, r1, r2 = l // 2, shape[0] // 2, shape[1] // 2
    NA, TWin = shape[0] + l - 1, shape[1] + l - 1
    ncx = -(-TWin // 8)
    origins = [(-k, -k) for k in range(1, 9)]                                   # first row / column at −1 … −8
    for k in range(1, 8):                                                       # the last rows / the last cell k over the edge
        wj0 = FW + k - 8 * ncx if TWin <= FW else -k                            # (the wide tile crosses the right edge at every offset)
        origins.append((fh + k - NA, wj0))
    out = [(ti0 + r1 + 1 + hw, wj0 + r2 + 1 + hw) for ti0, wj0 in origins]
    assert all(1 <= g1 <= fh and 1 <= g2 <= FW for g1, g2 in out), out
    return np.array(out, np.int32), origins


_CACHE = {}


def _case(oracle, l, shape, fh):
    """Frames (one per window), guesses, the oracle's positions and the restatement's counts: built once, left unchanged."""
    key = (l, shape)
    if key not in _CACHE:
        tw, radii = _tw_for_kernel_len(l), (shape[0] // 2, shape[1] // 2)
        rad = max(2, int(tw) // 2)
        guesses, origins = _guesses(l, shape, fh)
        rng = np.random.default_rng([l, shape[0], shape[1], fh])
        ii, jj = np.ogrid[:fh, :FW]
        frames = []
        for k, (g1, g2) in enumerate(guesses):
            f = np.full((fh, FW), FILL, np.uint8)
            ci, cj = min(max(g1 + 3 - k % 5, rad + 2), fh - rad - 1), min(max(g2 - 4 + k % 7, rad + 2), FW - rad - 1)   # a disc inside the frame
            f[(ii - (ci - 1)) ** 2 + (jj - (cj - 1)) ** 2 <= rad * rad] = 0
            f = np.clip(f.astype(np.int16) + rng.integers(-2, 3, f.shape), 0, 255).astype(np.uint8)
            # bright dots on the frame's own border, the bytes a wrong shift would lose or double: each is worth 123² to its
            # band's energy, enough to move a hull on these scenes (a full line would keep every block)
            f[::16, 0] = f[3::16, -1] = f[0, 5::16] = f[-1, 1::16] = 251
            frames.append(f)
        frames = np.stack(frames)
        K = oracle.dog_kernel(oracle.sigma(tw), True)
        ref = oracle.detect_batch(frames, FILL, K, radii, guesses)
        counts = [pr.kept_pairs(pr.prepass(fr.window_tile(f, FILL, l, radii, g), FILL, tw, True), l) for f, g in zip(frames, guesses)]
        _CACHE[key] = (frames, guesses, origins, ref, counts)
    return _CACHE[key]


def _stack(frames, pattern):
    """The frames at the odd places of a stack twice as long, rows FW + SLACK apart, GAP bytes between frames, the first
    frame BASE bytes into the buffer; every other byte holds `pattern`.  The buffer ends with the last frame's last pixel."""
    import torch
    n, fh, fw = frames.shape
    rs = fw + SLACK
    fs = fh * rs + GAP
    flat = np.full(BASE + (2 * n - 1) * fs + (fh - 1) * rs + fw, pattern, np.uint8)
    np.lib.stride_tricks.as_strided(flat[BASE + fs:], (n, fh, fw), (2 * fs, rs, 1))[:] = frames
    d_flat = torch.from_numpy(flat).cuda()
    view = torch.as_strided(d_flat, (2 * n, fh, fw), (fs, rs, 1), BASE)
    assert np.array_equal(view[1::2].cpu().numpy(), frames)
    return view, torch.arange(1, 2 * n, 2, dtype=torch.int32, device="cuda")


def _tracker(pt, vid, l, shape, fh, no_prune, batch):
    bt = pt.BatchTracker(fh, FW, _tw_for_kernel_len(l), shape, True, FILL)
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


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    return m


def test_guesses_reach_every_clamp_distance():
    """No GPU: the placements are what the text above says."""
    for vid, l, shape, fh in CONFIGS:
        _, origins = _guesses(l, shape, fh)
        NA, TWin = shape[0] + l - 1, shape[1] + l - 1
        assert sorted(-w for t, w in origins[:8]) == list(range(1, 9)) and sorted(-t for t, w in origins[:8]) == list(range(1, 9))
        assert sorted(t + NA - fh for t, w in origins[8:]) == list(range(1, 8))
        # by how many bytes the 8-byte cell over the right edge crosses it, on the tiles that reach that edge
        over = {(w - FW) % 8 for t, w in origins if w + 8 * -(-TWin // 8) > FW}
        assert over >= set(range(1, 8)), over
        assert FW % 4 and (TWin > FW) == (shape == (65, 101))


@pytest.mark.gpu
@pytest.mark.parametrize("vid,l,shape,fh", CONFIGS)
def test_prepass_on_frame_edges(pt, oracle, vid, l, shape, fh):
    import torch
    frames, guesses, origins, ref, counts = _case(oracle, l, shape, fh)
    n = len(frames)
    d_g = torch.from_numpy(guesses).cuda()
    seen = []
    for pattern in PATTERNS:
        d_f, d_idx = _stack(frames, pattern)
        bt = _tracker(pt, vid, l, shape, fh, 1, n)
        try:
            dense = bt.detect(d_f, d_g, frame_index=d_idx)
            bt.sync()
            dense = dense.cpu().numpy()
            assert bt.prune_counts() == (0, 0)
        finally:
            bt.close()
        assert np.array_equal(dense, ref), (pattern, np.argwhere(dense != ref)[:4])
        got = []
        for k in range(n):
            bt = _tracker(pt, vid, l, shape, fh, 0, 1)
            try:
                pos = bt.detect(d_f, d_g[k:k + 1].contiguous(), frame_index=d_idx[k:k + 1].contiguous())
                bt.sync()
                kc = bt.prune_counts()
                pos = pos.cpu().numpy()
            finally:
                bt.close()
            print(f"edges l={l} window={shape} pattern {pattern} tile origin {origins[k]}: kernel keeps {kc[0]} of {kc[1]}, restatement {counts[k]}; "
                  f"position {pos[0].tolist()} oracle {ref[k].tolist()}")
            assert kc == counts[k], (pattern, k, origins[k], kc, counts[k])
            assert np.array_equal(pos[0], ref[k]) and np.array_equal(pos[0], dense[k]), (pattern, k, origins[k], pos[0], ref[k], dense[k])
            got.append((kc, pos[0].tolist()))
        seen.append(got)
    assert seen[0] == seen[1]
    assert any(kept < total for kept, total in counts), counts      # the pre-pass prunes on these scenes at all
