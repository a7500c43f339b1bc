"""Buffer growth on a LIVE tracker.  Every other test creates a tracker and calls it at one size; here ONE tracker per case is
called with a small n, then a larger n (its device / pinned buffers are freed and reallocated behind work that may still be
queued), then the small n again (the larger buffers are kept), and every call's positions must equal the oracle's
(PARITY UNPINNED: the oracle is this repo's restatement of the reference functor, src/PawsomeTracker.jl:55-62).  The cases
are the smallest shapes that reach each place where the host code grows a buffer."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W = 120, 160


@pytest.fixture(scope="module")
def pt():
    import pawsometracker_jl_amd as m
    return m


def _batch(oracle, n, h, w, tw, ws, seed):
    """n noisy frames with guesses, the fill value and the oracle's positions (computed once for the largest n: windows are
    independent, so a smaller call is a prefix)."""
    from oracle import synth
    radii = (ws[0] // 2, ws[1] // 2)
    frames, guesses, _ = synth.make_batch(n, h, w, tw, radii, True, seed=seed, noise=3)
    fill = oracle.mode_u8(frames[0])
    ref = oracle.detect_batch(frames, fill, oracle.dog_kernel(oracle.sigma(tw), True), radii, guesses)
    return frames, guesses, fill, ref


def _clips(oracle, n_clips, n_frames, h, w, tw, ws, seed, fill=128):
    """n_clips clips of a dark disc on a random walk over ±3 noise, start guesses, and the oracle's serial chains
    (ij[k] = trckr(ij[k-1]), :167)."""
    from oracle import synth
    rng = np.random.Generator(np.random.PCG64(seed))
    radii = (ws[0] // 2, ws[1] // 2)
    K = oracle.dog_kernel(oracle.sigma(tw), True)
    frames = (fill + rng.integers(-3, 4, (n_clips, n_frames, h, w))).astype(np.uint8)
    starts = np.empty((n_clips, 2), np.int32)
    want = np.empty((n_clips, n_frames, 2), np.int32)
    for c in range(n_clips):
        ci, cj = h // 2 + 7 * c, w // 2 - 9 * c
        starts[c] = g = (ci + 2, cj - 3)
        for k in range(n_frames):
            ci = int(np.clip(ci + rng.integers(-6, 7), 5, h - 5))
            cj = int(np.clip(cj + rng.integers(-6, 7), 5, w - 5))
            disc = synth.disc_frame(h, w, (ci, cj), tw, True)
            frames[c, k][disc == 0] = 0
            g = oracle.detect(frames[c, k], fill, K, radii, g)
            want[c, k] = g
    return frames, starts, want


@pytest.mark.parametrize("name,tw,ws,variant,tuning,sizes", [
    # l = 29 roll kernel, 64 + 5 columns: one strip and five thin columns per window; the partial arrays grow
    ("strips_thin", 10, (33, 69), 129, None, (3, 40, 3)),
    # l = 65 roll kernel, 64 + 1 columns: the remainder column folded into the (only) strip; d_fold_r grows
    ("folded_column", 25, (33, 65), 100, "fold_always", (2, 24, 2)),
    # two-pass kernels, exact mode on: two-launch form, four-launch form, two-launch form; d_V, d_dc and d_map grow
    ("two_pass", 10, (33, 33), 200, None, (2, 20, 2)),
])
def test_batch_buffers_grow(pt, oracle, name, tw, ws, variant, tuning, sizes):
    import torch
    frames, guesses, fill, ref = _batch(oracle, max(sizes), H, W, tw, ws, seed=31)
    bt = pt.BatchTracker(H, W, tw, ws, True, fill)
    bt.set_variant(variant)
    if tuning:
        bt.set_tuning(tuning, 1)
    assert bt.exact_stats()[0], "exact mode is on by default"
    d_f, d_g = torch.from_numpy(frames).cuda(), torch.from_numpy(guesses).cuda()
    for n in sizes:
        assert bt.kernel_for_batch(n) == variant
        out = bt.detect(d_f[:n], d_g[:n].contiguous())
        bt.sync()
        assert np.array_equal(out.cpu().numpy(), ref[:n]), (name, n)
    bt.close()


@pytest.mark.parametrize("name,h,w,ws,variant,n_frames,clips", [
    # a window too large for the fused kernel (a 229×229 float tile): one cooperative launch of the tiled kernel per call;
    # its control words and partial slots grow with the number of clips
    ("tiled", 240, 320, (201, 201), None, 4, (1, 2, 1)),
    # pinned ring kernel: per-frame launches over all clips, the guesses carried in d_chain_tmp
    ("by_launches", H, W, (21, 21), 0, 3, (2, 5, 2)),
])
def test_chain_buffers_grow(pt, oracle, name, h, w, ws, variant, n_frames, clips):
    import torch
    tw, fill = 10, 128
    frames, starts, want = _clips(oracle, max(clips), n_frames, h, w, tw, ws, seed=47, fill=fill)
    bt = pt.BatchTracker(h, w, tw, ws, True, fill)
    if variant is None:
        assert bt.kernel_for_batch(1) == 400, "the window should be served by the tiled kernel"
    else:
        bt.set_variant(variant)
    d_f, d_s = torch.from_numpy(frames).cuda(), torch.from_numpy(starts).cuda()
    for nc in clips:
        out = bt.detect_chains(d_f[:nc], d_s[:nc].contiguous())
        bt.sync()
        assert np.array_equal(out.cpu().numpy(), want[:nc]), (name, nc)
    bt.close()


def test_host_ingest_slots_grow(pt, oracle):
    """pdog_detect_batch_host: the pinned staging and device tile slots, the centre guesses and the result arrays."""
    tw, ws = 10, (21, 21)
    frames, guesses, fill, ref = _batch(oracle, 50, H, W, tw, ws, seed=59)
    bt = pt.BatchTracker(H, W, tw, ws, True, fill)
    for n in (2, 50, 2):
        assert np.array_equal(bt.detect_host(frames[:n], guesses[:n]), ref[:n]), n
    bt.close()


def test_functor_buffers_appear_on_first_use(pt, oracle):
    """Tracker.__call__: the pinned tile on the first call, the response buffer on the first call that asks for one."""
    tw, ws = 10, (21, 21)
    frames, guesses, fill, ref = _batch(oracle, 3, H, W, tw, ws, seed=61)
    t = pt.Tracker(frames[0], tw, ws, True)
    assert t.img.fillvalue == fill
    got = []
    for k, want_resp in enumerate((False, True, False)):
        t.img.data[...] = frames[k]
        r = t(tuple(int(v) for v in guesses[k]), want_resp=want_resp)
        got.append(r[0] if want_resp else r)
    t.close()
    assert np.array_equal(np.array(got, np.int32), ref)
