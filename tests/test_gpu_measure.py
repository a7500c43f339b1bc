"""pdog_measure on the GPU (dog_measure_kernel, BatchTracker.measure, Tracker.measure, track_frames(subpixel=True)):
the five responses and the sub-pixel positions bit for bit against tests/measure_restatement.py — the responses are the
C oracle's (the reference's buff[I], src/PawsomeTracker.jl:57), the rule is this library's own — plus stream order, the
state detection reads, the accuracy condition on the spiral clip and every argument check."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measure_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    return m


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _scene(h, w, nf, seed, darker):
    """nf frames: background 128 with +-3 levels of noise and a few discs — some cut by the frame's border — so that
    responses near corners and edges are not flat; returned as a view with row stride w + 19."""
    from oracle import synth
    rng = np.random.default_rng(seed)
    wide = np.empty((nf, h, w + 19), np.uint8)
    wide[...] = rng.integers(0, 256, wide.shape)           # bytes past the row's end: must never be read as pixels
    for k in range(nf):
        f = np.full((h, w), 128, np.int16)
        for c in [(1, 1), (h, w), (1, w // 2), (h // 2, w), (h // 2, w // 2), (int(rng.integers(1, h + 1)), int(rng.integers(1, w + 1)))]:
            d = synth.disc_frame(h, w, c, 10, darker)
            f[d != 128] = d[d != 128]
        f += rng.integers(-3, 4, (h, w))
        wide[k, :, :w] = np.clip(f, 0, 255)
    return wide[:, :, :w]


def _positions(h, w, n, rng):
    """Corners, a point on each edge, the interior, positions outside the frame (clamped), then random ones."""
    fixed = [(1, 1), (1, w), (h, 1), (h, w), (1, w // 2), (h, w // 3), (h // 2, 1), (h // 3, w), (h // 2, w // 2),
             (0, 0), (-7, w // 2), (h + 5, w + 9), (h // 2, w + 1)]
    rand = [(int(rng.integers(-3, h + 4)), int(rng.integers(-3, w + 4))) for _ in range(max(0, n - len(fixed)))]
    return np.array((fixed + rand)[:n], np.int32)


def _measure_raw(pt, bt, frames_t, ij_t, fi_t, want_sub, want_resp):
    """pdog_measure itself, with either output NULL."""
    import torch
    n = ij_t.shape[0]
    sub = torch.full((n, 2), -1.0, dtype=torch.float64, device="cuda") if want_sub else None
    r5 = torch.full((n, 5), -1.0, dtype=torch.float64, device="cuda") if want_resp else None
    bt.use_torch_stream()
    rc = pt.lib().pdog_measure(bt._h, C.c_void_p(frames_t.data_ptr()), frames_t.stride(0), frames_t.stride(1), frames_t.shape[0],
                               C.c_void_p(fi_t.data_ptr()) if fi_t is not None else None, C.c_void_p(ij_t.data_ptr()), n,
                               C.c_void_p(r5.data_ptr()) if want_resp else None, C.c_void_p(sub.data_ptr()) if want_sub else None)
    assert rc == 0, pt.lib().pdog_last_error()
    bt.sync()
    return (sub.cpu().numpy() if want_sub else None), (r5.cpu().numpy() if want_resp else None)


def _strided_cuda(frames):
    """The frames on the device with the row stride of the host view (w + 19)."""
    import torch
    base = frames.base if frames.base is not None else frames
    t = torch.from_numpy(np.ascontiguousarray(base)).cuda()
    return t[:, :, :frames.shape[2]]


@pytest.mark.parametrize("darker", [True, False])
@pytest.mark.parametrize("target_width", [10, 25, 44])
def test_values_equal_the_restatement(pt, oracle, target_width, darker):
    import torch
    h, w, nf, fill = 60, 80, 3, 77                        # the fill differs from the background (128)
    frames = _scene(h, w, nf, 100 + target_width, darker)
    ft = _strided_cuda(frames)
    assert ft.stride(1) == w + 19
    K = oracle.dog_kernel(oracle.sigma(target_width), darker)
    bt = pt.BatchTracker(h, w, target_width, (21, 21), darker, fill)
    assert bt.info().kernel_len == K.shape[0]
    rng = np.random.default_rng(target_width)
    for n in (1, 13, 1000):
        ij = _positions(h, w, n, rng)
        fi = rng.integers(0, nf, n).astype(np.int32) if n > 1 else np.array([2], np.int32)    # repeats, any order
        ref_sub, ref_r5 = R.measure(oracle, frames, fill, K, ij, fi)
        ij_t, fi_t = torch.from_numpy(ij).cuda(), torch.from_numpy(fi).cuda()
        sub, r5 = bt.measure(ft, ij_t, frame_index=fi_t, want_resp=True)
        bt.sync()
        assert np.array_equal(_bits(r5.cpu().numpy()), _bits(ref_r5)), (target_width, darker, n)
        assert np.array_equal(_bits(sub.cpu().numpy()), _bits(ref_sub)), (target_width, darker, n)
        # each output on its own, the other NULL
        only_sub, none = _measure_raw(pt, bt, ft, ij_t, fi_t, True, False)
        assert none is None and np.array_equal(_bits(only_sub), _bits(ref_sub))
        none, only_r5 = _measure_raw(pt, bt, ft, ij_t, fi_t, False, True)
        assert none is None and np.array_equal(_bits(only_r5), _bits(ref_r5))
        assert np.array_equal(_bits(bt.measure(ft, ij_t, frame_index=fi_t).cpu().numpy()), _bits(ref_sub))
        # the kernel's other layout: the frame read in place (what a kernel too long for an LDS tile runs)
        bt.set_tuning("measure_global", 1)
        sub, r5 = bt.measure(ft, ij_t, frame_index=fi_t, want_resp=True)
        bt.set_tuning("measure_global", 0)
        assert np.array_equal(_bits(r5.cpu().numpy()), _bits(ref_r5)) and np.array_equal(_bits(sub.cpu().numpy()), _bits(ref_sub))
    # no frame index: position b looks at frame b
    ij = _positions(h, w, nf, rng)
    ref_sub, ref_r5 = R.measure(oracle, frames, fill, K, ij)
    sub, r5 = bt.measure(ft, torch.from_numpy(ij).cuda(), want_resp=True)
    assert np.array_equal(_bits(sub.cpu().numpy()), _bits(ref_sub)) and np.array_equal(_bits(r5.cpu().numpy()), _bits(ref_r5))
    # the clamp and the rule did something on these inputs
    assert (ref_sub != np.clip(ij, 1, (h, w))).any()
    bt.close()


@pytest.mark.parametrize("darker", [True, False])
@pytest.mark.parametrize("tw,l", [(120, 293), (170, 413)])
def test_values_at_long_kernels(pt, oracle, tw, l, darker):
    """target_width 120: l = 293, an 85 849-term chain per value; target_width 170: l = 413.  Kernels this long read the
    frame in place (no LDS tiles).  A few positions each."""
    import torch
    h, w, fill = 120, 160, 40
    frames = _scene(h, w, 1, 7, darker)
    ft = _strided_cuda(frames)
    K = oracle.dog_kernel(oracle.sigma(tw), darker)
    assert K.shape[0] == l
    bt = pt.BatchTracker(h, w, tw, (21, 21), darker, fill)
    ij = np.array([(1, 1), (h, w // 2), (h // 2, w // 2), (h + 30, -4), (37, 111)], np.int32)
    fi = np.zeros(len(ij), np.int32)
    ref_sub, ref_r5 = R.measure(oracle, frames, fill, K, ij, fi)
    sub, r5 = bt.measure(ft, torch.from_numpy(ij).cuda(), frame_index=torch.from_numpy(fi).cuda(), want_resp=True)
    bt.sync()
    assert np.array_equal(_bits(r5.cpu().numpy()), _bits(ref_r5))
    assert np.array_equal(_bits(sub.cpu().numpy()), _bits(ref_sub))
    bt.close()


def test_stream_order_and_detection_state(pt, oracle):
    """detect_chains then measure with no synchronisation in between gives what the synchronised sequence gives, and a
    measure leaves what detection reads alone: exact_stats() and the positions of a repeated detect."""
    import torch
    nc, nf, tw, ws = 8, 12, 10, (21, 21)
    clips = np.stack([R.spiral_clip(20 + c, True, nf)[0] for c in range(nc)])
    ft = torch.from_numpy(clips).cuda()
    starts = torch.tensor([[50, 50]] * nc, dtype=torch.int32, device="cuda")
    fill = oracle.mode_u8(clips[0, 0])
    bt = pt.BatchTracker(R.H, R.W, tw, ws, True, fill)
    # with a host wait between the two
    out_a = bt.detect_chains(ft, starts)
    bt.sync()
    sub_a, r5_a = bt.measure(ft.flatten(0, 1), out_a.view(-1, 2), want_resp=True)
    bt.sync()
    # queued back to back
    out_b = bt.detect_chains(ft, starts)
    sub_b, r5_b = bt.measure(ft.flatten(0, 1), out_b.view(-1, 2), want_resp=True)
    bt.sync()
    assert torch.equal(out_a, out_b)
    assert np.array_equal(_bits(sub_a.cpu().numpy()), _bits(sub_b.cpu().numpy()))
    assert np.array_equal(_bits(r5_a.cpu().numpy()), _bits(r5_b.cpu().numpy()))
    K = oracle.dog_kernel(oracle.sigma(tw), True)
    ref_sub, ref_r5 = R.measure(oracle, clips.reshape(-1, R.H, R.W), fill, K, out_a.view(-1, 2).cpu().numpy())
    assert np.array_equal(_bits(sub_b.cpu().numpy()), _bits(ref_sub)) and np.array_equal(_bits(r5_b.cpu().numpy()), _bits(ref_r5))
    assert (sub_b.view(nc, nf, 2).cpu().numpy() != out_b.cpu().numpy()).any()
    # detection state
    frames = ft.flatten(0, 1)
    guesses = out_a.view(-1, 2).contiguous()
    first = bt.detect(frames, guesses)
    bt.sync()
    stats, detail, variant = bt.exact_stats(), bt.exact_detail(), bt.info().variant
    bt.measure(frames, guesses, want_resp=True)
    bt.sync()
    assert bt.exact_stats() == stats and bt.exact_detail() == detail and bt.info().variant == variant
    second = bt.detect(frames, guesses)
    bt.sync()
    assert torch.equal(first, second)
    bt.close()


@pytest.mark.parametrize("darker", [True, False])
@pytest.mark.parametrize("target_width", [25, 10])
def test_track_frames_subpixel_on_the_spiral_clip(pt, oracle, target_width, darker):
    """Positions are the oracle chain's, `sub` is the restatement applied to it, and the accuracy condition: the RMSE of
    `sub` against the true centres is below half the RMSE of the integer positions on the same clip.  (The factor 2 is
    a condition, not a measurement: the oracle alone is 15x or better on these clips, tests/test_measure_cpu.py.)"""
    frames, centres = R.spiral_clip(0, darker)
    ws = pt.fix_window_size(pt.guess_window_size(target_width))
    ref_ij, fill, K = R.oracle_chain(oracle, frames, target_width, ws, darker)
    ref_sub, _ = R.measure(oracle, frames, fill, K, ref_ij)
    plain = pt.track_frames(frames, target_width=target_width, start_location=("ij", (50, 50)), darker_target=darker)
    got_ij, got_sub = pt.track_frames(frames, target_width=target_width, start_location=("ij", (50, 50)), darker_target=darker,
                                      subpixel=True)
    assert plain == ref_ij and got_ij == ref_ij           # the default return value is today's
    assert len(got_sub) == len(frames) and all(isinstance(s, tuple) and len(s) == 2 for s in got_sub)
    assert np.array_equal(_bits(np.array(got_sub)), _bits(ref_sub))
    e_int, e_sub = R.rmse(got_ij, centres), R.rmse(got_sub, centres)
    print(f"spiral clip tw={target_width} darker={darker}: RMSE integer {e_int:.4f} px, sub-pixel {e_sub:.4f} px")
    assert e_sub < 0.5 * e_int


def test_track_segments_subpixel_and_tracker_measure(pt, oracle):
    frames, _ = R.spiral_clip(3, True, 15)
    segs = [frames[:6], frames[6:11], frames[11:15]]
    plain = pt.track_segments(segs, [("ij", (50, 50)), None, None], target_width=10)
    ijs, sub = pt.track_segments(segs, [("ij", (50, 50)), None, None], target_width=10, subpixel=True)
    assert ijs == plain and len(sub) == 15
    t = pt.Tracker(frames[0], 10, (21, 21), True)
    K = oracle.dog_kernel(oracle.sigma(10), True)
    for k in range(15):                                    # every segment's tracker takes its fill from its own first frame
        fill = oracle.mode_u8(frames[0 if k < 6 else 6 if k < 11 else 11])
        ref_sub, _ = R.measure(oracle, frames[k:k + 1], fill, K, [ijs[k]])
        assert np.array_equal(_bits(np.array(sub[k])), _bits(ref_sub[0])), k
    # Tracker.measure on its current frame, responses included
    t.img.data[...] = frames[4]
    s, r5 = t.measure(ijs[4], want_resp=True)
    ref_sub, ref_r5 = R.measure(oracle, frames[4:5], t.img.fillvalue, K, [ijs[4]])
    assert np.array_equal(_bits(np.array(s)), _bits(ref_sub[0])) and np.array_equal(_bits(np.array(r5)), _bits(ref_r5[0]))
    assert t.measure(ijs[4]) == s and t(ijs[4]) == ijs[4]
    assert pt.subpixel(r5, ijs[4]) == s
    t.close()


def test_error_returns(pt):
    import torch
    L, E = pt.lib(), pt._lib.PDOG_E_ARG
    h, w = 40, 50
    bt = pt.BatchTracker(h, w, 10, (21, 21), True, 128)
    bt.use_torch_stream()
    f = torch.full((2, h, w), 128, dtype=torch.uint8, device="cuda")
    ij = torch.tensor([[5, 5], [6, 6]], dtype=torch.int32, device="cuda")
    sub = torch.zeros((2, 2), dtype=torch.float64, device="cuda")
    r5 = torch.zeros((2, 5), dtype=torch.float64, device="cuda")
    fi = torch.zeros(2, dtype=torch.int32, device="cuda")
    P = lambda t_: C.c_void_p(t_.data_ptr())

    def call(t=bt._h, frames=P(f), fs=h * w, rs=w, nf=2, index=None, pos=P(ij), n=2, o5=P(r5), osub=P(sub)):
        return L.pdog_measure(t, frames, fs, rs, nf, index, pos, n, o5, osub)

    assert call() == 0
    assert call(t=None) == E                               # null tracker
    assert call(frames=None) == E                          # null frames
    assert call(pos=None) == E                             # null d_ij
    assert call(o5=None, osub=None) == E                   # both outputs NULL
    assert b"pdog_measure" in L.pdog_last_error()
    assert call(n=-1) == E
    assert call(nf=0) == E and call(nf=-3) == E
    assert call(rs=w - 1) == E                             # row_stride < frame_w
    assert call(fs=-1) == E                                # negative frame_stride
    assert call(n=2, nf=1) == E                            # more positions than frames and no frame index (as for a batch)
    assert call(n=2, nf=1, index=P(fi)) == 0
    assert call(o5=None) == 0 and call(osub=None) == 0
    # n == 0 does nothing
    sub.fill_(-2.0)
    assert call(n=0) == 0
    bt.sync()
    assert (sub.cpu().numpy() == -2.0).all()
    bt.close()
