"""The diagnostic overlay on the GPU (pdog_diag_*, Diagnose, track_frames(diagnostic=...), track_segments): every
buffer bit for bit against the NumPy restatement of src/diagnose.jl:26-38 (tests/diag_restatement.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diag_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    return m


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _noise(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w), dtype=np.uint8)


def _walk(n, h, w, seed, step=9):
    """Corners, points that scale to 0, a jump across the whole frame and repeated points first, then a random walk."""
    rng = np.random.default_rng(seed)
    out = [(1, 1), (h, w), (1, w), (h, 1), (2, 2), (h, w), (1, 1), (1, 1), (h // 2, w // 2)]
    p = np.array([h // 2, w // 2])
    while len(out) < n:
        p = np.clip(p + rng.integers(-step, step + 1, 2), 1, [h, w])
        out.append((int(p[0]), int(p[1])))
    return np.array(out[:n], np.int32)


def _ref(frames, ij, darker=True, ref=None):
    ref = ref if ref is not None else R.Diagnose(darker)
    return ref.render(list(frames), [(int(p[0]), int(p[1])) for p in ij])


def _disc_clip(n, h, w, tw, seed):
    from oracle import synth
    rng = np.random.default_rng(seed)
    pos = np.clip(np.cumsum(rng.integers(-4, 5, (n, 2)), 0) + 50, 8, 92)
    return np.stack([synth.disc_frame(h, w, (int(p[0]), int(p[1])), tw, True) for p in pos]), pos


@pytest.mark.parametrize("darker", [True, False])
@pytest.mark.parametrize("h,w,n", [(100, 100, 40), (240, 320, 30), (271, 481, 20), (720, 1280, 12), (1080, 1920, 12),
                                   (2160, 3840, 10)])
def test_geometry_matrix(pt, h, w, n, darker):
    frames, ij = _noise(n, h, w, seed=h + w), _walk(n, h, w, seed=h)
    with pt.Diagnose(darker) as dia:
        got = dia(_cuda(frames), _cuda(ij)).cpu().numpy()
    assert np.array_equal(got, _ref(frames, ij, darker))


@pytest.mark.parametrize("n", [1, 99, 100, 101, 250])
def test_trace_length(pt, n):
    frames, ij = _noise(n, 120, 200, seed=n), _walk(n, 120, 200, seed=n, step=15)
    with pt.Diagnose() as dia:
        got = dia(_cuda(frames), _cuda(ij)).cpu().numpy()
    assert np.array_equal(got, _ref(frames, ij))


def test_row_and_frame_strides(pt):
    n, h, w = 30, 271, 481
    big = _cuda(_noise(2 * n, h + 5, w + 40, seed=7))
    frames = big[::2, 3:3 + h, 17:17 + w]
    assert frames.stride(1) == w + 40 and frames.stride(0) == 2 * (h + 5) * (w + 40)
    ij = _walk(n, h, w, seed=3)
    with pt.Diagnose() as dia:
        got = dia(frames, _cuda(ij)).cpu().numpy()
    assert np.array_equal(got, _ref(frames.cpu().numpy(), ij))


def test_unaligned_output(pt):
    import torch
    n, h, w = 5, 240, 320
    frames, ij = _noise(n, h, w, seed=4), _walk(n, h, w, seed=4)
    buf = torch.empty(n * 360 * 640 + 1, dtype=torch.uint8, device="cuda")
    out = buf[1:].view(n, 360, 640)
    with pt.Diagnose() as dia:
        dia(_cuda(frames), _cuda(ij), out=out)
    assert np.array_equal(out.cpu().numpy(), _ref(frames, ij))


def test_chunks_equal_one_call(pt):
    n, h, w = 250, 100, 100
    frames, ij = _noise(n, h, w, seed=11), _walk(n, h, w, seed=11, step=12)
    F, P = _cuda(frames), _cuda(ij)
    with pt.Diagnose() as dia:
        whole = dia(F, P).cpu().numpy()
    parts, k = [], 0
    with pt.Diagnose() as dia:
        for c in (1, 7, 100, 142):
            parts.append(dia(F[k:k + c], P[k:k + c]).cpu().numpy())
            k += c
    assert np.array_equal(np.concatenate(parts), whole)
    assert np.array_equal(whole, _ref(frames, ij))


def test_trace_runs_on_across_frame_sizes(pt):
    a, pa = _noise(40, 1080, 1920, seed=5), _walk(40, 1080, 1920, seed=5, step=40)
    b, pb = _noise(30, 720, 1280, seed=6), _walk(30, 720, 1280, seed=6, step=40)
    with pt.Diagnose() as dia:
        ga = dia(_cuda(a), _cuda(pa)).cpu().numpy()
        gb = dia(_cuda(b), _cuda(pb)).cpu().numpy()
    ref = R.Diagnose()
    assert np.array_equal(ga, _ref(a, pa, ref=ref))
    assert np.array_equal(gb, _ref(b, pb, ref=ref))
    assert not np.array_equal(gb[0], R.Diagnose()(b[0], tuple(pb[0])))    # the 1080p points are still drawn


def test_positions_outside_the_frame_are_clamped(pt):
    h, w = 240, 320
    ij = np.array([(0, 0), (-5, 400), (300, -2), (241, 321), (10 ** 6, 10 ** 6), (-10 ** 6, 5), (120, 160), (0, 160),
                   (240, 0), (5, 5), (1000, 1000), (1, 1)], np.int32)
    frames = _noise(len(ij), h, w, seed=9)
    with pt.Diagnose() as dia:
        got = dia(_cuda(frames), _cuda(ij)).cpu().numpy()
    clamped = [R.clamp_ij(h, w, p) for p in ij]
    assert np.array_equal(got, _ref(frames, ij)) and np.array_equal(got, _ref(frames, clamped))


def test_after_detect_chain_without_sync(pt):
    tw, h, w = 10, 100, 100
    frames, pos = _disc_clip(60, h, w, tw, seed=3)
    bt = pt.BatchTracker(h, w, tw, (21, 21), True, pt.mode(frames[0]))
    F = _cuda(frames)
    with pt.Diagnose(True) as dia:
        ij = bt.detect_chain(F, (50, 50))
        got = dia(F, ij).cpu().numpy()             # same stream, no host synchronisation in between
    bt.close()
    ij = ij.cpu().numpy()
    assert [tuple(p) for p in ij] == [tuple(p) for p in pos]
    assert np.array_equal(got, _ref(frames, ij))


def test_track_frames_diagnostic_sink(pt):
    frames, pos = _disc_clip(40, 100, 100, 10, seed=5)
    sink = []
    got = pt.track_frames(frames, target_width=10, start_location=("ij", (50, 50)), window_size=21, diagnostic=sink.append)
    assert got == [(int(p[0]), int(p[1])) for p in pos]
    assert len(sink) == len(frames) - 1                      # frames 2 ... n (:163-168); the bootstrap is not drawn
    ref = R.Diagnose(True)
    for k in range(1, len(frames)):
        assert np.array_equal(sink[k - 1], ref(frames[k], got[k])), k


def test_track_segments(pt, oracle):
    from oracle import synth
    from oracle.dog_oracle import OracleTracker
    tw, ws = 10, 21
    rng = np.random.default_rng(8)
    pos = np.clip(np.cumsum(rng.integers(-4, 5, (45, 2)), 0) + 50, 8, 92)
    segs, k = [], 0
    for h, w, n in ((100, 100, 20), (120, 160, 15), (100, 110, 10)):
        segs.append(np.stack([synth.disc_frame(h, w, (int(p[0]), int(p[1])), tw, True) for p in pos[k:k + n]]))
        k += n
    sink = []
    got = pt.track_segments(segs, [("ij", (50, 50)), None, None], target_width=tw, window_size=ws, diagnostic=sink.append)
    ref, end = [], (50, 50)
    for seg in segs:                                         # one OracleTracker loop per segment, started where the last ended
        ot = OracleTracker(seg[0], tw, (ws, ws), True, oracle)
        r = [ot(end)]
        for f in seg[1:]:
            ot.data[...] = f
            r.append(ot(r[-1]))
        ref += r
        end = r[-1]
    assert got == ref
    assert len(sink) == sum(len(s) - 1 for s in segs)
    d, j, k = R.Diagnose(True), 0, 0
    for seg in segs:
        for i in range(1, len(seg)):
            assert np.array_equal(sink[j], d(seg[i], got[k + i])), (j, k, i)
            j += 1
        k += len(seg)
    assert not np.array_equal(sink[19], R.Diagnose(True)(segs[1][1], got[21]))   # the trace ran on into segment 2


def test_bad_arguments(pt):
    import torch
    from pawsometracker_jl_amd import _lib
    L = pt.lib()
    E = _lib.PDOG_E_ARG
    h = C.c_void_p()
    assert L.pdog_diag_create(0, 1, None) == E
    assert L.pdog_diag_create(-1, 1, C.byref(h)) == E
    assert L.pdog_diag_create(1 << 20, 1, C.byref(h)) == E
    assert L.pdog_diag_create(0, 1, C.byref(h)) == 0
    frames = torch.from_numpy(_noise(2, 50, 60, seed=1)).cuda()
    ij = torch.tensor([[10, 10], [40, 50]], dtype=torch.int32, device="cuda")
    out = torch.empty((2, 360, 640), dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    base = dict(d=h, f=C.c_void_p(frames.data_ptr()), fs=3000, rs=60, fh=50, fw=60, n=2, p=C.c_void_p(ij.data_ptr()),
                o=C.c_void_p(out.data_ptr()))

    def render(**kw):
        a = dict(base, **kw)
        return L.pdog_diag_render(a["d"], s, a["f"], a["fs"], a["rs"], a["fh"], a["fw"], a["n"], a["p"], a["o"])

    for kw in (dict(d=None), dict(f=None), dict(p=None), dict(o=None), dict(fh=0), dict(fw=-1), dict(n=-1),
               dict(rs=59), dict(fs=-1)):
        assert render(**kw) == E, kw
        assert b"pdog_diag_render" in L.pdog_last_error()
    assert render(n=0, f=None, p=None, o=None) == 0          # nothing to do
    assert render() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), _ref(frames.cpu().numpy(), ij.cpu().numpy()))   # rejected calls left the trace alone
    assert L.pdog_diag_destroy(h) == 0
    assert L.pdog_diag_destroy(None) == 0
