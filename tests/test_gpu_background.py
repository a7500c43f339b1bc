"""The background model on the GPU (include/pawsome_background.h).  Every comparison is exact.

The model and the subtracted frames are held byte for byte to tests/background_restatement.py over frame widths 1, 3, 5, 67 and
160 (below a dword, below a 16-byte piece, no multiple of either, several blocks), heights 1 and 7, row strides with poisoned
slack, stacks whose base is 0 ... 3 bytes off, K = 1, 2, 3, 4, 5, 63 and 64 and both sides of every tier of the kernel (8 | 9,
16 | 17, 32 | 33), sample lists with duplicates, and constant, 0 / 255 alternating and random contents; a poisoned frame lies
right behind every stack.  The
subtraction also meets both saturations, a table with repeats in reversed order and output strides whose poisoned slack must
survive.  Every refusal leaves the model as it was.  track_video(background=...) on the clutter scene of
tests/background_scenes.py equals the restatement's chunk-free flow over the Float64 oracle position for position and state for
state — plain, predicted, exclusive and with the motion model — for chunks of 1, 7 and 60 steps.  The whole file fails on a
library without the symbols."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import background_restatement as BR  # noqa: E402
import background_scenes as BS  # noqa: E402

pytestmark = pytest.mark.gpu
POISON, SENTINEL = 0xA5, 0x5A
WIDTHS, HEIGHTS, KS = (1, 3, 5, 67, 160), (1, 7), (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64)
NF = 66


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    assert hasattr(m.lib(), "pdog_bg_estimate") and hasattr(m, "Background")
    return m


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _contents(kind, rng, n, h, w):
    if kind == "constant":
        return np.full((n, h, w), int(rng.integers(0, 256)), np.uint8)
    if kind == "alternating":                      # 0 / 255 in time, the phase per pixel
        return (((np.arange(n)[:, None, None] + rng.integers(0, 2, (h, w))[None]) % 2) * 255).astype(np.uint8)
    return rng.integers(0, 256, (n, h, w), dtype=np.uint8)


def _strided(host, off, row_slack, frame_slack, fill=POISON, tail=0):
    """host [n, h, w] laid into a poisoned flat buffer: base `off` bytes in, rows w + row_slack apart, frames frame_slack bytes
    further apart than they need; `tail` further frames' room behind them holds SENTINEL.  Returns (flat host copy, cuda view)."""
    import torch
    n, h, w = host.shape
    rs = w + row_slack
    fs = h * rs + frame_slack
    flat = np.full(off + (n + tail) * fs + 16, fill, np.uint8)
    flat[off + n * fs:off + (n + tail) * fs] = SENTINEL
    view = np.lib.stride_tricks.as_strided(flat[off:], (n, h, w), (fs, rs, 1))
    view[...] = host
    d_flat = torch.from_numpy(flat).cuda()
    return flat, d_flat, d_flat.as_strided((n, h, w), (fs, rs, 1), off)


def _sample_lists(rng, k):
    """Two lists per K: distinct frames in random order, and one with duplicates (for K >= 2)."""
    lists = [rng.permutation(NF)[:k].tolist()]
    if k >= 2:
        lists.append(rng.integers(0, max(2, k // 2), k).tolist())
    return lists


# ---- the median ----
@pytest.mark.parametrize("kind", ["constant", "alternating", "random"])
def test_estimate_equals_the_restatement(pt, kind):
    rng = np.random.default_rng(20261020)
    n_checked = 0
    for h in HEIGHTS:
        for w in WIDTHS:
            host = _contents(kind, rng, NF, h, w)
            with pt.Background(h, w) as bg:
                for off in range(4):
                    _, _, d_frames = _strided(host, off, row_slack=1 + off, frame_slack=off, tail=1)
                    assert d_frames.data_ptr() % 4 == off and d_frames.stride(1) > w
                    for k in KS:
                        for s in _sample_lists(rng, k):
                            got = bg.estimate(d_frames, s).image().cpu().numpy()
                            assert np.array_equal(got, BR.median(host, s)), (kind, h, w, off, k, s)
                            n_checked += 1
    assert n_checked == 2 * 5 * 4 * (2 * len(KS) - 1)


def test_estimate_on_a_dense_stack_and_more_than_one_block(pt):
    """Frames as torch lays them (row stride = w, odd: rows at every alignment), enough dwords for several blocks, every K."""
    rng = np.random.default_rng(3)
    h, w = 37, 67
    host = rng.integers(0, 256, (NF, h, w), dtype=np.uint8)
    host[:, :, 10:20] = rng.integers(100, 104, (NF, h, 10), dtype=np.uint8)          # ties everywhere
    d_frames = _cuda(host)
    with pt.Background(h, w) as bg:
        for k in range(1, 65):
            s = rng.integers(0, NF, k).tolist()
            assert np.array_equal(bg.estimate(d_frames, s).image().cpu().numpy(), BR.median(host, s)), k


# ---- the subtraction ----
def _saturating_pair(h, w):
    """A frame and a model whose differences run through -255, -129, -128, 0, 127, 128 and 255, pixel after pixel."""
    pairs = np.array([(0, 255), (0, 129), (0, 128), (77, 77), (127, 0), (128, 0), (255, 0)], np.uint8)
    idx = np.arange(h * w).reshape(h, w) % len(pairs)
    return pairs[idx, 0], pairs[idx, 1]


def test_subtract_equals_the_restatement(pt):
    rng = np.random.default_rng(20261021)
    n = 6
    table = list(range(n - 1, -1, -1)) + [0, 3, 3]                  # reversed, with repeats
    for h in HEIGHTS:
        for w in WIDTHS:
            host = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
            host[0], model = _saturating_pair(h, w)
            want = BR.subtract(host[table], model)
            assert {0, 128, 255} <= set(want[table.index(0)].ravel().tolist()) or h * w < 7
            with pt.Background(h, w) as bg:
                for off in range(4):
                    _, _, d_frames = _strided(host, off, row_slack=2 + off, frame_slack=3, tail=1)
                    _, _, d_model = _strided(model[None], (off + 1) % 4, row_slack=5, frame_slack=0)
                    bg.set(d_model[0])
                    assert np.array_equal(bg.image().cpu().numpy(), model), (h, w, off)               # set / get round trip
                    o_flat, d_oflat, d_out = _strided(np.zeros((len(table), h, w), np.uint8), (off + 2) % 4, row_slack=5, frame_slack=9)
                    assert bg.subtract(d_frames, table, out=d_out) is d_out
                    np.lib.stride_tricks.as_strided(o_flat[(off + 2) % 4:], want.shape, tuple(d_out.stride()))[...] = want
                    assert np.array_equal(d_oflat.cpu().numpy(), o_flat), (h, w, off)                 # the outputs, and the poison around them
                    assert np.array_equal(bg.subtract(d_frames, table).cpu().numpy(), want)           # a fresh, dense out
    # a model from an estimate, frames of several blocks, the identity table
    h, w = 37, 67
    host = rng.integers(0, 256, (9, h, w), dtype=np.uint8)
    with pt.Background(h, w) as bg:
        d = _cuda(host)
        got = bg.estimate(d, range(9)).subtract(d, range(9)).cpu().numpy()
        assert np.array_equal(got, BR.subtract(host, BR.median(host, range(9))))
        assert bg.subtract(d, []).shape == (0, h, w)


# ---- refusals ----
def test_refusals_leave_the_model_unchanged(pt):
    from pawsometracker_jl_amd import _lib
    L = pt.lib()
    rng = np.random.default_rng(5)
    h, w, n = 7, 67, 5
    host = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    d_frames = _cuda(host)
    d_out = _cuda(np.full((2, h, w), POISON, np.uint8))
    F, O = C.c_void_p(d_frames.data_ptr()), C.c_void_p(d_out.data_ptr())
    keep = []

    def T(*v):
        keep.append(np.array(v, np.int32))
        return C.c_void_p(keep[-1].ctypes.data)
    with pt.Background(h, w) as bg:
        H = bg._h
        # before any model: nothing to subtract, nothing to hand out
        assert L.pdog_bg_subtract_indexed(H, None, F, h * w, w, n, T(0), 1, O, h * w, w) == _lib.PDOG_E_ARG
        assert L.pdog_bg_get(H, None, O, w) == _lib.PDOG_E_ARG
        with pytest.raises(pt.PdogError):
            bg.image()
        assert (d_out.cpu().numpy() == POISON).all()
        before = bg.estimate(d_frames, [0, 1, 2]).image().cpu().numpy()
        assert np.array_equal(before, BR.median(host, [0, 1, 2]))
        many = T(*([0] * 65))
        refused = [
            lambda: L.pdog_bg_estimate(H, None, None, h * w, w, n, T(0), 1),
            lambda: L.pdog_bg_estimate(H, None, F, h * w, w, n, None, 1),
            lambda: L.pdog_bg_estimate(H, None, F, h * w, w, n, T(0, n), 2),            # an entry past the stack
            lambda: L.pdog_bg_estimate(H, None, F, h * w, w, n, T(3, -1, 0), 3),        # a negative entry
            lambda: L.pdog_bg_estimate(H, None, F, h * w, w, n, T(0), 0),
            lambda: L.pdog_bg_estimate(H, None, F, h * w, w, n, many, 65),
            lambda: L.pdog_bg_estimate(H, None, F, h * w, w - 1, n, T(0), 1),
            lambda: L.pdog_bg_estimate(H, None, F, -1, w, n, T(0), 1),
            lambda: L.pdog_bg_estimate(H, None, F, h * w, w, 0, T(0), 1),
            lambda: L.pdog_bg_set(H, None, None, w),
            lambda: L.pdog_bg_set(H, None, F, w - 1),
            lambda: L.pdog_bg_get(H, None, None, w),
            lambda: L.pdog_bg_get(H, None, O, w - 1),
            lambda: L.pdog_bg_subtract_indexed(H, None, None, h * w, w, n, T(0), 1, O, h * w, w),
            lambda: L.pdog_bg_subtract_indexed(H, None, F, h * w, w, n, None, 1, O, h * w, w),
            lambda: L.pdog_bg_subtract_indexed(H, None, F, h * w, w, n, T(0), 1, None, h * w, w),
            lambda: L.pdog_bg_subtract_indexed(H, None, F, h * w, w, n, T(0, n), 2, O, h * w, w),
            lambda: L.pdog_bg_subtract_indexed(H, None, F, h * w, w, n, T(0, -1), 2, O, h * w, w),    # no negative entries: no early end
            lambda: L.pdog_bg_subtract_indexed(H, None, F, h * w, w - 1, n, T(0), 1, O, h * w, w),
            lambda: L.pdog_bg_subtract_indexed(H, None, F, -1, w, n, T(0), 1, O, h * w, w),
            lambda: L.pdog_bg_subtract_indexed(H, None, F, h * w, w, n, T(0), 1, O, h * w, w - 1),
            lambda: L.pdog_bg_subtract_indexed(H, None, F, h * w, w, n, T(0, 1), 2, O, -1, w),
            lambda: L.pdog_bg_subtract_indexed(H, None, F, h * w, w, n, T(0), -1, O, h * w, w),
        ]
        for k, call in enumerate(refused):
            assert call() == _lib.PDOG_E_ARG, k
            assert L.pdog_last_error().startswith(b"pdog_bg_"), k
        import torch
        torch.cuda.synchronize()
        assert np.array_equal(bg.image().cpu().numpy(), before) and (d_out.cpu().numpy() == POISON).all()
        # the binding's own: a wrong frame size, a host tensor, too many samples
        with pytest.raises(ValueError):
            bg.estimate(d_frames[:, :, :60], [0])
        with pytest.raises(TypeError):
            bg.estimate(d_frames.cpu(), [0])
        with pytest.raises(ValueError):
            bg.estimate(d_frames, [0] * 65)
        with pytest.raises(ValueError):
            bg.subtract(d_frames, [0, 1, 2], out=d_out)
        with pytest.raises(pt.PdogError):
            bg.subtract(d_frames, [0, n])
        assert np.array_equal(bg.image().cpu().numpy(), before)
        assert np.array_equal(bg.subtract(d_frames, [4]).cpu().numpy(), BR.subtract(host[[4]], before))      # and it works afterwards
    bg.close()                                                                                              # closes once


# ---- track_video on the scene ----
@pytest.fixture(scope="module")
def oracle():
    from oracle.dog_oracle import Oracle
    return Oracle()


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(darker=True, second=False):
        if (darker, second) not in made:
            sc = BS.scene(darker, second)
            made[(darker, second)] = (sc, _cuda(sc.frames))
        return made[(darker, second)]
    return get


def _args(sc, **kw):
    return dict(rate=24, start=0, stop=sc.nf / 24, fps=24, target_width=sc.tw, window_size=sc.ws, darker_target=sc.darker,
                start_locations=[("ij", s) for s in sc.starts], **kw)


@pytest.mark.parametrize("loop", ["plain", "predict", "motion", "exclusive"])
def test_track_video_equals_the_flow_over_the_oracle(pt, oracle, scenes, loop):
    import torch
    two = loop in ("motion", "exclusive")
    sc, d_frames = scenes(True, two)
    K = 9
    want, want_state, sub, fill = BR.track_video(oracle, sc.frames, range(sc.nf), K, sc.tw, sc.ws, sc.darker, sc.starts, loop)
    kw = {} if loop == "plain" else {loop: True}
    first = None
    for chunk in (1, 7, 60, None):
        res = pt.track_video(d_frames, background=K, **({} if chunk is None else {"background_chunk": chunk}), **_args(sc, **kw))
        assert len(res) == (2 if loop == "plain" else 3) and len(res[0]) == sc.nf
        assert np.array_equal(res[1].cpu().numpy(), want), (loop, chunk)
        if loop != "plain":
            assert np.array_equal(res[2].cpu().numpy(), want_state), (loop, chunk)
        first = first or res
        assert torch.equal(res[1], first[1]) and np.array_equal(res[0], first[0])
    # the chain stays on its animal
    for t in range(len(sc.starts)):
        assert max(BS.errors([tuple(p) for p in want[t]], sc.truth[t])) <= 3
    # the model handed in as an image is the model estimated
    image = _cuda(BR.median(sc.frames, BR.samples(range(sc.nf), K)))
    res = pt.track_video(d_frames, background=image, background_chunk=7, **_args(sc, **kw))
    assert all(torch.equal(a, b) for a, b in zip(res[1:], first[1:]))


def test_track_video_bright_twin_and_a_table_that_skips_frames(pt, oracle, scenes):
    sc, d_frames = scenes(False, False)
    K, k0 = 15, 10
    table = pt.fps_table(24, sc.nf, k0 / 24, sc.nf / 24, 24)
    assert table.tolist() == list(range(k0, sc.nf))
    want, _, _, _ = BR.track_video(oracle, sc.frames, table, K, sc.tw, sc.ws, False, [sc.truth[0][k0]])
    args = _args(sc)
    args.update(start=k0 / 24, start_locations=("ij", sc.truth[0][k0]))
    for chunk in (7, 256):
        ts, idx = pt.track_video(d_frames, background=K, background_chunk=chunk, **args)
        assert np.array_equal(idx.cpu().numpy(), want), chunk
    assert max(BS.errors([tuple(p) for p in want[0]], sc.truth[0][k0:])) <= 3


def test_plain_chain_on_the_gpu_is_lost_without_the_model(pt, scenes):
    sc, d_frames = scenes(True, False)
    ts, idx = pt.track_video(d_frames, **_args(sc))
    err = BS.errors([tuple(p) for p in idx[0].cpu().numpy()], sc.truth[0])
    assert sum(e > 3 for e in err) >= 20 and err[-1] > 20
    ts2, idx2 = pt.track_video(d_frames, background=None, **_args(sc))          # background=None: the call without the keyword
    import torch
    assert torch.equal(idx, idx2) and np.array_equal(ts, ts2)


def test_subpixel_and_overlay_with_the_model(pt, oracle, scenes):
    import torch
    sc, d_frames = scenes(True, True)
    K = 9
    seen = []
    ts, idx, sub = pt.track_video(d_frames, background=K, background_chunk=7, subpixel=True, diagnostic_chunk=16,
                                  diagnostic=lambda k0, ov: seen.append((k0, ov.clone())), **_args(sc))
    ts2, idx2 = pt.track_video(d_frames, background=K, **_args(sc))
    assert torch.equal(idx, idx2) and sub.shape == (2, sc.nf, 2) and sub.dtype == torch.float64
    # subpixel: measure at the positions, on the subtracted frames under their fill
    d_sub = _cuda(BR.subtract(sc.frames, BR.median(sc.frames, BR.samples(range(sc.nf), K))))
    with pt.BatchTracker(*sc.hw, sc.tw, (sc.ws, sc.ws), sc.darker, oracle.mode_u8(d_sub[0].cpu().numpy())) as bt:
        fi = torch.arange(sc.nf, dtype=torch.int32, device="cuda").repeat(2)
        want = bt.measure(d_sub, idx.reshape(-1, 2).contiguous(), fi).view(2, sc.nf, 2)
        bt.sync()
    assert torch.equal(sub, want)
    # the overlay: the original frames under the same positions, through the table path
    assert [k0 for k0, _ in seen] == list(range(1, sc.nf, 16))
    with pt.Diagnose(sc.darker) as dia:
        dia.set_targets(2)
        want = dia.render_indexed(d_frames, np.arange(1, sc.nf), idx[:, 1:])
    assert torch.equal(torch.cat([ov for _, ov in seen]), want)
