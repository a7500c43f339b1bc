"""The overlay over a frame table and for several targets on the GPU (pdog_diag_render_indexed, Diagnose.render_indexed,
track_video(diagnostic=...), track_clips(diagnostic=...)): every buffer bit for bit against tests/overlay_restatement.py,
which builds on the restatement of src/diagnose.jl:26-38.  Frames are seeded noise, so a wrong frame shows; every target
walks from its own seed, so a swapped trace shows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diag_restatement as R  # noqa: E402
import overlay_restatement as OR  # noqa: E402

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
    """As in tests/test_gpu_diag.py: corners, points that scale to 0, a jump across the whole frame and repeated points first,
    then a random walk from the centre.  Walks of different seeds share the head and cross around the centre."""
    rng = np.random.default_rng(seed)
    out = [(1, 1), (h, w), (1, w), (h, 1), (2, 2), (h, w), (1, 1), (1, 1), (h // 2, w // 2)]
    p = np.array([h // 2, w // 2])
    while len(out) < n:
        p = np.clip(p + rng.integers(-step, step + 1, 2), 1, [h, w])
        out.append((int(p[0]), int(p[1])))
    return np.array(out[:n], np.int32)


def _walks(nt, n, h, w, seed, step=9):
    """[nt, n, 2]: target t walks from seed + 1000 t and skips the first t % 9 points of the head, so no two targets start alike."""
    return np.stack([_walk(n + t % 9, h, w, seed + 1000 * t, step)[t % 9:] for t in range(nt)]).astype(np.int32)


def _near(pos, want, tol=3):
    """Tracked positions follow the path they were started on (the overlay is checked bit for bit; this only tells the targets apart)."""
    return len(pos) == len(want) and all(abs(int(p[0]) - q[0]) <= tol and abs(int(p[1]) - q[1]) <= tol for p, q in zip(pos, want))


def _render(dia, frames, table, ij, out=None):
    return dia.render_indexed(frames, table, ij if hasattr(ij, "is_cuda") else _cuda(ij), out=out).cpu().numpy()


# ---- equivalence with the contiguous call ----
@pytest.mark.parametrize("h,w,n", [(100, 100, 12), (271, 481, 12), (1080, 1920, 9)])
def test_identity_table_one_target_is_the_contiguous_render(pt, h, w, n):
    frames, ij = _noise(n, h, w, seed=h + w), _walk(n, h, w, seed=h)
    F, P = _cuda(frames), _cuda(ij)
    want = R.Diagnose().render(list(frames), [tuple(p) for p in ij])
    with pt.Diagnose() as a, pt.Diagnose() as b:
        assert a.targets == 1
        got = _render(a, F, np.arange(n), P[None])
        plain = b(F, P).cpu().numpy()
    assert np.array_equal(got, plain) and np.array_equal(got, want)
    # the trace passes from __call__ to render_indexed and back: one restatement trace
    c = n // 3
    with pt.Diagnose() as dia:
        parts = [dia(F[:c], P[:c]).cpu().numpy(), _render(dia, F, np.arange(c, 2 * c), P[None, c:2 * c]),
                 dia(F[2 * c:], P[2 * c:]).cpu().numpy()]
    assert np.array_equal(np.concatenate(parts), want)


# ---- the table is honoured ----
TABLE9 = [3, 3, 0, 8, 5, 2, 7, 7, 1]          # repeats, skips, backward steps


def test_table_names_the_frame_of_every_output(pt):
    h, w = 271, 481
    frames, ij = _noise(9, h, w, seed=21), _walk(9, h, w, seed=22)
    pos = [tuple(p) for p in ij]
    want = R.Diagnose().render(list(frames[TABLE9]), pos)
    identity = R.Diagnose().render(list(frames), pos)
    assert all(not np.array_equal(want[k], identity[k]) for k in range(9) if TABLE9[k] != k)     # (not vacuous)
    assert np.array_equal(want, OR.Overlay(1).render(frames, TABLE9, ij[None]))
    with pt.Diagnose() as dia:
        assert np.array_equal(_render(dia, _cuda(frames), TABLE9, ij[None]), want)
    # the same on a strided, offset stack: rows 40 bytes wider, every second frame of a larger tensor
    big = _cuda(_noise(18, h + 5, w + 40, seed=7))
    view = big[::2, 3:3 + h, 17:17 + w]
    assert view.stride(1) == w + 40 and view.stride(0) == 2 * (h + 5) * (w + 40)
    host = view.cpu().numpy()
    want = R.Diagnose().render(list(host[TABLE9]), pos)
    assert not np.array_equal(want, R.Diagnose().render(list(host), pos))
    with pt.Diagnose() as dia:
        assert np.array_equal(_render(dia, view, TABLE9, ij[None]), want)


# ---- several targets ----
@pytest.mark.parametrize("nt", [1, 2, 3, 130])
def test_several_targets(pt, nt):
    h, w, n = 120, 200, 12
    frames = _noise(5, h, w, seed=nt)
    table = np.random.default_rng(nt).integers(0, 5, n)
    ij = _walks(nt, n, h, w, seed=nt, step=15)
    assert len({tuple(map(tuple, t)) for t in ij}) == nt
    with pt.Diagnose(False) as dia:
        dia.set_targets(nt)
        assert dia.targets == nt
        got = _render(dia, _cuda(frames), table, ij)
    assert np.array_equal(got, OR.Overlay(nt, False).render(frames, table, ij))


@pytest.fixture(scope="module")
def long_case():
    """3 targets over 250 steps on 120 x 200 frames, and the restatement's buffers: rendering is causal, so the first n of
    them are what n steps give — one reference for every length around the ring size and for the cut calls."""
    h, w, n = 120, 200, 250
    frames = _noise(6, h, w, seed=31)
    table = np.random.default_rng(32).integers(0, 6, n)
    ij = _walks(3, n, h, w, seed=33, step=6)
    return frames, table, ij, OR.Overlay(3).render(frames, table, ij)


@pytest.mark.parametrize("n", [99, 100, 101, 250])
def test_trace_length_around_the_ring(pt, long_case, n):
    frames, table, ij, want = long_case
    with pt.Diagnose() as dia:
        dia.set_targets(3)
        got = _render(dia, _cuda(frames), table[:n], np.ascontiguousarray(ij[:, :n]))
    assert np.array_equal(got, want[:n])


def test_cut_calls_equal_one_call(pt, long_case):
    frames, table, ij, want = long_case
    F, P = _cuda(frames), _cuda(ij)
    parts, k = [], 0
    with pt.Diagnose() as dia:
        dia.set_targets(3)
        for c in (1, 7, 100, 142):
            parts.append(_render(dia, F, table[k:k + c], P[:, k:k + c]))         # a column slice, as it lies
            k += c
    assert np.array_equal(np.concatenate(parts), want)


def test_column_slice_and_unaligned_output(pt):
    import torch
    h, w, nt, n = 120, 200, 3, 12
    frames = _noise(4, h, w, seed=41)
    table = [0, 3, 3, 1, 2, 0, 1, 1, 3, 2, 0, 2]
    wide = np.random.default_rng(42).integers(1, 120, (nt, 40, 2)).astype(np.int32)
    wide[:, 5:17] = _walks(nt, n, h, w, seed=43, step=15)
    P = _cuda(wide)[:, 5:17]
    assert P.stride(0) == 80 and not P.is_contiguous()
    buf = torch.empty(n * 360 * 640 + 1, dtype=torch.uint8, device="cuda")
    out = buf[1:].view(n, 360, 640)
    assert out.data_ptr() % 16 == 1
    with pt.Diagnose() as dia:
        dia.set_targets(nt)
        got = _render(dia, _cuda(frames), table, P, out=out)
    assert np.array_equal(got, OR.Overlay(nt).render(frames, table, wide[:, 5:17]))


# ---- handle state ----
def test_set_targets_empties_the_traces(pt):
    h, w, n = 120, 200, 10
    frames, table = _noise(3, h, w, seed=51), [0, 1, 2, 2, 1, 0, 0, 2, 1, 1]
    ij = _walks(2, n, h, w, seed=52)
    F, P = _cuda(frames), _cuda(ij)
    with pt.Diagnose() as fresh:
        fresh.set_targets(2)
        want = _render(fresh, F, table, P)
    assert np.array_equal(want, OR.Overlay(2).render(frames, table, ij))
    with pt.Diagnose() as dia:
        dia.set_targets(2)
        _render(dia, F, table, P)
        assert not np.array_equal(_render(dia, F, table, P), want)           # the traces ran on
        dia.set_targets(2)                                                    # the current number: emptied all the same
        assert np.array_equal(_render(dia, F, table, P), want)
        dia.set_targets(5)
        dia.set_targets(1)
        assert dia.targets == 1
        assert np.array_equal(dia(F[:3], P[0, :3]).cpu().numpy(), R.Diagnose().render(list(frames), [tuple(p) for p in ij[0, :3]]))
        for bad in (0, -1, 1025):
            with pytest.raises(ValueError):
                dia.set_targets(bad)
        assert pt.lib().pdog_diag_set_targets(dia._h, 1025) == pt._lib.PDOG_E_ARG and dia.targets == 1


def test_refused_calls_change_nothing(pt):
    import torch
    h, w, n = 120, 200, 6
    frames, table = _noise(4, h, w, seed=61), [1, 0, 3, 3, 2, 0]
    ij = _walks(2, n, h, w, seed=62)
    F, P = _cuda(frames), _cuda(ij)
    out = torch.full((n, 360, 640), 77, dtype=torch.uint8, device="cuda")
    E = pt._lib.PDOG_E_ARG
    with pt.Diagnose() as dia, pt.Diagnose() as clean:
        dia.set_targets(2)
        clean.set_targets(2)
        first = _render(dia, F, table, P)                                     # some trace to lose
        assert np.array_equal(first, _render(clean, F, table, P))
        for bad in ([1, 0, 4, 3, 2, 0], [1, 0, 3, 3, 2, -1]):                 # n_frames, -1
            with pytest.raises(pt.PdogError) as e:
                dia.render_indexed(F, bad, P, out=out)
            assert e.value.code == E and "pdog_diag_render_indexed" in str(e.value)
        with pytest.raises(pt.PdogError) as e:                                # three rows of positions for two targets
            dia.render_indexed(F, table, _cuda(_walks(3, n, h, w, seed=63)), out=out)
        assert e.value.code == E
        with pytest.raises(pt.PdogError) as e:                                # the contiguous call takes one row
            dia(F, P[0, :4])
        assert e.value.code == E and "pdog_diag_render" in str(e.value)
        torch.cuda.synchronize()
        assert bool((out == 77).all())                                        # nothing was launched
        got = _render(dia, F, table, P, out=out)
        assert np.array_equal(got, _render(clean, F, table, P))               # and the traces are what they were
    ref = OR.Overlay(2)
    ref.render(frames, table, ij)
    assert np.array_equal(got, ref.render(frames, table, ij))


# ---- behind the chains, on the same stream ----
def _two_discs(n, h, w, tw, bkgd=128):
    """n frames with two dark discs on separate paths (never closer than 40 pixels), and the paths."""
    from oracle import synth
    paths = [[(20 + k // 3, 20 + k) for k in range(n)], [(82 - k // 4, 85 - k) for k in range(n)]]
    frames = np.stack([np.minimum(synth.disc_frame(h, w, paths[0][k], tw, True, bkgd), synth.disc_frame(h, w, paths[1][k], tw, True, bkgd))
                       for k in range(n)])
    return frames, paths


def test_after_indexed_chains_without_sync(pt):
    tw, h, w = 10, 100, 100
    frames, paths = _two_discs(40, h, w, tw)
    table = pt.fps_table(30, 40, 0, pt.DEFAULT_STOP, 24)
    F = _cuda(frames)
    bt = pt.BatchTracker(h, w, tw, (21, 21), True, pt.mode(frames[0]))
    with pt.Diagnose() as dia:
        dia.set_targets(2)
        ij = bt.detect_chains_indexed(F, np.tile(table, (2, 1)), _cuda(np.array([paths[0][0], paths[1][0]], np.int32)))
        got = dia.render_indexed(F, table, ij).cpu().numpy()      # same stream, no host synchronisation in between
    bt.close()
    ij = ij.cpu().numpy()
    assert _near(ij[0], [paths[0][i] for i in table]) and _near(ij[1], [paths[1][i] for i in table])
    assert np.array_equal(got, OR.Overlay(2).render(frames, table, ij))


# ---- the top-level calls ----
def test_track_video_diagnostic(pt):
    import torch
    tw, h, w, nf = 10, 100, 100, 60
    frames, paths = _two_discs(nf, h, w, tw)
    F = _cuda(frames)
    locs = [("ij", paths[0][0]), ("ij", paths[1][0])]
    kw = dict(rate=30, fps=24, target_width=tw, window_size=21, start_locations=locs)
    sink = []
    ts, idx = pt.track_video(F, **kw, diagnostic=lambda k0, ov: sink.append((k0, ov.cpu().numpy())), diagnostic_chunk=7)
    table = pt.fps_table(30, nf, 0, pt.DEFAULT_STOP, 24)
    m = len(table)
    assert m == 48 and idx.shape == (2, m, 2) and len(ts) == m
    assert [k0 for k0, _ in sink] == list(range(1, m, 7)) and all(len(ov) == min(7, m - k0) for k0, ov in sink)
    got = np.concatenate([ov for _, ov in sink])
    assert got.shape == (m - 1, 360, 640)                                    # the bootstrap frame is not drawn
    pos = idx.cpu().numpy()
    assert _near(pos[0], [paths[0][i] for i in table]) and _near(pos[1], [paths[1][i] for i in table])
    assert np.array_equal(got, OR.Overlay(2).render(frames, table[1:], pos[:, 1:]))
    ts0, idx0 = pt.track_video(F, **kw)
    assert np.array_equal(ts, ts0) and torch.equal(idx, idx0)


def _clips(lens, nf, h, w, tw, bkgds):
    """[n_clips, nf, h, w]: clip c holds one disc on a path of its own over background bkgds[c]; frames beyond its length are noise."""
    from oracle import synth
    frames = _noise(len(lens) * nf, h, w, seed=71).reshape(len(lens), nf, h, w)
    paths = []
    for c, n in enumerate(lens):
        paths.append([(30 + 10 * c + k, 40 + 2 * k - 3 * c) for k in range(n)])
        for k in range(n):
            synth.disc_frame(h, w, paths[c][k], tw, True, bkgds[c], out=frames[c, k])
    return frames, paths


@pytest.mark.parametrize("lens,drawn", [((12, 1, 5), [0, 2]), ((12, 1, 5, 0), [0, 2, 3])])
def test_track_clips_diagnostic(pt, lens, drawn):
    import torch
    tw, h, w, nf = 10, 100, 100, 12
    frames, paths = _clips(lens, nf, h, w, tw, (128, 90, 160, 200))
    F = _cuda(frames)
    kw = dict(target_width=tw, window_size=21, lengths=list(lens),
              start_locations=[("ij", p[0]) if p else ("ij", (50, 50)) for p in paths])
    sink = []
    idx = pt.track_clips(F, **kw, diagnostic=lambda c, k0, ov: sink.append((c, k0, ov.cpu().numpy())), diagnostic_clips=drawn,
                         diagnostic_chunk=4)
    assert torch.equal(idx, pt.track_clips(F, **kw))
    pos = idx.cpu().numpy()
    assert {c for c, _, _ in sink} == {0, 2}                                 # nothing for a clip shorter than two frames
    for c in (0, 2):
        assert _near(pos[c, :lens[c]], paths[c])
        calls = [(k0, ov) for cc, k0, ov in sink if cc == c]
        assert [k0 for k0, _ in calls] == list(range(1, lens[c], 4))
        got = np.concatenate([ov for _, ov in calls])
        assert got.shape[0] == lens[c] - 1                                   # 11 and 4
        # a fresh trace per clip: each equals a restatement of its own
        assert np.array_equal(got, OR.Overlay(1).render(frames[c], np.arange(1, lens[c]), pos[c:c + 1, 1:lens[c]]))
    assert [c for c, _, _ in sink] == sorted(c for c, _, _ in sink)          # clip by clip, in the order asked for
