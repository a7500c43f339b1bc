"""The Python binding's own duties (no kernel of its own): a wrong argument is refused before anything reaches the library,
and every handle class closes once, as a context manager too, and refuses work afterwards.  One geometry throughout:
four 120 x 160 frames, target width 10 (l = 29), window (21, 33)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W, TW, WS, RADII, N = 120, 160, 10, (21, 33), (10, 16), 4


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    return m


@pytest.fixture(scope="module")
def case(oracle):
    """Frames, guesses, the fill and the oracle's positions."""
    from oracle import synth
    frames, guesses, _ = synth.make_batch(N, H, W, TW, RADII, True, seed=12, noise=3)
    fill = oracle.mode_u8(frames[0])
    ref = oracle.detect_batch(frames, fill, oracle.dog_kernel(oracle.sigma(TW), True), RADII, guesses)
    return frames, guesses, fill, ref


def test_rejection_leaves_the_handle_healthy(pt, case):
    import torch
    frames_h, guesses_h, fill, ref = case
    frames, guesses = torch.from_numpy(frames_h).cuda(), torch.from_numpy(guesses_h).cuda()
    clips = frames.view(2, 2, H, W)
    starts = guesses[:2].contiguous()
    wider = torch.zeros((N, H, W + 1), dtype=torch.uint8, device="cuda")
    every_other = torch.zeros((N, H, 2 * W), dtype=torch.uint8, device="cuda")[:, :, ::2]
    fi = torch.arange(N, dtype=torch.int32, device="cuda")
    bt = pt.BatchTracker(H, W, TW, WS, True, fill)
    dia = pt.Diagnose(True)
    bad = [
        (TypeError, lambda: bt.detect(frames.cpu(), guesses)),
        (TypeError, lambda: bt.detect(frames, guesses.cpu())),
        (ValueError, lambda: bt.detect(frames, torch.ones((N, 4), dtype=torch.int32, device="cuda")[:, :2])),
        (ValueError, lambda: bt.detect(frames, guesses, frame_index=fi[:3])),
        (ValueError, lambda: bt.detect_host(frames_h[:, :, :W - 1], guesses_h)),
        (ValueError, lambda: bt.detect_chain(wider, (60, 80))),
        (TypeError, lambda: bt.detect_chain_progress(frames.float(), (60, 80))),
        (ValueError, lambda: bt.detect_chain_progress(wider, (60, 80))),
        (TypeError, lambda: bt.detect_chains(frames, starts)),
        (ValueError, lambda: bt.detect_chains(wider.view(2, 2, H, W + 1), starts)),
        (ValueError, lambda: bt.detect_chains(clips[:, :1], starts)),
        (TypeError, lambda: bt.measure(frames, guesses.long())),
        (ValueError, lambda: bt.measure(frames, guesses, frame_index=fi[:2])),
        (ValueError, lambda: bt.clip_modes(every_other)),
        (TypeError, lambda: bt.clip_modes(frames, fi.long())),
        (ValueError, lambda: bt.clip_modes(frames, out=torch.empty(N + 1, dtype=torch.int32, device="cuda"))),
        (ValueError, lambda: bt.track_clips(clips, guesses)),
        (ValueError, lambda: bt.track_clips(clips, starts, fills=[fill])),
        (ValueError, lambda: bt.track_clips(clips, starts, lengths=np.array([[2, 2]]))),
        (TypeError, lambda: dia(frames, guesses.cpu())),
        (ValueError, lambda: dia(frames, guesses[:3].contiguous())),
        (ValueError, lambda: dia(frames, guesses, out=torch.empty((N, 360, 641), dtype=torch.uint8, device="cuda"))),
        (TypeError, lambda: pt.mode_device(frames_h[0])),
    ]
    for k, (exc, call) in enumerate(bad):
        with pytest.raises(exc) as e:
            call()
        assert type(e.value) is exc, (k, e.value)
    bt.sync()                                          # nothing was queued, nothing raised a flag
    assert bt.clips_counters() == (0, 0, 0, 0)
    out = bt.detect(frames, guesses)
    bt.sync()
    assert np.array_equal(out.cpu().numpy(), ref)
    assert dia(frames, out).shape == (N, 360, 640)     # Diagnose takes any frame size, by design
    assert dia(wider, out).shape == (N, 360, 640)
    torch.cuda.synchronize()
    dia.close()
    bt.close()


def _make(pt, name, case):
    frames, _, fill, _ = case
    if name == "Tracker":
        return pt.Tracker(frames[0], TW, WS, True)
    if name == "BatchTracker":
        return pt.BatchTracker(H, W, TW, WS, True, fill)
    if name == "GroupTracker":
        return pt.GroupTracker([0], H, W, TW, WS, True, fill)
    return pt.Diagnose(True)


@pytest.mark.parametrize("name", ["Tracker", "BatchTracker", "GroupTracker", "Diagnose"])
def test_close_twice_context_manager_and_use_after_close(pt, case, name):
    import torch
    frames_h, guesses_h, fill, ref = case
    frames, guesses = torch.from_numpy(frames_h).cuda(), torch.from_numpy(guesses_h).cuda()
    out = torch.empty((N, 2), dtype=torch.int32, device="cuda")
    use = {"Tracker": [lambda o: o((60, 80)), lambda o: o.info(), lambda o: o.measure((60, 80))],
           "BatchTracker": [lambda o: o.detect(frames, guesses), lambda o: o.sync(), lambda o: o.clip_modes(frames),
                            lambda o: o.detect_chain(frames, (60, 80)), lambda o: o.measure(frames, guesses)],
           "GroupTracker": [lambda o: o.detect([frames], [guesses], N, out), lambda o: o.sync(), lambda o: o.info()],
           "Diagnose": [lambda o: o(frames, guesses)]}[name]
    with _make(pt, name, case) as obj:
        assert obj._h
        if name == "BatchTracker":
            got = obj.detect(frames, guesses)
            obj.sync()
            assert np.array_equal(got.cpu().numpy(), ref)
    assert obj._h is None                              # closed on the way out
    obj.close()                                        # and closing again is harmless
    obj = _make(pt, name, case)
    obj.close()
    obj.close()
    assert obj._h is None
    for k, call in enumerate(use):                     # a null handle: refused by the library before it launches anything
        with pytest.raises((pt.PdogError, ValueError)):
            call(obj)
    torch.cuda.synchronize()


def test_clips_handle_is_closed_before_the_tracker_it_borrows(pt, case, monkeypatch):
    import torch
    frames_h, _, fill, _ = case
    frames = torch.from_numpy(frames_h).cuda()
    L = pt.lib()
    calls = []

    def recorded(name):
        real = getattr(L, name)

        def wrapper(h):
            calls.append((name, h.value))
            return real(h)
        monkeypatch.setattr(L, name, wrapper)

    recorded("pdog_clips_destroy")
    recorded("pdog_destroy")
    with pt.BatchTracker(H, W, TW, WS, True, fill) as bt:
        modes = bt.clip_modes(frames)
        bt.sync()
        tracker, clips = bt._h.value, bt._clips_handle().value
    assert modes.cpu().tolist() == [pt.mode(f) for f in frames_h]
    assert calls == [("pdog_clips_destroy", clips), ("pdog_destroy", tracker)]
    bt.close()
    del calls[:]
    pt.BatchTracker(H, W, TW, WS, True, fill).close()          # no clips handle was ever made: one call
    assert [name for name, _ in calls] == ["pdog_destroy"]
