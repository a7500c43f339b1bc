"""What a caller can observe of the tracker's plan (make_plan, csrc/pdog_plan.hpp, as pawsome_dog.hip applies it):
pdog_get_info, pdog_get_exact's state and threshold and pdog_kernel_for_batch, plain and after sequences of pdog_set_variant / pdog_set_tuning calls, compared with
tests/golden/dispatch_paths.json.  That file was recorded ONCE by record() below from the library of the commit BEFORE the
plan became one function (selected with PAWSOME_DOG_LIB; the file's header names the commit): this is a characterisation
test, the recording is the reference and is not re-recorded to make a change pass.  Trackers are created and asked questions;
only the last two tests launch anything."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "dispatch_paths.json")

from dispatch_cases import BATCHES, CASES, SEQUENCES  # shared with tests/test_plan_cpu.py, which replays them on the host


@pytest.fixture(scope="module")
def pt():
    import pawsometracker_jl_amd as m
    return m


def _snapshot(bt, status):
    """[status of the call before, variant, n_strips, strip_w, exact on, threshold, [path per batch size]]"""
    i = bt.info()
    on, thr, _ = bt.exact_stats()
    return [status, i.variant, i.n_strips, i.strip_w, on, thr, [bt.kernel_for_batch(n) for n in BATCHES]]


def _clear_hip_last_error():
    """The HIP call a refused pdog_create failed in stays the thread's last error, and the next checked launch of torch (any
    later test's) would report it: read it, which clears it."""
    import ctypes
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64.so" in line)
    ctypes.CDLL(path).hipGetLastError()


def _observe(pt, case):
    """{sequence: [snapshot after creation, snapshot after each call]} — a rejected call is its status code, and the state after
    it; a rejected pdog_create is [[status]]."""
    fh, fw, tw, ws = CASES[case]
    out = {}
    for name, calls in SEQUENCES.items():
        try:
            bt = pt.BatchTracker(fh, fw, tw, ws, True, 128)
        except pt.PdogError as e:
            out[name] = [[e.code]]
            _clear_hip_last_error()
            continue
        snaps = [_snapshot(bt, 0)]
        for call in calls:
            status = 0
            try:
                getattr(bt, call[0])(*call[1:])
            except pt.PdogError as e:
                status = e.code
            snaps.append(_snapshot(bt, status))
        bt.close()
        out[name] = snaps
    return out


def record():
    """PAWSOME_DOG_LIB=<the parent commit's libpawsome_dog.so> PAWSOME_DISPATCH_PARENT=<its commit> python tests/test_gpu_dispatch.py"""
    import sys
    sys.path.insert(0, ROOT)
    import pawsometracker_jl_amd as m
    doc = {"recorded_by": "tests/test_gpu_dispatch.py::record", "library_of_commit": os.environ["PAWSOME_DISPATCH_PARENT"],
           "snapshot": "[status, variant, n_strips, strip_w, exact, threshold, paths]", "batches": BATCHES,
           "cases": {case: _observe(m, case) for case in CASES}}
    with open(FIXTURE, "w") as f:
        f.write(json.dumps(doc, separators=(",", ":")).replace('"cases":{', '"cases":{\n').replace("]]],", "]]],\n").replace("]]]},", "]]]},\n") + "\n")
    print("recorded", FIXTURE, "from", m.LIB_PATH)


@pytest.fixture(scope="module")
def recording():
    with open(FIXTURE) as f:
        doc = json.load(f)
    assert doc["batches"] == BATCHES and sorted(doc["cases"]) == sorted(CASES)
    return doc["cases"]


@pytest.mark.parametrize("case", sorted(CASES))
def test_observable_plan_equals_the_recording(pt, recording, case):
    got = _observe(pt, case)
    for name in SEQUENCES:
        assert got[name] == recording[case][name], (case, name)


def test_recording_reaches_every_path_and_threshold(recording):
    """The recording holds every path id and, for each threshold of path_for_batch, a batch size on either side."""
    plain = {case: dict(zip(BATCHES, seqs["variants"][0][6])) for case, seqs in recording.items() if len(seqs["variants"][0]) > 1}
    seen = {p for seqs in recording.values() for snaps in seqs.values() for s in snaps if len(s) > 1 for p in s[6]}
    assert {300, 400, 200} <= seen
    assert any(100 <= p < 300 and p != 200 for p in seen), "no roll id"
    assert any(p < 100 for p in seen), "no ring id"
    assert plain["15x15_l153"][256] == 300 and plain["15x15_l153"][257] == 200            # two-pass trackers: n <= 256
    assert plain["63x63_l65"][1024] == 300 and plain["63x63_l65"][1200] == 100            # n * strips < 1200 …
    assert plain["257x257_l65"][17] == 200 and plain["257x257_l65"][256] == 100           # … with five strip-waves per window
    assert plain["45x45_l65"][4096] == 300 and plain["63x63_l65"][4096] == 100            # windows below 3000 pixels
    assert plain["257x257_l65"][2] == 400 and plain["257x257_l65"][3] == 200              # the tiled kernel: n <= 2
    assert any(s[0] != 0 for seqs in recording.values() for snaps in seqs.values() for s in snaps), "no rejected call recorded"
    # the window too tall for exact mode: the recorded library refuses to create it (PDOG_E_HIP: the finishing kernel's LDS limit
    # is raised for the refinement's block whether exact mode is on or not, and that block is beyond the device's LDS)
    assert recording["9801x45_l29"]["variants"] == [[2]]


def test_fused_plan_in_both_layouts_equals_oracle(pt, oracle):
    """8 windows of 45×45 through the fused kernel as launch_fused copies its plan: the compile-time-l layout, the runtime-l
    layout ("no_fused_c") and the compile-time-l layout again after the switch went back."""
    import torch
    from oracle import synth
    tw, radii = 25, (22, 22)
    frames, guesses, _ = synth.make_batch(8, 240, 320, tw, radii, True, seed=5, noise=3)
    fill = oracle.mode_u8(frames[0])
    ref = oracle.detect_batch(frames, fill, oracle.dog_kernel(oracle.sigma(tw), True), radii, guesses)
    bt = pt.BatchTracker(240, 320, tw, (45, 45), True, fill)
    assert bt.kernel_for_batch(8) == 300
    d_f, d_g = torch.from_numpy(frames).cuda(), torch.from_numpy(guesses).cuda()
    for step in (None, 1, 0):
        if step is not None:
            bt.set_tuning("no_fused_c", step)
        out = bt.detect(d_f, d_g)
        bt.sync()
        assert np.array_equal(out.cpu().numpy(), ref), step
    bt.close()


def test_functor_through_the_tiled_plan_and_the_mailbox(pt, oracle):
    """One functor call on a 129×129 window: the tiled kernel's plan, the guess and the answer through the mailbox, the
    ticket the host polls for."""
    rng = np.random.Generator(np.random.PCG64(11))
    h, w, tw, ws = 360, 480, 25, (129, 129)
    frame = (128 + rng.integers(-3, 4, (h, w))).astype(np.uint8)
    yy, xx = np.ogrid[0:h, 0:w]
    frame[(yy - 170) ** 2 + (xx - 260) ** 2 <= 144] = 5
    fill = oracle.mode_u8(frame)
    want = oracle.detect(frame, fill, oracle.dog_kernel(oracle.sigma(tw), True), (64, 64), (180, 240))
    t = pt.Tracker(frame, tw, ws, True)
    assert t.kernel_for_batch(1) == 400
    assert t((180, 240)) == want
    t.close()


if __name__ == "__main__":
    record()
