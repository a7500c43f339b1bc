#!/usr/bin/env python3
"""FrameBlobs.find (pdog_frame_blobs: seven kernels per round of steps) on 256 subtracted 1080p frames resident in HBM, device
events after warm-up, beside a device copy of the same frames — the project's usual yardstick — the calls alternated sample by
sample in one session.  Cases:
  discs    8 dark discs of width 25 per frame on a 128 +- 2 floor (tools/video_bench.py's video)
  noise    seeded noise: 41 % of the pixels at contrasts 8 ... 68
  spiral   ONE one-pixel-wide spiral that fills the frame (tests/frame_blobs_scenes.py): the longest chains a frame can hold
Every case holds the first frame's count and words to tests/frame_blobs_restatement.py before anything is timed, and reports
scipy.ndimage.label plus NumPy integer sums of --cpu-frames frames on 16 threads (a process pool) as us per frame.  A case whose
single frame takes so long that its samples would exceed --budget-ms is timed on fewer frames, and says so ("frames").
  video    track_video on one 1080p video of 2000 frames with 8 targets: find="frame" beside start_locations at the same places
           (the centre window holds no 8 animals to find): the feature runs on ONE frame, the difference should be one call
One JSON line per case; --out FILE also writes them all to FILE."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import frame_blobs_restatement as FR  # noqa: E402
import frame_blobs_scenes as FS  # noqa: E402
from video_bench import alternate, make_video, stats  # noqa: E402

H, W = 1080, 1920


def _cpu_one(frame):
    return FR.find(frame[None], cap=64)[0][0, 0]


def cpu_us_per_frame(frames, threads=16):
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    # (spawned, not forked: the workers import this file afresh, which touches no GPU, so the device stays this process's alone)
    with ProcessPoolExecutor(threads, mp_context=multiprocessing.get_context("spawn")) as ex:
        list(ex.map(_cpu_one, frames[:threads]))                # (the workers started and scipy imported)
        t0 = time.perf_counter()
        list(ex.map(_cpu_one, frames))
        return (time.perf_counter() - t0) * 1e6 / len(frames)


def make_frames(case, n):
    import torch
    if case == "discs":
        return make_video(n, H, W, 25, 8)[0]
    if case == "noise":
        g = torch.Generator(device="cuda").manual_seed(41)
        out = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
        for k0 in range(0, n, 32):
            k1 = min(n, k0 + 32)
            on = torch.rand((k1 - k0, H, W), device="cuda", generator=g) < 0.41
            s = torch.where(on, torch.randint(8, 69, on.shape, device="cuda", generator=g), torch.randint(-5, 8, on.shape, device="cuda", generator=g))
            out[k0:k1] = (128 - s).to(torch.uint8)
        return out
    one = torch.from_numpy(FS.draw(FS.pattern("spiral", H, W))).cuda()
    return one[None].repeat(n, 1, 1)


def run_case(pt, case, n, in_flight, reps, warmup, cpu_frames, budget_ms):
    import torch
    from video_bench import timed
    with pt.FrameBlobs(H, W, steps_in_flight=1) as fb:            # one frame, timed: how many frames the budget allows
        one = make_frames(case, 1)
        fb.find(one, connectivity=4)
        ms_one = max(timed(lambda: fb.find(one, connectivity=4)), timed(lambda: fb.find(one, connectivity=8)))
    n = int(min(n, max(1, budget_ms / ((reps + warmup) * ms_one))))
    frames = make_frames(case, n)
    copy = torch.empty_like(frames)
    r = dict(case=case, frames=n, one_frame_alone_ms=ms_one, frame_h=H, frame_w=W, steps_in_flight=in_flight, reps=reps, warmup=warmup)
    with pt.FrameBlobs(H, W, steps_in_flight=in_flight) as fb:
        host = frames[:1].cpu().numpy()
        count, words = fb.find(frames[:1])
        want = FR.find(host)
        r["equals_restatement"] = bool(np.array_equal(count.cpu().numpy(), want[0]) and np.array_equal(words.cpu().numpy(), want[1]))
        r["blobs_frame0"], r["mask_pixels_frame0"] = int(want[0][0, 0]), int(want[0][0, 1])
        for conn in (8, 4):
            calls = {"copy": lambda: copy.copy_(frames), f"find{conn}": (lambda conn=conn: fb.find(frames, connectivity=conn))}
            ms = alternate(calls, reps, warmup)
            torch.cuda.synchronize()
            r[f"find{conn}_ms"] = stats(ms[f"find{conn}"])
            r[f"find{conn}_us_per_frame"] = float(np.median(ms[f"find{conn}"])) * 1e3 / n
            r["copy_us_per_frame"] = float(np.median(ms["copy"])) * 1e3 / n
            r[f"find{conn}_over_copy"] = float(np.median(ms[f"find{conn}"]) / np.median(ms["copy"]))
    if cpu_frames:
        r["cpu_frames"] = cpu_frames
        r["cpu16_us_per_frame"] = cpu_us_per_frame(frames[:cpu_frames].cpu().numpy())
        r["cpu16_over_find8"] = r["cpu16_us_per_frame"] / r["find8_us_per_frame"]
    return r


def run_video(pt, n_frames, reps, warmup):
    import torch
    tw, nt = 25, 8
    frames, first = make_video(n_frames, H, W, tw, nt)
    args = dict(rate=30, start=0, stop=n_frames / 30, fps=24, target_width=tw)
    try:
        _, by_frame = pt.track_video(frames, n_targets=nt, find="frame", **args)
    except ValueError as e:                                    # (two discs that touch on the first frame are one blob)
        return dict(case="video", frames=n_frames, targets=nt, error=str(e))
    starts = [("ij", (int(i), int(j))) for i, j in by_frame[:, 0].cpu().tolist()]
    _, by_list = pt.track_video(frames, start_locations=starts, **args)
    calls = {"start_locations": lambda: pt.track_video(frames, start_locations=starts, **args),
             "find_frame": lambda: pt.track_video(frames, n_targets=nt, find="frame", **args)}
    ms = alternate(calls, reps, warmup)
    d = float(np.median(ms["find_frame"]) - np.median(ms["start_locations"]))
    found = sorted(tuple(p) for p in by_frame[:, 0].cpu().tolist())
    near = all(min(abs(p[0] - q[0]) + abs(p[1] - q[1]) for q in first.tolist()) <= 3 for p in found)
    return dict(case="video", frames=n_frames, steps=int(by_frame.shape[1]), targets=nt, frame_h=H, frame_w=W, reps=reps, warmup=warmup,
                every_disc_found=bool(near and len(set(found)) == nt), same_walk_as_a_list_of_those_starts=bool(torch.equal(by_frame, by_list)),
                ms={k: stats(v) for k, v in ms.items()}, find_frame_minus_start_locations_ms=d,
                find_frame_over_start_locations=float(np.median(ms["find_frame"]) / np.median(ms["start_locations"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("discs", "noise", "spiral", "video", "all"), default="all")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps-in-flight", type=int, default=32)
    ap.add_argument("--video-frames", type=int, default=2000)
    ap.add_argument("--cpu-frames", type=int, default=32)
    ap.add_argument("--budget-ms", type=float, default=15000.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "frame_blobs_bench measures on the GPU"
    import pawsometracker_jl_amd as pt
    results = []
    for case in (("discs", "noise", "spiral", "video") if args.case == "all" else (args.case,)):
        torch.cuda.empty_cache()
        r = run_video(pt, args.video_frames, args.reps, args.warmup) if case == "video" else \
            run_case(pt, case, args.frames, args.steps_in_flight, args.reps, args.warmup, args.cpu_frames, args.budget_ms)
        r["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(r), flush=True)
        results.append(r)
        if args.out:                                            # (after every case: a later case's trouble keeps the earlier ones)
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
