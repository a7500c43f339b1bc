#!/usr/bin/env python3
"""What the background model costs (pdog_bg_estimate, pdog_bg_subtract_indexed), each kernel beside two references timed in
the same session, the calls alternated:

estimate:  the median of K = 9, 25 and 64 frames of 1080p, against (copy) a device-to-device copy of K frames — the bytes the
           kernel must read; the copy also writes them — and (torch) what a user would write instead,
           frames[idx].sort(0).values[(K - 1) // 2].
subtract:  256 frames of 1080p through a table, against (copy) a copy of 256 frames — one frame read and one written per step,
           as the kernel — and (torch) (128 + frames[idx].to(int16) - model.to(int16)).clamp(0, 255).to(uint8).
video:     track_video on the 2000-frame 1080p video of tools/video_bench.py (30 -> 24 positions per second, 45 x 45 windows) for
           1 and 8 targets, background=25 against background=None: wall time of the whole call, host work included.

Device events (the video case: the host's clock around a synchronised call), medians of --reps samples after --warmup calls.
One JSON line per case; --out FILE writes them all (profiles/background_bench.json)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from tools.video_bench import alternate, make_video, stats  # noqa: E402

H, W = 1080, 1920


def run_estimate(pt, frames, k, reps, warmup):
    import torch
    n = frames.shape[0]
    samples = pt.background_samples(np.arange(n), k)
    idx = torch.from_numpy(samples).long().cuda()
    buf = torch.empty((k, H, W), dtype=torch.uint8, device="cuda")
    res = {}
    with pt.Background(H, W) as bg:
        calls = dict(kernel=lambda: bg.estimate(frames, samples),
                     copy=lambda: buf.copy_(frames[:k]),
                     torch=lambda: res.__setitem__("t", frames[idx].sort(0).values[(k - 1) // 2]))
        ms = alternate(calls, reps, warmup)
        equal = bool(torch.equal(bg.image(), res["t"]))
    med = {name: float(np.median(v)) for name, v in ms.items()}
    return dict(case="estimate", k=k, frame_h=H, frame_w=W, bytes_read=int(k * H * W), reps=reps, warmup=warmup,
                kernel_ms=stats(ms["kernel"]), copy_ms=stats(ms["copy"]), torch_ms=stats(ms["torch"]), equal=equal,
                kernel_over_copy=med["kernel"] / med["copy"], torch_over_kernel=med["torch"] / med["kernel"],
                kernel_read_GBps=k * H * W / med["kernel"] / 1e6)


def run_subtract(pt, frames, steps, reps, warmup):
    import torch
    n = frames.shape[0]
    table = np.floor(np.arange(steps) * (n / steps)).astype(np.int32)
    idx = torch.from_numpy(table).long().cuda()
    out = torch.empty((steps, H, W), dtype=torch.uint8, device="cuda")
    buf = torch.empty_like(out)
    res = {}
    with pt.Background(H, W) as bg:
        bg.estimate(frames, pt.background_samples(np.arange(n), 25))
        model = bg.image()
        calls = dict(kernel=lambda: bg.subtract(frames, table, out=out),
                     copy=lambda: buf.copy_(frames[:steps]),
                     torch=lambda: res.__setitem__("t", (128 + frames[idx].to(torch.int16) - model.to(torch.int16)).clamp(0, 255).to(torch.uint8)))
        ms = alternate(calls, reps, warmup)
        equal = bool(torch.equal(out, res["t"]))
    med = {name: float(np.median(v)) for name, v in ms.items()}
    return dict(case="subtract", steps=steps, frame_h=H, frame_w=W, bytes_read_and_written=int(2 * steps * H * W), reps=reps, warmup=warmup,
                kernel_ms=stats(ms["kernel"]), copy_ms=stats(ms["copy"]), torch_ms=stats(ms["torch"]), equal=equal,
                kernel_over_copy=med["kernel"] / med["copy"], torch_over_kernel=med["torch"] / med["kernel"],
                kernel_GBps=2 * steps * H * W / med["kernel"] / 1e6)


def run_video(pt, frames, first_pos, n_targets, reps, warmup):
    import torch
    locs = [("ij", (int(first_pos[t][0]), int(first_pos[t][1]))) for t in range(n_targets)]
    args = dict(rate=30, fps=24, target_width=25, window_size=45, start_locations=locs)
    wall = {"none": [], "background_25": []}
    for rep in range(warmup + reps):
        for name, kw in (("none", {}), ("background_25", dict(background=25))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ts, idx = pt.track_video(frames, **kw, **args)
            torch.cuda.synchronize()
            if rep >= warmup:
                wall[name].append((time.perf_counter() - t0) * 1e3)
    a, b = float(np.median(wall["none"])), float(np.median(wall["background_25"]))
    return dict(case="video", frames=int(frames.shape[0]), frame_h=H, frame_w=W, steps=len(ts), targets=n_targets, window=[45, 45],
                reps=reps, warmup=warmup, none_ms=stats(wall["none"]), background_25_ms=stats(wall["background_25"]),
                background_over_none=b / a, extra_us_per_step=(b - a) * 1e3 / len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("estimate", "subtract", "video", "all"), default="all")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--video-frames", type=int, default=2000)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "background_bench measures on the GPU"
    import pawsometracker_jl_amd as pt
    results = []

    def emit(r):
        r.update(device=torch.cuda.get_device_name(0), library=os.path.basename(pt.LIB_PATH))
        print(json.dumps(r), flush=True)
        results.append(r)

    frames, first_pos = make_video(args.video_frames, H, W, 25, 8)
    if args.case in ("estimate", "all"):
        for k in (9, 25, 64):
            emit(run_estimate(pt, frames, k, args.reps, args.warmup))
            torch.cuda.empty_cache()
    if args.case in ("subtract", "all"):
        emit(run_subtract(pt, frames, 256, args.reps, args.warmup))
        torch.cuda.empty_cache()
    if args.case in ("video", "all"):
        for nt in (1, 8):
            emit(run_video(pt, frames, first_pos, nt, max(3, args.reps // 4), min(args.warmup, 2)))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
