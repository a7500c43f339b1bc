#!/usr/bin/env python3
"""What the predicted chain (pdog_detect_chains_predicted) costs per step against the two calls a caller had before it: the plain
indexed chain (pdog_detect_chains_indexed — no prediction, no loss detection; its kernels are the parent commit's, figure for
figure: profiles/predict_kernel_regs.txt) and the stepped motion walk at one target per group and k = 1
(pdog_detect_chains_motion — the same rule, two launches per step).

The video of tools/video_bench.py: one 1080p video of 2000 frames, 30 -> 24 positions per second (1600 steps), target width 25,
45 x 45 and 257 x 257 windows, 1 / 8 / 64 independent targets.  Also 4096 clips of 32 steps that share the video's frames
through the table, and "held" cases: a noise-free flat video (every response exactly 0, every FP32 runner-up ties) with exact
mode on, where the indexed chain pays the Float64 refinement on every frame and the predicted chain holds the target and
refines nothing.  The three calls are alternated in one process, device events around whole calls, medians of --reps samples
after --warmup calls; us per step = median ms * 1000 / steps walked.  The predict counters say which path served each case.

One JSON line per case; --out FILE writes them all (profiles/predict_bench.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from tools.video_bench import alternate, make_video, stats  # noqa: E402

PATH_NAMES = ("fused", "persistent", "fallback")


def run_case(pt, name, frames, table, start, ws, reps, warmup, exact=True, motion=True):
    """table [n_clips, n_steps] (host), start int32 [n_clips, 2] (host).  first = 1: the starts are filed, the rest is walked."""
    import torch
    n, h, w = frames.shape
    tw = 25
    bt = pt.BatchTracker(h, w, tw, ws, True, 128)
    bt.set_exact(1 if exact else 0)
    starts = torch.from_numpy(np.ascontiguousarray(start, np.int32)).cuda()
    nc, ns = table.shape
    res = {}
    calls = dict(indexed=lambda: res.__setitem__("idx", bt.detect_chains_indexed(frames, table, starts, first=1)),
                 predicted=lambda: res.__setitem__("pred", bt.detect_chains_predicted(frames, table, starts, first=1)))
    if motion:
        calls["motion"] = lambda: res.__setitem__("mot", bt.detect_chains_motion(frames, table, starts.unsqueeze(1).contiguous(), 1, first=1))
    before, refined0 = bt.predict_counts(), bt.exact_stats()[2]
    ms = alternate(calls, reps, warmup)
    bt.sync()
    moved = [a - b for a, b in zip(bt.predict_counts(), before)]
    steps = ns - 1
    med = {k: float(np.median(v)) for k, v in ms.items()}
    r = dict(case=name, frames=n, frame_h=h, frame_w=w, clips=nc, steps=steps, window=list(ws), target_width=tw, exact=exact, reps=reps,
             warmup=warmup, path=[p for p, c in zip(PATH_NAMES, moved) if c], kernel_for_batch=bt.kernel_for_batch(nc),
             indexed_ms=stats(ms["indexed"]), predicted_ms=stats(ms["predicted"]),
             indexed_us_per_step=med["indexed"] * 1e3 / steps, predicted_us_per_step=med["predicted"] * 1e3 / steps,
             predicted_over_indexed=med["predicted"] / med["indexed"],
             held_share=float((res["pred"][1][:, 1:] == -1).float().mean()),
             same_positions_as_indexed_share=float((res["pred"][0] == res["idx"]).all(-1).float().mean()),
             refined_windows_all_calls=bt.exact_stats()[2] - refined0)
    if motion:
        r.update(motion_ms=stats(ms["motion"]), motion_us_per_step=med["motion"] * 1e3 / steps, predicted_over_motion=med["predicted"] / med["motion"],
                 predicted_faster_than_motion=bool(med["predicted"] < med["motion"]),
                 equals_motion=bool(torch.equal(res["pred"][0], res["mot"][0][:, 0]) and torch.equal(res["pred"][1], res["mot"][1][:, 0])))
    bt.close()
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--video-frames", type=int, default=2000)
    ap.add_argument("--windows", default="45,257")
    ap.add_argument("--targets", default="1,8,64")
    ap.add_argument("--clips", type=int, default=4096, help="clips of 32 steps over the shared frames (0: none)")
    ap.add_argument("--no-held", action="store_true", help="leave the flat-video cases out")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "predict_bench measures on the GPU"
    import pawsometracker_jl_amd as pt
    results = []

    def report(r):
        r.update(device=torch.cuda.get_device_name(0), library=os.path.basename(pt.LIB_PATH))
        print(json.dumps(r), flush=True)
        results.append(r)

    n, h, w = args.video_frames, 1080, 1920
    frames, first_pos = make_video(n, h, w, 25, 8)
    table = pt.fps_table(30, n, 0.0, pt.DEFAULT_STOP, 24)
    start_of = lambda k: first_pos[k % len(first_pos)] + (k // len(first_pos)) * np.array([1, -1])
    for ws in (int(v) for v in args.windows.split(",") if v):
        for nt in (int(v) for v in args.targets.split(",") if v):
            report(run_case(pt, "video", frames, np.tile(table, (nt, 1)), np.stack([start_of(k) for k in range(nt)]), (ws, ws), args.reps, args.warmup))
    if args.clips:
        rng = np.random.default_rng(3)
        first = rng.integers(0, n - 33, args.clips)
        tab = (first[:, None] + np.arange(33)[None]).astype(np.int32)                    # 32 steps behind the filed start
        # a clip starts where its disc is on its first frame: near enough is the disc's first place plus the walk's drift, so start
        # every clip on disc (clip mod 8)'s first place and let the first steps lock on or hold
        report(run_case(pt, "clips", frames, tab, np.stack([start_of(k % 8) for k in range(args.clips)]), (45, 45), args.reps, args.warmup))
    if not args.no_held:
        flat = torch.full((min(n, 400), h, w), 128, dtype=torch.uint8, device="cuda")
        ftab = np.arange(flat.shape[0], dtype=np.int32)
        for ws in (45, 257):
            for nt in (1, 8):
                report(run_case(pt, "held_flat_video_exact", flat, np.tile(ftab, (nt, 1)), np.stack([start_of(k) for k in range(nt)]), (ws, ws),
                                args.reps, args.warmup, exact=True, motion=True))
        report(run_case(pt, "held_flat_video_fp32", flat, ftab[None], np.stack([start_of(0)]), (45, 45), args.reps, args.warmup, exact=False, motion=False))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
