#!/usr/bin/env python3
"""What the exclusive walk (pdog_detect_chains_exclusive) costs per step against independent chains
(pdog_detect_chains_indexed) for the same targets on the same data.

The video bench's shape (tools/video_bench.py): one 1080p video of 2000 frames, 30 -> 24 positions per second (1600
steps), 45 x 45 windows, target width 25.  Cases, as groups x targets per group: 1 x 1, 1 x 8, 2 x 32 (64 targets: a group
holds at most 32) and 64 x 8 — every group walks the same table.  k, min_distance and min_ratio are the defaults
(min(32, 2 T), 25, 0.5).

Device events around whole calls, medians of --reps samples after --warmup calls, the two walks alternated in the same
process; us per step = median ms * 1000 / steps.  The exclusive walk is a detect batch with response maps, the peak
selection and the assignment kernel per step, whatever the size; the indexed chain takes whichever path the tracker picks
for that many clips (one launch that walks them all where a kernel does that).  Also reported: the share of steps in
which a target was held or took a later pick.  One JSON line per case; --out FILE writes them all
(profiles/exclusive_bench.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from tools.video_bench import alternate, make_video, stats  # noqa: E402


def run_case(pt, frames, first_pos, rate, fps, ws, n_groups, n_targets, reps, warmup):
    import torch
    n, h, w = frames.shape
    tw = 25
    table = pt.fps_table(rate, n, 0.0, pt.DEFAULT_STOP, fps)
    m = len(table)
    n_all = n_groups * n_targets
    start = np.stack([first_pos[k % len(first_pos)] + (k // len(first_pos)) * np.array([1, -1]) for k in range(n_all)]).astype(np.int32)
    starts = torch.from_numpy(start).cuda()
    bt = pt.BatchTracker(h, w, tw, ws, True, 128)
    res = {}
    out = torch.empty((n_all, m, 2), dtype=torch.int32, device="cuda")
    tab_all, tab_groups = np.tile(table, (n_all, 1)), np.tile(table, (n_groups, 1))
    starts3 = starts.view(n_groups, n_targets, 2)

    def exclusive():
        res["excl"] = bt.detect_chains_exclusive(frames, tab_groups, starts3)

    calls = dict(indexed=lambda: bt.detect_chains_indexed(frames, tab_all, starts, out=out), exclusive=exclusive)
    ms = alternate(calls, reps, warmup)
    bt.sync()
    state = res["excl"][1]
    ex, ix = float(np.median(ms["exclusive"])), float(np.median(ms["indexed"]))
    r = dict(case="exclusive_walk", frames=n, frame_h=h, frame_w=w, rate=rate, fps=fps, steps=m, groups=n_groups, targets_per_group=n_targets,
             window=list(ws), target_width=tw, reps=reps, warmup=warmup, kernel_for_batch=bt.kernel_for_batch(n_all),
             exclusive_ms=stats(ms["exclusive"]), indexed_ms=stats(ms["indexed"]),
             exclusive_us_per_step=ex * 1e3 / m, indexed_us_per_step=ix * 1e3 / m, exclusive_over_indexed=ex / ix,
             held_share=float((state == -1).float().mean()), later_pick_share=float((state > 1).float().mean()),
             same_positions_share=float((res["excl"][0].view(n_all, m, 2) == out).all(-1).float().mean()))
    bt.close()
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--video-frames", type=int, default=2000)
    ap.add_argument("--cases", default="1x1,1x8,2x32,64x8", help="groups x targets per group")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "exclusive_bench measures on the GPU"
    import pawsometracker_jl_amd as pt
    frames, first_pos = make_video(args.video_frames, 1080, 1920, 25, 8)
    results = []
    for case in args.cases.split(","):
        g, t = (int(v) for v in case.split("x"))
        r = run_case(pt, frames, first_pos, 30, 24, (45, 45), g, t, args.reps, args.warmup)
        r.update(device=torch.cuda.get_device_name(0), library=os.path.basename(pt.LIB_PATH))
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
