#!/usr/bin/env python3
"""prune_bench.py — kept ranges on the roll batch path (csrc/dog_prune.hpp): what share of the (slot, sub-chunk) pairs a
batch keeps, and what a step costs, in steady state.

bench.py's frame recipe (make_frames, its seed, its workloads, its guesses) with the noise level selectable; `--noise-only`
removes the discs (every window sees noise alone: nothing can be pruned, and the policy of launch_strips must stop paying
for the pre-pass).  After `--warmup` steps — long enough for that policy to settle — `--steps` steps are timed with HIP events
around pdog_detect_batch; the kept / total counts are read before and after them.  A library without the pre-pass (an older
build chosen through PAWSOME_DOG_LIB) reports no counts.  One JSON line on stdout."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--target-width", type=float, default=0.0)
    ap.add_argument("--noise", type=int, default=3)
    ap.add_argument("--noise-only", action="store_true", help="frames without a disc")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tuning", action="append", default=[], metavar="KEY=0|1")
    ap.add_argument("--no-exact", action="store_true")
    args = ap.parse_args()
    import torch
    import pawsometracker_jl_amd as pt
    fh, fw, tw, ws, batch, _ = bench.WORKLOADS[args.workload]
    batch = args.batch or batch
    tw = args.target_width or tw
    ws = (ws, ws) if not isinstance(ws, tuple) else (ws[1], ws[0])
    ws = tuple(int(v) // 2 * 2 + 1 for v in ws)
    radii = (ws[0] // 2, ws[1] // 2)
    dev = torch.device("cuda", 0)
    frames, guesses_h, _ = bench.make_frames(torch, batch, fh, fw, tw, radii, seed=0, noise=args.noise, device=dev)
    if args.noise_only:
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        frames = (128 + torch.randint(-args.noise, args.noise + 1, frames.shape, generator=g, device=dev, dtype=torch.int16)).clamp(0, 255).to(torch.uint8)
    fill = pt.mode(frames[0].cpu().numpy()) if args.noise else 128
    bt = pt.BatchTracker(fh, fw, tw, ws, True, fill, device=0)
    for kv in args.tuning:
        key, _, val = kv.partition("=")
        bt.set_tuning(key, int(val or 1))
    if args.no_exact:
        bt.set_exact(0)
    bt.reserve(batch)
    has_counts = hasattr(pt.lib(), "pdog_get_prune_counts")
    res = {"tool": "prune_bench", "workload": args.workload, "batch": batch, "target_width": tw, "noise": args.noise,
           "noise_only": args.noise_only, "tuning": args.tuning, "kernel_for_this_batch": bt.kernel_for_batch(batch), "fill": int(fill)}
    guesses = torch.from_numpy(guesses_h).to(dev)
    out = torch.empty((batch, 2), dtype=torch.int32, device=dev)
    for _ in range(args.warmup):
        bt.detect(frames, guesses, out=out)
    torch.cuda.synchronize()
    c_warm = bt.prune_counts() if has_counts else None
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for a, b in ev:
        a.record()
        bt.detect(frames, guesses, out=out)
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    res["kernel_ms"] = {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1], "mean": float(np.mean(ms)), "steps": args.steps}
    if has_counts:
        c_end = bt.prune_counts()
        pairs = c_end[1] - c_warm[1]
        res["prune"] = {"kept_share_warmup": c_warm[0] / c_warm[1] if c_warm[1] else None,
                        "kept_share_timed": (c_end[0] - c_warm[0]) / pairs if pairs else None,
                        "pairs_counted_per_timed_step": pairs / args.steps}
    res["positions_crc"] = int(np.bitwise_xor.reduce(out.cpu().numpy().astype(np.int64).ravel() * np.arange(1, 2 * batch + 1)))
    print(json.dumps(res))
    bt.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
