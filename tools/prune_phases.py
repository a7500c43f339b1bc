#!/usr/bin/env python3
"""prune_phases.py — where a workgroup of the roll batch path's pre-pass (csrc/dog_prune.hpp) spends its cycles.

Diagnostic build only (`make diag`, chosen through PAWSOME_DOG_LIB): thread 0 of every workgroup adds the cycles between its
phase stamps — DC level, energy pass, straddle pass, cell choice and E, patch, row pass, column pass, hulls, publish — to
counters behind the kept / total counts, and pdog_get_prune_counts prints their means per workgroup on stderr.  bench.py's
frame recipe and guesses (tools/pad_bench.py's placements: `bench`, or `inside` for tiles wholly inside the frame);
`--steps` batches and no warm-up: the counters add up from the tracker's first batch.  The product build prints no
phases; a JSON line with the kept share goes to stdout either way."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
import pad_bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--placement", default="bench", choices=("bench", "inside"))
    ap.add_argument("--target-width", type=float, default=0.0)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    import torch
    import pawsometracker_jl_amd as pt
    fh, fw, tw, ws, batch, _ = bench.WORKLOADS[args.workload]
    tw = args.target_width or tw
    ws = (ws, ws) if not isinstance(ws, tuple) else (ws[1], ws[0])
    ws = tuple(int(v) // 2 * 2 + 1 for v in ws)
    radii = (ws[0] // 2, ws[1] // 2)
    dev = torch.device("cuda", 0)
    frames, guesses_h, _ = bench.make_frames(torch, batch, fh, fw, tw, radii, seed=0, noise=3, device=dev)
    guesses_h = pad_bench.place(guesses_h, args.placement, fh, fw, radii, pad_bench.kernel_len(tw))
    bt = pt.BatchTracker(fh, fw, tw, ws, True, pt.mode(frames[0].cpu().numpy()), device=0)
    guesses = torch.from_numpy(guesses_h).to(dev)
    out = torch.empty((batch, 2), dtype=torch.int32, device=dev)
    for _ in range(args.steps):
        bt.detect(frames, guesses, out=out)
    torch.cuda.synchronize()
    kept, total = bt.prune_counts()   # (the diagnostic build prints the phase means here)
    print(json.dumps({"tool": "prune_phases", "workload": args.workload, "placement": args.placement, "target_width": tw, "steps": args.steps,
                      "kept_share": kept / total if total else None, "library": pt.LIB_PATH}))
    bt.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
