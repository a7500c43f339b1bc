#!/usr/bin/env python3
"""pdog_blob_split (blob_kernel's split instances) against pdog_blob (the same kernel without the cell) on the SAME positions:
frames resident in HBM, device events after warm-up, the two calls alternated sample by sample in one session.  Cases, on 64
frames of 1080p (tools/shape_bench.py's frames):
  t2, t8, t32   4096 positions at R = 25 (the wave tier) as 2048 sets of 2, 512 of 8 and 128 of 32 targets, every set
                clustered within R of a disc's centre
  t1            the same 4096 positions as 4096 sets of ONE target: the split instance with an empty rival list
  r127_t4       1024 positions at R = 127 (the workgroup tier) as 256 sets of 4
  r127_t1       the same as 1024 sets of one
Every case holds the split call's first ten integers to pdog_blob's wherever n_cell == n_mask and n_contact == 0 says that the
cell cut nothing, before anything is timed.  One JSON line per case; --out FILE also writes them all to FILE (the committed
record is profiles/split_bench.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

from shape_bench import disc_frames  # noqa: E402
from video_bench import alternate, stats  # noqa: E402

CASES = {"t2": (2048, 2, 25), "t8": (512, 8, 25), "t32": (128, 32, 25), "t1": (4096, 1, 25), "r127_t4": (256, 4, 127), "r127_t1": (1024, 1, 127)}


def clustered(centres, n_sets, n_targets, R, seed=1):
    """ij int32 cuda [n_sets, n_targets, 2] and the sets' frames [n_sets, n_targets]: every set around one disc, its targets
    within R / 2 of the disc's centre (so within R of one another)."""
    import torch
    rng = np.random.default_rng(seed)
    nf, per, _ = centres.shape
    k, d = rng.integers(0, nf, n_sets), rng.integers(0, per, n_sets)
    ij = centres[k, d][:, None, :] + rng.integers(-(R // 4), R // 4 + 1, (n_sets, n_targets, 2))
    fi = np.repeat(k[:, None], n_targets, 1)
    return torch.from_numpy(ij.astype(np.int32)).cuda(), torch.from_numpy(fi.astype(np.int32)).cuda()


def run_case(pt, name, bt, frames, reps, warmup, centres):
    import torch
    n_sets, n_targets, R = CASES[name]
    ij, fi = clustered(centres, n_sets, n_targets, R)
    flat_ij, flat_fi = ij.view(-1, 2), fi.view(-1)
    _, bsum = bt.blobs(frames, flat_ij, flat_fi, R, 8, 8, want_sums=True)
    _, ssum = bt.split_blobs(frames, ij, fi, R, 8, 8, want_sums=True)
    ssum = ssum.view(-1, 12)
    whole = (ssum[:, 10] == ssum[:, 8]) & (ssum[:, 11] == 0)
    r = dict(case=name, positions=n_sets * n_targets, n_sets=n_sets, n_targets=n_targets, radius=R, frame_h=int(frames.shape[1]),
             frame_w=int(frames.shape[2]), reps=reps, warmup=warmup,
             cell_cut_nothing=float(whole.double().mean()), integers_equal_blob_where_cell_cut_nothing=bool(torch.equal(ssum[whole, :10], bsum[whole])),
             blobs_not_empty=float((ssum[:, 0] > 0).double().mean()), contact=float((ssum[:, 11] > 0).double().mean()))
    calls = {"blob": lambda: bt.blobs(frames, flat_ij, flat_fi, R, 8, 8), "split": lambda: bt.split_blobs(frames, ij, fi, R, 8, 8)}
    ms = alternate(calls, reps, warmup)
    r["ms"] = {k: stats(v) for k, v in ms.items()}
    r["blob_us_per_position"] = float(np.median(ms["blob"])) * 1e3 / r["positions"]
    r["split_us_per_position"] = float(np.median(ms["split"])) * 1e3 / r["positions"]
    r["split_over_blob"] = float(np.median(ms["split"]) / np.median(ms["blob"]))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=tuple(CASES) + ("all",), default="all")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "split_bench measures on the GPU"
    import pawsometracker_jl_amd as pt
    frames, centres = disc_frames(64, 1080, 1920, 32)
    results = []
    with pt.BatchTracker(1080, 1920, 25, (45, 45), True, 128) as bt:
        for case in (tuple(CASES) if args.case == "all" else (args.case,)):
            r = run_case(pt, case, bt, frames, args.reps, args.warmup, centres)
            bt.sync()
            r["device"] = torch.cuda.get_device_name(0)
            r["library"] = os.path.basename(pt.LIB_PATH)
            print(json.dumps(r), flush=True)
            results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
