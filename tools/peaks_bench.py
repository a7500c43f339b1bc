#!/usr/bin/env python3
"""What the K-peaks selection (pdog_detect_peaks) costs on top of the detect call that writes the response map, and its two
paths against each other.

large:  cfg2's shape — 64 windows of 271 x 481 on 1080p frames, l = 65 — for K = 1, 4 and 16
small:  4096 windows of 45 x 45 on the same frames, K = 4
Frames: 128 +- 2 noise with 16 dark discs each (tools/video_bench.make_video), one window per frame (large) or 64 per frame
behind a frame index (small).  Legs, all writing the map into a buffer of the caller's:
    detect        BatchTracker.detect(want_resp=True) alone: the yardstick of the same build
    peaks_K       BatchTracker.detect_peaks(K, want_resp=True): the same launches and the selection kernel behind them
    peaks_scan_K  the same on a tracker with "peaks_no_list" set: the rounds scan the map instead of the LDS list
Device events, medians of --reps samples after --warmup calls of each leg, all legs of a case alternated sample by sample;
"spread" is (max - min) / median of a leg's samples.  Per K: peaks_over_detect = (peaks - detect) / detect, the selection's
cost as a share of the map-writing detect call, the same for the scan path, and list_over_scan = (peaks - detect) /
(peaks_scan - detect).  One JSON line per case; --out FILE writes them all (profiles/peaks_bench.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from tools.video_bench import alternate, make_video, stats  # noqa: E402


def run_case(pt, name, frames, ws, n, ks, reps, warmup):
    import torch
    nf, h, w = frames.shape
    rng = np.random.default_rng(len(name))
    r2 = (ws[0] // 2, ws[1] // 2)
    g = np.stack([rng.integers(r2[0] // 2, h - r2[0] // 2, n), rng.integers(r2[1] // 2, w - r2[1] // 2, n)], 1).astype(np.int32)
    d_g = torch.from_numpy(g).cuda()
    d_fi = torch.from_numpy((np.arange(n) % nf).astype(np.int32)).cuda()
    bt, bt_scan = (pt.BatchTracker(h, w, 25, ws, True, 128) for _ in range(2))
    bt_scan.set_tuning("peaks_no_list", 1)
    info = bt.info()
    r = dict(case=name, windows=n, window=[info.win_h, info.win_w], frame_h=h, frame_w=w, kernel_len=info.kernel_len,
             kernel=bt.kernel_for_batch(n), reps=reps, warmup=warmup)
    calls = {"detect": lambda: bt.detect(frames, d_g, d_fi, want_resp=True)}
    for k in ks:
        calls[f"peaks_{k}"] = lambda k=k: bt.detect_peaks(frames, d_g, k, None, d_fi, want_resp=True)
        calls[f"peaks_scan_{k}"] = lambda k=k: bt_scan.detect_peaks(frames, d_g, k, None, d_fi, want_resp=True)
    before = bt.peaks_counts()
    ms = alternate(calls, reps, warmup)
    bt.sync()
    bt_scan.sync()
    after = bt.peaks_counts()
    r["windows_whose_list_overflowed"] = (after[1] - before[1]) / max(1, after[0] - before[0])
    a = bt.detect_peaks(frames, d_g, max(ks), None, d_fi)
    b = bt_scan.detect_peaks(frames, d_g, max(ks), None, d_fi)
    r["equal"] = bool(all(torch.equal(x, y) for x, y in zip(a, b)))
    r["mean_count_at_max_k"] = float(a[2].float().mean())
    med = {k: float(np.median(v)) for k, v in ms.items()}
    r["ms"] = {k: stats(v) for k, v in ms.items()}
    for k in ks:
        step, scan = med[f"peaks_{k}"] - med["detect"], med[f"peaks_scan_{k}"] - med["detect"]
        r[f"k{k}"] = dict(peaks_over_detect=step / med["detect"], scan_over_detect=scan / med["detect"], list_over_scan=step / scan if scan > 0 else None)
    bt.close()
    bt_scan.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("large", "small", "all"), default="all")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "peaks_bench measures on the GPU"
    import pawsometracker_jl_amd as pt
    frames, _ = make_video(64, 1080, 1920, 25, 16)
    results = []
    cases = [("large", "cfg2_64x271x481", (270, 480), 64, (1, 4, 16)), ("small", "4096x45x45", (45, 45), 4096, (4,))]
    for which, name, ws, n, ks in cases:
        if args.case in (which, "all"):
            r = run_case(pt, name, frames, ws, n, ks, args.reps, args.warmup)
            r.update(device=torch.cuda.get_device_name(0), library=os.path.basename(pt.LIB_PATH))
            print(json.dumps(r), flush=True)
            results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
