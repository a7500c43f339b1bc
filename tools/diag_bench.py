#!/usr/bin/env python3
"""Diagnostic overlay (pdog_diag_render) on the GPU.  Cases: 1024 frames at 1080p, 256 frames at 4K (uniform noise,
resident in HBM, one call per step, device events after warm-up), and the cfg1 clip (100 frames 240x320, tw 25,
45x45 window) as a chain with and without the overlay, alternated in one session.  Reported: frames/s, bytes touched
(the source rows the mapping reads at 128-B line granularity plus 230 400 B out per frame), their share of the 6.29 TB/s
measured copy rate, the NumPy restatement's CPU time per frame and the device-to-host time of the full frames a host
renderer would need.  One JSON line per case; --out-dir DIR also writes DIR/r04_diag_<case>.json."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

COPY_RATE = 6.29e12     # B/s: measured float4 copy rate of the MI355X's HBM
LINE = 128


def bytes_touched(h, w):
    """Source bytes (128-B lines of the rows and columns the taps read, rows `w` bytes apart) and output bytes per frame."""
    import diag_restatement as R
    (i0, i1, _), (j0, j1, _) = R.maps(h, w)
    rows, cols = np.union1d(i0, i1) - 1, np.union1d(j0, j1) - 1
    lines = np.unique(((rows[:, None] * w + cols[None, :]) // LINE).ravel())
    return int(lines.size) * LINE, R.H * R.W


def walk(n, h, w, seed=0, step=9):
    rng = np.random.default_rng(seed)
    p = np.clip(np.cumsum(rng.integers(-step, step + 1, (n, 2)), 0) + [h // 2, w // 2], 1, [h, w])
    return p.astype(np.int32)


def timed(fn, reps):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def run_frames(name, n, h, w, reps, warmup):
    import torch
    import diag_restatement as R
    import pawsometracker_jl_amd as pt
    g = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device="cuda", generator=g)
    ij = torch.from_numpy(walk(n, h, w)).cuda()
    out = torch.empty((n, R.H, R.W), dtype=torch.uint8, device="cuda")
    with pt.Diagnose(True) as dia:
        for _ in range(warmup):
            dia(frames, ij, out=out)
        ms = timed(lambda: dia(frames, ij, out=out), reps)
    k = 4                                                   # a fresh handle on the first frames against the restatement
    with pt.Diagnose(True) as dia:
        chk = dia(frames[:k], ij[:k]).cpu().numpy()
    fr, pos = frames[:k].cpu().numpy(), [tuple(int(v) for v in p) for p in ij[:k].cpu().numpy()]
    t0 = time.perf_counter()
    ref = R.Diagnose(True).render(list(fr), pos)
    cpu_s = (time.perf_counter() - t0) / k
    host = torch.empty((min(n, 64), h, w), dtype=torch.uint8, pin_memory=True)
    d2h = timed(lambda: host.copy_(frames[:host.shape[0]], non_blocking=True), 5)
    src, dst = bytes_touched(h, w)
    med = float(np.median(ms))
    return dict(case=name, frames=n, frame_h=h, frame_w=w, reps=reps, warmup=warmup, ms_per_call_median=med,
                ms_per_call_min=float(min(ms)), ms_per_call_max=float(max(ms)), frames_per_s=n / (med * 1e-3),
                bytes_per_frame=dict(source=src, out=dst), achieved_TBps=n * (src + dst) / (med * 1e-3) / 1e12,
                share_of_copy_rate=n * (src + dst) / (med * 1e-3) / COPY_RATE,
                restatement_cpu_ms_per_frame=cpu_s * 1e3,
                d2h_full_frame_us=float(np.median(d2h)) * 1e3 / host.shape[0],
                checked_against_restatement=bool(np.array_equal(chk, ref)))


def run_cfg1(reps, warmup):
    import torch
    import pawsometracker_jl_amd as pt
    from bench import WORKLOADS, make_clip
    fh, fw, tw, ws, n, _ = WORKLOADS["cfg1"]
    ws = pt.fix_window_size(ws)
    frames_h, centres = make_clip(np, n, fh, fw, tw, (ws[0] // 2, ws[1] // 2), seed=0, noise=0)
    frames = torch.from_numpy(frames_h).cuda()
    start = (int(centres[0, 0]), int(centres[0, 1]))
    bt = pt.BatchTracker(fh, fw, tw, ws, True, pt.mode(frames_h[0]))
    bt.use_torch_stream()
    pos = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    buf = torch.empty((n, 360, 640), dtype=torch.uint8, device="cuda")
    dia = pt.Diagnose(True)

    def chain():
        bt.detect_chain(frames, start, out=pos)

    def both():
        bt.detect_chain(frames, start, out=pos)
        dia(frames, pos, out=buf)

    for _ in range(warmup):
        both()
    a, b = [], []
    for _ in range(reps):                                   # alternated: chain, chain + overlay, chain, ...
        a += timed(chain, 1)
        b += timed(both, 1)
    dia.close()
    bt.close()
    ma, mb = float(np.median(a)), float(np.median(b))
    return dict(case="cfg1", frames=n, frame_h=fh, frame_w=fw, reps=reps, warmup=warmup, chain_ms_median=ma,
                chain_overlay_ms_median=mb, overlay_overhead=mb / ma - 1, chain_us_per_frame=ma * 1e3 / n,
                chain_overlay_us_per_frame=mb * 1e3 / n, chain_ms_min=float(min(a)), chain_overlay_ms_min=float(min(b)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("1080p", "4k", "cfg1", "all"), default="all")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out-dir")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "diag_bench measures on the GPU"
    todo = ("1080p", "4k", "cfg1") if args.case == "all" else (args.case,)
    for case in todo:
        if case == "1080p":
            r = run_frames(case, 1024, 1080, 1920, args.reps, args.warmup)
        elif case == "4k":
            r = run_frames(case, 256, 2160, 3840, args.reps, args.warmup)
        else:
            r = run_cfg1(max(args.reps, 50), args.warmup)
        r["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(r), flush=True)
        if args.out_dir:
            with open(os.path.join(args.out_dir, f"r04_diag_{case}.json"), "w") as f:
                json.dump(r, f, indent=1)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
