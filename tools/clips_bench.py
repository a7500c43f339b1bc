#!/usr/bin/env python3
"""Many clips with their own fill and start (pdog_clips_*) on the GPU.

clip_modes: 4096 frames of 240x320, 256 frames of 1080p and one 4K frame (resident in HBM, device events after warm-up):
time per call, bytes read over the device-to-device copy rate measured in the same session, and the same modes from a loop
of mode_device calls over the same frames (one launch, one 2 KB read-back and one wait per frame: what the library
offered before).

track_clips: 4096 clips x 32 frames of 240x320, tw 25, 45x45 window, with 1, 5 and 30 distinct fills, first 0 and 1,
against detect_chains on the same clips under one fill, alternated; with the number of launches the walk queued.

One JSON line per case; --out FILE writes them all (profiles/clips_bench.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def timed(fn, reps, inner=1):
    """ms per call of fn, `reps` samples of `inner` back-to-back calls between two device events."""
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        for _ in range(inner):
            fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) / inner for a, b in ev]


def stats(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def copy_rate(reps=10):
    """Bytes read plus bytes written per second of a 1 GiB device-to-device copy, this session."""
    import torch
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda").random_(0, 256)
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    ms = timed(lambda: dst.copy_(src), reps)
    return 2 * src.numel() / (float(np.median(ms)) * 1e-3)


def run_modes(pt, name, n, h, w, reps, warmup, rate):
    import time
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(118, 139, (n, h, w), dtype=torch.uint8, device="cuda", generator=g)   # a noisy background
    bt = pt.BatchTracker(h, w, 25, (45, 45), True, 0)
    out = torch.empty((n,), dtype=torch.int32, device="cuda")
    inner = max(1, 64 // n)
    for _ in range(warmup):
        bt.clip_modes(frames, out=out)
    ms = timed(lambda: bt.clip_modes(frames, out=out), reps, inner)
    counters = bt.clips_counters()
    got = out.cpu().numpy()
    k = n                                                        # the per-frame way, over the same frames
    for b in range(min(k, 8)):
        pt.mode_device(frames[b])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop = [pt.mode_device(frames[b]) for b in range(k)]
    loop_ms = (time.perf_counter() - t0) * 1e3 / k
    bt.close()
    med = float(np.median(ms))
    return dict(case=f"modes_{name}", frames=n, frame_h=h, frame_w=w, reps=reps, warmup=warmup, calls_per_sample=inner,
                form="one workgroup per frame" if counters[0] else "several workgroups per frame", ms_per_call=stats(ms),
                us_per_frame=med * 1e3 / n, read_TBps=n * h * w / (med * 1e-3) / 1e12,
                share_of_copy_rate=n * h * w / (med * 1e-3) / rate, mode_device_loop_ms_per_frame=loop_ms,
                mode_device_loop_frames=k, speedup_over_loop=loop_ms * n / med, equal_to_loop=bool(list(got[:k]) == loop))


def make_clips(n_clips, n_frames, h, w, tw, bkgd, seed=0, chunk=64):
    """uint8 cuda [n_clips, n_frames, h, w]: a dark disc on a random walk over clip c's background bkgd[c], +-2 noise."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    frames = torch.empty((n_clips, n_frames, h, w), dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(seed)
    pos = np.cumsum(rng.integers(-4, 5, (n_clips, n_frames, 2)), 1) + rng.integers([40, 40], [h - 40, w - 40], (n_clips, 1, 2))
    pos = np.clip(pos, 1, [h, w]).astype(np.int32)
    ii = torch.arange(1, h + 1, device="cuda").view(1, 1, h, 1)
    jj = torch.arange(1, w + 1, device="cuda").view(1, 1, 1, w)
    d_pos = torch.from_numpy(pos).cuda()
    d_bk = torch.as_tensor(bkgd, dtype=torch.int16, device="cuda").view(-1, 1, 1, 1)
    for c0 in range(0, n_clips, chunk):
        c1 = min(n_clips, c0 + chunk)
        p = d_pos[c0:c1]
        disc = (ii - p[:, :, 0, None, None]) ** 2 + (jj - p[:, :, 1, None, None]) ** 2 <= (tw // 2) ** 2
        noise = torch.randint(-2, 3, (c1 - c0, n_frames, h, w), dtype=torch.int16, device="cuda", generator=g)
        frames[c0:c1] = torch.where(disc, torch.zeros_like(noise), d_bk[c0:c1] + noise).clamp_(0, 255).to(torch.uint8)
    return frames, pos[:, 0].copy()


def run_track(pt, n_clips, n_frames, reps, warmup):
    import torch
    h, w, tw, ws = 240, 320, 25, (45, 45)
    results = []
    for n_fills in (1, 5, 30):
        values = 60 + 6 * np.arange(n_fills)
        fills = values[np.arange(n_clips) % n_fills].astype(np.int32)
        frames, start = make_clips(n_clips, n_frames, h, w, tw, fills)
        starts = torch.from_numpy(start).cuda()
        bt = pt.BatchTracker(h, w, tw, ws, True, int(fills[0]))
        out = torch.empty((n_clips, n_frames, 2), dtype=torch.int32, device="cuda")
        ref = torch.empty_like(out)
        calls = dict(chains=lambda: bt.detect_chains(frames, starts, out=ref),
                     first0=lambda: bt.track_clips(frames, starts, fills=fills, first=0, out=out),
                     first1=lambda: bt.track_clips(frames, starts, fills=fills, first=1, out=out))
        for fn in calls.values():
            for _ in range(warmup):
                fn()
        bt.sync()
        ms = {k: [] for k in calls}
        for _ in range(reps):                                    # alternated
            for k, fn in calls.items():
                ms[k] += timed(fn, 1)
        bt.sync()
        before = bt.clips_counters()
        calls["first0"]()
        bt.sync()
        after = bt.clips_counters()
        batches = after[2] - before[2]
        same = bool(torch.equal(out, ref)) if n_fills == 1 else None
        bt.close()
        med = {k: float(np.median(v)) for k, v in ms.items()}
        results.append(dict(case=f"track_{n_fills}_fills", clips=n_clips, frames_per_clip=n_frames, frame_h=h, frame_w=w,
                            window=list(ws), target_width=tw, distinct_fills=n_fills, reps=reps, warmup=warmup,
                            detect_chains_ms=stats(ms["chains"]), track_first0_ms=stats(ms["first0"]), track_first1_ms=stats(ms["first1"]),
                            detect_chains_Mframes_per_s=n_clips * n_frames / med["chains"] / 1e3,
                            track_first0_Mframes_per_s=n_clips * n_frames / med["first0"] / 1e3,
                            track_first1_Mframes_per_s=n_clips * (n_frames - 1) / med["first1"] / 1e3,
                            first0_over_chains=med["first0"] / med["chains"], first1_over_chains=med["first1"] / med["chains"],
                            first0_batches=batches, first0_took_chains_fast_path=bool(after[3] > before[3]),
                            first0_launches_beside_the_batches=0 if after[3] > before[3] else 2 + n_frames,
                            first0_equal_to_chains=same))
        del frames
        torch.cuda.empty_cache()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("modes", "track", "all"), default="all")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "clips_bench measures on the GPU"
    import pawsometracker_jl_amd as pt
    results = []

    def emit(r):
        r["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(r), flush=True)
        results.append(r)

    if args.case in ("modes", "all"):
        rate = copy_rate()
        emit(dict(case="copy_rate", read_plus_write_TBps=rate / 1e12))
        for name, n, h, w in (("4096x240x320", 4096, 240, 320), ("256x1080p", 256, 1080, 1920), ("1x4k", 1, 2160, 3840)):
            emit(run_modes(pt, name, n, h, w, args.reps, args.warmup, rate))
            torch.cuda.empty_cache()
    if args.case in ("track", "all"):
        for r in run_track(pt, args.clips, args.frames, max(5, args.reps // 2), args.warmup):
            emit(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
