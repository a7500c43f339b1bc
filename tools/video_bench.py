#!/usr/bin/env python3
"""What a frame table costs (pdog_detect_chains_indexed) against the contiguous chain (pdog_detect_chains) on the same data.

clips:  4096 clips x 32 frames of 240x320, 45x45 windows (the shape of profiles/clips_bench.json), identity table.
video:  one 1080p video of 2000 frames, 30 -> 24 positions per second (1600 steps), 1, 8 and 64 targets sharing it, 45x45
        and 257x257 windows: us per frame and target through the table, and what the library offered before — gather the
        selected frames into K contiguous copies and run the contiguous chain over them — with the bytes of HBM that needs
        ("does not fit" where the copies do not fit beside the video).

Device events, medians of --reps samples after --warmup calls, the indexed and the contiguous chain alternated (the gather
of the copies is timed on its own, before them, with fewer samples where the copies exceed 16 GB); the clips case also reports
the host's time inside one call of each.  With PAWSOME_DOG_LIB naming a
build without the indexed entry point (the parent's) only the contiguous legs run: the yardstick in that build.
One JSON line per case; --out FILE writes them all (profiles/video_bench.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(calls, reps, warmup):
    """{name: [ms, ...]}: `reps` samples of every call, alternated, after `warmup` calls of each."""
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            ms[k].append(timed(fn))
    return ms


def host_time(fn, bt, reps):
    """Median ms the HOST spends inside one call (the call is asynchronous: it returns once everything is queued), the
    stream drained before each sample: for the indexed chain that is the table's check, its copy to pinned memory and
    the queueing of the upload, all of which lie in front of the launch."""
    import time
    t = []
    for _ in range(reps):
        bt.sync()
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    bt.sync()
    return float(np.median(t))


def stats(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)), spread=float((max(ms) - min(ms)) / np.median(ms)))


def make_video(n, h, w, tw, n_discs, seed=0, chunk=50):
    """uint8 cuda [n, h, w]: n_discs dark discs on slow random walks over a 128 +- 2 background; their first places."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    pos = np.cumsum(rng.integers(-3, 4, (n, n_discs, 2)), 0) + rng.integers([60, 60], [h - 60, w - 60], (1, n_discs, 2))
    pos = np.clip(pos, 40, [h - 40, w - 40]).astype(np.int32)
    frames = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    ii = torch.arange(1, h + 1, device="cuda").view(1, h, 1)
    jj = torch.arange(1, w + 1, device="cuda").view(1, 1, w)
    d_pos = torch.from_numpy(pos).cuda()
    for k0 in range(0, n, chunk):
        k1 = min(n, k0 + chunk)
        img = 128 + torch.randint(-2, 3, (k1 - k0, h, w), dtype=torch.int16, device="cuda", generator=g)
        for d in range(n_discs):
            p = d_pos[k0:k1, d]
            img[(ii - p[:, 0, None, None]) ** 2 + (jj - p[:, 1, None, None]) ** 2 <= (tw // 2) ** 2] = 0
        frames[k0:k1] = img.to(torch.uint8)
    return frames, pos[0]


def run_clips(pt, n_clips, n_frames, reps, warmup, indexed):
    import torch
    from tools.clips_bench import make_clips
    h, w, tw, ws = 240, 320, 25, (45, 45)
    frames, start = make_clips(n_clips, n_frames, h, w, tw, np.full(n_clips, 128))
    starts = torch.from_numpy(start).cuda()
    bt = pt.BatchTracker(h, w, tw, ws, True, 128)
    ref = torch.empty((n_clips, n_frames, 2), dtype=torch.int32, device="cuda")
    out = torch.empty_like(ref)
    flat = frames.flatten(0, 1)
    table = np.arange(n_clips * n_frames, dtype=np.int32).reshape(n_clips, n_frames)
    calls = dict(contiguous=lambda: bt.detect_chains(frames, starts, out=ref))
    if indexed:
        calls["indexed"] = lambda: bt.detect_chains_indexed(flat, table, starts, out=out)
    ms = alternate(calls, reps, warmup)
    bt.sync()
    host = {k: host_time(fn, bt, reps) for k, fn in calls.items()}
    r = dict(case="clips_identity", clips=n_clips, frames_per_clip=n_frames, frame_h=h, frame_w=w, window=list(ws), target_width=tw,
             reps=reps, warmup=warmup, contiguous_ms=stats(ms["contiguous"]),
             contiguous_us_per_frame=float(np.median(ms["contiguous"])) * 1e3 / (n_clips * n_frames))
    if indexed:
        r.update(indexed_ms=stats(ms["indexed"]), indexed_over_contiguous=float(np.median(ms["indexed"]) / np.median(ms["contiguous"])),
                 table_bytes=int(table.nbytes), equal=bool(torch.equal(out, ref)),
                 host_ms_per_call=dict(contiguous=host["contiguous"], indexed=host["indexed"]))
    bt.close()
    return r


def run_video(pt, frames, first_pos, rate, fps, ws, n_targets, reps, warmup, indexed):
    import torch
    n, h, w = frames.shape
    tw = 25
    table = pt.fps_table(rate, n, 0.0, pt.DEFAULT_STOP, fps) if indexed else np.floor(np.arange(int(n * fps / rate)) * rate / fps + 0.5).astype(np.int32)
    m = len(table)
    start = np.stack([first_pos[k % len(first_pos)] + (k // len(first_pos)) * np.array([1, -1]) for k in range(n_targets)]).astype(np.int32)
    starts = torch.from_numpy(start).cuda()
    bt = pt.BatchTracker(h, w, tw, ws, True, 128)
    r = dict(case="video", frames=n, frame_h=h, frame_w=w, rate=rate, fps=fps, steps=m, targets=n_targets, window=list(ws), target_width=tw,
             reps=reps, warmup=warmup, video_bytes=int(frames.numel()))
    out, tab = None, None
    calls = {}
    if indexed:
        out = torch.empty((n_targets, m, 2), dtype=torch.int32, device="cuda")
        tab = np.tile(table, (n_targets, 1))
        calls["indexed"] = lambda: bt.detect_chains_indexed(frames, tab, starts, out=out)
        r["table_bytes"] = int(tab.nbytes)
    # what the library offered before: K contiguous copies of the selected frames, then the contiguous chain over them
    need = n_targets * m * h * w
    r["copies_bytes"] = int(need)
    free, _ = torch.cuda.mem_get_info()
    fits = need + (2 << 30) <= free
    r["copies"] = "fit" if fits else "does not fit"
    copies = None
    if fits:
        d_tab = torch.from_numpy(np.ascontiguousarray(table)).long().cuda()
        copies = torch.empty((n_targets, m, h, w), dtype=torch.uint8, device="cuda")
        ref = torch.empty((n_targets, m, 2), dtype=torch.int32, device="cuda")

        def gather():
            for k in range(n_targets):
                torch.index_select(frames, 0, d_tab, out=copies[k])
        few = max(3, reps // 4) if need > (16 << 30) else reps
        g = alternate(dict(gather=gather), few, min(warmup, 2))["gather"]       # (leaves the copies filled)
        r.update(gather_reps=few, gather_ms=stats(g))
        calls["contiguous"] = lambda: bt.detect_chains(copies, starts, out=ref)
    ms = alternate(calls, reps, warmup)                                          # the two chains alternated, `reps` samples each
    bt.sync()
    if indexed:
        r.update(indexed_ms=stats(ms["indexed"]), indexed_us_per_frame_and_target=float(np.median(ms["indexed"])) * 1e3 / (m * n_targets))
    if fits:
        gm, c = float(np.median(g)), float(np.median(ms["contiguous"]))
        r.update(contiguous_ms=stats(ms["contiguous"]), contiguous_us_per_frame_and_target=c * 1e3 / (m * n_targets),
                 gather_plus_contiguous_us_per_frame_and_target=(gm + c) * 1e3 / (m * n_targets))
        if indexed:
            r.update(equal=bool(torch.equal(out, ref)), indexed_over_contiguous=float(np.median(ms["indexed"])) / c)
    del copies
    bt.close()
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("clips", "video", "all"), default="all")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--video-frames", type=int, default=2000)
    ap.add_argument("--targets", default="1,8,64")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "video_bench measures on the GPU"
    import pawsometracker_jl_amd as pt
    indexed = hasattr(pt.lib(), "pdog_detect_chains_indexed")
    results = []

    def emit(r):
        r.update(device=torch.cuda.get_device_name(0), library=os.path.basename(pt.LIB_PATH), has_indexed=indexed)
        print(json.dumps(r), flush=True)
        results.append(r)

    if args.case in ("clips", "all"):
        emit(run_clips(pt, args.clips, args.frames, args.reps, args.warmup, indexed))
        torch.cuda.empty_cache()
    if args.case in ("video", "all"):
        frames, first_pos = make_video(args.video_frames, 1080, 1920, 25, 8)
        for ws in ((45, 45), (257, 257)):
            for k in (int(v) for v in args.targets.split(",")):
                emit(run_video(pt, frames, first_pos, 30, 24, ws, k, args.reps, args.warmup, indexed))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
