#!/usr/bin/env python3
"""What the overlay over a frame table costs (pdog_diag_render_indexed) against what a user paid before: gather the selected
frames into a second stack, then pdog_diag_render over the copy.

video:  the 2000-frame 1080p video of tools/video_bench.py, 30 -> 24 positions per second (1600 steps, 1599 rendered: the
        bootstrap frame is not drawn), in chunks of 256 steps into one reused buffer, for 1, 8 and 64 targets whose
        positions are the indexed chain's (45x45 windows); for one target also the contiguous render over the gathered
        copy, in the same chunks, and the gather on its own; the chain's time beside them.
small:  the 100x100 case of the tests (60 frames, 48 steps, two targets, chunks of 7).

Device events, medians of --reps samples after --warmup calls of each leg, all legs of a case alternated sample by sample;
"spread" is (max - min) / median of a leg's samples.  One JSON line per case; --out FILE writes them all
(profiles/overlay_bench.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from tools.video_bench import alternate, make_video, stats  # noqa: E402


def chunks(n, chunk):
    return [(k0, min(n, k0 + chunk)) for k0 in range(1, n, chunk)]


def run_case(pt, name, frames, first_pos, rate, fps, tw, ws, targets, chunk, reps, warmup):
    import torch
    n, h, w = frames.shape
    table = pt.fps_table(rate, n, 0.0, pt.DEFAULT_STOP, fps)
    m = len(table)
    cuts = chunks(m, chunk)
    buf = torch.empty((min(chunk, m - 1), 360, 640), dtype=torch.uint8, device="cuda")
    bt = pt.BatchTracker(h, w, tw, ws, True, 128)
    r = dict(case=name, frames=n, frame_h=h, frame_w=w, rate=rate, fps=fps, steps=m, rendered=m - 1, chunk=chunk, window=list(ws),
             target_width=tw, reps=reps, warmup=warmup)
    calls, keep = {}, []
    for nt in targets:
        start = np.stack([first_pos[k % len(first_pos)] + (k // len(first_pos)) * np.array([1, -1]) for k in range(nt)]).astype(np.int32)
        starts, tab = torch.from_numpy(start).cuda(), np.tile(table, (nt, 1))
        ij = torch.empty((nt, m, 2), dtype=torch.int32, device="cuda")
        dia = pt.Diagnose(True)
        dia.set_targets(nt)
        keep.append(dia)

        def chain(starts=starts, tab=tab, ij=ij):
            bt.detect_chains_indexed(frames, tab, starts, first=1, out=ij)

        def indexed(dia=dia, ij=ij):
            for k0, k1 in cuts:
                dia.render_indexed(frames, table[k0:k1], ij[:, k0:k1], out=buf[:k1 - k0])
        chain()
        calls[f"chain_{nt}"] = chain
        calls[f"indexed_{nt}"] = indexed
        if nt == 1:         # what a user paid before: a second stack of the selected frames, then the contiguous render
            d_tab = torch.from_numpy(np.ascontiguousarray(table[1:])).long().cuda()
            copy = torch.empty((m - 1, h, w), dtype=torch.uint8, device="cuda")
            plain = pt.Diagnose(True)
            keep.append(plain)
            r["copy_bytes"] = int(copy.numel())

            def gather(d_tab=d_tab, copy=copy):
                torch.index_select(frames, 0, d_tab, out=copy)

            def contiguous(plain=plain, copy=copy, ij=ij):
                for k0, k1 in cuts:
                    plain(copy[k0 - 1:k1 - 1], ij[0, k0:k1], out=buf[:k1 - k0])
            gather()
            calls["gather"] = gather
            calls["contiguous_1"] = contiguous
            # the two renders draw the same bytes (fresh traces, last chunk)
            a, b = pt.Diagnose(True), pt.Diagnose(True)
            k0, k1 = cuts[-1]
            x = a.render_indexed(frames, table[k0:k1], ij[:, k0:k1]).clone()
            r["equal"] = bool(torch.equal(x, b(copy[k0 - 1:k1 - 1], ij[0, k0:k1])))
            a.close()
            b.close()
    ms = alternate(calls, reps, warmup)
    bt.sync()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    r["ms"] = {k: stats(v) for k, v in ms.items()}
    if "contiguous_1" in med:
        r.update(indexed_over_contiguous=med["indexed_1"] / med["contiguous_1"],
                 indexed_over_gather_plus_contiguous=med["indexed_1"] / (med["gather"] + med["contiguous_1"]),
                 condition_met=bool(med["indexed_1"] <= med["gather"] + med["contiguous_1"]))
    ts = sorted(targets)
    if len(ts) > 1:         # overlay launches only: the resize does not depend on the number of targets
        r["us_per_added_target"] = {f"{a}->{b}": (med[f"indexed_{b}"] - med[f"indexed_{a}"]) * 1e3 / (b - a) for a, b in zip(ts, ts[1:])}
    r["indexed_us_per_rendered_frame"] = {str(nt): med[f"indexed_{nt}"] * 1e3 / (m - 1) for nt in targets}
    for d in keep:
        d.close()
    bt.close()
    torch.cuda.empty_cache()
    return r


def small_video(n, h, w, tw):
    """The 100 x 100 stack of tests/test_gpu_overlay.py: two dark discs on separate paths."""
    import torch
    from oracle import synth
    paths = [[(20 + k // 3, 20 + k) for k in range(n)], [(82 - k // 4, 85 - k) for k in range(n)]]
    frames = np.stack([np.minimum(synth.disc_frame(h, w, paths[0][k], tw, True), synth.disc_frame(h, w, paths[1][k], tw, True)) for k in range(n)])
    return torch.from_numpy(frames).cuda(), np.array([paths[0][0], paths[1][0]], np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("video", "small", "all"), default="all")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--video-frames", type=int, default=2000)
    ap.add_argument("--targets", default="1,8,64")
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "overlay_bench measures on the GPU"
    import pawsometracker_jl_amd as pt
    results = []

    def emit(r):
        r.update(device=torch.cuda.get_device_name(0), library=os.path.basename(pt.LIB_PATH))
        print(json.dumps(r), flush=True)
        results.append(r)

    if args.case in ("small", "all"):
        frames, first_pos = small_video(60, 100, 100, 10)
        emit(run_case(pt, "small_100x100", frames, first_pos, 30, 24, 10, (21, 21), [1, 2], 7, args.reps, args.warmup))
    if args.case in ("video", "all"):
        frames, first_pos = make_video(args.video_frames, 1080, 1920, 25, 8)
        emit(run_case(pt, "video_1080p", frames, first_pos, 30, 24, 25, (45, 45), [int(v) for v in args.targets.split(",")], args.chunk,
                      args.reps, args.warmup))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
