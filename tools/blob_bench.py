#!/usr/bin/env python3
"""pdog_blob (blob_kernel) against pdog_shape (shape_kernel) on the same positions: frames resident in HBM, device events after
warm-up, the two calls alternated sample by sample in one session.  Cases:
  p4096       4096 positions at R = 25 (the wave tier) on 64 frames of 1080p (tools/shape_bench.py's frames and positions)
  p1024_r127  1024 positions at R = 127 (the workgroup tier) on the same frames
  chains      the 131 072 positions of a 4096 x 32 detect_chains call (240 x 320) at R = 25
  comb_r127   ONE position at R = 127 on the adversarial mask of tests/blob_scenes.py (the vertical comb: a serpentine of pitch 2,
              one sweep per row of way) against the same call on the same mask transposed (corridors along the rows, which the
              run-fill crosses in one sweep each): what the sweeps cost
Every case holds pdog_blob's integers to pdog_shape's where the mask is one component (n == n_mask) before anything is timed.
With PAWSOME_DOG_LIB naming the ablation build (make diag) every case also reports the sweeps per position (its counter,
pdog_blob_debug_sweeps); with it naming a build without pdog_blob (the parent's) only the pdog_shape leg runs: the yardstick in
that build.  One JSON line per case; --out FILE also writes them all to FILE."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

from shape_bench import disc_frames, positions_on  # noqa: E402
from video_bench import alternate, stats  # noqa: E402


def sweeps_of(pt, bt, call, n):
    """The ablation build's counter around one call: uint32 [n] on the host, or None in a build without it."""
    import torch
    fn = getattr(pt.lib(), "pdog_blob_debug_sweeps", None)
    if fn is None:
        return None
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
    buf = torch.zeros(n, dtype=torch.int32, device="cuda")
    assert fn(C.c_void_p(buf.data_ptr())) == 0
    call()
    bt.sync()
    assert fn(None) == 0
    return buf.cpu().numpy().astype(np.int64)


def run_case(pt, name, bt, frames, ij, fi, R, reps, warmup):
    import torch
    n = ij.shape[0]
    has_blob = hasattr(pt.lib(), "pdog_blob")
    calls = {"shape": lambda: bt.shapes(frames, ij, fi, R, 8)}
    r = dict(case=name, positions=n, radius=R, frame_h=int(frames.shape[1]), frame_w=int(frames.shape[2]), reps=reps, warmup=warmup)
    if has_blob:
        _, ssum = bt.shapes(frames, ij, fi, R, 8, want_sums=True)
        for conn in (4, 8):
            _, bsum = bt.blobs(frames, ij, fi, R, 8, conn, want_sums=True)
            one = bsum[:, 0] == bsum[:, 8]
            r[f"one_component_{conn}"] = float(one.double().mean())
            r[f"integers_equal_shape_where_one_component_{conn}"] = bool(torch.equal(bsum[one, :8], ssum[one]) and torch.equal(bsum[:, 8], ssum[:, 0]))
            calls[f"blob{conn}"] = (lambda conn=conn: bt.blobs(frames, ij, fi, R, 8, conn))
            sw = sweeps_of(pt, bt, calls[f"blob{conn}"], n)
            if sw is not None:
                r[f"sweeps_{conn}"] = dict(mean=float(sw.mean()), median=float(np.median(sw)), max=int(sw.max()))
        r["masks_not_empty"] = float((ssum[:, 0] > 0).double().mean())
    ms = alternate(calls, reps, warmup)
    r["ms"] = {k: stats(v) for k, v in ms.items()}
    r["shape_us_per_position"] = float(np.median(ms["shape"])) * 1e3 / n
    if has_blob:
        for conn in (4, 8):
            r[f"blob{conn}_over_shape"] = float(np.median(ms[f"blob{conn}"]) / np.median(ms["shape"]))
    return r


def run_chains(pt, reps, warmup, n_clips, n_frames=32):
    import torch
    from bench import make_clip
    fh, fw, tw, ws = 240, 320, 25, (45, 45)
    base_h, centres = make_clip(np, n_frames, fh, fw, tw, (22, 22), seed=0, noise=0)
    base = torch.from_numpy(base_h).cuda().to(torch.int16)
    frames = torch.empty((n_clips, n_frames, fh, fw), dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    for c0 in range(0, n_clips, 128):
        nz = torch.randint(-3, 4, (min(128, n_clips - c0), n_frames, fh, fw), dtype=torch.int16, device="cuda", generator=g)
        frames[c0:c0 + nz.shape[0]] = (base[None] + nz).clamp_(0, 255).to(torch.uint8)
    del base
    starts = torch.tensor([[int(centres[0, 0]), int(centres[0, 1])]] * n_clips, dtype=torch.int32, device="cuda")
    with pt.BatchTracker(fh, fw, tw, ws, True, 128) as bt:
        out = bt.detect_chains(frames, starts)
        bt.sync()
        flat, pos = frames.flatten(0, 1), out.view(-1, 2)
        fi = torch.arange(pos.shape[0], dtype=torch.int32, device="cuda")
        r = run_case(pt, "chains", bt, flat, pos, fi, 25, reps, warmup)
        bt.sync()
    r.update(clips=n_clips, frames_per_clip=n_frames)
    return r


def run_comb(pt, reps, warmup):
    """One position at R = 127: the vertical comb of tests/blob_scenes.py and the same mask transposed."""
    import torch
    import blob_scenes as BLS
    c, flat = BLS.geodesic(127, "vertical comb"), BLS.geodesic(127, "horizontal comb")
    ij = torch.from_numpy(c.ij).cuda()
    out = dict(case="comb_r127", positions=1, radius=127, reps=reps, warmup=warmup)
    with pt.BatchTracker(BLS.BIG, BLS.BIG, 25, (45, 45), True, 128) as bt:
        calls = {}
        for name, f in (("comb", c.frames), ("transposed", flat.frames)):
            d = torch.from_numpy(f).cuda()
            calls[f"shape_{name}"] = (lambda d=d: bt.shapes(d, ij, None, 127, 8))
            if hasattr(pt.lib(), "pdog_blob"):
                calls[f"blob4_{name}"] = (lambda d=d: bt.blobs(d, ij, None, 127, 8, 4))
                _, s = bt.blobs(d, ij, None, 127, 8, 4, want_sums=True)
                out[f"pixels_{name}"] = int(s[0, 0])
                sw = sweeps_of(pt, bt, calls[f"blob4_{name}"], 1)
                if sw is not None:
                    out[f"sweeps_{name}"] = int(sw[0])
        ms = alternate(calls, reps, warmup)
        bt.sync()
    out["ms"] = {k: stats(v) for k, v in ms.items()}
    if "blob4_comb" in ms:
        extra = float(np.median(ms["blob4_comb"]) - np.median(ms["blob4_transposed"]))
        out["comb_minus_transposed_ms"] = extra
        if "sweeps_comb" in out:
            out["us_per_sweep"] = extra * 1e3 / max(out["sweeps_comb"] - out["sweeps_transposed"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("p4096", "chains", "p1024_r127", "comb_r127", "all"), default="all")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "blob_bench measures on the GPU"
    import pawsometracker_jl_amd as pt
    todo = ("p4096", "p1024_r127", "comb_r127", "chains") if args.case == "all" else (args.case,)
    results = []
    frames = centres = None
    for case in todo:
        if case in ("p4096", "p1024_r127"):
            if frames is None:
                frames, centres = disc_frames(64, 1080, 1920, 32)
            n, R = (4096, 25) if case == "p4096" else (1024, 127)
            ij, fi = positions_on(centres, n)
            with pt.BatchTracker(1080, 1920, 25, (45, 45), True, 128) as bt:
                r = run_case(pt, case, bt, frames, ij, fi, R, args.reps, args.warmup)
                bt.sync()
        else:
            frames = centres = None
            torch.cuda.empty_cache()
            r = run_comb(pt, args.reps, args.warmup) if case == "comb_r127" else run_chains(pt, args.reps, args.warmup, args.clips)
        r["device"] = torch.cuda.get_device_name(0)
        r["library"] = os.path.basename(pt.LIB_PATH)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
