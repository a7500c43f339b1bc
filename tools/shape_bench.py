#!/usr/bin/env python3
"""pdog_shape (shape_kernel) on the GPU.  Cases, frames resident in HBM, device events after warm-up, the compared calls
alternated in one session:
  p4096       4096 positions at R = 25 on 64 frames of 1080p (floor 128 +- 2, dark discs of width 25; the positions on and
              around the discs)
  chains      the 131 072 positions of a 4096 x 32 detect_chains call (240 x 320, a dark disc on a spiral, +- 3 levels of noise)
              at R = 25
  p1024_r127  1024 positions at R = 127 on the 1080p frames
Every case sets the call against (i) pdog_measure on the same positions with the same tracker (target_width 25, l = 65), (ii) a
torch formulation a user would write — gather the patches, sort for the median, masked sums, in chunks of positions that fit
memory — and (iii) a device copy of the patches' bounding boxes (a torch gather into a dense tensor).  The torch formulation's
sums are held against the call's, all of them, before anything is timed.
  video       track_video on the 2000-frame 1080p video of tools/video_bench.py (8 targets), with and without shape=True
One JSON line per case; --out FILE also writes them all to FILE."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

from video_bench import alternate, make_video, stats  # noqa: E402


def torch_patches(frames, ij, fi, R, fill):
    """The bounding boxes of the patches, [n, D, D] uint8, the fill outside the frame: what (iii) copies and (ii) starts from."""
    import torch
    nf, h, w = frames.shape
    d = torch.arange(-R, R + 1, device=frames.device)
    i = ij[:, 0].long().clamp(1, h) - 1
    j = ij[:, 1].long().clamp(1, w) - 1
    rows = i[:, None] + d[None, :]
    cols = j[:, None] + d[None, :]
    inside = ((rows >= 0) & (rows < h))[:, :, None] & ((cols >= 0) & (cols < w))[:, None, :]
    flat = (fi.long()[:, None, None] * h + rows.clamp(0, h - 1)[:, :, None]) * w + cols.clamp(0, w - 1)[:, None, :]
    p = frames.reshape(-1)[flat]
    return torch.where(inside, p, torch.full_like(p, fill))


def torch_shapes(frames, ij, fi, R, fill, darker, min_contrast, chunk):
    """Steps 1 - 6 of the rule in torch: sums int64 [n, 8]."""
    import torch
    d = torch.arange(-R, R + 1, device=frames.device)
    dy, dx = d[:, None].expand(2 * R + 1, 2 * R + 1), d[None, :].expand(2 * R + 1, 2 * R + 1)
    disc = (dy * dy + dx * dx <= R * R).reshape(-1)
    y, x = dy.reshape(-1)[disc].long(), dx.reshape(-1)[disc].long()
    rank = (int(disc.sum()) - 1) // 2
    out = []
    for k0 in range(0, ij.shape[0], chunk):
        p = torch_patches(frames, ij[k0:k0 + chunk], fi[k0:k0 + chunk], R, fill)
        centre = p[:, R - 1:R + 2, R - 1:R + 2].reshape(-1, 9).long()
        v = p.reshape(p.shape[0], -1)[:, disc]
        b = v.sort(dim=1).values[:, rank].long()
        s = (b[:, None] - v.long()) if darker else (v.long() - b[:, None])
        s3 = (b[:, None] - centre) if darker else (centre - b[:, None])
        c = s3.max(dim=1).values.clamp(min=0)
        m = ((2 * s >= c[:, None]) & (c >= min_contrast)[:, None]).long()
        out.append(torch.stack([m.sum(1), (m * y).sum(1), (m * x).sum(1), (m * y * y).sum(1), (m * y * x).sum(1), (m * x * x).sum(1), b, c], 1))
    return torch.cat(out)


def run_case(name, bt, frames, ij, fi, R, reps, warmup, chunk):
    import torch
    n = ij.shape[0]
    fill, darker = bt.info().fill, bool(bt.info().darker_target)
    shp, sums = bt.shapes(frames, ij, fi, R, 8, want_sums=True)
    ref = torch_shapes(frames, ij, fi, R, fill, darker, 8, chunk)
    ok = bool(torch.equal(sums.long(), ref))
    calls = {
        "shape": lambda: bt.shapes(frames, ij, fi, R, 8),
        "shape_sums_only": lambda: bt.shapes(frames, ij, fi, R, 8, want_sums=True),
        "measure": lambda: bt.measure(frames, ij, fi),
        "torch": lambda: torch_shapes(frames, ij, fi, R, fill, darker, 8, chunk),
        "patch_copy": lambda: [torch_patches(frames, ij[k:k + chunk], fi[k:k + chunk], R, fill) for k in range(0, n, chunk)],
    }
    ms = alternate(calls, reps, warmup)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    D = 2 * R + 1
    return dict(case=name, positions=n, radius=R, frame_h=int(frames.shape[1]), frame_w=int(frames.shape[2]), reps=reps, warmup=warmup,
                ms={k: stats(v) for k, v in ms.items()}, shape_us_per_position=med["shape"] * 1e3 / n,
                shape_over_measure=med["shape"] / med["measure"], shape_over_torch=med["shape"] / med["torch"],
                shape_over_patch_copy=med["shape"] / med["patch_copy"], patch_bytes=n * D * D,
                patch_gbytes_per_s=n * D * D / (med["shape"] * 1e-3) / 1e9, masks_not_empty=float((sums[:, 0] > 0).double().mean()),
                sums_equal_the_torch_formulation=ok)


def disc_frames(nf, h, w, per_frame, seed=0):
    """uint8 cuda [nf, h, w]: floor 128 +- 2 and per_frame dark discs of width 25 per frame; their centres [nf, per_frame, 2], 1-based."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    c = np.stack([rng.integers(1, h + 1, (nf, per_frame)), rng.integers(1, w + 1, (nf, per_frame))], 2).astype(np.int32)
    frames = (128 + torch.randint(-2, 3, (nf, h, w), dtype=torch.int16, device="cuda", generator=g)).to(torch.uint8)
    ii = torch.arange(1, h + 1, device="cuda").view(h, 1)
    jj = torch.arange(1, w + 1, device="cuda").view(1, w)
    for k in range(nf):
        for ci, cj in c[k]:
            i0, i1, j0, j1 = max(ci - 13, 0), min(ci + 12, h), max(cj - 13, 0), min(cj + 12, w)
            box = frames[k, i0:i1, j0:j1]
            box[(ii[i0:i1] - int(ci)) ** 2 + (jj[:, j0:j1] - int(cj)) ** 2 <= 144] = 0
    return frames, c


def positions_on(c, n, seed=1):
    """n positions on and around the discs of disc_frames, and their frames."""
    import torch
    rng = np.random.default_rng(seed)
    nf, per, _ = c.shape
    k = rng.integers(0, nf, n)
    d = rng.integers(0, per, n)
    ij = c[k, d] + rng.integers(-6, 7, (n, 2))
    return torch.from_numpy(ij.astype(np.int32)).cuda(), torch.from_numpy(k.astype(np.int32)).cuda()


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
        r = run_case("chains", bt, flat, pos, fi, 25, reps, warmup, 8192)
        ms = alternate({"chain": lambda: bt.detect_chains(frames, starts, out=out)}, reps, warmup)
        bt.sync()
    r["chain_ms"] = stats(ms["chain"])
    r["shape_over_chain"] = r["ms"]["shape"]["median"] / r["chain_ms"]["median"]
    r.update(clips=n_clips, frames_per_clip=n_frames)
    return r


def run_video(pt, reps, warmup, n_frames, n_targets=8):
    import torch
    h, w, tw = 1080, 1920, 25
    frames, first = make_video(n_frames, h, w, tw, n_targets)
    kw = dict(rate=30, start=0, stop=n_frames / 30, fps=24, target_width=tw, window_size=45, darker_target=True,
              start_locations=[("ij", (int(p[0]), int(p[1]))) for p in first])
    plain = pt.track_video(frames, **kw)
    res = pt.track_video(frames, shape=True, **kw)
    same = bool(torch.equal(plain[1], res[1]))
    ms = alternate({"track_video": lambda: pt.track_video(frames, **kw), "track_video_shape": lambda: pt.track_video(frames, shape=True, **kw)},
                   reps, warmup)
    width = res[2][..., 5]
    return dict(case="video", frames=n_frames, steps=int(res[1].shape[1]), targets=n_targets, frame_h=h, frame_w=w, reps=reps, warmup=warmup,
                ms={k: stats(v) for k, v in ms.items()},
                shape_adds=float(np.median(ms["track_video_shape"]) / np.median(ms["track_video"]) - 1.0), indices_unchanged=same,
                median_width=float(width[~torch.isnan(width)].median()), shapes_not_nan=float((~torch.isnan(width)).double().mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("p4096", "chains", "p1024_r127", "video", "all"), default="all")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--video-frames", type=int, default=2000)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "shape_bench measures on the GPU"
    import pawsometracker_jl_amd as pt
    todo = ("p4096", "p1024_r127", "chains", "video") if args.case == "all" else (args.case,)
    results = []
    frames = centres = None
    for case in todo:
        if case in ("p4096", "p1024_r127"):
            if frames is None:
                frames, centres = disc_frames(64, 1080, 1920, 32)
            n, R, chunk = (4096, 25, 4096) if case == "p4096" else (1024, 127, 256)
            ij, fi = positions_on(centres, n)
            with pt.BatchTracker(1080, 1920, 25, (45, 45), True, 128) as bt:
                r = run_case(case, bt, frames, ij, fi, R, args.reps, args.warmup, chunk)
                bt.sync()
        else:
            frames = centres = None
            torch.cuda.empty_cache()
            r = run_chains(pt, args.reps, args.warmup, args.clips) if case == "chains" else run_video(pt, max(3, args.reps // 2), 1, args.video_frames)
        r["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
