#!/usr/bin/env python3
"""pdog_measure (dog_measure_kernel) on the GPU.  Cases, frames resident in HBM, one call per step, device events after
warm-up, median of the repeats:
  1080p    4096 positions on 64 frames of 1080p noise, target_width 25 (l = 65): five 4 225-term Float64 chains per position
  1080p_1  the same tracker, ONE position: the latency floor of a call
  l293     4096 positions on the same frames, target_width 120 (l = 293): five 85 849-term chains per position
  chains   4096 clips x 32 frames of 240x320 (a dark disc on a spiral, +-3 levels of noise), 45x45 windows, target_width
           25: detect_chains alone, detect_chains followed by measure on its 131 072 positions, and measure alone —
           alternated in one session; the cost of the measurement as a fraction of the chain it follows
Every measure time is taken for both layouts of the kernel, alternated: each position's pixel tile staged in LDS (the
default) and the frame read in place (pdog_set_tuning "measure_global": the path of kernels too long for a tile).
Every case checks a handful of its outputs bit for bit against tests/measure_restatement.py and the two layouts against
each other.  One JSON line per case;
--out FILE also writes them all to FILE."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402


def timed(fn, reps):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def stats(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def check(oracle, frames_t, fill, tw, darker, ij_t, fi_t, sub_t, r5_t, k=6):
    """The first k positions against the restatement, bit for bit."""
    import measure_restatement as R
    K = oracle.dog_kernel(oracle.sigma(tw), darker)
    ij = ij_t[:k].cpu().numpy()
    fi = fi_t[:k].cpu().numpy() if fi_t is not None else np.arange(k)
    frames = [frames_t[int(f)].cpu().numpy() for f in fi]
    ref_sub, ref_r5 = R.measure(oracle, frames, fill, K, ij)
    eq = lambda a, b: bool(np.array_equal(np.ascontiguousarray(a).view(np.uint64), b.view(np.uint64)))
    return eq(sub_t[:k].cpu().numpy(), ref_sub) and eq(r5_t[:k].cpu().numpy(), ref_r5)


def run_positions(name, oracle, tw, n, reps, warmup, frames):
    import torch
    import pawsometracker_jl_amd as pt
    nf, h, w = frames.shape
    rng = np.random.default_rng(1)
    ij = torch.from_numpy(np.stack([rng.integers(1, h + 1, n), rng.integers(1, w + 1, n)], 1).astype(np.int32)).cuda()
    fi = torch.from_numpy(rng.integers(0, nf, n).astype(np.int32)).cuda()
    bt = pt.BatchTracker(h, w, tw, pt.fix_window_size(pt.guess_window_size(tw)), True, 128)
    l = bt.info().kernel_len
    call = lambda: bt.measure(frames, ij, frame_index=fi, want_resp=True)
    ms, ms_global = [], []
    for layout, acc in ((0, ms), (1, ms_global)):
        bt.set_tuning("measure_global", layout)
        for _ in range(warmup):
            call()
    for _ in range(reps):                                   # alternated: LDS tiles, frame reads, LDS tiles, ...
        for layout, acc in ((0, ms), (1, ms_global)):
            bt.set_tuning("measure_global", layout)
            acc += timed(call, 1)
    sub_g, r5_g = call()
    bt.set_tuning("measure_global", 0)
    sub, r5 = call()
    bt.sync()
    ok = check(oracle, frames, 128, tw, True, ij, fi, sub, r5) and torch.equal(sub, sub_g) and torch.equal(r5, r5_g)
    bt.close()
    med = float(np.median(ms))
    terms = 5 * n * l * l
    return dict(case=name, positions=n, frame_h=h, frame_w=w, target_width=tw, kernel_len=l, reps=reps, warmup=warmup,
                ms_per_call=stats(ms), ms_per_call_reading_the_frame=stats(ms_global), us_per_position=med * 1e3 / n, terms_per_call=terms,
                float64_mul_add_pairs_per_s=terms / (med * 1e-3), checked_against_restatement=ok)


def run_chains(oracle, reps, warmup, n_clips=4096, n_frames=32):
    import torch
    import pawsometracker_jl_amd as pt
    from bench import make_clip
    fh, fw, tw, ws = 240, 320, 25, (45, 45)
    base_h, centres = make_clip(np, n_frames, fh, fw, tw, (22, 22), seed=0, noise=0)
    base = torch.from_numpy(base_h).cuda().to(torch.int16)
    frames = torch.empty((n_clips, n_frames, fh, fw), dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    for c0 in range(0, n_clips, 128):                       # every clip its own +-3 levels of noise
        nz = torch.randint(-3, 4, (min(128, n_clips - c0), n_frames, fh, fw), dtype=torch.int16, device="cuda", generator=g)
        frames[c0:c0 + nz.shape[0]] = (base[None] + nz).clamp_(0, 255).to(torch.uint8)
    del base
    starts = torch.tensor([[int(centres[0, 0]), int(centres[0, 1])]] * n_clips, dtype=torch.int32, device="cuda")
    fill = 128
    bt = pt.BatchTracker(fh, fw, tw, ws, True, fill)
    out = torch.empty((n_clips, n_frames, 2), dtype=torch.int32, device="cuda")
    flat, pos = frames.flatten(0, 1), out.view(-1, 2)

    def chain():
        bt.detect_chains(frames, starts, out=out)

    def both():
        bt.detect_chains(frames, starts, out=out)
        bt.measure(flat, pos)

    def measure():
        bt.measure(flat, pos)

    for _ in range(warmup):
        both()
    bt.set_tuning("measure_global", 1)
    measure()
    bt.set_tuning("measure_global", 0)
    a, b, m, mg = [], [], [], []
    for _ in range(reps):                                   # alternated: chain, chain + measure, measure, chain, ...
        a += timed(chain, 1)
        b += timed(both, 1)
        m += timed(measure, 1)
        bt.set_tuning("measure_global", 1)                  # (drains the stream; outside the timed windows)
        mg += timed(measure, 1)
        bt.set_tuning("measure_global", 0)
    sub, r5 = bt.measure(flat, pos, want_resp=True)
    bt.sync()
    err = int((out.cpu().numpy() - centres[None]).__abs__().max())
    ok = check(oracle, flat, fill, tw, True, pos, None, sub, r5)
    moved = float((sub != pos.to(torch.float64)).any(1).double().mean())
    bt.close()
    ma, mb, mm = float(np.median(a)), float(np.median(b)), float(np.median(m))
    n = n_clips * n_frames
    return dict(case="chains", clips=n_clips, frames_per_clip=n_frames, frame_h=fh, frame_w=fw, target_width=tw, window=list(ws),
                kernel_len=65, positions=n, reps=reps, warmup=warmup, chain_ms=stats(a), chain_then_measure_ms=stats(b),
                measure_ms=stats(m), measure_reading_the_frame_ms=stats(mg), measure_over_chain=mm / ma, chain_then_measure_over_chain=mb / ma,
                measure_us_per_position=mm * 1e3 / n, chain_us_per_frame=ma * 1e3 / n, chain_max_abs_error_px=err,
                positions_moved_by_the_rule=moved, checked_against_restatement=ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("1080p", "1080p_1", "l293", "chains", "all"), default="all")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "measure_bench measures on the GPU"
    from oracle.dog_oracle import Oracle
    oracle = Oracle()
    todo = ("1080p", "1080p_1", "l293", "chains") if args.case == "all" else (args.case,)
    results = []
    frames = None
    for case in todo:
        if case != "chains" and frames is None:
            g = torch.Generator(device="cuda").manual_seed(0)
            frames = torch.randint(0, 256, (64, 1080, 1920), dtype=torch.uint8, device="cuda", generator=g)
        if case == "1080p":
            r = run_positions(case, oracle, 25, 4096, args.reps, args.warmup, frames)
        elif case == "1080p_1":
            r = run_positions(case, oracle, 25, 1, args.reps, args.warmup, frames)
        elif case == "l293":
            r = run_positions(case, oracle, 120, 4096, max(5, args.reps // 4), 1, frames)
        else:
            frames = None
            torch.cuda.empty_cache()
            r = run_chains(oracle, args.reps, args.warmup, args.clips)
        r["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
