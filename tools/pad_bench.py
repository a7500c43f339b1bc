#!/usr/bin/env python3
"""pad_bench.py — the roll kernels' padding-only sub-chunks (csrc/dog_roll.hpp, "padding rows"): how many there are for a set
of guesses, and what a step costs with them.

bench.py's frame recipe (make_frames, its seed, its workloads) with the guess placement selectable:
  --placement bench    bench.py's own guesses: centres uniform over the frame, guesses within ± radii ÷ 2, clipped
  --placement inside   every tile wholly inside the frame (no padding anywhere): the control for interior windows
  --placement edge     every window hangs over the top (even windows) or the bottom (odd) edge by 64 … 127 tile rows
The host-side COUNT walks every (window, strip, sub-chunk) as roll_strip does and counts the pairs the kernel skips — all 8
rows outside the frame, or the strip's staged columns all outside — and prices them with an instruction model: 450 VALU
instructions per sub-chunk for staging and row pass, 48 for peak tracking and loop, 32 packed FMAs per tap block of the column
pass (shortened like the prologue and epilogue bodies), a skipped sub-chunk 40.  A count, not a measurement.
The TIMING is HIP events around pdog_detect_batch, `--steps` of them after `--warmup`; one JSON line on stdout.  The `inside`
and `edge` placements move the guesses away from the discs the frames hold: many windows then see noise only, exact mode
re-decides their near-ties, and that work is timed with the kernels — `--no-exact` times the kernels alone.
`--count-only` needs no GPU."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

CH, TW, QB, THIN_MAX = 8, 64, 2, 6   # dog_roll.hpp: rows per sub-chunk, strip width, tap pairs per block; pawsome_dog.hip: kThinMax


def kernel_len(tw):
    sigma = float(tw) / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    return 4 * int(np.ceil(sigma * np.sqrt(2.0))) + 1


def roll_sb(L):
    return ((TW + L - 1 + 7) // 8 + 3) // 4 * 4


def place(guesses, placement, fh, fw, radii, L):
    """bench.py's guesses moved to the asked placement (rows only for `edge`; `inside` clips both coordinates)."""
    g = guesses.astype(np.int64).copy()
    hw, (r1, r2) = L // 2, radii
    if placement == "inside":
        g[:, 0] = np.clip(g[:, 0], r1 + hw + 1, fh - r1 - hw)
        g[:, 1] = np.clip(g[:, 1], r2 + hw + 1, fw - r2 - hw)
    elif placement == "edge":
        NA = 2 * r1 + 1 + L - 1
        over = 64 + np.arange(len(g)) % 64                     # tile rows outside the frame
        ti0 = np.where(np.arange(len(g)) % 2 == 0, -over, fh - NA + over)
        g[:, 0] = ti0 + r1 + 1 + hw
        assert (g[:, 0] >= -hw).all() and (g[:, 0] <= fh + hw + 1).all(), "edge placement leaves the reference's range"
    return g.astype(np.int32)


def count_padding(guesses, fh, fw, radii, L, nstrips=None):
    """(strip, sub-chunk) pairs, the padding-only ones among them, the share of tile rows outside the frame and the
    instruction model's share of the roll kernel's VALU instructions that the skip removes."""
    hw, (r1, r2) = L // 2, radii
    n1, n2 = 2 * r1 + 1, 2 * r2 + 1
    NA, nsub = n1 + L - 1, (n1 + L - 1 + CH - 1) // CH
    rem = n2 % TW
    ncols = n2 - rem if (n2 > TW and 0 < rem <= THIN_MAX) else n2
    if nstrips is None:
        nstrips = (ncols + TW - 1) // TW
    x0 = [min(s * TW, ncols - TW) if ncols >= TW else 0 for s in range(nstrips)]
    nb = ((L + 1) // 2 + QB - 1) // QB                          # roll_col_blocks
    c0 = (n1 + 2) // 4                                          # roll_epi_c0
    sc = np.arange(nsub)
    blocks = np.maximum(0, np.minimum(nb, 2 * sc + 2) - np.maximum(0, 2 * sc - c0))
    cost = 450 + 48 + 32 * blocks                               # per (strip, sub-chunk)
    g = guesses.astype(np.int64)
    ti0 = g[:, 0] - r1 - 1 - hw
    wj0 = g[:, 1] - r2 - 1 - hw
    gi0 = ti0[:, None] + CH * sc[None, :]                       # [n, nsub]
    rows_pad = (gi0 + CH - 1 < 0) | (gi0 >= fh)
    pairs = skipped = 0
    total = saved = 0
    for s in range(nstrips):
        tj0 = wj0 + x0[s]
        cols_out = (tj0 + 8 * roll_sb(L) <= 0) | (tj0 >= fw)
        pad = rows_pad | cols_out[:, None]
        pairs += pad.size
        skipped += int(pad.sum())
        total += int(cost.sum()) * len(g)
        saved += int(((cost - 40)[None, :] * pad).sum())
    rows = ti0[:, None] + np.arange(NA)[None, :]
    return {"pairs": pairs, "padding_only_pairs": skipped, "padding_only_frac": skipped / pairs,
            "tile_rows_outside_frac": float(((rows < 0) | (rows >= fh)).mean()), "model_valu_frac_saved": saved / total}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--placement", default="bench", choices=("bench", "inside", "edge"))
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--target-width", type=float, default=0.0)
    ap.add_argument("--noise", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tuning", action="append", default=[], metavar="KEY=0|1")
    ap.add_argument("--no-exact", action="store_true",
                    help="exact mode off: the moved guesses leave many windows without their target, and the refinement of their "
                         "near-ties would be timed with the kernels")
    ap.add_argument("--count-only", action="store_true", help="print the host-side count and leave (no GPU)")
    args = ap.parse_args()
    fh, fw, tw, ws, batch, _ = bench.WORKLOADS[args.workload]
    batch = args.batch or batch
    tw = args.target_width or tw
    ws = (ws, ws) if not isinstance(ws, tuple) else (ws[1], ws[0])
    ws = tuple(int(v) // 2 * 2 + 1 for v in ws)                # window sizes are made odd (fix_window_size)
    radii = (ws[0] // 2, ws[1] // 2)
    L = kernel_len(tw)
    res = {"tool": "pad_bench", "workload": args.workload, "placement": args.placement, "batch": batch, "target_width": tw,
           "kernel_len": L, "window": list(ws), "tuning": args.tuning}
    if args.count_only:
        rng = np.random.Generator(np.random.PCG64(0))          # make_frames' guesses, without the frames
        ci, cj = rng.integers(1, fh + 1, batch), rng.integers(1, fw + 1, batch)
        di = rng.integers(-(radii[0] // 2), radii[0] // 2 + 1, batch)
        dj = rng.integers(-(radii[1] // 2), radii[1] // 2 + 1, batch)
        guesses = np.stack([np.clip(ci + di, 1, fh), np.clip(cj + dj, 1, fw)], 1).astype(np.int32)
        res["count"] = count_padding(place(guesses, args.placement, fh, fw, radii, L), fh, fw, radii, L)
        print(json.dumps(res))
        return 0
    import torch
    import pawsometracker_jl_amd as pt
    assert tuple(pt.fix_window_size(ws)) == ws, (ws, pt.fix_window_size(ws))
    dev = torch.device("cuda", 0)
    frames, guesses_h, _ = bench.make_frames(torch, batch, fh, fw, tw, radii, seed=0, noise=args.noise, device=dev)
    fill = pt.mode(frames[0].cpu().numpy()) if args.noise else 128
    guesses_h = place(guesses_h, args.placement, fh, fw, radii, L)
    bt = pt.BatchTracker(fh, fw, tw, ws, True, fill, device=0)
    for kv in args.tuning:
        key, _, val = kv.partition("=")
        bt.set_tuning(key, int(val or 1))
    if args.no_exact:
        bt.set_exact(0)
    bt.reserve(batch)
    bt.use_torch_stream()
    info = bt.info()
    assert info.kernel_len == L, (info.kernel_len, L)
    res["count"] = count_padding(guesses_h, fh, fw, radii, L, nstrips=info.n_strips)
    res["kernel_for_this_batch"] = bt.kernel_for_batch(batch)
    res["fill"] = int(fill)
    guesses = torch.from_numpy(guesses_h).to(dev)
    out = torch.empty((batch, 2), dtype=torch.int32, device=dev)
    for _ in range(args.warmup):
        bt.detect(frames, guesses, out=out)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    torch.cuda.synchronize()
    refined0 = bt.exact_stats()[2]
    for a, b in ev:
        a.record()
        bt.detect(frames, guesses, out=out)
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    res["kernel_ms"] = {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1], "mean": float(np.mean(ms)), "steps": args.steps}
    res["exact"] = {"on": not args.no_exact, "refined_windows_per_step": (bt.exact_stats()[2] - refined0) / args.steps}
    res["positions_crc"] = int(np.bitwise_xor.reduce(out.cpu().numpy().astype(np.int64).ravel() * np.arange(1, 2 * batch + 1)))
    print(json.dumps(res))
    bt.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
