#!/usr/bin/env python3
"""What the walk with a motion model (pdog_detect_chains_motion) costs per step against the exclusive walk
(pdog_detect_chains_exclusive), which is the yardstick: existing code, the same detect_peaks per step, another kernel behind it.

The video of tools/exclusive_bench.py: one 1080p video of 2000 frames, 30 -> 24 positions per second (1600 steps), 45 x 45
windows, target width 25; cases as groups x targets per group, 1 x 1, 1 x 8, 2 x 32 and 64 x 8.  k, min_distance, min_ratio,
min_response and coast are the defaults (min(32, 2 T), 25, 0.5, 0, 8).  Three calls are alternated in one process — the
exclusive walk, the motion walk with its lists read from global memory (the product's choice) and the motion walk with its
lists staged in LDS (pdog_set_tuning "motion_lds") —, device events around whole calls, medians of --reps samples after
--warmup calls; us per step = median ms * 1000 / steps.  Also reported: the share of (target, step) pairs that were held and
that were contested (the latter re-derived on the host from the positions and states, as the rule defines it).

--kernel times the motion kernel alone in both forms on lists made to be contested (lattice positions, every window seeing
every blob): 64 x 8 with k = 16 and 2 x 32 with k = 32, events around 200 launches.

--fast times one more case: eight discs on circles around the frame centre, 18 ... 24 px per frame (the path bends by about
1 px per frame), every frame a step, walked at 31 x 31 and at 45 x 45 by both rules; reported beside the times is the share of
steps more than 3 px off the true position.

One JSON line per case; --out FILE writes them all (profiles/motion_bench.json)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from tools.video_bench import alternate, make_video, stats, timed  # noqa: E402


def shares(out, state, hw, d, coast):
    """(held share, contested share) of a walk filed with first = 1: out [G, T, m, 2], state [G, T, m] (numpy).  The carry of
    include/pawsome_motion.h replayed over the positions and states: that is all it depends on."""
    G, T, m = state.shape
    p = out[:, :, 0].astype(np.int64)
    v = np.zeros((G, T, 2), np.int64)
    nh = np.zeros((G, T), np.int64)
    hi = np.array(hw, np.int64)
    contested = 0
    for s in range(1, m):
        c = np.clip(p + v, 1, hi)
        p2, st = out[:, :, s].astype(np.int64), state[:, :, s]
        d2 = ((p2[:, :, None, :] - c[:, None, :, :]) ** 2).sum(-1)              # [G, t, u]: p'_t against c_u
        d2[:, np.arange(T), np.arange(T)] = d * d
        cont = (d2 < d * d).any(-1) & (st >= 1)
        contested += int(cont.sum())
        held = st == -1
        nh = np.where(held, nh + 1, 0)
        v = np.where((held & (nh < coast))[..., None] | cont[..., None], v, np.where(held[..., None], 0, p2 - p))
        p = p2
    n = G * T * (m - 1)
    return float((state[:, :, 1:] == -1).sum()) / n, contested / n


def run_case(pt, frames, first_pos, rate, fps, ws, n_groups, n_targets, reps, warmup):
    import torch
    n, h, w = frames.shape
    tw = 25
    table = pt.fps_table(rate, n, 0.0, pt.DEFAULT_STOP, fps)
    m = len(table)
    n_all = n_groups * n_targets
    start = np.stack([first_pos[k % len(first_pos)] + (k // len(first_pos)) * np.array([1, -1]) for k in range(n_all)]).astype(np.int32)
    starts3 = torch.from_numpy(start).cuda().view(n_groups, n_targets, 2)
    tab = np.tile(table, (n_groups, 1))
    bt, bt_lds = pt.BatchTracker(h, w, tw, ws, True, 128), pt.BatchTracker(h, w, tw, ws, True, 128)
    bt_lds.set_tuning("motion_lds", 1)
    res = {}
    calls = dict(exclusive=lambda: res.__setitem__("excl", bt.detect_chains_exclusive(frames, tab, starts3, first=1)),
                 motion=lambda: res.__setitem__("mot", bt.detect_chains_motion(frames, tab, starts3, first=1)),
                 motion_lds=lambda: res.__setitem__("lds", bt_lds.detect_chains_motion(frames, tab, starts3, first=1)))
    ms = alternate(calls, reps, warmup)
    bt.sync()
    bt_lds.sync()
    out, state = res["mot"][0].cpu().numpy(), res["mot"][1].cpu().numpy()
    held, contested = shares(out, state, (h, w), 25, 8)
    ex, mo, ml = (float(np.median(ms[k])) for k in ("exclusive", "motion", "motion_lds"))
    r = dict(case="motion_walk", frames=n, frame_h=h, frame_w=w, rate=rate, fps=fps, steps=m, groups=n_groups, targets_per_group=n_targets,
             window=list(ws), target_width=tw, reps=reps, warmup=warmup, kernel_for_batch=bt.kernel_for_batch(n_all),
             exclusive_ms=stats(ms["exclusive"]), motion_ms=stats(ms["motion"]), motion_lds_ms=stats(ms["motion_lds"]),
             exclusive_us_per_step=ex * 1e3 / m, motion_us_per_step=mo * 1e3 / m, motion_lds_us_per_step=ml * 1e3 / m,
             motion_over_exclusive=mo / ex, motion_lds_over_motion=ml / mo, held_share=held, contested_share=contested,
             same_positions_as_exclusive_share=float((res["mot"][0] == res["excl"][0]).all(-1).float().mean()),
             lds_equals_global=bool(torch.equal(res["lds"][0], res["mot"][0]) and torch.equal(res["lds"][1], res["mot"][1])))
    bt.close()
    bt_lds.close()
    torch.cuda.empty_cache()
    return r


def run_kernel(pt, n_groups, n_targets, k, launches=200):
    """The kernel alone on contested lists: every target of a group sees the same k blobs on a lattice 12 px wide (d = 25: a
    taken blob blocks its neighbours), in its own order and with its own values."""
    import torch
    rng = np.random.default_rng(7)
    G, T = n_groups, n_targets
    blobs = (rng.integers(0, 24, (G, 1, k, 2)) * 12 + 300).astype(np.int32)
    order = np.argsort(rng.random((G, T, k)), -1)
    ij = np.take_along_axis(np.broadcast_to(blobs, (G, T, k, 2)), order[..., None], 2).astype(np.int32)
    peak = (0.5 + rng.random((G, T, k))).astype(np.float32)
    peak[:, :, 0] = 2.0
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    prev, ijd, pkd, cnt = d(ij[:, :, 0] + 3), d(ij), d(peak), d(np.full((G, T), k, np.int32))
    out = {}
    for name, lds in (("global", 0), ("lds", 1)):
        bt = pt.BatchTracker(1080, 1920, 25, (45, 45), True, 128)
        bt.set_tuning("motion_lds", lds)
        mstate = torch.zeros((G, T, 4), dtype=torch.int32, device="cuda")

        def many():
            for _ in range(launches):
                out[name] = bt.assign_motion(prev, mstate, ijd, pkd, cnt)
        many()
        t = [timed(many) for _ in range(5)]
        out[name + "_us"] = float(np.median(t)) * 1e3 / launches
        bt.sync()
        bt.close()
    st = out["global"][1]
    return dict(case="motion_kernel_alone", groups=G, targets_per_group=T, k=k, launches=launches, global_us_per_launch=out["global_us"],
                lds_us_per_launch=out["lds_us"], held_share=float((st == -1).float().mean()), later_pick_share=float((st > 1).float().mean()),
                lds_equals_global=bool(torch.equal(out["global"][0], out["lds"][0]) and torch.equal(st, out["lds"][1])),
                note="us per launch includes the Python call: the difference between the two forms is the kernels'")


def make_fast_video(n, h, w, tw, n_discs, omega=0.05, chunk=50):
    """uint8 cuda [n, h, w] and the true positions [n, n_discs, 2]: discs on circles of radius 360 ... 480 around the centre."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(1)
    radius = np.linspace(360, 480, n_discs)
    phase = np.arange(n_discs) * 2 * math.pi / n_discs
    ang = omega * np.arange(n)[:, None] + phase[None]
    pos = np.rint(np.stack([h / 2 + radius * np.sin(ang), w / 2 + radius * np.cos(ang)], -1)).astype(np.int32)
    frames = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    ii = torch.arange(1, h + 1, device="cuda").view(1, h, 1)
    jj = torch.arange(1, w + 1, device="cuda").view(1, 1, w)
    d_pos = torch.from_numpy(pos).cuda()
    for k0 in range(0, n, chunk):
        k1 = min(n, k0 + chunk)
        img = 128 + torch.randint(-2, 3, (k1 - k0, h, w), dtype=torch.int16, device="cuda", generator=g)
        for dsc in range(n_discs):
            p = d_pos[k0:k1, dsc]
            img[(ii - p[:, 0, None, None]) ** 2 + (jj - p[:, 1, None, None]) ** 2 <= (tw // 2) ** 2] = 0
        frames[k0:k1] = img.to(torch.uint8)
    return frames, pos


def run_fast(pt, n_frames, reps, warmup):
    import torch
    h, w, tw, T = 1080, 1920, 25, 8
    frames, pos = make_fast_video(n_frames, h, w, tw, T)
    table = np.arange(n_frames, dtype=np.int32)[None]
    starts = torch.from_numpy(pos[0][None].copy()).cuda()
    speed = np.hypot(*np.diff(pos.astype(np.float64), axis=0).transpose(2, 0, 1)).mean(0)
    r = dict(case="motion_fast_targets", frames=n_frames, frame_h=h, frame_w=w, steps=n_frames, groups=1, targets_per_group=T, target_width=tw,
             px_per_frame=[round(float(s), 1) for s in speed], reps=reps, warmup=warmup)
    for ws in (31, 45):
        bt = pt.BatchTracker(h, w, tw, (ws, ws), True, 128)
        res = {}
        calls = dict(exclusive=lambda: res.__setitem__("excl", bt.detect_chains_exclusive(frames, table, starts, first=1)),
                     motion=lambda: res.__setitem__("mot", bt.detect_chains_motion(frames, table, starts, first=1)))
        ms = alternate(calls, reps, warmup)
        bt.sync()
        truth = torch.from_numpy(pos.transpose(1, 0, 2).copy()).cuda()             # [T, n, 2]
        off = lambda o: float(((o[0][0] - truth).double().pow(2).sum(-1).sqrt() > 3).float()[:, 1:].mean())
        r[f"window_{ws}"] = dict(exclusive_us_per_step=float(np.median(ms["exclusive"])) * 1e3 / n_frames,
                                 motion_us_per_step=float(np.median(ms["motion"])) * 1e3 / n_frames,
                                 exclusive_ms=stats(ms["exclusive"]), motion_ms=stats(ms["motion"]),
                                 exclusive_steps_above_3px_share=off(res["excl"]), motion_steps_above_3px_share=off(res["mot"]),
                                 motion_held_share=float((res["mot"][1][:, :, 1:] == -1).float().mean()))
        bt.close()
    r["motion_31_over_motion_45"] = r["window_31"]["motion_us_per_step"] / r["window_45"]["motion_us_per_step"]
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--video-frames", type=int, default=2000)
    ap.add_argument("--cases", default="1x1,1x8,2x32,64x8", help="groups x targets per group ('' for none)")
    ap.add_argument("--kernel", action="store_true", help="also time the kernel alone, lists in global memory against LDS")
    ap.add_argument("--fast", action="store_true", help="also time the fast targets at 31 x 31 and 45 x 45")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "motion_bench measures on the GPU"
    import pawsometracker_jl_amd as pt
    results = []

    def report(r):
        r.update(device=torch.cuda.get_device_name(0), library=os.path.basename(pt.LIB_PATH))
        print(json.dumps(r), flush=True)
        results.append(r)

    if args.cases:
        frames, first_pos = make_video(args.video_frames, 1080, 1920, 25, 8)
        for case in args.cases.split(","):
            g, t = (int(v) for v in case.split("x"))
            report(run_case(pt, frames, first_pos, 30, 24, (45, 45), g, t, args.reps, args.warmup))
        del frames
        torch.cuda.empty_cache()
    if args.kernel:
        report(run_kernel(pt, 64, 8, 16))
        report(run_kernel(pt, 2, 32, 32))
    if args.fast:
        report(run_fast(pt, args.video_frames, args.reps, args.warmup))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
