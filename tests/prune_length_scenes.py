"""Scenes that put every kept-range form of the roll batch path (csrc/dog_prune.hpp, the PRUNE instances of csrc/dog_roll.hpp)
in front of every compiled kernel length, shared by tests/test_prune_lengths_cpu.py (which shows, with
tests/prune_restatement.py alone, that the forms occur) and tests/test_gpu_prune_lengths.py (which holds the kernels to them).

What a kept range [ba, bb) changes in roll_strip depends on the kernel length l: the loop starts at sub-chunk ba — a shortened
prologue body when ba < roll_prologue_len(l), else phase ba mod (roll_slots(l) / 8) of the full body —, outputs above row 8·ba
are held back from the peak, and the loop ends at prune_sc_hi(ba, bb, l, nsub).  CLASSES names the forms; `classes_of` reads
them off the restatement's hulls.

Geometry: a window of n1(l) × 131 (strips at window columns 0 and 64, remainder columns 128, 129, 130) whose padded tile lies
inside a frame of (n1 + 2 l) × 400: the frame's edges are tests/test_gpu_prepass_edges.py's subject.  n1(l) = 2 l + 29 (odd): a
disc in the window's last rows starts its hull near block nblk − l/8 − 2, which must reach roll_prologue_len(l) ≈ l/8; the
dense Float64 oracle stays below 1e10 multiply-adds per length (l = 149: ten windows of 327 × 131).

Ten windows per length, discs of the target's radius (0 for dark targets, 255 for bright ones) on fill 128, noise ± 2 on
every second one.  A disc's row is chosen for the first kept block it should give (`_row_for`); its centre sits on tile
coordinate 7 mod 8 where it can, so that a disc smaller than a cell lies across four cells and the first largest 3 × 3-cell
sum belongs to a cell whose 8 × 8 pixels hold the centre (a disc inside one cell ties nine 3 × 3 sums and the first of them
misses it).  Test code only: the library never imports it."""
import numpy as np

import fp32_restatement as fr
import prune_restatement as pr

FILL, FW, N2, CH, TW = 128, 400, 131, 8, 64
LENGTHS = tuple(range(17, 150, 4))
TWO_SIGN = 8                      # index of the window that holds a disc of either sign
CLASSES = (
    "strip: ba == 0 and bb + tail < nsub",
    "strip: 0 < ba < prologue",
    "strip: ba >= prologue",
    "three phases of ba",
    "bb == nblk",
    "0 < ba and bb < nblk",
    "empty strip beside a kept one",
    "remainder column kept with ba > 0",
    "remainder columns empty",
)


def tw_for_kernel_len(l):
    for tw10 in range(20, 1400):
        if fr.kernel_len(fr.sigma_of(tw10 / 10)) == l:
            return tw10 / 10
    raise AssertionError(l)


def variant_id(l):
    return 100 if l == 65 else 100 + l


# csrc/dog_roll.hpp
def roll_slots(l):
    return (l - 1 + 2 * CH - 1) // CH * CH


def roll_phases(l):
    return roll_slots(l) // CH


def roll_prologue_len(l):
    blocks = ((l + 1) // 2 + 1) // 2          # roll_col_blocks, ROLL_QB = 2
    return (blocks - 2 + 1) // 2


def n1_of(l):
    return 2 * l + 29


def geometry(l):
    """(frame height, window (n1, n2), radii, the 1-based guess at the frame's centre, disc radius)."""
    n1 = n1_of(l)
    fh = n1 + 2 * l
    return fh, (n1, N2), (n1 // 2, N2 // 2), (fh // 2 + 1, FW // 2 + 1), max(2, int(tw_for_kernel_len(l)) // 2)


def _on7(v, hw):
    """The smallest value ≥ v whose tile coordinate (v + l÷2) is 7 mod 8."""
    return v + (7 - (v + hw)) % 8


def _on7_down(v, hw):
    """The largest value ≤ v whose tile coordinate is 7 mod 8."""
    return v - (v + hw - 7) % 8


def _row_for(ba, l):
    """A window row for a disc whose hull should start at block ba: the hull of a disc at row y starts near (y − l÷2) ÷ 8."""
    return _on7(l // 2 + CH * ba + 1, l // 2)


def _placements(l):
    """Per window: a list of (window row, window column, is the target's sign) and whether it carries noise."""
    hw, (n1, _), rad = l // 2, geometry(l)[1], geometry(l)[4]
    p = roll_prologue_len(l)
    # left: a disc no input of strip 1 or of the remainder columns reaches (for long kernels its centre lies left of the window,
    # in the tile's margin); right: centred on the remainder columns
    tc = min(TW - 1 - rad, hw + 20)           # the left disc's tile column: its last column below 64, the first that strip 1 reads
    tc -= (tc - 7) % 8
    assert tc >= rad, (l, tc, rad)
    left, right, mid = tc - hw, 129, 64
    inside = max(left, _on7(4, hw))           # … and one whose centre lies in the window whatever l: L is taken at its centre
    bottom = _on7_down(n1 - 2, hw)
    return [
        ([(_on7(2, hw), left, True)], False),                         # first rows
        ([(_row_for(1, l), right, True)], True),                      # first kept block inside the prologue, on the remainder columns
        ([(_row_for(max(1, p - 1), l), left, True)], False),          # the prologue's last shortened body
        ([(_row_for(p, l), inside, True)], True),                       # the first full body
        ([(_row_for(p + 1, l), right, True)], False),
        ([(bottom, inside, True)], True),                             # last rows: prune_sc_hi clamps to nsub
        ([(bottom, right, True)], False),
        ([(_row_for(p + 2, l), mid, True)], True),                    # across the strip boundary
        # TWO_SIGN, equal contrast, far apart in rows: the other sign's hull ends two blocks above the window's last, so a weaker L has blocks to add
        ([(_on7(2, hw), inside, True), (_on7_down(CH * (-(-n1 // CH) - 2) - hw - CH, hw), inside, False)], False),
        ([(_row_for(p + 3, l), 96, True)], True),
    ]


def scenes(l, darker):
    """(frames [10][fh][400] uint8, guesses [10][2] int32 (1-based), fill) for kernel length l."""
    fh, (n1, n2), (r1, r2), g, rad = geometry(l)
    hw = l // 2
    ti0, wj0 = g[0] - r1 - 1 - hw, g[1] - r2 - 1 - hw      # frame row / column of the tile's first pixel
    assert ti0 >= 0 and wj0 >= 0 and ti0 + n1 + l - 1 <= fh and wj0 + n2 + l - 1 <= FW
    rng = np.random.default_rng([l, int(darker)])
    ii, jj = np.ogrid[:fh, :FW]
    frames = []
    for discs, noisy in _placements(l):
        f = np.full((fh, FW), FILL, np.uint8)
        for y, x, target in discs:
            cy, cx = ti0 + hw + y, wj0 + hw + x
            assert rad <= cy < fh - rad and wj0 + rad <= cx < wj0 + n2 + l - 1 - rad, (l, y, x)
            dark = darker == target
            # contrast 127 either way in the window that holds both signs
            f[(ii - cy) ** 2 + (jj - cx) ** 2 <= rad * rad] = (1 if len(discs) > 1 else 0) if dark else 255
        if noisy:
            f = np.clip(f.astype(np.int16) + rng.integers(-2, 3, f.shape), 0, 255).astype(np.uint8)
        frames.append(f)
    return np.stack(frames), np.tile(np.array(g, np.int32), (len(frames), 1)), FILL


def tiles(l, frames, guesses, fill):
    radii = geometry(l)[2]
    return [fr.window_tile(f, fill, l, radii, g) for f, g in zip(frames, guesses)]


def restate(l, darker, frames, guesses, fill):
    """The restatement's pre-pass of every window."""
    tw = tw_for_kernel_len(l)
    return [pr.prepass(t, fill, tw, darker) for t in tiles(l, frames, guesses, fill)]


def classes_of(l, pps):
    """Which of CLASSES the hulls of these windows show, as {class: [(window, slot, ba, bb), …]}."""
    p, nb = roll_prologue_len(l), roll_phases(l)
    found = {c: [] for c in CLASSES}
    phases = {}
    for w, pp in enumerate(pps):
        nstrips = sum(1 for _, width in pp["slots"] if width > 1)
        hull, nblk, nsub = pp["hull"], pp["nblk"], pp["nsub"]
        assert nstrips == 2 and len(hull) == 5
        for s, (ba, bb) in enumerate(hull):
            hit = (w, s, ba, bb)
            if bb == ba:
                continue
            strip = s < nstrips
            if strip and ba == 0 and bb + pr.tail(l) < nsub:
                found[CLASSES[0]].append(hit)
            if strip and 0 < ba < p:
                found[CLASSES[1]].append(hit)
            if strip and ba >= p:
                found[CLASSES[2]].append(hit)
            if strip:
                phases.setdefault(ba % nb, hit)
            if bb == nblk:
                found[CLASSES[4]].append(hit)
            if 0 < ba and bb < nblk:
                found[CLASSES[5]].append(hit)
            if not strip and ba > 0:
                found[CLASSES[7]].append(hit)
        kept = [bb > ba for ba, bb in hull]
        if any(kept[:nstrips]) and not all(kept[:nstrips]):
            found[CLASSES[6]].append((w, kept.index(False), 0, 0))
        if not any(kept[nstrips:]) and any(kept[:nstrips]):
            found[CLASSES[8]].append((w, nstrips, 0, 0))
    if len(phases) >= 3:
        found[CLASSES[3]] = list(phases.values())
    return found


def counts(l, pps):
    """(kept, total) per window."""
    return [pr.kept_pairs(pp, l) for pp in pps]
