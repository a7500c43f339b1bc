"""The roll kernel's slot machine with the range-end entry (csrc/dog_roll.hpp: roll_col_body ENTRY, roll_strip; the rule is
csrc/dog_roll_range.hpp's), in NumPy float32, for one window column at l = 17, 21 and 65.

The machine is restated as the kernel runs it: S = roll_slots(l) accumulator slots, output y in slot (y − y_lo) mod S, the
sub-chunks of a kept range numbered from its start, sub-chunk j running tap blocks qlo … min(2 j + 2, blocks) − 1 in the order
(block, row, channel, pair), a pair (T[tt], T[tt − 1]) feeding the two outputs of a slot pair, the tt = 0 pair of the first
channel by MULTIPLY (which restarts the slots), everything else by fr.fma32, T[−1] = T[l] = 0; the emit part reads the 8
outputs whose last row the sub-chunk holds.  qlo = roll_end_entry(roll_end_qlo(8·sc − y_end)) — the exact first block rounded
down to the entry step, 4 blocks at these lengths —, restated here the way
tests/prune_length_scenes.py restates roll_prologue_len (tests/range_end_main.cpp holds the header itself to the pairs).

For every range length n = prune_tail + 1 … prune_tail + 2·NBODY + 1 — from the shortest range, where prologue and end meet in
one sub-chunk, to ranges with full bodies that are not entered late in between, every phase of the ring at both ends — both
for a range that ends inside the window and for one the window's bottom cuts off (n1 mod 8 = 5: the clipped y_end = n1 − 1),
every emitted output y_lo ≤ y ≤ y_end is BIT-EQUAL to the plain chain of its terms in ascending tap order, first term by
multiply.  (The plain chain carries the pairing's two zero taps where the machine meets them: an odd output starts from its
pair's T[−1] product, an even one ends with T[l]; with exact zeros among the R values they decide the sign of a zero.)
For l = 21 the emitted rows include the four past 8·bb.  The R values are random with both signs and exact zeros.  One set of
machines starts with NaN in every slot: no emitted output ever reads a slot it did not start itself.  A rule one step too
eager is run beside it and must be caught."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_restatement as fr  # noqa: E402
import prune_length_scenes as ps  # noqa: E402
import prune_restatement as pr  # noqa: E402

CH, QB = 8, 2


# csrc/dog_roll_range.hpp
def col_blocks(l):
    return ((l + 1) // 2 + QB - 1) // QB


def end_y(sc_hi, l, n1):
    return min(CH * sc_hi - l, n1 - 1)


def end_qlo(tm):
    return (tm + 1) >> 2 if tm > 0 else 0


def entry_step(l):
    return 4 if l <= 81 else 8


def end_entry(qlo, l):
    """The block the kernel enters at: qlo rounded down to the step."""
    return qlo & ~(entry_step(l) - 1)


def sc_hi_of(ba, bb, l, nsub):
    return min(bb + pr.tail(l), nsub)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def _column(l, n1, seed):
    """R = (R+, R−) of one column for every tile row (and the rows a last sub-chunk reads past the tile), both signs, exact zeros."""
    rng = np.random.default_rng([l, seed])
    rows = CH * (-(-(n1 + l - 1) // CH)) + CH
    R = (rng.standard_normal((rows, 2)) * np.exp(rng.uniform(-3, 3, (rows, 2)))).astype(np.float32)
    R[rng.random((rows, 2)) < 0.12] = 0.0
    R[rng.random(rows) < 0.05] = 0.0                     # whole rows of zeros: both channels
    return R


def _taps(l, darker):
    """T[c][t + 1] for t = −1 … l: the column table with its two zero taps."""
    _, _, _, col = fr.tap_tables(ps.tw_for_kernel_len(l), darker)
    assert col.shape == (2, l)
    T = np.zeros((2, l + 2), np.float32)
    T[:, 1:l + 1] = col
    return T


def _plain(l, R, T, n1):
    """Every output y of the window by its own chain: ascending taps, (+, −) per tap, first term by multiply; an odd output
    starts from the T[−1] pair of row y − 1, an even one ends with the T[l] pair of row y + l."""
    y = np.arange(n1)
    odd = (y & 1) == 1
    with np.errstate(invalid="ignore"):
        pre = fr.fma32(R[np.maximum(y - 1, 0), 1], T[1, 0], R[np.maximum(y - 1, 0), 0] * T[0, 0])
        first = R[y, 0] * T[0, 1]
        acc = np.where(odd, fr.fma32(R[y, 0], T[0, 1], pre), first).astype(np.float32)
        acc = fr.fma32(R[y, 1], T[1, 1], acc)
        for t in range(1, l):
            acc = fr.fma32(R[y + t, 0], T[0, t + 1], acc)
            acc = fr.fma32(R[y + t, 1], T[1, t + 1], acc)
        post = fr.fma32(R[y + l, 1], T[1, l + 1], fr.fma32(R[y + l, 0], T[0, l + 1], acc))
    return np.where(odd, acc, post).astype(np.float32)


def _machines(l, R, T, n1, cases):
    """All cases at once (a vector of independent machines that differ in their range, their entry rule and their first slot
    contents).  cases: (ba, bb, mode, seed_nan), mode 0: no entry (qlo = 0), 1: the rule, 2: one step too eager.
    Returns per case {y: value} of the emitted outputs."""
    S = ps.roll_slots(l)
    NB, NQB, NPRO = S // CH, col_blocks(l), ps.roll_prologue_len(l)
    nsub = -(-(n1 + l - 1) // CH)
    ba = np.array([c[0] for c in cases])
    hi = np.array([sc_hi_of(c[0], c[1], l, nsub) for c in cases])
    mode = np.array([c[2] for c in cases])
    y_end = np.array([end_y(h, l, n1) for h in hi])
    acc = np.where(np.array([c[3] for c in cases])[:, None], np.float32(np.nan), np.float32(0)) * np.ones((1, S), np.float32)
    acc = acc.astype(np.float32)
    out = [dict() for _ in cases]
    for rel in range(int((hi - ba).max())):
        sc = ba + rel
        live = sc < hi
        tm = CH * sc - y_end
        qlo = np.where(mode == 0, 0, np.array([end_entry(end_qlo(int(v)), l) for v in tm]) + entry_step(l) * (mode == 2))
        qhi = min(2 * rel + 2, NQB) if rel < NPRO else NQB
        phase = rel % NB
        for qb in range(qhi):
            on = live & (qb >= qlo)
            if not on.any():
                continue
            for i in range(CH):
                par, amod = i & 1, CH * phase + i
                r = R[np.where(live, CH * sc + i, 0)]                     # [case][channel] (a machine past its range is masked off)
                for c in (0, 1):
                    for m in range(QB):
                        tt = par + 2 * (QB * qb + m)
                        if tt - 1 > l - 1:
                            continue
                        slot = (amod - tt) % S
                        assert slot % 2 == 0
                        tx, ty = T[c, tt + 1], T[c, tt]                  # (T[tt], T[tt − 1])
                        with np.errstate(invalid="ignore"):
                            if tt == 0 and c == 0:
                                nx, ny = r[:, c] * tx, r[:, c] * ty
                            else:
                                nx, ny = fr.fma32(r[:, c], tx, acc[:, slot]), fr.fma32(r[:, c], ty, acc[:, slot + 1])
                        acc[:, slot] = np.where(on, nx, acc[:, slot])
                        acc[:, slot + 1] = np.where(on, ny, acc[:, slot + 1])
        for k in np.flatnonzero(live):                                    # the emit part
            for i in range(CH):
                y = CH * int(sc[k]) - (l - 1) + i
                if CH * int(ba[k]) <= y < n1:
                    out[k][y] = acc[k, (CH * phase + i - (l - 1)) % S]
    return out, y_end


@pytest.mark.parametrize("l", (17, 21, 65))
def test_every_emitted_output_is_the_plain_chain(l):
    NB, tail, NPRO = ps.roll_phases(l), pr.tail(l), ps.roll_prologue_len(l)
    assert (NB, tail) == {17: (3, 2), 21: (4, 3), 65: (9, 8)}[l]
    n1 = CH * (2 * NB + tail + 6) + 5                                     # n1 mod 8 = 5: a clipped y_end inside a sub-chunk
    nblk, nsub = -(-n1 // CH), -(-(n1 + l - 1) // CH)
    lengths = list(range(tail + 1, tail + 2 * NB + 2))
    ranges = []
    for n in lengths:                                                     # ends inside the window: ba = 1, bb = ba + n − tail
        ranges.append((1, 1 + n - tail))
        assert ranges[-1][1] + tail < nsub and sc_hi_of(*ranges[-1], l, nsub) - 1 == n
    clipped = [(nsub - n, nblk) for n in lengths if 0 <= nsub - n < nblk]  # cut off by the window's bottom: sc_hi = nsub
    assert len(clipped) >= len(lengths) - 1 and all(sc_hi_of(a, b, l, nsub) == nsub for a, b in clipped)
    ranges += clipped
    assert min(sc_hi_of(a, b, l, nsub) - a for a, b in ranges) < NPRO + tail          # prologue and end in one sub-chunk
    assert max(sc_hi_of(a, b, l, nsub) - a for a, b in ranges) >= NPRO + tail + NB     # full bodies without entry in between
    cases = [(a, b, 1, False) for a, b in ranges] + [(a, b, 1, True) for a, b in ranges] + [(a, b, 0, False) for a, b in ranges]
    eager = [(a, b, 2, False) for a, b in ranges]
    for darker in (True, False):
        R, T = _column(l, n1, int(darker)), _taps(l, darker)
        plain = _plain(l, R, T, n1)
        assert np.isfinite(plain).all() and (R == 0).any() and (R > 0).any() and (R < 0).any()
        out, y_end = _machines(l, R, T, n1, cases + eager)
        past = 0
        for k, (a, b, mode, nan) in enumerate(cases):
            ys = sorted(out[k])
            assert ys == list(range(CH * a, int(y_end[k]) + 1)), (l, a, b, ys[:3], ys[-3:], y_end[k])
            past += sum(1 for y in ys if y >= CH * b)
            got = np.array([out[k][y] for y in ys], np.float32)
            assert np.array_equal(_bits(got), _bits(plain[ys])), (l, darker, a, b, mode, nan, [y for y, g in zip(ys, got) if _bits(g) != _bits(plain[y])][:5])
        assert (past > 0) == (l == 21)                                    # l = 21: the four rows emitted past 8·bb
        caught = 0
        for k, (a, b, _, _) in enumerate(eager, start=len(cases)):
            ys = sorted(out[k])
            caught += not np.array_equal(_bits(np.array([out[k][y] for y in ys], np.float32)), _bits(plain[ys]))
        assert caught == len(eager), (l, caught, len(eager))             # entering one step later loses a term in EVERY range
