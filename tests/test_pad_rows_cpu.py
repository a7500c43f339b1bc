"""The zero-sign argument behind the roll kernels' padding-only sub-chunks (csrc/dog_roll.hpp, "padding rows"), in NumPy
float32.  A sub-chunk of 8 tile rows that all lie outside the frame holds (fill − dc) = +0 everywhere when dc == fill, and the
kernel then skips its row pass and column FMAs.  What it skips must be the identity, bit for bit:
  * the row pass of +0 inputs gives R = (+0, +0);
  * the first (+, −) term pair of an output — a multiply by s·g₊[0], then an FMA with −s·g₋[0] — gives +0 for either sign of
    s, and the odd output of the register pair starts from (+0)·T[−1] = +0: "slot := +0" is what the kernel computes;
  * every later term fma(+0, t, a) returns a for every a that is not −0, and −0 cannot stand in an accumulator at a row
    boundary: a finished (+, −) pair of zero products cancels to +0 under round-to-nearest.
For a zero product the product-then-add IS the FMA (the product is exact), so plain float32 arithmetic states it; fma32 of
tests/fp32_restatement.py is run beside it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_restatement as fr  # noqa: E402

PZERO = np.float32(0.0)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _taps(tw=25.0):
    """The float32 tables of both signs of s: row[c][k] = g±[k]; col[c][t] = (s·g₊[t], −s·g₋[t])."""
    out = []
    for darker in (True, False):
        _, _, row, col = fr.tap_tables(tw, darker)
        out.append((row, col))
    return out


def test_zero_product_then_add_is_the_fma():
    """fma(+0, t, a) for finite t: the exact product is ±0, so one rounding of (product + a) is the float32 sum."""
    rng = np.random.default_rng(0)
    t = np.concatenate([rng.standard_normal(64), -rng.random(64), [1e-30, -1e-30, 3e38, -3e38]]).astype(np.float32)
    a = np.concatenate([rng.standard_normal(len(t) - 2) * 1e3, [0.0, 0.0]]).astype(np.float32)
    with np.errstate(all="raise"):
        prod = PZERO * t
        assert np.all(prod == 0) and np.array_equal(np.signbit(prod), np.signbit(t))     # (+0)·t = ±0 by the sign of t
        assert _same_bits(fr.fma32(PZERO, t, a), prod + a)


def test_row_pass_of_zeros_is_plus_zero():
    for row, _ in _taps():
        l = row.shape[1]
        for c in (0, 1):
            assert np.all(row[c] > 0) and np.all(np.isfinite(row[c]))                   # every Gaussian tap is positive and finite
            acc = PZERO
            for k in range(l // 2):
                s2 = PZERO + PZERO                                                       # the pair sum a[x−k] + a[x+k]
                acc = fr.fma32(s2, row[c, k], acc)
            acc = fr.fma32(PZERO, row[c, l // 2], acc)
            assert _same_bits(acc, PZERO)


def test_first_term_pair_gives_plus_zero_for_both_signs_of_s():
    for _, col in _taps():
        first = np.float32(PZERO * col[0, 0])                                            # the tt == 0 multiply: ±0 by the sign of s
        assert first == 0 and np.signbit(first) == np.signbit(col[0, 0])
        second = fr.fma32(PZERO, col[1, 0], first)                                       # adds (+0)·(−s·g₋[0]) = ∓0
        assert np.signbit(col[1, 0]) != np.signbit(col[0, 0])
        assert _same_bits(second, PZERO)
        assert _same_bits(first + PZERO * col[1, 0], PZERO)                              # product-then-add, the same bits
        odd = np.float32(PZERO * np.float32(0.0))                                        # the odd output of the pair: (+0)·T[−1]
        assert _same_bits(odd, PZERO)
    signs = {bool(np.signbit(col[0, 0])) for _, col in _taps()}
    assert signs == {False, True}                                                        # both signs of s were met


def test_later_terms_leave_normal_values_and_plus_zero_alone():
    rng = np.random.default_rng(1)
    normal = (rng.standard_normal(4096) * np.exp(rng.uniform(-20, 20, 4096))).astype(np.float32)
    assert np.all(np.abs(normal) >= np.finfo(np.float32).tiny)
    acc0 = np.concatenate([normal, np.zeros(8, np.float32)])
    for _, col in _taps():
        l = col.shape[1]
        acc = acc0.copy()
        for t in range(l):                                                               # a whole column of padding rows: 2·l zero terms
            acc = fr.fma32(PZERO, col[0, t], acc)
            acc = fr.fma32(PZERO, col[1, t], acc)
        assert _same_bits(acc, acc0)
        plain = acc0.copy()
        for t in range(l):
            plain = (plain + PZERO * col[0, t]) + PZERO * col[1, t]
        assert _same_bits(plain, acc0)


def test_minus_zero_is_the_one_value_a_zero_term_changes_and_no_boundary_holds_it():
    """fma(+0, t, −0) with t > 0 is +0: the skip would differ there.  The accumulators never hold −0 between rows: whatever the
    sign of s, a row's two zero products have opposite signs and their sum is +0 (round to nearest), also on top of +0."""
    assert not _same_bits(fr.fma32(PZERO, np.float32(1.0), np.float32(-0.0)), np.float32(-0.0))
    for _, col in _taps():
        for t in range(col.shape[1]):
            for start in (None, PZERO):                                                  # a first term (multiply), or a later one on +0
                a = np.float32(PZERO * col[0, t]) if start is None else fr.fma32(PZERO, col[0, t], start)
                a = fr.fma32(PZERO, col[1, t], a)
                assert _same_bits(a, PZERO)


def test_whole_response_of_a_padding_only_tile_is_plus_zero():
    """The emulation of the roll order on an all-fill tile: every response is +0 — what the skipped sub-chunks leave."""
    for darker in (True, False):
        tile = np.full((21 + 16, 45 + 16), 128, np.uint8)
        resp = fr.response_f32(tile, 128, 6.0, darker, "roll")
        assert fr.kernel_len(fr.sigma_of(6.0)) == 17 and resp.shape == (21, 45)
        assert _same_bits(resp, np.zeros_like(resp))
