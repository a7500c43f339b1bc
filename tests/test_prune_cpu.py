"""The pre-pass of the roll batch path (csrc/dog_prune.hpp) stated in NumPy (tests/prune_restatement.py) and held against
the float32 emulation of the roll order (tests/fp32_restatement.py) on small tiles, l = 17 and 65:
  * every 8-row output block's Cauchy–Schwarz bound plus δ(V) is at least the largest emulated |response| in the block;
  * L, evaluated from its 8 × 8 pixels' own input patch in the roll order, equals the emulated map's largest value at those
    pixels bit for bit, and so is at most the emulated maximum;
  * every slot's hull keeps every pixel within T_max of the maximum;
  * clean and lightly noisy discs prune (kept < total), flat and noise-only windows keep everything.
No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_restatement as fr  # noqa: E402
import prune_restatement as pr  # noqa: E402

FILL = 128


def _disc(h, w, centre, rad, value, bkgd):
    f = np.full((h, w), bkgd, np.uint8)
    ii, jj = np.ogrid[:h, :w]
    f[(ii - centre[0]) ** 2 + (jj - centre[1]) ** 2 <= rad * rad] = value
    return f


def _noisy(f, levels, seed):
    rng = np.random.default_rng(seed)
    return np.clip(f.astype(np.int16) + rng.integers(-levels, levels + 1, f.shape), 0, 255).astype(np.uint8)


# (name, tw, window (n1, n2), frame builder, fill, guess, prunes?)
def _cases():
    out = []
    for tw, ws in ((6, (41, 70)), (25, (65, 65)), (25, (129, 70))):
        l = fr.kernel_len(fr.sigma_of(tw))
        fh, fw = ws[0] + l + 40, ws[1] + l + 60
        c = (fh // 2 + 3, fw // 2 - 5)
        rad = max(2, int(tw) // 2)
        clean = _disc(fh, fw, c, rad, 0, FILL)
        out += [
            (f"clean-{tw}-{ws}", tw, ws, clean, FILL, (c[0] - 4, c[1] + 6), True),
            (f"noisy3-{tw}-{ws}", tw, ws, _noisy(clean, 3, 1), FILL, (c[0] + 5, c[1] - 3), True),
            (f"edge-{tw}-{ws}", tw, ws, _noisy(_disc(fh, fw, (4, 7), rad, 0, FILL), 2, 2), FILL, (1, 3), True),
            (f"flat-{tw}-{ws}", tw, ws, np.full((fh, fw), FILL, np.uint8), FILL, c, False),
            (f"noise-only-{tw}-{ws}", tw, ws, _noisy(np.full((fh, fw), FILL, np.uint8), 3, 3), FILL, c, False),
            (f"noise40-{tw}-{ws}", tw, ws, _noisy(clean, 40, 4), FILL, c, None),
            (f"dc-off-fill-{tw}-{ws}", tw, ws, _noisy(_disc(fh, fw, c, rad, 0, 60), 2, 5), FILL, (c[0] + 2, c[1] + 2), None),
        ]
    return out


CASES = _cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bound_lower_bound_and_hull(case):
    _bound_lower_bound_and_hull(case, True)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bound_lower_bound_and_hull_bright_sign(case):
    """The same scenes read for bright targets (PruneGeo::darker = 0: the cell sums and the tap tables take the other sign): the
    bound, L ≤ the maximum, the hull and the maximum's own block.  What the scenes say about pruning holds for their dark discs only."""
    _bound_lower_bound_and_hull(case, False)


def _bound_lower_bound_and_hull(case, darker):
    name, tw, ws, frame, fill, guess, prunes = case
    if not darker:
        prunes = None
    l = fr.kernel_len(fr.sigma_of(tw))
    radii = (ws[0] // 2, ws[1] // 2)
    tile = fr.window_tile(frame, fill, l, radii, guess)
    resp = fr.response_f32(tile, fill, tw, darker, "roll")
    pp = pr.prepass(tile, fill, tw, darker)          # (L comes from the pixels' own patch, not from resp)
    n1, n2 = resp.shape
    if name.startswith("dc-off-fill"):
        assert pp["dc"] != fill
    M = float(resp.max())
    (oy, ox), blk = pp["origin"], 8
    assert 0 <= oy <= n1 - min(blk, n1) and 0 <= ox <= n2 - min(blk, n2)
    # L, evaluated from the patch alone, is bit for bit the largest of the map's values at those 8 × 8 pixels — a value the strips
    # produce — and so at most the maximum
    assert np.float32(pp["L"]).view(np.int32) == resp[oy:oy + blk, ox:ox + blk].max().view(np.int32), name
    assert pp["L"] <= M
    if prunes is True:                              # … and the cell sums lead it to the target: within 35 % of the peak (the 8 × 8 pixels may miss a 7-pixel disc's centre)
        assert pp["L"] >= 0.65 * M, (name, pp["L"], M)
    absr = np.abs(resp.astype(np.float64))
    for s, (c0, w) in enumerate(pp["slots"]):
        for j in range(pp["nblk"]):
            bound = pp["norm"] * np.sqrt(float(pp["E"][s, j:j + pp["span"]].sum())) / 255.0
            assert bound + pp["dV"] >= absr[8 * j:8 * j + 8, c0:c0 + w].max(), (name, s, j)
        ba, bb = pp["hull"][s]
        near = np.argwhere(resp[:, c0:c0 + w].astype(np.float64) >= M - pp["Tmax"])
        for y, _ in near:
            assert 8 * ba <= y < 8 * bb, (name, s, int(y), (ba, bb))
        my, mx = np.unravel_index(int(np.argmax(resp)), resp.shape)
        if c0 <= mx < c0 + w:                       # the maximum's own block is kept
            assert ba <= my // 8 < bb, (name, s, (int(my), int(mx)), (ba, bb))
    kept, total = pr.kept_pairs(pp, l)
    print(name, "kept", kept, "of", total, "L", pp["L"], "max", M)
    if prunes is True:
        assert kept < total, name
    if prunes is False:
        assert kept == total, name


def test_kernel_norm_is_the_dense_kernels():
    for tw in (6, 25, 44):
        gp, gm, _, _ = fr.tap_tables(tw, True)
        K = np.outer(gp, gp) - np.outer(gm, gm)
        n = pr.kernel_norm_up(gp, gm)
        assert n >= np.sqrt((K * K).sum()) and n <= np.sqrt((K * K).sum()) * (1 + 1e-6)
    assert abs(pr.kernel_norm_up(*fr.tap_tables(25, True)[:2]) - 0.01022) < 1e-5


def test_prototype_table_matches_the_header():
    """include/pawsome_prune.h against _lib.PRUNE_PROTOTYPES, in the header's order, and the library exports every name."""
    import ctypes as C
    import re
    import pawsometracker_jl_amd as pt
    from pawsometracker_jl_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(root, "include", "pawsome_prune.h")).read(), flags=re.S)
    hdr = re.sub(r"^\s*#.*$", " ", hdr, flags=re.M)
    found = [(m.group(1), m.group(2)) for m in re.finditer(r"int\s+(pdog_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)]
    assert [n for n, _ in found] == list(_lib.PRUNE_PROTOTYPES) and len(found) == 2
    for name, args in found:
        restype, argtypes = _lib.PRUNE_PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == len(args.split(","))
        for ctype, decl in zip(argtypes, args.split(",")):
            assert (("*" in decl or "[" in decl) and (ctype is C.c_void_p or issubclass(ctype, C._Pointer))) or (decl.split()[0] == "int" and ctype is C.c_int), (name, decl)
        fn = getattr(pt.lib(), name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    assert '#include "pawsome_prune.h"' in open(os.path.join(root, "include", "pawsome_dog.h")).read()
