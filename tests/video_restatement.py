"""What the frame-table entry points must reproduce, restated in plain Python: the time axis of
src/PawsomeTracker.jl:150-152 and the frames its ffmpeg line (:155) selects in exact rationals (`fractions`; the two places
where the reference or the header prescribe a Float64 product say so), and the chain
over a frame table (:161-167 on selected frames) as a loop over the CPU oracle's functor.  TEST HELPER: nothing here
loads the library under test."""
import math
from fractions import Fraction

import numpy as np


def _q(v):
    """A number as the exact rational the library receives: a float stands for its binary value."""
    return Fraction(v)


def time_axis_len(start, stop, fps):
    """n = round(Int, fps * (stop - start)) (:150-151).  The reference forms the difference and the product in Float64, and
    so does this (3.21 - 0.21 is 3.0 there, and 12.5 * 3.0 a tie); the rounding itself is exact, ties to even.  None where
    the library refuses (stop <= start, fps <= 0, n < 1)."""
    if not (stop > start) or not (fps > 0):
        return None
    n = round(Fraction(float(fps) * (float(stop) - float(start))))     # round(Fraction) rounds half to even
    return n if n >= 1 else None


def time_axis_at(start, stop, fps, j):
    """ts[j] of range(start, stop, n) (:152) as an exact rational: start + j (stop - start) / (n - 1); start for n = 1."""
    n = time_axis_len(start, stop, fps)
    return _q(start) if n == 1 else _q(start) + j * (_q(stop) - _q(start)) / (n - 1)


def time_axis_float(start, stop, fps):
    """The same in Float64, operation by operation as include/pawsome_video.h states it: numpy's float64 arithmetic is IEEE
    double with every operation rounded on its own, so the library must give these bits."""
    n = time_axis_len(start, stop, fps)
    if n is None:
        return None
    start, stop = float(start), float(stop)
    if n == 1:
        return np.array([start])
    step = (stop - start) / float(n - 1)
    return start + np.arange(n, dtype=np.float64) * step


def time_axis_tolerance(start, stop):
    """Float64 against the exact value: the difference, the quotient and the product each round once (relative 2^-53 on
    a magnitude of at most |stop - start|) and so does the final sum (on at most max(|start|, |stop|))."""
    return 4 * 2.0 ** -53 * max(abs(start), abs(stop), abs(stop - start))


def fps_table(rate, n_frames, start, stop, fps):
    """The frames `ffmpeg -ss start -i f -t stop-start -vf fps=fps` selects, as include/pawsome_video.h recollects the
    rule, with the output slot o(i) = floor(i fps / rate + 1/2) in exact rationals.  The first frame i0 = ceil(start *
    rate) takes the Float64 product, as the header states: start = 0.2 at rate 30 means frame 6, which the exact product of
    the two binary values (a hair above 6) would miss.  None where the library refuses."""
    n = time_axis_len(start, stop, fps)
    if n is None or not (rate > 0) or n_frames <= 0 or not (start >= 0):
        return None
    i0 = math.ceil(float(start) * float(rate))
    if i0 >= n_frames:
        return None
    last = n_frames - 1 - i0
    o = lambda i: math.floor(Fraction(i) * _q(fps) / _q(rate) + Fraction(1, 2))
    count = min(n, o(last) + 1)
    slots = [o(i) for i in range(last + 1)]              # non-decreasing, slots[0] = 0
    out, i = [], 0
    for j in range(count):
        while i < last and slots[i + 1] <= j:            # max{ i : o(i) <= j }: the later frame of a slot wins, a gap repeats
            i += 1
        out.append(i0 + i)
    return out


def row_len(row):
    """Steps of a clip: the count of leading non-negative entries of its row."""
    n = 0
    while n < len(row) and row[n] >= 0:
        n += 1
    return n


def chain_indexed(oracle, frames, row, tw, ws, darker, start, fill, first=0):
    """out[0] = functor(frame row[0], start) (first = 0) or start as given (first = 1); out[k] = functor(frame row[k],
    out[k-1]) for k < row_len(row), under `fill`.  frames: host uint8 [n_frames, h, w]; ws in (h, w) order."""
    K = oracle.dog_kernel(oracle.sigma(tw), darker)
    radii = (ws[0] // 2, ws[1] // 2)
    out = []
    for k in range(row_len(row)):
        if k == 0 and first == 1:
            out.append((int(start[0]), int(start[1])))
        else:
            out.append(tuple(oracle.detect(frames[row[k]], fill, K, radii, out[-1] if k else start)))
    return out
