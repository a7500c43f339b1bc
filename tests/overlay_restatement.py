"""NumPy restatement of the overlay over a frame table and for several targets (include/pawsome_overlay.h), built on
tests/diag_restatement.py: output k is resize(frames[table[k]]); on it, for every target, the dot at the target's scaled
position of step k and the path of the target's own trace (its last <= 100 scaled points, oldest first).  All draws are of
one colour, so the targets need no order among themselves.  Test code only: the library never imports it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diag_restatement as R  # noqa: E402


class Overlay:
    """One trace per target, running on across calls like diag_restatement.Diagnose's single one."""

    def __init__(self, n_targets=1, darker_target=True):
        self.color = 255 if darker_target else 0
        self.traces = [[] for _ in range(n_targets)]

    def set_targets(self, n_targets):
        self.traces = [[] for _ in range(n_targets)]

    def step(self, img, ijs):
        """One output: img resized, then every target's push, dot and path (ijs: one 1-based (row, col) per target)."""
        assert len(ijs) == len(self.traces)
        img = np.asarray(img)
        h, w = img.shape
        buf = R.resize(img)
        for trace, ij in zip(self.traces, ijs):
            q = R.point(h, w, (int(ij[0]), int(ij[1])))
            trace.append(q)
            del trace[:-R.TRACE]
            R.dot(buf, q, self.color)
            for a, b in zip(trace[:-1], trace[1:]):
                R.bresenham(buf, a, b, self.color)
        return buf

    def render(self, frames, table, ij):
        """frames [n_frames, h, w], table [n_steps], ij [n_targets, n_steps, 2] -> uint8 [n_steps, 360, 640]."""
        ij = np.asarray(ij)
        assert ij.shape == (len(self.traces), len(table), 2)
        if len(table) == 0:
            return np.zeros((0, R.H, R.W), np.uint8)
        return np.stack([self.step(frames[int(f)], ij[:, k]) for k, f in enumerate(table)])
