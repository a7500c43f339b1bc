"""The per-clip flow that track_clips / BatchTracker.track_clips must reproduce, restated on the CPU oracle: one
OracleTracker per clip with ITS OWN mode as fill (src/PawsomeTracker.jl:47-48), the bootstrap of :92-107 and the loop of
:161-167 — the same steps as pawsometracker.jl_amd/tracker.py's get_start_ij_and_tracker and _track_one, on the oracle.
TEST HELPER — plus the synthetic clips the clips tests share."""
import numpy as np

from oracle import synth
from oracle.dog_oracle import OracleTracker


def make_clip(h, w, tw, bkgd, start, step, n_frames, rng, noise=2):
    """n_frames frames of a dark disc walking from `start` (1-based row, col) by `step` per frame, +-noise grey levels."""
    fr = np.stack([synth.disc_frame(h, w, (start[0] + k * step[0], start[1] + k * step[1]), tw, True, bkgd=bkgd)
                   for k in range(n_frames)])
    return np.clip(fr.astype(np.int16) + rng.integers(-noise, noise + 1, fr.shape), 0, 255).astype(np.uint8)


def chain(oracle, clip, tw, ws, darker, start, fill=None, first=0, length=None):
    """out[0] = functor(frame 0, start) (first = 0) or start as given (first = 1); out[k] = functor(frame k, out[k-1]) for
    k < length.  fill None: the clip's own mode (what OracleTracker computes), otherwise forced."""
    n = len(clip) if length is None else int(length)
    if n == 0:
        return []
    ot = OracleTracker(clip[0], tw, ws, darker, oracle)
    if fill is not None:
        ot.fill = int(fill)
    out = [ot(start) if first == 0 else (int(start[0]), int(start[1]))]
    for f in clip[1:n]:
        ot.data[...] = f                                         # :166
        out.append(ot(out[-1]))                                  # :167
    return out


def get_guess(start_location, shape, sar=1.0):
    """src/PawsomeTracker.jl:74-90 with the spellings of tracker.py's get_guess."""
    if start_location is None:
        return (shape[0] // 2, shape[1] // 2)
    if isinstance(start_location, tuple) and len(start_location) == 2 and start_location[0] == "ij":
        return (int(start_location[1][0]), int(start_location[1][1]))
    x, y = start_location
    return (int(np.rint(y)), int(np.rint(x / sar)))


def bootstrap(oracle, img, tw, ws, darker, start_location, sar=1.0):
    """src/PawsomeTracker.jl:92-107: the first position of a clip whose first frame is img."""
    guess = get_guess(start_location, img.shape, sar)
    if start_location is None:                                   # :99-107, the sz .÷ 4 window
        return OracleTracker(img, tw, (img.shape[0] // 4, img.shape[1] // 4), darker, oracle)(guess)
    return OracleTracker(img, tw, ws, darker, oracle)(guess)     # :94-95


def track_clip(oracle, clip, tw, ws, darker, start_location, sar=1.0, length=None):
    """One clip as the reference's track_one tracks it (ws already in (h, w) order): a list of `length` positions."""
    n = len(clip) if length is None else int(length)
    if n == 0:
        return []
    ij = bootstrap(oracle, clip[0], tw, ws, darker, start_location, sar)
    return chain(oracle, clip, tw, ws, darker, ij, first=1, length=n)
