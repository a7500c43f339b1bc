"""MI355X-native DoG + argmax hot path behind PawsomeTracker's `Tracker` API.

Directory name follows the build contract (`pawsometracker.jl_amd/`); import it
as `pawsometracker_jl_amd` (the loader stub at the repo root registers it).
"""
from ._lib import LIB_PATH, PdogError, lib  # noqa: F401
from .tracker import (DEFAULT_STOP, Tracker, fix_window_size, fps_table, get_guess, get_sigma,  # noqa: F401
                      get_start_ij_and_tracker, guess_window_size, headings, mode, shape_derive, subpixel, time_axis,
                      track_clips, track_frames, track_segments, track_video)
from .batch import BatchTracker, GroupTracker, gather_positions, mode_device, shard_range  # noqa: F401
from .diagnose import DIAG_MAX_TARGETS, DIAG_SIZE, Diagnose, diag_point  # noqa: F401
from .background import BG_MAX_SAMPLES, Background, background_samples  # noqa: F401
from ._lib import SHAPE_MAX_RADIUS  # noqa: F401
from .frame_blobs import FB_WORDS, FrameBlobs, frame_blobs_derive  # noqa: F401
