"""The trackers, call sequences and batch sizes of the plan's characterisation recording (tests/golden/dispatch_paths.json):
tests/test_gpu_dispatch.py asks a tracker on the GPU, tests/test_plan_cpu.py replays the same through csrc/pdog_plan.hpp on
the host."""

# name: (frame_h, frame_w, target_width, window)
CASES = {
    "45x45_l29": (1080, 1920, 10, (45, 45)),          # the default window at the reference test's target width
    "45x45_l65": (1080, 1920, 25, (45, 45)),          # … and at the default one
    "63x63_l65": (1080, 1920, 25, (63, 63)),          # past 3000 pixels: the batch-size threshold decides
    "257x257_l65": (1080, 1920, 25, (257, 257)),      # cfg3: four strips and a thin column, tiled below three windows
    "257x257_l109": (1080, 1920, 44, (257, 257)),
    "513x513_l65_4k": (2160, 3840, 25, (513, 513)),   # cfg4
    "271x481_l65": (1080, 1920, 25, (271, 481)),      # cfg2
    "205x205_l293": (1080, 1920, 120, (205, 205)),    # cfg5: no roll instance, the two-pass path
    "15x15_l153": (1080, 1920, 63, (15, 15)),         # a two-pass tracker whose window fits the fused kernel: 256 | 257
    "45x45_l13": (1080, 1920, 4, (45, 45)),           # below ROLL_LMIN: a ring kernel
    "9801x45_l29": (1080, 1920, 10, (9801, 45)),      # too tall for the refinement's LDS block: exact mode is off
}
V, T = "set_variant", "set_tuning"
SEQUENCES = {
    "variants": [(V, 0), (V, 10), (V, 100), (V, 200), (V, 300), (V, -1)],
    "no_fused_c": [(T, "no_fused_c", 1), (T, "no_fused_c", 0)],
    "no_tiled": [(T, "no_tiled", 1), (T, "no_tiled", 0)],
    "v100_no_fused_c": [(V, 100), (T, "no_fused_c", 1)],
    "no_fused_c_v100": [(T, "no_fused_c", 1), (V, 100)],
}
BATCHES = [1, 2, 3, 16, 17, 256, 257, 1024, 1200, 4096]
