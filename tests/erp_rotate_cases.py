"""The (shape, angles) cases the CPU and the GPU tests of erp_rotate share (tests/test_erp_rotate_cpu.py holds every one
of them at least 1e-6 of a 1/256-pixel step away from a rounding boundary of the map, in both directions, which is what
lets tests/test_gpu_erp_rotate.py ask the device's map for equality)."""
SHAPES = [(32, 64), (50, 100), (48, 130), (6, 2100)]          # (6, 2100) is wider than any column tile
ANGLES = [(30, 20, 10), (-75.5, 90, 0), (0, -90, 45), (123.25, -33.5, -170)]   # degrees: yaw, pitch, roll
CASES = [(h, w, a) for (h, w) in SHAPES for a in ANGLES]


def case_id(case):
    return "%dx%d_%g_%g_%g" % ((case[0], case[1]) + tuple(case[2]))
