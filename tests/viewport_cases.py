"""The cases the CPU and the GPU tests of viewport.py share: source h x w, view vh x vw, ss, then yaw, pitch, roll, hfov,
vfov in degrees.  tests/test_viewport_cpu.py holds every grid sample of every one of them at least 1e-6 of a 1/256-pixel
step away from a rounding boundary of the map, which is what lets tests/test_gpu_viewport.py ask the device's map for
equality.  (Neighbouring choices do not hold the margin: vfov 100 in the third row, ss 2 in the fourth and ss 4 in the
second fall to 1e-7 .. 7e-7.  A changed case keeps the margin test green by other angles, never by a lower margin.)"""
CASES = [
    (32, 64, 9, 15, 1, (30, 20, 10, 90, 67.5)),           # one tile
    (50, 99, 37, 70, 2, (-75.5, 90, 0, 60, 60)),          # odd width, every footprint at a pole, ragged tile
    (6, 2100, 5, 300, 1, (0, -90, 45, 120, 101)),         # wider than any tile
    (32, 64, 37, 70, 3, (123.25, -33.5, -170, 100.5, 40)),   # inexact scale
    (50, 99, 9, 15, 4, (30, 20, 10, 90, 67.5)),
    (50, 99, 5, 300, 2, (123.25, -33.5, -170, 100.5, 40)),
]
ANGLES = [CASES[k][5] for k in range(4)]   # the four angle sets


def case_id(case):
    return "%dx%d_%dx%d_ss%d_%g_%g_%g_%g_%g" % (tuple(case[:5]) + tuple(case[5]))
