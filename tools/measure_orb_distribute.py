"""Measurement of DESIGN.md section 16 (1 x MI355X, idle): MVO_HOST_TIMING=1 python tools/measure_orb_distribute.py.  One context,
one 640 x 480 frame of the world texture at full and at a quarter of its contrast, nfeatures 2000: the two detectors alternate,
three repetitions of 200 rounds.  Prints one JSON line per repetition: wall time per call of both detectors and the device time
of their kernels (k_fast_cells + k_ic_angle beside k_fast_harris; k_pyramid is common to both).  With MVO_HOST_TIMING=1 the
library prints the host stages of both to stderr every 200 frames (quadtree beside retain)."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__
mvo = __graft_entry__.load_package()
import orb_distribute_numpy as D
from test_gpu_orb_distribute import texture_frame

P = dict(nfeatures=2000, scale_factor=1.2, nlevels=4, fast_threshold=20, pyramid_interpolation=1, grid_size=16,
         max_keypoints=1 << 20, grid_max_per_cell=1 << 20)
ctx = mvo.Context(0, **P)
ctx.orb_distribute_configure()
for name, quarter in (("full", False), ("quarter", True)):
    img = np.repeat(texture_frame(mvo, quarter)[:, :, None], 3, axis=2)
    want = D.OrbDistribute(**P).detect(img)
    got = ctx.calc_keypoints_distributed(img, cap=4096)
    n_cand = len(ctx.debug_distribute_candidates())
    n_old = len(ctx.calc_keypoints(img, cap=4096))
    print(json.dumps(dict(frame=name, equal_to_transcription=got.tobytes() == want.tobytes(), candidates=n_cand,
                          keypoints_distributed=len(got), keypoints_existing=n_old)), flush=True)
    assert got.tobytes() == want.tobytes()
    paths = dict(distributed=lambda: ctx.calc_keypoints_distributed(img, cap=4096), existing=lambda: ctx.calc_keypoints(img, cap=4096))
    for f in paths.values():
        for _ in range(20): f()
    for rep in range(3):
        ctx.profile_enable(True); ctx.profile_reset()
        wall = dict((k, 0.0) for k in paths)
        for _ in range(200):
            for k, f in paths.items():
                t0 = time.perf_counter(); f(); wall[k] += time.perf_counter() - t0
        prof = ctx.profile_get()
        ctx.profile_enable(False)
        # (profiling brackets every launch with two events: the wall times below are taken in a second pass without them)
        wall2 = dict((k, 0.0) for k in paths)
        for _ in range(200):
            for k, f in paths.items():
                t0 = time.perf_counter(); f(); wall2[k] += time.perf_counter() - t0
        print(json.dumps(dict(frame=name, rep=rep, wall_us={k: round(v / 200 * 1e6, 1) for k, v in wall2.items()},
                              wall_us_profiled={k: round(v / 200 * 1e6, 1) for k, v in wall.items()}, kernels=prof), default=str), flush=True)
ctx.close()
