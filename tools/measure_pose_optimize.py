"""Measurement of DESIGN.md section 21 (1 x MI355X): python tools/measure_pose_optimize.py.  mvo_optimize_pose beside
mvo_solve_pnp_ransac on the same matches, n = 300, 1000 and 2000, two scenes: the test scene (0.5 px noise, every fifth
observation moved by (40, -30) px, a start 2 degrees and about 5 % of the depth away) and one where half the pixels are replaced
by random ones, so that RANSAC's adaptive count stays above its 100 iterations; one context in "latency" mode and in "shared"
mode: wall clock of the two Python methods with profiling off, the kernels' device time with profiling on (mvo_profile_get);
three repetitions of 100 calls, one JSON line each."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__
mvo = __graft_entry__.load_package()
import pose_optimize_numpy as R

K = {k: float(np.float32(v)) for k, v in R.FR1_K.items()}
CALLS = 100


def scenes(n):
    rng = np.random.RandomState(n)
    p3, p2, T, _, _ = R.scene(rng, n, 0.5, 5)
    yield "test", p3, p2, T
    p3, p2, T, _, _ = R.scene(rng, n, 0.5)
    p2 = p2.copy()
    bad = rng.permutation(n)[:n // 2]
    p2[bad] = np.stack([rng.uniform(0, 640, len(bad)), rng.uniform(0, 480, len(bad))], 1).astype(np.float32)
    yield "half_random", p3, p2, T


ctx = mvo.Context(0)
for mode in ("latency", "shared"):
    ctx.ba_set_mode(mode)
    for n in (300, 1000, 2000):
        for name, p3, p2, T in scenes(n):
            T_init = R.perturbed(T, 2.0, (0.1, -0.1, 0.15))
            want = R.optimize_pose(p3, p2, None, T_init, K)
            got = ctx.optimize_pose(p3, p2, T_init, K)
            equal = all(g.tobytes() == np.ascontiguousarray(w).tobytes() for g, w in zip(got, want))
            pnp = ctx.solve_pnp_ransac(p3, p2, K)
            paths = dict(optimize_pose=lambda: ctx.optimize_pose(p3, p2, T_init, K), solve_pnp_ransac=lambda: ctx.solve_pnp_ransac(p3, p2, K))
            for f in paths.values():
                for _ in range(10): f()
            reps = []
            for rep in range(3):
                wall = {}
                for key, f in paths.items():
                    t0 = time.perf_counter()
                    for _ in range(CALLS): f()
                    wall[key] = round((time.perf_counter() - t0) / CALLS * 1e6, 1)
                ctx.profile_enable(True); ctx.profile_reset()
                for f in paths.values():
                    for _ in range(CALLS): f()
                prof = {k: round(v[1] / v[0] * 1e3, 1) for k, v in ctx.profile_get().items() if v[0]}
                ctx.profile_enable(False)
                reps.append(dict(wall_us=wall, kernel_us_per_launch=prof))
            print(json.dumps(dict(mode=mode, n=n, scene=name, equal_to_transcription=bool(equal), info=got[4].tolist(),
                                  pnp_ok=bool(pnp["ok"]), pnp_inliers=int(len(pnp["inliers"])), reps=reps)), flush=True)
ctx.close()
