"""Measurement of DESIGN.md section 22 (1 x MI355X): python tools/measure_local_map.py.  mvo_map_match_knn2_local beside
mvo_map_match_knn2_projection, the first search, on the same resident map and the same frame keypoints: the shared scene of
tests/local_map_numpy.py with 700 and 2000 map points, 1100 and 2000 keypoints (and none: the prologue and the delivery alone),
8 levels; the first search with its 8 px radius
scaled by the keypoint's level.  One context: wall clock of the two Python methods with profiling off, the kernels' device time
with profiling on (mvo_profile_get); ten calls to warm up, then three repetitions of 100 calls, one JSON line per scene."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__
mvo = __graft_entry__.load_package()
import local_map_numpy as LM

CALLS, L = 100, 8

ctx = mvo.Context(0)
for n_map, nt in ((700, 0), (700, 1100), (2000, 0), (2000, 2000)):
    s = LM._scene(n_map, nt, L, 7 * n_map + nt)
    a = (s["T"], s["K"], s["cols"], s["rows"], s["t"], s["txy"], s["t_level"], s["level_scale"])
    scale = s["level_scale"][s["octave"]].astype(np.float32)
    m = ctx.map_create()
    ctx.map_upload(m, s["pos"], s["desc"])
    ctx.map_upload_view(m, s["normal"], s["max_dist"])
    want = LM.knn2(s["pos"], s["desc"], s["normal"], s["max_dist"], *a, s["skip"])
    got = ctx.map_match_knn2_local(m, *a, s["skip"])
    equal = all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    first = ctx.map_match_knn2_projection(m, s["T"], s["K"], s["cols"], s["rows"], s["t"], s["txy"], 8.0, scale)
    paths = dict(local=lambda: ctx.map_match_knn2_local(m, *a, s["skip"]),
                 projection=lambda: ctx.map_match_knn2_projection(m, s["T"], s["K"], s["cols"], s["rows"], s["t"], s["txy"], 8.0, scale))
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
    print(json.dumps(dict(n_map=n_map, nt=nt, levels=L, equal_to_transcription=bool(equal),
                          local=dict(active=int((got[3] >= 0).sum()), candidates=int(got[3][got[3] > 0].sum())),
                          projection=dict(in_view=int((first[3] >= 0).sum()), candidates=int(first[3][first[3] > 0].sum())),
                          reps=reps)), flush=True)
    ctx.map_release(m)
ctx.close()
