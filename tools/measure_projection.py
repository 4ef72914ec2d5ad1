"""Measurement of DESIGN.md section 15 (1 x MI355X): python tools/measure_projection.py.  The fused call against the two older paths at
1500 map points x 2000 keypoints, three repetitions of 200 alternating rounds; prints one JSON line each."""
import importlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__
mvo = __graft_entry__.load_package()
import torch
import projection_numpy as P
from test_gpu_projection_match import map_points, random_pose

rng = np.random.RandomState(3)
n_map, nt, COLS, ROWS, K = 1500, 2000, 640, 480, P.FR1_K
desc, t = mvo.synth.match_inputs("perturbed", n_map, nt, seed=5)
T = random_pose(rng)
pos = map_points(rng, n_map, T, K)
txy = rng.uniform([0, 0], [COLS, ROWS], (nt, 2)).astype(np.float32)
scale = (np.float32(1.2) ** rng.randint(0, 4, nt)).astype(np.float32)
ctx = mvo.Context(0)
m = ctx.map_create(); ctx.map_upload(m, pos, desc)
d_t = torch.from_numpy(t).cuda(); torch.cuda.synchronize()
want = P.knn2(pos, desc, T, K, COLS, ROWS, t, txy, 8.0, scale)
got = ctx.map_match_knn2_projection_dev(m, T, K, COLS, ROWS, d_t.data_ptr(), txy, 8.0, scale)
ok = all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
cnt = want[3]
print(json.dumps(dict(equal_to_transcription=ok, in_view=int((cnt >= 0).sum()), cand_per_point=float(cnt[cnt >= 0].mean()))), flush=True)
assert ok

def fused():
    ctx.map_match_knn2_projection_dev(m, T, K, COLS, ROWS, d_t.data_ptr(), txy, 8.0, scale)
def parent():
    idx, px, d = ctx.map_points_in_view(m, T, K, COLS, ROWS, cap=n_map)
    ctx.match_features_dev(d, len(idx), d_t.data_ptr(), nt, method=2, lowe_ratio=0.8)
def radius50():
    idx, px, d = ctx.map_points_in_view(m, T, K, COLS, ROWS, cap=n_map)
    ctx.match_features(desc[idx], t, method=3, xy1=px, xy2=txy, max_px=50.0)
paths = dict(fused=fused, parent=parent, radius50=radius50)
for f in paths.values():
    for _ in range(20): f()
for rep in range(3):
    ctx.profile_enable(True); ctx.profile_reset()
    wall = dict((k, 0.0) for k in paths)
    for _ in range(200):
        for k, f in paths.items():
            t0 = time.perf_counter(); f(); wall[k] += time.perf_counter() - t0
    prof = ctx.profile_get()
    print(json.dumps(dict(rep=rep, wall_us={k: round(v / 200 * 1e6, 1) for k, v in wall.items()}, kernels=prof), default=str), flush=True)
ctx.map_release(m); ctx.close()
