"""Measurement of DESIGN.md section 14 (1 x MI355X): python tools/measure_epipolar.py.  The gated call against the all-pairs 2-NN at
1200 queries x 1500 trains, scaled 2 px band, three repetitions of 200 alternating rounds; prints one JSON line each."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__
mvo = __graft_entry__.load_package()
import torch
import epipolar_numpy as E
from test_gpu_epipolar_match import random_pose

rng = np.random.RandomState(3)
nq, nt = 1200, 1500
q, t = mvo.synth.match_inputs("perturbed", nq, nt, seed=5)
qxy = rng.uniform([0, 0], [640, 480], (nq, 2)).astype(np.float32)
txy = rng.uniform([0, 0], [640, 480], (nt, 2)).astype(np.float32)
F = mvo.fundamental_from_poses(random_pose(rng), random_pose(rng), E.FR1_K)
scale = (np.float32(1.2) ** rng.randint(0, 4, nt)).astype(np.float32)
ctx = mvo.Context(0)
d_q, d_t = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda(); torch.cuda.synchronize()
want = E.knn2(q, qxy, t, txy, F, 2.0, scale)
got = ctx.match_knn2_epipolar_dev(d_q.data_ptr(), qxy, d_t.data_ptr(), txy, F, 2.0, scale)
ok = all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
print(json.dumps(dict(equal_to_transcription=ok, cand_per_query=float(want[2].mean()))), flush=True)
assert ok

def gated():
    ctx.match_knn2_epipolar_dev(d_q.data_ptr(), qxy, d_t.data_ptr(), txy, F, 2.0, scale)
def all_pairs():
    ctx.match_knn2_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt)
paths = dict(gated=gated, all_pairs=all_pairs)
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
ctx.close()
