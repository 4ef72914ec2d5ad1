"""Measurement of DESIGN.md section 17 (1 x MI355X): python tools/measure_map_refresh.py.  mvo_map_refresh at 1000 map points x 20
observations (what a keyframe of the 640 x 480 runs holds): wall clock of the C call and of the Python method with profiling
off, the kernel's device time with profiling on, and the same call without observations (upload of the starts, launch and wait
only); three repetitions of 200 calls, one JSON line each."""
import ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__
mvo = __graft_entry__.load_package()
import map_refresh_numpy as R
from test_gpu_map_refresh import observations, points_in_view

rng = np.random.RandomState(3)
n, m_obs = 1000, 20
pos = points_in_view(rng, n)
desc = rng.randint(0, 256, (n, 32)).astype(np.uint8)
obs_desc, obs_cam, start = observations(rng, [m_obs] * n, 0.08)
none = np.zeros(n + 1, np.int32)
ctx = mvo.Context(0)
m = ctx.map_create(); ctx.map_upload(m, pos, desc)
want = R.refresh(pos, desc, obs_desc, obs_cam, start)
got = ctx.map_refresh(m, obs_desc, obs_cam, start)
ok = got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and R.same_f64(got[2], want[2])
print(json.dumps(dict(equal_to_transcription=bool(ok), n=n, n_obs=len(obs_desc), other_than_first=int((want[0] > 0).sum()))), flush=True)
assert ok
choice, out, norm = np.zeros(n, np.int32), np.zeros((n, 32), np.uint8), np.zeros((n, 3))
p = lambda a: a.ctypes.data_as(C.c_void_p)

def c_call():
    assert ctx.lib.mvo_map_refresh(ctx.h, m, p(obs_desc), p(obs_cam), p(start), len(obs_desc), p(choice), p(out), p(norm)) == 0
def c_call_no_obs():
    assert ctx.lib.mvo_map_refresh(ctx.h, m, None, None, p(none), 0, p(choice), p(out), p(norm)) == 0
def method():
    ctx.map_refresh(m, obs_desc, obs_cam, start)
paths = dict(c_call=c_call, c_call_no_obs=c_call_no_obs, method=method)
for f in paths.values():
    for _ in range(20): f()
for rep in range(3):
    wall = dict((k, 0.0) for k in paths)
    for _ in range(200):
        for k, f in paths.items():
            t0 = time.perf_counter(); f(); wall[k] += time.perf_counter() - t0
    ctx.profile_enable(True); ctx.profile_reset()
    for _ in range(200): c_call()
    prof = ctx.profile_get()
    ctx.profile_reset()
    for _ in range(200): c_call_no_obs()
    prof0 = ctx.profile_get()
    ctx.profile_enable(False)
    print(json.dumps(dict(rep=rep, wall_us={k: round(v / 200 * 1e6, 1) for k, v in wall.items()}, kernels=prof, kernels_no_obs=prof0),
                     default=str), flush=True)
ctx.map_release(m); ctx.close()
