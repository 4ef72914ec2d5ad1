"""Measurement of DESIGN.md section 18 (1 x MI355X): python tools/measure_map_refine.py.  mvo_map_refine_positions at 1000 map points
x 20 observations in 20 frames (what a keyframe of the 640 x 480 runs holds), one context in latency mode: wall clock of the C
call and of the Python method with profiling off, the kernel's device time with profiling on (mvo_profile_enable); three
repetitions of 200 calls, one JSON line each.  The positions are put back before every call, so every call does the same work."""
import ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__
mvo = __graft_entry__.load_package()
import map_refine_numpy as R

rng = np.random.RandomState(3)
n, m_obs = 1000, 20
K = {k: float(np.float32(v)) for k, v in R.FR1_K.items()}
truth, pos, T, frame, uv, start, _ = R.scene(rng, [m_obs] * n, 20, 0.5, 5, K=K)
T = np.ascontiguousarray(T, np.float64)
ctx = mvo.Context(0)
m = ctx.map_create(); ctx.map_upload(m, pos, np.zeros((n, 32), np.uint8))
want = R.refine(pos, T, K, frame, uv, start)
got = ctx.map_refine_positions(m, T, K, frame, uv, start)
ok = all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
print(json.dumps(dict(equal_to_transcription=bool(ok), n=n, n_obs=len(uv), refined=int((want[2][:, 0] == 0).sum()),
                      accepted_steps_mean=float(want[2][:, 1].mean()), trials_mean=float(want[2][:, 2].mean()), trials_max=int(want[2][:, 2].max()))), flush=True)
assert ok
out_pos, chi2, info, flags = np.zeros((n, 3), np.float32), np.zeros((n, 2)), np.zeros((n, 3), np.int32), np.zeros(len(uv), np.uint8)
p = lambda a: a.ctypes.data_as(C.c_void_p)
k = [C.c_double(K[name]) for name in ("fx", "fy", "cx", "cy")]

def reset():
    ctx.map_update_positions(m, pos, first=0)
def c_call():
    assert ctx.lib.mvo_map_refine_positions(ctx.h, m, p(T), 20, *k, p(frame), p(uv), p(start), len(uv), None, p(out_pos), p(chi2), p(info), p(flags)) == 0
def method():
    ctx.map_refine_positions(m, T, K, frame, uv, start)
paths = dict(c_call=c_call, method=method)
for f in paths.values():
    for _ in range(20): reset(); f()
for rep in range(3):
    wall = dict((name, 0.0) for name in paths)
    for _ in range(200):
        for name, f in paths.items():
            reset()
            t0 = time.perf_counter(); f(); wall[name] += time.perf_counter() - t0
    ctx.profile_enable(True); ctx.profile_reset()
    for _ in range(200): reset(); c_call()
    prof = ctx.profile_get()
    ctx.profile_enable(False)
    assert out_pos.tobytes() == want[0].tobytes()
    print(json.dumps(dict(rep=rep, wall_us={name: round(v / 200 * 1e6, 1) for name, v in wall.items()}, kernels=prof), default=str), flush=True)
ctx.map_release(m); ctx.close()
