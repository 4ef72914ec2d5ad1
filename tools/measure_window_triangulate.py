"""Measurement of DESIGN.md section 20 (1 x MI355X): python tools/measure_window_triangulate.py.  The triangulation of new map
points against the window at 1500 keypoints x 19 frames x 1500 keypoints (what a keyframe of the 640 x 480 runs holds), one context
in latency mode: wall clock of the two C calls (mvo_window_triangulate_search, mvo_window_triangulate) and of the Python method with
profiling off, the device time of both kernels with profiling on (mvo_profile_enable); and the same work done the only way it could
be done before: 19 calls of mvo_match_knn2_epipolar, one per frame, each with its own upload, launch and wait, then 19 calls of
mvo_triangulate_points on as many pairs as the frame contributed (they cannot set aside the keypoints that are not free, and leave
the verification to the host; the work per pair is the same).  Three repetitions of 100 calls, one JSON line each."""
import ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__
mvo = __graft_entry__.load_package()
import window_triangulate_numpy as W
import test_gpu_window_triangulate as T

n, F, nk, REPS = 1500, 19, 1500, 100
K = W.FR1_K
s = W.scene(np.random.RandomState(5), n, [nk] * F, K=K, scales=True)
curr, frames = s["curr"], s["frames"]
ctx = mvo.Context(0)
want = W.window_triangulate(curr, frames, K)
got_raw, got = ctx.window_triangulate_search(curr, frames, K), ctx.window_triangulate(curr, frames, K)
T.assert_same(got_raw, want[3], T.RAW, "measure")
T.assert_same(got, want[:3], T.RULE, "measure")
pairs = want[1]
print(json.dumps(dict(equal_to_transcription=True, keypoints=n, n_frames=F, keypoints_per_frame=nk, counts=want[2].tolist(),
                      gated_pairs=int(np.maximum(want[3][2], 0).sum()), active_rows=int((want[3][2] >= 0).sum()))), flush=True)
carr, _, ckeep = ctx._fuse_frames([curr])
arr, _, keep = ctx._fuse_frames(frames)
p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
k = [C.c_double(K[name]) for name in ("fx", "fy", "cx", "cy")]
idx, dist, cnt = np.zeros((F, n, 2), np.int32), np.zeros((F, n, 2), np.int32), np.zeros((F, n), np.int32)
points, prs = np.zeros(n, mvo.WINDOW_POINT_DTYPE), np.zeros(F * nk, mvo.WINDOW_PAIR_DTYPE)
n_points, n_pairs, counts = C.c_int(), C.c_int(), np.zeros(12, np.int32)
Fs = [np.ascontiguousarray(mvo.fundamental_from_poses(curr["T"], fr["T"], K), np.float64).reshape(9) for fr in frames]
rel = [W.relative(curr, fr, 0.0) for fr in frames]
Rs, ts = [np.ascontiguousarray(r[0]) for r in rel], [np.ascontiguousarray(r[1]) for r in rel]
per = [pairs[pairs["frame"] == f] for f in range(F)]
kf = [np.ascontiguousarray(frames[f]["xy"][per[f]["train"]]) for f in range(F)]
kc = [np.ascontiguousarray(curr["xy"][per[f]["keypoint"]]) for f in range(F)]
out_f, out_c = [np.zeros((len(x), 3), np.float32) for x in kf], [np.zeros((len(x), 3), np.float32) for x in kf]

def c_search():
    assert ctx.lib.mvo_window_triangulate_search(ctx.h, carr, arr, F, *k, C.c_double(2.0), C.c_double(0.0), p(idx), p(dist), p(cnt)) == 0
def c_window():
    assert ctx.lib.mvo_window_triangulate(ctx.h, carr, arr, F, *k, None, p(points), n, C.byref(n_points), p(prs), len(prs), C.byref(n_pairs),
                                          p(counts)) == 0
def method():
    ctx.window_triangulate(curr, frames, K)
def per_frame():      # the search and the triangulation on the terms of the code before this call existed
    for f, fr in enumerate(frames):
        assert ctx.lib.mvo_match_knn2_epipolar(ctx.h, p(curr["desc"]), p(curr["xy"]), n, p(fr["desc"]), p(fr["xy"]), p(fr["scale"]), nk, p(Fs[f]),
                                               C.c_double(2.0), p(idx[f]), p(dist[f]), p(cnt[f])) == 0
    for f in range(F):
        if len(kf[f]):
            assert ctx.lib.mvo_triangulate_points(ctx.h, p(kf[f]), p(kc[f]), len(kf[f]), *k, p(Rs[f]), p(ts[f]), p(out_f[f]), p(out_c[f])) == 0
paths = dict(c_search=c_search, c_window_triangulate=c_window, method=method, per_frame_19_plus_19_calls=per_frame)
for f in paths.values():
    for _ in range(5): f()
for r in range(3):
    wall = dict((name, 0.0) for name in paths)
    for _ in range(REPS):
        for name, f in paths.items():
            t0 = time.perf_counter(); f(); wall[name] += time.perf_counter() - t0
    ctx.profile_enable(True); ctx.profile_reset()
    for _ in range(REPS): c_window(); per_frame()
    prof = ctx.profile_get()
    ctx.profile_enable(False)
    c_search()
    assert idx.tobytes() == want[3][0].tobytes() and cnt.tobytes() == want[3][2].tobytes()
    print(json.dumps(dict(rep=r, wall_us={name: round(v / REPS * 1e6, 1) for name, v in wall.items()}, kernels=prof), default=str), flush=True)
ctx.close()
