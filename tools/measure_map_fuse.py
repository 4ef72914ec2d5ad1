"""Measurement of DESIGN.md section 19 (1 x MI355X): python tools/measure_map_fuse.py.  The fusion search at 1000 map points x 20
frames x 1500 keypoints (what a keyframe of the 640 x 480 runs holds), one context in latency mode: wall clock of the two C calls
(mvo_map_fuse_search, mvo_map_fuse) and of the Python method with profiling off, the kernel's device time with profiling on
(mvo_profile_enable); and the same search done the only way it could be done before: 20 calls of mvo_map_match_knn2_projection,
one per frame, each with its own upload, launch and wait (they cannot set aside the pairs already connected; the work per pair
is the same).  Three repetitions of 200 calls, one JSON line each."""
import ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__
mvo = __graft_entry__.load_package()
import map_fuse_numpy as M

n, F, nk, COLS, ROWS = 1000, 20, 1500, 640, 480
K = M.FR1_K
s = M.scene(np.random.RandomState(5), n, [nk] * F, K=K, cols=COLS, rows=ROWS, scales=True)
pos, desc, frames = s["pos"], s["desc"], s["frames"]
ctx = mvo.Context(0)
m = ctx.map_create(); ctx.map_upload(m, pos, desc)
raw = M.search(pos, desc, frames, K, COLS, ROWS, M.DEFAULT_MAX_PX)
want = M.resolve(n, frames, raw[0], raw[1], M.DEFAULT_MAX_HAMMING)
got_raw, got = ctx.map_fuse_search(m, frames, K, COLS, ROWS, M.DEFAULT_MAX_PX), ctx.map_fuse(m, frames, K, COLS, ROWS)
ok = all(g.tobytes() == w.tobytes() for g, w in zip(got_raw, raw)) and got[0].tobytes() == want[0].tobytes() and \
    np.stack([got[1][k] for k in got[1].dtype.names], 1).tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
print(json.dumps(dict(equal_to_transcription=bool(ok), n_map=n, n_frames=F, keypoints_per_frame=nk, counts=want[2].tolist(),
                      gated_pairs=int(np.maximum(raw[2], 0).sum()), active_pairs=int((raw[2] >= 0).sum()))), flush=True)
assert ok
arr, _, keep = ctx._fuse_frames(frames)
p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
k = [C.c_double(K[name]) for name in ("fx", "fy", "cx", "cy")]
idx, dist = np.zeros((F, n, 2), np.int32), np.zeros((F, n, 2), np.int32)
cnt, px = np.zeros((F, n), np.int32), np.zeros((F, n, 2), np.float32)
rep, added, n_added, counts = np.zeros(n, np.int32), np.zeros((F * nk, 3), np.int32), C.c_int(), np.zeros(6, np.int32)
Ts = [np.ascontiguousarray(fr["T"], np.float64).reshape(16) for fr in frames]

def c_search():
    assert ctx.lib.mvo_map_fuse_search(ctx.h, m, arr, F, *k, COLS, ROWS, C.c_double(M.DEFAULT_MAX_PX), p(idx), p(dist), p(cnt), p(px)) == 0
def c_fuse():
    assert ctx.lib.mvo_map_fuse(ctx.h, m, arr, F, *k, COLS, ROWS, None, p(rep), p(added), len(added), C.byref(n_added), p(counts)) == 0
def method():
    ctx.map_fuse(m, frames, K, COLS, ROWS)
def per_frame():      # the search on the terms of the code before this call existed
    for f, fr in enumerate(frames):
        assert ctx.lib.mvo_map_match_knn2_projection(ctx.h, m, p(Ts[f]), *k, COLS, ROWS, p(fr["desc"]), p(fr["xy"]), p(fr["scale"]), nk,
                                                     C.c_double(M.DEFAULT_MAX_PX), p(px[f]), p(idx[f]), p(dist[f]), p(cnt[f])) == 0
paths = dict(c_search=c_search, c_fuse=c_fuse, method=method, per_frame_20_calls=per_frame)
for f in paths.values():
    for _ in range(10): f()
for r in range(3):
    wall = dict((name, 0.0) for name in paths)
    for _ in range(200):
        for name, f in paths.items():
            t0 = time.perf_counter(); f(); wall[name] += time.perf_counter() - t0
    ctx.profile_enable(True); ctx.profile_reset()
    for _ in range(200): c_search(); per_frame()
    prof = ctx.profile_get()
    ctx.profile_enable(False)
    c_search()
    assert idx.tobytes() == raw[0].tobytes() and cnt.tobytes() == raw[2].tobytes()
    print(json.dumps(dict(rep=r, wall_us={name: round(v / 200 * 1e6, 1) for name, v in wall.items()}, kernels=prof), default=str), flush=True)
ctx.map_release(m); ctx.close()
