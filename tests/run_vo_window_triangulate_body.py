"""Body shared by tests/test_gpu_run_vo_window_triangulate.py (MI355X) and tests/test_run_vo_window_triangulate_sim.py (emulated
build): run_vo on the 24 rendered frames of tests/test_gpu_run_vo.py with `map_point_create_from_window: 1`, alone and together with
`map_point_fuse: 1`, `map_point_refine_positions: 1` and `map_point_refresh: 1`, with the key 0 and without the key.  From the
frame log alone, for every keyframe inserted while tracking: the numpy transcription (tests/window_triangulate_numpy.py) reproduces
the points (WPTS, WPTP, WPTC), the pairs (WPRS, WPRP, WPRC) and the counts (WCNT) from the set-up (WSET) and the buffered frames
(WKPN, WTWC, WDSC, WPIX, WSCL, WCON) byte for byte; the keyframe is the last of those frames; the new map points (WIDS, WPOS) are
the points in world coordinates, with ids of their own, and the map grew by exactly their number before the culling (WMSZ).  Over
the run there is a new point.  The log of the run with the key 0 has none of the records and equals the log of the run without the
key byte for byte; the trajectory stays inside the sanity bounds of test_gpu_run_vo.py."""
import subprocess

import numpy as np

import run_vo_map_refine_body as RF
import run_vo_map_refresh_body as RB
import vo_chain
import window_triangulate_numpy as W
from test_gpu_run_vo import EXE, _read_traj
from test_window_triangulate_host import SETUP, world_position

TAGS = ("WSET", "WKPN", "WTWC", "WDSC", "WPIX", "WSCL", "WCON", "WPTS", "WPTP", "WPTC", "WPRS", "WPRP", "WPRC", "WCNT", "WIDS", "WPOS",
        "WMSZ")
N, K0, K1 = RB.N, 0, RB.K1
BUFF = 20          # TrackingState::kBuffSize_

_CACHE = {}


def run(mvo, tmp_path, key, others, env):
    """key: None (absent), 0 or 1; others: the fusion, the refinement and the refresh on as well.  A run is made once per session
    and library and then shared, read-only; the frames on disk are those of the map-point refresh's body."""
    tmp_path.mkdir(exist_ok=True)
    which = (key, others, env.get("LD_LIBRARY_PATH", ""))
    if which in _CACHE:
        return _CACHE[which]
    if key is None and not others:
        _CACHE[which] = RB.run(mvo, tmp_path, None, False, env)     # the same run: no key of any kind
        return _CACHE[which]
    truth, base, base_traj = RB.dataset(mvo, tmp_path)
    out = tmp_path / ("window_%s_%d" % (key, others))
    out.mkdir()
    log_path, traj_path = out / "frames.log", out / "cam_traj.txt"
    assert base.count(base_traj) == 1
    text = base.replace(base_traj, str(traj_path)) + "save_frame_log_to: %s\nscale_factor: 1.2\n" % log_path
    if key is not None:
        text += "map_point_create_from_window: %d\n" % key
    if others:
        text += "map_point_fuse: 1\nmap_point_refine_positions: 1\nmap_point_refresh: 1\n"
    cfg = out / "config.yaml"
    cfg.write_text(text)
    r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    _CACHE[which] = dict(truth=truth, stdout=r.stdout, raw=open(log_path, "rb").read(), log=vo_chain.read_frame_log(log_path),
                         traj=_read_traj(traj_path))
    return _CACHE[which]


def window_records(rec):
    """The call of one keyframe as the transcription takes it."""
    setup = np.frombuffer(rec["WSET"], "<f8")
    kp = np.frombuffer(rec["WKPN"], "<i4")
    first = np.r_[0, np.cumsum(kp)]
    T = np.frombuffer(rec["WTWC"], "<f8").reshape(-1, 4, 4)
    desc = np.frombuffer(rec["WDSC"], np.uint8).reshape(-1, 32)
    xy = np.frombuffer(rec["WPIX"], "<f4").reshape(-1, 2)
    scale, conn = np.frombuffer(rec["WSCL"], "<f4"), np.frombuffer(rec["WCON"], "<i4")
    assert len(T) == len(kp) and len(desc) == len(xy) == len(scale) == len(conn) == first[-1]
    frames = [dict(desc=desc[a:b], xy=xy[a:b], scale=scale[a:b], conn=conn[a:b], T=T[f]) for f, (a, b) in enumerate(zip(first[:-1], first[1:]))]
    return setup, frames, first


def same(raw, want):
    """The bytes of a record against an array: equal, a NaN being a NaN whatever its sign."""
    want = np.ascontiguousarray(want)
    if len(raw) != want.nbytes:
        return False
    got = np.frombuffer(raw, want.dtype).reshape(want.shape)
    if want.dtype.kind == "f":
        u = "u%d" % want.dtype.itemsize
        return bool(((got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))).all())
    return raw == want.tobytes()


def check_on(on, others):
    log = on["log"]
    assert len(log) == N and len(on["traj"]) == N
    buff, n_keyframes, totals, ids_seen = [], 0, np.zeros(12, np.int64), set()
    for i, rec in enumerate(log):
        what = "frame %d: " % i
        tracked = "MORD" in rec
        if i in (K0, K1) or tracked:      # TrackingState::pushFrameToBuff
            buff = (buff + [i])[-BUFF:]
        flags = np.frombuffer(rec["FLAG"], "<i4") if tracked else np.zeros(2, "<i4")
        if not (tracked and flags[1]):
            assert not any(t in rec for t in TAGS), what + "not a keyframe inserted while tracking, yet it has window records"
            continue
        for t in TAGS:
            assert t in rec, what + "a keyframe without its %s record" % t
        setup, frames, first = window_records(rec)
        P = dict(W.DEFAULTS, ratio_factor=1.5 * 1.2)
        assert setup[4:].tolist() == [float(P[k]) for k in SETUP]
        K = dict(zip(("fx", "fy", "cx", "cy"), setup[:4]))
        assert len(frames) == len(buff) and 2 <= len(frames) <= BUFF
        pose = np.frombuffer(rec["POSE"], "<f8").reshape(4, 4)
        assert np.array_equal(frames[-1]["T"], pose), what + "the newest pose of the window is not the frame's"
        assert [len(fr["desc"]) for fr in frames] == [len(log[g]["KPTS"]) // 28 for g in buff], what + "the frames are not those of the buffer"
        assert frames[-1]["desc"].tobytes() == rec["DESC"]
        curr, older = frames[-1], frames[:-1]
        points, pairs, counts, _ = W.window_triangulate(curr, older, K, **P)
        for tag, want in (("WPTS", np.stack([points[k] for k in ("keypoint", "frame", "train", "hamming")], 1).astype(np.int32)),
                          ("WPTP", points["p_curr"]), ("WPTC", points["cos2"]),
                          ("WPRS", np.stack([pairs[k] for k in ("frame", "keypoint", "train", "hamming", "status")], 1).astype(np.int32)),
                          ("WPRP", np.concatenate([pairs["p_curr"], pairs["p_frame"]], 1)), ("WPRC", pairs["cos2"]), ("WCNT", counts)):
            assert same(rec[tag], want), what + "%s differs from the transcription" % tag
        # the new map points
        ids, size = np.frombuffer(rec["WIDS"], "<i4"), np.frombuffer(rec["WMSZ"], "<i4")
        assert len(ids) == len(points) == counts[11] and size[1] - size[0] == len(points), what + "the map did not grow by the new points"
        assert len(set(ids.tolist())) == len(ids) and not (set(ids.tolist()) & ids_seen), what + "an id was given twice"
        ids_seen |= set(ids.tolist())
        assert same(rec["WPOS"], world_position(points["p_curr"], pose)), what + "WPOS is not the points in world coordinates"
        # both keypoints of a new point were free
        assert (curr["conn"][points["keypoint"]] == -1).all()
        assert all(older[f]["conn"][j] == -1 for f, j in zip(points["frame"], points["train"]))
        after = np.frombuffer(rec["MIDS"], "<i4")
        n_keyframes += 1
        totals += counts
        print(what + "%d frames: free %d, active frames %d, rows %d, pairs %d, rejects (finite, depth, parallax, reprojection f, "
              "reprojection c, scale) %s, accepted %d, new points %d; I3DM %d; map %d -> %d, after the insertion %d (%d new ones kept)"
              % (len(frames), counts[0], counts[1], counts[2], counts[3], counts[4:10].tolist(), counts[10], counts[11],
                 len(rec["I3DM"]) // 16, size[0], size[1], len(after), len(set(after.tolist()) & set(ids.tolist()))))
    assert n_keyframes >= 2 and on["stdout"].count("new map points from the window") == n_keyframes
    assert totals[11] >= 1, "no new point over the run: %r" % totals
    err_t, err_r, travelled = RF.trajectory_error(on)
    print("others %d: %d keyframes, totals %s; max translation error %.3f of %.3f travelled, max rotation error %.2f deg"
          % (others, n_keyframes, totals.tolist(), err_t.max(), travelled, err_r.max()))
    # the sanity bounds of test_gpu_run_vo.py: 30 % of the distance travelled, 3 degrees
    assert err_t.max() < 0.3 * travelled and err_r.max() < 3.0, (on["stdout"], err_t, err_r)


def check_off(mvo, tmp_path, env):
    absent = run(mvo, tmp_path, None, False, env)
    zero = run(mvo, tmp_path, 0, False, env)
    assert zero["raw"] == absent["raw"], "the log with map_point_create_from_window: 0 differs from the log without the key"
    assert not any(t in rec for rec in zero["log"] for t in TAGS)
    assert "from the window" not in zero["stdout"] + absent["stdout"]
    assert np.array_equal(zero["traj"], absent["traj"])


def check_window(mvo, tmp_path, env, others):
    check_on(run(mvo, tmp_path, 1, others, env), others)
