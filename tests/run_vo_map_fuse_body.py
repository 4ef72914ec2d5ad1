"""Body shared by tests/test_gpu_run_vo_map_fuse.py (MI355X) and tests/test_run_vo_map_fuse_sim.py (emulated build): run_vo on the
24 rendered frames of tests/test_gpu_run_vo.py with `map_point_fuse: 1`, alone and together with `map_point_refine_positions: 1`
and `map_point_refresh: 1`, with the key 0 and without the key.  From the frame log alone, for every keyframe inserted while
tracking: the numpy transcription (tests/map_fuse_numpy.py) reproduces replaced_by (UREP), the added observations (UADD) and the
counts (UCNT) from the set-up (USET), the map as resident (UPOS, UMDS) and the buffered frames (UKPN, UTWC, UDSC, UPIX, USCL, UCON)
byte for byte; the map after the call (UIDS, and MIDS after the insertion) is the map before it (UMID) without the replaced
points, in number exactly the points replaced; the connections the NEXT fuse reads in the frames both calls share are those this
call left -- every connection of a replaced point names its survivor, every added observation is connected -- so no connection
names a replaced id; with the other two keys on, the observation counts of the refinement (FOBS) and of the refresh (ROBS) at
the same keyframe are the fused ones.  Over the run there is a merge and an added observation.  The log of the run with the key 0
has none of the records and equals the log of the run without the key byte for byte; the trajectory stays inside the sanity
bounds of test_gpu_run_vo.py."""
import subprocess

import numpy as np

import map_fuse_numpy as M
import run_vo_map_refine_body as RF
import run_vo_map_refresh_body as RB
import vo_chain
from test_gpu_run_vo import EXE, _read_traj

TAGS = ("USET", "UMID", "UPOS", "UMDS", "UKPN", "UTWC", "UDSC", "UPIX", "USCL", "UCON", "UREP", "UADD", "UCNT", "UIDS")
N, K0, K1 = RB.N, 0, RB.K1
BUFF = 20          # TrackingState::kBuffSize_

_CACHE = {}


def run(mvo, tmp_path, key, others, env):
    """key: None (absent), 0 or 1; others: the refinement and the refresh on as well.  A run is made once per session and library
    and then shared, read-only; the frames on disk are those of the map-point refresh's body."""
    tmp_path.mkdir(exist_ok=True)
    which = (key, others, env.get("LD_LIBRARY_PATH", ""))
    if which in _CACHE:
        return _CACHE[which]
    if key is None and not others:
        _CACHE[which] = RB.run(mvo, tmp_path, None, False, env)     # the same run: no key of any kind
        return _CACHE[which]
    truth, base, base_traj = RB.dataset(mvo, tmp_path)
    out = tmp_path / ("fuse_%s_%d" % (key, others))
    out.mkdir()
    log_path, traj_path = out / "frames.log", out / "cam_traj.txt"
    assert base.count(base_traj) == 1
    text = base.replace(base_traj, str(traj_path)) + "save_frame_log_to: %s\nscale_factor: 1.2\n" % log_path
    if key is not None:
        text += "map_point_fuse: %d\n" % key
    if others:
        text += "map_point_refine_positions: 1\nmap_point_refresh: 1\n"
    cfg = out / "config.yaml"
    cfg.write_text(text)
    r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    _CACHE[which] = dict(truth=truth, stdout=r.stdout, raw=open(log_path, "rb").read(), log=vo_chain.read_frame_log(log_path),
                         traj=_read_traj(traj_path))
    return _CACHE[which]


def fuse_records(rec):
    """The call of one keyframe as the transcription takes it."""
    setup = np.frombuffer(rec["USET"], "<f8")
    kp = np.frombuffer(rec["UKPN"], "<i4")
    first = np.r_[0, np.cumsum(kp)]
    T = np.frombuffer(rec["UTWC"], "<f8").reshape(-1, 4, 4)
    desc = np.frombuffer(rec["UDSC"], np.uint8).reshape(-1, 32)
    xy = np.frombuffer(rec["UPIX"], "<f4").reshape(-1, 2)
    scale, conn = np.frombuffer(rec["USCL"], "<f4"), np.frombuffer(rec["UCON"], "<i4")
    assert len(T) == len(kp) and len(desc) == len(xy) == len(scale) == len(conn) == first[-1]
    frames = [dict(desc=desc[a:b], xy=xy[a:b], scale=scale[a:b], conn=conn[a:b], T=T[f]) for f, (a, b) in enumerate(zip(first[:-1], first[1:]))]
    return setup, frames, first


def check_on(on, others):
    log = on["log"]
    assert len(log) == N and len(on["traj"]) == N
    buff, left, n_keyframes, totals = [], None, 0, np.zeros(6, np.int64)
    for i, rec in enumerate(log):
        what = "frame %d: " % i
        tracked = "MORD" in rec
        if i in (K0, K1) or tracked:      # TrackingState::pushFrameToBuff
            buff = (buff + [i])[-BUFF:]
        flags = np.frombuffer(rec["FLAG"], "<i4") if tracked else np.zeros(2, "<i4")
        if not (tracked and flags[1]):
            assert not any(t in rec for t in TAGS), what + "not a keyframe inserted while tracking, yet it has fusion records"
            continue
        for t in TAGS:
            assert t in rec, what + "a keyframe without its %s record" % t
        setup, frames, first = fuse_records(rec)
        assert len(setup) == 8 and setup[4:].tolist() == [640.0, 480.0, M.DEFAULT_MAX_PX, M.DEFAULT_MAX_HAMMING]
        K = dict(zip(("fx", "fy", "cx", "cy"), setup[:4]))
        ids = np.frombuffer(rec["UMID"], "<i4")
        pos = np.frombuffer(rec["UPOS"], "<f4").reshape(-1, 3)
        desc = np.frombuffer(rec["UMDS"], np.uint8).reshape(-1, 32)
        n = len(ids)
        assert len(pos) == n == len(desc) and n > 100 and len(frames) == len(buff) and 2 <= len(frames) <= BUFF
        assert np.array_equal(frames[-1]["T"], np.frombuffer(rec["POSE"], "<f8").reshape(4, 4)), what + "the newest pose of the window is not the frame's"
        assert [len(fr["desc"]) for fr in frames] == [len(log[g]["KPTS"]) // 28 for g in buff], what + "the frames are not those of the buffer"
        assert frames[-1]["desc"].tobytes() == rec["DESC"]
        rep, added, counts = M.fuse(pos, desc, frames, K, 640, 480, setup[6], int(setup[7]))
        assert rec["UREP"] == rep.tobytes(), what + "UREP differs from the transcription"
        assert rec["UADD"] == added.tobytes(), what + "UADD differs from the transcription"
        assert rec["UCNT"] == counts.tobytes(), what + "UCNT differs from the transcription"
        after = np.frombuffer(rec["UIDS"], "<i4")
        assert sorted(after.tolist()) == sorted(ids[rep == np.arange(n)].tolist()), what + "the map after the call is not the map without the replaced points"
        assert n - len(after) == counts[5], what + "the map did not shrink by exactly the number of points replaced"
        assert np.array_equal(np.frombuffer(rec["MIDS"], "<i4"), after), what + "MIDS is not the map after the call"
        # the connections the call read, against what the previous call left in the frames both share
        row = {int(p): k for k, p in enumerate(ids)}
        if left is not None:
            shared = 0
            for g, was in left.items():
                if g not in buff:
                    continue
                now = frames[buff.index(g)]["conn"]
                want = np.array([c if c < 0 else row.get(c, -2) for c in was], np.int32)
                assert np.array_equal(now, want), what + "the connections of frame %d are not those the previous fusion left" % g
                shared += 1
            assert shared >= 2
        # ... and what this call leaves: ids, -1 free, -2 a point that left the map
        left = {}
        for f, g in enumerate(buff):
            c = frames[f]["conn"]
            left[g] = [int(ids[rep[x]]) if x >= 0 else int(x) for x in c]
        for f, j, p in added.tolist():
            assert left[buff[f]][j] == -1
            left[buff[f]][j] = int(ids[p])
        replaced = set(ids[rep != np.arange(n)].tolist())
        assert not any(x in replaced for c in left.values() for x in c)
        observed = {}
        for c in left.values():
            for x in c:
                if x >= 0:
                    observed[x] = observed.get(x, 0) + 1
        if others:      # the refinement and the refresh of the same keyframe read the fused observations
            want = np.array([min(observed.get(int(p), 0), 64) for p in after], np.int32)
            for tag in ("FOBS", "ROBS"):
                got = np.diff(np.frombuffer(rec[tag], "<i4"))
                assert np.array_equal(got, want), what + "%s does not carry the fused observation counts" % tag
        n_keyframes += 1
        totals += counts
        print(what + "%d map points, %d frames, %d keypoints: candidates %d, merges %d (refused %d), observations added %d (refused %d), "
              "points replaced %d -> %d map points" % (n, len(frames), first[-1], *counts.tolist(), len(after)))
    assert n_keyframes >= 2 and on["stdout"].count("map points fused into others") == n_keyframes
    assert totals[1] >= 1 and totals[3] >= 1, "no merge or no added observation over the run: %r" % totals
    err_t, err_r, travelled = RF.trajectory_error(on)
    print("others %d: %d keyframes, totals %s; max translation error %.3f of %.3f travelled, max rotation error %.2f deg"
          % (others, n_keyframes, totals.tolist(), err_t.max(), travelled, err_r.max()))
    # the sanity bounds of test_gpu_run_vo.py: 30 % of the distance travelled, 3 degrees
    assert err_t.max() < 0.3 * travelled and err_r.max() < 3.0, (on["stdout"], err_t, err_r)


def check_off(mvo, tmp_path, env):
    absent = run(mvo, tmp_path, None, False, env)
    zero = run(mvo, tmp_path, 0, False, env)
    assert zero["raw"] == absent["raw"], "the log with map_point_fuse: 0 differs from the log without the key"
    assert not any(t in rec for rec in zero["log"] for t in TAGS)
    assert "map points fused" not in zero["stdout"] + absent["stdout"]
    assert np.array_equal(zero["traj"], absent["traj"])


def check_fuse(mvo, tmp_path, env, others):
    check_on(run(mvo, tmp_path, 1, others, env), others)
