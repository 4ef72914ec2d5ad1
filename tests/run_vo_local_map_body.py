"""Body shared by tests/test_gpu_run_vo_local_map.py (MI355X) and tests/test_run_vo_local_map_sim.py (emulated build): run_vo on
the 24 rendered frames of tests/run_vo_projection_body.py with `tracking_match_by_projection: 1`,
`tracking_pose_by_optimization: 1` and `tracking_local_map: 1`, with the third key 0 and without it.  From the frame log alone, for
every tracked frame whose second search was made: LINI is the pose the first optimisation gave (OTWC); LSKP and LLVL are the masks
of the first pass's inlier matches (the non-flagged matches of MPRJ: their map rows, through the points in view of PPOS under
PRED, and their keypoints); LPOS / LDSC are the map of the first search (PPOS / PDSC); the numpy transcription
(tests/local_map_numpy.py) reproduces LMAT from LSET, LINI, LSKP, LLVL, LPOS, LDSC, LNRM, LMXD, KPTS and DESC byte for byte; LP3D /
LP2D / LSIG are the first pass's inlier matches in their order followed by the new matches in trainIdx order; the transcription of
the optimisation (tests/pose_optimize_numpy.py) reproduces LTWC, LINF, LCHI and LOUT; LAPP follows from them; and where the pass
was applied MMAP is the first pass's inlier matches without the flagged ones and POSE lies within one frame's motion of LTWC.
Every frame that tracks without the key tracks with it, the pass is applied on at least three quarters of the tracked frames, and
the trajectory stays inside the sanity bounds of test_gpu_run_vo.py.  With the key 0 the log and the trajectory equal those
without the key byte for byte; the key on without `tracking_pose_by_optimization` makes run_vo fail with a message that says so."""
import subprocess

import numpy as np

import local_map_numpy as LM
import pose_optimize_numpy as R
import projection_numpy as P
import run_vo_pose_optimize_body as OB
import run_vo_projection_body as PB
import vo_chain
from test_gpu_run_vo import EXE, _read_traj, _write_dataset

TAGS = ("LSET", "LINI", "LSKP", "LLVL", "LPOS", "LDSC", "LNRM", "LMXD", "LMAT")
OPT_TAGS = ("LP3D", "LP2D", "LSIG", "LTWC", "LINF", "LCHI", "LOUT")
N, K1 = PB.N, PB.K1
LEVELS = 4          # level_pyramid of the run (the default)
NO_NEW, TOO_MANY, NOT_OPTIMISED, TOO_FAR, APPLIED = range(5)

_CACHE = {}


def run(mvo, tmp_path, key, env, optimisation=True, expect_failure=False):
    """key: None (absent), 0 or 1.  A run is made once per session and library and then shared, read-only."""
    which = (key, optimisation, env.get("LD_LIBRARY_PATH", ""))
    if which in _CACHE:
        return _CACHE[which]
    tmp_path.mkdir(exist_ok=True)
    log_path = tmp_path / "frames.log"
    extra = "save_frame_log_to: %s\nscale_factor: %r\n" % (log_path, PB.SCALE_FACTOR) + OB.PROJECTION
    if optimisation:
        extra += "tracking_pose_by_optimization: 1\n"
    if key is not None:
        extra += "tracking_local_map: %d\n" % key
    scene, frames, truth, cfg = _write_dataset(mvo, tmp_path, N, K1, extra)
    r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=900, env=env)
    if expect_failure:
        return r
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("a second time from the optimised pose" in r.stdout) == bool(key)
    _CACHE[which] = dict(scene=scene, truth=truth, stdout=r.stdout, raw=open(log_path, "rb").read(), log=vo_chain.read_frame_log(log_path),
                         traj=_read_traj(tmp_path / "cam_traj.txt"))
    return _CACHE[which]


def traj_errors(res):
    est, gt = res["traj"], np.stack(res["truth"])
    err_t = np.linalg.norm(est[K1:, :3, 3] - gt[K1:, :3, 3], axis=1)
    cosang = (np.einsum("nij,nij->n", est[K1:, :3, :3], gt[K1:, :3, :3]) - 1) / 2
    err_r = np.degrees(np.arccos(np.clip(cosang, -1, 1)))
    return err_t, err_r, np.linalg.norm(gt[-1, :3, 3] - gt[K1, :3, 3])


def check_on(on, off):
    log = on["log"]
    assert len(log) == N == len(off["log"]) and len(on["traj"]) == N
    n_tracked = n_made = n_applied = 0
    new_per_frame, conn_on, conn_off = [], [], []
    for i, (rec, rec0) in enumerate(zip(log, off["log"])):
        what = "frame %d: " % i
        assert not any(t in rec0 for t in TAGS + OPT_TAGS + ("LAPP",)), what + "the key is off, the log has its records"
        if "MORD" not in rec:
            assert not any(t in rec for t in TAGS + OPT_TAGS + ("LAPP",))
            continue
        n_tracked += 1
        good, good0 = (int(np.frombuffer(x["FLAG"], "<i4")[0]) for x in (rec, rec0))
        assert good or not good0, what + "tracks without the key and not with it"
        fallback = int(np.frombuffer(rec["OFBK"], "<i4")[0])
        if "LAPP" not in rec:
            assert fallback == 1 or not good, what + "the pose came from the optimisation and the second search was not made"
            assert not any(t in rec for t in TAGS + OPT_TAGS)
            continue
        assert fallback == 0 and good, what + "the second search was made on a frame it is not for"
        n_made += 1
        for t in TAGS:
            assert t in rec, what + "the pass was made, %s is missing" % t
        setup = np.frombuffer(rec["LSET"], "<f8")
        ls = LM.level_scales(PB.SCALE_FACTOR, LEVELS)
        names = ("min_view_cos", "radius_near", "radius_far", "near_cos", "radius_scale", "lowe_ratio", "max_hamming")
        assert setup[6] == LEVELS and setup[7:14].tolist() == [LM.DEFAULTS[k] for k in names] and setup[14:].tobytes() == ls.tobytes()
        K = dict(zip(("fx", "fy", "cx", "cy"), setup[:4]))
        assert setup[:4].tobytes() == np.frombuffer(rec["OSET"], "<f8")[:4].tobytes()
        cols, rows = int(setup[4]), int(setup[5])
        assert rec["LINI"] == rec["OTWC"], what + "the pose going in is not the optimised one"
        T = np.frombuffer(rec["LINI"], "<f8").reshape(4, 4)
        kp = np.frombuffer(rec["KPTS"], PB.KEYPOINT)
        txy = np.stack([kp["x"], kp["y"]], 1)
        desc = np.frombuffer(rec["DESC"], np.uint8).reshape(-1, 32)
        assert rec["LPOS"] == rec["PPOS"] and rec["LDSC"] == rec["PDSC"], what + "the map is not the map of the first search"
        pos = np.frombuffer(rec["LPOS"], "<f4").reshape(-1, 3)
        mdesc = np.frombuffer(rec["LDSC"], np.uint8).reshape(-1, 32)
        normal = np.frombuffer(rec["LNRM"], "<f4").reshape(-1, 3)
        max_dist = np.frombuffer(rec["LMXD"], "<f4")
        assert len(pos) == len(mdesc) == len(normal) == len(max_dist) == len(np.frombuffer(rec["MORD"], "<i4"))
        assert (max_dist > 0).all(), what + "a map point without max_dist_"
        # the masks: the first pass's inlier matches = the non-flagged matches of MPRJ, whose queryIdx counts the points in view
        handed = np.frombuffer(rec["MPRJ"], P.DMATCH)
        first = handed[np.frombuffer(rec["OOUT"], np.uint8) == 0]
        pred = np.frombuffer(rec["PRED"], "<f8").reshape(4, 4)
        in_view = np.nonzero(P.project_map(pos, pred, K, cols, rows)[2])[0]
        first_rows = in_view[first["queryIdx"]]
        skip = np.zeros(len(pos), np.uint8)
        skip[first_rows] = 1
        t_level = kp["octave"].astype(np.int32)
        t_level[first["trainIdx"]] = -2
        assert rec["LSKP"] == skip.tobytes(), what + "LSKP is not the points of the first pass's inlier matches"
        assert rec["LLVL"] == t_level.tobytes(), what + "LLVL is not the octaves with the connected keypoints marked"
        # the search
        want = LM.match_features(pos, mdesc, normal, max_dist, T, K, cols, rows, desc, txy, t_level, ls, skip)
        assert rec["LMAT"] == want.tobytes(), what + "LMAT differs from the transcription"
        applied, outcome = np.frombuffer(rec["LAPP"], "<i4").tolist()
        new_per_frame.append(len(want))
        inl = np.frombuffer(rec["MMAP"], P.DMATCH)
        if len(want) == 0 or len(first) + len(want) > 4096:
            assert (applied, outcome) == (0, NO_NEW if len(want) == 0 else TOO_MANY) and not any(t in rec for t in OPT_TAGS)
            assert inl.tobytes() == first.tobytes()
            continue
        for t in OPT_TAGS:
            assert t in rec, what + "the second optimisation was called, %s is missing" % t
        rows_ = np.concatenate([first_rows, want["queryIdx"]])
        kps = np.concatenate([first["trainIdx"], want["trainIdx"]])
        scale = PB.octave_scales(kp["octave"])[kps].astype(np.float64)
        sig = (1.0 / (scale * scale)).astype(np.float32)
        assert rec["LP3D"] == pos[rows_].tobytes() and rec["LP2D"] == txy[kps].tobytes(), what + "the pairs or their order"
        assert rec["LSIG"] == sig.tobytes(), what + "LSIG is not (float)(1 / (scale scale))"
        Twc, _, outlier, chi2, info, _ = R.optimize_pose(pos[rows_], txy[kps], sig, T, K)
        assert rec["LTWC"] == Twc.tobytes(), what + "LTWC differs from the transcription"
        assert rec["LINF"] == info.tobytes() and rec["LCHI"] == chi2.tobytes() and rec["LOUT"] == outlier.tobytes(), what
        # (PRVP holds the previous frame's pose as this frame found it: max_possible_dist_to_prev_keyframe is 0.3)
        near = np.linalg.norm(Twc[:3, 3] - np.frombuffer(rec["PRVP"], "<f8").reshape(2, 4, 4)[1][:3, 3]) < 0.3
        want_outcome = NOT_OPTIMISED if info[0] != R.OPTIMISED else (APPLIED if near else TOO_FAR)
        assert (applied, outcome) == (int(want_outcome == APPLIED), want_outcome), what + "LAPP %r" % ((applied, outcome),)
        nf = len(first)
        if applied:
            n_applied += 1
            assert inl.tobytes() == first[outlier[:nf] == 0].tobytes(), what + "MMAP is not the first pass without the flagged matches"
            moved = np.abs(np.frombuffer(rec["POSE"], "<f8") - np.frombuffer(rec["LTWC"], "<f8")).max()
            assert moved < 0.02, what + "POSE does not follow from LTWC"
            conn_on.append(int((outlier == 0).sum()))
        else:
            assert inl.tobytes() == first.tobytes()
            conn_on.append(nf)
        conn_off.append(nf)
        print(what + "%d first-pass inliers, %d new matches, info %s, chi2 %.1f -> %.1f, %d flagged, outcome %d"
              % (nf, len(want), info.tolist(), chi2[0], chi2[1], int(outlier.sum()), outcome))
    assert n_tracked == N - K1 - 1
    print("%d tracked frames, second search made on %d, applied on %d; new matches per frame %s; connections per frame %.1f -> %.1f"
          % (n_tracked, n_made, n_applied, new_per_frame, np.mean(conn_off), np.mean(conn_on)))
    assert 4 * n_applied >= 3 * n_tracked, "the pass was applied on %d of %d tracked frames" % (n_applied, n_tracked)
    for name, res in (("with the key", on), ("without", off)):
        err_t, err_r, travelled = traj_errors(res)
        print("%s: max translation error %.4f of %.3f travelled, max rotation error %.3f deg" % (name, err_t.max(), travelled, err_r.max()))
    err_t, err_r, travelled = traj_errors(on)
    assert err_t.max() < 0.3 * travelled and err_r.max() < 3.0, (on["stdout"], err_t, err_r)


def check_off(mvo, tmp_path, env):
    absent = run(mvo, tmp_path / "absent", None, env)
    zero = run(mvo, tmp_path / "zero", 0, env)
    assert zero["raw"] == absent["raw"], "the log with tracking_local_map: 0 differs from the log without the key"
    assert np.array_equal(zero["traj"], absent["traj"])


def check_tracked(mvo, tmp_path, env):
    check_on(run(mvo, tmp_path / "on", 1, env), run(mvo, tmp_path / "absent", None, env))


def check_alone(mvo, tmp_path, env):
    r = run(mvo, tmp_path / "alone", 1, env, optimisation=False, expect_failure=True)
    assert r.returncode != 0 and "tracking_local_map requires tracking_pose_by_optimization: 1" in r.stdout + r.stderr
