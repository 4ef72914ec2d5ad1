"""Body shared by tests/test_gpu_run_vo_pose_optimize.py (MI355X) and tests/test_run_vo_pose_optimize_sim.py (emulated build):
run_vo on the 24 rendered frames of tests/run_vo_projection_body.py with `tracking_match_by_projection: 1` and
`tracking_pose_by_optimization: 1`, with the second key 0 and without it.  From the frame log alone, for every tracked frame whose
optimisation was called: the numpy transcription (tests/pose_optimize_numpy.py) reproduces OTWC, OTCW, OINF, OCHI and OOUT from
OSET, OINI, OP3D, OP2D and OSIG byte for byte; OINI is the logged prediction (PRED), OP2D the pixels of the matched keypoints
(MPRJ into KPTS), OSIG their (float)(1 / (scale scale)); where OFBK is 0 the frame's inlier matches (MMAP) are the non-flagged
matches of MPRJ in order and, for a frame that tracks, its POSE (logged after the bundle adjustment that starts from OTWC) lies
within one frame's motion of OTWC.  Every frame that tracks with projection alone tracks
with the key on, at most a quarter of the tracked frames fall back to solvePnPRansac, and the trajectory stays inside the sanity
bounds of test_gpu_run_vo.py.  With the key 0 the log and the trajectory equal those without the key byte for byte; the key on
without tracking by projection makes run_vo fail with a message that says so."""
import subprocess

import numpy as np

import pose_optimize_numpy as R
import projection_numpy as P
import run_vo_projection_body as PB
import vo_chain
from test_gpu_run_vo import EXE, _read_traj, _write_dataset

TAGS = ("OSET", "OINI", "OP3D", "OP2D", "OSIG", "OTWC", "OTCW", "OINF", "OCHI", "OOUT")
N, K1 = PB.N, PB.K1
PROJECTION = ("tracking_match_by_projection: 1\nprojection_match_max_pixel_dist: %r\nprojection_match_lowe_ratio: %r\n"
              "projection_match_max_hamming: %d\n" % (PB.MAX_PX, PB.LOWE_RATIO, PB.MAX_HAMMING))


_CACHE = {}


def run(mvo, tmp_path, key, env, projection=True, expect_failure=False):
    """key: None (absent), 0 or 1.  A run is made once per session and library and then shared, read-only."""
    which = (key, projection, env.get("LD_LIBRARY_PATH", ""))
    if which in _CACHE:
        return _CACHE[which]
    tmp_path.mkdir(exist_ok=True)
    log_path = tmp_path / "frames.log"
    extra = "save_frame_log_to: %s\nscale_factor: %r\n" % (log_path, PB.SCALE_FACTOR) + (PROJECTION if projection else "")
    if key is not None:
        extra += "tracking_pose_by_optimization: %d\n" % key
    scene, frames, truth, cfg = _write_dataset(mvo, tmp_path, N, K1, extra)
    r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=900, env=env)
    if expect_failure:
        return r
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("robust optimisation over all matches" in r.stdout) == bool(key)
    _CACHE[which] = dict(scene=scene, truth=truth, stdout=r.stdout, raw=open(log_path, "rb").read(), log=vo_chain.read_frame_log(log_path),
                         traj=_read_traj(tmp_path / "cam_traj.txt"))
    return _CACHE[which]


def check_on(on, off):
    log = on["log"]
    assert len(log) == N == len(off["log"]) and len(on["traj"]) == N
    n_tracked = n_called = n_fallback = 0
    for i, (rec, rec0) in enumerate(zip(log, off["log"])):
        what = "frame %d: " % i
        assert not any(t in rec0 for t in TAGS + ("OFBK",)), what + "the key is off, the log has its records"
        if "MORD" not in rec:
            assert not any(t in rec for t in TAGS + ("OFBK",))
            continue
        n_tracked += 1
        good, good0 = (int(np.frombuffer(x["FLAG"], "<i4")[0]) for x in (rec, rec0))
        assert good or not good0, what + "tracks with projection alone and not with the key on"
        assert "OFBK" in rec, what + "a tracked frame without OFBK"
        fallback = int(np.frombuffer(rec["OFBK"], "<i4")[0])
        n_fallback += fallback
        handed, inl = (np.frombuffer(rec[t], P.DMATCH) for t in ("MPRJ", "MMAP"))
        if "OSET" not in rec:
            assert fallback == 1 and len(handed) < R.DEFAULTS["min_inliers"] and not any(t in rec for t in TAGS)
            continue
        n_called += 1
        for t in TAGS:
            assert t in rec, what + "the optimisation was called, %s is missing" % t
        setup = np.frombuffer(rec["OSET"], "<f8")
        names = ("rounds", "iterations", "min_inliers", "chi2_threshold", "huber_delta", "rel_tolerance")
        assert len(setup) == 10 and setup[4:].tolist() == [R.DEFAULTS[k] for k in names]
        K = dict(zip(("fx", "fy", "cx", "cy"), setup[:4]))
        init = np.frombuffer(rec["OINI"], "<f8").reshape(4, 4)
        p3 = np.frombuffer(rec["OP3D"], "<f4").reshape(-1, 3)
        p2 = np.frombuffer(rec["OP2D"], "<f4").reshape(-1, 2)
        sig = np.frombuffer(rec["OSIG"], "<f4")
        assert rec["OINI"] == rec["PRED"], what + "the initial pose is not the predicted one"
        kp = np.frombuffer(rec["KPTS"], PB.KEYPOINT)
        assert len(p3) == len(p2) == len(sig) == len(handed) >= R.DEFAULTS["min_inliers"]
        assert p2.tobytes() == np.stack([kp["x"], kp["y"]], 1)[handed["trainIdx"]].tobytes(), what + "OP2D is not the matched keypoints"
        scale = PB.octave_scales(kp["octave"])[handed["trainIdx"]].astype(np.float64)
        assert sig.tobytes() == (1.0 / (scale * scale)).astype(np.float32).tobytes(), what + "OSIG is not (float)(1 / (scale scale))"
        Twc, Tcw, outlier, chi2, info, rows = R.optimize_pose(p3, p2, sig, init, K)
        assert rec["OTWC"] == Twc.tobytes(), what + "OTWC differs from the transcription"
        assert rec["OTCW"] == Tcw.tobytes(), what + "OTCW differs from the transcription"
        assert rec["OINF"] == info.tobytes(), what + "OINF differs from the transcription: %r" % (info,)
        assert rec["OCHI"] == chi2.tobytes(), what + "OCHI differs from the transcription"
        assert rec["OOUT"] == outlier.tobytes(), what + "OOUT differs from the transcription"
        assert fallback == (info[0] != R.OPTIMISED)
        if not fallback:
            assert inl.tobytes() == handed[outlier == 0].tobytes(), what + "the inlier matches are not the non-flagged matches"
            if good:
                # POSE is logged after callBundleAdjustment, which starts from OTWC and moves it: the scene has unit scale and
                # the motion per frame is about 0.02, so a pose further than that from OTWC did not come from it
                moved = np.abs(np.frombuffer(rec["POSE"], "<f8") - np.frombuffer(rec["OTWC"], "<f8")).max()
                print(what + "the bundle adjustment moved the optimised pose by %.2e" % moved)
                assert moved < 0.02, what + "POSE does not follow from OTWC"
        print(what + "%d matches, info %s, chi2 %.1f -> %.1f, fell back %d, tracked %d (projection alone: %d)"
              % (len(handed), info.tolist(), chi2[0], chi2[1], fallback, good, good0))
    assert n_tracked == N - K1 - 1 and n_called >= n_tracked - 2
    print("%d tracked frames, %d optimised, %d fell back" % (n_tracked, n_called, n_fallback))
    assert 4 * n_fallback <= n_tracked, "%d of %d tracked frames fell back to solvePnPRansac" % (n_fallback, n_tracked)
    # the sanity bounds of test_gpu_run_vo.py: 30 % of the distance travelled, 3 degrees
    est, gt = on["traj"], np.stack(on["truth"])
    err_t = np.linalg.norm(est[K1:, :3, 3] - gt[K1:, :3, 3], axis=1)
    cosang = (np.einsum("nij,nij->n", est[K1:, :3, :3], gt[K1:, :3, :3]) - 1) / 2
    err_r = np.degrees(np.arccos(np.clip(cosang, -1, 1)))
    travelled = np.linalg.norm(gt[-1, :3, 3] - gt[K1, :3, 3])
    print("max translation error %.3f of %.3f travelled, max rotation error %.2f deg" % (err_t.max(), travelled, err_r.max()))
    assert err_t.max() < 0.3 * travelled and err_r.max() < 3.0, (on["stdout"], err_t, err_r)


def check_off(mvo, tmp_path, env):
    absent = run(mvo, tmp_path / "absent", None, env)
    zero = run(mvo, tmp_path / "zero", 0, env)
    # (the two logs name their own path nowhere: the records hold data only)
    assert zero["raw"] == absent["raw"], "the log with tracking_pose_by_optimization: 0 differs from the log without the key"
    assert np.array_equal(zero["traj"], absent["traj"])


def check_optimised(mvo, tmp_path, env):
    check_on(run(mvo, tmp_path / "on", 1, env), run(mvo, tmp_path / "absent", None, env))


def check_alone(mvo, tmp_path, env):
    r = run(mvo, tmp_path / "alone", 1, env, projection=False, expect_failure=True)
    assert r.returncode != 0 and "tracking_pose_by_optimization requires tracking_match_by_projection: 1" in r.stdout + r.stderr
