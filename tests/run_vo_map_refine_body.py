"""Body shared by tests/test_gpu_run_vo_map_refine.py (MI355X) and tests/test_run_vo_map_refine_sim.py (emulated build): run_vo on
the 24 rendered frames of tests/test_gpu_run_vo.py with `map_point_refine_positions: 1`, with it and `map_point_refresh: 1`
together, with the key 0 and without the key.  From the frame log alone, for every keyframe inserted while tracking: the numpy
transcription (tests/map_refine_numpy.py) reproduces the positions after the call (FAFT), chi2 (FCHI), status / steps / trials
(FINF) and the outlier flags (FOUT) from the set-up (FSET), the window's poses (FTWC), the observation arrays (FOBS, FFRM, FPIX)
and the positions before (FBEF) byte for byte, some point there has three observations or more, and the map logged after the
insertion (MPOS) carries the refined positions.  The log of the run with the key 0 has none of the records and equals the log of
the run without the key byte for byte.  Every frame that tracks with the key off tracks with it on, and the trajectory stays
inside the sanity bounds of test_gpu_run_vo.py."""
import subprocess

import numpy as np

import map_refine_numpy as R
import run_vo_map_refresh_body as RB
import vo_chain
from test_gpu_run_vo import EXE, _read_traj

TAGS = ("FSET", "FTWC", "FOBS", "FFRM", "FPIX", "FBEF", "FAFT", "FCHI", "FINF", "FOUT")
N, K1 = RB.N, RB.K1

_CACHE = {}


def run(mvo, tmp_path, key, refresh, env):
    """key: None (absent), 0 or 1.  A run is made once per session and library and then shared, read-only; the frames on disk
    are those of the map-point refresh's body."""
    tmp_path.mkdir(exist_ok=True)
    which = (key, refresh, env.get("LD_LIBRARY_PATH", ""))
    if which in _CACHE:
        return _CACHE[which]
    if key is None and not refresh:
        _CACHE[which] = RB.run(mvo, tmp_path, None, False, env)     # the same run: no key of either kind
        return _CACHE[which]
    truth, base, base_traj = RB.dataset(mvo, tmp_path)
    out = tmp_path / ("refine_%s_%d" % (key, refresh))
    out.mkdir()
    log_path, traj_path = out / "frames.log", out / "cam_traj.txt"
    assert base.count(base_traj) == 1
    text = base.replace(base_traj, str(traj_path)) + "save_frame_log_to: %s\nscale_factor: 1.2\n" % log_path
    if key is not None:
        text += "map_point_refine_positions: %d\n" % key
    if refresh:
        text += "map_point_refresh: 1\n"
    cfg = out / "config.yaml"
    cfg.write_text(text)
    r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    _CACHE[which] = dict(truth=truth, stdout=r.stdout, raw=open(log_path, "rb").read(), log=vo_chain.read_frame_log(log_path),
                         traj=_read_traj(traj_path))
    return _CACHE[which]


def trajectory_error(res):
    est, gt = res["traj"], np.stack(res["truth"])
    err_t = np.linalg.norm(est[K1:, :3, 3] - gt[K1:, :3, 3], axis=1)
    cosang = (np.einsum("nij,nij->n", est[K1:, :3, :3], gt[K1:, :3, :3]) - 1) / 2
    err_r = np.degrees(np.arccos(np.clip(cosang, -1, 1)))
    return err_t, err_r, np.linalg.norm(gt[-1, :3, 3] - gt[K1, :3, 3])


def check_on(on, off, refresh):
    log = on["log"]
    assert len(log) == N == len(off["log"]) and len(on["traj"]) == N
    n_keyframes = n_refined = 0
    for i, (rec, rec0) in enumerate(zip(log, off["log"])):
        what = "frame %d: " % i
        tracked = "MORD" in rec
        flags = np.frombuffer(rec["FLAG"], "<i4") if tracked else np.zeros(2, "<i4")
        if tracked:
            good0 = int(np.frombuffer(rec0["FLAG"], "<i4")[0])
            assert flags[0] or not good0, what + "tracks with the key off and not with it on"
        if not (tracked and flags[1]):
            assert not any(t in rec for t in TAGS), what + "not a keyframe inserted while tracking, yet it has refinement records"
            continue
        for t in TAGS:
            assert t in rec, what + "a keyframe without its %s record" % t
        setup = np.frombuffer(rec["FSET"], "<f8")
        assert len(setup) == 8 and setup[4:].tolist() == [R.DEFAULTS[k] for k in ("max_trials", "min_observations", "huber_delta", "rel_tolerance")]
        K = dict(zip(("fx", "fy", "cx", "cy"), setup[:4]))
        T = np.frombuffer(rec["FTWC"], "<f8").reshape(-1, 4, 4)
        start = np.frombuffer(rec["FOBS"], "<i4")
        frame = np.frombuffer(rec["FFRM"], "<i4")
        uv = np.frombuffer(rec["FPIX"], "<f4").reshape(-1, 2)
        before = np.frombuffer(rec["FBEF"], "<f4").reshape(-1, 3)
        n = len(start) - 1
        ids = np.frombuffer(rec["MIDS"], "<i4")
        assert len(ids) == n == len(before) and len(frame) == len(uv) == start[-1] and n > 100 and 2 <= len(T) <= 20
        assert np.array_equal(T[-1], np.frombuffer(rec["POSE"], "<f8").reshape(4, 4)), what + "the newest pose of the window is not the frame's"
        m_i = np.diff(start)
        assert (m_i >= 3).any(), what + "no point with three observations: the check would be vacuous"
        pos, chi2, info, outlier = R.refine(before, T, K, frame, uv, start)
        assert rec["FAFT"] == pos.tobytes(), what + "FAFT differs from the transcription"
        assert rec["FCHI"] == chi2.tobytes(), what + "FCHI differs from the transcription"
        assert rec["FINF"] == info.tobytes(), what + "FINF differs from the transcription"
        assert rec["FOUT"] == outlier.tobytes(), what + "FOUT differs from the transcription"
        assert rec["MPOS"] == rec["FAFT"], what + "the map after the insertion does not carry the refined positions"
        if refresh:
            assert rec["RPOS"] == rec["FAFT"], what + "the refresh did not see the refined positions"
        n_keyframes += 1
        n_refined += int((info[:, 0] == 0).sum())
        print(what + "%d map points, %d observations in %d frames, %d points with m >= 3 (max %d); status counts %s, %d flagged"
              % (n, start[-1], len(T), (m_i >= 3).sum(), m_i.max(), np.bincount(info[:, 0], minlength=4).tolist(), outlier.sum()))
    assert n_keyframes >= 2 and on["stdout"].count("map point positions refined") == n_keyframes and n_refined > 0
    err_t, err_r, travelled = trajectory_error(on)
    e0_t, e0_r, _ = trajectory_error(off)
    print("refresh %d: %d keyframes refined; max translation error %.3f of %.3f travelled, max rotation error %.2f deg (key off: %.3f, %.2f deg)"
          % (refresh, n_keyframes, err_t.max(), travelled, err_r.max(), e0_t.max(), e0_r.max()))
    # the sanity bounds of test_gpu_run_vo.py: 30 % of the distance travelled, 3 degrees
    assert err_t.max() < 0.3 * travelled and err_r.max() < 3.0, (on["stdout"], err_t, err_r)


def check_off(mvo, tmp_path, env):
    absent = run(mvo, tmp_path, None, False, env)
    zero = run(mvo, tmp_path, 0, False, env)
    assert zero["raw"] == absent["raw"], "the log with map_point_refine_positions: 0 differs from the log without the key"
    assert not any(t in rec for rec in zero["log"] for t in TAGS)
    assert "map point positions" not in zero["stdout"] + absent["stdout"]
    assert np.array_equal(zero["traj"], absent["traj"])


def check_refine(mvo, tmp_path, env, refresh):
    off = RB.run(mvo, tmp_path, 1, False, env) if refresh else run(mvo, tmp_path, None, False, env)
    check_on(run(mvo, tmp_path, 1, refresh, env), off, refresh)
