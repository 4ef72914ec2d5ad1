"""Body shared by tests/test_gpu_run_vo_map_refresh.py (MI355X) and tests/test_run_vo_map_refresh_sim.py (emulated build): run_vo
on the 24 rendered frames of tests/test_gpu_run_vo.py with `map_point_refresh: 1`, with it and `tracking_match_by_projection: 1`
together, with the key 0 and without the key.  From the frame log alone, for every keyframe inserted while tracking: the numpy
transcription (tests/map_refresh_numpy.py) reproduces the chosen observations (RCHO) and the normals (RNRM) from the observation
arrays (ROBS, RDSC, RCAM) and the resident positions (RPOS) byte for byte, and some point there has three observations or more.
With projection on, the map the next tracked frame's matcher saw (PDSC) carries the chosen descriptors.  The log of the run with
the key 0 has none of the records and equals the log of the run without the key byte for byte.  Every frame that tracks with the
key off tracks with it on, and the trajectory stays inside the sanity bounds of test_gpu_run_vo.py."""
import subprocess

import numpy as np

import map_refresh_numpy as R
import vo_chain
from test_gpu_run_vo import EXE, _read_traj, _write_dataset

TAGS = ("ROBS", "RDSC", "RCAM", "RPOS", "RCHO", "RNRM")
N, K1 = 24, 5


_CACHE = {}


def dataset(mvo, tmp_path):
    """The 24 frames, written once per session; every run gets a config of its own beside them."""
    if "dataset" not in _CACHE:
        (tmp_path / "frames").mkdir()
        scene, frames, truth, cfg = _write_dataset(mvo, tmp_path / "frames", N, K1)
        _CACHE["dataset"] = (truth, cfg.read_text(), str(tmp_path / "frames" / "cam_traj.txt"))
    return _CACHE["dataset"]


def run(mvo, tmp_path, key, projection, env):
    """key: None (absent), 0 or 1.  A run is made once per session and library and then shared, read-only."""
    tmp_path.mkdir(exist_ok=True)
    which = (key, projection, env.get("LD_LIBRARY_PATH", ""))
    if which in _CACHE:
        return _CACHE[which]
    truth, base, base_traj = dataset(mvo, tmp_path)
    out = tmp_path / ("run_%s_%d" % (key, projection))
    out.mkdir()
    log_path, traj_path = out / "frames.log", out / "cam_traj.txt"
    assert base.count(base_traj) == 1
    text = base.replace(base_traj, str(traj_path)) + "save_frame_log_to: %s\nscale_factor: 1.2\n" % log_path
    if key is not None:
        text += "map_point_refresh: %d\n" % key
    if projection:
        text += "tracking_match_by_projection: 1\n"
    cfg = out / "config.yaml"
    cfg.write_text(text)
    r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    _CACHE[which] = dict(truth=truth, stdout=r.stdout, raw=open(log_path, "rb").read(), log=vo_chain.read_frame_log(log_path),
                         traj=_read_traj(traj_path))
    return _CACHE[which]


def check_on(on, off, projection):
    log = on["log"]
    assert len(log) == N == len(off["log"]) and len(on["traj"]) == N
    n_refreshed, n_other, n_ties, carried = 0, 0, 0, None
    for i, (rec, rec0) in enumerate(zip(log, off["log"])):
        what = "frame %d: " % i
        tracked = "MORD" in rec
        flags = np.frombuffer(rec["FLAG"], "<i4") if tracked else np.zeros(2, "<i4")
        if tracked:
            good0 = int(np.frombuffer(rec0["FLAG"], "<i4")[0])
            assert flags[0] or not good0, what + "tracks with the key off and not with it on"
        if projection and tracked and carried is not None:
            # the first tracked frame after a refresh: its matcher saw the chosen descriptors (the map changes at keyframes only)
            ids, chosen = carried
            mord = np.frombuffer(rec["MORD"], "<i4")
            pdsc = np.frombuffer(rec["PDSC"], np.uint8).reshape(-1, 32)
            row = {int(p): k for k, p in enumerate(mord)}
            still = [p for p in chosen if p in row]
            assert len(still) > 50, what + "too few refreshed points still in the map to mean anything"
            for p in still:
                assert pdsc[row[p]].tobytes() == chosen[p], what + "PDSC of map point %d is not its chosen observation" % p
            carried = None
        if not (tracked and flags[1]):
            assert not any(t in rec for t in TAGS), what + "not a keyframe inserted while tracking, yet it has refresh records"
            continue
        for t in TAGS:
            assert t in rec, what + "a keyframe without its %s record" % t
        start = np.frombuffer(rec["ROBS"], "<i4")
        n = len(start) - 1
        obs_desc = np.frombuffer(rec["RDSC"], np.uint8).reshape(-1, 32)
        obs_cam = np.frombuffer(rec["RCAM"], "<f8").reshape(-1, 3)
        pos = np.frombuffer(rec["RPOS"], "<f4").reshape(-1, 3)
        ids = np.frombuffer(rec["MIDS"], "<i4")
        assert len(ids) == n == len(pos) and len(obs_desc) == len(obs_cam) == start[-1] and n > 100
        assert rec["RPOS"] == rec["MPOS"], what + "RPOS is not the map after the insertion"
        m_i = np.diff(start)
        assert (m_i >= 3).any(), what + "no point with three observations: the check would be vacuous"
        choice, desc, norm = R.refresh(pos, np.zeros((n, 32), np.uint8), obs_desc, obs_cam, start)
        assert rec["RCHO"] == choice.tobytes(), what + "RCHO differs from the transcription"
        got_norm = np.frombuffer(rec["RNRM"], "<f8").reshape(-1, 3)
        assert R.same_f64(got_norm, norm), what + "RNRM differs from the transcription"
        assert np.isnan(norm).any() or rec["RNRM"] == norm.tobytes()
        n_refreshed += 1
        n_other += int((choice > 0).sum())
        n_ties += sum(R.tie_decided(obs_desc, start, k) for k in range(n) if m_i[k] >= 3)
        carried = (ids, {int(ids[k]): desc[k].tobytes() for k in range(n) if choice[k] >= 0})
        print(what + "%d map points, %d observations, %d points with m >= 3 (max %d), %d took another descriptor than their first"
              % (n, start[-1], (m_i >= 3).sum(), m_i.max(), (choice > 0).sum()))
    assert n_refreshed >= 2 and on["stdout"].count("map points refreshed") == n_refreshed
    assert n_other > 0, "no map point ever took another observation's descriptor"
    # the sanity bounds of test_gpu_run_vo.py: 30 % of the distance travelled, 3 degrees
    est, gt = on["traj"], np.stack(on["truth"])
    err_t = np.linalg.norm(est[K1:, :3, 3] - gt[K1:, :3, 3], axis=1)
    cosang = (np.einsum("nij,nij->n", est[K1:, :3, :3], gt[K1:, :3, :3]) - 1) / 2
    err_r = np.degrees(np.arccos(np.clip(cosang, -1, 1)))
    travelled = np.linalg.norm(gt[-1, :3, 3] - gt[K1, :3, 3])
    print("projection %d: %d refreshes, %d ties among the points with m >= 3; max translation error %.3f of %.3f travelled, max rotation "
          "error %.2f deg" % (projection, n_refreshed, n_ties, err_t.max(), travelled, err_r.max()))
    assert err_t.max() < 0.3 * travelled and err_r.max() < 3.0, (on["stdout"], err_t, err_r)


def check_off(mvo, tmp_path, env):
    absent = run(mvo, tmp_path, None, False, env)
    zero = run(mvo, tmp_path, 0, False, env)
    assert zero["raw"] == absent["raw"], "the log with map_point_refresh: 0 differs from the log without the key"
    assert not any(t in rec for rec in zero["log"] for t in TAGS)
    assert "map points refreshed" not in zero["stdout"] + absent["stdout"]
    assert np.array_equal(zero["traj"], absent["traj"])


def check_refresh(mvo, tmp_path, env, projection):
    check_on(run(mvo, tmp_path, 1, projection, env), run(mvo, tmp_path, None, projection, env), projection)
