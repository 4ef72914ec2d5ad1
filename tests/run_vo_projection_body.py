"""Body shared by tests/test_gpu_run_vo_projection.py (MI355X) and tests/test_run_vo_projection_sim.py (emulated build): run_vo
on the 24 rendered frames of tests/test_gpu_run_vo.py with `tracking_match_by_projection: 1` and, for comparison, without it.
From the frame log alone, for every tracked frame: predict_pose of the two logged poses (PRVP) is the logged prediction (PRED)
exactly; the numpy transcription (tests/projection_numpy.py) reproduces the matches handed to PnP (MPRJ) byte for byte from the
map as the matcher saw it (PPOS, PDSC), PRED and the frame's KPTS / DESC; the PnP inliers (MMAP) are among them.  Every frame
that tracks with the key off tracks with it on, and the trajectory stays inside the sanity bounds of test_gpu_run_vo.py."""
import subprocess

import numpy as np

import projection_numpy as P
import vo_chain
from test_gpu_run_vo import EXE, _read_traj, _write_dataset

KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])
MAX_PX, LOWE_RATIO, MAX_HAMMING, SCALE_FACTOR = 8.0, 0.8, 64, 1.2
N, K1 = 24, 5


def octave_scales(octave):
    """(float)(scale_factor multiplied by itself `octave` times, starting from 1.0), as the mirror header computes it"""
    table, s = [], 1.0
    for _ in range(int(octave.max()) + 1 if len(octave) else 1):
        table.append(np.float32(s))
        s = s * SCALE_FACTOR
    return np.array(table, np.float32)[octave]


def run(mvo, tmp_path, on, env):
    tmp_path.mkdir(exist_ok=True)
    log_path = tmp_path / "frames.log"
    extra = "save_frame_log_to: %s\nscale_factor: %r\n" % (log_path, SCALE_FACTOR)
    if on:
        extra += ("tracking_match_by_projection: 1\nprojection_match_max_pixel_dist: %r\nprojection_match_lowe_ratio: %r\n"
                  "projection_match_max_hamming: %d\n" % (MAX_PX, LOWE_RATIO, MAX_HAMMING))
    scene, frames, truth, cfg = _write_dataset(mvo, tmp_path, N, K1, extra)
    r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("tracked by projection" in r.stdout) == on
    return dict(scene=scene, frames=frames, truth=truth, stdout=r.stdout, log=vo_chain.read_frame_log(log_path),
                traj=_read_traj(tmp_path / "cam_traj.txt"))


def check(mvo, on, off):
    scene, log = on["scene"], on["log"]
    rows, cols = on["frames"][0].shape[:2]
    assert len(log) == N == len(off["log"]) and len(on["traj"]) == N
    n_tracked, n_with_prev2 = 0, 0
    for i, (rec, rec0) in enumerate(zip(log, off["log"])):
        what = "frame %d: " % i
        assert not any(t in rec0 for t in ("PRVP", "PRED", "PPOS", "PDSC", "MPRJ")), what + "the key is off, the log has its records"
        if "MORD" not in rec:
            assert "PRED" not in rec
            continue
        n_tracked += 1
        for tag in ("PRVP", "PRED", "PPOS", "PDSC", "MPRJ"):
            assert tag in rec, what + "a tracked frame without its %s record" % tag
        prvp = np.frombuffer(rec["PRVP"], "<f8").reshape(2, 4, 4)
        pred = np.frombuffer(rec["PRED"], "<f8").reshape(4, 4)
        no_prev2 = prvp[0].tobytes() == prvp[1].tobytes()
        n_with_prev2 += not no_prev2
        assert mvo.predict_pose(None if no_prev2 else prvp[0], prvp[1]).tobytes() == pred.tobytes(), what + "PRED is not predict_pose(PRVP)"
        pos = np.frombuffer(rec["PPOS"], "<f4").reshape(-1, 3)
        desc = np.frombuffer(rec["PDSC"], np.uint8).reshape(-1, 32)
        assert len(pos) == len(desc) == len(rec["MORD"]) // 4 and len(pos) > 100
        kp = np.frombuffer(rec["KPTS"], KEYPOINT)
        d = np.frombuffer(rec["DESC"], np.uint8).reshape(-1, 32)
        kxy = np.stack([kp["x"], kp["y"]], 1)
        want = P.match_features(pos, desc, pred, scene.K, cols, rows, d, kxy, MAX_PX, LOWE_RATIO, MAX_HAMMING, octave_scales(kp["octave"]))
        in_view = P.project_map(pos, pred, scene.K, cols, rows)[2]
        want["queryIdx"] = (np.cumsum(in_view) - 1)[want["queryIdx"]]      # renumbered to the candidate list, as PnP gets them
        assert len(want) > 50, what + "too few matches to mean anything"
        assert rec["MPRJ"] == want.tobytes(), what + "MPRJ (%d) differs from the transcription (%d)" % (len(rec["MPRJ"]) // 16, len(want))
        handed, inl = (np.frombuffer(rec[t], P.DMATCH) for t in ("MPRJ", "MMAP"))
        good, good0 = (int(np.frombuffer(x["FLAG"], "<i4")[0]) for x in (rec, rec0))
        if good:
            assert set(zip(inl["queryIdx"].tolist(), inl["trainIdx"].tolist())) <= set(zip(handed["queryIdx"].tolist(), handed["trainIdx"].tolist()))
        print(what + "map %d, in view %d, handed to PnP %d, PnP inliers %d (key off: %d), tracked %d (key off: %d)"
              % (len(pos), in_view.sum(), len(handed), len(inl), len(rec0["MMAP"]) // 16, good, good0))
        assert good or not good0, what + "tracks with the key off and not with it on"
    assert n_tracked == N - K1 - 1 and n_with_prev2 >= n_tracked - 2
    # the sanity bounds of test_gpu_run_vo.py: 30 % of the distance travelled, 3 degrees
    est, gt = on["traj"], np.stack(on["truth"])
    err_t = np.linalg.norm(est[K1:, :3, 3] - gt[K1:, :3, 3], axis=1)
    cosang = (np.einsum("nij,nij->n", est[K1:, :3, :3], gt[K1:, :3, :3]) - 1) / 2
    err_r = np.degrees(np.arccos(np.clip(cosang, -1, 1)))
    travelled = np.linalg.norm(gt[-1, :3, 3] - gt[K1, :3, 3])
    print("max translation error %.3f of %.3f travelled, max rotation error %.2f deg" % (err_t.max(), travelled, err_r.max()))
    assert err_t.max() < 0.3 * travelled and err_r.max() < 3.0, (on["stdout"], err_t, err_r)
