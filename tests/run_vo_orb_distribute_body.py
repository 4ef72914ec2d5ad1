"""Body shared by tests/test_gpu_run_vo_orb_distribute.py (MI355X) and tests/test_run_vo_orb_distribute_sim.py (emulated
build): run_vo on the 24 rendered frames of tests/test_gpu_run_vo.py with `orb_distribute_keypoints: 1` and, for comparison,
without it.  From the frame log alone, for every frame: the numpy transcription (tests/orb_distribute_numpy.py) of the frame's
image gives the logged candidate and key-point counts per level (ODCN) and, after cv::ORB::compute's border filter
(tests/orb_numpy.py), the logged key points and descriptors (KPTS, DESC) byte for byte.  Every frame that tracks with the key
off tracks with it on; the run with the key off is the seeded run it was (tests/golden/run_vo_seeded_24_traj.txt)."""
import os
import subprocess

import numpy as np

import orb_distribute_numpy as D
import orb_numpy as N
import vo_chain
from conftest import GOLDEN
from test_gpu_run_vo import EXE, _read_traj, _write_dataset

N_FRAMES, K1 = 24, 5
# host/include/my_slam/basics/config.h = config/config.yaml:65-69,94-95; max_number_of_keypoints from the test's config.yaml
ORB = dict(nfeatures=8000, scale_factor=1.2, nlevels=4, fast_threshold=20, max_keypoints=1500, grid_size=16, grid_max_per_cell=8)
PARAMS = dict(ini_threshold=20, min_threshold=7, cell_size=30, edge_threshold=19)
NEW_TAGS = ("ORBD", "ODCN")


def run(mvo, tmp_path, on, env):
    tmp_path.mkdir(exist_ok=True)
    log_path = tmp_path / "frames.log"
    extra = "save_frame_log_to: %s\n" % log_path
    if on:
        extra += "orb_distribute_keypoints: 1\n"
    scene, frames, truth, cfg = _write_dataset(mvo, tmp_path, N_FRAMES, K1, extra)
    r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("cell-wise FAST (20 / 7, cells of 30 px, edge 19)" in r.stdout) == on
    return dict(frames=frames, truth=truth, stdout=r.stdout, log=vo_chain.read_frame_log(log_path),
                traj=_read_traj(tmp_path / "cam_traj.txt"))


def check(on, off):
    log, log0 = on["log"], off["log"]
    assert len(log) == N_FRAMES == len(log0)
    # the key off: none of the new records, and the run recorded before the key existed
    assert not any(t in rec for rec in log0 for t in NEW_TAGS)
    assert "map seeded from frames 0 and 5: 692 map points" in off["stdout"], off["stdout"]
    assert "frames 24, tracked 18, lost 0, keyframes 7, map points 1219 ->" in off["stdout"], off["stdout"]
    before = _read_traj(os.path.join(GOLDEN, "run_vo_seeded_24_traj.txt"))
    assert np.abs(off["traj"] - before).max() < 1e-4
    # the key on
    assert np.frombuffer(log[0]["ORBD"], "<i4").tolist() == [PARAMS[k] for k in ("ini_threshold", "min_threshold", "cell_size",
                                                                                "edge_threshold")]
    assert not any("ORBD" in rec for rec in log[1:])
    det, orb = D.OrbDistribute(**ORB, **PARAMS), N.Orb(**ORB)
    n_tracked = n_tracked0 = 0
    for i, (rec, rec0, img) in enumerate(zip(log, log0, on["frames"])):
        what = "frame %d: " % i
        pyr = det.pyramid(img)
        cand = det.candidates(img, pyr)
        detected = det.detect(img, pyr, cand)
        kept, desc = orb.compute(img, detected)
        counts = np.frombuffer(rec["ODCN"], "<i4")
        assert counts[0] == 4 and len(counts) == 9, what + "ODCN layout"
        assert counts[1:5].tolist() == np.bincount(cand[:, 2], minlength=4).tolist(), what + "candidates per level"
        assert counts[5:9].tolist() == np.bincount(detected["octave"], minlength=4).tolist(), what + "key points per level"
        assert rec["KPTS"] == kept.tobytes(), what + "KPTS (%d) differs from the transcription (%d)" % (len(rec["KPTS"]) // 28, len(kept))
        assert rec["DESC"] == desc.tobytes(), what + "DESC differs from the transcription"
        assert len(kept) > 500
        if "FLAG" in rec0:
            good, good0 = (int(np.frombuffer(x["FLAG"], "<i4")[0]) for x in (rec, rec0))
            n_tracked += good
            n_tracked0 += good0
            print(what + "%d candidates, %d key points detected, %d described (key off: %d); tracked %d (key off: %d)"
                  % (len(cand), len(detected), len(kept), len(rec0["KPTS"]) // 28, good, good0))
            assert good or not good0, what + "tracks with the key off and not with it on"
    assert n_tracked0 == N_FRAMES - K1 - 1 and n_tracked >= n_tracked0
    # the sanity bounds of test_gpu_run_vo.py: 30 % of the distance travelled, 3 degrees
    est, gt = on["traj"], np.stack(on["truth"])
    err_t = np.linalg.norm(est[K1:, :3, 3] - gt[K1:, :3, 3], axis=1)
    cosang = (np.einsum("nij,nij->n", est[K1:, :3, :3], gt[K1:, :3, :3]) - 1) / 2
    err_r = np.degrees(np.arccos(np.clip(cosang, -1, 1)))
    travelled = np.linalg.norm(gt[-1, :3, 3] - gt[K1, :3, 3])
    print("max translation error %.3f of %.3f travelled, max rotation error %.2f deg" % (err_t.max(), travelled, err_r.max()))
    assert err_t.max() < 0.3 * travelled and err_r.max() < 3.0, (on["stdout"], err_t, err_r)
