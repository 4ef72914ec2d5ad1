"""TEST AID shared by tests/test_oracle_chain_init.py (CPU), tests/test_run_vo_init_sim.py (CPU, emulated build of the kernels)
and tests/test_gpu_run_vo_init.py (MI355X): the sequence, its config.yaml and the comparison of a run of host/driver/run_vo
under `init_from_images: 1` with the oracle chain from images (tests/vo_chain_init.py).

The sequence is the one tests/test_gpu_run_vo.py uses: 24 PNG-sized frames of synth.Scene3D(amp=0.6, tilt=0.3), stride 1, at most
1500 keypoints.  The initialisation thresholds are the reference's (config/config.yaml:105-113: 1.0 / 20 / 15 / 50 / 2.0 / 0.8),
NONE changed: the camera moves 2 cm per frame in front of a ~2 m deep scene, about 5.5 px of mean displacement per frame, so the
50 px of min_pixel_dist are reached at frame 9 (oracle chain: 50.7 px there, 45.8 px at frame 8) -- inside the n - 12 = 12 the
tracking part of the test needs.  Frames and the chain without a map order are computed once per session and shared."""
import functools
import os
import re
import subprocess

import numpy as np

import vo_chain
import vo_chain_init
from conftest import GOLDEN, ROOT, assert_struct_equal
from finish_restate import DEFAULTS as INIT_DEFAULTS

EXE = os.path.join(ROOT, "monocular-visual-odometry_amd", "host", "driver", "run_vo")
N_FRAMES = 24
MAX_KEYPOINTS = 1500
INIT_PARAMS = dict(INIT_DEFAULTS)                      # the reference's values, as they are
INIT_YAML = """min_triang_angle: %(min_triang_angle)r
max_ratio_between_max_angle_and_median_angle: %(max_ratio_to_median)r
assumed_mean_pts_depth_during_vo_init: %(assumed_mean_depth)r
min_inlier_matches: %(min_inlier_matches)d
min_pixel_dist: %(min_pixel_dist)r
min_median_triangulation_angle: %(min_median_triangulation_angle)r
feature_match_method_index_initialization: 1
max_matching_pixel_dist_in_initialization: 100
"""
INIT_DTYPE = np.dtype([("slot", "<i4"), ("n_slot_inliers", "<i4"), ("n_kept", "<i4"), ("scaled", "<i4"), ("criteria", "<i4", 3),
                       ("good", "<i4"), ("mean_depth", "<f8"), ("scale", "<f8"), ("median_angle", "<f8"), ("mean_pixel_dist", "<f8")])


@functools.lru_cache(maxsize=None)
def sequence():
    """(scene, frames, ground-truth poses)"""
    import __graft_entry__ as graft
    scene = graft.load_package().synth.Scene3D(amp=0.6, tilt=0.3)
    frames = [scene.frame(i) for i in range(N_FRAMES)]
    for f in frames:
        f.setflags(write=False)
    return scene, frames, np.stack([scene.pose(i) for i in range(N_FRAMES)])


_CHAIN = {}


def chain_alone(O):
    """The oracle chain from images with ascending ids as the map's order (no run involved), computed once."""
    if "c" not in _CHAIN:
        scene, frames, _ = sequence()
        _CHAIN["c"] = vo_chain_init.run_oracle_chain_from_images(O, frames, scene.K, O.default_params(max_keypoints=MAX_KEYPOINTS),
                                                                INIT_PARAMS, fix_map_points=True, map_order=None)
    return _CHAIN["c"]


def read_traj(path):
    rows = np.loadtxt(path).reshape(-1, 12)
    T = np.tile(np.eye(4), (len(rows), 1, 1))
    T[:, :3, 3] = rows[:, :3]
    T[:, :3, :3] = rows[:, 3:].reshape(-1, 3, 3).transpose(0, 2, 1)
    return T


def write_traj(path, poses):
    with open(path, "w") as f:
        for T in poses:
            f.write(" ".join("%.17g" % v for v in np.concatenate([T[:3, 3], T[:3, :3].T.ravel()])) + "\n")


def write_images(tmp_path):
    from PIL import Image
    data = tmp_path / "dataset"
    data.mkdir()
    for i, img in enumerate(sequence()[1]):
        Image.fromarray(img[:, :, ::-1]).save(data / ("rgb_%05d.png" % i))   # PIL wants RGB; the files hold what imread returns as BGR
    return data


def write_config(tmp_path, data, name, dataset_extra="", extra=""):
    """A config.yaml of the reference's layout whose dataset section has NO true_traj_filename unless dataset_extra adds it."""
    K = sequence()[0].K
    cfg = tmp_path / (name + ".yaml")
    cfg.write_text("""%%YAML:1.0
dataset_name: "synthetic"
synthetic:
  dataset_dir: %s
  num_images: %d
  camera_info.fx: %r
  camera_info.fy: %r
  camera_info.cx: %r
  camera_info.cy: %r
%smax_num_imgs_to_proc: 300
save_predicted_traj_to: %s
max_number_of_keypoints: %d
is_ba_fix_map_points: "true"
%s""" % (data, N_FRAMES, K["fx"], K["fy"], K["cx"], K["cy"], dataset_extra, tmp_path / (name + "_traj.txt"), MAX_KEYPOINTS, extra))
    return cfg, tmp_path / (name + "_traj.txt")


class Run:
    """One run_vo process; several may be in flight at once (each config writes files of its own)."""

    def __init__(self, cfg, traj, log=None, timeout=300):
        self.cfg, self.traj, self.log, self.timeout = cfg, traj, log, timeout
        self.proc = subprocess.Popen([EXE, str(cfg)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        self.stdout = None

    def wait(self):
        if self.stdout is None:
            try:
                self.stdout, err = self.proc.communicate(timeout=self.timeout)
            except subprocess.TimeoutExpired:
                self.proc.kill()
                self.proc.communicate()
                raise
            assert self.proc.returncode == 0, self.stdout + err
        return self


def aligned_errors(est, gt, f):
    """Errors of the poses f.. against the ground truth after the similarity alignment the two trajectories leave free.  Both
    start at the identity (the first keyframe IS the world frame, and synth.Scene3D.pose(0) = I), so rotation and translation of
    the alignment are fixed and only the scale is free -- the one thing initialisation sets arbitrarily (mean depth := 0.8).
    Fitting a rotation as well would fit nothing real: the path is nearly a straight line, which leaves the rotation about it
    undetermined.  Scale = least squares over the positions.  Returns (scale, max |s p - p_gt|, max rotation error in degrees)."""
    X, Y = est[f:, :3, 3], gt[f:, :3, 3]
    s = float((X * Y).sum() / (X * X).sum())
    err_t = np.linalg.norm(s * X - Y, axis=1)
    cosang = (np.einsum("nij,nij->n", est[f:, :3, :3], gt[f:, :3, :3]) - 1) / 2
    return s, float(err_t.max()), float(np.degrees(np.arccos(np.clip(cosang, -1, 1))).max())


def start_runs_from_images(tmp_path, data, timeout=300):
    """Two runs with `init_from_images: 1`, no truth file on disk, the same inputs, files of their own."""
    runs = []
    for name in ("init", "init_again"):
        log_path = tmp_path / (name + ".log")
        cfg, traj = write_config(tmp_path, data, name, extra="init_from_images: 1\nsave_frame_log_to: %s\n%s"
                                 % (log_path, INIT_YAML % INIT_PARAMS))
        assert not any("truth" in p.name for p in tmp_path.iterdir()) and "true_traj_filename" not in cfg.read_text()
        runs.append(Run(cfg, traj, log_path, timeout))
    return runs


def run_equals_the_chain(O, runs):
    """run_vo with `init_from_images: 1` and no truth file, against run_oracle_chain_from_images.  Returns the measured figures."""
    scene, frames, gt = sequence()
    r = runs[0].wait()
    traj = r.traj
    log = vo_chain.read_frame_log(r.log)
    assert len(log) == N_FRAMES
    est = read_traj(traj)
    assert len(est) == N_FRAMES                      # every frame gets a trajectory row

    def map_order(idx, ids):                         # the host container's iteration order (see vo_chain.py)
        order = np.frombuffer(log[idx]["MORD"], "<i4")
        assert set(order.tolist()) == ids, "frame %d: the map of the run and of the oracle chain hold different points" % idx
        return order

    ch, hist = vo_chain_init.run_oracle_chain_from_images(O, frames, scene.K, O.default_params(max_keypoints=MAX_KEYPOINTS),
                                                          INIT_PARAMS, fix_map_points=True, map_order=map_order)
    f = ch.init_frame
    assert f is not None
    printed = re.findall(r"initialised at frame (\d+)", r.stdout)
    assert printed == [str(f)], r.stdout
    assert "never initialised" not in r.stdout
    n_key = n_tracked = n_rejected = 0
    worst_pose = worst_pt = 0.0
    init_rec = None
    for i, (rec, fr) in enumerate(zip(log, ch.frames)):
        what = "frame %d: " % i
        assert np.frombuffer(rec["FRAM"], "<i4")[0] == i
        assert_struct_equal(np.frombuffer(rec["KPTS"], O.KEYPOINT_DTYPE), fr.kps, what + "keypoints")
        assert rec["DESC"] == fr.desc.tobytes(), what + "descriptors"
        T_run = np.frombuffer(rec["POSE"], "<f8").reshape(4, 4)
        assert ("INIT" in rec) == (fr.rec["state"] == "DOING_INITIALIZATION"), what + "state"
        assert ("FLAG" in rec) == (fr.rec["state"] == "DOING_TRACKING"), what + "state"
        if i == 0:
            assert not ({"MREF", "INIT", "FLAG", "MIDS"} & set(rec)) and np.array_equal(T_run, np.eye(4)), what + "the first keyframe"
        elif i <= f:                                 # an initialisation frame: everything bit for bit
            res = fr.rec["init"]
            assert_struct_equal(np.frombuffer(rec["MREF"], O.DMATCH_DTYPE), fr.rec["matches_with_ref"], what + "matches with the first keyframe")
            got = np.frombuffer(rec["INIT"], INIT_DTYPE)[0]
            want = (res["slot"], res["n_slot_inliers"], res["n_kept"], int(res["scaled"]), [int(c) for c in res["criteria"]], int(res["good"]))
            have = (int(got["slot"]), int(got["n_slot_inliers"]), int(got["n_kept"]), int(got["scaled"]), got["criteria"].tolist(), int(got["good"]))
            assert have == want, what + "INIT %r, the chain has %r" % (have, want)
            assert_struct_equal(np.frombuffer(rec["IREF"], O.DMATCH_DTYPE), fr.rec["inliers_matches_with_ref"], what + "the slot's inliers")
            assert_struct_equal(np.frombuffer(rec["I3DM"], O.DMATCH_DTYPE), fr.rec["inliers_matches_for_3d"], what + "kept matches")
            assert rec["I3DP"] == np.ascontiguousarray(fr.rec["inliers_pts3d"], "<f4").tobytes(), what + "kept points"
            assert rec["POSE"] == np.ascontiguousarray(hist[i], "<f8").tobytes(), what + "pose"
            for key in ("mean_depth", "scale", "median_angle"):
                assert got[key] == res[key], what + key
            assert np.array_equal(got["mean_pixel_dist"], res["mean_pixel_dist"], equal_nan=True), what + "mean_pixel_dist"
            if i < f:
                n_rejected += 1
                assert "MIDS" not in rec and np.array_equal(T_run, np.eye(4)), what + "a rejected frame keeps the first keyframe's pose"
            else:
                init_rec = got
                ids = np.frombuffer(rec["MIDS"], "<i4")
                pos = np.frombuffer(rec["MPOS"], "<f4").reshape(-1, 3)
                assert set(ids.tolist()) == set(fr.rec["map_after"]) and len(ids) == res["n_kept"], what + "the map after initialisation"
                ref_pos = np.stack([fr.rec["map_after"][int(m)] for m in ids])
                assert np.array_equal(pos, ref_pos), what + "map positions"
        else:                                        # tracking: what test_run_vo_equals_the_oracle_chain compares, its tolerances
            good, is_key = np.frombuffer(rec["FLAG"], "<i4")
            assert (bool(good), bool(is_key)) == (fr.rec["good"], fr.rec["is_keyframe"]), what + "tracking / keyframe decision"
            assert_struct_equal(np.frombuffer(rec["MMAP"], O.DMATCH_DTYPE), fr.rec["matches_with_map"], what + "PnP inlier matches")
            n_tracked += int(good)
            if "MREF" in rec:
                n_key += 1
                assert_struct_equal(np.frombuffer(rec["MREF"], O.DMATCH_DTYPE), fr.rec["matches_with_ref"], what + "matches_with_ref_")
                assert_struct_equal(np.frombuffer(rec["IREF"], O.DMATCH_DTYPE), fr.rec["inliers_matches_with_ref"], what + "epipolar inliers")
                assert_struct_equal(np.frombuffer(rec["I3DM"], O.DMATCH_DTYPE), fr.rec["inliers_matches_for_3d"], what + "triangulation survivors")
                p_run = np.frombuffer(rec["I3DP"], "<f4").reshape(-1, 3)
                p_orc = fr.rec["inliers_pts3d"]
                worst_pt = max(worst_pt, float((np.abs(p_run - p_orc) / np.abs(p_orc).max(axis=1, keepdims=True)).max()))
                ids = np.frombuffer(rec["MIDS"], "<i4")
                pos = np.frombuffer(rec["MPOS"], "<f4").reshape(-1, 3)
                assert set(ids.tolist()) == set(fr.rec["map_after"]), what + "map after insertion and culling"
                ref_pos = np.stack([fr.rec["map_after"][int(m)] for m in ids])
                worst_pt = max(worst_pt, float((np.abs(pos - ref_pos) / np.abs(ref_pos).max(axis=1, keepdims=True)).max()))
            else:
                assert "map_after" not in fr.rec, what + "the oracle chain inserted a keyframe, the run did not"
            worst_pose = max(worst_pose, float(np.abs(T_run - hist[i]).max()))
    # the conditions tests/test_oracle_chain_init.py establishes on the chain alone hold on the run
    assert n_rejected >= 2 and f <= N_FRAMES - 12 and int(init_rec["slot"]) == 0, (n_rejected, f, init_rec)
    assert n_tracked == N_FRAMES - f - 1 and n_key >= 2, (n_tracked, n_key)
    assert worst_pose < 1e-4 and worst_pt < 1e-5, (worst_pose, worst_pt)
    assert np.abs(est - hist).max() < 1e-4           # the trajectory FILE carries the same poses
    scale, err_t, err_r = aligned_errors(est, gt, f)
    travelled = float(np.linalg.norm(gt[-1, :3, 3] - gt[f, :3, 3]))
    print("run from images: initialised at frame %d (slot %d, n_kept %d) after %d rejected frames; %d tracked, %d keyframes; against "
          "the chain max |dT| %.3g, max rel point error %.3g; against ground truth (scale %.4f) %.4f m = %.1f %% of %.3f m, %.2f deg"
          % (f, init_rec["slot"], init_rec["n_kept"], n_rejected, n_tracked, n_key, worst_pose, worst_pt, scale, err_t,
             100 * err_t / travelled, travelled, err_r))
    assert err_t < 0.3 * travelled and err_r < 3.0, (err_t, travelled, err_r)
    # determinism: a second run writes the identical trajectory file
    assert runs[1].wait().traj.read_text() == traj.read_text()
    return dict(f=f, slot=int(init_rec["slot"]), n_kept=int(init_rec["n_kept"]), rejected=n_rejected, worst_pose=worst_pose,
                worst_pt=worst_pt, err_t=err_t, travelled=travelled, err_r=err_r)


def start_run_out_of_reach(tmp_path, data, timeout=300):
    prm = dict(INIT_PARAMS, min_pixel_dist=1e6)
    cfg, traj = write_config(tmp_path, data, "never", extra="init_from_images: 1\n" + INIT_YAML % prm)
    return Run(cfg, traj, None, timeout)


def never_initialises(run):
    """Thresholds out of reach: exit 0, N identity rows, the last line says that it never initialised."""
    r = run.wait()
    est = read_traj(r.traj)
    assert est.shape == (N_FRAMES, 4, 4) and np.array_equal(est, np.tile(np.eye(4), (N_FRAMES, 1, 1)))
    assert "never initialised" in r.stdout.strip().splitlines()[-1], r.stdout
    assert "initialised at frame" not in r.stdout


SEED_K1 = 5


def start_seeded_runs(tmp_path, data, with_key_zero=True, timeout=300):
    """The ground-truth-seeded start: the key absent and, unless with_key_zero is False, `init_from_images: 0`."""
    write_traj(tmp_path / "cam_traj_truth.txt", sequence()[2])
    ds = "  true_traj_filename: %s\n" % (tmp_path / "cam_traj_truth.txt")
    runs = []
    for name, extra in (("seeded", ""), ("seeded0", "init_from_images: 0\n"))[:2 if with_key_zero else 1]:
        log_path = tmp_path / (name + ".log")
        cfg, traj = write_config(tmp_path, data, name, dataset_extra=ds, extra="init_keyframe_0: 0\ninit_keyframe_1: %d\n"
                                 "save_frame_log_to: %s\n%s" % (SEED_K1, log_path, extra))
        runs.append(Run(cfg, traj, log_path, timeout))
    return runs


def seeded_run_is_unchanged(O, runs):
    """Without the key the program is the ground-truth-seeded run it was: the key absent and `init_from_images: 0` (where both ran)
    print the same and write the same trajectory file and the same frame log byte for byte, the log holds none of the new records, the lines printed and the trajectory are
    those recorded before the key existed, and the poses are those of the seeded oracle chain (tests/vo_chain.py, the yardstick of tests/test_gpu_run_vo.py) within its 1e-4."""
    scene, frames, gt = sequence()
    k1 = SEED_K1
    out = [(r.wait().stdout.replace(str(r.traj), "TRAJ"), r.traj.read_text(), r.log.read_bytes()) for r in runs]
    assert all(o == out[0] for o in out)
    assert "map seeded from frames 0 and %d" % k1 in out[0][0] and "initialised" not in out[0][0]
    # what the program printed and wrote for this sequence before the key existed (recorded from that binary on the emulated
    # build, tests/golden/run_vo_seeded_24_traj.txt; the text holds six significant digits)
    assert "map seeded from frames 0 and 5: 692 map points" in out[0][0], out[0][0]
    assert "frames 24, tracked 18, lost 0, keyframes 7, map points 1219 -> TRAJ" in out[0][0], out[0][0]
    before = read_traj(os.path.join(GOLDEN, "run_vo_seeded_24_traj.txt"))
    assert np.abs(read_traj(runs[0].traj) - before).max() < 1e-4
    log = vo_chain.read_frame_log(runs[0].log)
    assert len(log) == N_FRAMES and not any("INIT" in rec for rec in log)

    def map_order(idx, ids):
        order = np.frombuffer(log[idx]["MORD"], "<i4")
        assert set(order.tolist()) == ids
        return order

    _, hist = vo_chain.run_oracle_chain(O, frames, scene.K, gt, 0, k1, O.default_params(max_keypoints=MAX_KEYPOINTS),
                                        fix_map_points=True, map_order=map_order)
    assert np.abs(read_traj(runs[0].traj) - hist).max() < 1e-4
