"""Wall time of mvo_find_homography (host clock around the synchronous call, warmed up, >= 50 repeats) at 500 / 1000 / 2000
matches with 0 / 50 % wrong matches, beside the sequential CPU restatement of the same call (tests/homography_restatement.cpp).
--essential: the same for mvo_esti_motion_by_essential (thick scene) beside mvo_find_essential_inliers on the same matches
(the difference is what recoverPose adds), and mvo_check_init_scores on both models, beside the restatement
(tests/init_motion_restatement.cpp; its RANSAC stage is the CPU oracle's).
--poses: mvo_estimate_possible_relative_poses (planar scene) beside the sum of the separate mvo_esti_motion_by_essential +
mvo_find_homography + mvo_check_init_scores calls on the same matches, and beside the sequential restatement
(tests/pose_restate.py; its E RANSAC stage is the CPU oracle's).
--finish: mvo_init_two_view (thick scene, the E slot is chosen) beside mvo_estimate_possible_relative_poses on the same matches
in the same run: the difference is what the finish adds (k_init_finish, its read-back and the host tail).
Per-kernel device times: run it under rocprofv3 --kernel-trace --stats.
Usage: python tools/init_probe.py [--essential | --poses | --finish] [--reps 50] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import h_restate as HR  # noqa: E402
import init_restate as IR  # noqa: E402
import pose_restate as PR  # noqa: E402


def timed(fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts) * 1e3), float(np.min(ts) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--essential", action="store_true")
    ap.add_argument("--poses", action="store_true")
    ap.add_argument("--finish", action="store_true")
    a = ap.parse_args()
    mvo = graft.load_package()
    ctx = mvo.Context(0)
    R = HR.Restatement()
    rows = []
    if a.essential:
        O = graft.load_oracle()
        O.build()
        IRR = IR.Restatement()
        for n in (500, 1000, 2000):
            for frac in (0.0, 0.5):
                pr = HR.two_view(n, 200 + n, planar=False, noise=0.5, outlier_frac=frac)
                s, d, K = pr["src"], pr["dst"], IR.kdict(pr["K"])
                g = ctx.esti_motion_by_essential(s, d, K)
                h = ctx.find_homography(s, d)
                H = IR.scale_by_22(h["H"])
                em_med, _ = timed(lambda: ctx.find_essential_inliers(s, d, K), a.reps)
                rp_med, rp_min = timed(lambda: ctx.esti_motion_by_essential(s, d, K), a.reps)
                sc_med, sc_min = timed(lambda: ctx.check_init_scores(s, d, K, g["E"], g["inliers"], H, h["inliers"]), a.reps)
                cpu_rp, _ = timed(lambda: IRR.esti_motion_by_essential(O, s, d, pr["K"]), max(5, a.reps // 10))
                cpu_sc, _ = timed(lambda: IRR.check_init_scores(s, d, pr["K"], g["E"], g["inliers"], H, h["inliers"]),
                                  max(5, a.reps // 10))
                rows.append(dict(n=n, outliers=frac, n_inl_e=len(g["inliers"]), n_inl_h=len(h["inliers"]),
                                 find_essential_ms_median=em_med, esti_motion_ms_median=rp_med, esti_motion_ms_min=rp_min,
                                 scores_ms_median=sc_med, scores_ms_min=sc_min, cpu_esti_motion_ms_median=cpu_rp,
                                 cpu_scores_ms_median=cpu_sc))
                print(json.dumps(rows[-1]), flush=True)
    if a.poses:
        O = graft.load_oracle()
        O.build()
        PRR = PR.Restatement()
        for n in (500, 1000, 2000):
            for frac in (0.0, 0.5):
                pr = HR.two_view(n, 300 + n, planar=True, noise=0.5, outlier_frac=frac)
                s, d, K = pr["src"], pr["dst"], IR.kdict(pr["K"])
                g = ctx.estimate_possible_relative_poses(s, d, K)

                def separate():
                    e = ctx.esti_motion_by_essential(s, d, K)
                    h = ctx.find_homography(s, d)
                    ctx.check_init_scores(s, d, K, e["E"], e["inliers"], IR.scale_by_22(h["H"]), h["inliers"])

                po_med, po_min = timed(lambda: ctx.estimate_possible_relative_poses(s, d, K), a.reps)
                sep_med, sep_min = timed(separate, a.reps)
                cpu_med, _ = timed(lambda: PRR.estimate_possible_relative_poses(O, s, d, pr["K"]), max(5, a.reps // 10))
                rows.append(dict(n=n, outliers=frac, n_inl_e=len(g["inliers_e"]), n_inl_h=len(g["inliers_h"]),
                                 n_slots=len(g["solutions"]), best=g["best"], ratio=g["ratio"], poses_ms_median=po_med,
                                 poses_ms_min=po_min, separate_ms_median=sep_med, separate_ms_min=sep_min,
                                 cpu_restatement_ms_median=cpu_med))
                print(json.dumps(rows[-1]), flush=True)
    if a.finish:
        for n in (500, 1000, 2000):
            for frac in (0.0, 0.5):
                pr = HR.two_view(n, 400 + n, planar=False, noise=0.5, outlier_frac=frac)
                s, d, K = pr["src"], pr["dst"], IR.kdict(pr["K"])
                g = ctx.init_two_view(s, d, K)
                po_med, po_min = timed(lambda: ctx.estimate_possible_relative_poses(s, d, K), a.reps)
                in_med, in_min = timed(lambda: ctx.init_two_view(s, d, K), a.reps)
                rows.append(dict(n=n, outliers=frac, slot=g["slot"], n_slot_inliers=g["n_slot_inliers"], n_kept=g["n_kept"],
                                 good=g["good"], poses_ms_median=po_med, poses_ms_min=po_min, init_two_view_ms_median=in_med,
                                 init_two_view_ms_min=in_min, finish_adds_ms_median=in_med - po_med))
                print(json.dumps(rows[-1]), flush=True)
    for n in (() if a.essential or a.poses or a.finish else (500, 1000, 2000)):
        for frac in (0.0, 0.5):
            pr = HR.two_view(n, 100 + n, planar=True, noise=0.5, outlier_frac=frac)
            s, d = pr["src"], pr["dst"]
            ctx.find_homography(s, d)
            dbg = ctx.debug_homography()
            gpu_med, gpu_min = timed(lambda: ctx.find_homography(s, d), a.reps)
            cpu_med, cpu_min = timed(lambda: R.find_homography(s, d), max(5, a.reps // 10))
            rows.append(dict(n=n, outliers=frac, iters_run=dbg["iters_run"], evaluated=dbg["evaluated"],
                             lm_iters=dbg["lm_iters"], gpu_ms_median=gpu_med, gpu_ms_min=gpu_min,
                             cpu_restatement_ms_median=cpu_med))
            print(json.dumps(rows[-1]), flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
