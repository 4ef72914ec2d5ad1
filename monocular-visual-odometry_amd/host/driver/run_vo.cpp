// host/driver/run_vo.cpp -- headless run_vo: the reference's main loop (run_vo.cpp:58-154) without the displays, over the
// reference's own inputs and outputs: config.yaml (dataset section, camera intrinsics, max_num_imgs_to_proc,
// save_predicted_traj_to), `<dataset_dir>/rgb_%05d.png`, and the 12-number-per-line trajectory file
// (src/vo/vo_io.cpp:13-117).  Every frame goes through the hot path on the MI355X: Frame::calcKeyPoints /
// calcDescriptors, map points in view, matchFeatures, solvePnPRansac, the sliding-window bundle adjustment, and on
// keyframes the epipolar inlier filter + triangulation + culling (my_slam/vo/tracking_loop.h = the DOING_TRACKING branch of
// VisualOdometry::addFrame, vo_addFrame.cpp:70-124).
//
// Two ways to start, chosen by the key `init_from_images` (0 / 1, default 0):
//   1  from the images alone, like the reference: my_slam::vo::VisualOdometry (my_slam/vo/vo.h) takes every frame;
//      the first one is the first keyframe at the identity, the following ones go through the monocular initialisation
//      (matchFeatures with the first keyframe, mvo_init_two_view, isVoGoodToInit_) until one passes and fills the map,
//      the rest is tracked.  The loop is run_vo.cpp:110-148: createFrame -> addFrame -> pose history -> clearNoUsed().
//      Frames the initialisation rejects carry the first keyframe's pose, the identity.  `true_traj_filename` and
//      `init_keyframe_0/1` are neither needed nor read.  The program says `initialised at frame N`, or in its last line
//      that it never initialised (the trajectory is written and the exit status is 0 either way, as in the reference).
//   0  the map is seeded from two frames whose poses are taken from the dataset's ground-truth trajectory
//      (`true_traj_filename`, config.yaml:24; keys `init_keyframe_0/1` pick the frames, default 0 and 5): their matches
//      are filtered and triangulated exactly as a keyframe insertion does it (vo_addFrame.cpp:96-118), which also fixes
//      the scale.  From then on nothing of the ground truth is used.
// Optional keys `camera_info.k1`, `.k2`, `.p1`, `.p2`, `.k3` in the dataset section (cv2.calibrateCamera's vector; a missing
// one is 0): with at least one of them every image is undistorted on the device right after basics::imread
// (my_slam/basics/undistort.h = cv2.undistort(img, K, dist) of python_tools/undistort_all_images.py:11-37), so the frame holds
// what an undistorted file on disk would have held.  Without them the images are taken as undistorted (config.yaml:17,39).
// Optional key `triangulation_match_by_epipolar_line` (0 / 1, default 0): 1 makes every keyframe insertion while tracking (and
// the seeding of the map under `init_from_images: 0`) match the new keyframe with its reference keyframe along the epipolar
// lines of their two estimated poses (my_slam/geometry/epipolar_match.h; the reference's README.md:212,272) instead of over all
// pairs (vo_addFrame.cpp:99).  The initialisation has no pose yet and keeps matchFeatures.  Its three parameters, optional as
// well: `epipolar_match_max_line_dist` (px at pyramid level 0, default 2.0), `epipolar_match_lowe_ratio` (default 0.8),
// `epipolar_match_max_hamming` (default 64).  With the key on, a keyframe's part of the frame log carries two more records
// after MREF: EPIF = int32 id_ of the reference keyframe, int32 0, the 9 f64 of F (x_curr^T F x_ref = 0), row-major; and
// EPIR = the 16 f64 of the reference keyframe's T_w_c_ as F was computed from it (its POSE record dates from its own frame;
// the window bundle adjustment of the frames since has moved it).  F = mvo_fundamental_from_poses(EPIR, this frame's POSE).
// Optional key `tracking_match_by_projection` (0 / 1, default 0): 1 makes every tracked frame start from a constant-velocity
// prediction of its pose (from the last two frames) instead of the last keyframe's, project the resident map with it and match
// each point in view within a radius of its projection (my_slam/vo/projection_match.h; the reference's README.md:212) instead
// of getMappointsInCurrentView_ + matchFeatures (vo.cpp:267-289).  Its three parameters, optional as well:
// `projection_match_max_pixel_dist` (px at pyramid level 0, default 8.0), `projection_match_lowe_ratio` (default 0.8),
// `projection_match_max_hamming` (default 64).  With the key on, a tracked frame's part of the frame log carries five more
// records after MORD: PRVP = the 32 f64 of T_prev2 and T_prev as used (T_prev twice without a prev2), PRED = the 16 f64 of
// the predicted pose, PPOS / PDSC = the map's positions (n x 3 f32) and descriptors (n x 32) as uploaded, in MORD order,
// MPRJ = the matches handed to PnP before the inlier selection (queryIdx -> index among the points in view).
// Optional key `tracking_pose_by_optimization` (0 / 1, default 0; requires `tracking_match_by_projection: 1`, run_vo ends with an
// error that says so otherwise): 1 makes every tracked frame with at least min_inliers matches take its pose from a robust
// motion-only optimisation from the predicted pose over all the matches (my_slam/vo/pose_optimization.h; ORB-SLAM's
// Optimizer::PoseOptimization) instead of solvePnPRansac (vo.cpp:326-329): its non-outliers stand in for the
// PnP inliers, its pose for invT(convertRt2T(R, t)); a frame whose optimisation ends with a status other than 0 falls back to
// solvePnPRansac exactly as without the key.  Optional keys `pose_optimization_rounds` (default 4), `pose_optimization_iterations`
// (10), `pose_optimization_min_inliers` (10), `pose_optimization_chi2_threshold` (5.991).  With the key on, a tracked frame's part
// of the frame log carries after MPRJ, if the optimisation was called: OSET = fx, fy, cx, cy, rounds, iterations, min_inliers,
// chi2_threshold, huber_delta, rel_tolerance (f64), OINI = the initial pose (16 f64), OP3D / OP2D / OSIG = the matches' map
// points (n x 3 f32), pixels (n x 2 f32) and inv_sigma2 (n f32), OTWC / OTCW = the result (16 f64 each), OINF = info (6 int32),
// OCHI = chi2 (2 f64), OOUT = the outlier flags (n); and always OFBK = int32, 1 if the frame fell back.
// Optional key `tracking_local_map` (0 / 1, default 0; requires `tracking_pose_by_optimization: 1`, run_vo ends with an error that
// says so otherwise): 1 makes every tracked frame whose pose came from the optimisation search the map a second time from that
// pose -- the points the first search left unmatched that face the camera within their range of distances, against the free
// keypoints of their predicted pyramid level or the one below within 2.5 to 4 px at that level (my_slam/vo/local_map.h; ORB-SLAM's
// Tracking::TrackLocalMap) -- and optimise the pose again over the union.  Optional keys
// `local_map_min_view_cos` (default 0.5), `local_map_radius_near` (2.5), `local_map_radius_far` (4.0), `local_map_radius_scale`
// (1.0), `local_map_lowe_ratio` (0.8), `local_map_max_hamming` (100).  With the key on, a tracked frame's part of the frame log
// carries after OFBK, if the pass was made: LSET = fx, fy, cx, cy, cols, rows, n_levels, min_view_cos, radius_near, radius_far,
// near_cos, radius_scale, lowe_ratio, max_hamming, then the n_levels level scales (f64), LINI = the pose going in (16 f64), LSKP =
// the skip mask (n), LLVL = the keypoints' levels (nt int32, -2: connected), LPOS / LDSC / LNRM / LMXD = the map as resident:
// positions (n x 3 f32), descriptors (n x 32), normals (n x 3 f32), largest distances (n f32), LMAT = the new matches (queryIdx =
// map row); if the second optimisation was called LP3D / LP2D / LSIG = its points, pixels and inv_sigma2 (f32), LTWC = its pose
// (16 f64), LINF = info (6 int32), LCHI = chi2 (2 f64), LOUT = the outlier flags; and LAPP = int32 applied, int32 outcome (0: no new
// matches, 1: more than 4096 observations, 2: not optimised, 3: moved too far from the previous frame, 4: applied).
// Optional key `orb_distribute_keypoints` (0 / 1, default 0): 1 makes Frame::calcKeyPoints extract the ORB-SLAM way -- FAST cell by
// cell with two thresholds, a quadtree spread per level (my_slam/geometry/orb_distribute.h; the reference's README.md section 5)
// -- instead of cv::ORB::detect (feature_match.cpp:22-23).  Its four parameters, optional as well: `orb_distribute_ini_threshold`
// (default 20), `orb_distribute_min_threshold` (7), `orb_distribute_cell_size` (30), `orb_distribute_edge_threshold` (19).  With
// the key on, the first frame of the log carries ORBD = the four parameters (int32) after FRAM and every frame ODCN after DESC = int32
// nlevels, the candidates per level, the key points per level as detected (KPTS holds those calcDescriptors kept).
// Optional key `map_point_refresh` (0 / 1, default 0): 1 makes every keyframe insertion while tracking end, right after the culling
// (optimizeMap_), with a refresh of the map points from their observations in the last 20 frames (my_slam/vo/map_refresh.h;
// ORB-SLAM's MapPoint::ComputeDistinctiveDescriptors and UpdateNormalAndDepth): the descriptor becomes the observation with the
// least median Hamming distance to the others, the normal the mean unit viewing direction; the reference keeps both from the frame
// that created the point (vo.cpp:528-576).  With the key on, a keyframe's part of the frame log carries six more records after
// MPOS, in the order of MIDS: ROBS = the n + 1 observation starts (int32), RDSC / RCAM = the observations' descriptors (n_obs x
// 32) and camera centres (n_obs x 3 f64), RPOS = the positions as resident (n x 3 f32), RCHO = the chosen observation per point
// (int32, -1: none), RNRM = the normals (n x 3 f64); and MORD of such a frame stays what its own tracking step saw.
// Optional key `map_point_refine_positions` (0 / 1, default 0): 1 makes every keyframe insertion while tracking refine, after the
// culling and before the refresh above, the position of every map point from all its observations in the last 20 frames with the
// poses fixed (my_slam/vo/map_refine.h; a Huber-weighted Levenberg-Marquardt per point); the reference sets
// a position once from two views (vo.cpp:528-576) and its bundle adjustment keeps the points fixed (config.yaml:123).  Optional
// keys `map_point_refine_max_trials` (default 20), `map_point_refine_huber_delta` (default sqrt(5.991)).  With the key on, a
// keyframe's part of the frame log carries ten more records after MPOS, in the order of the map the call read: FSET = fx, fy,
// cx, cy, max_trials, min_observations, huber_delta, rel_tolerance (f64), FTWC = the poses of the window (n_frames x 16 f64),
// FOBS = the n + 1 observation starts (int32), FFRM / FPIX = the observations' frame indices (int32) and pixels (n_obs x 2 f32),
// FBEF / FAFT = the positions before and after (n x 3 f32), FCHI = chi2 before and after (n x 2 f64), FINF = status, accepted
// steps, trials (n x 3 int32), FOUT = the outlier flags (n_obs); and MORD of such a frame stays what its own tracking step saw.
// Optional key `map_point_fuse` (0 / 1, default 0): 1 makes every keyframe insertion while tracking fuse, after the culling and
// before the refinement and the refresh above, the map points that are one physical point, and connect every buffered frame that
// sees a point without having matched it (my_slam/vo/map_fuse.h; ORB-SLAM's ORBmatcher::Fuse and MapPoint::Replace, DESIGN.md
// section 19); the reference creates a new point whenever the matched keypoint of the previous keyframe is none (vo.cpp:528-576).
// Optional keys `map_point_fuse_max_px` (default 3.0), `map_point_fuse_max_hamming` (default 50).  With the key on, a keyframe's part
// of the frame log carries fourteen more records after MPOS: USET = fx, fy, cx, cy, cols, rows, max_px, max_hamming (f64), UMID /
// UPOS / UMDS = the ids, positions (n x 3 f32) and descriptors (n x 32) of the map the call read, UKPN = the keypoints per
// buffered frame (int32), UTWC = their poses (n_frames x 16 f64), UDSC / UPIX / USCL / UCON = frame after frame the descriptors,
// pixels (f32), scales (f32) and connections (int32: map row, -1 free, -2 a point that left the map), UREP = replaced_by (n
// int32), UADD = the added observations (frame, keypoint, point: n_added x 3 int32), UCNT = the six counts, UIDS = the ids of the
// map after the call in its new iteration order; and MORD of such a frame stays what its own tracking step saw.
// Optional key `map_point_create_from_window` (0 / 1, default 0): 1 makes every keyframe insertion while tracking create, right
// after the reference's own new points and before the culling, a map point for every keypoint of the keyframe that has none and
// finds a verified partner along its epipolar line in any other buffered frame (my_slam/vo/window_triangulate.h; ORB-SLAM's
// LocalMapping::CreateNewMapPoints); the reference triangulates against the reference keyframe only
// (vo_addFrame.cpp:104-116).  Optional keys `map_point_create_max_line_px` (default 2.0), `map_point_create_lowe_ratio` (0.8),
// `map_point_create_max_hamming` (64), `map_point_create_max_cos_parallax` (0.9998), `map_point_create_min_baseline` (0.0).  With
// the key on, a keyframe's part of the frame log carries seventeen more records after I3DP: WSET = fx, fy, cx, cy, max_line_px,
// lowe_ratio, max_hamming, max_cos_parallax, max_reproj_chi2, ratio_factor, min_baseline (f64), WKPN = the keypoints per buffered
// frame, the keyframe last (int32), WTWC = their poses (n_frames x 16 f64), WDSC / WPIX / WSCL / WCON = frame after frame the
// descriptors, pixels (f32), scales (f32) and connections (int32: -1 free), WPTS / WPTP / WPTC = the new points (keypoint, frame,
// train, hamming: n x 4 int32; p_curr: n x 3 f32; cos2: f64), WPRS / WPRP / WPRC = every pair after the filter (frame, keypoint,
// train, hamming, status: m x 5 int32; p_curr, p_frame: m x 6 f32; cos2: f64), WCNT = the twelve counts, WIDS / WPOS = the ids and
// world positions (n x 3 f32) of the new map points, WMSZ = the size of the map before and after (2 int32).
// Optional key `save_frame_log_to`: a binary per-frame record of what the rows produced (keypoints, descriptors, the map's
// iteration order, inlier matches, keyframe products, pose) for tests/test_gpu_run_vo.py and tests/run_vo_init_body.py,
// which compose the same run from the oracle and compare stage by stage.  Under `init_from_images` every initialisation
// frame adds MREF, INIT (int32 slot, n_slot_inliers, n_kept, scaled, criteria[3], good; then f64 mean_depth, scale,
// median_angle, mean_pixel_dist), IREF, I3DM, I3DP, and the frame that initialises MIDS / MPOS.
//   run_vo <config.yaml>
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "my_slam/basics/image_io.h"
#include "my_slam/basics/undistort.h"
#include "my_slam/vo/tracking_loop.h"
#include "my_slam/vo/vo.h"
#include "my_slam/vo/vo_io.h"

// Bound weakly: a build of the library without the host side of the initialisation (the emulated libmvo_sim.so of tests/sim)
// still serves the seeded start; asking such a library for `init_from_images` is an error, not a fall-back.
#pragma weak mvo_init_two_view
// ... or without the undistortion: asking such a library for it (`camera_info.k1` ...) is an error as well
#pragma weak mvo_undistort_configure
#pragma weak mvo_undistort
// ... or without the pose-guided matcher (`triangulation_match_by_epipolar_line`): an error, not a fall-back
#pragma weak mvo_fundamental_from_poses
#pragma weak mvo_match_features_epipolar
// ... or without tracking by projection (`tracking_match_by_projection`): likewise
#pragma weak mvo_predict_pose
#pragma weak mvo_map_match_features_projection
// ... or without the pose optimisation (`tracking_pose_by_optimization`): likewise
#pragma weak mvo_optimize_pose
// ... or without the second search of the local map (`tracking_local_map`): likewise
#pragma weak mvo_map_upload_view
#pragma weak mvo_map_match_features_local
// ... or without the map-point refresh (`map_point_refresh`): likewise
#pragma weak mvo_map_refresh
// ... or without the position refinement (`map_point_refine_positions`): likewise
#pragma weak mvo_map_refine_positions
// ... or without the fusion of duplicate map points (`map_point_fuse`): likewise
#pragma weak mvo_map_fuse
// ... or without the new map points from the window (`map_point_create_from_window`): likewise
#pragma weak mvo_window_triangulate
// ... or without the cell-wise detector (`orb_distribute_keypoints`): likewise
#pragma weak mvo_orb_distribute_configure
#pragma weak mvo_calc_keypoints_distributed

using namespace my_slam;

namespace {
// record = 4-character tag, int64 byte count, payload; a frame starts with "FRAM"
struct FrameLog {
    FILE* f = nullptr;
    bool params_logged = false;  // ORBD goes into the first frame
    ~FrameLog() {
        if (f) fclose(f);
    }
    void put(const char* tag, const void* p, size_t bytes) {
        if (!f) return;
        const long long n = (long long)bytes;
        fwrite(tag, 1, 4, f);
        fwrite(&n, 8, 1, f);
        if (bytes) fwrite(p, 1, bytes, f);
    }
    template <class T>
    void vec(const char* tag, const vector<T>& v) {
        put(tag, v.data(), v.size() * sizeof(T));
    }
    void frame(int img_id, const vo::Frame::Ptr& fr) {
        static_assert(sizeof(cv::KeyPoint) == 28 && sizeof(cv::DMatch) == 16, "record layouts");
        const int head[2] = {img_id, fr->id_};
        put("FRAM", head, sizeof head);
        if (geometry::orbDistributeKeypoints() && !params_logged) {
            const mvo_orb_distribute_params p = geometry::orbDistributeParams();
            put("ORBD", &p, sizeof p);
            params_logged = true;
        }
        vec("KPTS", fr->keypoints_);
        put("DESC", fr->descriptors_.data, (size_t)fr->descriptors_.rows * 32);
        if (!fr->distribute_candidates_per_level_.empty()) {  // `orb_distribute_keypoints: 1`
            vector<int> rec(1, (int)fr->distribute_candidates_per_level_.size());
            rec.insert(rec.end(), fr->distribute_candidates_per_level_.begin(), fr->distribute_candidates_per_level_.end());
            rec.insert(rec.end(), fr->distribute_keypoints_per_level_.begin(), fr->distribute_keypoints_per_level_.end());
            vec("ODCN", rec);
        }
    }
    // opens the log of `save_frame_log_to`, if asked for
    void open() {
        if (!basics::Config::has("save_frame_log_to")) return;
        f = fopen(basics::Config::get<string>("save_frame_log_to").c_str(), "wb");
        if (!f) throw std::runtime_error("cannot open save_frame_log_to");
    }
    void tracked(const vo::MapOnDevice& dev_map, const vo::Frame::Ptr& fr, bool good, bool is_keyframe) {
        vector<int> order;
        for (const vo::MapPoint::Ptr& p : dev_map.order()) order.push_back(p->id_);
        if (fr->refreshed_) order = fr->refresh_order_before_;  // `map_point_refresh: 1`: the refresh has re-read the map since
        if (fr->positions_refined_) order = fr->refine_order_before_;  // `map_point_refine_positions: 1`: likewise, and it came first
        if (fr->fused_) order = fr->fuse_order_before_;  // `map_point_fuse: 1`: likewise, and it came before both
        vec("MORD", order);  // iteration order of Map::map_points_ when the frame looked at the map
        if (!fr->projection_pred_T_.empty()) {  // `tracking_match_by_projection: 1`: what the matcher saw
            vec("PRVP", fr->projection_prev_T_);
            double T[16];
            for (int i = 0; i < 16; ++i) T[i] = fr->projection_pred_T_.at<double>(i / 4, i % 4);
            put("PRED", T, sizeof T);
            vec("PPOS", fr->projection_map_pos_);
            vec("PDSC", fr->projection_map_desc_);
            vec("MPRJ", fr->projection_matches_);
        }
        if (fr->pose_opt_fallback_ >= 0) {  // `tracking_pose_by_optimization: 1`: what the call saw and gave, if it was made
            if (!fr->pose_opt_setup_.empty()) {
                vec("OSET", fr->pose_opt_setup_);
                vec("OINI", fr->pose_opt_init_);
                vec("OP3D", fr->pose_opt_p3_);
                vec("OP2D", fr->pose_opt_p2_);
                vec("OSIG", fr->pose_opt_sigma_);
                vec("OTWC", fr->pose_opt_T_w_c_);
                vec("OTCW", fr->pose_opt_T_c_w_);
                vec("OINF", fr->pose_opt_info_);
                vec("OCHI", fr->pose_opt_chi2_);
                vec("OOUT", fr->pose_opt_outlier_);
            }
            put("OFBK", &fr->pose_opt_fallback_, sizeof(int));
        }
        if (fr->local_map_applied_ >= 0) {  // `tracking_local_map: 1`: what the pass saw and gave, if it was made
            vec("LSET", fr->local_map_setup_);
            vec("LINI", fr->local_map_init_);
            vec("LSKP", fr->local_map_skip_);
            vec("LLVL", fr->local_map_t_level_);
            vec("LPOS", fr->local_map_pos_);
            vec("LDSC", fr->local_map_desc_);
            vec("LNRM", fr->local_map_normal_);
            vec("LMXD", fr->local_map_max_dist_);
            vec("LMAT", fr->local_map_matches_);
            if (!fr->local_map_info_.empty()) {
                vec("LP3D", fr->local_map_p3_);
                vec("LP2D", fr->local_map_p2_);
                vec("LSIG", fr->local_map_sigma_);
                vec("LTWC", fr->local_map_T_w_c_);
                vec("LINF", fr->local_map_info_);
                vec("LCHI", fr->local_map_chi2_);
                vec("LOUT", fr->local_map_outlier_);
            }
            const int applied[2] = {fr->local_map_applied_, fr->local_map_outcome_};
            put("LAPP", applied, sizeof applied);
        }
        vec("MMAP", fr->matches_with_map_);  // the PnP inliers' matches (vo.cpp:336-349)
        const int flags[2] = {good ? 1 : 0, is_keyframe ? 1 : 0};
        put("FLAG", flags, sizeof flags);
    }
    void keyframe(const vo::Map::Ptr& map, const vo::Frame::Ptr& fr) {
        vec("MREF", fr->matches_with_ref_);
        if (!fr->epipolar_F_.empty()) {  // `triangulation_match_by_epipolar_line: 1`
            unsigned char rec[8 + 72];
            const int head[2] = {fr->epipolar_ref_id_, 0};
            std::memcpy(rec, head, 8);
            std::memcpy(rec + 8, fr->epipolar_F_.ptr<double>(0), 72);
            put("EPIF", rec, sizeof rec);
            double T[16];
            for (int i = 0; i < 16; ++i) T[i] = fr->epipolar_ref_T_w_c_.at<double>(i / 4, i % 4);
            put("EPIR", T, sizeof T);
        }
        triangulated(fr);
        if (fr->window_created_) {  // `map_point_create_from_window: 1`: what the call saw and gave
            vec("WSET", fr->window_setup_);
            vec("WKPN", fr->window_kp_count_);
            vec("WTWC", fr->window_T_w_c_);
            vec("WDSC", fr->window_desc_);
            vec("WPIX", fr->window_xy_);
            vec("WSCL", fr->window_scale_);
            vec("WCON", fr->window_conn_);
            vec("WPTS", fr->window_points_);
            vec("WPTP", fr->window_points_p_);
            vec("WPTC", fr->window_points_cos2_);
            vec("WPRS", fr->window_pairs_);
            vec("WPRP", fr->window_pairs_p_);
            vec("WPRC", fr->window_pairs_cos2_);
            vec("WCNT", fr->window_counts_);
            vec("WIDS", fr->window_ids_);
            vec("WPOS", fr->window_world_);
            vec("WMSZ", fr->window_map_size_);
            const vector<int>& c = fr->window_counts_;
            printf("frame %d: %d new map points from the window (%d free keypoints, %d active frames, %d pairs, %d accepted), map %d -> %d\n",
                   fr->id_, c[11], c[0], c[1], c[3], c[10], fr->window_map_size_[0], fr->window_map_size_[1]);  // (with or without a log file)
        }
        mapAfter(map);
        if (fr->fused_) {  // `map_point_fuse: 1`: what the call saw and gave
            vec("USET", fr->fuse_setup_);
            vec("UMID", fr->fuse_map_ids_);
            vec("UPOS", fr->fuse_map_pos_);
            vec("UMDS", fr->fuse_map_desc_);
            vec("UKPN", fr->fuse_kp_count_);
            vec("UTWC", fr->fuse_T_w_c_);
            vec("UDSC", fr->fuse_desc_);
            vec("UPIX", fr->fuse_xy_);
            vec("USCL", fr->fuse_scale_);
            vec("UCON", fr->fuse_conn_);
            vec("UREP", fr->fuse_replaced_by_);
            vec("UADD", fr->fuse_added_);
            vec("UCNT", fr->fuse_counts_);
            vec("UIDS", fr->fuse_map_ids_after_);
            const vector<int>& c = fr->fuse_counts_;
            printf("frame %d: %d of %d map points fused into others (%d merges refused), %d observations added (%d refused) of %d candidates\n",
                   fr->id_, c[5], (int)fr->fuse_replaced_by_.size(), c[2], c[3], c[4], c[0]);  // (with or without a log file)
        }
        if (fr->positions_refined_) {  // `map_point_refine_positions: 1`: what the call saw and gave
            vec("FSET", fr->refine_setup_);
            vec("FTWC", fr->refine_T_w_c_);
            vec("FOBS", fr->refine_obs_start_);
            vec("FFRM", fr->refine_obs_frame_);
            vec("FPIX", fr->refine_obs_uv_);
            vec("FBEF", fr->refine_pos_before_);
            vec("FAFT", fr->refine_pos_after_);
            vec("FCHI", fr->refine_chi2_);
            vec("FINF", fr->refine_info_);
            vec("FOUT", fr->refine_outlier_);
            int n_refined = 0, n_flagged = 0;
            for (size_t i = 0; i < fr->refine_info_.size(); i += 3) n_refined += fr->refine_info_[i] == 0 ? 1 : 0;
            for (unsigned char c : fr->refine_outlier_) n_flagged += c ? 1 : 0;
            printf("frame %d: %d of %d map point positions refined from %d observations (%d flagged as outliers)\n", fr->id_, n_refined,
                   (int)fr->refine_info_.size() / 3, fr->refine_obs_start_.back(), n_flagged);  // (with or without a log file)
        }
        if (fr->refreshed_) {  // `map_point_refresh: 1`: what the refresh saw and gave
            vec("ROBS", fr->refresh_obs_start_);
            vec("RDSC", fr->refresh_obs_desc_);
            vec("RCAM", fr->refresh_obs_cam_);
            vec("RPOS", fr->refresh_pos_);
            vec("RCHO", fr->refresh_choice_);
            vec("RNRM", fr->refresh_norm_);
            int n_seen = 0, n_moved = 0;
            for (int c : fr->refresh_choice_) n_seen += c >= 0 ? 1 : 0, n_moved += c > 0 ? 1 : 0;
            printf("frame %d: %d map points refreshed from %d observations (%d observed, %d took another descriptor than their first)\n",
                   fr->id_, (int)fr->refresh_choice_.size(), fr->refresh_obs_start_.back(), n_seen, n_moved);  // (with or without a log file)
        }
    }
    void initialization(const vo::Map::Ptr& map, const vo::Frame::Ptr& fr, const vo::InitReport& rep, bool initialized) {
        vec("MREF", fr->matches_with_ref_);  // the matches with the first keyframe
        const int head[8] = {rep.slot, rep.n_slot_inliers, rep.n_kept, rep.scaled, rep.criteria[0], rep.criteria[1], rep.criteria[2], rep.good};
        const double tail[4] = {rep.mean_depth, rep.scale, rep.median_angle, rep.mean_pixel_dist};
        unsigned char rec[sizeof head + sizeof tail];
        std::memcpy(rec, head, sizeof head);
        std::memcpy(rec + sizeof head, tail, sizeof tail);
        put("INIT", rec, sizeof rec);
        triangulated(fr);
        if (initialized) mapAfter(map);
    }
    void triangulated(const vo::Frame::Ptr& fr) {
        vec("IREF", fr->inliers_matches_with_ref_);
        vec("I3DM", fr->inliers_matches_for_3d_);
        vec("I3DP", fr->inliers_pts3d_);
    }
    void mapAfter(const vo::Map::Ptr& map) {
        vector<int> ids;
        vector<float> pos;
        for (auto& kv : map->map_points_) {
            ids.push_back(kv.first);
            pos.push_back(kv.second->pos_.x);
            pos.push_back(kv.second->pos_.y);
            pos.push_back(kv.second->pos_.z);
        }
        vec("MIDS", ids);  // the map after the insertion (+ culling)
        vec("MPOS", pos);
    }
    void pose(const vo::Frame::Ptr& fr) {
        double T[16];
        for (int i = 0; i < 16; ++i) T[i] = fr->T_w_c_.at<double>(i / 4, i % 4);
        put("POSE", T, sizeof T);
    }
};

// basics::imread, then basics::undistort when the dataset section carries distortion coefficients
cv::Mat readFrameImage(const string& path, const cv::Mat& K, const vector<double>& dist) {
    cv::Mat img = basics::imread(path);
    if (img.data == nullptr || dist.empty()) return img;
    return basics::undistort(img, K, dist);
}

// `init_from_images: 1`: the reference's loop (run_vo.cpp:110-148) around VisualOdometry::addFrame
int runFromImages(const vector<string>& image_paths, const cv::Mat& K, const vector<double>& dist, int n_proc, FrameLog& log) {
    if (!mvo_init_two_view) throw std::runtime_error("init_from_images: this libmvo_hip.so has no mvo_init_two_view");
    vo::VisualOdometry::Ptr odometry(new vo::VisualOdometry(K));
    vector<cv::Mat> cam_pose_history;
    int n_tracked = 0, n_lost = 0, n_keyframes = 0, n_rejected = 0, init_frame = -1;
    for (int img_id = 0; img_id < n_proc; img_id++) {
        cv::Mat rgb_img = readFrameImage(image_paths[img_id], K, dist);
        if (rgb_img.data == nullptr) {
            printf("The image file %s is empty. Finished.\n", image_paths[img_id].c_str());
            break;
        }
        vo::Frame::Ptr frame = vo::Frame::createFrame(rgb_img);
        odometry->addFrame(frame);
        const vo::VisualOdometry::LastFrame& did = odometry->last();
        log.frame(img_id, frame);
        if (did.state_before == vo::VisualOdometry::DOING_INITIALIZATION) {
            log.initialization(odometry->getMap(), frame, did.init, did.initialized);
            if (did.initialized) {
                init_frame = img_id;
                printf("initialised at frame %d: slot %d, %d of %d matches kept, %d map points\n", img_id, did.init.slot, did.init.n_kept,
                       (int)frame->matches_with_ref_.size(), (int)odometry->getMap()->map_points_.size());
            } else {
                n_rejected++;
            }
        } else if (did.state_before == vo::VisualOdometry::DOING_TRACKING) {
            n_tracked += did.is_pnp_good ? 1 : 0;
            n_lost += did.is_pnp_good ? 0 : 1;
            n_keyframes += did.is_keyframe ? 1 : 0;
            log.tracked(odometry->getMapOnDevice(), frame, did.is_pnp_good, did.is_keyframe);
            if (did.is_keyframe) log.keyframe(odometry->getMap(), frame);
        }
        log.pose(frame);
        cam_pose_history.push_back(frame->T_w_c_.clone());  // run_vo.cpp:139-142
        frame->clearNoUsed();  // keeps keypoints_ and descriptors_: what the later frames match the first keyframe with
    }
    const string save_predicted_traj_to = basics::Config::get<string>("save_predicted_traj_to");
    vo::writePoseToFile(save_predicted_traj_to, cam_pose_history);
    printf("frames %d, tracked %d, lost %d, keyframes %d, map points %d -> %s\n", (int)cam_pose_history.size(), n_tracked, n_lost,
           n_keyframes, (int)odometry->getMap()->map_points_.size(), save_predicted_traj_to.c_str());
    if (init_frame < 0)
        printf("never initialised: %d frames rejected, every pose is the first keyframe's\n", n_rejected);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: run_vo <config.yaml>\n");
        return 2;
    }
    try {
        basics::Config::setParameterFile(argv[1]);
        const string dataset_name = basics::Config::get<string>("dataset_name");
        const string sec = dataset_name + ".";
        const string dataset_dir = basics::Config::get<string>(sec + "dataset_dir");
        const int num_images = basics::Config::get<int>(sec + "num_images");
        const vector<string> image_paths = vo::readImagePaths(dataset_dir, num_images, "/rgb_%05d.png");
        const cv::Mat K = vo::readCameraIntrinsics(dataset_name);
        const vector<double> dist = vo::readCameraDistortion(dataset_name);
        if (!dist.empty()) {
            if (!mvo_undistort_configure || !mvo_undistort)
                throw std::runtime_error("camera_info.k1 ... k3: this libmvo_hip.so has no mvo_undistort");
            printf("undistorting every image: k1 %g, k2 %g, p1 %g, p2 %g, k3 %g\n", dist[0], dist[1], dist[2], dist[3], dist[4]);
        }
        if (basics::Config::has("triangulation_match_by_epipolar_line") && basics::Config::get<int>("triangulation_match_by_epipolar_line") != 0) {
            if (!mvo_fundamental_from_poses || !mvo_match_features_epipolar)
                throw std::runtime_error("triangulation_match_by_epipolar_line: this libmvo_hip.so has no mvo_match_features_epipolar");
            printf("keyframes are matched along the epipolar lines of their poses\n");
        }
        if (vo::trackingMatchByProjection()) {
            if (!mvo_predict_pose || !mvo_map_match_features_projection)
                throw std::runtime_error("tracking_match_by_projection: this libmvo_hip.so has no mvo_map_match_features_projection");
            printf("frames are tracked by projection of the map with a predicted pose\n");
        }
        if (vo::trackingPoseByOptimization()) {
            if (!vo::trackingMatchByProjection())
                throw std::runtime_error("tracking_pose_by_optimization requires tracking_match_by_projection: 1");
            if (!mvo_optimize_pose) throw std::runtime_error("tracking_pose_by_optimization: this libmvo_hip.so has no mvo_optimize_pose");
            printf("tracked frames take their pose from a robust optimisation over all matches\n");
        }
        if (vo::trackingLocalMap()) {
            if (!vo::trackingPoseByOptimization())
                throw std::runtime_error("tracking_local_map requires tracking_pose_by_optimization: 1");
            if (!mvo_map_upload_view || !mvo_map_match_features_local)
                throw std::runtime_error("tracking_local_map: this libmvo_hip.so has no mvo_map_match_features_local");
            printf("tracked frames search the local map a second time from the optimised pose\n");
        }
        if (vo::mapPointRefresh()) {
            if (!mvo_map_refresh) throw std::runtime_error("map_point_refresh: this libmvo_hip.so has no mvo_map_refresh");
            printf("map points take descriptor and normal from their observations at every keyframe\n");
        }
        if (vo::mapPointRefinePositions()) {
            if (!mvo_map_refine_positions)
                throw std::runtime_error("map_point_refine_positions: this libmvo_hip.so has no mvo_map_refine_positions");
            printf("map point positions are refined from all their observations at every keyframe\n");
        }
        if (vo::mapPointFuse()) {
            if (!mvo_map_fuse) throw std::runtime_error("map_point_fuse: this libmvo_hip.so has no mvo_map_fuse");
            printf("duplicate map points are fused and missed observations added at every keyframe\n");
        }
        if (vo::mapPointCreateFromWindow()) {
            if (!mvo_window_triangulate) throw std::runtime_error("map_point_create_from_window: this libmvo_hip.so has no mvo_window_triangulate");
            printf("new map points are triangulated against every buffered frame at every keyframe\n");
        }
        if (geometry::orbDistributeKeypoints()) {
            if (!mvo_orb_distribute_configure || !mvo_calc_keypoints_distributed)
                throw std::runtime_error("orb_distribute_keypoints: this libmvo_hip.so has no mvo_calc_keypoints_distributed");
            const mvo_orb_distribute_params p = geometry::orbDistributeParams();
            printf("key points by cell-wise FAST (%d / %d, cells of %d px, edge %d) and a quadtree spread\n", p.ini_threshold,
                   p.min_threshold, p.cell_size, p.edge_threshold);
        }
        const int max_num_imgs_to_proc = basics::Config::get<int>("max_num_imgs_to_proc");
        const bool init_from_images = basics::Config::has("init_from_images") && basics::Config::get<int>("init_from_images") != 0;
        if (init_from_images) {
            FrameLog log;
            log.open();
            return runFromImages(image_paths, K, dist, std::min(max_num_imgs_to_proc, (int)image_paths.size()), log);
        }
        const vector<cv::Mat> truth = vo::readPoseFromFile(basics::Config::get<string>(sec + "true_traj_filename"));
        const int k0 = basics::Config::has("init_keyframe_0") ? basics::Config::get<int>("init_keyframe_0") : 0;
        const int k1 = basics::Config::has("init_keyframe_1") ? basics::Config::get<int>("init_keyframe_1") : 5;
        if (k0 < 0 || k1 <= k0 || k1 >= (int)truth.size()) throw std::runtime_error("init_keyframe_0/1 outside the ground-truth trajectory");

        FrameLog log;
        log.open();
        vo::TrackingState st;
        vector<cv::Mat> cam_pose_history;
        int n_tracked = 0, n_lost = 0, n_keyframes = 0;
        const int n_proc = std::min(max_num_imgs_to_proc, (int)image_paths.size());
        for (int img_id = 0; img_id < n_proc; img_id++) {
            cv::Mat rgb_img = readFrameImage(image_paths[img_id], K, dist);
            if (rgb_img.data == nullptr) {
                printf("The image file %s is empty. Finished.\n", image_paths[img_id].c_str());
                break;
            }
            vo::Frame::Ptr frame = vo::Frame::createFrame(rgb_img);
            frame->calcKeyPoints();  // vo_addFrame.cpp:24-25
            frame->calcDescriptors();
            log.frame(img_id, frame);
            if (img_id < k1) {
                // before the map exists: pose = the last known one (the reference's INITIALIZATION keeps the first pose)
                frame->T_w_c_ = (img_id >= k0 ? truth[k0] : cv::Mat::eye(4, 4, CV_64FC1)).clone();
                if (img_id == k0) {
                    st.pushFrameToBuff(frame);
                    st.map_->insertKeyFrame(frame);
                    st.ref_ = st.prev_ = frame;
                }
            } else if (img_id == k1) {
                // seed the map: the two keyframes get their ground-truth poses, their matches are filtered, triangulated
                // and culled like any keyframe insertion (vo_addFrame.cpp:96-118), then pushed to the map (vo.cpp:528-576)
                frame->T_w_c_ = truth[k1].clone();
                st.pushFrameToBuff(frame);
                vo::triangulateWithReferenceKeyframe(frame, st.ref_, K);
                vo::pushCurrPointsToMap(st, frame);
                st.map_->insertKeyFrame(frame);
                log.keyframe(st.map_, frame);
                st.ref_ = st.prev_ = frame;
                printf("map seeded from frames %d and %d: %d map points\n", k0, k1, (int)st.map_->map_points_.size());
                if (st.map_->map_points_.size() < 10) throw std::runtime_error("too few map points after seeding");
            } else {
                bool is_keyframe = false;
                const bool good = vo::trackFrame(st, frame, K, &is_keyframe);
                n_tracked += good ? 1 : 0;
                n_lost += good ? 0 : 1;
                n_keyframes += is_keyframe ? 1 : 0;
                log.tracked(st.dev_map_, frame, good, is_keyframe);
                if (is_keyframe) log.keyframe(st.map_, frame);
            }
            log.pose(frame);
            cam_pose_history.push_back(frame->T_w_c_.clone());  // run_vo.cpp:139-142
            frame->clearNoUsed();
        }
        const string save_predicted_traj_to = basics::Config::get<string>("save_predicted_traj_to");
        vo::writePoseToFile(save_predicted_traj_to, cam_pose_history);
        printf("frames %d, tracked %d, lost %d, keyframes %d, map points %d -> %s\n", (int)cam_pose_history.size(), n_tracked, n_lost,
               n_keyframes, (int)st.map_->map_points_.size(), save_predicted_traj_to.c_str());
    } catch (const std::exception& e) {
        fprintf(stderr, "run_vo: %s\n", e.what());
        return 1;
    }
    return 0;
}
