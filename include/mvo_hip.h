/* include/mvo_hip.h -- C-ABI of libmvo_hip.so: the MI355X (gfx950) implementation of the per-frame
 * hot path of felixchenfy/Monocular-Visual-Odometry (ORB extract + grid sampling, Hamming/L1 descriptor
 * matching with the reference's filters, sliding-window bundle adjustment).
 *
 * Every entry point names the reference interface it replaces (paths relative to the reference repo).
 * Conventions: plain pointers and sizes, caller-allocated buffers, int status (0 = MVO_OK, <0 = error),
 * never throws, never prints; one mvo_ctx per host thread, one HIP stream per ctx.  Host pointers unless
 * the name ends in _dev.  There is NO CPU fallback: without a usable HIP device mvo_create fails with
 * MVO_ERR_NO_DEVICE and nothing else can be called.
 */
#ifndef MVO_HIP_H
#define MVO_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVO_OK 0
#define MVO_ERR_INVALID (-1)   /* bad argument (e.g. wrong method index: feature_match.cpp:225 throws) */
#define MVO_ERR_NO_DEVICE (-2) /* no HIP device / kernels not loadable */
#define MVO_ERR_CAPACITY (-3)  /* caller buffer or internal candidate buffer too small */
#define MVO_ERR_HIP (-4)       /* HIP runtime error, see mvo_last_error */
#define MVO_ERR_STATE (-5)     /* call order violated (e.g. reuse_pyramid without a pyramid) */

typedef struct mvo_ctx mvo_ctx;

/* cv::KeyPoint, 28 bytes (Frame::keypoints_, include/my_slam/vo/frame.h:32). */
typedef struct {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} mvo_keypoint;

/* cv::DMatch, 16 bytes (Frame::matches_with_ref_, frame.h:38). */
typedef struct {
    int32_t queryIdx, trainIdx, imgIdx;
    float distance;
} mvo_dmatch;

/* The values the reference latches from config/config.yaml:65-69,94-95 in function-local statics
 * (src/geometry/feature_match.cpp:16-19, 42-45, 56-59). */
typedef struct {
    int32_t nfeatures;         /* number_of_keypoints_to_extract */
    float scale_factor;        /* scale_factor */
    int32_t nlevels;           /* level_pyramid (1..8) */
    int32_t fast_threshold;    /* score_threshold */
    int32_t max_keypoints;     /* max_number_of_keypoints */
    int32_t grid_size;         /* kpts_uniform_selection_grid_size */
    int32_t grid_max_per_cell; /* kpts_uniform_selection_max_pts_per_grid */
    /* How cv::ORB resamples its pyramid -- a property of the OpenCV version, not of config.yaml: 1 = INTER_LINEAR_EXACT
     * (OpenCV >= 3.4, what the reference's README asks for: bit-exact 8.8 fixed point), 0 = INTER_LINEAR (older
     * OpenCV: 11-bit coefficients from float coordinates, truncating vertical pass). */
    int32_t pyramid_interpolation;
} mvo_orb_params;

/* ---- context ------------------------------------------------------------------------------- */
int mvo_create(mvo_ctx** ctx, int device);
/* A second context for the SAME host thread that works on the parent's HIP stream instead of a stream of its own: own
 * workspaces, error state and mode, no further hardware queue.  For callers that give one sequence two contexts so that two
 * of its calls can be in progress at once (the bundle adjustment of frame i between its _begin and _end, the extraction of
 * frame i+1 meanwhile).  The HIP runtime spreads its streams over a fixed number of hardware queues in the order of their
 * creation; with two streams per sequence the extraction streams of 24 sequences ended up three to a queue on half of the
 * queues (measured: 3443 / 3551 -> 3874 / 3910 frames/s with sibling contexts).  Destroy the sibling before its parent. */
int mvo_create_sibling(mvo_ctx* parent, mvo_ctx** ctx);
void mvo_destroy(mvo_ctx* ctx);
/* A number that identifies this ctx for the lifetime of the process (never reused, unlike its address): what per-ctx state
 * kept OUTSIDE the library (e.g. "parameters already latched", feature_match.cpp:16-19) is keyed by.  0 for a null ctx. */
unsigned long long mvo_ctx_uid(const mvo_ctx* ctx);
const char* mvo_last_error(const mvo_ctx* ctx);
/* Blocks until all work queued on the ctx stream is done. */
int mvo_synchronize(mvo_ctx* ctx);
/* How the host threads of this process wait for `device` (hipSetDeviceFlags): 0 auto (the runtime's choice: spinning while
 * there are enough cores), 1 spin, 2 yield, 3 block on an interrupt.  A process whose waiting threads outnumber its CPUs
 * (one rank of a multi-GPU node confined to its share of the cores, 24 sequence threads each) should yield or block.  No
 * reference counterpart (OpenCV / g2o do not wait for a device). */
/* (The calling thread's current HIP device is left as it was.) */
#define MVO_WAIT_AUTO 0
#define MVO_WAIT_SPIN 1
#define MVO_WAIT_YIELD 2
#define MVO_WAIT_BLOCK 3
int mvo_set_wait_policy(int device, int policy);
/* Replaces basics::Config::get<...> latching in feature_match.cpp:16-19,42-45,56-59.  Also resets the
 * latched grid dimensions (feature_match.cpp:59-62 latches rows/cols from the FIRST image). */
int mvo_orb_configure(mvo_ctx* ctx, const mvo_orb_params* params);

/* ---- extraction ---------------------------------------------------------------------------- */
/* geometry::calcKeyPoints (src/geometry/feature_match.cpp:11-36; called from Frame::calcKeyPoints,
 * include/my_slam/vo/frame.h:73-76): cv::ORB::detect + selectUniformKptsByGrid.  image: u8, `channels`
 * = 1 (gray) or 3/4 (BGR[A] as cv::imread gives, run_vo.cpp:114).  The device pyramid built here stays
 * cached in the ctx for mvo_calc_descriptors(reuse_pyramid=1).
 * Input limits (deviation 6): every pyramid level must be at least 8 px in each
 * direction (cvRound(width / scale_factor^(nlevels-1)) >= 8, same for height) and width at most 8192 px;
 * otherwise MVO_ERR_INVALID.  cv::ORB has neither limit: it returns no keypoints from a level under
 * 63 px (so none at all from a frame that small) and the keypoints of the larger levels otherwise. */
int mvo_calc_keypoints(mvo_ctx* ctx, const uint8_t* image, int width, int height, int stride,
                       int channels, mvo_keypoint* kps, int cap, int* n);
/* Same with the image already resident in HBM (bench: inputs resident when the timed region starts). */
int mvo_calc_keypoints_dev(mvo_ctx* ctx, const void* d_image, int width, int height, int stride,
                           int channels, mvo_keypoint* kps, int cap, int* n);
/* ---- extraction, the ORB-SLAM way (README.md section 5: "use the ORB-SLAM's method for extracting enough uniformly
 * distributed keypoints across different scales"; the reference names the method and has no function for it).  A second
 * detector next to mvo_calc_keypoints*, chosen per call; the arithmetic is declared in DESIGN.md section 16: FAST-9/16 scored
 * cell by cell (cells of about cell_size px inside the edge_threshold border) with 3 x 3 non-maximum suppression per cell, a
 * cell keeping its corners of score >= ini_threshold or, if it has none, those >= min_threshold; per level a quadtree that
 * splits the candidates until the level's quota of leaves is reached and keeps the best-scored candidate of every leaf; the
 * intensity-centroid angle for the kept points.  Pyramid, per-level scale and quota are those of mvo_orb_configure;
 * fast_threshold is not used.  response = the FAST score. */
typedef struct {
    int32_t ini_threshold;  /* 1..255, default 20 */
    int32_t min_threshold;  /* 1..ini_threshold, default 7 */
    int32_t cell_size;      /* 8..32, default 30 (a cell row is one 64-bit lane mask on the device: cells span < 2 * cell_size) */
    int32_t edge_threshold; /* 19..31, default 19 */
} mvo_orb_distribute_params;
/* params == NULL restores the defaults.  MVO_ERR_INVALID for a value outside the ranges above. */
int mvo_orb_distribute_configure(mvo_ctx* ctx, const mvo_orb_distribute_params* params);
/* Arguments, limits and the cached pyramid as for mvo_calc_keypoints; selectUniformKptsByGrid follows as there.  A level too
 * small for one cell yields no keypoints.  Up to two keypoints more than its quota can come from a level. */
int mvo_calc_keypoints_distributed(mvo_ctx* ctx, const uint8_t* image, int width, int height, int stride,
                                   int channels, mvo_keypoint* kps, int cap, int* n);
int mvo_calc_keypoints_distributed_dev(mvo_ctx* ctx, const void* d_image, int width, int height, int stride,
                                       int channels, mvo_keypoint* kps, int cap, int* n);
/* The candidates of the last mvo_calc_keypoints_distributed* in their declared order (level, cell row, cell column, y, x),
 * level coordinates.  out == NULL only queries the count. */
typedef struct {
    int32_t x, y, level, score;
} mvo_distribute_candidate;
int mvo_debug_get_distribute_candidates(mvo_ctx* ctx, mvo_distribute_candidate* out, int cap, int* n);

/* geometry::calcDescriptors (feature_match.cpp:38-49; Frame::calcDescriptors, frame.h:77-86):
 * cv::ORB::compute.  May DROP keypoints (feature_match.h:15-17): kps/n are in/out.  desc: n*32 bytes.
 * rgb (optional): n*3 bytes, the per-keypoint colour of frame.h:80-85 / basics::getPixelAt
 * (src/basics/opencv_funcs.cpp:10-32).  reuse_pyramid != 0: `image` must be the image of the last
 * mvo_calc_keypoints[_dev] call on this ctx (the pyramid is NOT rebuilt; image is still read for rgb
 * and may be NULL if rgb is NULL). */
int mvo_calc_descriptors(mvo_ctx* ctx, const uint8_t* image, int width, int height, int stride,
                         int channels, int reuse_pyramid, mvo_keypoint* kps, int* n, uint8_t* desc,
                         uint8_t* rgb);
/* Descriptors stay on the device as well (d_desc_out receives a device pointer owned by the ctx, valid
 * until the extraction after the next one on this ctx: two buffers alternate) so the matcher can consume them without a PCIe round trip. */
int mvo_calc_descriptors_dev(mvo_ctx* ctx, mvo_keypoint* kps, int* n, uint8_t* desc,
                             const void** d_desc_out);
/* geometry::selectUniformKptsByGrid (feature_match.cpp:51-84), host-side, in place. grid dims are the
 * latched ones (first call: rows = image_rows / grid_size, cols = image_cols / grid_size). */
int mvo_select_uniform_kpts_by_grid(mvo_ctx* ctx, mvo_keypoint* kps, int* n, int image_rows,
                                    int image_cols);

/* ---- undistortion -------------------------------------------------------------------------- */
/* cv2.undistort(img, K, dist) as python_tools/undistort_all_images.py:11-37 applies it to every image of a dataset
 * before run_vo sees it (config/config.yaml:17,39: "The images should all be undistorted"): cv::undistort with
 * newCameraMatrix = K, i.e. initUndistortRectifyMap to 1/32 px fixed-point maps followed by remap(INTER_LINEAR,
 * BORDER_CONSTANT, 0).  The declared arithmetic, and where it deviates from OpenCV's loops (closed form per pixel,
 * no stripes, int32 coordinates), is DESIGN.md section 13.
 * coeffs in OpenCV's order k1, k2, p1, p2, k3, k4, k5, k6; n_coeffs 4, 5 or 8 (entries beyond n_coeffs are ignored
 * and taken as 0).  The 12- and 14-coefficient models (thin prism, tilt) are MVO_ERR_INVALID. */
typedef struct {
    double fx, fy, cx, cy;
    double coeffs[8];
    int32_t n_coeffs;
} mvo_undistort_params;
/* Builds the map of a width x height image on the device and keeps it in the ctx (python_tools/undistort_all_images.py:11-37
 * computes it again for every image; config/config.yaml:17,39).  The same values again cost nothing; other values
 * rebuild the map.  width at most 8192, width * height at most 2^30, fx and fy non-zero, every value finite;
 * otherwise MVO_ERR_INVALID and the previous configuration stays. */
int mvo_undistort_configure(mvo_ctx* ctx, const mvo_undistort_params* params, int width, int height);
/* cv2.undistort of one image (python_tools/undistort_all_images.py:11-37; config/config.yaml:17,39).  image / out:
 * u8, channels 1, 3 or 4, each handled independently; stride >= width * channels on both sides; out has the size
 * and channel count of the input, bytes of out beyond width * channels of a row are not written.  MVO_ERR_STATE
 * before mvo_undistort_configure or with another size than the configured one. */
int mvo_undistort(mvo_ctx* ctx, const uint8_t* image, int width, int height, int stride, int channels, uint8_t* out,
                  int out_stride);
/* The same with source and destination in HBM (python_tools/undistort_all_images.py:11-37; config/config.yaml:17,39):
 * what a resident pipeline places in front of mvo_calc_keypoints_dev.  d_out is the caller's and must not overlap
 * d_image (MVO_ERR_INVALID).  Asynchronous on the ctx stream, like the extraction that follows it there. */
int mvo_undistort_dev(mvo_ctx* ctx, const void* d_image, int width, int height, int stride, int channels,
                      void* d_out, int out_stride);

/* ---- matching ------------------------------------------------------------------------------ */
/* cv::BFMatcher("BruteForce-Hamming")::knnMatch(k=2) as used at feature_match.cpp:203-208: exact
 * 2-NN, equal distances keep the lower train index first.  idx/dist: nq x 2 int32; a missing
 * neighbour is (-1, INT32_MAX). */
int mvo_match_knn2(mvo_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* idx,
                   int32_t* dist);
int mvo_match_knn2_dev(mvo_ctx* ctx, const void* d_q, int nq, const void* d_t, int nt, int32_t* idx,
                       int32_t* dist);
/* geometry::matchByRadiusAndBruteForce (feature_match.cpp:86-124): per query the first minimum of
 * sum|a-b| over the 32 descriptor bytes among trains within max_px pixels; idx -1 if none.
 * `sum` is 32x the reference's mean-abs-difference. qxy/txy: n x 2 float (KeyPoint::pt). */
int mvo_match_radius_l1(mvo_ctx* ctx, const uint8_t* q, const float* qxy, int nq, const uint8_t* t,
                        const float* txy, int nt, float max_px, int32_t* idx, int32_t* sum);
/* geometry::matchFeatures (feature_match.cpp:126-239; callers vo_addFrame.cpp:42,99, vo.cpp:283).
 * method 1: exact 1-NN (replaces cv::FlannBasedMatcher(LshIndexParams(5,10,2)), which is approximate
 * and RNG-seeded) + d < max(min_d * xiang_gao_ratio, 30); method 2: Lowe ratio d0 < lowe_ratio * d1;
 * method 3: radius-gated L1 + the method-1 threshold; anything else MVO_ERR_INVALID.  Always followed
 * by removeDuplicatedMatches.  The ratios are passed as the reference latches them: get<int> at
 * feature_match.cpp:137-139 turns 0.8 into 1. */
int mvo_match_features(mvo_ctx* ctx, const uint8_t* d1, int n1, const uint8_t* d2, int n2, int method,
                       double xiang_gao_ratio, double lowe_ratio, const float* xy1, const float* xy2,
                       float max_px, mvo_dmatch* out, int cap, int* n);
/* matchFeatures methods 1 / 2 with both descriptor sets already in HBM (device pointers, e.g. the ones
 * mvo_calc_descriptors_dev returns for frame i-1 and frame i). */
int mvo_match_features_dev(mvo_ctx* ctx, const void* d_d1, int n1, const void* d_d2, int n2, int method,
                           double xiang_gao_ratio, double lowe_ratio, mvo_dmatch* out, int cap, int* n);
/* geometry::removeDuplicatedMatches (feature_match.cpp:241-260), host-side, in place. */
int mvo_remove_duplicated_matches(mvo_dmatch* m, int* n);

/* ---- pose-guided matching ------------------------------------------------------------------- */
/* What the reference names as its missing piece and has no function for: README.md:212 (Results: "too few keypoints
 * matches ... doing guided matching based on the estimated camera motion") and README.md:272 (To Do: "Utilize epipolar
 * constraint to do feature matching").  Frame 1 is the query, frame 2 the train; F is 3 x 3 f64 row-major with
 * x2^T F x1 = 0 in pixels.  A pair (i, j) competes only if train keypoint j lies within its tolerance of the epipolar
 * line of query i; the arithmetic of line and gate is declared operation by operation in DESIGN.md section 14:
 *   a = (F0 x + F1 y) + F2, b = (F3 x + F4 y) + F5, c = (F6 x + F7 y) + F8, nrm = a a + b b       (x, y = qxy[i] as f64)
 *   num = (a u + b v) + c;  pass = nrm > 0 && num num <= tol2[j] nrm                                (u, v = txy[j] as f64)
 *   tol2[j] = tl tl, tl = max_line_px * (t_scale ? t_scale[j] : 1)
 * The gate is inclusive; a NaN or a line with nrm == 0 gives the query no candidates.
 * MVO_ERR_INVALID: a null pointer with a positive count, a non-finite F entry, max_line_px negative or NaN, a t_scale
 * entry negative or not finite.  MVO_ERR_CAPACITY: nt > 65535.  nq == 0 or nt == 0 succeed (nt == 0: every idx -1). */
/* README.md:212, README.md:272.  Raw: per query the two nearest gated trains in 256-bit Hamming space, equal distances
 * keep the lower train index first (the tie rule of mvo_match_knn2); a missing neighbour is (-1, INT32_MAX).
 * idx / dist: nq x 2 int32; n_candidates (optional, nq): the number of trains that passed the gate. */
int mvo_match_knn2_epipolar(mvo_ctx* ctx, const uint8_t* q, const float* qxy, int nq, const uint8_t* t,
                            const float* txy, const float* t_scale /* nt or NULL */, int nt, const double* F,
                            double max_line_px, int32_t* idx, int32_t* dist, int32_t* n_candidates);
/* README.md:212, README.md:272.  The same with both descriptor sets already in HBM (the pointers
 * mvo_calc_descriptors_dev returns); qxy, txy and t_scale stay host pointers. */
int mvo_match_knn2_epipolar_dev(mvo_ctx* ctx, const void* d_q, const float* qxy, int nq, const void* d_t,
                                const float* txy, const float* t_scale, int nt, const double* F, double max_line_px,
                                int32_t* idx, int32_t* dist, int32_t* n_candidates);
/* README.md:212, README.md:272.  The raw call followed by the filter: query i is kept if idx0 >= 0, d0 <= max_hamming
 * and (idx1 < 0 or (double)d0 < lowe_ratio * (double)d1) -- a single candidate passes on the ceiling alone.  Then one
 * query per train survives: the smallest distance, on equal distance the lower queryIdx (independent of order, unlike
 * removeDuplicatedMatches).  out is sorted by trainIdx; imgIdx 0 and distance = (float)d0 as mvo_match_features fills
 * them.  MVO_ERR_CAPACITY (with *n set) if cap is too small. */
int mvo_match_features_epipolar(mvo_ctx* ctx, const uint8_t* d1, const float* xy1, int n1, const uint8_t* d2,
                                const float* xy2, const float* scale2, int n2, const double* F, double max_line_px,
                                double lowe_ratio, int max_hamming, mvo_dmatch* out, int cap, int* n);
/* README.md:212 ("based on the estimated camera motion").  Host-side, no ctx: F with x2^T F x1 = 0 from the two
 * camera-to-world poses (row-major 4 x 4) and the intrinsics: T_2_1 = inv(T_w_c_2) * T_w_c_1 (mvo_invert_pose),
 * E = [t]x R, F = K^-T E K^-1.  MVO_ERR_INVALID if a pose is singular or fx / fy is 0. */
int mvo_fundamental_from_poses(const double* T_w_c_1, const double* T_w_c_2, double fx, double fy, double cx,
                               double cy, double* F);

/* ---- bundle adjustment --------------------------------------------------------------------- */
/* The graph optimization::bundleAdjustment builds (src/optimization/g2o_ba.cpp:172-317), flattened:
 * pose vertices 0..F-1 (VertexSE3Expmap), point vertices (VertexSBAPointXYZ, marginalized), one
 * EdgeProjectXYZ2UV + RobustKernelHuber per observation, CameraParameters(f, (cx, cy), 0). */
typedef struct {
    int32_t n_poses, n_points, n_edges;
    double* pose_T_w_c;        /* n_poses x 16 row-major 4x4 cam->world (Frame::T_w_c_), in/out */
    double* points;            /* n_points x 3, in/out (the adapter stores them back as f32, :308-316) */
    const int32_t* edge_pose;  /* n_edges: index into poses */
    const int32_t* edge_point; /* n_edges: index into points */
    const double* edge_uv;     /* n_edges x 2 measured pixel */
    double focal, cx, cy;      /* K(0,0), K(0,2), K(1,2) -- fy is ignored by the reference (:219-222) */
    double info[4];            /* information_matrix (config.yaml:122) */
    double huber_delta;        /* g2o::RobustKernelHuber default delta = 1 */
    int32_t fix_points;        /* is_fix_map_pts */
    const uint8_t* pose_fixed; /* optional per-pose setFixed flags; NULL = none (as the reference) */
    int32_t max_iterations;    /* optimizer.optimize(50) */
} mvo_ba_problem;

typedef struct {
    int32_t iterations, trials, terminated;
    int32_t failed_solves;     /* trials whose reduced system was "not positive" for Eigen::LDLT (g2o: solve() returns false) */
    double chi2_initial, chi2_final, lambda_final;
    int32_t stale_steps;       /* of those: g2o applied the solver's previous x and accepted it (negative predicted decrease) */
    int32_t reserved_;
} mvo_ba_stats;

/* optimization::bundleAdjustment (g2o_ba.cpp:172-317; caller VisualOdometry::callBundleAdjustment_,
 * src/vo/vo.cpp:458-462).  The solver stack g2o_ba.cpp:193-200 builds is followed to the letter: Levenberg-Marquardt with
 * g2o's lambda / nu rules, Schur complement on the points, the reduced system through Eigen::LDLT's pivot order and sign rule
 * (LinearSolverDense), and -- as OptimizationAlgorithmLevenberg::solve does -- a FAILED linear solve still applies the solver's
 * previous x and scores it with chi2 = DBL_MAX (stats->failed_solves / ->stale_steps). */
int mvo_bundle_adjustment(mvo_ctx* ctx, mvo_ba_problem* problem, mvo_ba_stats* stats);
/* How this ctx shares the GPU (no reference counterpart: g2o and cv::ORB are single-threaded).
 * LATENCY (default): one sequence wants its frame back as fast as possible -- a window is cut into ~300 observations per
 * workgroup (the 5-keyframe window of the benchmark: 28 CUs of one XCD, shortest solve) and solved by a launch of its own;
 * the detection kernel also puts its candidates in order on the device.
 * THROUGHPUT: many sequences are in flight on this GPU -- CU time counts, not latency.  While the offered load keeps it
 * busy (128 submissions in a row at a rate x solve time of >= 8 of its 16 slots; it leaves after 80 ms below 7), 5-keyframe windows are cut into ~670 observations
 * per workgroup (14 CUs) and go to the resident solver service: a grid that stays on the device (2 x 14 CUs of every XCD)
 * and pulls windows from pinned mailboxes, no launch per window.  With less load the windows take the LATENCY cut on the
 * launch path and the CUs stay with whoever has work.  Detection leaves the interleaving of a tile row's candidates to the
 * calling thread (~75 us of host time per frame instead of ~8 us of kernel time), and descriptors are sampled from whole
 * blurred pyramid levels (one blur of every level behind the detection kernel instead of one blur per keypoint window: a fifth
 * of the instructions, one launch more).
 * The summation order of a solve (hence the last bits of its result) follows the cut; every cut is deterministic and is what
 * mvo_debug_get_ba_plan reports.  Results of the extraction do not depend on the mode.
 * SHARED: many sequences are in flight, but the bundle adjustment is not what their frames mostly wait for (tracking rows --
 * map points in view, solvePnPRansac -- or other stages in the loop: ~2500 windows/s on this GPU instead of ~5000).  Windows keep the
 * THROUGHPUT cut but always take the launch path (1...16 windows per grid): a resident grid would hold 208 CUs for slots that
 * are half empty (tracking rows in the loop: 1800 frames/s with the grid, 2470 without).  The caller knows its loop; the library's
 * load estimate only sees submission times and cannot tell a saturated launch path from a loop that is busy elsewhere. */
#define MVO_BA_MODE_LATENCY 0
#define MVO_BA_MODE_THROUGHPUT 1
#define MVO_BA_MODE_SHARED 2
int mvo_ba_set_mode(mvo_ctx* ctx, int mode);
/* Admission gate of the extraction / matching kernels (no reference counterpart).  Contexts in THROUGHPUT or SHARED mode pass a
 * process-wide, per-device counting gate around every launch-and-wait section of mvo_calc_keypoints*, mvo_calc_descriptors* and
 * the matchers: at most `n` such sections are in flight on a device at once (default 8; 0 = no limit).  With 24-32 sequences
 * next to the resident solver grid the frames' kernels share the few CUs the grid leaves; more than ~8 frames interleaving
 * there LOWER their combined throughput (14 in flight: 3400 frames/s of extraction, 8-9: 4600; values 4...12 are within 4 % of
 * each other).  LATENCY-mode contexts never wait at the gate.  Returns the previous value. */
int mvo_set_extract_concurrency(int n);

/* ---- operating knobs, in one place -------------------------------------------------------------------------------------
 * What a caller chooses (API):
 *   mvo_ba_set_mode(ctx, LATENCY | THROUGHPUT | SHARED)   how this ctx shares the GPU (above)
 *   mvo_set_extract_concurrency(n)                        admission gate of the frame kernels (above)
 *   mvo_set_wait_policy(device, AUTO|SPIN|YIELD|BLOCK)    how host threads wait for the device
 *   mvo_orb_params.pyramid_interpolation                  which OpenCV resampling the pyramid restates
 * Environment variables, read once at start-up -- defaults in [] -- for A/B measurements and development; results never
 * depend on them except through the summation plan of a BA window, which mvo_debug_get_ba_plan always reports:
 *   MVO_EXTRACT_CONCURRENCY [8]   start-up value of mvo_set_extract_concurrency
 *   MVO_BA_SERVICE [1]            resident solver service: 0 never, 1 by offered load (mvo_ba_set_mode), 2 always
 *   MVO_BA_XCD_RESERVE [4]        CUs per XCD a BA window leaves to other kernels (28 workgroups of a LATENCY window, 2 x 14 of THROUGHPUT windows)
 *   MVO_BA_WGS, MVO_BA_NSPLIT     force the workgroups / Schur column pieces of a window (= the debug keys ba_wgs, ...)
 *   MVO_BA_CU_SHARE [all]         CUs one launch-path grid may take
 *   MVO_BA_GROUPS [1], MVO_BA_ALIAS_SL [1], MVO_BA_BLOCK_SOLVER [0]   A/B switches of DESIGN.md 4.3 (grouped Schur exchange,
 *                                 reduced system inside the U area, block LDL^T for the 5-pose class)
 *   MVO_BRIEF_LEVEL_BLUR [by mode] 1 = descriptors from whole blurred levels (k_blur + k_brief_sample), 0 = per-keypoint windows
 *   MVO_BA_UV_GLOBAL [1]          0 = the measurements of a > 512-observation range never leave LDS (1: device memory when LDS would cost a chunk)
 *   MVO_PNP_CHUNK [by mode]       0 = solvePnPRansac always evaluates all hypotheses at once, n = the first n for every ctx
 *                                 (default: the first 32 for a THROUGHPUT / SHARED ctx whose previous RANSAC loop was short)
 *   MVO_BRIEF_WAVES [4], MVO_MATCH_SLICE [256], MVO_PYR_FULL_POOL [0], MVO_PNP_OCC [by mode]   kernel shape A/Bs
 *   MVO_BA_PLAN_TRACE, MVO_HOST_TIMING   development output on stderr
 * mvo_debug_set(key, value) (bottom of this file) sets the same switches at run time for the tests. */

/* The same call in two halves, so that the host thread can do other work (e.g. extract the next frame on another
 * ctx) while the window is being solved: _begin builds the window, uploads it and queues the launch, _end blocks
 * until it is done and writes poses / points / stats back like mvo_bundle_adjustment.  One solve in flight per ctx;
 * `problem` must stay valid between the two calls. */
int mvo_bundle_adjustment_begin(mvo_ctx* ctx, const mvo_ba_problem* problem);
int mvo_bundle_adjustment_end(mvo_ctx* ctx, mvo_ba_problem* problem, mvo_ba_stats* stats);
/* n independent windows (e.g. the windows of n sequences) solved in one grid (8 windows x 32 workgroups fill the 256
 * CUs; more than 8 are split over consecutive launches).  Same results as n mvo_bundle_adjustment calls.
 * Concurrency note: every BA launch of the process is issued by one service thread per device, which also batches
 * windows submitted by different ctx / host threads at the same time -- callers need no co-ordination. */
int mvo_ba_solve_batch(mvo_ctx* ctx, mvo_ba_problem* problems, int n, mvo_ba_stats* stats);

/* The same solve with the window resident in HBM: mvo_ba_prepare uploads the graph once (inputs + the
 * pose / point adjacency the kernels need), mvo_ba_solve_resident runs one full optimize(50) from the
 * resident initial state (asynchronous on the ctx stream; may be repeated), mvo_ba_fetch copies the
 * refined poses (n_poses x 16) / points (n_points x 3, untouched when fix_points) / stats back. */
typedef struct mvo_ba_handle mvo_ba_handle;
int mvo_ba_prepare(mvo_ctx* ctx, const mvo_ba_problem* problem, mvo_ba_handle** handle);
int mvo_ba_solve_resident(mvo_ctx* ctx, mvo_ba_handle* handle);
int mvo_ba_fetch(mvo_ctx* ctx, mvo_ba_handle* handle, double* poses, double* points, mvo_ba_stats* stats);
void mvo_ba_release(mvo_ctx* ctx, mvo_ba_handle* handle);

/* ---- tracking: the steps between matching and bundle adjustment -------- */
/* The map (vo::Map::map_points_, include/my_slam/vo/map.h:19: MapPoint::pos_ + descriptor_) kept resident in
 * HBM so that map descriptors never cross PCIe between frames.  The order of the uploaded arrays is the
 * host's iteration order of map_points_; indices returned below refer to it. */
typedef struct mvo_map mvo_map;
int mvo_map_create(mvo_ctx* ctx, mvo_map** map);
void mvo_map_release(mvo_ctx* ctx, mvo_map* map);
/* Replaces the device copy: pos n x 3 float (cv::Point3f), desc n x 32 bytes. */
int mvo_map_upload(mvo_ctx* ctx, mvo_map* map, const float* pos, const uint8_t* desc, int n);
/* Positions [first, first+n) only -- what bundleAdjustment writes back (g2o_ba.cpp:306-316). */
int mvo_map_update_positions(mvo_ctx* ctx, mvo_map* map, const float* pos, int first, int n);
/* VisualOdometry::getMappointsInCurrentView_ (src/vo/vo.cpp:16-49): the map points with p_cam.z >= 0 whose
 * pixel lies strictly inside the cols x rows image, in map order.  T_w_c: 4x4 row-major double (inverted
 * on the host like cv::Mat::inv()).  idx / px (n x 2, cv::Point2f) are host outputs of capacity cap;
 * *d_desc_out receives a device pointer (owned by the ctx, valid until the next call) to the gathered
 * n x 32 descriptors = `corresponding_mappoints_descriptors`, ready for mvo_match_features_dev. */
int mvo_map_points_in_view(mvo_ctx* ctx, mvo_map* map, const double* T_w_c, double fx, double fy, double cx,
                           double cy, int cols, int rows, int32_t* idx, float* px, int cap, int* n,
                           const void** d_desc_out);
/* cv::solvePnPRansac(pts_3d, pts_2d, K, cv::Mat(), R_vec, t, false, iterations, reprojection_error,
 * confidence, inliers) as called at src/vo/vo.cpp:326-329 (flags = SOLVEPNP_ITERATIVE): RANSAC over 5-point
 * EPnP hypotheses with the subsets cv::RNG((uint64)-1) draws, then DLT + Levenberg-Marquardt on the inliers.
 * pts3d n x 3 float, pts2d n x 2 float.  *found = 0 when no hypothesis reaches 5 inliers (solvePnPRansac
 * returns false) or n < 5; inliers (ascending indices into the pairs) needs capacity cap >= n. */
int mvo_solve_pnp_ransac(mvo_ctx* ctx, const float* pts3d, const float* pts2d, int n, double fx, double fy,
                         double cx, double cy, int iterations, float reprojection_error, double confidence,
                         double* rvec, double* tvec, int32_t* inliers, int cap, int* n_inliers, int* found);
/* ---- tracking by projection ----------------------------------------------------------------- */
/* Pose-guided matching for the step that runs on every frame, poseEstimationPnP_ (vo.cpp:267-289), which in the
 * reference projects the map with the LAST KEYFRAME's pose and then searches without a radius; README.md:212 names the
 * remedy ("doing guided matching based on the estimated camera motion").  The resident map (mvo_map_*) is projected with
 * T_w_c -- a prediction of the current pose, mvo_predict_pose -- and map point i (the query) competes for frame keypoint
 * j (the train) only if j lies within its radius of i's projection.  Declared operation by operation in DESIGN.md
 * section 15:
 *   projection and in_view: the arithmetic of mvo_map_points_in_view, bit for bit (T_c_w by mvo_invert_pose)
 *   du = (double)txy[j].x - (double)u, dv = (double)txy[j].y - (double)v, d2 = du du + dv dv
 *   pass = in_view && d2 <= r2[j];   r2[j] = rj rj, rj = max_px * (t_scale ? (double)t_scale[j] : 1)
 * The gate is inclusive, a NaN fails, there is no square root.  One launch (k_map_match_projection) per call; the map's
 * positions and descriptors never leave HBM.
 * MVO_ERR_INVALID: a null pointer with a positive count, a null map, a singular or non-finite pose, fx or fy 0, cols or
 * rows <= 0, max_px negative or NaN, a t_scale entry negative or not finite.  MVO_ERR_CAPACITY: nt > 65535.  An empty
 * map succeeds and writes nothing; nt == 0 succeeds (points in view: n_candidates 0, the others -1). */
/* README.md:212, vo.cpp:267-289.  Raw: one row per map point, in the order of the uploaded arrays.  In view: px = its
 * pixel, idx / dist = the two nearest gated keypoints in 256-bit Hamming space, equal distances keep the lower train
 * index first, a missing neighbour is (-1, INT32_MAX), n_candidates = the number of keypoints that passed the gate.
 * Not in view: px (0, 0), idx (-1, -1), dist (INT32_MAX, INT32_MAX), n_candidates -1.
 * px (n_map x 2 f32) and n_candidates (n_map) are optional; idx / dist: n_map x 2 int32. */
int mvo_map_match_knn2_projection(mvo_ctx* ctx, mvo_map* map, const double* T_w_c, double fx, double fy, double cx,
                                  double cy, int cols, int rows, const uint8_t* t, const float* txy,
                                  const float* t_scale /* nt or NULL */, int nt, double max_px, float* px, int32_t* idx,
                                  int32_t* dist, int32_t* n_candidates);
/* README.md:212, vo.cpp:267-289.  The same with the frame's descriptors already in HBM (the pointer
 * mvo_calc_descriptors_dev returns); txy and t_scale stay host pointers. */
int mvo_map_match_knn2_projection_dev(mvo_ctx* ctx, mvo_map* map, const double* T_w_c, double fx, double fy, double cx,
                                      double cy, int cols, int rows, const void* d_t, const float* txy,
                                      const float* t_scale, int nt, double max_px, float* px, int32_t* idx,
                                      int32_t* dist, int32_t* n_candidates);
/* README.md:212, vo.cpp:267-289.  The raw call followed by the filter of mvo_match_features_epipolar, unchanged: query
 * i is kept if idx0 >= 0, d0 <= max_hamming and (idx1 < 0 or (double)d0 < lowe_ratio * (double)d1); one query per train
 * survives (smallest distance, then the lower queryIdx); out is sorted by trainIdx, imgIdx 0, distance (float)d0;
 * queryIdx is the MAP index.  px (n_map x 2) and in_view (n_map uint8) are optional.  MVO_ERR_CAPACITY (with *n set) if
 * cap is too small. */
int mvo_map_match_features_projection(mvo_ctx* ctx, mvo_map* map, const double* T_w_c, double fx, double fy, double cx,
                                      double cy, int cols, int rows, const uint8_t* t, const float* txy,
                                      const float* t_scale, int nt, double max_px, double lowe_ratio, int max_hamming,
                                      float* px, uint8_t* in_view, mvo_dmatch* out, int cap, int* n);
/* include/my_slam/vo/map.h:19 (map_points_.size(), of the resident copy).  The number of points the last mvo_map_upload
 * left resident: the number of rows the three calls above write. */
int mvo_map_size(mvo_ctx* ctx, mvo_map* map, int* n);
/* README.md:212 ("based on the estimated camera motion"), vo.cpp:267-289.  Host-side, no ctx: the constant-velocity
 * prediction D = inv(T_prev2) * T_prev, T_pred = T_prev * D of row-major 4 x 4 camera-to-world poses (inv =
 * mvo_invert_pose, each product summed k = 0..3 in order, no re-orthonormalisation).  T_w_c_prev2 NULL: T_pred = T_prev.
 * MVO_ERR_INVALID for a singular T_prev2. */
int mvo_predict_pose(const double* T_w_c_prev2 /* or NULL */, const double* T_w_c_prev, double* T_w_c_pred);
/* The reference's poseEstimationPnP_ (vo.cpp:291-347) runs cv::solvePnPRansac from minimal subsets even when every match already
 * lies within a few pixels of a predicted pose, and its optimizeSingleFrame (g2o_ba.cpp:34-170, called at vo.cpp:466) has no
 * outlier rounds.  ORB-SLAM's TrackWithMotionModel instead calls Optimizer::PoseOptimization: a robust motion-only optimisation
 * from the predicted pose over all matches, inliers and outliers classified in four rounds.  This is that step, declared
 * operation by operation in DESIGN.md section 21, f64, every operation one IEEE operation in the written order:
 *   state     (R, t) = rows 0..2 of T_c_w; T_c_w^0 = mvo_invert_pose(T_w_c_init)
 *   q_r       ((R_r0 P_x + R_r1 P_y) + R_r2 P_z) + t_r, P = (double)pts3d[k];  u = (fx q_x) / q_z + cx, v likewise
 *   e, c      (u - (double)uv_x, v - (double)uv_y);  c = (e_x e_x + e_y e_y) s_k, s_k = (double)inv_sigma2[k] or 1.0
 *   rho, w    c <= d d ? c : (2 d) sqrt(c) - d d;  c <= d d ? 1 : d / sqrt(c), d = huber_delta; without the kernel c and 1
 *   J         A [-[q]x | I] for the left update q' = q + w x q + v, A the 2 x 3 derivative of the projection
 *   sums      H = sum (w s_k) J^T J (21), b = sum (w s_k) J^T e (6), chi2 = sum rho: slot k mod 256 adds its observations in
 *             ascending k from 0.0, then eight times S <- S[even] + S[odd]
 *   trial     lambda = 1e-3 max diag H at the start of a round; (H + lambda I) delta = -b by 6 x 6 Cholesky; W = Rodrigues(omega),
 *             R' = W R, t' = W t + upsilon; accepted if every participating observation has q_z > 0 at the new state and
 *             chi2' < chi2: the state moves, lambda *= 0.1, the round ends when chi2 - chi2' <= rel_tolerance chi2; otherwise
 *             lambda *= 10; at most `iterations` trials per round
 *   rounds    each starts again from T_c_w^0 with the current inlier set, the kernel on except in the last of >= 2 rounds; after
 *             a round every observation is classified at its final state: outlier = !(q_z > 0) || c > chi2_threshold; an
 *             observation with !(q_z > 0) at the initial pose never takes part and is always an outlier; fewer than min_inliers
 *             left stops the loop
 * info = (status, rounds run, trials, accepted steps, inliers, observations in front at the start).  Status 0: optimised;
 * 1: the inliers fell below min_inliers, the pose of that round is still reported; 2: fewer than min_inliers observations in
 * front at the start (or n == 0, without a launch): the pose is the initial one, bit for bit, every flag 1, chi2 (0, 0); 3: no
 * trial was accepted in any round: the pose is the initial one, bit for bit, the flags are the classification at it.
 * chi2 = (start of round 0, end of the last round run).  T_c_w is the final state of the last round run (last row 0 0 0 1),
 * T_w_c = mvo_invert_pose(T_c_w).
 * MVO_ERR_INVALID: a null pointer with a positive count, a singular or non-finite pose, fx or fy 0 or intrinsics not finite, a
 * non-finite pts3d or pts2d, an inv_sigma2 entry that is negative or not finite, params out of range.  MVO_ERR_CAPACITY:
 * n > 4096.  In every error case nothing is written. */
typedef struct {
    int32_t rounds;          /* 1..8,  default 4 */
    int32_t iterations;      /* 1..64, default 10: LM trials per round */
    int32_t min_inliers;     /* 6..4096, default 10 */
    double chi2_threshold;   /* > 0, finite; default 5.991 */
    double huber_delta;      /* > 0, finite; default sqrt(5.991) */
    double rel_tolerance;    /* >= 0, finite; default 1e-6 */
} mvo_pose_optimize_params;  /* NULL = defaults */
/* ORB-SLAM Optimizer::PoseOptimization in place of cv::solvePnPRansac at vo.cpp:291-347 when the matches come from a predicted
 * pose.  One upload, one launch (k_pose_optimize: one workgroup runs every round, trial and classification), one wait. */
int mvo_optimize_pose(mvo_ctx* ctx, const float* pts3d /* n x 3, world */, const float* pts2d /* n x 2 */,
                      const float* inv_sigma2 /* n or NULL = 1 */, int n, const double* T_w_c_init, double fx, double fy,
                      double cx, double cy, const mvo_pose_optimize_params* params, double* T_w_c /* 16 */,
                      double* T_c_w /* 16, may be NULL */, uint8_t* outlier /* n */, double* chi2 /* 2 */, int32_t* info /* 6 */);
/* The rounds of the last mvo_optimize_pose of this ctx that launched, for localising a parity failure: one row of 6 doubles per
 * round run (inliers going in, chi2 at the start, chi2 at the end, trials, accepted steps, inliers coming out); *n_rounds is
 * set; MVO_ERR_CAPACITY if cap < *n_rounds, MVO_ERR_STATE before the first such call. */
int mvo_debug_get_pose_optimize(mvo_ctx* ctx, double* rows /* cap x 6 */, int cap, int* n_rounds);
/* ---- tracking the local map ------------------------------------------------------------------- */
/* The reference's per-frame step ends with the pose (vo.cpp:267-347); ORB-SLAM's Tracking::TrackLocalMap goes on: with the
 * optimised pose it projects every local map point the first search left unmatched (SearchLocalPoints, Frame::isInFrustum,
 * ORBmatcher::SearchByProjection(F, vpMapPoints, th)) and optimises the pose again over the union.  This is that second
 * search, declared operation by operation in DESIGN.md section 22, f64, every operation one IEEE operation in the written
 * order, nothing from libm but sqrt.  Per map point i:
 *   projection, in_view   the arithmetic of mvo_map_points_in_view, bit for bit (T_c_w by mvo_invert_pose)
 *   dist      d_r = (double)pos_r - T_w_c[4 r + 3];  s = d_x d_x; s = s + d_y d_y; s = s + d_z d_z;  dist = sqrt(s)
 *   in_range  md = (double)max_dist[i];  md > 0 && dist >= 0.8 * (md / level_scale[L-1]) && dist <= 1.2 * md
 *   vc        ((d_x n_x + d_y n_y) + d_z n_z) / dist, n the f32 normal widened;  facing = vc >= min_view_cos (a NaN fails)
 *   lv        the number of l in 0..L-2 with dist * level_scale[l] < md
 *   r2        r r, r = (((vc > near_cos) ? radius_near : radius_far) * radius_scale) * level_scale[lv]
 *   active    in_view && in_range && facing && !skip[i]
 * Per pair: du, dv, d2 as in tracking by projection; pass = active && d2 <= r2 && (t_level[j] == lv || t_level[j] == lv - 1).
 * The gate is inclusive.  One launch (k_map_match_local) per call; positions, descriptors and view data never leave HBM. */
typedef struct {
    double min_view_cos;  /* finite; default 0.5 (Frame::isInFrustum: viewCos < viewingCosLimit rejects) */
    double radius_near;   /* >= 0, finite; default 2.5 (ORBmatcher::RadiusByViewingCos) */
    double radius_far;    /* >= 0, finite; default 4.0 */
    double near_cos;      /* finite; default 0.998 */
    double radius_scale;  /* >= 0, finite; default 1.0 (the th of SearchByProjection) */
    double lowe_ratio;    /* the filter of mvo_map_match_features_local; default 0.8 */
    int32_t max_hamming;  /* ... default 100 (ORBmatcher::TH_HIGH) */
    int32_t pad;
} mvo_local_map_params;   /* NULL = defaults */
/* MapPoint::GetNormal / MapPoint::GetMaxDistanceInvariance of the resident copy: normal n x 3 f32, max_dist n f32, n =
 * mvo_map_size.  Stored as they come (a non-finite normal fails the facing test, max_dist <= 0 the range test).
 * mvo_map_upload invalidates them: the calls below return MVO_ERR_INVALID until they are given again. */
int mvo_map_upload_view(mvo_ctx* ctx, mvo_map* map, const float* normal /* n x 3 */, const float* max_dist /* n */);
/* Tracking::SearchLocalPoints (Frame::isInFrustum + ORBmatcher::SearchByProjection(F, vpMapPoints, th)).  Raw: one row per
 * map point.  Active: px = its pixel, idx / dist = the two nearest passing keypoints in 256-bit Hamming space with the tie rule
 * and the missing-neighbour convention of mvo_match_knn2, n_candidates = the number of passing keypoints, level = lv, view_cos =
 * vc.  Not active: px (0, 0), idx (-1, -1), dist (INT32_MAX, INT32_MAX), n_candidates -1, level -1, view_cos 0.0.
 * t_level[j]: the octave of keypoint j in 0..n_levels-1, or -2 for a keypoint that is already connected and never passes.
 * skip (n_map uint8 or NULL): nonzero for a point already matched in this frame.  level_scale: n_levels (1..16) positive,
 * finite, strictly increasing.  px, n_candidates, level and view_cos are optional.
 * MVO_ERR_INVALID: a null pointer with a positive count, a null map, no view data since the last upload, a singular or
 * non-finite pose, fx or fy 0, cols or rows <= 0, a bad level_scale, a t_level entry outside its set, a parameter outside its
 * range.  MVO_ERR_CAPACITY: nt > 65535.  Every check comes before the upload and nothing is written on error.  An empty map
 * succeeds and writes nothing; nt == 0 succeeds (active points: n_candidates 0). */
int mvo_map_match_knn2_local(mvo_ctx* ctx, mvo_map* map, const double* T_w_c, double fx, double fy, double cx, double cy,
                             int cols, int rows, const uint8_t* t, const float* txy, const int32_t* t_level, int nt,
                             const uint8_t* skip /* n_map or NULL */, const double* level_scale, int n_levels,
                             const mvo_local_map_params* params, float* px, int32_t* idx, int32_t* dist,
                             int32_t* n_candidates, int32_t* level, double* view_cos);
/* Tracking::SearchLocalPoints.  The same with the frame's descriptors already in HBM; the other arrays stay host pointers. */
int mvo_map_match_knn2_local_dev(mvo_ctx* ctx, mvo_map* map, const double* T_w_c, double fx, double fy, double cx, double cy,
                                 int cols, int rows, const void* d_t, const float* txy, const int32_t* t_level, int nt,
                                 const uint8_t* skip, const double* level_scale, int n_levels,
                                 const mvo_local_map_params* params, float* px, int32_t* idx, int32_t* dist,
                                 int32_t* n_candidates, int32_t* level, double* view_cos);
/* ORBmatcher::SearchByProjection(F, vpMapPoints, th), its acceptance rule: the raw call, then point i is kept if idx0 >= 0,
 * d0 <= max_hamming and (idx1 < 0 or t_level[idx0] != t_level[idx1] or (double)d0 <= lowe_ratio * (double)d1) -- the ratio
 * counts only between neighbours of one level, and it is inclusive; one point per keypoint survives (smallest distance, then
 * the lower map index); out is sorted by trainIdx, imgIdx 0, distance (float)d0, queryIdx the MAP index.  px (n_map x 2) and
 * level (n_map) are optional.  MVO_ERR_CAPACITY (with *n set) if cap is too small. */
int mvo_map_match_features_local(mvo_ctx* ctx, mvo_map* map, const double* T_w_c, double fx, double fy, double cx, double cy,
                                 int cols, int rows, const uint8_t* t, const float* txy, const int32_t* t_level, int nt,
                                 const uint8_t* skip, const double* level_scale, int n_levels,
                                 const mvo_local_map_params* params, float* px, int32_t* level, mvo_dmatch* out, int cap,
                                 int* n);
/* ---- map points refreshed from their observations --------------------------------------------- */
/* The reference gives a map point the descriptor and the viewing direction of the ONE frame that created it
 * (pushCurrPointsToMap_, vo.cpp:528-576) and never writes them again; ORB-SLAM, whose matching the calls above follow, keeps a
 * map point as the summary of all its observations.  Declared operation by operation in DESIGN.md section 17:
 *   D[k][j]   256-bit Hamming distance of observations k and j of the point, D[k][k] = 0 included
 *   med[k]    the element at index (m - 1) / 2 (integer division) of row k sorted ascending (ORB-SLAM's vDists[0.5*(N-1)])
 *   choice    the k with the smallest med[k], the lowest k on a tie
 *   normal    p = (double) of the resident f32 position; per observation d_r = p_r - c_r, s = d_x d_x; s = s + d_y d_y;
 *             s = s + d_z d_z; u_r = d_r / sqrt(s); S_r = sum of u_r from 0.0 in observation order; t = S_x S_x; t = t + S_y S_y;
 *             t = t + S_z S_z; norm_r = S_r / sqrt(t).  A point at a camera centre gives NaN, written as it comes.
 * Observations of point i are rows obs_start[i] .. obs_start[i + 1] - 1 of obs_desc / obs_cam (the camera centres, world
 * coordinates); n = mvo_map_size.  A point without observations: choice -1, descriptor unchanged, norm_out (0, 0, 0).
 * MVO_ERR_INVALID: a null map, a null pointer with a positive count, obs_start[0] != 0, obs_start[n] != n_obs, a decreasing
 * obs_start, a non-finite obs_cam.  MVO_ERR_CAPACITY: a point with more than 64 observations; nothing is written.  An empty
 * map succeeds without a launch; n_obs == 0 succeeds, every choice -1. */
/* ORB-SLAM MapPoint::ComputeDistinctiveDescriptors + MapPoint::UpdateNormalAndDepth, in place of vo.cpp:528-576's single copy
 * (MapPoint::descriptor_, norm_; norm_ is read by getViewAngle_, vo.cpp:578-584).  One launch (k_map_refresh): the resident
 * descriptor of every observed point becomes its chosen observation's 32 bytes, in HBM.  desc_out receives the resident
 * descriptors after the call. */
int mvo_map_refresh(mvo_ctx* ctx, mvo_map* map, const uint8_t* obs_desc /* n_obs x 32 */, const double* obs_cam /* n_obs x 3 */,
                    const int32_t* obs_start /* n + 1, n = mvo_map_size */, int n_obs, int32_t* choice /* n */,
                    uint8_t* desc_out /* n x 32, may be NULL */, double* norm_out /* n x 3 */);
/* include/my_slam/vo/map.h:19 (map_points_: MapPoint::pos_, descriptor_ of the resident copy).  The resident arrays, for
 * tests: pos n x 3 f32, desc n x 32 (either may be NULL); *n = mvo_map_size; MVO_ERR_CAPACITY (with *n set) if cap < *n. */
int mvo_debug_get_map(mvo_ctx* ctx, mvo_map* map, float* pos, uint8_t* desc, int cap, int* n);
/* ---- map point positions refined from all their observations ----------------------------------- */
/* The reference sets a map point's position once, from two views (pushCurrPointsToMap_, vo.cpp:528-576), and runs its bundle
 * adjustment with the points fixed (config.yaml:123, is_ba_fix_map_points: "true"): the BA moves poses against these positions
 * and nothing corrects them.  This is the other half of that alternation: the poses fixed, every point an independent
 * 3-unknown least-squares problem over all its observations (ORB-SLAM's local mapping, g2o's structure-only solver).
 * Declared operation by operation in DESIGN.md section 18, f64, every operation one IEEE operation in the written order:
 *   p         (double) of the resident f32 position; T_c_w = mvo_invert_pose(T_w_c) of the observation's frame
 *   q_r       ((R_r0 p_x + R_r1 p_y) + R_r2 p_z) + t_r;  u = (fx q_x) / q_z + cx, v likewise
 *   e         (u - (double)uv_x, v - (double)uv_y);  e2 = e_x e_x + e_y e_y;  d = huber_delta
 *   rho, w    e2 <= d d ? e2 : (2 d) sqrt(e2) - d d;   e2 <= d d ? 1 : d / sqrt(e2)
 *   J         [fx / q_z, 0, -((fx q_x) / (q_z q_z)); 0, fy / q_z, -((fy q_y) / (q_z q_z))] R
 *   H, b, chi2   the sums of w (J0c J0d + J1c J1d), w (J0c e_x + J1c e_y), rho from 0.0 in observation order
 *   LM        lambda = 1e-3 max(H00, H11, H22); a trial solves (H + lambda I) d = -b by 3 x 3 Cholesky, p' = p + d, accepted
 *             if every observation has q_z > 0 at p' and chi2' < chi2: the state moves, lambda *= 0.1, and the loop ends when
 *             chi2 - chi2' <= rel_tolerance chi2; otherwise lambda *= 10; at most max_trials trials in all
 * Observations of point i are rows obs_start[i] .. obs_start[i + 1] - 1 of obs_frame / obs_uv (the convention of
 * mvo_map_refresh); n = mvo_map_size.  info[i] = (status, accepted steps, trials); status 0: refined, the resident position
 * becomes (float)p; 1: fewer than min_observations observations; 2: at the start some observation sees the point at depth
 * !(q_z > 0); 3: no trial accepted (or lambda not positive and finite at the start).  Only status 0 writes the resident
 * position; every other status leaves its bytes untouched and reports them in pos_out.  chi2[i] = (before, after), both 0 for
 * status 1 and 2; obs_outlier[k] = e2 > d d at the final p, 0 for status 1 and 2.
 * MVO_ERR_INVALID: a null map, a null pointer with a positive count, obs_start[0] != 0, obs_start[n] != n_obs, a decreasing
 * obs_start, an obs_frame outside [0, n_frames), a singular or non-finite pose, fx or fy 0 or intrinsics not finite, a non-finite
 * obs_uv, params out of range.  MVO_ERR_CAPACITY: a point with more than 64 observations, n_frames > 64.  In every error case
 * nothing is written.  An empty map succeeds without a launch. */
typedef struct {
    int32_t max_trials;       /* 1..64, default 20 */
    int32_t min_observations; /* 2..64, default 2 */
    double huber_delta;       /* > 0, finite; default sqrt(5.991) (ORB-SLAM, monocular) */
    double rel_tolerance;     /* >= 0, finite; default 1e-6 */
} mvo_map_refine_params;      /* NULL = defaults */
/* ORB-SLAM's per-point structure-only refinement in place of vo.cpp:528-576's single two-view triangulation, the points-free
 * half that config.yaml:123 (is_ba_fix_map_points) leaves out of the bundle adjustment.  One launch (k_map_refine); pos_out
 * receives the resident positions after the call. */
int mvo_map_refine_positions(mvo_ctx* ctx, mvo_map* map, const double* T_w_c /* n_frames x 16 */, int n_frames, double fx, double fy,
                             double cx, double cy, const int32_t* obs_frame /* n_obs */, const float* obs_uv /* n_obs x 2 */,
                             const int32_t* obs_start /* n + 1, n = mvo_map_size */, int n_obs,
                             const mvo_map_refine_params* params, float* pos_out /* n x 3 */, double* chi2 /* n x 2 */,
                             int32_t* info /* n x 3 */, uint8_t* obs_outlier /* n_obs, may be NULL */);
/* ---- duplicate map points fused over the buffered frames ---------------------------------------- */
/* The reference creates a map point whenever the matched keypoint of the previous keyframe is not one already
 * (pushCurrPointsToMap_, vo.cpp:528-576), even when the current keypoint is connected to a map point through the PnP inliers:
 * one physical point enters the map under several ids, each with part of the observations, and a buffered frame that sees a
 * point without having matched it contributes nothing.  ORB-SLAM's local mapping answers both with SearchInNeighbors:
 * ORBmatcher::Fuse projects every map point into every neighbouring keyframe, and MapPoint::Replace merges two points that
 * claim one keypoint.  Declared operation by operation in DESIGN.md section 19:
 *   seen[i]     64-bit mask, bit f set when some conn[f][j] == i
 *   search      per (frame f, map point i): the projection, in_view and the gate of mvo_map_match_knn2_projection with
 *               T_c_w[f] = mvo_invert_pose(T_w_c[f]); active = in_view && !(seen[i] >> f & 1); r2[j] = (max_px scale[j])^2, and
 *               -1.0 for a keypoint with conn == -2, which never passes; the two nearest gated keypoints, equal distances keep
 *               the lower keypoint; a pair that is not active writes the "not in view" row
 *   candidate   (d, f, i, j) with j = idx0 >= 0 and d = dist0 <= max_hamming; no ratio test
 *   claimant    per (f, j) the candidate with the smallest d, then the lower i, wins
 *   merges      the winners with conn[f][j] = i2 >= 0 in ascending (d, f, i), union-find over the map rows, a component's mask the
 *               OR of its members' seen: same component -> nothing; masks intersect -> refused (two points observed in one frame
 *               are two points); else united
 *   additions   after all merges the winners with conn[f][j] == -1 in the same order: bit f of the component's mask set ->
 *               refused; else the bit is set and (f, j, survivor) appended to `added`
 *   survivor    of a component: the member with the largest popcount of its own seen, the lower row on a tie;
 *               replaced_by[i] = the survivor's row (i itself for a point no merge touched)
 * MVO_ERR_INVALID: a null map, a null pointer with a positive count, a conn outside [-2, n_map), a singular or non-finite pose,
 * fx or fy 0, cols or rows <= 0, max_px negative or NaN, a scale entry negative or not finite, max_hamming outside 0..256.
 * MVO_ERR_CAPACITY: n_frames > 64, a frame with more than 65535 keypoints, cap_added too small (*n_added is set).  Every other
 * check precedes the upload, and on error nothing else is written.  An empty map or n_frames == 0 succeeds without a launch; a
 * frame with n == 0 succeeds.  Neither call changes the resident arrays: the caller removes the replaced rows. */
typedef struct {
    const uint8_t* desc;   /* n x 32 */
    const float* xy;       /* n x 2 */
    const float* scale;    /* n or NULL: the t_scale of mvo_map_match_knn2_projection */
    const int32_t* conn;   /* n: >= 0 the map row this keypoint is connected to, -1 free, -2 connected to a point that left
                              the map */
    int32_t n;             /* 0..65535 */
    double T_w_c[16];
} mvo_fuse_frame;
typedef struct { int32_t frame, keypoint, point; } mvo_fuse_observation;
typedef struct { double max_px; int32_t max_hamming; } mvo_map_fuse_params; /* NULL = defaults: 3.0, 50 */
/* ORB-SLAM ORBmatcher::Fuse (the projection search of every map point in every neighbouring keyframe) where vo.cpp:528-576 only
 * ever creates points.  Raw: n_frames blocks of one row per map point, each row by the conventions of
 * mvo_map_match_knn2_projection (not active: px (0, 0), idx (-1, -1), dist (INT32_MAX, INT32_MAX), n_candidates -1).  One upload,
 * one launch (k_map_fuse_search), one wait.  idx / dist: n_frames x n_map x 2 int32; n_candidates (n_frames x n_map) and px
 * (n_frames x n_map x 2 f32) are optional. */
int mvo_map_fuse_search(mvo_ctx* ctx, mvo_map* map, const mvo_fuse_frame* frames, int n_frames, double fx, double fy, double cx,
                        double cy, int cols, int rows, double max_px, int32_t* idx, int32_t* dist, int32_t* n_candidates, float* px);
/* ORB-SLAM ORBmatcher::Fuse + MapPoint::Replace in place of vo.cpp:528-576's unconditional new point: the search above, then the
 * rule on the host.  replaced_by: n_map rows; added: up to cap_added observations, *n_added of them written; counts[6] =
 * candidates, merges accepted, merges refused, observations added, observations refused, points replaced. */
int mvo_map_fuse(mvo_ctx* ctx, mvo_map* map, const mvo_fuse_frame* frames, int n_frames, double fx, double fy, double cx, double cy,
                 int cols, int rows, const mvo_map_fuse_params* params, int32_t* replaced_by /* n_map */,
                 mvo_fuse_observation* added, int cap_added, int* n_added, int32_t* counts /* 6 */);
/* ---- new map points triangulated against every buffered frame ------------------------------------ */
/* The reference triangulates a new keyframe against its reference keyframe only (triangulateWithReferenceKeyframe,
 * vo_addFrame.cpp:104-116; pushCurrPointsToMap_, vo.cpp:528-576): a keypoint without a partner there, or with too little
 * parallax, gets no map point although the other buffered frames see it from wider baselines.  ORB-SLAM's local mapping has
 * LocalMapping::CreateNewMapPoints: every keypoint without a map point is searched along its epipolar line in every
 * neighbouring keyframe, triangulated and verified.  Declared operation by operation in DESIGN.md section 20:
 *   frame f     M_f = mvo_invert_pose(T_w_c_curr) T_w_c_f (R_f, t_f its rows), F_f = mvo_fundamental_from_poses(curr, f);
 *               active when b2 = (tx tx + ty ty) + tz tz satisfies b2 > 0 && b2 >= min_baseline^2
 *   search      per (frame f, keypoint i of curr): the line and the gate of mvo_match_knn2_epipolar with F_f; active = conn_c[i]
 *               == -1 && frame active && nrm > 0; tol2[j] = (max_line_px scale_f[j])^2, and -1.0 for a keypoint of f with
 *               conn != -1, which never passes; the two nearest gated keypoints, equal distances keep the lower keypoint; a pair
 *               that is not active writes idx (-1, -1), dist (INT32_MAX, INT32_MAX), n_candidates -1
 *   pairs       per frame the filter of mvo_match_features_epipolar (ceiling, ratio, one query per train); ordered by (f, j)
 *   verify      per pair pw::triangulate_match(xy_f[j], xy_c[i], R_f, t_f) = the arithmetic of mvo_triangulate_points, then
 *               status = 1 (a float not finite) | 2 (a depth not positive) | 4 (parallax: dot <= 0 or cos2 >= max_cos_parallax^2)
 *               | 8, 16 (reprojection in f, in curr: e2 > max_reproj_chi2 scale^2) | 32 (scale consistency against ratio_factor)
 *   choice      per keypoint of curr the pair with status 0 and the smallest cos2, then the lower frame; sorted by keypoint
 * MVO_ERR_INVALID: a null pointer with a positive count, a singular or non-finite pose, fx or fy 0 or non-finite intrinsics, a
 * negative or NaN max_line_px, min_baseline, max_reproj_chi2 or ratio_factor, lowe_ratio NaN, max_cos_parallax outside [0, 1],
 * max_hamming outside 0..256, a scale entry negative or not finite.  MVO_ERR_CAPACITY: n_frames > 64, more than 65535 keypoints
 * in a frame or in curr, cap_points or cap_pairs too small (*n_points, *n_pairs are set, nothing else is written).  Every check
 * precedes the upload, and on error nothing else is written.  n_frames == 0, no free keypoint and no pair succeed without the
 * launch they would feed.  No resident map is read or changed.  Only conn == -1 ("free") matters in a frame and in curr. */
typedef struct {
    double max_line_px;       /* 2.0 */
    double lowe_ratio;        /* 0.8 */
    int32_t max_hamming;      /* 64 */
    double max_cos_parallax;  /* 0.9998 */
    double max_reproj_chi2;   /* 5.991 */
    double ratio_factor;      /* 1.8 */
    double min_baseline;      /* 0.0 */
} mvo_window_triangulate_params; /* NULL = the defaults beside the fields */
typedef struct {
    int32_t frame, keypoint, train, hamming, status;
    float p_curr[3], p_frame[3]; /* the point in the camera of curr, in the camera of the frame */
    double cos2;
} mvo_window_pair;
typedef struct {
    int32_t keypoint, frame, train, hamming;
    float p_curr[3];
    double cos2;
} mvo_window_point;
/* ORB-SLAM ORBmatcher::SearchForTriangulation against every neighbouring keyframe where vo_addFrame.cpp:104-116 has one pair of
 * views.  Raw: n_frames blocks of one row per keypoint of curr, each row by the conventions of mvo_match_knn2_epipolar.  One
 * upload, one launch (k_window_epipolar_search), one wait.  idx / dist: n_frames x curr->n x 2 int32; n_candidates (n_frames x
 * curr->n) is optional. */
int mvo_window_triangulate_search(mvo_ctx* ctx, const mvo_fuse_frame* curr, const mvo_fuse_frame* frames, int n_frames, double fx,
                                  double fy, double cx, double cy, double max_line_px, double min_baseline, int32_t* idx,
                                  int32_t* dist, int32_t* n_candidates);
/* ORB-SLAM LocalMapping::CreateNewMapPoints in place of vo_addFrame.cpp:104-116's single pair of views: one upload, the search
 * launch, one wait, the filter, one small upload, the verification launch (k_window_verify), one wait, the choice.  points: up
 * to cap_points, *n_points of them written; pairs (may be NULL, then cap_pairs and n_pairs are not looked at): every pair after
 * the filter with its status; counts[12] = free keypoints of curr, active frames, rows with idx0 >= 0, pairs after the filter,
 * pairs failing bit 1, 2, 4, 8, 16, 32, accepted pairs, new points. */
int mvo_window_triangulate(mvo_ctx* ctx, const mvo_fuse_frame* curr, const mvo_fuse_frame* frames, int n_frames, double fx, double fy,
                           double cx, double cy, const mvo_window_triangulate_params* params, mvo_window_point* points,
                           int cap_points, int* n_points, mvo_window_pair* pairs /* may be NULL */, int cap_pairs, int* n_pairs,
                           int32_t* counts /* 12 */);
/* ---- keyframe insertion: epipolar inlier filter, triangulation, culling ---- */
/* geometry::helperTriangulatePoints (src/geometry/motion_estimation.cpp:214-247, called at
 * vo_addFrame.cpp:114-116): pixel2CamNormPlane on the matched pixels of the previous / current keyframe
 * (n x 2 float each, KeyPoint::pt), cv::triangulatePoints with [I|0] and [R|t] = T_curr_to_prev, then
 * basics::transCoord.  Outputs n x 3 float (either may be NULL): the points in the previous camera frame
 * (doTriangulation, epipolar_geometry.cpp:130-175) and what helperTriangulatePoints returns. */
int mvo_triangulate_points(mvo_ctx* ctx, const float* kp_prev, const float* kp_curr, int n, double fx, double fy,
                           double cx, double cy, const double* R, const double* t, float* pts3d_in_prev,
                           float* pts3d_in_curr);
/* geometry::helperFindInlierMatchesByEpipolarCons (src/geometry/motion_estimation.cpp:182-198, called at
 * vo_addFrame.cpp:104-106) = the inlier mask of cv::findEssentialMat(pts1, pts2, focal = (fx + fy) / 2,
 * pp = Point2f(cx, cy), cv::RANSAC, prob, threshold) (epipolar_geometry.cpp:17-47): RANSAC (cv::RNG subsets, at
 * most 1000 iterations, adaptive count) over five-point hypotheses scored by the Sampson distance.  kp_prev /
 * kp_curr: the matched pixels (n x 2 float); inliers: ascending indices into the matches, capacity cap >= n. */
int mvo_find_essential_inliers(mvo_ctx* ctx, const float* kp_prev, const float* kp_curr, int n, double fx, double fy,
                               double cx, double cy, double prob, double threshold, int32_t* inliers, int cap,
                               int* n_inliers);
/* cv::findHomography(src, dst, cv::RANSAC, threshold, noArray(), 2000, confidence) as estiMotionByHomography calls
 * it during the monocular initialisation (src/geometry/motion_estimation.cpp, reached from vo_addFrame.cpp:36-69;
 * the reference passes threshold 3 and the default confidence 0.995).  src / dst: the matched pixels of the first
 * keyframe and of the current frame (n x 2 float).  RANSAC over 4-point normalised DLT hypotheses (cv::RNG
 * subsets with checkSubset, at most 2000 iterations, adaptive count), then for n > 4 the DLT on the inliers and
 * 10 Levenberg-Marquardt iterations on the 8 free entries.  H: row-major 3 x 3 as findHomography returns it (not
 * divided by H(2,2)); found = 0 when findHomography returns an empty matrix (n < 4, no subset passes checkSubset,
 * no hypothesis with 4 inliers).  inliers: ascending indices of the RANSAC mask, capacity cap >= n. */
int mvo_find_homography(mvo_ctx* ctx, const float* src, const float* dst, int n, double threshold, double confidence,
                        double* H, int32_t* inliers, int cap, int* n_inliers, int* found);
/* estiMotionByEssential (src/geometry/epipolar_geometry.cpp:17-57), the essential-matrix branch of the monocular
 * initialisation (called at src/geometry/motion_estimation.cpp:44-50): findEssentialMat(pts1, pts2, focal, pp,
 * RANSAC, prob, threshold) exactly as mvo_find_essential_inliers runs it (the reference passes prob 0.999 and threshold
 * 1.0, config/config.yaml:101-102), E /= E(2,2), then recoverPose(E, pts1, pts2, R, t, focal, pp, mask) with
 * focal = (fx + fy) / 2, pp = the cv::Point2f (cx, cy) and distanceThresh 50, then t /= sqrt(t1^2 + t2^2 + t0^2).
 * Both divisions by a scalar multiply by its reciprocal (cv::Mat::convertTo).  E, R: row-major 3 x 3; t: 3.
 * inliers: ascending indices of the RANSAC mask (taken before recoverPose), capacity cap >= n.  found = 0 when
 * n < 5, when RANSAC finds no model, and when n == 5 and the five-point solver returns several candidates (the
 * reference's decomposeEssentialMat asserts on the stacked 3k x 3 matrix; DESIGN.md section 2, deviation 7).
 * Rotation-only scenes are not special-cased: E, R and t are whatever the decomposition of the fitted E gives. */
int mvo_esti_motion_by_essential(mvo_ctx* ctx, const float* pts1, const float* pts2, int n, double fx, double fy,
                                 double cx, double cy, double prob, double threshold, double* E, double* R, double* t,
                                 int32_t* inliers, int cap, int* n_inliers, int* found);
/* checkEssentialScore and checkHomographyScore (src/geometry/motion_estimation.cpp:501-664, sigma 1 by default,
 * include/my_slam/geometry/motion_estimation.h:104,110; called at motion_estimation.cpp:135-138).  E: as
 * mvo_esti_motion_by_essential returns it; H: mvo_find_homography's H times 1 / H(2,2); K = [fx 0 cx; 0 fy cy; 0 0 1].
 * inl_e / inl_h: the lists to score (indices into pts1 / pts2).  Either model may be NULL: its score is then 0 and
 * its kept list empty.  score_*: the sums in the declared block order of DESIGN.md section 12 (NaN for a match on
 * the epipole, as the reference's loop gives); kept_*: the entries that passed both terms, in list order, capacity
 * n_e / n_h.  The reference leaves checkHomographyScore's sum uninitialised; it starts from 0.0 here (DESIGN.md
 * section 2, deviation 8). */
int mvo_check_init_scores(mvo_ctx* ctx, const float* pts1, const float* pts2, int n, double fx, double fy, double cx,
                          double cy, const double* E, const int32_t* inl_e, int n_e, const double* H,
                          const int32_t* inl_h, int n_h, double sigma, double* score_e, double* score_h, int32_t* kept_e,
                          int* n_kept_e, int32_t* kept_h, int* n_kept_h);
/* estiMotionByHomography + removeWrongRtOfHomography (src/geometry/epipolar_geometry.cpp:59-128), the homography
 * branch of the monocular initialisation: findHomography exactly as mvo_find_homography runs it (H, inliers, cap,
 * n_inliers and found are that call's outputs, except that H is returned times 1 / H(2,2)), then
 * decomposeHomographyMat(H, K) (OpenCV's HomographyDecompInria, K = [fx 0 cx; 0 fy cy; 0 0 1]), each t times
 * 1 / sqrt(t1^2 + t2^2 + t0^2), and filterHomographyDecompByVisibleRefpoints on the inliers' pixel2CamNormPlane
 * points.  Rs (4 x 9, row-major), ts (4 x 3), normals (4 x 3): the n_solutions surviving candidates in OpenCV's
 * order (Ra ta na), (Ra -ta -na), (Rb tb nb), (Rb -tb -nb); unused rows are zero.  A rotation-only H decomposes to
 * one candidate with a zero normal, which the filter removes.  Declared arithmetic: DESIGN.md section 12. */
int mvo_esti_motion_by_homography(mvo_ctx* ctx, const float* pts1, const float* pts2, int n, double fx, double fy,
                                  double cx, double cy, double threshold, double confidence, double* H,
                                  int32_t* inliers, int cap, int* n_inliers, double* Rs, double* ts, double* normals,
                                  int* n_solutions, int* found);

/* Result of mvo_estimate_possible_relative_poses.  The caller sets the four buffers and their capacities; the call
 * fills the rest.  Slot 0 is the E motion (present[0] = found_e), slots 1 .. n_slots - 1 the surviving H candidates
 * (h_candidate[s]: their index 0..3 in the decomposition).  The points of slot s are pts3d[pts_offset[s] ..
 * pts_offset[s] + pts_count[s]) (x, y, z per point, in camera 1), one per entry of the slot's inlier list, slot after
 * slot.  best: the chosen slot, -1 when the reference's rule picks a slot that does not exist (DESIGN.md section 2,
 * deviation 11). */
typedef struct {
    int32_t* inliers_e; /* capacity cap_inliers >= n */
    int32_t* inliers_h; /* capacity cap_inliers >= n */
    int cap_inliers;
    float* pts3d;       /* capacity cap_pts points: n_inliers_e + 4 n_inliers_h suffices */
    int cap_pts;
    double E[9], H[9];  /* E times 1 / E(2,2), H times 1 / H(2,2); zero when absent */
    int found_e, found_h, n_inliers_e, n_inliers_h;
    int n_slots;
    int32_t present[5], h_candidate[5], pts_offset[5], pts_count[5];
    double R[5][9], t[5][3], normal[5][3]; /* normal of slot 0: zero */
    double score_e, score_h, ratio;
    int best;
} mvo_init_poses;

/* geometry::helperEstimatePossibleRelativePosesByEpipolarGeometry (src/geometry/motion_estimation.cpp:10-157) with
 * is_calc_homo = true, the entry point of the monocular initialisation: mvo_esti_motion_by_essential (prob,
 * threshold) and mvo_esti_motion_by_homography (h_threshold, h_confidence) on the same matches, the solution table,
 * doTriangulation of every slot on its inlier list (the arithmetic of mvo_triangulate_points), the two scores of
 * mvo_check_init_scores (sigma), ratio = score_h / (score_e + score_h), and the choice: the H slot with the strictly
 * largest |n_z| when ratio > 0.5 (first slot on ties), else slot 0.  motion_cam2_to_cam1 == 0: every slot's (R, t)
 * is replaced by the inverse of [R t; 0 1] (basics::invRt, the LU of mvo_invert_pose) after the triangulation.
 * An absent model scores 0 (deviations 9 and 10).  The E / H records of the single calls
 * (mvo_debug_get_*) describe this call afterwards. */
int mvo_estimate_possible_relative_poses(mvo_ctx* ctx, const float* pts1, const float* pts2, int n, double fx,
                                         double fy, double cx, double cy, double prob, double threshold,
                                         double h_threshold, double h_confidence, double sigma,
                                         int motion_cam2_to_cam1, mvo_init_poses* out);
/* Parameters of the finish of the monocular initialisation (config/config.yaml:105-113): min_triang_angle and
 * max_ratio_to_median of retainGoodTriangulationResult_, assumed_mean_pts_depth_during_vo_init, and the three
 * thresholds of isVoGoodToInit_.  The reference's values: 1.0, 20, 0.8, 15, 50, 2.0. */
typedef struct {
    double min_triang_angle, max_ratio_to_median, assumed_mean_depth;
    int min_inlier_matches;
    double min_pixel_dist, min_median_triangulation_angle;
} mvo_init_params;
/* Result of mvo_init_two_view.  The caller sets the three buffers and cap (>= n); the call fills the rest.
 * matches_for_3d: curr_->inliers_matches_for_3d_ as indices into the input matches; pts3d_in_curr (x, y, z per
 * point): curr_->inliers_pts3d_; angles: curr_->triangulation_angles_of_inliers_ (degrees), n_kept entries each.
 * slot: the chosen solution (poses->best); n_slot_inliers: the length of its inlier list; scaled: 1 when the depth
 * scaling ran (n_kept >= 20), else 0 with mean_depth = scale = 0 and points, t and T_w_c unscaled (vo.cpp:94-99).
 * R, t: the motion of the chosen slot, t times scale when scaled; T_w_c: curr_->T_w_c_.  mean_pixel_dist: the mean
 * of criteria_1 (NaN when nothing is kept); mean / median / min / max_angle: what isVoGoodToInit_ prints (0 when
 * nothing is kept); criteria[3] and good: its three tests and their conjunction. */
typedef struct {
    int32_t* matches_for_3d;
    float* pts3d_in_curr;
    double* angles;
    int cap;
    int slot, n_slot_inliers, n_kept, scaled;
    double R[9], t[3], T_w_c[16], mean_depth, scale;
    double mean_pixel_dist, mean_angle, median_angle, min_angle, max_angle;
    int criteria[3], good;
} mvo_init_result;
/* The DOING_INITIALIZATION step after the matching: VisualOdometry::estimateMotionAnd3DPoints_ (src/vo/vo.cpp:53-110)
 * and VisualOdometry::isVoGoodToInit_ (vo.cpp:112-170) as vo_addFrame.cpp:50-56 calls them.  Runs
 * mvo_estimate_possible_relative_poses with motion_cam2_to_cam1 = 1 (vo.cpp:66; poses receives exactly that call's
 * outputs), then on slot poses->best: basics::transCoord of the slot's points into the current camera, the pose
 * T = T_w_c_ref * [R t; 0 1]^-1 (the LU of mvo_invert_pose; the product summed k = 0..3 in order),
 * retainGoodTriangulationResult_ (vo.cpp:181-244, the rule of mvo_retain_good_triangulation on cosines computed by
 * the device: acos, the sort for the median and the keep list are host-side), the N < 20 early return, the depth
 * scaling to assumed_mean_depth with the pose recomputed from the scaled t, and the three criteria, which are
 * evaluated in either case.  T_w_c_ref: ref_->T_w_c_, row-major 4 x 4.  A NaN angle (a cosine outside [-1, 1] by
 * rounding, or a zero ray) is treated exactly as mvo_retain_good_triangulation treats it: both comparisons of the
 * keep rule are false for it, so the point is kept, and it takes part in the sort for the median as it is.
 * best == -1 (deviations 9-11; the reference would index list_R[-1]): nothing is launched,
 * slot = -1, n_kept = 0, all criteria and good are 0, T_w_c = T_w_c_ref, and the call returns MVO_OK (deviation 12). */
int mvo_init_two_view(mvo_ctx* ctx, const float* pts1, const float* pts2, int n, double fx, double fy, double cx,
                      double cy, double prob, double threshold, double h_threshold, double h_confidence, double sigma,
                      const double* T_w_c_ref, const mvo_init_params* params, mvo_init_poses* poses,
                      mvo_init_result* out);
/* VisualOdometry::retainGoodTriangulationResult_ (src/vo/vo.cpp:181-244), host-side (acos + a sort for the
 * median): keep[i] lists the points whose triangulation angle (degrees) is >= min_triang_angle and at most
 * max_ratio_to_median times the median; angles (n, may be NULL) receives every angle. */
int mvo_retain_good_triangulation(const float* pts3d_in_curr, int n, const double* T_w_c_curr, const double* T_w_c_ref,
                                  double min_triang_angle, double max_ratio_to_median, int32_t* keep, int* n_keep,
                                  double* angles);
/* cv::Rodrigues(rvec -> R, 3x3 row-major) as used at vo.cpp:334; host-side. */
int mvo_rodrigues(const double* rvec, double* R);
/* cv::Mat::inv() of a 4x4 double matrix (LU with partial pivoting) -- the T_w_c <-> T_c_w flips at
 * vo.cpp:31,349; host-side.  MVO_ERR_INVALID if singular. */
int mvo_invert_pose(const double* T, double* T_inv);

/* ---- measurement --------------------------------------------------------------------------- */
/* BA launches issued on `device` by this process since the last reset: number of launches, windows solved by them,
 * and the sum of the launch durations (HIP events on the launch stream, milliseconds). */
int mvo_ba_launch_stats(int device, long long* launches, long long* windows, double* ms, int reset);
/* Wall-clock (ms, since the last reset of mvo_ba_launch_stats) the launch thread spent: [0] waiting for work, [1] waiting
 * for a full batch, [2] building + issuing launches, [3] waiting for the kernels, [4] publishing results. */
int mvo_debug_ba_service_times(int device, double* out5);
/* Resident solver service (throughput mode): windows it solved and how often the resident grid was put on the device since
 * the last reset of mvo_ba_launch_stats (those windows count as one launch each there, `ms` = their solve times on the
 * device clock). */
int mvo_debug_ba_resident_stats(int device, long long* windows, long long* grid_starts);
/* Shader-clock cycles the resident grid spent on those windows (sum over the windows, workgroup 0 of each, load to write-back;
 * divided by their `ms` this is the clock the solver ran at under load). */
int mvo_debug_ba_resident_cycles(int device, double* shader_cycles);
/* Times a window that cannot use the resident grid (pose-only, another solver class, rows in LDS only) made the grid leave
 * since the last reset: every such switch drains the 16 slots and relaunches the grid afterwards -- mixed workloads pay for it. */
int mvo_debug_ba_path_switches(int device, long long* n);
/* Test hook: replays the resident solver service's demand estimate (see mvo_ba_set_mode) over n submission times (seconds,
 * ascending); decisions[i] = 1 if a window submitted at times[i] would go to the resident grid.  Returns the number of
 * changes of mind.  Touches no device. */
int mvo_debug_ba_demand_replay(const double* times, int n, uint8_t* decisions);
/* When enabled every kernel launch is bracketed by hipEvents on the ctx stream; times accumulate per
 * kernel name until reset. */
int mvo_profile_enable(mvo_ctx* ctx, int on);
int mvo_profile_reset(mvo_ctx* ctx);
/* Returns the number of distinct kernels; fills up to cap entries. */
typedef struct {
    char name[48];
    int64_t launches;
    double total_ms;
} mvo_kernel_time;
int mvo_profile_get(mvo_ctx* ctx, mvo_kernel_time* out, int cap);

/* ---- debug / test hooks (used by tests/ to localise a parity failure; not part of the drop-in) ---- */
/* key "ba_mfma": 1 (default) = matrix-core contractions, 0 = plain VALU loops computing the same sums;
 * key "ba_wgs": workgroups (CUs) one BA window is split over, 0 (default) = automatic;
 * key "pnp_replay_skew": 1 = the device replays the RANSAC loop with a wrong confidence, so that the host's
 * verification of the selected hypothesis has something to correct (tests only). */
int mvo_debug_set(const char* key, int value);
/* LM trace of the last solve on this ctx (handle == NULL: mvo_bundle_adjustment; else that resident window), after
 * mvo_debug_ba_trace_enable(ctx, 1): one row {lambda the trial was solved with, robust chi2 it reached, gain ratio,
 * accepted} per trial. */
int mvo_debug_ba_trace_enable(mvo_ctx* ctx, int on);
int mvo_debug_get_ba_trace(mvo_ctx* ctx, mvo_ba_handle* handle, double* rows, int cap, int* n);
/* Summation plan of that window: number of landmark ranges (workgroups), column splits of a Schur chain, and the
 * first landmark of every range (wgs + 1 entries) -- what the oracle needs to restate the device sums bit for bit.
 * nsplit: bits 0..15 = the column splits; bits 16.. = K when the window's Schur exchange is grouped (windows of more than
 * 32 workgroups add the partials of the workgroups g = k mod K first -- one XCD each --, then the K group sums), else 0. */
int mvo_debug_get_ba_plan(mvo_ctx* ctx, mvo_ba_handle* handle, int* wgs, int* nsplit, int32_t* wg_pt_start, int cap);
/* Shader-clock cycles the last fetched BA solve spent per phase (ids in csrc/ba_kernels.hip), and the number
 * of workgroups it ran on. */
int mvo_debug_get_ba_phases(mvo_ctx* ctx, long long* cycles, int n, int* wgs);
/* Copies cached pyramid level `level` (raw gray or blurred) WITH its 32-px frame: (h+64) rows of `stride`
 * bytes.  out == NULL only queries the geometry. */
int mvo_debug_get_level(mvo_ctx* ctx, int level, int blurred, uint8_t* out, int cap, int* w, int* h, int* stride);
/* FAST+NMS survivors of the last detection in canonical (level,row,col) order as 16-byte records
 * {int16 x, y; int32 level<<16|fast_score; float harris; float angle}. */
int mvo_debug_get_candidates(mvo_ctx* ctx, void* out, int cap, int* n);
/* The map of the last mvo_undistort_configure (the counterpart of initUndistortRectifyMap inside cv2.undistort,
 * python_tools/undistort_all_images.py:11-37; config/config.yaml:17,39), row-major width x height: source column
 * ix and row iy of the top-left tap and the 1/32 px fractions ax, ay (0..31).  Any output may be NULL.
 * MVO_ERR_STATE without a configuration, MVO_ERR_CAPACITY when cap < width * height. */
int mvo_debug_get_undistort_map(mvo_ctx* ctx, int32_t* ix, int32_t* iy, uint8_t* ax, uint8_t* ay, int cap);

/* Record of the last mvo_solve_pnp_ransac on this ctx: models (iterations x 12: R row-major, t) and inlier
 * counts of every hypothesis, info[6] = {best iteration, iterations the sequential loop would have run,
 * DLT used, LM iterations, LM residual evaluations, hypotheses evaluated (negative when the host had to correct
 * the device's choice of hypothesis)}. */
int mvo_debug_get_pnp(mvo_ctx* ctx, double* models, int32_t* counts, int cap, int32_t* info);

/* Record of the last mvo_find_essential_inliers on this ctx: inlier counts of every evaluated hypothesis
 * (iterations x 10 candidates, -1 = no such candidate), info[5] = {best iteration, best candidate, iterations
 * the sequential loop ran, iterations evaluated, 0}.  Returns the number of evaluated iterations. */
int mvo_debug_get_essential(mvo_ctx* ctx, int32_t* counts, int cap_iters, int32_t* info);

/* Record of the last mvo_find_homography on this ctx: the inlier count of every evaluated hypothesis (-1 = runKernel
 * found no model), info[6] = {selected iteration (-1: none), iterations the sequential loop ran, iterations
 * evaluated, subsets drawn before getSubset gave up (2000 when it never did), LM iterations, DLT re-fit on the
 * inliers used}.  Returns the number of evaluated iterations. */
int mvo_debug_get_homography(mvo_ctx* ctx, int32_t* counts, int cap_iters, int32_t* info);

/* Record of the last mvo_esti_motion_by_essential on this ctx (zeros and chosen = -1 when it found no model):
 * good[4] = recoverPose's counts for (R1, t), (R2, t), (R1, -t), (R2, -t); chosen = the index picked (0..3);
 * R1R2t = R1 (9), R2 (9), t (3) of decomposeEssentialMat; masks[i] bit k set when match i passes combination k
 * and the RANSAC mask.  Returns n (the number of masks). */
int mvo_debug_get_recover_pose(mvo_ctx* ctx, int32_t* good, int32_t* chosen, double* R1R2t, uint8_t* masks, int cap);
/* Record of the last homography decomposition (mvo_esti_motion_by_homography or mvo_estimate_possible_relative_poses
 * on this ctx): Hn (9) after its 1 / w[1] scaling, w (3, descending), branch[2] = {1 for the rotation-only branch
 * else 0, the index of the largest |S_ii| or -1}, the raw candidates Rs (4 x 9), ts (4 x 3, before t / |t|), normals
 * (4 x 3) and rejected[4], the number of H inliers that reject each candidate (a candidate survives at 0).  Returns
 * the number of candidates: 0 when there was no H, 1 for the rotation-only branch, else 4. */
int mvo_debug_get_homography_decomposition(mvo_ctx* ctx, double* Hn, double* w, int32_t* branch, double* Rs,
                                           double* ts, double* normals, int32_t* rejected);
/* Record of the last mvo_init_two_view on this ctx, what k_init_finish wrote for every entry of the chosen slot's
 * inlier list, in list order: p_curr (n x 3 float, before the keep rule and the scaling), cosang (the cosine of the
 * triangulation angle) and pixdist (basics::calcDist of the match's two pixels).  Any buffer may be NULL; *n receives
 * the number of entries (0 after a call with best == -1). */
int mvo_debug_get_init_finish(mvo_ctx* ctx, float* p_curr, double* cosang, double* pixdist, int cap, int* n);

#ifdef __cplusplus
}
#endif
#endif
