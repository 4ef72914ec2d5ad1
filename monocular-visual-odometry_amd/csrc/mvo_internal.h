// csrc/mvo_internal.h -- context, device buffers and launch plumbing shared by the HIP translation units.
#ifndef MVO_INTERNAL_H
#define MVO_INTERNAL_H
#include <hip/hip_runtime.h>
#include <stdint.h>

// The dynamic LDS segment of a kernel and kernel-only attributes.  tests/sim compiles the kernel SOURCES for the host against an
// emulation of the HIP runtime (a test aid: MVO_KERNEL_SIM is defined by its stand-in for <hip/hip_runtime.h>, the library has
// no CPU path); there the segment comes from the emulated launch and the attributes mean nothing.
#ifndef MVO_KERNEL_SIM
#define MVO_DYN_LDS(T, name) extern __shared__ T name[]
#define MVO_DYN_LDS_ALIGNED16(T, name) extern __shared__ __attribute__((aligned(16))) T name[]
#define MVO_WAVES_PER_EU(lo, hi) __attribute__((amdgpu_waves_per_eu(lo, hi)))
#define MVO_WAIT_VM0() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")  // this wave's global stores have left for memory
// the value of a 32-bit vector register is taken as unknown from here on: keeps loop-invariant unpacking / address arithmetic
// INSIDE a loop (hoisted, a dozen packed table entries become three dozen live registers)
#define MVO_OPAQUE(x) asm volatile("" : "+v"(x))
#else
#define MVO_DYN_LDS(T, name) T* name = static_cast<T*>(emu_dyn_lds())
#define MVO_DYN_LDS_ALIGNED16(T, name) T* name = static_cast<T*>(emu_dyn_lds())
#define MVO_WAVES_PER_EU(lo, hi)
#define MVO_WAIT_VM0() __atomic_thread_fence(__ATOMIC_SEQ_CST)
#define MVO_OPAQUE(x) (void)(x)
#endif

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <atomic>
#include <string>
#include <vector>

#include "../../include/mvo_hip.h"

struct mvo_ctx;
int mvo_set_err(mvo_ctx* c, int code, const char* what, hipError_t e);
#define MVO_HIP(call)                                                            \
    do {                                                                         \
        hipError_t e__ = (call);                                                 \
        if (e__ != hipSuccess) {                                                 \
            (void)hipGetLastError(); /* clear the sticky error */                \
            return mvo_set_err(ctx, MVO_ERR_HIP, #call, e__);                    \
        }                                                                        \
    } while (0)

// hipFree / hipHostFree with the resident solver grid of `device` taken off first (both synchronise with every stream of the
// device; the grid never ends on its own)
void ba_service_free(int device, void* p, bool host);
inline void mvo_free_on_current_device(void* p) {
    int d = 0;
    (void)hipGetDevice(&d);
    ba_service_free(d, p, false);
}

// One grow-on-demand device buffer: a pointer and its capacity in elements, owned once.  release() frees through
// mvo_free_on_current_device, so an owner is destroyed only on the paths that have made ctx->device current: mvo_destroy,
// which resets the per-feature states of mvo_ctx, and mvo_map_release.  Neither ensure preserves the contents.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;  // elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    operator T*() const { return p; }
    void release() {
        if (p) mvo_free_on_current_device(p);
        p = nullptr;
        cap = 0;
    }
    // room for exactly n elements plus pad_bytes: the fixed-size buffers and the image staging
    int ensure_exact(mvo_ctx* ctx, size_t n, size_t pad_bytes = 0) {
        if (n <= cap) return MVO_OK;
        release();
        void* q = nullptr;
        MVO_HIP(hipMalloc(&q, n * sizeof(T) + pad_bytes));
        p = static_cast<T*>(q);  // (pointer and capacity are set only once the allocation stands)
        cap = n;
        return MVO_OK;
    }
    // room for n elements, max(floor, n + n / 2) when it grows: everything sized by a count of matches or points
    int ensure(mvo_ctx* ctx, size_t n, size_t floor) { return n <= cap ? MVO_OK : ensure_exact(ctx, std::max(floor, n + n / 2)); }
};

#define MVO_MAX_LEVELS 8
#define MVO_BORDER 32  // ORB: max(edgeThreshold 31, descPatchSize 22, HARRIS_BLOCK/2) + 1

// One pyramid level inside the device pyramid buffers (raw, blurred share the geometry).
struct LevelInfo {
    int w, h;        // interior size
    int stride;      // bytes per bordered row, multiple of 64
    int off;         // byte offset of bordered row 0 inside the pyramid buffer
    int tiles_x;     // 64-px-wide NMS cell columns (FAST tiles are 64 x 16 interior pixels)
    int tiles_y;
    int tile_off;    // first FAST tile of this level in the flattened tile list
    int cell_off;    // first (row, tile column) cell of this level in the cell arrays
    int btiles_x;    // blur tiles (64 x 16) over the bordered extent
    int btiles_y;
    int btile_off;
    int tab_off;     // offset of this level's resize tables: [x entries w][y entries h]
    float scale;     // layerScale[level]
};
struct PyrInfo {
    int nlevels;
    int n_cells;
    int n_tiles;
    int n_btiles;
    LevelInfo lv[MVO_MAX_LEVELS];
};

// FAST+NMS survivor as the device emits it (16 bytes), canonical order: level, row, column.
struct DevCandidate {
    int16_t x, y;
    int32_t level_score;  // level << 16 | fast score
    float harris;
    float angle;
};
// Keypoint as uploaded for the rBRIEF kernel.
struct DevDescKp {
    int16_t cx, cy;  // cvRound(pt * 1/scale) in level coordinates
    int32_t level;
    float a, b;  // cos / sin of the keypoint angle, computed on the host
};
struct ResizeEntry {
    int32_t ofs;
    int16_t c0, c1;
};

// Pyramid kernel (k_pyramid): 64 x 16 output tiles; the source regions of a tile, level by level down to the base of
// its level group, are staged in LDS.  pyr_regions() is the one statement of that footprint arithmetic: the device
// uses it per tile, the host uses it to check that every tile of a group fits PYR_LDS_BYTES (otherwise the group runs
// the per-pixel chain kernel).
#define PT_W 64
#define PT_H 16
#define PYR_LDS_BYTES 32768
struct PyrRegion {
    int x0, y0, w, h;  // interior coordinates of its level
};
#ifdef __HIPCC__
#define MVO_HD __host__ __device__
#else
#define MVO_HD
#endif
// reg[d] (d = 1 .. depth) = region of level l-d needed for the interior box [xlo, xhi] x [ylo, yhi] of level l;
// off[d] = its byte offset in the LDS pool.  Returns the pool bytes used.
MVO_HD inline int pyr_regions(const PyrInfo& P, const ResizeEntry* tabs, int l, int depth, int xlo, int xhi, int ylo,
                              int yhi, PyrRegion* reg, int* off) {
    int used = 0;
    for (int d = 1; d <= depth; ++d) {
        const int m = l - d + 1;  // destination level of this step; the region lives on level m-1
        const ResizeEntry* tx = tabs + P.lv[m].tab_off;
        const ResizeEntry* ty = tx + P.lv[m].w;
        const int sw = P.lv[m - 1].w, sh = P.lv[m - 1].h;
        const int x0 = tx[xlo].ofs, x1 = tx[xhi].ofs + 1 < sw - 1 ? tx[xhi].ofs + 1 : sw - 1;
        const int y0 = ty[ylo].ofs, y1 = ty[yhi].ofs + 1 < sh - 1 ? ty[yhi].ofs + 1 : sh - 1;
        reg[d].x0 = x0;
        reg[d].y0 = y0;
        reg[d].w = x1 - x0 + 1;
        reg[d].h = y1 - y0 + 1;
        off[d] = used;
        used += (reg[d].w * reg[d].h + 15) & ~15;
        xlo = x0, xhi = x1, ylo = y0, yhi = y1;
    }
    return used;
}

// The regions of one tile as orb_setup_geometry works them out once per image geometry (the tile grid of a pyramid never
// changes between frames): k_pyramid reads its entry instead of deriving it -- a serial chain of dependent table look-ups on ONE
// thread in front of every deep tile.  128 bytes per bordered tile.
struct PyrTileRegs {
    PyrRegion reg[5];  // [1 .. depth]
    int off[5];
    int pad[7];
};
static_assert(sizeof(PyrTileRegs) == 128, "one 128-byte line per tile");

// k_fast_harris output: every 64 x 16 tile owns FT_TILE_CAP record slots (3x3 NMS leaves at most one survivor per
// 2 x 2 pixels: 256 per tile) and one count, in pinned host memory
#define FT_TILE_CAP 256
#define FT_ROW_TILES 128  // tiles per tile row the in-kernel ordering handles (images up to 8192 px wide)
inline size_t orb_detect_counts_bytes(int n_tiles) { return ((size_t)n_tiles * 4 + 63) / 64 * 64; }
inline size_t orb_detect_host_bytes(int n_tiles) {
    return orb_detect_counts_bytes(n_tiles) + (size_t)n_tiles * FT_TILE_CAP * sizeof(DevCandidate);
}

// tracking rows (track_kernels.hip / track_host.cpp)
struct TrackCamera {
    double fx, fy, cx, cy;
};
struct InitScoreArgs {  // k_init_scores: F21, H21, H12 (row-major), 1 / sigma^2, which models exist
    double f[9], h[9], hi[9];
    double inv_s2;
    int has_e, has_h;
};
// k_h_decompose's double output (hd_wave.h, track_host.cpp)
constexpr int kHdHs = 0;   // H * (1 / H(2,2)), 9
constexpr int kHdHn = 9;   // Hn after the 1 / w[1] scaling, 9
constexpr int kHdW = 18;   // singular values of (K^-1 H) K, 3
constexpr int kHdR = 21;   // R of the 4 raw candidates, 4 x 9
constexpr int kHdT = 57;   // t of the 4 raw candidates (before normalisation), 4 x 3
constexpr int kHdN = 69;   // n of the 4 raw candidates, 4 x 3
constexpr int kHdTn = 81;  // t / |t| of the 4 candidates, 4 x 3
constexpr int kHdOut = 93;
// its int output: [0..3] rejecting matches per candidate, [4] arrivals (both zeroed by the launch), [5] number of
// candidates (1: rotation-only, 4: general), [6] branch (-1: rotation-only, else the index of the largest |S_ii|),
// [7] number of survivors, [8..11] their indices in candidate order
constexpr int kHdCnt = 12;
struct TrackViewArgs {
    double T[12];  // rows 0..2 of T_c_w = inv(T_w_c)
    double fx, fy, cx, cy;
    int cols, rows;
};
struct mvo_track_state;  // device buffers of the tracking rows, allocated on first use
struct mvo_map {  // the resident map (mvo_map_*, track_host.cpp): n x 3 f32 positions, n x 32 descriptor bytes
    DevBuf<float> d_pos;
    DevBuf<uint8_t> d_desc;
    int n = 0;
    // the view data of the points (mvo_map_upload_view, local_map_host.cpp): n x 3 f32 mean normals, n f32 largest distances
    DevBuf<float> d_normal, d_max_dist;
    bool has_view = false;  // given since the last mvo_map_upload
};

// undistortion (undistort_kernels.hip / undistort_host.cpp)
struct UndistortArgs {  // k_undistort_map: the model with 1 / fx, 1 / fy taken on the host, missing coefficients 0
    double fx, fy, cx, cy, ifx, ify;
    double k1, k2, p1, p2, k3, k4, k5, k6;
};
// k_undistort_map's record of one output pixel, 8 bytes: iu = cvRound(u * 32), iv = cvRound(v * 32).  The integer
// coordinate is the arithmetic shift iu >> 5, the 1/32 px fraction iu & 31.
struct UndistortRec {
    int32_t iu, iv;
};
struct mvo_undistort_state {  // mvo_ctx::undist, used by undistort_host.cpp
    bool configured = false;
    mvo_undistort_params params{};  // as configured, coefficients beyond n_coeffs zeroed
    int w = 0, h = 0;
    DevBuf<UndistortRec> d_map;
    DevBuf<uint8_t> d_src, d_dst;  // staging of the host-pointer form
};

// what the pose-gated matchers share (guided_knn2.h: the kernel body; guided_match_host.h: the host tail)
#define GK_MAX_GROUPS 8  // train groups of guided_knn2() (workgroups per group of 64 queries)
struct GuidedPartials {  // the scratch as the kernels take it
    unsigned long long* key;  // GK_MAX_GROUPS x nq partial key pairs
    int32_t *cnt, *arrive;    // as many partial counts; one arrival counter per group of 64 queries
};
struct GuidedScratch {  // one per matcher; keys, counts and counters are one allocation (methods: guided_match_host.h)
    DevBuf<uint8_t> buf;
    unsigned long long* d_part = nullptr;  // views into buf
    int32_t *d_part_cnt = nullptr, *d_arrive = nullptr;
    int cap = 0;  // queries
    int ensure(mvo_ctx* ctx, int n);  // room for n queries: max(4096, 1.5 n) when it grows, the counters zeroed on ctx->stream
    void release();
    GuidedPartials partials() const { return {d_part, d_part_cnt, d_arrive}; }
};
struct FrameScratch {  // the same for the launches over every buffered frame: map fusion, window triangulation (method: guided_match_host.h)
    DevBuf<uint8_t> d_part;    // partial key pairs, then the partial counts: one block per frame
    DevBuf<int32_t> d_arrive;  // arrival counters, one per (frame, group of 64 queries): self re-arming, zeroed when allocated
    size_t keys_b = 0;         // bytes of the key pairs of the last ensure
    // rows_all = frames x queries, n_arrive = frames x groups of 64 queries
    int ensure(mvo_ctx* ctx, size_t rows_all, int ngroups, size_t n_arrive);
    GuidedPartials partials() const {
        return {reinterpret_cast<unsigned long long*>(d_part.p), reinterpret_cast<int32_t*>(d_part.p + keys_b), d_arrive.p};
    }
};

// pose-guided matching (epipolar_kernels.hip / epipolar_host.cpp)
struct EpipolarArgs {  // k_knn2_epipolar: F row-major, x2^T F x1 = 0
    double f[9];
};
struct mvo_epipolar_state {  // mvo_ctx::epi, used by epipolar_host.cpp
    DevBuf<uint8_t> d_q, d_t;  // staging of the host-pointer form
    DevBuf<float> d_qxy, d_txy;
    DevBuf<double> d_tol2;
    GuidedScratch scratch;
};

// tracking by projection (projection_kernels.hip / projection_host.cpp)
struct mvo_projection_state {  // mvo_ctx::proj, used by projection_host.cpp
    DevBuf<uint8_t> d_t;  // staging of the host-pointer form
    DevBuf<double> d_tg;  // nt x ((double)x, (double)y, r2): the gate's view of the frame keypoints
    GuidedScratch scratch;
};

// cell-wise FAST + quadtree spread (orb_distribute_kernels.hip / orb_distribute_host.cpp)
#define DC_MAX_CELL_SIZE 32                        // cell_size W: wCell, hCell <= 2 W - 1 = 63 -> one 64-bit ballot per cell row
#define DC_MAX_SCORED (2 * DC_MAX_CELL_SIZE - 1)   // scored pixels of a cell per direction
struct DistCell {  // one cell of k_fast_cells, made once per image geometry (32 bytes)
    int32_t x0, y0;  // iniX, iniY in level coordinates: the origin of the staged patch
    int32_t pw, ph;  // staged patch: maxXc - iniX, maxYc - iniY; the scored pixels are [3, pw - 3) x [3, ph - 3) of it
    int32_t level;
    int32_t slot;    // first record of the cell's slot in the pinned buffer
    int32_t cap;     // ceil(sw / 2) * ceil(sh / 2): the most strict 3 x 3 maxima sw x sh scored pixels can hold
    int32_t pad;
};
struct DistRecord {  // a survivor as k_fast_cells emits it and a kept point as k_ic_angle reads it (8 bytes)
    int16_t x, y;         // level coordinates
    int32_t level_score;  // level << 16 | FAST score
};
struct DistLevel {  // step 1 / step 6 geometry of a level
    int minX, minY, width, height;
    int cell0, ncells;  // its cells in the table (cell row, cell column order)
};
struct mvo_orb_distribute_state {  // mvo_ctx::dist, used by orb_distribute_host.cpp
    mvo_orb_distribute_params params{20, 7, 30, 19};
    // what the cell table below was made for
    bool made = false;
    mvo_orb_params made_orb{};
    mvo_orb_distribute_params made_params{};
    int made_w = 0, made_h = 0;
    std::vector<DistCell> cells;
    DistLevel lv[MVO_MAX_LEVELS] = {};
    size_t n_records = 0;  // sum of the slot capacities
    int kp_cap = 0;        // most key points a frame can keep (quota + 2 per level, or the initial nodes)
    DevBuf<DistCell> d_cells;
    DevBuf<signed char> d_disc;  // (u, v) of the 749 pixels of the IC-angle disc
    int disc_n = 0;
    std::vector<mvo_distribute_candidate> last_cand;  // step 5 of the last call (debug getter)
};

// map points refreshed from their observations (map_refresh_kernels.hip / map_refresh_host.cpp)
#define MR_MAX_OBS 64  // observations per map point: one lane each
struct mvo_refresh_state {  // mvo_ctx::refresh, used by map_refresh_host.cpp
    DevBuf<uint8_t> d_in;  // one upload per call: the camera centres, the descriptors, the n + 1 starts
};

// map point positions refined from all their observations (map_refine_kernels.hip / map_refine_host.cpp)
#define MF_MAX_FRAMES 64  // poses per call: 12 doubles each in LDS
struct MapRefineArgs {
    double fx, fy, cx, cy;
    double delta, rel_tol;  // huber_delta, rel_tolerance
    int32_t max_trials, min_obs, n_frames;
};
struct mvo_refine_state {  // mvo_ctx::refine, used by map_refine_host.cpp
    DevBuf<uint8_t> d_in;  // one upload per call: the inverted poses, the pixels, the frame indices, the n + 1 starts
};

// duplicate map points fused over the buffered frames (map_fuse_kernels.hip / map_fuse_host.cpp)
struct MapFuseArgs {
    double fx, fy, cx, cy;
    int cols, rows;
};
struct MapFuseFrame {  // one row of k_map_fuse_search's per-frame table, read from HBM (128 bytes)
    double T[12];      // rows 0..2 of T_c_w = inv(T_w_c)
    const uint4* t;    // nt x 32 descriptor bytes
    const double* tg;  // nt x ((double)x, (double)y, r2), r2 = -1.0 for a keypoint that never passes
    int32_t nt, slice; // slice = guided_slice(nt, the launch's train groups)
    int32_t pad[2];
};
struct mvo_fuse_state {  // mvo_ctx::fuse, used by map_fuse_host.cpp
    DevBuf<uint8_t> d_in;  // one upload per call: the frame table, the seen masks, the parked keypoints, the descriptors
    FrameScratch scratch;  // queries: the map points
};

// new map points triangulated against every buffered frame (window_triangulate_kernels.hip / window_triangulate_host.cpp;
// DESIGN.md section 20)
struct WindowFrame {   // one row of the per-frame table of k_window_epipolar_search and k_window_verify, read from HBM (200 bytes)
    double F[9];       // mvo_fundamental_from_poses(curr, frame): the line of a keypoint of curr in the frame
    double R[9], tr[3];  // M = inv(T_w_c_curr) T_w_c_frame: frame coordinates -> coordinates of curr
    const uint4* d;    // nt x 32 descriptor bytes
    const double* tg;  // nt x ((double)u, (double)v, tol2), tol2 = -1.0 for a keypoint that is not free
    int32_t nt, slice; // slice = guided_slice(nt, the launch's train groups)
    int32_t active;    // the baseline test
    int32_t pad;
};
struct WindowPairIn {  // one pair as k_window_verify reads it (32 bytes)
    int32_t frame, pad;
    float uf, vf, uc, vc;  // the keypoint of the frame, the keypoint of curr
    float sf, sc;          // their scales (1 without scales)
};
struct WindowPairOut {  // ... and as it delivers it (40 bytes)
    float p_curr[3], p_frame[3];
    double cos2;
    int32_t status, pad;
};
struct WindowVerifyArgs {
    double fx, fy, cx, cy;
    double c2max, chi2, rf2;  // max_cos_parallax^2, max_reproj_chi2, ratio_factor^2
};
struct mvo_window_state {  // mvo_ctx::window, used by window_triangulate_host.cpp
    DevBuf<uint8_t> d_in;  // one upload per call: the frame table, curr (free flags, pixels, descriptors), the frames' keypoints
    FrameScratch scratch;  // queries: the keypoints of curr
    DevBuf<WindowPairIn> d_pairs;  // the small upload in front of the verification
};

// the per-frame pose from a robust motion-only optimisation (pose_optimize_kernels.hip / pose_optimize_host.cpp)
#define PO_MAX_OBS 4096  // observations per call: 24 bytes each in LDS, 16 per lane
#define PO_MAX_ROUNDS 8
struct PoseOptArgs {
    double T0[12];  // rows 0..2 of T_c_w^0
    double fx, fy, cx, cy;
    double delta, chi2_thr, rel_tol;  // huber_delta, chi2_threshold, rel_tolerance
    int32_t rounds, iterations, min_inliers, has_sigma;
};
struct PoseOptOut {  // what k_pose_optimize writes into the ctx's pinned staging, the n flags behind it
    double Tcw[12];
    double chi2[2];
    double rows[PO_MAX_ROUNDS * 6];
    int32_t info[6];
    int32_t pad[2];
};
struct mvo_pose_opt_state {  // mvo_ctx::pose_opt, used by pose_optimize_host.cpp
    DevBuf<uint8_t> d_in;    // one upload per call: pts3d, pts2d, inv_sigma2
    int n_rounds = 0;        // rows of the last call that launched (mvo_debug_get_pose_optimize)
    double rows[PO_MAX_ROUNDS * 6] = {0};
};

// the local map tracked from the optimised pose (local_map_kernels.hip / local_map_host.cpp)
#define LM_MAX_LEVELS 16
struct LocalMapArgs {  // k_map_match_local: everything but the arrays travels in the kernel arguments
    TrackViewArgs view;
    double O[3];                         // the camera centre, T_w_c[4 r + 3]
    double level_scale[LM_MAX_LEVELS];   // entries behind n_levels repeat the last one
    double min_view_cos, radius_near, radius_far, near_cos, radius_scale;
    int32_t n_levels, pad;
};
struct mvo_local_map_state {  // mvo_ctx::local_map, used by local_map_host.cpp
    DevBuf<uint8_t> d_in;  // one upload per call: the parked keypoints, the skip mask, the descriptors of the host-pointer form
    GuidedScratch scratch;
};

struct ProfEntry {
    int64_t launches = 0;
    double ms = 0;
};

// Admission gate of the extraction / matching launches of THROUGHPUT-mode contexts (many sequences share the GPU): at most
// `g_extract_concurrency` such launch-and-wait sections are in flight per device (0 = no limit).  The kernels of a frame run on
// the CUs the resident solver grid leaves free; their combined throughput DROPS when too many frames interleave there
// (round 4: 14 frames at once -> 3400 frames/s of extraction, 8-9 at once -> 4600), so the excess waits at the door.
extern std::atomic<int> g_extract_concurrency;
struct ExtractGate {
    int device = -1;
    explicit ExtractGate(const mvo_ctx* ctx);
    ~ExtractGate() { release(); }
    void release();
    ExtractGate(const ExtractGate&) = delete;
    ExtractGate& operator=(const ExtractGate&) = delete;
};

inline unsigned long long mvo_next_ctx_uid() {
    static std::atomic<unsigned long long> n{0};
    return ++n;
}
struct mvo_ctx {
    unsigned long long uid = mvo_next_ctx_uid();  // mvo_ctx_uid: never reused
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = true;  // false: a sibling ctx on its parent's stream (mvo_create_sibling)
    std::string err;
    // --- ORB
    mvo_orb_params orb{};
    bool orb_configured = false;
    int grid_rows = 0, grid_cols = 0;  // latched from the first image
    int img_w = 0, img_h = 0;
    PyrInfo pyr{};
    std::vector<int> quota;
    bool pyr_valid = false, blur_valid = false;
    bool pyr_group_tiled[MVO_MAX_LEVELS] = {false};  // per level group: every tile's regions fit the LDS pool
    int pyr_group_lds[MVO_MAX_LEVELS] = {0};         // ... and the bytes of it the hungriest tile of the group needs
    int pyr_levels_built = 0;
    DevBuf<uint8_t> d_img;  // image staging of the host-pointer forms (mvo_stage_image)
    uint8_t *d_raw = nullptr, *d_blur = nullptr;
    size_t pyr_bytes = 0;
    ResizeEntry* d_tabs = nullptr;
    PyrTileRegs* d_pyr_regs = nullptr;  // per bordered tile: the source regions of k_pyramid (orb_setup_geometry)
    // k_fast_harris: per-tile record slots + line counts in device memory, arrival counter per tile row (self re-arming)
    void* d_fh_slots = nullptr;
    void* d_fh_line = nullptr;
    int32_t* d_fh_arrive = nullptr;
    std::vector<DevCandidate> last_cand;  // canonical candidate list of the last detection (debug getter)
    DevDescKp* d_kp = nullptr;
    uint8_t* d_desc = nullptr;      // descriptors of the current extraction (one of the two halves below)
    uint8_t* d_desc_buf = nullptr;  // 2 x kp_cap x 32: ping-pong so that frame i-1 survives frame i
    int desc_flip = 0;
    int kp_cap = 0;
    // pinned host staging
    uint8_t* h_pin = nullptr;
    size_t h_pin_cap = 0;
    hipEvent_t ev = nullptr;
    // --- matcher
    DevBuf<uint8_t> d_mq, d_mt;
    DevBuf<float> d_mqxy, d_mtxy;
    DevBuf<int32_t> d_mout;
    int32_t* d_marrive = nullptr;  // k_knn2 arrival counters (inside the d_mout allocation)
    // --- tracking rows
    mvo_track_state* track = nullptr;
    // record of the last mvo_init_two_view (init_host.cpp; mvo_debug_get_init_finish)
    bool init_called = false;
    std::vector<float> init_p_curr;
    std::vector<double> init_cosang, init_pixdist;
    // --- per-feature state, each made by the first call of its feature (mvo_state) and reset by mvo_destroy: undistortion,
    // pose-guided matching, tracking by projection, cell-wise FAST + quadtree spread, map points refreshed from / refined over
    // their observations, duplicate map points fused, new map points triangulated against the buffered frames, the pose from
    // a robust motion-only optimisation, the local map tracked from the optimised pose
    std::unique_ptr<mvo_undistort_state> undist;
    std::unique_ptr<mvo_epipolar_state> epi;
    std::unique_ptr<mvo_projection_state> proj;
    std::unique_ptr<mvo_orb_distribute_state> dist;
    std::unique_ptr<mvo_refresh_state> refresh;
    std::unique_ptr<mvo_refine_state> refine;
    std::unique_ptr<mvo_fuse_state> fuse;
    std::unique_ptr<mvo_window_state> window;
    std::unique_ptr<mvo_pose_opt_state> pose_opt;
    std::unique_ptr<mvo_local_map_state> local_map;
    // --- BA diagnostics of the last fetched solve
    long long ba_phase[16] = {0};
    int ba_wgs = 0, ba_trials = 0;
    int ba_throughput_mode = 0;  // mvo_ba_set_mode: 0 = latency (default), 1 = throughput (fewer, fuller workgroups per window)
    bool ba_never_resident = false;  // MVO_BA_MODE_SHARED: throughput cut, launch path only
    struct mvo_ba_pool* ba_pool = nullptr;  // pooled BA workspaces (ba_host.cpp)
    // --- profiling
    bool prof = false;
    std::map<std::string, ProfEntry> prof_acc;
    std::vector<std::pair<std::string, std::pair<hipEvent_t, hipEvent_t>>> prof_pending;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_pool;
};
// a per-feature state of mvo_ctx, made on first use
template <class State>
State* mvo_state(std::unique_ptr<State>& p) {
    if (!p) p.reset(new State());
    return p.get();
}

// profiling brackets
void mvo_prof_begin(mvo_ctx* c, const char* name);
void mvo_prof_end(mvo_ctx* c);
void mvo_prof_collect(mvo_ctx* c);
struct ProfScope {
    mvo_ctx* c;
    ProfScope(mvo_ctx* c_, const char* name) : c(c_) {
        if (c->prof) mvo_prof_begin(c, name);
    }
    ~ProfScope() {
        if (c->prof) mvo_prof_end(c);
    }
};

// MVO_HOST_TIMING=1: per-stage wall clock of the host half (printed every 200 frames to stderr; development aid)
struct HostTimes {
    double acc[8] = {0};
    long n = 0;
    std::chrono::steady_clock::time_point t;
    bool on = std::getenv("MVO_HOST_TIMING") != nullptr;
    void start() {
        if (on) t = std::chrono::steady_clock::now();
    }
    void lap(int k) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        acc[k] += std::chrono::duration<double, std::micro>(now - t).count();
        t = now;
    }
    void frame(const char* const* names, int cnt) {
        if (!on || ++n % 200) return;
        std::fprintf(stderr, "[mvo host us/frame]");
        for (int k = 0; k < cnt; ++k) std::fprintf(stderr, " %s %.1f", names[k], acc[k] / 200), acc[k] = 0;
        std::fprintf(stderr, "\n");
    }
};

int mvo_ensure_pinned(mvo_ctx* ctx, size_t bytes);
// h rows of `stride` bytes from the host into ctx->d_img, on ctx->stream (mvo_api.cpp)
int mvo_stage_image(mvo_ctx* ctx, const uint8_t* img, int h, int stride);

// orb_kernels.hip
int orb_launch_pyramid(mvo_ctx* ctx, const uint8_t* d_img, int stride, int channels, int nlevels);
int orb_launch_detect(mvo_ctx* ctx, uint8_t* host, bool ordered);
int orb_launch_blur(mvo_ctx* ctx, int nlevels);
bool orb_brief_from_levels(const mvo_ctx* ctx);
int orb_launch_brief(mvo_ctx* ctx, int n, const DevDescKp* kps, uint8_t* desc_host);
// match_kernels.hip
int match_launch_knn2(mvo_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int32_t* d_out,
                      int32_t* final_out);
int match_launch_radius_l1(mvo_ctx* ctx, const uint8_t* d_q, const float* d_qxy, int nq, const uint8_t* d_t,
                           const float* d_txy, int nt, float max_px, int32_t* d_out);
// track_kernels.hip
int track_launch_map_in_view(mvo_ctx* ctx, const float* d_pos, const uint8_t* d_desc, int n, const TrackViewArgs& a,
                             int32_t* d_idx, float* d_px, uint8_t* d_desc_out, int32_t* d_n);
int track_launch_pnp_hypotheses(mvo_ctx* ctx, const float* d_p3, const float* d_p2, int n, const int32_t* d_subsets,
                                int n_hyp, const TrackCamera& cam, float thr2, double* d_models, int32_t* d_counts,
                                uint8_t* d_masks, double* h_models, int32_t* h_counts);
int track_launch_pnp_refine(mvo_ctx* ctx, const float* d_p3, const float* d_p2, const uint8_t* d_masks, int n,
                            const TrackCamera& cam, const double* d_models, const int32_t* d_counts, int n_hyp,
                            double confidence, int forced_best, int mode, double* d_Mg, double* d_mg,
                            uint8_t* d_best_mask, double* d_out);
int track_launch_triangulate(mvo_ctx* ctx, const float* d_kp1, const float* d_kp2, int n, const TrackCamera& cam,
                             const double* R, const double* t, float* d_prev, float* d_curr);
int track_launch_em_hypotheses(mvo_ctx* ctx, const double* d_q1, const double* d_q2, int n, const int32_t* d_subsets,
                               int n_hyp, float thr2, double* d_E, int32_t* d_nm, int32_t* d_counts);
int track_launch_em_mask(mvo_ctx* ctx, const double* d_q1, const double* d_q2, int n, const double* d_E, float thr2,
                         uint8_t* d_mask);
int track_launch_h_hypotheses(mvo_ctx* ctx, const float* d_src, const float* d_dst, int n, const int32_t* d_subsets,
                              int n_hyp, float thr2, double* d_H, int32_t* d_counts);
int track_launch_h_mask(mvo_ctx* ctx, const float* d_src, const float* d_dst, int n, const double* d_H, float thr2,
                        uint8_t* d_mask);
int track_launch_h_refine(mvo_ctx* ctx, const float* d_src, const float* d_dst, const uint8_t* d_mask, int n,
                          const double* d_H, double* d_out);
int track_launch_recover_pose(mvo_ctx* ctx, const double* d_q1, const double* d_q2, int n, const double* d_E,
                              const uint8_t* d_ransac_mask, uint8_t* d_masks, int32_t* d_cnt, double* d_out);
int track_launch_init_scores(mvo_ctx* ctx, const float* d_kp1, const float* d_kp2, const int32_t* d_lists, int n_e,
                             int n_h, const InitScoreArgs& a, double* d_scores, int32_t* d_kept, int32_t* d_n_kept);
int track_launch_h_decompose(mvo_ctx* ctx, const float* d_kp1, const float* d_kp2, const uint8_t* d_mask, int n,
                             const double* d_H, const TrackCamera& cam, int32_t* d_cnt, double* d_out);
int track_launch_init_triangulate(mvo_ctx* ctx, const float* d_kp1, const float* d_kp2, int n, const TrackCamera& cam,
                                  const double* d_e_out, const uint8_t* d_e_mask, const double* d_h_out,
                                  const int32_t* d_h_cnt, const uint8_t* d_h_mask, float* d_pts);
int track_launch_init_finish(mvo_ctx* ctx, const float* d_pts, const int32_t* d_list, int m, const double* d_R,
                             const double* d_t, const float* d_kp1, const float* d_kp2, const double* T_w_c_curr,
                             const double* T_w_c_ref, float* d_p_curr, double* d_cosang, double* d_pixdist);
// undistort_kernels.hip
int undistort_launch_map(mvo_ctx* ctx, const UndistortArgs& a, int w, int h, UndistortRec* d_map);
int undistort_launch_remap(mvo_ctx* ctx, const UndistortRec* d_map, const uint8_t* d_src, int w, int h, int stride,
                           int channels, uint8_t* d_out, int out_stride);
// epipolar_kernels.hip
int epipolar_launch_knn2(mvo_ctx* ctx, const uint8_t* d_q, const float* d_qxy, int nq, const uint8_t* d_t, const float* d_txy,
                         const double* d_tol2, int nt, const EpipolarArgs& a, GuidedPartials part, int32_t* out);
// projection_kernels.hip
int projection_launch(mvo_ctx* ctx, const float* d_pos, const uint8_t* d_desc, int n_map, const TrackViewArgs& a, const uint8_t* d_t,
                      const double* d_tg, int nt, GuidedPartials part, int32_t* out);
// orb_distribute_kernels.hip
int dist_launch_cells(mvo_ctx* ctx, const DistCell* d_cells, int n_cells, int thr_min, int thr_ini, int32_t* counts,
                      DistRecord* records);
int dist_launch_ic_angle(mvo_ctx* ctx, const signed char* d_disc, int disc_n, const DistRecord* kps, int n, float* angles);
// map_refresh_kernels.hip
int map_refresh_launch(mvo_ctx* ctx, const float* d_pos, uint8_t* d_desc, int n, const uint8_t* d_obs_desc, const double* d_obs_cam,
                       const int32_t* d_obs_start, int32_t* out_choice, uint8_t* out_desc, double* out_norm);
// map_refine_kernels.hip
int map_refine_launch(mvo_ctx* ctx, float* d_pos, int n, const MapRefineArgs& a, const double* d_Tcw, const float* d_uv,
                      const int32_t* d_frame, const int32_t* d_obs_start, float* out_pos, double* out_chi2, int32_t* out_info,
                      uint8_t* out_outlier);
// map_fuse_kernels.hip
int map_fuse_launch(mvo_ctx* ctx, const float* d_pos, const uint8_t* d_desc, int n_map, const MapFuseArgs& a, const MapFuseFrame* d_frames,
                    int n_frames, int ngroups, const unsigned long long* d_seen, GuidedPartials part, int32_t* out);
// window_triangulate_kernels.hip
int window_launch_search(mvo_ctx* ctx, const uint8_t* d_desc, const float* d_xy, const uint8_t* d_free, int nq, const WindowFrame* d_frames,
                         int n_frames, int ngroups, GuidedPartials part, int32_t* out);
int window_launch_verify(mvo_ctx* ctx, const WindowPairIn* d_pairs, int n, const WindowFrame* d_frames, const WindowVerifyArgs& a,
                         WindowPairOut* out);
// pose_optimize_kernels.hip
int pose_optimize_launch(mvo_ctx* ctx, const float* d_p3, const float* d_p2, const float* d_s, int n, const PoseOptArgs& a, PoseOptOut* out,
                         uint8_t* out_outlier);
// local_map_kernels.hip
int local_map_launch(mvo_ctx* ctx, const float* d_pos, const uint8_t* d_desc, const float* d_normal, const float* d_max_dist, int n_map,
                     const LocalMapArgs& a, const uint8_t* d_t, const double* d_tg, const uint8_t* d_skip, int nt, GuidedPartials part,
                     int32_t* out);
extern int g_pyr_force_chain;  // test hook (orb_kernels.hip)
extern int g_match_mfma;       // test hook (match_kernels.hip)
extern int g_pnp_replay_skew;  // test hook: the device replays the RANSAC loop with a wrong confidence
// track_host.cpp
void track_release(mvo_ctx* ctx);
// What the last mvo_estimate_possible_relative_poses(n matches) of this ctx left on the device, for the finish of the
// initialisation (init_host.cpp): the matched pixels, the E list followed by the H list, k_recover_pose's and
// k_h_decompose's outputs and k_init_triangulate's [5][n] points; and out, room for k_init_finish's results on m
// list entries (28 m bytes).  These buffers stay valid until the next call of that family on the ctx (track_host.cpp).
struct TrackInitView {
    const float *kp1, *kp2, *pts;
    const int32_t* lists;
    const double *e_out, *h_out;
    uint8_t* out;
};
int track_init_view(mvo_ctx* ctx, int n, int m, TrackInitView* v);
// ba_host.cpp (planning, pooled workspaces, launch service) + ba_kernels.hip (k_ba_lm)
struct mvo_ba_handle;
int ba_solve_device(mvo_ctx* ctx, mvo_ba_problem* p, mvo_ba_stats* st);
int ba_begin_device(mvo_ctx* ctx, const mvo_ba_problem* p);
int ba_end_device(mvo_ctx* ctx, mvo_ba_problem* p, mvo_ba_stats* st);
int ba_solve_batch_device(mvo_ctx* ctx, mvo_ba_problem* ps, int n, mvo_ba_stats* sts);
int ba_prepare_device(mvo_ctx* ctx, const mvo_ba_problem* p, mvo_ba_handle** out);
int ba_run_device(mvo_ctx* ctx, mvo_ba_handle* H);
int ba_fetch_device(mvo_ctx* ctx, mvo_ba_handle* H, double* poses, double* points, mvo_ba_stats* st);
void ba_release_device(mvo_ctx* ctx, mvo_ba_handle* H);
void ba_pool_release(mvo_ctx* ctx);
void ba_set_trace(mvo_ctx* ctx, int on);
int ba_get_trace(mvo_ctx* ctx, mvo_ba_handle* H, double* rows, int cap, int* n);
int ba_get_plan(mvo_ctx* ctx, mvo_ba_handle* H, int* G, int* nsplit, int32_t* wg_pt, int cap);
void ba_launch_stats(int device, long long* launches, long long* windows, double* ms, int reset);
void ba_service_times(int device, double* out5);
void ba_service_park(int device);
void ba_resident_stats(int device, long long* windows, long long* grid_starts, double* cycles = nullptr, long long* path_switches = nullptr);

#endif
