// csrc/guided_match_host.h -- what the host sides of the pose-gated matchers share.  epipolar_host.cpp and projection_host.cpp:
// the partial scratch of guided_knn2() (guided_knn2.h), the checks of the train set, and the filter with the
// one-query-per-train rule behind both mvo_*_features_* entry points.  map_fuse_host.cpp and window_triangulate_host.cpp, whose
// launches run over every buffered frame: their scratch, the checks of one mvo_fuse_frame and the packing of the frames'
// keypoints.  Inline, included by those files only: no translation unit refers to another, and no build file lists a further one.
#ifndef MVO_GUIDED_MATCH_HOST_H
#define MVO_GUIDED_MATCH_HOST_H
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "guided_knn2.h"
#include "staged_call.h"

inline void GuidedScratch::release() {
    buf.release();
    d_part = nullptr, d_part_cnt = nullptr, d_arrive = nullptr;
    cap = 0;
}

inline int GuidedScratch::ensure(mvo_ctx* ctx, int n) {
    if (n <= cap) return MVO_OK;
    release();
    const size_t c = (size_t)std::max(4096, n + n / 2);
    // partial key pairs, partial counts, one arrival counter per group of 64 queries (self re-arming, zeroed once)
    const size_t keys = GK_MAX_GROUPS * c * 8, cnts = GK_MAX_GROUPS * c * 4, ctr = (c / 64 + 2) * 4;
    if (int r = buf.ensure_exact(ctx, keys + cnts + ctr)) return r;
    d_part = reinterpret_cast<unsigned long long*>(buf.p);
    d_part_cnt = reinterpret_cast<int32_t*>(buf.p + keys);
    d_arrive = reinterpret_cast<int32_t*>(buf.p + keys + cnts);
    MVO_HIP(hipMemsetAsync(d_arrive, 0, ctr, ctx->stream));
    cap = (int)c;
    return MVO_OK;
}

inline int FrameScratch::ensure(mvo_ctx* ctx, size_t rows_all, int ngroups, size_t n_arrive) {
    keys_b = align64(rows_all * ngroups * 8);
    int r;
    if ((r = d_part.ensure(ctx, keys_b + rows_all * ngroups * 4, (size_t)1 << 18))) return r;
    const size_t had = d_arrive.cap;
    if ((r = d_arrive.ensure(ctx, n_arrive, 4096))) return r;
    if (d_arrive.cap != had)  // the counters re-arm themselves: zeroed once per allocation
        MVO_HIP(hipMemsetAsync(d_arrive, 0, d_arrive.cap * sizeof(int32_t), ctx->stream));
    return MVO_OK;
}

// nt <= 65535 (the train index lives in the low 16 bits of a key), t_scale finite and >= 0; who: the entry point the caller
// used, named in the message
inline int guided_check_trains(mvo_ctx* ctx, const char* who, const float* t_scale, int nt) {
    const char* what = nullptr;
    if (nt > 65535) what = ": more than 65535 train descriptors";
    for (int j = 0; !what && t_scale && j < nt; ++j)
        if (!std::isfinite(t_scale[j]) || t_scale[j] < 0) what = ": t_scale entry negative or not finite";
    if (!what) return MVO_OK;
    return mvo_set_err(ctx, nt > 65535 ? MVO_ERR_CAPACITY : MVO_ERR_INVALID, (std::string(who) + what).c_str(), hipSuccess);
}

inline double guided_tol2(double max_px, const float* t_scale, int j) {  // the squared tolerance of train j
    const double tl = max_px * (t_scale ? (double)t_scale[j] : 1.0);
    return tl * tl;
}

// One mvo_fuse_frame: n and the pointers, n <= 65535, T_w_c finite and, where T_c_w (16 doubles) is asked for, its inverse; then
// keypoint by keypoint also(j), the caller's own check, and scale finite and >= 0.  fail(what[, code]) words the caller's error.
template <class Fail, class Also>
int guided_check_frame(const mvo_fuse_frame& F, double* T_c_w, Fail fail, Also also) {
    if (F.n < 0 || (F.n && (!F.desc || !F.xy || !F.conn))) return fail("bad arguments");
    if (F.n > 65535) return fail("a frame with more than 65535 keypoints", MVO_ERR_CAPACITY);
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(F.T_w_c[k])) return fail("T_w_c is not finite");
    if (T_c_w && mvo_invert_pose(F.T_w_c, T_c_w) != MVO_OK) return fail("T_w_c is singular");
    for (int j = 0; j < F.n; ++j) {
        if (int r = also(j)) return r;
        if (F.scale && (!std::isfinite(F.scale[j]) || F.scale[j] < 0)) return fail("scale entry negative or not finite");
    }
    return MVO_OK;
}

struct FrameSlice {  // the keypoints of one frame inside the packed blocks
    size_t first;    // keypoints of the frames before it
    int32_t nt, slice;
};
// The keypoints of every frame, frame after frame: keypoint k's ((double)x, (double)y, tol2(F, j)) at h_tg + 3 k and its
// descriptor at h_desc + 32 k.  slice = guided_slice(nt, ngroups).
template <class Tol2>
std::vector<FrameSlice> guided_pack_frames(const mvo_fuse_frame* frames, int n_frames, int ngroups, double* h_tg, uint8_t* h_desc, Tol2 tol2) {
    std::vector<FrameSlice> at((size_t)n_frames);
    size_t first = 0;
    for (int f = 0; f < n_frames; ++f) {
        const mvo_fuse_frame& F = frames[f];
        at[f] = {first, F.n, guided_slice(F.n, ngroups)};
        for (int j = 0; j < F.n; ++j) {
            double* g = h_tg + 3 * (first + j);
            g[0] = (double)F.xy[2 * j], g[1] = (double)F.xy[2 * j + 1];
            g[2] = tol2(F, j);
        }
        if (F.n) std::memcpy(h_desc + first * 32, F.desc, (size_t)F.n * 32);
        first += (size_t)F.n;
    }
    return at;
}

// idx, dist: n1 x 2 of a raw call against n2 trains.  Query i is kept under the ceiling and the Lowe ratio (a single candidate
// on the ceiling alone); per train the claiming query with the smallest (distance, queryIdx) survives.
inline int guided_filter_matches(mvo_ctx* ctx, const int32_t* idx, const int32_t* dist, int n1, int n2, double lowe_ratio,
                                 int max_hamming, mvo_dmatch* out, int cap, int* n) {
    std::vector<int32_t> owner(n2 > 0 ? n2 : 1, -1);
    for (int i = 0; i < n1; ++i) {  // queries arrive in ascending order
        const int j = idx[2 * i], d0 = dist[2 * i];
        if (j < 0 || d0 > max_hamming) continue;
        if (idx[2 * i + 1] >= 0 && !((double)d0 < lowe_ratio * (double)dist[2 * i + 1])) continue;
        if (owner[j] < 0 || d0 < dist[2 * owner[j]]) owner[j] = i;
    }
    int cnt = 0;
    for (int j = 0; j < n2; ++j) cnt += owner[j] >= 0 ? 1 : 0;
    *n = cnt;
    if (cnt > cap || (cnt && !out)) return mvo_set_err(ctx, MVO_ERR_CAPACITY, "match buffer too small", hipSuccess);
    int k = 0;
    for (int j = 0; j < n2; ++j)
        if (owner[j] >= 0) out[k++] = {owner[j], j, 0, (float)dist[2 * owner[j]]};
    return MVO_OK;
}

#endif
