// csrc/guided_match_host.h -- what the host sides of the pose-gated matchers (epipolar_host.cpp, projection_host.cpp) share:
// the partial scratch of guided_knn2() (guided_knn2.h), the checks of the train set, and the filter with the
// one-query-per-train rule behind both mvo_*_features_* entry points.  Inline, included by those two files only: neither
// translation unit refers to the other, and no build file lists a further one.
#ifndef MVO_GUIDED_MATCH_HOST_H
#define MVO_GUIDED_MATCH_HOST_H
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "mvo_internal.h"

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
