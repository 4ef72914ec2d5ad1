// csrc/window_triangulate_host.cpp -- host side of the triangulation of new map points against every buffered frame
// (include/mvo_hip.h: mvo_window_triangulate_search, mvo_window_triangulate): argument checks, the relative poses and the
// fundamental matrices, one upload, the search launch, the filter (guided_match_host.h), one small upload, the verification
// launch and the choice.  The kernels are in window_triangulate_kernels.hip, the rule in DESIGN.md section 20.  No other
// translation unit refers to this one.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "guided_match_host.h"

namespace {

struct Search {
    std::vector<WindowFrame> rows;  // device pointers not yet set
    int n_free = 0, n_active = 0;
    bool launched = false;
};

// The checks, the upload, the launch, the wait.  On success, when s.launched, the raw results lie in ctx->h_pin: idx, dist,
// n_candidates, n_frames blocks of curr->n rows each, and the frame table is on the device.
int search(mvo_ctx* ctx, const mvo_fuse_frame* curr, const mvo_fuse_frame* frames, int n_frames, double fx, double fy, double cx, double cy,
           double max_line_px, double min_baseline, const char* who, Search& s) {
    auto fail = [&](const char* what, int code = MVO_ERR_INVALID) {  // the message names the entry point the caller used
        return mvo_set_err(ctx, code, (std::string(who) + ": " + what).c_str(), hipSuccess);
    };
    if (!curr || n_frames < 0 || (n_frames && !frames)) return fail("bad arguments");
    if (n_frames > MF_MAX_FRAMES) return fail("more than 64 frames", MVO_ERR_CAPACITY);
    if (fx == 0 || fy == 0 || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy))
        return fail("fx or fy 0, or intrinsics not finite");
    if (!(max_line_px >= 0)) return fail("max_line_px negative or NaN");
    if (!(min_baseline >= 0)) return fail("min_baseline negative or NaN");
    // (the inverse is not asked for: a singular pose is reported behind the scales, by the calls below)
    auto check_frame = [&](const mvo_fuse_frame& F) { return guided_check_frame(F, nullptr, fail, [](int) { return (int)MVO_OK; }); };
    if (int r = check_frame(*curr)) return r;
    double Tci[16];
    if (mvo_invert_pose(curr->T_w_c, Tci) != MVO_OK) return fail("T_w_c is singular");
    s.rows.assign((size_t)n_frames, WindowFrame());
    size_t total = 0;
    int nt_max = 0;
    for (int f = 0; f < n_frames; ++f) {
        const mvo_fuse_frame& F = frames[f];
        if (int r = check_frame(F)) return r;
        WindowFrame& row = s.rows[f];
        if (mvo_fundamental_from_poses(curr->T_w_c, F.T_w_c, fx, fy, cx, cy, row.F) != MVO_OK) return fail("T_w_c is singular");
        double M[16];
        for (int i = 0; i < 4; ++i)  // M = inv(T_w_c_curr) * T_w_c_f, summed k = 0..3 in order
            for (int j = 0; j < 4; ++j) {
                double acc = 0;
                for (int k = 0; k < 4; ++k) acc += Tci[4 * i + k] * F.T_w_c[4 * k + j];
                M[4 * i + j] = acc;
            }
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) row.R[3 * i + j] = M[4 * i + j];
            row.tr[i] = M[4 * i + 3];
        }
        const double b2 = (row.tr[0] * row.tr[0] + row.tr[1] * row.tr[1]) + row.tr[2] * row.tr[2];
        row.active = (b2 > 0 && b2 >= min_baseline * min_baseline) ? 1 : 0;
        s.n_active += row.active;
        row.nt = F.n, row.pad = 0;
        total += (size_t)F.n;
        nt_max = std::max(nt_max, (int)F.n);
    }
    const int nq = curr->n;
    for (int i = 0; i < nq; ++i) s.n_free += curr->conn[i] == -1 ? 1 : 0;
    if (n_frames == 0 || s.n_free == 0) return MVO_OK;
    const int ngroups = guided_groups(nt_max), nbx = (nq + 63) / 64;
    const size_t rows_all = (size_t)n_frames * nq;
    // pinned staging: the kernel writes its rows x 20 bytes of results straight into the first part; the second carries the
    // frame table (first in d_in: the verification reads it there), curr and the gate's view and the descriptors of every frame
    // up (one copy)
    BlockCursor in;
    const size_t i_tab = in.block((size_t)n_frames * sizeof(WindowFrame)), i_free = in.block((size_t)nq), i_cxy = in.block((size_t)nq * 8);
    const size_t i_cdesc = in.block((size_t)nq * 32), i_tg = in.block(total * 24), i_desc = in.last(total * 32);
    mvo_window_state* e = mvo_state(ctx->window);
    StagedCall call{ctx};
    int r = call.begin(e->d_in, in.bytes, (size_t)1 << 20, align64(rows_all * 20),
                       [&] { return e->scratch.ensure(ctx, rows_all, ngroups, (size_t)n_frames * nbx); });
    if (r) return r;
    for (int i = 0; i < nq; ++i) call.h_in[i_free + i] = curr->conn[i] == -1 ? 1 : 0;
    std::memcpy(call.h_in + i_cxy, curr->xy, (size_t)nq * 8);
    std::memcpy(call.h_in + i_cdesc, curr->desc, (size_t)nq * 32);
    const std::vector<FrameSlice> at =
        guided_pack_frames(frames, n_frames, ngroups, reinterpret_cast<double*>(call.h_in + i_tg), call.h_in + i_desc,
                           [max_line_px](const mvo_fuse_frame& F, int j) { return F.conn[j] == -1 ? guided_tol2(max_line_px, F.scale, j) : -1.0; });
    for (int f = 0; f < n_frames; ++f) {
        WindowFrame& row = s.rows[f];
        row.d = reinterpret_cast<const uint4*>(e->d_in + i_desc + at[f].first * 32);
        row.tg = reinterpret_cast<const double*>(e->d_in + i_tg + at[f].first * 24);
        row.slice = at[f].slice;
    }
    std::memcpy(call.h_in + i_tab, s.rows.data(), (size_t)n_frames * sizeof(WindowFrame));
    if ((r = call.upload(e->d_in))) return r;
    ExtractGate gate(ctx);
    if ((r = window_launch_search(ctx, e->d_in + i_cdesc, reinterpret_cast<const float*>(e->d_in + i_cxy), e->d_in + i_free, nq,
                                  reinterpret_cast<const WindowFrame*>(e->d_in + i_tab), n_frames, ngroups, e->scratch.partials(),
                                  reinterpret_cast<int32_t*>(call.h_out))) ||
        (r = call.finish(gate)))
        return r;
    s.launched = true;
    return MVO_OK;
}

}  // namespace

extern "C" {

// ORB-SLAM ORBmatcher::SearchForTriangulation over every neighbouring keyframe; the reference has one pair of views
// (vo_addFrame.cpp:104-116)
int mvo_window_triangulate_search(mvo_ctx* ctx, const mvo_fuse_frame* curr, const mvo_fuse_frame* frames, int n_frames, double fx,
                                  double fy, double cx, double cy, double max_line_px, double min_baseline, int32_t* idx,
                                  int32_t* dist, int32_t* n_candidates) {
    if (!ctx) return MVO_ERR_INVALID;
    if (curr && curr->n > 0 && n_frames > 0 && (!idx || !dist))
        return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_window_triangulate_search: bad arguments", hipSuccess);
    Search s;
    if (int r = search(ctx, curr, frames, n_frames, fx, fy, cx, cy, max_line_px, min_baseline, "mvo_window_triangulate_search", s)) return r;
    const size_t rows_all = (size_t)n_frames * curr->n;
    if (!s.launched) {  // no frame, no keypoint or no free keypoint: every row is the row of a pair that is not active
        for (size_t k = 0; k < 2 * rows_all; ++k) idx[k] = -1, dist[k] = INT_MAX;
        for (size_t k = 0; n_candidates && k < rows_all; ++k) n_candidates[k] = -1;
        return MVO_OK;
    }
    std::memcpy(idx, ctx->h_pin, rows_all * 8);
    std::memcpy(dist, ctx->h_pin + rows_all * 8, rows_all * 8);
    if (n_candidates) std::memcpy(n_candidates, ctx->h_pin + rows_all * 16, rows_all * 4);
    return MVO_OK;
}

// ORB-SLAM LocalMapping::CreateNewMapPoints in place of vo_addFrame.cpp:104-116's single pair of views
int mvo_window_triangulate(mvo_ctx* ctx, const mvo_fuse_frame* curr, const mvo_fuse_frame* frames, int n_frames, double fx, double fy,
                           double cx, double cy, const mvo_window_triangulate_params* params, mvo_window_point* points,
                           int cap_points, int* n_points, mvo_window_pair* pairs, int cap_pairs, int* n_pairs, int32_t* counts) {
    if (!ctx) return MVO_ERR_INVALID;
    auto fail = [&](const char* what, int code = MVO_ERR_INVALID) {
        return mvo_set_err(ctx, code, (std::string("mvo_window_triangulate: ") + what).c_str(), hipSuccess);
    };
    if (!n_points || !counts || cap_points < 0 || (cap_points && !points) || (pairs && (cap_pairs < 0 || !n_pairs))) return fail("bad arguments");
    mvo_window_triangulate_params P{2.0, 0.8, 64, 0.9998, 5.991, 1.8, 0.0};
    if (params) P = *params;
    if (P.max_hamming < 0 || P.max_hamming > 256) return fail("max_hamming outside 0..256");
    if (std::isnan(P.lowe_ratio)) return fail("lowe_ratio NaN");
    if (!(P.max_cos_parallax >= 0 && P.max_cos_parallax <= 1)) return fail("max_cos_parallax outside [0, 1] or NaN");
    if (!(P.max_reproj_chi2 >= 0)) return fail("max_reproj_chi2 negative or NaN");
    if (!(P.ratio_factor >= 0)) return fail("ratio_factor negative or NaN");
    Search s;
    if (int r = search(ctx, curr, frames, n_frames, fx, fy, cx, cy, P.max_line_px, P.min_baseline, "mvo_window_triangulate", s)) return r;
    const int nq = curr->n;
    int32_t cnt[12] = {s.n_free, s.n_active, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<mvo_window_pair> pr;
    if (s.launched) {
        const int32_t* idx = reinterpret_cast<const int32_t*>(ctx->h_pin);
        const int32_t* dist = idx + 2 * (size_t)n_frames * nq;
        std::vector<mvo_dmatch> m;
        for (int f = 0; f < n_frames; ++f) {
            const int32_t *fi = idx + 2 * (size_t)f * nq, *fd = dist + 2 * (size_t)f * nq;
            for (int i = 0; i < nq; ++i) cnt[2] += fi[2 * i] >= 0 ? 1 : 0;
            const int n2 = frames[f].n;
            m.resize((size_t)std::max(n2, 1));
            int k = 0;
            if (int r = guided_filter_matches(ctx, fi, fd, nq, n2, P.lowe_ratio, P.max_hamming, m.data(), n2, &k)) return r;
            for (int a = 0; a < k; ++a) {  // in ascending train index
                mvo_window_pair w{};
                w.frame = f, w.keypoint = m[a].queryIdx, w.train = m[a].trainIdx, w.hamming = (int32_t)m[a].distance;
                pr.push_back(w);
            }
        }
    }
    const int np = (int)pr.size();
    cnt[3] = np;
    if (np) {
        // (the results of the search have been read: the staging buffer is free again; the frame table stays on the device)
        // The device is current and the stream idle behind the search, and the pairs have a buffer of their own type: stage()
        // in place of begin()
        mvo_window_state* e = ctx->window.get();
        StagedCall call{ctx};
        int r;
        if ((r = e->d_pairs.ensure(ctx, (size_t)np, 4096)) ||
            (r = call.stage(align64((size_t)np * sizeof(WindowPairOut)), (size_t)np * sizeof(WindowPairIn))))
            return r;
        WindowPairIn* h_pairs = reinterpret_cast<WindowPairIn*>(call.h_in);
        for (int a = 0; a < np; ++a) {
            const mvo_fuse_frame& F = frames[pr[a].frame];
            const int i = pr[a].keypoint, j = pr[a].train;
            h_pairs[a] = {pr[a].frame, 0, F.xy[2 * j], F.xy[2 * j + 1], curr->xy[2 * i], curr->xy[2 * i + 1], F.scale ? F.scale[j] : 1.0f,
                          curr->scale ? curr->scale[i] : 1.0f};
        }
        if ((r = call.upload(e->d_pairs))) return r;
        WindowVerifyArgs a;
        a.fx = fx, a.fy = fy, a.cx = cx, a.cy = cy;
        a.c2max = P.max_cos_parallax * P.max_cos_parallax, a.chi2 = P.max_reproj_chi2, a.rf2 = P.ratio_factor * P.ratio_factor;
        ExtractGate gate(ctx);
        if ((r = window_launch_verify(ctx, e->d_pairs, np, reinterpret_cast<const WindowFrame*>(e->d_in.p), a,
                                      reinterpret_cast<WindowPairOut*>(call.h_out))) ||
            (r = call.finish(gate)))
            return r;
        const WindowPairOut* o = reinterpret_cast<const WindowPairOut*>(call.h_out);
        for (int k = 0; k < np; ++k) {
            std::memcpy(pr[k].p_curr, o[k].p_curr, sizeof pr[k].p_curr);
            std::memcpy(pr[k].p_frame, o[k].p_frame, sizeof pr[k].p_frame);
            pr[k].cos2 = o[k].cos2, pr[k].status = o[k].status;
            for (int b = 0; b < 6; ++b) cnt[4 + b] += (o[k].status >> b) & 1;
            cnt[10] += o[k].status == 0 ? 1 : 0;
        }
    }
    // the choice: per keypoint the accepted pair with the smallest cos2; frames ascend, so only a smaller cos2 replaces
    std::vector<int32_t> best((size_t)std::max(nq, 1), -1);
    for (int k = 0; k < np; ++k) {
        if (pr[k].status != 0) continue;
        int32_t& b = best[pr[k].keypoint];
        if (b < 0 || pr[k].cos2 < pr[b].cos2) b = k;
    }
    int n_new = 0;
    for (int i = 0; i < nq; ++i) n_new += best[i] >= 0 ? 1 : 0;
    cnt[11] = n_new;
    *n_points = n_new;
    if (pairs) *n_pairs = np;
    if (n_new > cap_points) return fail("cap_points too small", MVO_ERR_CAPACITY);
    if (pairs && np > cap_pairs) return fail("cap_pairs too small", MVO_ERR_CAPACITY);
    int k = 0;
    for (int i = 0; i < nq; ++i) {
        if (best[i] < 0) continue;
        const mvo_window_pair& w = pr[best[i]];
        mvo_window_point q{};
        q.keypoint = i, q.frame = w.frame, q.train = w.train, q.hamming = w.hamming, q.cos2 = w.cos2;
        std::memcpy(q.p_curr, w.p_curr, sizeof q.p_curr);
        points[k++] = q;
    }
    if (pairs && np) std::memcpy(pairs, pr.data(), (size_t)np * sizeof(mvo_window_pair));
    std::memcpy(counts, cnt, sizeof cnt);
    return MVO_OK;
}

}  // extern "C"
