// csrc/map_fuse_host.cpp -- host side of the fusion of duplicate map points (include/mvo_hip.h: mvo_map_fuse_search,
// mvo_map_fuse): argument checks, the seen masks, the pose inverses, one upload, the launch, the results, and the serial
// resolution (one claimant per keypoint, union-find merges, additions, survivors).  The kernel is in map_fuse_kernels.hip,
// the rule in DESIGN.md section 19.  No other translation unit refers to this one.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "guided_match_host.h"

namespace {

// The checks, the upload, the launch, the wait.  On success the raw results lie in ctx->h_pin: idx, dist, px, n_candidates,
// n_frames blocks of n_map rows each; seen receives the masks.  *launched is false when there was nothing to search.
int search(mvo_ctx* ctx, mvo_map* map, const mvo_fuse_frame* frames, int n_frames, double fx, double fy, double cx, double cy, int cols,
           int rows, double max_px, const char* who, std::vector<unsigned long long>& seen, bool* launched) {
    auto fail = [&](const char* what, int code = MVO_ERR_INVALID) {  // the message names the entry point the caller used
        return mvo_set_err(ctx, code, (std::string(who) + ": " + what).c_str(), hipSuccess);
    };
    *launched = false;
    if (!map || n_frames < 0 || (n_frames && !frames)) return fail("bad arguments");
    if (n_frames > MF_MAX_FRAMES) return fail("more than 64 frames", MVO_ERR_CAPACITY);
    if (fx == 0 || fy == 0 || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy))
        return fail("fx or fy 0, or intrinsics not finite");
    if (cols <= 0 || rows <= 0) return fail("cols or rows <= 0");
    if (!(max_px >= 0)) return fail("max_px negative or NaN");
    const int n_map = map->n;
    seen.assign((size_t)n_map, 0ull);
    std::vector<double> Tcw(12 * (size_t)n_frames);
    size_t total = 0;
    int nt_max = 0;
    for (int f = 0; f < n_frames; ++f) {
        const mvo_fuse_frame& F = frames[f];
        double Ti[16];
        auto conn_and_seen = [&](int j) -> int {
            if (F.conn[j] < -2 || F.conn[j] >= n_map) return fail("conn outside [-2, n_map)");
            if (F.conn[j] >= 0) seen[F.conn[j]] |= 1ull << f;
            return MVO_OK;
        };
        if (int r = guided_check_frame(F, Ti, fail, conn_and_seen)) return r;
        std::memcpy(&Tcw[12 * (size_t)f], Ti, 12 * sizeof(double));
        total += (size_t)F.n;
        nt_max = std::max(nt_max, (int)F.n);
    }
    if (n_map == 0 || n_frames == 0) return MVO_OK;
    const int ngroups = guided_groups(nt_max), nbx = (n_map + 63) / 64;
    const size_t rows_all = (size_t)n_frames * n_map;
    // pinned staging: the kernel writes its rows x 28 bytes of results straight into the first part; the second carries the
    // frame table, the masks, the gate's view of every keypoint and the descriptors up (one copy)
    BlockCursor in;
    const size_t i_tab = in.block((size_t)n_frames * sizeof(MapFuseFrame)), i_seen = in.block((size_t)n_map * 8);
    const size_t i_tg = in.block(total * 24), i_desc = in.last(total * 32);
    mvo_fuse_state* e = mvo_state(ctx->fuse);
    StagedCall call{ctx};
    int r = call.begin(e->d_in, in.bytes, (size_t)1 << 20, align64(rows_all * 28),
                       [&] { return e->scratch.ensure(ctx, rows_all, ngroups, (size_t)n_frames * nbx); });
    if (r) return r;
    std::memcpy(call.h_in + i_seen, seen.data(), (size_t)n_map * 8);
    const std::vector<FrameSlice> at =
        guided_pack_frames(frames, n_frames, ngroups, reinterpret_cast<double*>(call.h_in + i_tg), call.h_in + i_desc,
                           [max_px](const mvo_fuse_frame& F, int j) { return F.conn[j] == -2 ? -1.0 : guided_tol2(max_px, F.scale, j); });
    MapFuseFrame* h_tab = reinterpret_cast<MapFuseFrame*>(call.h_in + i_tab);
    for (int f = 0; f < n_frames; ++f) {
        MapFuseFrame& row = h_tab[f];
        std::memcpy(row.T, &Tcw[12 * (size_t)f], sizeof row.T);
        row.t = reinterpret_cast<const uint4*>(e->d_in + i_desc + at[f].first * 32);
        row.tg = reinterpret_cast<const double*>(e->d_in + i_tg + at[f].first * 24);
        row.nt = at[f].nt, row.slice = at[f].slice;
        row.pad[0] = row.pad[1] = 0;
    }
    if ((r = call.upload(e->d_in))) return r;
    MapFuseArgs a;
    a.fx = fx, a.fy = fy, a.cx = cx, a.cy = cy;
    a.cols = cols, a.rows = rows;
    ExtractGate gate(ctx);
    if ((r = map_fuse_launch(ctx, map->d_pos, map->d_desc, n_map, a, reinterpret_cast<const MapFuseFrame*>(e->d_in + i_tab), n_frames,
                             ngroups, reinterpret_cast<const unsigned long long*>(e->d_in + i_seen), e->scratch.partials(),
                             reinterpret_cast<int32_t*>(call.h_out))) ||
        (r = call.finish(gate)))
        return r;
    *launched = true;
    return MVO_OK;
}

struct Components {  // union-find over the map rows; a root carries the OR of its members' masks
    std::vector<int32_t> parent;
    std::vector<unsigned long long> mask;
    explicit Components(const std::vector<unsigned long long>& seen) : parent(seen.size()), mask(seen) {
        for (size_t i = 0; i < parent.size(); ++i) parent[i] = (int32_t)i;
    }
    int32_t find(int32_t i) {
        while (parent[i] != i) i = parent[i] = parent[parent[i]];
        return i;
    }
};

}  // namespace

extern "C" {

// ORB-SLAM ORBmatcher::Fuse, the search; the reference has no counterpart (vo.cpp:528-576 only creates points)
int mvo_map_fuse_search(mvo_ctx* ctx, mvo_map* map, const mvo_fuse_frame* frames, int n_frames, double fx, double fy, double cx,
                        double cy, int cols, int rows, double max_px, int32_t* idx, int32_t* dist, int32_t* n_candidates, float* px) {
    if (!ctx) return MVO_ERR_INVALID;
    if (map && map->n && n_frames > 0 && (!idx || !dist))
        return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_map_fuse_search: bad arguments", hipSuccess);
    std::vector<unsigned long long> seen;
    bool launched;
    if (int r = search(ctx, map, frames, n_frames, fx, fy, cx, cy, cols, rows, max_px, "mvo_map_fuse_search", seen, &launched)) return r;
    if (!launched) return MVO_OK;
    const size_t rows_all = (size_t)n_frames * map->n;
    std::memcpy(idx, ctx->h_pin, rows_all * 8);
    std::memcpy(dist, ctx->h_pin + rows_all * 8, rows_all * 8);
    if (px) std::memcpy(px, ctx->h_pin + rows_all * 16, rows_all * 8);
    if (n_candidates) std::memcpy(n_candidates, ctx->h_pin + rows_all * 24, rows_all * 4);
    return MVO_OK;
}

// ORB-SLAM ORBmatcher::Fuse + MapPoint::Replace, in place of vo.cpp:528-576's unconditional new point
int mvo_map_fuse(mvo_ctx* ctx, mvo_map* map, const mvo_fuse_frame* frames, int n_frames, double fx, double fy, double cx, double cy,
                 int cols, int rows, const mvo_map_fuse_params* params, int32_t* replaced_by, mvo_fuse_observation* added, int cap_added,
                 int* n_added, int32_t* counts) {
    if (!ctx) return MVO_ERR_INVALID;
    auto fail = [&](const char* what, int code = MVO_ERR_INVALID) {
        return mvo_set_err(ctx, code, (std::string("mvo_map_fuse: ") + what).c_str(), hipSuccess);
    };
    if (!n_added || !counts || cap_added < 0 || (cap_added && !added) || (map && map->n && !replaced_by)) return fail("bad arguments");
    mvo_map_fuse_params P{3.0, 50};
    if (params) P = *params;
    if (P.max_hamming < 0 || P.max_hamming > 256) return fail("max_hamming outside 0..256");
    std::vector<unsigned long long> seen;
    bool launched;
    if (int r = search(ctx, map, frames, n_frames, fx, fy, cx, cy, cols, rows, P.max_px, "mvo_map_fuse", seen, &launched)) return r;
    const int n_map = map->n;
    int32_t cnt[6] = {0, 0, 0, 0, 0, 0};
    std::vector<int32_t> rep((size_t)n_map);
    for (int i = 0; i < n_map; ++i) rep[i] = i;
    std::vector<mvo_fuse_observation> add;
    if (launched) {
        const int32_t* idx = reinterpret_cast<const int32_t*>(ctx->h_pin);
        const int32_t* dist = idx + 2 * (size_t)n_frames * n_map;
        // one claimant per keypoint: queries arrive in ascending i, a later one takes the keypoint only with a smaller d
        // a winner (d, f, i, j) as one integer whose order is the declared one: d <= 256 | f < 64 | i < 2^31 | j < 2^16
        typedef unsigned long long Winner;
        auto winner = [](int32_t d, int32_t f, int32_t i, int32_t j) {
            return ((((Winner)d << 6 | (Winner)f) << 31 | (Winner)i) << 16) | (Winner)j;
        };
        auto frame_of = [](Winner w) { return (int32_t)(w >> 47 & 63); };
        auto point_of = [](Winner w) { return (int32_t)(w >> 16 & 0x7fffffffu); };
        auto keypoint_of = [](Winner w) { return (int32_t)(w & 0xffffu); };
        std::vector<Winner> merges, additions;
        std::vector<int32_t> owner;
        for (int f = 0; f < n_frames; ++f) {
            const mvo_fuse_frame& F = frames[f];
            const int32_t *fi = idx + 2 * (size_t)f * n_map, *fd = dist + 2 * (size_t)f * n_map;
            owner.assign((size_t)F.n, -1);
            for (int i = 0; i < n_map; ++i) {
                const int32_t j = fi[2 * i], d = fd[2 * i];
                if (j < 0 || d > P.max_hamming) continue;
                ++cnt[0];
                if (owner[j] < 0 || d < fd[2 * owner[j]]) owner[j] = i;
            }
            for (int j = 0; j < F.n; ++j) {
                if (owner[j] < 0) continue;
                if (F.conn[j] >= 0) merges.push_back(winner(fd[2 * owner[j]], f, owner[j], j));
                if (F.conn[j] == -1) additions.push_back(winner(fd[2 * owner[j]], f, owner[j], j));
            }
        }
        std::sort(merges.begin(), merges.end());  // ascending (d, f, i); (f, i) names one winner at most
        std::sort(additions.begin(), additions.end());
        Components C(seen);
        for (const Winner& w : merges) {
            const int32_t a = C.find(point_of(w)), b = C.find(frames[frame_of(w)].conn[keypoint_of(w)]);
            if (a == b) continue;
            if (C.mask[a] & C.mask[b]) {
                ++cnt[2];
                continue;
            }
            C.parent[b] = a;
            C.mask[a] |= C.mask[b];
            ++cnt[1];
        }
        // survivors: the largest popcount of a member's own mask, the lower row on a tie (rows ascend, so only more wins)
        std::vector<int32_t> best((size_t)n_map, -1);
        for (int i = 0; i < n_map; ++i) {
            const int32_t root = C.find(i);
            if (best[root] < 0 || __builtin_popcountll(seen[i]) > __builtin_popcountll(seen[best[root]])) best[root] = i;
        }
        for (int i = 0; i < n_map; ++i) {
            rep[i] = best[C.find(i)];
            cnt[5] += rep[i] != i ? 1 : 0;
        }
        for (const Winner& w : additions) {
            const int32_t f = frame_of(w), root = C.find(point_of(w));
            if ((C.mask[root] >> f) & 1ull) {
                ++cnt[4];
                continue;
            }
            C.mask[root] |= 1ull << f;
            add.push_back({f, keypoint_of(w), best[root]});
            ++cnt[3];
        }
    }
    *n_added = (int)add.size();
    if ((int)add.size() > cap_added) return fail("cap_added too small", MVO_ERR_CAPACITY);
    if (n_map) std::memcpy(replaced_by, rep.data(), (size_t)n_map * 4);
    if (!add.empty()) std::memcpy(added, add.data(), add.size() * sizeof(mvo_fuse_observation));
    std::memcpy(counts, cnt, sizeof cnt);
    return MVO_OK;
}

}  // extern "C"
