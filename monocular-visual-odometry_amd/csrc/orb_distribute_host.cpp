// csrc/orb_distribute_host.cpp -- host side of the ORB-SLAM style detector (include/mvo_hip.h: mvo_orb_distribute_configure,
// mvo_calc_keypoints_distributed, its _dev form, mvo_debug_get_distribute_candidates): the cell table of an image geometry,
// the orchestration of k_fast_cells and k_ic_angle (orb_distribute_kernels.hip) and the quadtree spread.  The arithmetic is
// declared in DESIGN.md section 16.  The quadtree stays on the host for the reason retainBest does (orb_host.cpp): it is
// order-sensitive and handles <= 10^4 items.  No other translation unit refers to this one.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "mvo_internal.h"

int orb_setup_geometry(mvo_ctx* ctx, int w, int h);
int orb_grid_select(mvo_ctx* ctx, std::vector<mvo_keypoint>& kps, int image_rows, int image_cols);

static thread_local HostTimes g_ht_distribute;

namespace {

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// (u, v) of the pixels of cv::ORB's intensity-centroid disc (halfPatchSize 15, the umax table), row-major
int ic_disc(signed char* disc) {
    const int hp = 15;
    int umax[hp + 2];
    const int vmax = (int)std::floor(hp * std::sqrt(2.f) / 2 + 1), vmin = (int)std::ceil(hp * std::sqrt(2.f) / 2);
    for (int v = 0; v <= vmax; ++v) umax[v] = (int)std::lrint(std::sqrt((double)hp * hp - v * v));
    for (int v = hp, v0 = 0; v >= vmin; --v) {
        while (umax[v0] == umax[v0 + 1]) ++v0;
        umax[v] = v0;
        ++v0;
    }
    int n = 0;
    for (int v = -hp; v <= hp; ++v) {
        const int d = umax[v < 0 ? -v : v];
        for (int u = -d; u <= d; ++u) {
            disc[2 * n] = (signed char)u;
            disc[2 * n + 1] = (signed char)v;
            ++n;
        }
    }
    return n;
}

// Step 1 for every level of the pyramid of ctx (orb_setup_geometry has run): the cell table, the record slots, the levels'
// quadtree extents.  Made once per (image size, ORB parameters, detector parameters).
int setup_cells(mvo_ctx* ctx, int w, int h) {
    mvo_orb_distribute_state* s = mvo_state(ctx->dist);
    if (s->made && s->made_w == w && s->made_h == h && !std::memcmp(&s->made_orb, &ctx->orb, sizeof ctx->orb) &&
        !std::memcmp(&s->made_params, &s->params, sizeof s->params))
        return MVO_OK;
    s->made = false;
    const PyrInfo& P = ctx->pyr;
    const int W = s->params.cell_size, E = s->params.edge_threshold;
    s->cells.clear();
    size_t slot = 0;
    int kp_cap = 0;
    for (int l = 0; l < P.nlevels; ++l) {
        DistLevel& D = s->lv[l];
        D.minX = D.minY = E - 3;
        const int maxX = P.lv[l].w - E + 3, maxY = P.lv[l].h - E + 3;
        D.width = maxX - D.minX;
        D.height = maxY - D.minY;
        D.cell0 = (int)s->cells.size();
        D.ncells = 0;
        if (D.width < W || D.height < W) continue;  // nCols == 0 or nRows == 0: the level gives no key points
        const int nCols = D.width / W, nRows = D.height / W;
        const int wCell = ceil_div(D.width, nCols), hCell = ceil_div(D.height, nRows);
        for (int i = 0; i < nRows; ++i) {
            const int iniY = D.minY + i * hCell, maxYc = std::min(iniY + hCell + 6, maxY);
            if (iniY >= maxY - 3) continue;
            for (int j = 0; j < nCols; ++j) {
                const int iniX = D.minX + j * wCell, maxXc = std::min(iniX + wCell + 6, maxX);
                if (iniX >= maxX - 6) continue;
                const int sw = maxXc - iniX - 6, sh = maxYc - iniY - 6;
                if (sw <= 0 || sh <= 0) continue;  // no scored pixel
                if (sw > DC_MAX_SCORED || sh > DC_MAX_SCORED)
                    return mvo_set_err(ctx, MVO_ERR_INVALID, "cell larger than the detection kernel's tile", hipSuccess);
                DistCell c{};
                c.x0 = iniX, c.y0 = iniY, c.pw = maxXc - iniX, c.ph = maxYc - iniY;
                c.level = l;
                c.slot = (int)slot;
                c.cap = ceil_div(sw, 2) * ceil_div(sh, 2);
                slot += (size_t)c.cap;
                s->cells.push_back(c);
            }
        }
        D.ncells = (int)s->cells.size() - D.cell0;
        const int nIni = std::max(1, (2 * D.width + D.height) / (2 * D.height));
        kp_cap += std::max(ctx->quota[l] + 2, nIni);
    }
    s->n_records = slot;
    s->kp_cap = kp_cap;
    s->d_cells.release();
    if (!s->cells.empty()) {
        if (int r = s->d_cells.ensure_exact(ctx, s->cells.size())) return r;
        MVO_HIP(hipMemcpy(s->d_cells, s->cells.data(), s->cells.size() * sizeof(DistCell), hipMemcpyHostToDevice));
    }
    if (!s->d_disc) {
        signed char disc[768 * 2] = {0};
        s->disc_n = ic_disc(disc);
        if (int r = s->d_disc.ensure_exact(ctx, sizeof disc)) return r;
        MVO_HIP(hipMemcpy(s->d_disc, disc, sizeof disc, hipMemcpyHostToDevice));
    }
    s->made_orb = ctx->orb;
    s->made_params = s->params;
    s->made_w = w, s->made_h = h;
    s->made = true;
    return MVO_OK;
}

// ---------------------------------------------------------------------------------------------- step 6: the quadtree
// A node owns the range [b, e) of `ord`, indices into the level's candidates in candidate order; a split partitions the range
// stably into its four children, so every node keeps candidate order and no node allocates.
struct QNode {
    int x0, x1, y0, y1;
    int b, e;
};
struct QuadTree {
    const mvo_distribute_candidate* c;  // the level's candidates
    int minX, minY;
    std::vector<int> ord, tmp;

    // the non-empty children of n in the declared order
    int split(const QNode& n, QNode* kids) {
        const int hx = (n.x1 - n.x0 + 1) / 2, hy = (n.y1 - n.y0 + 1) / 2;
        const int mx = n.x0 + hx, my = n.y0 + hy;
        int cnt[4] = {0, 0, 0, 0};
        auto child = [&](int i) { return (c[i].x - minX >= mx ? 1 : 0) + (c[i].y - minY >= my ? 2 : 0); };
        for (int k = n.b; k < n.e; ++k) ++cnt[child(ord[k])];
        int start[4], at = n.b;
        for (int q = 0; q < 4; ++q) start[q] = at, at += cnt[q];
        int fill[4] = {start[0], start[1], start[2], start[3]};
        for (int k = n.b; k < n.e; ++k) tmp[fill[child(ord[k])]++] = ord[k];
        std::copy(tmp.begin() + n.b, tmp.begin() + n.e, ord.begin() + n.b);
        const int bx[4][2] = {{n.x0, mx}, {mx, n.x1}, {n.x0, mx}, {mx, n.x1}};
        const int by[4][2] = {{n.y0, my}, {n.y0, my}, {my, n.y1}, {my, n.y1}};
        int nk = 0;
        for (int q = 0; q < 4; ++q)
            if (cnt[q]) kids[nk++] = QNode{bx[q][0], bx[q][1], by[q][0], by[q][1], start[q], start[q] + cnt[q]};
        return nk;
    }

    // the kept candidates (indices into c) in leaf order
    void run(int n, int width, int height, int N, std::vector<int>& keep) {
        keep.clear();
        if (n == 0) return;
        ord.resize(n);
        tmp.resize(n);
        std::vector<QNode> nodes, next;
        // initial nodes: vertical strips; the candidates of a strip keep candidate order
        const int nIni = std::max(1, (2 * width + height) / (2 * height));
        {
            std::vector<int> cnt(nIni, 0), strip(n);
            for (int i = 0; i < n; ++i) {
                int k = 0;  // the strip with k width / nIni <= x < (k + 1) width / nIni
                const int x = c[i].x - minX;
                while (k + 1 < nIni && x >= (k + 1) * width / nIni) ++k;
                strip[i] = k;
                ++cnt[k];
            }
            std::vector<int> start(nIni + 1, 0);
            for (int k = 0; k < nIni; ++k) start[k + 1] = start[k] + cnt[k];
            std::vector<int> fill(start.begin(), start.end() - 1);
            for (int i = 0; i < n; ++i) ord[fill[strip[i]]++] = i;
            for (int k = 0; k < nIni; ++k)
                if (cnt[k]) nodes.push_back(QNode{k * width / nIni, (k + 1) * width / nIni, 0, height, start[k], start[k + 1]});
        }
        std::vector<int> S, kidn;
        std::vector<QNode> kids;
        for (;;) {
            S.clear();
            for (int p = 0; p < (int)nodes.size(); ++p)
                if (nodes[p].e - nodes[p].b > 1) S.push_back(p);
            if (S.empty() || (int)nodes.size() >= N) break;
            bool stop = false;
            kidn.assign(nodes.size(), -1);
            kids.resize(nodes.size() * 4);
            if ((int)nodes.size() + 3 * (int)S.size() <= N) {
                for (int p : S) kidn[p] = split(nodes[p], &kids[(size_t)p * 4]);
            } else {
                std::sort(S.begin(), S.end(), [&](int a, int b) {
                    const int ca = nodes[a].e - nodes[a].b, cb = nodes[b].e - nodes[b].b;
                    return ca != cb ? ca > cb : a < b;
                });
                int len = (int)nodes.size();
                for (int p : S) {
                    kidn[p] = split(nodes[p], &kids[(size_t)p * 4]);
                    len += kidn[p] - 1;
                    if (len >= N) {
                        stop = true;
                        break;
                    }
                }
            }
            next.clear();
            for (int p = 0; p < (int)nodes.size(); ++p) {
                if (kidn[p] < 0) next.push_back(nodes[p]);
                else next.insert(next.end(), kids.begin() + (size_t)p * 4, kids.begin() + (size_t)p * 4 + kidn[p]);
            }
            nodes.swap(next);
            if (stop) break;
        }
        for (const QNode& nd : nodes) {
            int best = ord[nd.b];
            for (int k = nd.b + 1; k < nd.e; ++k)
                if (c[ord[k]].score > c[best].score) best = ord[k];
            keep.push_back(best);
        }
    }
};

// the detector on an image already in device memory; leaves the raw pyramid cached in the ctx
int detect_device(mvo_ctx* ctx, const uint8_t* d_img, int w, int h, int stride, int channels, std::vector<mvo_keypoint>& out) {
    HostTimes& ht = g_ht_distribute;
    ht.start();
    int r = orb_setup_geometry(ctx, w, h);
    if (r) return r;
    if ((r = setup_cells(ctx, w, h))) return r;
    mvo_orb_distribute_state* s = ctx->dist.get();
    const PyrInfo& P = ctx->pyr;
    const int n_cells = (int)s->cells.size();
    ctx->pyr_valid = ctx->blur_valid = false;
    // pinned: [int32 count x cells][8-byte records x slots][8-byte kept points x kp_cap][float angle x kp_cap]
    const size_t counts_bytes = round_up((size_t)n_cells * 4, 64), rec_bytes = s->n_records * sizeof(DistRecord);
    const size_t kp_bytes = round_up((size_t)s->kp_cap * sizeof(DistRecord), 64);
    if ((r = mvo_ensure_pinned(ctx, counts_bytes + rec_bytes + kp_bytes + (size_t)s->kp_cap * 4 + 64))) return r;
    int32_t* counts = reinterpret_cast<int32_t*>(ctx->h_pin);
    DistRecord* records = reinterpret_cast<DistRecord*>(ctx->h_pin + counts_bytes);
    DistRecord* kept = reinterpret_cast<DistRecord*>(ctx->h_pin + counts_bytes + rec_bytes);
    float* angles = reinterpret_cast<float*>(ctx->h_pin + counts_bytes + rec_bytes + kp_bytes);
    {
        ExtractGate gate(ctx);
        if ((r = orb_launch_pyramid(ctx, d_img, stride, channels, P.nlevels))) return r;
        if ((r = dist_launch_cells(ctx, s->d_cells, n_cells, s->params.min_threshold, s->params.ini_threshold, counts, records))) return r;
        MVO_HIP(hipEventRecord(ctx->ev, ctx->stream));
        // a ctx that describes from whole blurred levels has them blurred now, behind the event: while this thread spreads the
        // candidates
        if (orb_brief_from_levels(ctx) && (r = orb_launch_blur(ctx, P.nlevels))) return r;
        ht.lap(0);
        MVO_HIP(hipEventSynchronize(ctx->ev));
    }
    ht.lap(1);
    // step 5: a cell is the unit of the candidate order and its slot is row-major already: the slots are appended
    std::vector<mvo_distribute_candidate>& cand = s->last_cand;
    size_t total = 0;
    for (int k = 0; k < n_cells; ++k) total += (size_t)counts[k];
    cand.resize(total);
    mvo_distribute_candidate* o = cand.data();
    int level_start[MVO_MAX_LEVELS + 1] = {0};
    for (int l = 0; l < P.nlevels; ++l) {
        level_start[l] = (int)(o - cand.data());
        for (int k = s->lv[l].cell0; k < s->lv[l].cell0 + s->lv[l].ncells; ++k) {
            // the slots are freshly written by the device: pull the next cell's lines in while this one is copied
            if (k + 1 < n_cells) {
                const char* nx = (const char*)(records + s->cells[k + 1].slot);
                for (int b = 0, nb = counts[k + 1] * (int)sizeof(DistRecord); b < nb; b += 64) __builtin_prefetch(nx + b);
            }
            const DistRecord* rec = records + s->cells[k].slot;
            for (int i = 0; i < counts[k]; ++i) *o++ = {rec[i].x, rec[i].y, l, rec[i].level_score & 0xffff};
        }
    }
    level_start[P.nlevels] = (int)cand.size();
    ht.lap(2);
    // step 6
    QuadTree qt;
    std::vector<int> keep, kept_idx;
    for (int l = 0; l < P.nlevels; ++l) {
        qt.c = cand.data() + level_start[l];
        qt.minX = s->lv[l].minX, qt.minY = s->lv[l].minY;
        qt.run(level_start[l + 1] - level_start[l], s->lv[l].width, s->lv[l].height, ctx->quota[l], keep);
        for (int i : keep) kept_idx.push_back(level_start[l] + i);
    }
    ht.lap(3);
    const int n = (int)kept_idx.size();
    if (n > s->kp_cap) return mvo_set_err(ctx, MVO_ERR_CAPACITY, "more key points than the quadtree can leave", hipSuccess);
    // step 7
    for (int i = 0; i < n; ++i) {
        const mvo_distribute_candidate& c = cand[kept_idx[i]];
        kept[i].x = (int16_t)c.x;
        kept[i].y = (int16_t)c.y;
        kept[i].level_score = (c.level << 16) | c.score;
    }
    {
        ExtractGate gate(ctx);
        if ((r = dist_launch_ic_angle(ctx, s->d_disc, s->disc_n, kept, n, angles))) return r;
        MVO_HIP(hipStreamSynchronize(ctx->stream));
    }
    out.clear();
    out.reserve(n);
    for (int i = 0; i < n; ++i) {
        const mvo_distribute_candidate& c = cand[kept_idx[i]];
        const float sf = P.lv[c.level].scale;
        mvo_keypoint k;
        k.x = (float)c.x * sf;
        k.y = (float)c.y * sf;
        k.size = 31 * sf;
        k.angle = angles[i];
        k.response = (float)c.score;
        k.octave = c.level;
        k.class_id = -1;
        out.push_back(k);
    }
    ctx->pyr_valid = true;
    ctx->pyr_levels_built = P.nlevels;
    ht.lap(4);
    static const char* const names[] = {"launch", "wait", "append", "quadtree", "angle"};
    ht.frame(names, 5);
    return MVO_OK;
}

int check_image(mvo_ctx* ctx, const void* img, int w, int h, int stride, int ch, const mvo_keypoint* kps, const int* n) {
    if (!ctx) return MVO_ERR_INVALID;
    if (!img || w < 1 || h < 1 || (ch != 1 && ch != 3 && ch != 4) || stride < w * ch)
        return mvo_set_err(ctx, MVO_ERR_INVALID, "bad image arguments", hipSuccess);
    if (!kps || !n) return mvo_set_err(ctx, MVO_ERR_INVALID, "null output", hipSuccess);
    return MVO_OK;
}

int finish(mvo_ctx* ctx, const uint8_t* d_img, int w, int h, int stride, int ch, mvo_keypoint* kps, int cap, int* n) {
    std::vector<mvo_keypoint> v;
    int r = detect_device(ctx, d_img, w, h, stride, ch, v);
    if (r) return r;
    if ((r = orb_grid_select(ctx, v, h, w))) return r;  // step 8
    if (ctx->prof) mvo_prof_collect(ctx);
    *n = (int)v.size();
    if ((int)v.size() > cap) return mvo_set_err(ctx, MVO_ERR_CAPACITY, "keypoint buffer too small", hipSuccess);
    std::copy(v.begin(), v.end(), kps);
    return MVO_OK;
}

}  // namespace

extern "C" {

// README.md section 5 ("use the ORB-SLAM's method for extracting enough uniformly distributed keypoints across different
// scales"): the parameters of that method
int mvo_orb_distribute_configure(mvo_ctx* ctx, const mvo_orb_distribute_params* p) {
    if (!ctx) return MVO_ERR_INVALID;
    const mvo_orb_distribute_params def{20, 7, 30, 19};
    if (!p) p = &def;
    if (p->ini_threshold < 1 || p->ini_threshold > 255 || p->min_threshold < 1 || p->min_threshold > p->ini_threshold ||
        p->cell_size < 8 || p->cell_size > DC_MAX_CELL_SIZE || p->edge_threshold < 19 || p->edge_threshold > 31)
        return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_orb_distribute_configure: parameter out of range", hipSuccess);
    mvo_state(ctx->dist)->params = *p;
    return MVO_OK;
}

int mvo_calc_keypoints_distributed(mvo_ctx* ctx, const uint8_t* image, int w, int h, int stride, int ch, mvo_keypoint* kps,
                                   int cap, int* n) {
    int r = check_image(ctx, image, w, h, stride, ch, kps, n);
    if (r) return r;
    MVO_HIP(hipSetDevice(ctx->device));
    if ((r = mvo_stage_image(ctx, image, h, stride))) return r;  // (the staging buffer mvo_calc_keypoints uploads into)
    return finish(ctx, ctx->d_img, w, h, stride, ch, kps, cap, n);
}

int mvo_calc_keypoints_distributed_dev(mvo_ctx* ctx, const void* d_image, int w, int h, int stride, int ch, mvo_keypoint* kps,
                                       int cap, int* n) {
    int r = check_image(ctx, d_image, w, h, stride, ch, kps, n);
    if (r) return r;
    MVO_HIP(hipSetDevice(ctx->device));
    return finish(ctx, (const uint8_t*)d_image, w, h, stride, ch, kps, cap, n);
}

int mvo_debug_get_distribute_candidates(mvo_ctx* ctx, mvo_distribute_candidate* out, int cap, int* n) {
    if (!ctx || !n) return MVO_ERR_INVALID;
    const std::vector<mvo_distribute_candidate> none;
    const std::vector<mvo_distribute_candidate>& c = ctx->dist ? ctx->dist->last_cand : none;
    *n = (int)c.size();
    if (!out) return MVO_OK;
    if ((int)c.size() > cap) return mvo_set_err(ctx, MVO_ERR_CAPACITY, "candidate buffer too small", hipSuccess);
    std::copy(c.begin(), c.end(), out);
    return MVO_OK;
}

}  // extern "C"
