// tests/sim/guided_host_check.cpp -- TEST AID, a program of its own for a sanitizer build of csrc/guided_match_host.h on the
// CPU (guided_host_check.mk): the filter behind both mvo_*_features_* entry points and the GuidedScratch bookkeeping, with
// the device allocations served by hip_emu/.  Exercises empty inputs, a single candidate, ties on distance, the capacity
// error, the train checks and grow / regrow / release of the scratch; prints "guided_host_check ok" and returns 0.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "guided_match_host.h"

// what guided_match_host.h takes from the other translation units of the library
int mvo_set_err(mvo_ctx* c, int code, const char* what, hipError_t) {
    c->err = what;
    return code;
}
void ba_service_free(int, void* p, bool) { (void)hipFree(p); }

#define CHECK(x)                                                       \
    do {                                                               \
        if (!(x)) {                                                    \
            std::printf("line %d: %s is false\n", __LINE__, #x);       \
            return 1;                                                  \
        }                                                              \
    } while (0)

int main() {
    mvo_ctx* ctx = new mvo_ctx();
    const int M = INT_MAX;
    int n = -1;
    std::vector<mvo_dmatch> out(8);
    // no query, no train, neither
    CHECK(guided_filter_matches(ctx, nullptr, nullptr, 0, 5, 0.8, 64, out.data(), 8, &n) == MVO_OK && n == 0);
    const int32_t none_i[2] = {-1, -1}, none_d[2] = {M, M};
    CHECK(guided_filter_matches(ctx, none_i, none_d, 1, 0, 0.8, 64, nullptr, 0, &n) == MVO_OK && n == 0);
    CHECK(guided_filter_matches(ctx, nullptr, nullptr, 0, 0, 0.8, 64, nullptr, 0, &n) == MVO_OK && n == 0);
    // a single candidate passes on the ceiling alone: at it, and above it
    const int32_t one_i[4] = {2, -1, 1, -1}, one_d[4] = {64, M, 65, M};
    CHECK(guided_filter_matches(ctx, one_i, one_d, 2, 3, 0.8, 64, out.data(), 8, &n) == MVO_OK && n == 1);
    CHECK(out[0].queryIdx == 0 && out[0].trainIdx == 2 && out[0].imgIdx == 0 && out[0].distance == 64.f);
    // ties: queries 0, 1, 2 claim train 1 at distances 7, 5, 5 -> the lower query of the nearer two; query 3 fails the ratio
    // on equal distances (5 < 1.0 * 5 is false); query 4 takes the last train
    const int32_t tie_i[10] = {1, 0, 1, 0, 1, 0, 0, 2, 3, 0}, tie_d[10] = {7, 90, 5, 90, 5, 90, 5, 5, 9, 200};
    CHECK(guided_filter_matches(ctx, tie_i, tie_d, 5, 4, 1.0, 64, out.data(), 8, &n) == MVO_OK && n == 2);
    CHECK(out[0].queryIdx == 1 && out[0].trainIdx == 1 && out[0].distance == 5.f && out[1].queryIdx == 4 && out[1].trainIdx == 3);
    // the buffer is too small, or missing: the count is still reported
    CHECK(guided_filter_matches(ctx, tie_i, tie_d, 5, 4, 1.0, 64, out.data(), 1, &n) == MVO_ERR_CAPACITY && n == 2);
    CHECK(guided_filter_matches(ctx, tie_i, tie_d, 5, 4, 1.0, 64, nullptr, 8, &n) == MVO_ERR_CAPACITY && ctx->err == "match buffer too small");
    // the train checks
    const float good[3] = {1.f, 1.2f, 0.f}, neg[3] = {1.f, -1.f, 1.f}, nan[3] = {1.f, 1.f, NAN};
    CHECK(guided_check_trains(ctx, "f", nullptr, 65535) == MVO_OK && guided_check_trains(ctx, "f", good, 3) == MVO_OK);
    CHECK(guided_check_trains(ctx, "f", nullptr, 0) == MVO_OK && guided_check_trains(ctx, "f", neg, 1) == MVO_OK);
    CHECK(guided_check_trains(ctx, "f", good, 65536) == MVO_ERR_CAPACITY && ctx->err == "f: more than 65535 train descriptors");
    CHECK(guided_check_trains(ctx, "g", neg, 3) == MVO_ERR_INVALID && ctx->err == "g: t_scale entry negative or not finite");
    CHECK(guided_check_trains(ctx, "g", nan, 3) == MVO_ERR_INVALID);
    CHECK(guided_tol2(2.0, nullptr, 1) == 4.0 && guided_tol2(2.0, good, 1) == (2.0 * (double)1.2f) * (2.0 * (double)1.2f));
    // the scratch: first use, a smaller request, regrow past the floor, release (twice)
    GuidedScratch s;
    s.release();
    CHECK(s.ensure(ctx, 64) == MVO_OK && s.cap == 4096 && s.d_part);
    CHECK((char*)s.d_part_cnt == (char*)s.d_part + GK_MAX_GROUPS * 4096 * 8 && (char*)s.d_arrive == (char*)s.d_part_cnt + GK_MAX_GROUPS * 4096 * 4);
    (void)hipStreamSynchronize(ctx->stream);
    for (int g = 0; g < 4096 / 64 + 2; ++g) CHECK(s.d_arrive[g] == 0);
    std::memset(s.d_part, 0xab, GK_MAX_GROUPS * 4096 * 12 + (4096 / 64 + 2) * 4);  // every byte of the block is ours
    const unsigned long long* first = s.d_part;
    CHECK(s.ensure(ctx, 4096) == MVO_OK && s.d_part == first && s.cap == 4096);
    CHECK(s.ensure(ctx, 4200) == MVO_OK && s.cap == 6300);
    (void)hipStreamSynchronize(ctx->stream);
    for (int g = 0; g < 6300 / 64 + 2; ++g) CHECK(s.d_arrive[g] == 0);
    std::memset(s.d_part, 0xcd, GK_MAX_GROUPS * (size_t)6300 * 12 + (6300 / 64 + 2) * 4);
    const GuidedPartials p = s.partials();
    CHECK(p.key == s.d_part && p.cnt == s.d_part_cnt && p.arrive == s.d_arrive);
    s.release();
    CHECK(!s.d_part && !s.d_part_cnt && !s.d_arrive && s.cap == 0);
    s.release();
    delete ctx;
    std::printf("guided_host_check ok\n");
    return 0;
}
