// tests/sim/staged_call_check.cpp -- TEST AID, a program of its own for a sanitizer build of csrc/staged_call.h and of the
// FrameScratch / guided_pack_frames part of csrc/guided_match_host.h on the CPU (staged_call_check.mk), with the device and
// pinned allocations served by hip_emu/ (a dropped block is a leak LeakSanitizer reports, a write past one an AddressSanitizer
// error).  The block cursor; then begin / upload / finish and the scratch through four steps taken from the floors: below the
// floor, the first size above it, the first size above one and a half times that, small again.  Prints "staged_call_check ok"
// and returns 0.
#include <cstdio>
#include <cstring>
#include <vector>

#include "guided_match_host.h"

// what the headers take from the other translation units of the library
int mvo_set_err(mvo_ctx* c, int code, const char* what, hipError_t) {
    c->err = what;
    return code;
}
void ba_service_free(int, void* p, bool) { (void)hipFree(p); }
int mvo_ensure_pinned(mvo_ctx* ctx, size_t bytes) {  // exactly what is asked: a write past it is reported
    if (ctx->h_pin_cap >= bytes) return MVO_OK;
    if (ctx->h_pin) (void)hipHostFree(ctx->h_pin);
    ctx->h_pin = nullptr, ctx->h_pin_cap = 0;
    if (hipHostMalloc((void**)&ctx->h_pin, bytes, 0) != hipSuccess) return MVO_ERR_HIP;
    ctx->h_pin_cap = bytes;
    return MVO_OK;
}
static int g_gates_open = 0, g_collected = 0;
ExtractGate::ExtractGate(const mvo_ctx*) : device(0) { ++g_gates_open; }
void ExtractGate::release() {
    if (device >= 0) --g_gates_open;
    device = -1;
}
void mvo_prof_collect(mvo_ctx*) { ++g_collected; }

#define CHECK(x)                                                       \
    do {                                                               \
        if (!(x)) {                                                    \
            std::printf("line %d: %s is false\n", __LINE__, #x);       \
            return 1;                                                  \
        }                                                              \
    } while (0)

// one staged call of in_bytes up and out_bytes down: the parts of the pinned buffer, every byte of both and of d_in written
static int staged(mvo_ctx* ctx, DevBuf<uint8_t>& d_in, size_t in_bytes, size_t floor, size_t out_bytes, size_t want_cap, int step) {
    StagedCall call{ctx};
    CHECK(call.begin(d_in, in_bytes, floor, out_bytes) == MVO_OK);
    CHECK(d_in.cap == want_cap && call.h_out == ctx->h_pin && call.h_in == ctx->h_pin + out_bytes && call.in_bytes == in_bytes);
    CHECK(ctx->h_pin_cap >= out_bytes + in_bytes);
    std::memset(call.h_out, 0, out_bytes);
    for (size_t k = 0; k < in_bytes; ++k) call.h_in[k] = (uint8_t)(k * 7 + step);
    CHECK(call.upload(d_in) == MVO_OK);
    for (size_t k = 0; k < in_bytes; ++k) CHECK(d_in.p[k] == (uint8_t)(k * 7 + step));
    std::memset(d_in.p, 0x5a, d_in.cap);  // usable to its last byte
    ExtractGate gate(ctx);
    CHECK(g_gates_open == 1);
    const int collected = g_collected;
    CHECK(call.finish(gate) == MVO_OK && g_gates_open == 0 && g_collected == collected + (ctx->prof ? 1 : 0));
    return 0;
}

// part_bytes as DESIGN.md section 19 declares them: the key pairs padded to 64 bytes, the counts behind them
static size_t part_bytes(size_t rows_all, int ngroups) { return (rows_all * ngroups * 8 + 63) / 64 * 64 + rows_all * ngroups * 4; }

static int scratch_step(mvo_ctx* ctx, FrameScratch& s, size_t rows_all, int ngroups, size_t n_arrive, size_t want_part, size_t want_arrive,
                        bool reallocated) {
    const int32_t* before = s.d_arrive.p;
    CHECK(s.ensure(ctx, rows_all, ngroups, n_arrive) == MVO_OK);
    CHECK(s.d_part.cap == want_part && s.d_arrive.cap == want_arrive);
    (void)hipStreamSynchronize(ctx->stream);
    if (reallocated) {
        for (size_t k = 0; k < s.d_arrive.cap; ++k) CHECK(s.d_arrive.p[k] == 0);
    } else {
        CHECK(s.d_arrive.p == before && s.d_arrive.p[0] == 0x77777777);  // (left as the kernels re-arm them: not zeroed again)
    }
    const GuidedPartials p = s.partials();
    CHECK((uint8_t*)p.key == s.d_part.p && (uint8_t*)p.cnt == s.d_part.p + (rows_all * ngroups * 8 + 63) / 64 * 64 && p.arrive == s.d_arrive.p);
    CHECK((uint8_t*)(p.cnt + rows_all * ngroups) <= s.d_part.p + s.d_part.cap);
    std::memset(s.d_part.p, 0x66, s.d_part.cap);
    std::memset(s.d_arrive.p, 0x77, s.d_arrive.cap * sizeof(int32_t));
    return 0;
}

int main() {
    mvo_ctx* ctx = new mvo_ctx();
    CHECK(align64(0) == 0 && align64(1) == 64 && align64(64) == 64 && align64(65) == 128);
    // the cursor: blocks start on multiples of 64, the last one adds no padding
    BlockCursor c;
    CHECK(c.block(0) == 0 && c.bytes == 0);
    CHECK(c.block(96) == 0 && c.block(1) == 128 && c.block(64) == 192 && c.block(0) == 256 && c.last(5) == 256 && c.bytes == 261);
    BlockCursor fuse;  // map fusion's upload at 3 frames, 70 map points, 100 keypoints: table, masks, triples, descriptors
    CHECK(fuse.block(3 * sizeof(MapFuseFrame)) == 0 && fuse.block(70 * 8) == 384 && fuse.block(100 * 24) == 384 + 576 &&
          fuse.last(100 * 32) == 384 + 576 + 2432 && fuse.bytes == 384 + 576 + 2432 + 3200);
    // begin / upload / finish: floor 2^20 bytes, then max(floor, 1.5 n)
    const size_t F20 = (size_t)1 << 20, grown = F20 + 1, grown_cap = grown + grown / 2, regrown = grown_cap + 1;
    {
        DevBuf<uint8_t> d_in;
        if (staged(ctx, d_in, 1000, F20, 4096, F20, 1)) return 1;
        if (staged(ctx, d_in, F20, F20, 64, F20, 2)) return 1;
        ctx->prof = true;
        if (staged(ctx, d_in, grown, F20, 100, grown_cap, 3)) return 1;
        ctx->prof = false;
        if (staged(ctx, d_in, grown_cap, F20, 0, grown_cap, 4)) return 1;
        if (staged(ctx, d_in, regrown, F20, 64, regrown + regrown / 2, 5)) return 1;
        if (staged(ctx, d_in, 1000, F20, 4096, regrown + regrown / 2, 6)) return 1;
        DevBuf<uint8_t> small;  // pose optimisation's floor
        if (staged(ctx, small, 64 * 24, (size_t)1 << 16, 768, (size_t)1 << 16, 7)) return 1;
        if (staged(ctx, small, 65537, (size_t)1 << 16, 768, 65537 + 32768, 8)) return 1;
    }
    {  // also(): between d_in and the pinned buffer; its error ends begin
        DevBuf<uint8_t> d_in;
        StagedCall call{ctx};
        const uint8_t* pinned = ctx->h_pin;
        const size_t pinned_cap = ctx->h_pin_cap;
        CHECK(call.begin(d_in, 100, 4096, pinned_cap, [&] { return d_in.cap == 4096 ? (int)MVO_ERR_CAPACITY : (int)MVO_OK; }) == MVO_ERR_CAPACITY);
        CHECK(ctx->h_pin == pinned && ctx->h_pin_cap == pinned_cap && !call.h_in);
        // stage(): the pinned buffer alone
        CHECK(call.stage(pinned_cap, 100) == MVO_OK && ctx->h_pin_cap == pinned_cap + 100 && call.h_in == ctx->h_pin + pinned_cap);
        std::memset(call.h_out, 1, pinned_cap + 100);
    }
    {  // the scratch of the launches over every frame: d_part floor 2^18 bytes, d_arrive floor 4096 counters
        const size_t P18 = (size_t)1 << 18;
        size_t r1 = 64;
        while (part_bytes(r1, 1) <= P18) ++r1;  // the first rows_all whose partials pass the floor
        const size_t p1 = part_bytes(r1, 1), cap1 = p1 + p1 / 2;
        size_t r2 = r1;
        while (part_bytes(r2, 1) <= cap1) ++r2;  // ... and the first that passes what that grew to
        const size_t p2 = part_bytes(r2, 1);
        CHECK(part_bytes(r1 - 1, 1) <= P18 && part_bytes(r2 - 1, 1) <= cap1);
        FrameScratch s;
        if (scratch_step(ctx, s, 2 * 64, 1, 2, P18, 4096, true)) return 1;
        if (scratch_step(ctx, s, r1, 1, 4097, cap1, 4097 + 2048, true)) return 1;
        if (scratch_step(ctx, s, r2, 1, 6146, p2 + p2 / 2, 6146 + 3073, true)) return 1;
        if (scratch_step(ctx, s, 2 * 64, 1, 2, p2 + p2 / 2, 6146 + 3073, false)) return 1;
        if (scratch_step(ctx, s, 3 * 70, 3, 6, p2 + p2 / 2, 6146 + 3073, false)) return 1;  // the counts start behind padded keys
        // the partials alone grow: the counters stay as they are
        FrameScratch t;
        if (scratch_step(ctx, t, 64, 1, 1, P18, 4096, true)) return 1;
        if (scratch_step(ctx, t, r1, 1, 1, cap1, 4096, false)) return 1;
    }
    {  // the packing: two frames, the second empty, a third behind it
        const float xy0[4] = {1.5f, 2.5f, 3.f, 4.f}, xy2[2] = {7.f, 8.f}, sc0[2] = {1.f, 2.f};
        const int32_t conn0[2] = {-1, 5}, conn2[1] = {-1};
        std::vector<uint8_t> d0(64, 0x11), d2(32, 0x22);
        mvo_fuse_frame fr[3] = {};
        fr[0].n = 2, fr[0].desc = d0.data(), fr[0].xy = xy0, fr[0].scale = sc0, fr[0].conn = conn0;
        fr[2].n = 1, fr[2].desc = d2.data(), fr[2].xy = xy2, fr[2].conn = conn2;
        std::vector<double> tg(9, -7.0);
        std::vector<uint8_t> desc(96, 0);
        const std::vector<FrameSlice> at = guided_pack_frames(fr, 3, 2, tg.data(), desc.data(), [](const mvo_fuse_frame& F, int j) {
            return F.conn[j] == -1 ? guided_tol2(3.0, F.scale, j) : -1.0;
        });
        CHECK(at.size() == 3 && at[0].first == 0 && at[0].nt == 2 && at[0].slice == 1 && at[1].first == 2 && at[1].nt == 0 && at[1].slice == 0);
        CHECK(at[2].first == 2 && at[2].nt == 1 && at[2].slice == guided_slice(1, 2));
        const double want[9] = {1.5, 2.5, 9.0, 3.0, 4.0, -1.0, 7.0, 8.0, 9.0};
        CHECK(!std::memcmp(tg.data(), want, sizeof want));
        CHECK(desc[0] == 0x11 && desc[63] == 0x11 && desc[64] == 0x22 && desc[95] == 0x22);
    }
    (void)hipHostFree(ctx->h_pin);
    delete ctx;
    std::printf("staged_call_check ok\n");
    return 0;
}
