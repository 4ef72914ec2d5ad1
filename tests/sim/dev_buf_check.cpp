// tests/sim/dev_buf_check.cpp -- TEST AID, a program of its own for a sanitizer build of DevBuf (csrc/mvo_internal.h) on the CPU
// (dev_buf_check.mk), with the device allocations served by hip_emu/ (its hipMalloc is aligned_alloc, so a block that is
// dropped is a leak LeakSanitizer reports, and a write past a block an AddressSanitizer error).  For both ensure flavours: first
// use, a smaller request, growth one past the capacity, every byte of the new block, release (twice); then a struct of several
// buffers deleted with live blocks.  Prints "dev_buf_check ok" and returns 0.
#include <cstdio>
#include <cstring>

#include "mvo_internal.h"

// what DevBuf takes from the other translation units of the library
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

struct Several {  // as the state structs hold them
    DevBuf<double> a, b;
    DevBuf<uint8_t> c;
    DevBuf<int32_t> never_used;
};

int main() {
    mvo_ctx* ctx = new mvo_ctx();
    // ensure: max(floor, n + n / 2) elements when it grows
    DevBuf<double> g;
    g.release();
    CHECK(!g.p && g.cap == 0);
    CHECK(g.ensure(ctx, 0, 4096) == MVO_OK && !g.p && g.cap == 0);  // nothing asked, nothing allocated
    CHECK(g.ensure(ctx, 64, 4096) == MVO_OK && g.p && g.cap == 4096);
    std::memset(g.p, 0xab, 4096 * sizeof(double));
    const double* first = g.p;
    CHECK(g.ensure(ctx, 1, 4096) == MVO_OK && g.ensure(ctx, 4096, 4096) == MVO_OK && g.p == first && g.cap == 4096);
    CHECK(g.ensure(ctx, 4097, 4096) == MVO_OK && g.cap == 4097 + 2048);
    std::memset(g.p, 0xcd, (size_t)6145 * sizeof(double));
    CHECK(g.ensure(ctx, 6145, 4096) == MVO_OK && g.cap == 6145);
    CHECK(g.ensure(ctx, 6146, 4096) == MVO_OK && g.cap == 6146 + 3073);
    std::memset(g.p, 0xef, (size_t)9219 * sizeof(double));
    CHECK((double*)g == g.p);
    g.release();
    CHECK(!g.p && g.cap == 0);
    g.release();
    // ensure_exact: what is asked plus the padding bytes
    DevBuf<int32_t> e;
    CHECK(e.ensure_exact(ctx, 1000, 64) == MVO_OK && e.p && e.cap == 1000);
    std::memset(e.p, 0x11, 1000 * sizeof(int32_t) + 64);
    const int32_t* efirst = e.p;
    CHECK(e.ensure_exact(ctx, 999, 64) == MVO_OK && e.ensure_exact(ctx, 1000) == MVO_OK && e.p == efirst && e.cap == 1000);
    CHECK(e.ensure_exact(ctx, 1001, 64) == MVO_OK && e.cap == 1001);
    std::memset(e.p, 0x22, 1001 * sizeof(int32_t) + 64);
    CHECK(e.ensure_exact(ctx, 12) == MVO_OK && e.cap == 1001);
    e.release();
    CHECK(!e.p && e.cap == 0);
    e.release();
    // the owners: a struct deleted with live buffers leaves nothing behind, and so does a buffer that goes out of scope
    Several* s = new Several();
    CHECK(s->a.ensure(ctx, 10, 128) == MVO_OK && s->b.ensure_exact(ctx, 7) == MVO_OK && s->c.ensure(ctx, 5000, 4096) == MVO_OK);
    CHECK(s->a.cap == 128 && s->b.cap == 7 && s->c.cap == 7500 && !s->never_used.p);
    std::memset(s->c.p, 0x33, 7500);
    delete s;
    {
        DevBuf<uint8_t> scoped;
        CHECK(scoped.ensure_exact(ctx, 100, 64) == MVO_OK);
        std::memset(scoped.p, 0x44, 164);
    }
    delete ctx;
    std::printf("dev_buf_check ok\n");
    return 0;
}
