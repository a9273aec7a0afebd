// buffer_check — the failure contract of the owning buffers (csrc/rc_common.h: DevBuf, PinBuf),
// on a host WITHOUT a GPU, where every hipMalloc / hipHostMalloc fails cleanly.
//
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -g -O1 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=all -I include -I <pkg>/csrc tools/buffer_check.cpp -o buffer_check
//   buffer_check
//
// Links nothing of the library (rc::set_last_error is defined here).  Every allocation fails, so
// the program asserts what a failed reserve leaves behind, for both kinds: it throws rc::Error with
// RC_ERR_OOM, the buffer is empty, a second reserve throws again, g_alloc_count rose by one per
// attempt; reserve(0), reset, move and swap of empty buffers do nothing wrong; and a two-buffer
// workspace written zero / reserve / record reads size 0 afterwards.  Exit status 1 at the first
// miss, 2 if an allocation succeeds (a host with a device: the expectations are not for it).  The
// success paths are the GPU suite's.
#include <cstdio>
#include <cstdlib>

#include "rc_common.h"

void rc::set_last_error(const std::string &) {}

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

// reserve(n) must throw RC_ERR_OOM after exactly one counted attempt and leave b empty
template <typename B>
static void expect_oom(B &b, size_t n) {
    const int64_t before = rc::g_alloc_count.load();
    int code = RC_OK;
    try {
        b.reserve(n);
    } catch (const rc::Error &e) {
        code = e.code;
    }
    if (code == RC_OK) {
        std::fprintf(stderr, "an allocation succeeded: this host has a device\n");
        std::exit(2);
    }
    CHECK(code == RC_ERR_OOM);
    CHECK(rc::g_alloc_count.load() == before + 1);
    CHECK(b.get() == nullptr && b.capacity() == 0 && b.empty());
}

template <typename B>
static void check_kind() {
    B a, b;
    const int64_t before = rc::g_alloc_count.load();
    a.reserve(0);
    a.reset();
    CHECK(a.empty() && a.capacity() == 0 && rc::g_alloc_count.load() == before);
    expect_oom(a, 1000);
    expect_oom(a, 1000);  // not an early return on a stale capacity
    expect_oom(a, 1);
    B c(std::move(a));
    CHECK(c.empty() && c.capacity() == 0 && a.empty() && a.capacity() == 0);
    b = std::move(c);
    CHECK(b.empty() && c.empty());
    b.swap(a);
    CHECK(a.empty() && b.empty() && a.capacity() == 0 && b.capacity() == 0);
    expect_oom(b, 7);  // still usable after the moves
}

// A recorded size beside two buffers, as rc_index's ws_nq or BatchWs's caps: zero, reserve, record.
struct Workspace {
    int n = 0;
    rc::DevBuf<float> q;
    rc::PinBuf<uint64_t> keys;
    void ensure(int want) {
        if (want <= n) return;
        n = 0;
        q.reserve((size_t)want * 64);
        keys.reserve((size_t)want);
        n = want;
    }
};

int main() {
    check_kind<rc::DevBuf<float>>();
    check_kind<rc::PinBuf<float>>();
    check_kind<rc::DevBuf<void>>();
    CHECK(rc::min_capacity(rc::DevBuf<int>(), rc::PinBuf<int>()) == 0);
    Workspace ws;
    for (int round = 0; round < 2; ++round) {
        int code = RC_OK;
        try {
            ws.ensure(4);
        } catch (const rc::Error &e) {
            code = e.code;
        }
        CHECK(code == RC_ERR_OOM);
        CHECK(ws.n == 0 && ws.q.empty() && ws.keys.empty());
    }
    std::puts("buffer_check: ok");
    return 0;
}
