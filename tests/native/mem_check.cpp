// mem_check.cpp — the owning buffers of csrc/gicp_mem.h exercised on the CPU (tests/test_mem_cpu.py builds this
// with the address and undefined-behaviour sanitizers and runs it).  The four seam functions are defined here
// on malloc / free with counters and a switch that makes the k-th allocation fail, so growth, failure, moves,
// swaps and allocate-initialise-publish are checked where a fault costs nothing.  Prints one "ok <case>" line
// per case and "PASS" at the end; any failed check prints "FAIL ..." and the exit status is 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "../../generalized-icp_amd/csrc/gicp_mem.h"
#include "../../include/gicp_hip.h"

namespace {
long n_alloc = 0, n_free = 0, live_bytes = 0;
long fail_at = 0;                      // > 0: the allocation with this ordinal (n_alloc + 1) throws
std::map<void*, size_t> live;          // block -> bytes
int failures = 0;

void* counted_alloc(size_t bytes, const char* what) {
    if (fail_at && n_alloc + 1 == fail_at) {
        fail_at = 0;
        throw gicp::Fail{GICP_E_HIP, std::string(what) + ": out of memory (injected)"};
    }
    void* p = std::malloc(bytes);
    if (!p) std::abort();
    ++n_alloc;
    live[p] = bytes;
    live_bytes += (long)bytes;
    return p;
}
void counted_free(void* p) {
    auto it = live.find(p);
    if (it == live.end()) {
        std::printf("FAIL free of a block that is not live\n");
        ++failures;
        return;
    }
    live_bytes -= (long)it->second;
    live.erase(it);
    ++n_free;
    std::free(p);
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++failures;                                                    \
        }                                                                  \
    } while (0)
}  // namespace

namespace gicp {
void* dev_alloc(size_t bytes) { return counted_alloc(bytes, "hipMalloc"); }
void dev_free(void* p) noexcept { counted_free(p); }
void* pinned_alloc(size_t bytes) { return counted_alloc(bytes, "hipHostMalloc"); }
void pinned_free(void* p) noexcept { counted_free(p); }
}  // namespace gicp

using gicp::DevBuf;
using gicp::PinnedBuf;

namespace {

// the rule of DevBuf::reserve, restated: n <= cap keeps the buffer, else max(n, floor(cap * 1.125), 1)
template <class Buf>
void growth_policy() {
    const size_t req[] = {100, 50, 100, 101, 0, 112, 113, 114, 127, 128, 1000, 1, 1125, 1126, 0};
    Buf b;
    CHECK(b.empty() && b.capacity() == 0 && b.get() == nullptr);
    size_t cap = 0;
    long allocs = 0;
    bool held = false;
    const long a0 = n_alloc;
    for (size_t n : req) {
        if (!(held && n <= cap)) {
            size_t want = n;
            if ((size_t)(cap * 1.125) > want) want = (size_t)(cap * 1.125);
            if (want < 1) want = 1;
            cap = want;
            held = true;
            ++allocs;
        }
        b.reserve(n);
        CHECK(b.capacity() == cap);
        CHECK(!b.empty() && live.count(b.get()) && live[b.get()] == cap * sizeof(*b.get()));
        CHECK(n_alloc - a0 == allocs);
        CHECK((long)live.size() == 1);   // the old block is freed before the new one is taken
        std::memset(b.get(), 0xA5, b.capacity() * sizeof(*b.get()));   // the whole capacity is writable
    }
    CHECK(allocs == 7);   // 100, 112 (101), 126 (113), 141 (127), 1000, 1125, 1265 (1126)
    // a first reserve of 0 takes one element, and the exact form takes exactly what it is asked for
    Buf z;
    z.reserve(0);
    CHECK(z.capacity() == 1 && !z.empty());
    z.alloc(40);
    CHECK(z.capacity() == 40);
    z.alloc(7);
    CHECK(z.capacity() == 7 && live[z.get()] == 7 * sizeof(*z.get()));
    z.alloc(0);
    CHECK(z.capacity() == 1);
}

void failure_injection() {
    const long live0 = (long)live.size();
    DevBuf<double> b;
    for (int form = 0; form < 2; ++form) {   // reserve, then the exact form
        // the first allocation fails
        fail_at = n_alloc + 1;
        int code = 0;
        try {
            form ? b.alloc(64) : b.reserve(64);
        } catch (const gicp::Fail& f) {
            code = f.code;
            CHECK(!f.msg.empty());
        }
        CHECK(code == GICP_E_HIP);
        CHECK(b.empty() && b.capacity() == 0 && b.get() == nullptr);
        CHECK((long)live.size() == live0);
        form ? b.alloc(64) : b.reserve(64);   // the same request again succeeds
        CHECK(!b.empty() && b.capacity() == 64);
        // a growing allocation fails: the old block is gone (freed first) and no capacity is left behind
        fail_at = n_alloc + 1;
        code = 0;
        try {
            form ? b.alloc(1000) : b.reserve(1000);
        } catch (const gicp::Fail& f) {
            code = f.code;
        }
        CHECK(code == GICP_E_HIP);
        CHECK(b.empty() && b.capacity() == 0);
        CHECK((long)live.size() == live0);
        b.reserve(10);   // a smaller request than the lost capacity still allocates: nothing stale skips it
        CHECK(!b.empty() && b.capacity() == 10);
        form ? b.alloc(1000) : b.reserve(1000);
        CHECK(b.capacity() == 1000);
        b.reset();
        CHECK(b.empty() && b.capacity() == 0 && (long)live.size() == live0);
    }
}

struct TwoClouds {   // as Cloud: plain fields beside several buffers of different element types and sizes
    int64_t n = 0;
    DevBuf<double> xyz;
    DevBuf<int32_t> perm, inv;
    PinnedBuf<float> host;
    void build(int64_t np) {
        xyz.reserve((size_t)np * 4);
        perm.reserve((size_t)np);
        inv.reserve((size_t)np);
        host.reserve((size_t)np / 2);
        n = np;
    }
};

void moves_and_swaps() {
    const long live0 = (long)live.size(), f0 = n_free;
    DevBuf<int32_t> a;
    a.reserve(10);
    int32_t* pa = a.get();
    DevBuf<int32_t> b(std::move(a));   // move construction
    CHECK(a.empty() && a.capacity() == 0 && b.get() == pa && b.capacity() == 10);
    CHECK(n_free == f0);
    DevBuf<int32_t> c;
    c.reserve(20);
    int32_t* pc = c.get();
    c = std::move(b);                  // move assignment onto a non-empty buffer: its block is freed once
    CHECK(n_free == f0 + 1 && !live.count(pc));
    CHECK(b.empty() && c.get() == pa && c.capacity() == 10);
    std::swap(c, c);                   // self-swap keeps the block
    CHECK(c.get() == pa && c.capacity() == 10 && live.count(pa) && n_free == f0 + 1);
    int32_t* raw = c;                  // the implicit conversion launch sites use
    CHECK(raw == pa && !!c && !b);
    c.reset();
    CHECK((long)live.size() == live0);

    TwoClouds s, t;
    s.build(100);
    t.build(300);
    double* sx = s.xyz;
    double* tx = t.xyz;
    const long before = (long)live.size(), fr = n_free, al = n_alloc;
    std::swap(s, t);                   // the one-line swap of gicp_target_to_source / gicp_commit_target
    CHECK(n_free == fr && n_alloc == al && (long)live.size() == before);
    CHECK(s.n == 300 && t.n == 100 && s.xyz.get() == tx && t.xyz.get() == sx);
    CHECK(s.xyz.capacity() == 1200 && t.xyz.capacity() == 400 && s.host.capacity() == 150 && t.perm.capacity() == 100);
    t.n = 0;                           // the side that keeps spare buffers ...
    t.build(120);                      // ... grows them for the next cloud: four blocks freed, four taken
    CHECK(n_free == fr + 4 && n_alloc == al + 4 && (long)live.size() == before);
    CHECK(t.xyz.capacity() == 480 && t.perm.capacity() == 120 && t.host.capacity() == 60);
    s.build(250);                      // fits: nothing happens
    CHECK(n_alloc == al + 4 && s.xyz.get() == tx);
}

struct Owner {
    DevBuf<uint32_t> tickets;
    PinnedBuf<double> state;
};

void publish_after_init() {
    const long live0 = (long)live.size();
    Owner o;
    // the product's pattern, with the initialisation failing: the member stays empty, the local's block is freed
    int code = 0;
    try {
        if (!o.tickets)
            gicp::alloc_init(o.tickets, 128, [](uint32_t*) { throw gicp::Fail{GICP_E_HIP, "hipMemsetAsync: injected"}; });
    } catch (const gicp::Fail& f) {
        code = f.code;
    }
    CHECK(code == GICP_E_HIP && o.tickets.empty() && o.tickets.capacity() == 0);
    CHECK((long)live.size() == live0);
    // the allocation itself failing leaves the same state
    fail_at = n_alloc + 1;
    code = 0;
    try {
        if (!o.state) gicp::alloc_init(o.state, 8, [](double* h) { std::memset(h, 0, sizeof(double) * 8); });
    } catch (const gicp::Fail& f) {
        code = f.code;
    }
    CHECK(code == GICP_E_HIP && o.state.empty() && (long)live.size() == live0);
    // the next call redoes the block and publishes initialised contents
    if (!o.tickets) gicp::alloc_init(o.tickets, 128, [](uint32_t* d) { std::memset(d, 0, sizeof(uint32_t) * 128); });
    if (!o.state) gicp::alloc_init(o.state, 8, [](double* h) { std::memset(h, 0, sizeof(double) * 8); });
    CHECK(o.tickets.capacity() == 128 && o.state.capacity() == 8 && (long)live.size() == live0 + 2);
    bool zero = true;
    for (int i = 0; i < 128; ++i) zero = zero && o.tickets[i] == 0;
    for (int i = 0; i < 8; ++i) zero = zero && o.state[i] == 0.0;
    CHECK(zero);
}

template <class F>
void run(const char* name, F&& f) {
    const int before = failures;
    f();
    if ((long)live.size() != 0 || live_bytes != 0) {
        std::printf("FAIL %s: %ld blocks, %ld bytes live after the case\n", name, (long)live.size(), live_bytes);
        ++failures;
    }
    if (failures == before) std::printf("ok %s\n", name);
}

}  // namespace

int main() {
    run("growth_policy_device", growth_policy<DevBuf<double>>);
    run("growth_policy_pinned", growth_policy<PinnedBuf<int32_t>>);
    run("failure_injection", failure_injection);
    run("moves_and_swaps", moves_and_swaps);
    run("publish_after_init", publish_after_init);
    std::printf("allocations %ld frees %ld live blocks %ld live bytes %ld\n", n_alloc, n_free, (long)live.size(), live_bytes);
    if (n_alloc != n_free || live_bytes != 0 || !live.empty()) {
        std::printf("FAIL leak\n");
        ++failures;
    }
    std::printf(failures ? "FAILED %d\n" : "PASS\n", failures);
    return failures ? 1 : 0;
}
