// host_check.cpp — the host-only unit of the library (csrc/gicp_hostmath.cpp) exercised on the CPU: the tiling and
// its thread pool, the shard split, the accept threshold and the host scans.  tests/test_host_cpu.py builds this
// with gicp_hostmath.cpp, once under the address and undefined-behaviour sanitizers and once under the thread
// sanitizer, and runs it.  Prints one "ok <case>" line per case and "PASS" at the end; any failed check prints
// "FAIL ..." and the exit status is 1.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <memory>
#include <vector>

#include "../../generalized-icp_amd/csrc/gicp_hostmath.h"

using namespace gicp;

namespace {
int failures = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (failures < 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;   // fixed seed: the same inputs in every run
double uniform() {                            // xorshift64*, 53 bits
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0);
}

// the kernels' Morton code of grid cell g (axis a on bits a, a + dim, ...), and its inverse per axis
uint32_t morton(const uint32_t* g, int dim, int bits) {
    uint32_t c = 0;
    for (int b = 0; b < bits; ++b)
        for (int a = 0; a < dim; ++a) c |= ((g[a] >> b) & 1u) << (b * dim + a);
    return c;
}
int cell(uint32_t code, int a, int dim, int bits) {
    int g = 0;
    for (int b = 0; b < bits; ++b) g |= (int)((code >> (b * dim + a)) & 1u) << b;
    return g;
}

// sorted codes of n points: dist 0 uniform, 1 a thin slab (the last axis in 0.5 .. 0.501), 2 cubed uniform
std::vector<uint32_t> make_codes(int dim, int dist, int n) {
    const int bits = dim == 3 ? 10 : 16;
    std::vector<uint32_t> codes((size_t)n);
    for (auto& c : codes) {
        uint32_t g[3] = {0, 0, 0};
        for (int a = 0; a < dim; ++a) {
            double u = uniform();
            if (dist == 1 && a == dim - 1) u = 0.5 + 0.001 * u;
            if (dist == 2) u = u * u * u;
            g[a] = std::min<uint32_t>((1u << bits) - 1, (uint32_t)std::ldexp(u, bits));
        }
        c = morton(g, dim, bits);
    }
    std::sort(codes.begin(), codes.end());
    return codes;
}

struct Table {
    std::vector<int32_t> start, count;
    std::vector<uint32_t> first_code;
    int cap = -1;
    bool operator==(const Table& o) const {
        return cap == o.cap && start == o.start && count == o.count && first_code == o.first_code;
    }
};
Table build(const std::vector<uint32_t>& codes, int dim, int maxp, int hint, WorkerPool& pool) {
    Table t;
    t.start = {7, 7};   // stale contents must not survive
    build_tile_table(codes, dim, dim == 3 ? 10 : 16, t.start, t.count, t.first_code, t.cap, hint, pool, maxp);
    return t;
}

template <class F>
void for_each_input(F&& f) {
    rng_state = 0x9E3779B97F4A7C15ull;
    for (int dim = 2; dim <= 3; ++dim)
        for (int dist = 0; dist < 3; ++dist)
            for (int n : {1, 63, 64, 65, 1000, 20000}) {
                const std::vector<uint32_t> codes = make_codes(dim, dist, n);
                for (int maxp : {64, 32, 16}) f(codes, dim, maxp);
            }
}

void tiling_partition() {
    WorkerPool pool(7);
    for_each_input([&](const std::vector<uint32_t>& codes, int dim, int maxp) {
        const int bits = dim == 3 ? 10 : 16;
        const int64_t n = (int64_t)codes.size();
        const Table t = build(codes, dim, maxp, 0, pool);
        const size_t nt = t.start.size();
        CHECK(nt > 0 && t.count.size() == nt && t.first_code.size() == nt);
        CHECK(t.cap >= 0 && t.cap <= 4 * (bits - 1));
        const int cap = tile_cap_of(t.cap);
        int64_t next = 0;
        for (size_t k = 0; k < nt && next <= n; ++k) {
            CHECK(t.start[k] == next);                          // contiguous, in order
            CHECK(t.count[k] >= 1 && t.count[k] <= maxp);
            if (t.start[k] != next || t.count[k] < 1 || next + t.count[k] > n) break;
            CHECK(t.first_code[k] == codes[(size_t)next]);
            for (int a = 0; a < dim; ++a) {
                int lo = 1 << 30, hi = -1;
                for (int64_t i = next; i < next + t.count[k]; ++i) {
                    const int g = cell(codes[(size_t)i], a, dim, bits);
                    lo = std::min(lo, g);
                    hi = std::max(hi, g);
                }
                CHECK(hi - lo <= cap);
            }
            next += t.count[k];
        }
        CHECK(next == n);                                       // ... and they cover [0, n)
        CHECK((int64_t)nt <= (int64_t)(1.35 * std::ceil(n / (double)maxp)) + 2 || t.cap == 4 * (bits - 1));
    });
}

void tiling_independent_of_hint_and_threads() {
    WorkerPool none(0), seven(7);
    for_each_input([&](const std::vector<uint32_t>& codes, int dim, int maxp) {
        const int kmax = 4 * ((dim == 3 ? 10 : 16) - 1);
        const Table ref = build(codes, dim, maxp, 0, none);
        int turn = 0;
        for (int h : {1, ref.cap - 2, ref.cap - 1, ref.cap, ref.cap + 1, ref.cap + 2, kmax - 1, kmax, kmax + 1}) {
            const int hint = std::max(0, std::min(kmax + 1, h));
            CHECK(build(codes, dim, maxp, hint, turn++ % 2 ? none : seven) == ref);
        }
    });
}

void worker_pool() {
    for (int workers : {0, 1, 7}) {
        WorkerPool pool(workers);
        for (int n : {0, 1, 3, 16, 1000}) {
            // plain ints: a task run twice at once, or after run() has returned, is a data race the thread
            // sanitizer reports; one run twice in turn shows in the count
            std::vector<int> hits((size_t)n, 0);
            int outside = 0;
            for (int gen = 1; gen <= 200; ++gen) {
                pool.run(n, [&](int k) {
                    if (k < 0 || k >= n) ++outside;
                    else ++hits[(size_t)k];
                });
                bool once = true;
                for (int k = 0; k < n; ++k) once = once && hits[(size_t)k] == gen;
                CHECK(once);
            }
            CHECK(outside == 0);
        }
    }
}

void shard_tile_count_case() {
    constexpr int kChunkTiles = kShardChunk * kCorrWaves;
    for (int nshards = 1; nshards <= 5; ++nshards)
        for (int ntiles : {0, 1, 63, 64, 65, 3 * kChunkTiles + 1}) {
            int sum = 0;
            for (int shard = 0; shard < nshards; ++shard) {
                int direct = 0;
                for (int t = 0; t < ntiles; ++t) direct += (t / kChunkTiles) % nshards == shard;
                const int got = shard_tile_count(ntiles, shard, nshards);
                CHECK(got == direct);
                sum += got;
            }
            CHECK(sum == ntiles);
        }
}

void accept_d2_max_case() {
    const double inf = std::numeric_limits<double>::infinity();
    for (double dc : {0.0, 5e-324, 1e-160, 0.1, 0.5, 1.0, 150.0, 1e160}) {
        const double x = accept_d2_max(dc);
        CHECK(std::sqrt(x) <= dc);
        CHECK(dc < std::sqrt(std::nextafter(x, inf)));
    }
    CHECK(accept_d2_max(inf) == inf);
    CHECK(std::isnan(accept_d2_max(std::nan(""))));
}

template <class F>
int code_thrown(F&& f) {
    try {
        f();
    } catch (const Fail& e) {
        return e.msg.empty() ? -1000 : e.code;
    }
    return GICP_OK;
}

void scan_bounds_case() {
    const double bad[3] = {std::nan(""), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()};
    for (int dim = 2; dim <= 3; ++dim) {
        const int n = 257;
        std::vector<double> xyz((size_t)n * dim);
        for (auto& v : xyz) v = 200.0 * uniform() - 100.0;
        double mn[3], mx[3];
        scan_bounds(xyz.data(), n, dim, mn, mx);
        for (int a = 0; a < 3; ++a) {
            double lo = 0.0, hi = 0.0;   // an axis the cloud does not have reads 0
            for (int i = 0; a < dim && i < n; ++i) {
                lo = i ? std::min(lo, xyz[(size_t)i * dim + a]) : xyz[a];
                hi = i ? std::max(hi, xyz[(size_t)i * dim + a]) : xyz[a];
            }
            CHECK(mn[a] == lo && mx[a] == hi);
        }
        scan_bounds(xyz.data(), 1, dim, mn, mx);   // one row: its own bounds
        CHECK(mn[0] == xyz[0] && mx[dim - 1] == xyz[(size_t)dim - 1]);
        for (int row : {0, n - 1})
            for (int a = 0; a < dim; ++a)
                for (double b : bad) {
                    std::vector<double> v = xyz;
                    v[(size_t)row * dim + a] = b;
                    CHECK(code_thrown([&] { scan_bounds(v.data(), n, dim, mn, mx); }) == GICP_E_INVALID);
                }
    }
    const int n = 100;
    std::vector<double> stamps((size_t)n);
    for (auto& s : stamps) s = uniform();
    CHECK(code_thrown([&] { scan_stamps(stamps.data(), n, 0.5); }) == GICP_OK);
    for (double b : bad) {
        CHECK(code_thrown([&] { scan_stamps(stamps.data(), n, b); }) == GICP_E_INVALID);
        for (int row : {0, n - 1}) {
            std::vector<double> s = stamps;
            s[(size_t)row] = b;
            CHECK(code_thrown([&] { scan_stamps(s.data(), n, 0.5); }) == GICP_E_INVALID);
        }
    }
}

template <class F>
void run(const char* name, F&& f) {
    const int before = failures;
    f();
    if (failures == before) std::printf("ok %s\n", name);
}

}  // namespace

int main() {
    run("tiling_partition", tiling_partition);
    run("tiling_independent_of_hint_and_threads", tiling_independent_of_hint_and_threads);
    run("worker_pool", worker_pool);
    run("shard_tile_count", shard_tile_count_case);
    run("accept_d2_max", accept_d2_max_case);
    run("scan_bounds", scan_bounds_case);
    std::printf(failures ? "FAILED %d\n" : "PASS\n", failures);
    return failures ? 1 : 0;
}
