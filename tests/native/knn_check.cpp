// knn_check.cpp — the host yardstick of the k-nearest-neighbour queries (csrc/gicp_hostmath.cpp gicp_knn_host,
// DESIGN.md §3r) exercised on the CPU: tests/test_knn_native_cpu.py links this file with gicp_hostmath.cpp by the
// host compiler alone, under the address and undefined-behaviour sanitizers, and runs it as a child process.  Each
// case is checked against a full sort of all rows by (d2, index) with the same distance function (gicp_filter.h).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../generalized-icp_amd/csrc/gicp_filter.h"
#include "../../include/gicp_hip.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAIL %s\n", what);
        ++failures;
    }
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
double uniform(double lo, double hi) {   // xorshift64*: the clouds are the same on every run
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    const uint64_t r = rng_state * 0x2545F4914F6CDD1Dull;
    return lo + (hi - lo) * (double)(r >> 11) * (1.0 / 9007199254740992.0);
}

template <int D>
std::vector<double> cloud(int64_t n, double half) {
    std::vector<double> p((size_t)n * D);
    for (auto& v : p) v = uniform(-half, half);
    return p;
}

// queries == nullptr: a self-query
template <int D>
void run_case(const char* name, const std::vector<double>& p, const std::vector<double>* qs, int k, double maxd) {
    const int64_t M = (int64_t)p.size() / D;
    const std::vector<double>& q = qs ? *qs : p;
    const int64_t Q = (int64_t)q.size() / D;
    const double lim = maxd > 0.0 ? maxd * maxd : std::numeric_limits<double>::infinity();
    // exactly-sized outputs: a write past their end is the sanitizer's to find
    std::vector<int64_t> index((size_t)Q * k);
    std::vector<double> d2((size_t)Q * k);
    std::vector<int32_t> count((size_t)Q);
    const int rc = gicp_knn_host(p.data(), M, qs ? q.data() : nullptr, qs ? Q : 0, D, k, maxd, index.data(), d2.data(),
                                 count.data());
    bool ok = rc == GICP_OK;
    std::vector<std::pair<double, int64_t>> all((size_t)M);
    int64_t kept = 0;
    for (int64_t i = 0; ok && i < Q; ++i) {
        for (int64_t j = 0; j < M; ++j) all[j] = {gicp::filter_d2<D>(&p[j * D], &q[i * D]), j};
        std::sort(all.begin(), all.end());   // (d2, index), ascending
        int n = 0;
        while (n < k && n < M && all[n].first <= lim) ++n;
        ok = count[i] == n;
        for (int m = 0; ok && m < k; ++m) {
            const double wd = m < n ? all[m].first : std::numeric_limits<double>::infinity();
            const int64_t wi = m < n ? all[m].second : -1;
            ok = index[i * k + m] == wi && std::memcmp(&d2[i * k + m], &wd, sizeof wd) == 0;
        }
        kept += n;
    }
    // the optional outputs
    ok = ok && gicp_knn_host(p.data(), M, qs ? q.data() : nullptr, qs ? Q : 0, D, k, maxd, nullptr, nullptr, nullptr) == GICP_OK;
    expect(ok, name);
    if (ok) std::printf("ok %s_%dd %lld queries, %lld entries\n", name, D, (long long)Q, (long long)kept);
}

template <int D>
void cases() {
    const std::vector<double> p = cloud<D>(700, 5.0), q = cloud<D>(130, 6.0);
    run_case<D>("random_k8", p, &q, 8, 0.0);
    run_case<D>("random_k1", p, &q, 1, 0.0);
    run_case<D>("random_k32_radius", p, &q, 32, 1.5);
    run_case<D>("self_k20", p, nullptr, 20, 0.0);
    // fewer rows than k: pads and counts
    const std::vector<double> few = cloud<D>(5, 1.0);
    run_case<D>("few_rows_k8", few, &q, 8, 0.0);
    run_case<D>("one_row_k32", cloud<D>(1, 1.0), &q, 32, 0.0);
    // exact ties: the integer lattice in reversed row order, queries at points, edge midpoints and cell centres,
    // the bound exactly on a shell
    std::vector<double> lat, lq;
    for (int i = 5 * 5 * (D == 3 ? 5 : 1) - 1; i >= 0; --i) {
        const int c[3] = {i % 5, (i / 5) % 5, i / 25};
        for (int a = 0; a < D; ++a) lat.push_back((double)c[a]);
    }
    for (int t = 0; t < 3; ++t)
        for (int a = 0; a < D; ++a) lq.push_back(t == 0 ? 2.0 : t == 1 ? (a == 0 ? 1.5 : 2.0) : 1.5);
    run_case<D>("lattice_k3", lat, &lq, 3, 0.0);
    run_case<D>("lattice_k9_on_the_bound", lat, &lq, 9, 1.0);
    run_case<D>("lattice_self", lat, nullptr, 2 * D + 2, 0.0);
    // 70 coincident rows
    std::vector<double> co = cloud<D>(40, 2.0);
    for (int i = 0; i < 70 * D; ++i) co.push_back(0.375);
    run_case<D>("coincident_k32", co, nullptr, 32, 0.0);
    // refusals write nothing and leave a message
    std::vector<int64_t> index(8, 77);
    std::vector<double> bad = q;
    bad[3] = std::nan("");
    bool ok = gicp_knn_host(p.data(), 700, bad.data(), 4, D, 2, 0.0, index.data(), nullptr, nullptr) == GICP_E_INVALID &&
              std::strstr(gicp_last_host_error(), "non-finite") != nullptr;
    ok = ok && gicp_knn_host(p.data(), 700, q.data(), 4, D, 0, 0.0, index.data(), nullptr, nullptr) == GICP_E_INVALID;
    ok = ok && gicp_knn_host(p.data(), 700, q.data(), 4, D, 33, 0.0, index.data(), nullptr, nullptr) == GICP_E_INVALID;
    ok = ok && gicp_knn_host(p.data(), 700, q.data(), 0, D, 2, 0.0, index.data(), nullptr, nullptr) == GICP_E_INVALID;
    ok = ok && gicp_knn_host(p.data(), 700, q.data(), 4, D, 2, -1.0, index.data(), nullptr, nullptr) == GICP_E_INVALID;
    ok = ok && gicp_knn_host(p.data(), 0, q.data(), 4, D, 2, 0.0, index.data(), nullptr, nullptr) == GICP_E_INVALID;
    ok = ok && gicp_knn_host(p.data(), 700, q.data(), 4, 4, 2, 0.0, index.data(), nullptr, nullptr) == GICP_E_INVALID;
    for (int64_t v : index) ok = ok && v == 77;
    expect(ok, "refused");
    if (ok) std::printf("ok refused_%dd\n", D);
}

}  // namespace

int main() {
    cases<2>();
    cases<3>();
    if (failures) std::printf("FAILED %d\n", failures);
    else std::printf("PASS\n");
    return failures ? 1 : 0;
}
