// sor_check.cpp — the host yardstick of statistical outlier removal (csrc/gicp_hostmath.cpp gicp_sor_points_host,
// DESIGN.md §3s) exercised on the CPU: tests/test_sor_native_cpu.py links this file with gicp_hostmath.cpp by the
// host compiler alone, under the address and undefined-behaviour sanitizers, and runs it as a child process.  Each
// case is checked against a full sort of every row's distances and the definition written out with the shared
// functions (gicp_filter.h, gicp_sor.h); the outputs are exactly sized.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../generalized-icp_amd/csrc/gicp_filter.h"
#include "../../generalized-icp_amd/csrc/gicp_sor.h"
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

// a uniform cloud, every 25th row pushed far out
template <int D>
std::vector<double> cloud(int64_t n, double half) {
    std::vector<double> p((size_t)n * D);
    for (auto& v : p) v = uniform(-half, half);
    for (int64_t i = 0; i < n; i += 25)
        for (int a = 0; a < D; ++a) p[i * D + a] += 20.0 * half;
    return p;
}

// T(v) as the definition states it: padded with +0.0 to a power of two, halved until one value is left
double tree(std::vector<double> v) {
    size_t size = 1;
    while (size < v.size()) size *= 2;
    v.resize(size, 0.0);
    for (; size > 1; size /= 2)
        for (size_t i = 0; i < size / 2; ++i) v[i] = gicp::sor_add(v[2 * i], v[2 * i + 1]);
    return v[0];
}

bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

template <int D>
void run_case(const char* name, const std::vector<double>& p, int k, double ratio) {
    const int64_t M = (int64_t)p.size() / D;
    const gicp_sor s{k, 0, ratio};
    std::vector<double> mean((size_t)M), dev((size_t)M), d;
    for (int64_t i = 0; i < M; ++i) {
        d.clear();
        for (int64_t j = 0; j < M; ++j)
            if (j != i) d.push_back(gicp::filter_d2<D>(&p[j * D], &p[i * D]));
        std::sort(d.begin(), d.end());
        mean[i] = gicp::sor_mean(d.data(), (int)std::min<int64_t>(k, M - 1));
    }
    const double mu = gicp::sor_mu(tree(mean), M);
    for (int64_t i = 0; i < M; ++i) dev[i] = gicp::sor_dev2(mean[i], mu);
    const double sigma = gicp::sor_sigma(tree(dev), M);
    const double thr = gicp::sor_thr(mu, ratio, sigma);
    std::vector<int64_t> want;
    for (int64_t i = 0; i < M; ++i)
        if (gicp::sor_keeps(mean[i], thr)) want.push_back(i);
    // the count first (every output NULL), then exactly-sized outputs: a write past their end is the sanitizer's
    int64_t m0 = -1;
    bool ok = gicp_sor_points_host(p.data(), M, D, &s, nullptr, nullptr, nullptr, nullptr, &m0) == GICP_OK &&
              m0 == (int64_t)want.size();
    std::vector<double> out((size_t)M * D), got_mean((size_t)M), st(3);
    std::vector<int64_t> idx((size_t)M);
    int64_t m1 = -1;
    ok = ok && gicp_sor_points_host(p.data(), M, D, &s, out.data(), idx.data(), got_mean.data(), st.data(), &m1) == GICP_OK &&
         m1 == m0;
    ok = ok && same(st[0], mu) && same(st[1], sigma) && same(st[2], thr);
    for (int64_t i = 0; ok && i < M; ++i) ok = same(got_mean[i], mean[i]);
    for (int64_t m = 0; ok && m < m1; ++m) {
        ok = idx[m] == want[m];
        for (int a = 0; ok && a < D; ++a) ok = same(out[m * D + a], p[want[m] * D + a]);
    }
    expect(ok, name);
    if (ok) std::printf("ok %s_%dd %lld rows, %lld kept\n", name, D, (long long)M, (long long)m1);
}

template <int D>
void cases() {
    const std::vector<double> p = cloud<D>(700, 5.0);
    run_case<D>("random_k8", p, 8, 1.0);
    run_case<D>("random_k1", p, 1, 1.0);
    run_case<D>("random_k31_ratio0", p, 31, 0.0);
    // fewer rows than k + 1: n_i = M - 1
    run_case<D>("two_rows_k8", cloud<D>(2, 1.0), 8, 1.0);
    run_case<D>("five_rows_k31", cloud<D>(5, 1.0), 31, 2.0);
    run_case<D>("nine_rows_k8", cloud<D>(9, 1.0), 8, 1.0);
    // exact ties: the integer lattice in reversed row order
    std::vector<double> lat;
    for (int i = 5 * 5 * (D == 3 ? 5 : 1) - 1; i >= 0; --i) {
        const int c[3] = {i % 5, (i / 5) % 5, i / 25};
        for (int a = 0; a < D; ++a) lat.push_back((double)c[a]);
    }
    run_case<D>("lattice_k6", lat, 6, 1.0);
    // 70 coincident rows: their means are 0
    std::vector<double> co = cloud<D>(40, 2.0);
    for (int i = 0; i < 70 * D; ++i) co.push_back(0.375);
    run_case<D>("coincident_k31", co, 31, 1.0);
    // refusals write nothing and leave a message
    std::vector<int64_t> idx(700, 77);
    int64_t m = 5;
    const gicp_sor good{4, 0, 1.0}, k0{0, 0, 1.0}, k32{32, 0, 1.0}, neg{4, 0, -1.0}, nanr{4, 0, std::nan("")};
    std::vector<double> bad = p;
    bad[3] = std::nan("");
    bool ok = gicp_sor_points_host(bad.data(), 700, D, &good, nullptr, idx.data(), nullptr, nullptr, &m) == GICP_E_INVALID &&
              std::strstr(gicp_last_host_error(), "non-finite") != nullptr;
    ok = ok && gicp_sor_points_host(p.data(), 700, D, &k0, nullptr, idx.data(), nullptr, nullptr, &m) == GICP_E_INVALID;
    ok = ok && gicp_sor_points_host(p.data(), 700, D, &k32, nullptr, idx.data(), nullptr, nullptr, &m) == GICP_E_INVALID &&
         std::strstr(gicp_last_host_error(), "sor: k must be") != nullptr;
    ok = ok && gicp_sor_points_host(p.data(), 700, D, &neg, nullptr, idx.data(), nullptr, nullptr, &m) == GICP_E_INVALID;
    ok = ok && gicp_sor_points_host(p.data(), 700, D, &nanr, nullptr, idx.data(), nullptr, nullptr, &m) == GICP_E_INVALID;
    ok = ok && gicp_sor_points_host(p.data(), 1, D, &good, nullptr, idx.data(), nullptr, nullptr, &m) == GICP_E_INVALID &&
         std::strstr(gicp_last_host_error(), "at least 2 rows") != nullptr;
    ok = ok && gicp_sor_points_host(p.data(), 700, 4, &good, nullptr, idx.data(), nullptr, nullptr, &m) == GICP_E_INVALID;
    ok = ok && gicp_sor_points_host(p.data(), 700, D, nullptr, nullptr, idx.data(), nullptr, nullptr, &m) == GICP_E_INVALID;
    ok = ok && gicp_sor_points_host(p.data(), 700, D, &good, nullptr, idx.data(), nullptr, nullptr, nullptr) == GICP_E_INVALID;
    std::vector<double> wide = {1e200, 0, 0, -1e200, 0, 0, 0, 1e200, 0};
    ok = ok && gicp_sor_points_host(wide.data(), 3, 3, &good, nullptr, idx.data(), nullptr, nullptr, &m) == GICP_E_INVALID &&
         std::strstr(gicp_last_host_error(), "not finite") != nullptr;
    for (int64_t v : idx) ok = ok && v == 77;
    ok = ok && m == 5;
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
