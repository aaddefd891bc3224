// gicp_hostmath.cpp — host arithmetic of the library with no HIP call in it (gicp_hostmath.h).
#include "gicp_hostmath.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>

#include "gicp_cluster.h"
#include "gicp_filter.h"
#include "gicp_sor.h"
#include "gicp_sweep.h"

namespace gicp {

void default_params(int dim, gicp_params* p) {
    std::memset(p, 0, sizeof(*p));
    p->max_iterations = 100;
    p->k_neighbors = dim == 2 ? 6 : 20;
    p->tolerance = 1e-6;
    p->max_distance_correspondence = 150.0;
    p->max_distance_nearest_neighbors = 50.0;
    p->epsilon = 100.0;
    p->ratio = 0.1;
    p->fixed_iterations = 0;
    p->min_neighbors = dim;
}

gicp_params resolve(int dim, const gicp_params* in) {
    gicp_params p;
    default_params(dim, &p);
    if (!in) return p;
    p = *in;
    if (p.k_neighbors <= 0) p.k_neighbors = dim == 2 ? 6 : 20;
    if (p.min_neighbors <= 0) p.min_neighbors = dim;
    if (p.epsilon == 0.0) p.epsilon = 100.0;
    if (p.cov_model < GICP_COV_PLANE_TO_PLANE || p.cov_model > GICP_COV_POINT_TO_PLANE)
        throw Fail{GICP_E_INVALID, "cov_model must be GICP_COV_PLANE_TO_PLANE, _POINT_TO_POINT or _POINT_TO_PLANE"};
    if (p.robust_kernel < GICP_ROBUST_NONE || p.robust_kernel > GICP_ROBUST_TUKEY)
        throw Fail{GICP_E_INVALID, "robust_kernel must be GICP_ROBUST_NONE, _HUBER, _CAUCHY, _GEMAN_MCCLURE or _TUKEY"};
    if (p.robust_kernel != GICP_ROBUST_NONE && !(std::isfinite(p.robust_scale) && p.robust_scale > 0.0))
        throw Fail{GICP_E_INVALID, "robust_scale must be finite and > 0 with a robust kernel"};
    if (p.rotation_epsilon <= 0.0 && p.transformation_epsilon > 0.0) p.rotation_epsilon = 1.0 - p.transformation_epsilon;
    return p;
}

// fp32-screen error bound: E bounds the error of one coordinate difference
Margin make_margin(int dim, float rho_q, float rho_db, double dmax) {
    const double E = std::ldexp(8.0 * rho_q + 3.0 * rho_db + 3.0 * dmax, -23) + 1e-30;
    Margin m;
    m.a = (float)(2.0 * std::sqrt((double)dim) * E);
    m.b = (float)(dim * E * E);
    m.c = (float)std::ldexp(1.0, -16);
    return m;
}
float screen_bound(const Margin& m, double d) {
    const double d2 = d * d;
    const double b = d2 + 2.0 * (m.a * d + m.b + m.c * d2);
    return (float)(b * (1.0 + 1e-6)) + 1e-30f;
}

// The largest double x with sqrt(x) <= dc (sqrt correctly rounded, as on the device), so the accept
// test of gicp.py:136, !(distance > d_c) with distance = sqrt(d2), is exactly d2 <= accept_d2_max(d_c)
double accept_d2_max(double dc) {
    if (!(dc >= 0.0) || std::isinf(dc)) return dc;   // d_c = +inf accepts everything; NaN nothing
    double x = dc * dc;
    while (std::sqrt(x) > dc) x = std::nextafter(x, 0.0);
    while (std::sqrt(std::nextafter(x, INFINITY)) <= dc) x = std::nextafter(x, INFINITY);
    return x;
}

// Cut the Morton-sorted points into tiles: runs of <= 64 consecutive points whose bounding box (in
// Morton grid cells) stays within an extent cap E.  E is the smallest cap (steps of 2^(1/4)) whose
// tile count stays <= 1.35x the minimum ceil(n/64): tiles are as compact as that budget allows, and
// the cap bounds the largest tile, which sets both the widest query wave and the loosest box.
void build_tile_table(const std::vector<uint32_t>& codes, int dim, int bits, std::vector<int32_t>& start,
                      std::vector<int32_t>& count, std::vector<uint32_t>& first_code, int& cap_out, int k_hint,
                      WorkerPool& pool, int maxp) {
    const int64_t n = (int64_t)codes.size();
    static const double budget = [] {   // GICP_TILE_BUDGET: tile-count budget over ceil(n / 64)
        const char* e = std::getenv("GICP_TILE_BUDGET");
        const double b = e ? std::atof(e) : 1.35;
        return b >= 1.0 ? b : 1.35;
    }();
    const int64_t target = (int64_t)(budget * std::ceil(n / (double)maxp)) + 2;   // (maxp <= 64 points a tile)
    // decode the grid coordinates once
    auto compact3 = [](uint32_t x) {   // inverse of the kernels' spread3
        x &= 0x09249249u;
        x = (x | (x >> 2)) & 0x030C30C3u;
        x = (x | (x >> 4)) & 0x0300F00Fu;
        x = (x | (x >> 8)) & 0x030000FFu;
        x = (x | (x >> 16)) & 0x000003FFu;
        return x;
    };
    auto compact2 = [](uint32_t x) {
        x &= 0x55555555u;
        x = (x | (x >> 1)) & 0x33333333u;
        x = (x | (x >> 2)) & 0x0F0F0F0Fu;
        x = (x | (x >> 4)) & 0x00FF00FFu;
        x = (x | (x >> 8)) & 0x0000FFFFu;
        return x;
    };
    std::vector<uint16_t> g((size_t)n * dim);
    constexpr int kSeg = 16;   // fixed segments (independent of the host's core count: deterministic)
    pool.run(kSeg, [&](int k) {
        for (int64_t i = n * k / kSeg; i < n * (k + 1) / kSeg; ++i) {
            const uint32_t c = codes[i];
            for (int a = 0; a < dim; ++a)
                g[(size_t)i * dim + a] = (uint16_t)(dim == 3 ? compact3(c >> a) : compact2(c >> a));
        }
    });
    // greedy cut of points [b, e) (a forced break at b); appends (start, count) pairs if `out`
    auto cut_seg = [&](int64_t b, int64_t e, int E, std::vector<int32_t>* out) -> int64_t {
        int64_t nt = 0, i0 = b;
        int lo0 = 0, lo1 = 0, lo2 = 0, hi0 = 0, hi1 = 0, hi2 = 0;
        const uint16_t* gp = g.data();
        for (int64_t i = b; i < e; ++i) {
            const int v0 = gp[i * dim], v1 = gp[i * dim + 1], v2 = dim == 3 ? gp[i * dim + 2] : 0;
            if (i > i0) {
                const int n0 = std::min(lo0, v0), x0 = std::max(hi0, v0);
                const int n1 = std::min(lo1, v1), x1 = std::max(hi1, v1);
                const int n2 = std::min(lo2, v2), x2 = std::max(hi2, v2);
                if (i - i0 < maxp && x0 - n0 <= E && x1 - n1 <= E && x2 - n2 <= E) {
                    lo0 = n0, hi0 = x0, lo1 = n1, hi1 = x1, lo2 = n2, hi2 = x2;
                    continue;
                }
                ++nt;
                if (out) {
                    out->push_back((int32_t)i0);
                    out->push_back((int32_t)(i - i0));
                }
                i0 = i;
            }
            lo0 = hi0 = v0, lo1 = hi1 = v1, lo2 = hi2 = v2;
        }
        if (e > i0) {
            ++nt;
            if (out) {
                out->push_back((int32_t)i0);
                out->push_back((int32_t)(e - i0));
            }
        }
        return nt;
    };
    // the 16 segments are cut concurrently on the pool
    std::vector<std::vector<int32_t>> seg_out(kSeg);
    auto cut = [&](int E, bool emit) -> int64_t {
        int64_t nt_seg[kSeg] = {};
        pool.run(kSeg, [&](int k) {
            if (emit) seg_out[k].clear();
            nt_seg[k] = cut_seg(n * k / kSeg, n * (k + 1) / kSeg, E, emit ? &seg_out[k] : nullptr);
        });
        int64_t nt = 0;
        for (int k = 0; k < kSeg; ++k) nt += nt_seg[k];
        if (emit)
            for (int k = 0; k < kSeg; ++k)
                for (size_t j = 0; j < seg_out[k].size(); j += 2) {
                    start.push_back(seg_out[k][j]);
                    count.push_back(seg_out[k][j + 1]);
                    first_code.push_back(codes[seg_out[k][j]]);
                }
        return nt;
    };
    // smallest cap on the grid E_k = 2 * 2^(k/4) meeting the budget (the count falls as E grows):
    // a short walk from the previous cloud's k when given (a frame stream changes little), else a
    // binary search over k
    const auto cap_of = tile_cap_of;
    const int kmax = 4 * (bits - 1);   // cap_of(kmax) = 2^bits: one Morton run per tile
    int klo = 0, khi = kmax;
    if (k_hint > 0 && k_hint < kmax) {   // walk from the hint: usually hint feasible, hint-1 not
        if (cut(cap_of(k_hint), false) <= target) {
            khi = k_hint;
            klo = k_hint - 1;
            if (cut(cap_of(klo), false) <= target) {
                khi = klo;
                klo = 0;
            } else {
                klo = k_hint;
            }
        } else {
            klo = k_hint + 1;
        }
    }
    while (klo < khi) {
        const int km = (klo + khi) / 2;
        if (cut(cap_of(km), false) <= target) khi = km;
        else klo = km + 1;
    }
    const int E = cap_of(klo);
    cap_out = klo;
    start.clear();
    count.clear();
    first_code.clear();
    cut(E, true);
}

// Tiles of shard `shard` of `nshards` (the k_corr split: chunks of kShardChunk units of kCorrWaves tiles, dealt
// round-robin), or all of them when nshards = 1.
int shard_tile_count(int ntiles, int shard, int nshards) {
    if (nshards <= 1) return ntiles;
    constexpr int kChunkTiles = kShardChunk * kCorrWaves;
    const int nchunks = (ntiles + kChunkTiles - 1) / kChunkTiles;
    int mine = 0;
    for (int c = shard; c < nchunks; c += nshards) mine += std::min(kChunkTiles, ntiles - c * kChunkTiles);
    return mine;
}

// Morton seed lookup (DevCloud::seed_tab) over the tiles' first codes: 2^sb buckets of the code's top bits, about
// 4 per tile, and one closing entry.  Returns the shift that takes a code to its bucket (DevCloud::seed_shift).
int build_seed_table(const std::vector<uint32_t>& tcode, int code_bits, std::vector<int32_t>& seed) {
    const int ntiles = (int)tcode.size();
    int sb = 2;
    while ((1 << sb) < 4 * ntiles && sb < 20) ++sb;
    sb = std::min(sb, code_bits);
    const int shift = code_bits - sb;
    const size_t nb = (size_t)1 << sb;
    seed.resize(nb + 1);
    int t = 0;   // last tile whose first code <= p << shift (0 if none)
    for (size_t p = 0; p < nb; ++p) {
        const uint64_t lim = (uint64_t)p << shift;
        while (t + 1 < ntiles && (uint64_t)tcode[t + 1] <= lim) ++t;
        seed[p] = t;
    }
    seed[nb] = ntiles - 1;
    return shift;
}

// Bounds of a host cloud and its finiteness test in one fused, branch-free pass (v - v is NaN for NaN and +-inf).
void scan_bounds(const double* xyz, int64_t n, int dim, double (&mn)[3], double (&mx)[3]) {
    for (int a = 0; a < 3; ++a) mn[a] = mx[a] = 0.0;
    bool finite = true;
    auto scan = [&](auto D_) {
        constexpr int D = decltype(D_)::value;
        double lo[D], hi[D], acc[D];
        for (int a = 0; a < D; ++a) lo[a] = hi[a] = xyz[a], acc[a] = 0.0;
        for (int64_t i = 0; i < n; ++i)
            for (int a = 0; a < D; ++a) {
                const double v = xyz[i * D + a];
                lo[a] = v < lo[a] ? v : lo[a];
                hi[a] = v > hi[a] ? v : hi[a];
                acc[a] += v - v;
            }
        for (int a = 0; a < D; ++a) {
            mn[a] = lo[a], mx[a] = hi[a];
            finite = finite && acc[a] == 0.0 && std::isfinite(lo[a]) && std::isfinite(hi[a]);
        }
    };
    if (dim == 3) scan(std::integral_constant<int, 3>{});
    else scan(std::integral_constant<int, 2>{});
    if (!finite) throw Fail{GICP_E_INVALID, "cloud contains non-finite coordinates"};
}

// the finiteness test of a sweep's stamps and reference stamp (v - v is NaN for NaN and +-inf)
void scan_stamps(const double* stamps, int64_t n, double ref) {
    if (!std::isfinite(ref)) throw Fail{GICP_E_INVALID, "sweep reference stamp is not finite"};
    double acc = 0.0;
    for (int64_t i = 0; i < n; ++i) acc += stamps[i] - stamps[i];
    if (!(acc == 0.0)) throw Fail{GICP_E_INVALID, "sweep contains non-finite stamps"};
}

// doubles from the ordered-integer form gicp_voxel.hip reduces min / max in
double dec_ordered(unsigned long long e) {
    const unsigned long long b = (e >> 63) ? (e & 0x7FFFFFFFFFFFFFFFull) : ~e;
    double v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}

// the bounds in the result words of a device reduction (gicp_internal.h kVoxelRes): min[3], then max[3]
void decode_bounds(const unsigned long long* res, int dim, double (&mn)[3], double (&mx)[3]) {
    for (int a = 0; a < 3; ++a) mn[a] = mx[a] = 0.0;
    for (int a = 0; a < dim; ++a) {
        mn[a] = dec_ordered(res[a]);
        mx[a] = dec_ordered(res[3 + a]);
    }
}

// The voxel filter's lowest cell per axis and key bits: division by a positive leaf is monotone, so every point's
// cell lies in [floor(min / leaf), floor(max / leaf)], computed here as the device computes it.  Returns the
// bits the sort covers (>= 1).
int voxel_key_bits(int dim, const double (&mn)[3], const double (&mx)[3], double leaf, double (&cmin)[3], int32_t (&bits)[3]) {
    const double lim = dim == 3 ? 2097152.0 : 2147483648.0;   // 2^21, 2^31 cells per axis
    int total = 0;
    for (int a = 0; a < dim; ++a) {
        const double c0 = std::floor(mn[a] / leaf), c1 = std::floor(mx[a] / leaf);
        const double range = c1 - c0 + 1.0;
        if (!(std::fabs(c0) < 4503599627370496.0 && std::fabs(c1) < 4503599627370496.0 && range <= lim)) {
            char b[160];
            std::snprintf(b, sizeof b, "voxel grid too wide: axis %d spans %.6g cells of leaf %g (at most 2^%d per axis in %d-D)",
                          a, range, leaf, dim == 3 ? 21 : 31, dim);
            throw Fail{GICP_E_INVALID, b};
        }
        cmin[a] = c0;
        uint64_t r = (uint64_t)range - 1;
        int nb = 0;
        while (r) ++nb, r >>= 1;
        bits[a] = nb;
        total += nb;
    }
    return std::max(1, total);
}

// The local map's window: its half-width R in cells, and the key bits per axis ceil(log2(2 R + 1))
int64_t map_window_cells(int dim, double leaf, double max_range, int& bits) {
    const double R = std::ceil(max_range / leaf);
    const double lim = dim == 3 ? 2097152.0 : 2147483648.0;   // 2^21, 2^31 cells per axis (the filter's limits)
    if (!(2.0 * R + 1.0 <= lim)) {
        char b[160];
        std::snprintf(b, sizeof b, "map window too wide: %.6g cells of leaf %g per axis (at most 2^%d per axis in %d-D)",
                      2.0 * R + 1.0, leaf, dim == 3 ? 21 : 31, dim);
        throw Fail{GICP_E_INVALID, b};
    }
    uint64_t r = (uint64_t)(2 * (int64_t)R);
    bits = 0;
    while (r) ++bits, r >>= 1;
    return (int64_t)R;
}

// ... and its lowest cell on `axis` when centred on the coordinate t
int64_t map_window_lo(int axis, double t, double leaf, int64_t R) {
    const double c = std::floor(t / leaf);   // the centre cell
    if (!(std::fabs(c) + (double)R < 2147483648.0)) {
        char b[160];
        std::snprintf(b, sizeof b, "map window leaves the int32 cell range: axis %d is centred on cell %.6g with a half-width of %lld cells",
                      axis, c, (long long)R);
        throw Fail{GICP_E_INVALID, b};
    }
    return (int64_t)c - R;
}

// ---- motion compensation (gicp_sweep.h) ----

// The twist xi = Log(M) of a rigid motion M ((dim+1)^2 row-major, last row not read): 3-D (omega[3], v[3]),
// 2-D (omega, v[2]).  Refuses what is no constant-velocity sweep: a non-finite M, a linear part that is no
// rotation, more than a quarter turn per stamp unit (which also keeps Log well conditioned: theta <= pi / 2).
void motion_twist(int dim, const double* M, double* xi) {
    if (dim != 2 && dim != 3) throw Fail{GICP_E_INVALID, "dim must be 2 or 3"};
    if (!M || !xi) throw Fail{GICP_E_INVALID, "motion and twist must not be NULL"};
    const int w = dim + 1;
    double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, t[3] = {0, 0, 0};
    for (int r = 0; r < dim; ++r) {
        for (int c = 0; c < w; ++c)
            if (!std::isfinite(M[r * w + c])) throw Fail{GICP_E_INVALID, "motion contains non-finite values"};
        for (int c = 0; c < dim; ++c) R[r][c] = M[r * w + c];
        t[r] = M[r * w + dim];
    }
    double dev = 0.0;
    for (int a = 0; a < dim; ++a)
        for (int b = 0; b < dim; ++b) {
            double g = a == b ? -1.0 : 0.0;
            for (int k = 0; k < dim; ++k) g += R[k][a] * R[k][b];
            dev = std::max(dev, std::fabs(g));
        }
    const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                       R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
    if (!(dev <= 1e-9) || !(det > 0.0)) {
        char b[128];
        std::snprintf(b, sizeof b, "motion is not rigid: max|R^T R - I| = %.3g (at most 1e-9), det R = %.3g", dev, det);
        throw Fail{GICP_E_INVALID, b};
    }
    const char* turn = "motion rotates by more than a quarter turn per stamp unit";
    double A, B, C;
    if (dim == 3) {
        const double cs = 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1.0);
        if (cs < 0.0) throw Fail{GICP_E_INVALID, turn};
        // a = sin(theta) axis, from the skew part; theta = atan2(|a|, cos(theta)) is accurate at every angle
        const double a[3] = {0.5 * (R[2][1] - R[1][2]), 0.5 * (R[0][2] - R[2][0]), 0.5 * (R[1][0] - R[0][1])};
        const double sn = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        const double f = sn > 0.0 ? std::atan2(sn, cs) / sn : 1.0;
        const double o[3] = {f * a[0], f * a[1], f * a[2]};
        sweep_coeffs(o[0] * o[0] + o[1] * o[1] + o[2] * o[2], A, B, C);
        // v solves V v = t, V = I + B o^ + C o^2 (o^2 = o o^T - |o|^2 I)
        const double K[3][3] = {{0, -o[2], o[1]}, {o[2], 0, -o[0]}, {-o[1], o[0], 0}};
        double V[3][3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                double k2 = 0.0;
                for (int k = 0; k < 3; ++k) k2 += K[r][k] * K[k][c];
                V[r][c] = (r == c ? 1.0 : 0.0) + B * K[r][c] + C * k2;
            }
        const double c00 = V[1][1] * V[2][2] - V[1][2] * V[2][1], c01 = V[1][2] * V[2][0] - V[1][0] * V[2][2],
                     c02 = V[1][0] * V[2][1] - V[1][1] * V[2][0];
        const double dV = V[0][0] * c00 + V[0][1] * c01 + V[0][2] * c02;
        const double inv[3][3] = {
            {c00, V[0][2] * V[2][1] - V[0][1] * V[2][2], V[0][1] * V[1][2] - V[0][2] * V[1][1]},
            {c01, V[0][0] * V[2][2] - V[0][2] * V[2][0], V[0][2] * V[1][0] - V[0][0] * V[1][2]},
            {c02, V[0][1] * V[2][0] - V[0][0] * V[2][1], V[0][0] * V[1][1] - V[0][1] * V[1][0]}};
        for (int r = 0; r < 3; ++r) {
            xi[r] = o[r];
            xi[3 + r] = (inv[r][0] * t[0] + inv[r][1] * t[1] + inv[r][2] * t[2]) / dV;
        }
    } else {
        if (R[0][0] < 0.0) throw Fail{GICP_E_INVALID, turn};
        const double o = std::atan2(R[1][0] - R[0][1], R[0][0] + R[1][1]);
        sweep_coeffs(o * o, A, B, C);
        // V = (A  -B o; B o  A)
        const double Bo = B * o, dV = A * A + Bo * Bo;
        xi[0] = o;
        xi[1] = (A * t[0] + Bo * t[1]) / dV;
        xi[2] = (A * t[1] - Bo * t[0]) / dV;
    }
}

void deskew_host(const double* xyz, const double* stamps, int64_t n, int dim, const double* xi, double ref, double* out) {
    if (dim == 3)
        for (int64_t i = 0; i < n; ++i) sweep_point<3>(xi, stamps[i] - ref, xyz + i * 3, out + i * 3);
    else
        for (int64_t i = 0; i < n; ++i) sweep_point<2>(xi, stamps[i] - ref, xyz + i * 2, out + i * 2);
}

// ---- input filters (gicp_filter.h) ----

// what gicp_set_filter, gicp_filter_points and gicp_filter_points_host refuse alike
void check_filter(const gicp_filter& f) {
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(f.center[a])) throw Fail{GICP_E_INVALID, "filter: center is not finite"};
    if (!std::isfinite(f.min_range) || !std::isfinite(f.max_range) || !std::isfinite(f.radius))
        throw Fail{GICP_E_INVALID, "filter: min_range, max_range and radius must be finite"};
    if (f.min_range < 0.0 || f.max_range < 0.0 || f.radius < 0.0)
        throw Fail{GICP_E_INVALID, "filter: min_range, max_range and radius must be >= 0 (0 turns each off)"};
    if (f.max_range > 0.0 && f.min_range > f.max_range) {
        char b[128];
        std::snprintf(b, sizeof b, "filter: min_range %g exceeds max_range %g", f.min_range, f.max_range);
        throw Fail{GICP_E_INVALID, b};
    }
    if (f.radius > 0.0 && f.min_neighbors < 1) throw Fail{GICP_E_INVALID, "filter: min_neighbors must be >= 1 with a radius"};
}

bool filter_crops(const gicp_filter& f) { return f.min_range > 0.0 || f.max_range > 0.0; }

// a stage left no row (stage 0: the crop of n rows, 1: radius outlier removal of the n rows the crop left)
void fail_filter_empty(int stage, int64_t n, const gicp_filter& f) {
    char b[200];
    if (stage == 0)
        std::snprintf(b, sizeof b, "filter: the range crop removed all %lld points (min_range %g, max_range %g)", (long long)n,
                      f.min_range, f.max_range);
    else
        std::snprintf(b, sizeof b,
                      "filter: radius outlier removal removed all %lld points the crop left (radius %g, min_neighbors %d)",
                      (long long)n, f.radius, (int)f.min_neighbors);
    throw Fail{GICP_E_INVALID, b};
}

// The grid of radius outlier removal over the cropped cloud's bounds.  The limit is stated in cells of edge
// `radius`; the keys are those of the voxel filter's grid with leaf = radius kRorEdge (gicp_filter.h), which spans
// no more cells.  Returns the bits the sort covers; cmax: the highest cell per axis relative to cmin.  stage: the
// stage a refusal names ("filter"; "cluster" for Euclidean cluster extraction, which walks the same grid).
int ror_key_bits(int dim, const double (&mn)[3], const double (&mx)[3], double radius, double& leaf, double (&cmin)[3],
                 int32_t (&bits)[3], int64_t (&cmax)[3], const char* stage) {
    const double lim = dim == 3 ? 2097152.0 : 2147483648.0;   // 2^21, 2^31 cells per axis
    for (int a = 0; a < dim; ++a) {
        const double c0 = std::floor(mn[a] / radius), c1 = std::floor(mx[a] / radius);
        const double range = c1 - c0 + 1.0;
        char b[224];
        if (!(range <= lim)) {
            std::snprintf(b, sizeof b,
                          "%s: radius grid too wide: axis %c spans %.6g cells of edge radius = %g (at most 2^%d per axis in "
                          "%d-D); crop the far returns first with a max_range",
                          stage, "xyz"[a], range, radius, dim == 3 ? 21 : 31, dim);
            throw Fail{GICP_E_INVALID, b};
        }
        if (!(std::fabs(c0) < 34359738368.0 && std::fabs(c1) < 34359738368.0)) {   // 2^35: see kRorEdge
            std::snprintf(b, sizeof b, "%s: axis %c lies beyond 2^35 cells of edge radius = %g from the origin", stage, "xyz"[a],
                          radius);
            throw Fail{GICP_E_INVALID, b};
        }
    }
    leaf = radius * kRorEdge;
    const int end_bit = voxel_key_bits(dim, mn, mx, leaf, cmin, bits);
    for (int a = 0; a < 3; ++a) cmax[a] = a < dim ? (int64_t)(std::floor(mx[a] / leaf) - cmin[a]) : 0;
    return end_bit;
}

namespace {

// f(b, e) for every run [b, e) of the sorted (key, row) pairs that holds neighbour cells of the cell of `key`: the
// device's runs (gicp_runs_dev.h), clipped at the ends of the last axis, rows of cells outside the grid skipped
template <int D, class F>
void host_runs(const std::vector<std::pair<uint64_t, int64_t>>& ks, uint64_t key, const int32_t (&bits)[3], const int64_t (&cmax)[3],
               F&& f) {
    const int bl = bits[D - 1], bm = D == 3 ? bits[1] : 0;
    auto first = [&](uint64_t k) { return std::lower_bound(ks.begin(), ks.end(), std::make_pair(k, (int64_t)-1)) - ks.begin(); };
    const int64_t cl = (int64_t)(key & ((1ull << bl) - 1ull));
    const int64_t cm = D == 3 ? (int64_t)((key >> bl) & ((1ull << bm) - 1ull)) : 0;
    const int64_t ch = (int64_t)(key >> (bl + bm));
    const int64_t l0 = cl > 0 ? cl - 1 : 0, l1 = cl < cmax[D - 1] ? cl + 1 : cl;
    for (int dh = -1; dh <= 1; ++dh) {
        const int64_t h = ch + dh;
        if (h < 0 || h > cmax[0]) continue;
        for (int dm = (D == 3 ? -1 : 0); dm <= (D == 3 ? 1 : 0); ++dm) {
            const int64_t mm = cm + dm;
            if (D == 3 && (mm < 0 || mm > cmax[1])) continue;
            const uint64_t row = (((uint64_t)h << bm) | (uint64_t)mm) << bl;
            f((int64_t)first(row | (uint64_t)l0), (int64_t)first((row | (uint64_t)l1) + 1));
        }
    }
}

// The cells of the rows `rows` of xyz on the grid of ror_key_bits, as sorted (key, position in rows) pairs
template <int D>
std::vector<std::pair<uint64_t, int64_t>> host_keys(const double* xyz, const int64_t* rows, int64_t m, double leaf,
                                                    const double (&cmin)[3], const int32_t (&bits)[3]) {
    std::vector<std::pair<uint64_t, int64_t>> ks((size_t)m);
    for (int64_t s = 0; s < m; ++s) {
        uint64_t key = 0;
        for (int a = 0; a < D; ++a)
            key = (key << bits[a]) | (uint64_t)(int64_t)(std::floor(xyz[(rows ? rows[s] : s) * D + a] / leaf) - cmin[a]);
        ks[s] = {key, s};
    }
    std::sort(ks.begin(), ks.end());
    return ks;
}

// The host yardstick: the device's algorithm as plain loops -- keys of the same grid, one sort, and per point the
// same clipped key runs searched in the sorted keys.
template <int D>
void filter_host(const double* xyz, int64_t N, const gicp_filter& f, double* out_xyz, int64_t* out_index, int32_t* out_count,
                 int64_t* M_out) {
    std::vector<int64_t> rows;   // survivors of the crop, ascending
    rows.reserve((size_t)N);
    const double lo2 = f.min_range * f.min_range, hi2 = f.max_range * f.max_range;
    for (int64_t i = 0; i < N; ++i) {
        const bool k = !filter_crops(f) || crop_keeps(filter_d2<D>(xyz + i * D, f.center), lo2, hi2);
        if (k) rows.push_back(i);
        if (out_count) out_count[i] = k ? 0 : -1;
    }
    if (rows.empty()) fail_filter_empty(0, N, f);
    const int64_t m = (int64_t)rows.size();
    std::vector<char> keep((size_t)m, 1);
    if (f.radius > 0.0) {
        double mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
        for (int a = 0; a < D; ++a) mn[a] = mx[a] = xyz[rows[0] * D + a];
        for (int64_t s = 0; s < m; ++s)
            for (int a = 0; a < D; ++a) {
                const double v = xyz[rows[s] * D + a];
                mn[a] = v < mn[a] ? v : mn[a];
                mx[a] = v > mx[a] ? v : mx[a];
            }
        double leaf, cmin[3];
        int32_t bits[3];
        int64_t cmax[3];
        ror_key_bits(D, mn, mx, f.radius, leaf, cmin, bits, cmax);
        const std::vector<std::pair<uint64_t, int64_t>> ks = host_keys<D>(xyz, rows.data(), m, leaf, cmin, bits);   // (key, survivor)
        const double r2 = f.radius * f.radius;
        for (int64_t j = 0; j < m; ++j) {
            const double* p = xyz + rows[ks[j].second] * D;
            int32_t count = 0;
            host_runs<D>(ks, ks[j].first, bits, cmax, [&](int64_t b, int64_t e) {
                for (int64_t t = b; t < e; ++t)
                    if (t != j && ror_near(filter_d2<D>(p, xyz + rows[ks[t].second] * D), r2)) ++count;
            });
            const int64_t s = ks[j].second;
            keep[s] = count >= f.min_neighbors;
            if (out_count) out_count[rows[s]] = count;
        }
    }
    int64_t M = 0;
    for (int64_t s = 0; s < m; ++s) {
        if (!keep[s]) continue;
        for (int a = 0; a < D; ++a) out_xyz[M * D + a] = xyz[rows[s] * D + a];
        if (out_index) out_index[M] = rows[s];
        ++M;
    }
    if (M == 0) fail_filter_empty(1, m, f);
    *M_out = M;
}

}  // namespace

// the argument checks of both one-shot entry points, and the finiteness test
void check_filter_args(const double* xyz, int64_t N, int dim, const gicp_filter* f, const double* out_xyz, const int64_t* M_out) {
    check_cloud_args(xyz, N, dim);
    if (!f) throw Fail{GICP_E_INVALID, "filter must not be NULL"};
    if (!out_xyz || !M_out) throw Fail{GICP_E_INVALID, "out_xyz and M_out must not be NULL"};
    check_filter(*f);
    double mn[3], mx[3];
    scan_bounds(xyz, N, dim, mn, mx);
}

void filter_points_host(const double* xyz, int64_t N, int dim, const gicp_filter* f, double* out_xyz, int64_t* out_index,
                        int32_t* out_count, int64_t* M_out) {
    check_filter_args(xyz, N, dim, f, out_xyz, M_out);
    *M_out = 0;
    if (dim == 3) filter_host<3>(xyz, N, *f, out_xyz, out_index, out_count, M_out);
    else filter_host<2>(xyz, N, *f, out_xyz, out_index, out_count, M_out);
}

// ---- exact k-nearest-neighbour queries ----

// what gicp_knn, gicp_knn_points and gicp_knn_host refuse alike of the query side (queries == NULL: a self-query,
// Q and dim are the database's); the finiteness scans are the callers'
void check_knn_args(const double* queries, int64_t Q, int dim, int k, double max_distance) {
    if (k < 1 || k > kKnnMaxK) throw Fail{GICP_E_INVALID, "k must be 1..gicp_knn_max_k() (32)"};
    if (!(std::isfinite(max_distance) && max_distance >= 0.0))
        throw Fail{GICP_E_INVALID, "max_distance must be finite and >= 0 (0 sets no limit)"};
    if (!queries) return;
    if (dim != 2 && dim != 3) throw Fail{GICP_E_INVALID, "dim must be 2 or 3"};
    if (Q < 1) throw Fail{GICP_E_INVALID, "queries must be a non-empty Q x dim array (Q >= 1)"};
    if (Q > (int64_t)0x7FFFFFFF - 64) throw Fail{GICP_E_INVALID, "too many queries (> 2^31)"};
}

namespace {
// The contract as a loop over all pairs: per query the k first rows of the order (d2, original index).  Rows come
// in ascending index, so a row displaces a kept one only when its d2 is strictly smaller.
template <int D>
void knn_brute(const double* xyz, int64_t M, const double* qs, int64_t Q, int k, double maxd2, int64_t* index, double* dist2,
               int32_t* count) {
    std::vector<double> d(k);
    std::vector<int64_t> id(k);
    for (int64_t qi = 0; qi < Q; ++qi) {
        const double* q = qs + qi * D;
        int n = 0;
        for (int64_t j = 0; j < M; ++j) {
            const double d2 = filter_d2<D>(xyz + j * D, q);
            if (!(d2 <= maxd2) || (n == k && !(d2 < d[k - 1]))) continue;
            int m = n < k ? n : k - 1;
            for (; m > 0 && d2 < d[m - 1]; --m) d[m] = d[m - 1], id[m] = id[m - 1];
            d[m] = d2;
            id[m] = j;
            if (n < k) ++n;
        }
        for (int m = 0; m < k; ++m) {
            if (index) index[qi * k + m] = m < n ? id[m] : -1;
            if (dist2) dist2[qi * k + m] = m < n ? d[m] : INFINITY;
        }
        if (count) count[qi] = n;
    }
}
}  // namespace

void knn_host(const double* xyz, int64_t M, const double* queries, int64_t Q, int dim, int k, double max_distance,
              int64_t* index, double* dist2, int32_t* count) {
    check_cloud_args(xyz, M, dim);
    check_knn_args(queries, Q, dim, k, max_distance);
    double mn[3], mx[3];
    scan_bounds(xyz, M, dim, mn, mx);   // (the finiteness tests: nothing is written before them)
    if (queries) scan_bounds(queries, Q, dim, mn, mx);
    const double* qs = queries ? queries : xyz;
    const int64_t nq = queries ? Q : M;
    const double maxd2 = max_distance > 0.0 ? max_distance * max_distance : INFINITY;
    if (dim == 3) knn_brute<3>(xyz, M, qs, nq, k, maxd2, index, dist2, count);
    else knn_brute<2>(xyz, M, qs, nq, k, maxd2, index, dist2, count);
}

// ---- statistical outlier removal (gicp_sor.h) ----

// what gicp_set_sor, gicp_sor_points and gicp_sor_points_host refuse alike of the setting
void check_sor(const gicp_sor& s) {
    if (s.k < 1 || s.k > kSorMaxK) throw Fail{GICP_E_INVALID, "sor: k must be 1..gicp_sor_max_k() (31)"};
    if (!(std::isfinite(s.std_ratio) && s.std_ratio >= 0.0)) throw Fail{GICP_E_INVALID, "sor: std_ratio must be finite and >= 0"};
}

// a stage needs two rows: a row's neighbours are the others
void check_sor_rows(int64_t m) {
    if (m >= 2) return;
    char b[128];
    std::snprintf(b, sizeof b, "sor: statistical outlier removal needs at least 2 rows (the stage got %lld)", (long long)m);
    throw Fail{GICP_E_INVALID, b};
}

// A stage's rows must span a squared extent that fp64 holds: beyond it d2 between rows overflows, the sum of the
// means need not be finite, and the search's margin (the diagonal) is infinite.  Refused before anything is launched,
// by the device path and the host yardstick alike.
void check_sor_extent(int dim, const double (&mn)[3], const double (&mx)[3]) {
    double diag2 = 0.0;
    for (int a = 0; a < dim; ++a) {
        const double e = mx[a] - mn[a];
        diag2 += e * e;
    }
    if (!std::isfinite(diag2)) throw Fail{GICP_E_INVALID, "sor: the squared extent of the rows is not finite (the cloud is too wide for fp64 distances)"};
}

// the argument checks of both one-shot entry points, the finiteness test and the bounds it yields
void check_sor_args(const double* xyz, int64_t N, int dim, const gicp_sor* s, const int64_t* M_out, double (&mn)[3],
                    double (&mx)[3]) {
    check_cloud_args(xyz, N, dim);
    if (!s) throw Fail{GICP_E_INVALID, "sor must not be NULL"};
    if (!M_out) throw Fail{GICP_E_INVALID, "M_out must not be NULL"};
    check_sor(*s);
    check_sor_rows(N);
    scan_bounds(xyz, N, dim, mn, mx);
    check_sor_extent(dim, mn, mx);
}

// what a stage of m rows refuses of its own result: a sum of the means that is not finite, no row kept
void check_sor_result(double t_mean, int64_t kept, int64_t m, const gicp_sor& s) {
    char b[200];
    if (!std::isfinite(t_mean)) {
        std::snprintf(b, sizeof b, "sor: the sum of the %lld mean neighbour distances is not finite (the cloud is too wide for fp64)",
                      (long long)m);
        throw Fail{GICP_E_INVALID, b};
    }
    if (kept <= 0) {
        std::snprintf(b, sizeof b, "sor: statistical outlier removal removed all %lld points (k %d, std_ratio %g)", (long long)m,
                      (int)s.k, s.std_ratio);
        throw Fail{GICP_E_INVALID, b};
    }
}

namespace {
// T(v): the pairwise tree in row order (an odd element is carried: it would meet the +0.0 of the padding)
double sor_tree(std::vector<double>& v) {
    size_t n = v.size();
    while (n > 1) {
        const size_t h = n / 2;
        for (size_t i = 0; i < h; ++i) v[i] = sor_add(v[2 * i], v[2 * i + 1]);
        if (n & 1) v[h] = sor_add(v[n - 1], 0.0);
        n = h + (n & 1);
    }
    return v[0];
}

template <int D>
void sor_host(const double* xyz, int64_t N, const gicp_sor& s, double* out_xyz, int64_t* out_index, double* out_mean,
              double* out_stats, int64_t* M_out) {
    // the self-query for k + 1 rows; entry 0 is the row's own zero, or that of a coincident row of lower index
    const int kk = s.k + 1;
    std::vector<double> d2((size_t)N * kk);
    std::vector<int32_t> cnt((size_t)N);
    knn_brute<D>(xyz, N, xyz, N, kk, INFINITY, nullptr, d2.data(), cnt.data());
    std::vector<double> mean((size_t)N), v((size_t)N);
    for (int64_t i = 0; i < N; ++i) v[i] = mean[i] = sor_mean(&d2[(size_t)i * kk + 1], cnt[i] - 1);
    const double t = sor_tree(v);
    const double mu = sor_mu(t, N);
    for (int64_t i = 0; i < N; ++i) v[i] = sor_dev2(mean[i], mu);
    const double sigma = sor_sigma(sor_tree(v), N);
    const double thr = sor_thr(mu, s.std_ratio, sigma);
    int64_t M = 0;
    for (int64_t i = 0; i < N; ++i) M += sor_keeps(mean[i], thr) ? 1 : 0;
    check_sor_result(t, M, N, s);
    M = 0;
    for (int64_t i = 0; i < N; ++i) {
        if (out_mean) out_mean[i] = mean[i];
        if (!sor_keeps(mean[i], thr)) continue;
        if (out_xyz)
            for (int a = 0; a < D; ++a) out_xyz[M * D + a] = xyz[i * D + a];
        if (out_index) out_index[M] = i;
        ++M;
    }
    if (out_stats) out_stats[0] = mu, out_stats[1] = sigma, out_stats[2] = thr;
    *M_out = M;
}
}  // namespace

void sor_points_host(const double* xyz, int64_t N, int dim, const gicp_sor* s, double* out_xyz, int64_t* out_index,
                     double* out_mean, double* out_stats, int64_t* M_out) {
    double mn[3], mx[3];
    check_sor_args(xyz, N, dim, s, M_out, mn, mx);   // (a refused call writes nothing, *M_out included)
    if (dim == 3) sor_host<3>(xyz, N, *s, out_xyz, out_index, out_mean, out_stats, M_out);
    else sor_host<2>(xyz, N, *s, out_xyz, out_index, out_mean, out_stats, M_out);
}

// ---- Euclidean cluster extraction (gicp_cluster.h) ----

// what gicp_set_cluster, gicp_cluster_points and gicp_cluster_points_host refuse alike of the setting
void check_cluster(const gicp_cluster& c) {
    if (!(std::isfinite(c.radius) && c.radius > 0.0)) throw Fail{GICP_E_INVALID, "cluster: radius must be finite and > 0"};
    if (c.min_size < 1) throw Fail{GICP_E_INVALID, "cluster: min_size must be >= 1"};
    if (c.max_size < 0 || (c.max_size > 0 && c.max_size < c.min_size)) {
        char b[160];
        std::snprintf(b, sizeof b, "cluster: max_size %d must be 0 (no upper limit) or at least min_size %d", (int)c.max_size,
                      (int)c.min_size);
        throw Fail{GICP_E_INVALID, b};
    }
}

// the argument checks of both one-shot entry points, the finiteness test and the bounds it yields
void check_cluster_args(const double* xyz, int64_t N, int dim, const gicp_cluster* c, double (&mn)[3], double (&mx)[3]) {
    if (!xyz || (dim != 2 && dim != 3)) throw Fail{GICP_E_INVALID, "cluster: the cloud must be an N x 2 or N x 3 array"};
    if (N < 1 || N > (int64_t)0x7FFFFFFF - 64) throw Fail{GICP_E_INVALID, "cluster: the cloud must hold 1 .. 2^31 - 65 rows"};
    if (!c) throw Fail{GICP_E_INVALID, "cluster: the setting must not be NULL"};
    check_cluster(*c);
    try {
        scan_bounds(xyz, N, dim, mn, mx);
    } catch (const Fail& f) {
        throw Fail{f.code, "cluster: " + f.msg};
    }
}

// what a stage of m rows in `clusters` clusters refuses of its own result: no row kept
void check_cluster_result(int64_t kept, int64_t m, int64_t clusters, const gicp_cluster& c) {
    if (kept > 0) return;
    char b[224];
    std::snprintf(b, sizeof b, "cluster: none of the %lld clusters of the %lld points has a size in [min_size %d, max_size %d] (radius %g)",
                  (long long)clusters, (long long)m, (int)c.min_size, (int)c.max_size, c.radius);
    throw Fail{GICP_E_INVALID, b};
}

namespace {
// The host yardstick: a union-find over the pairs the device's grid proposes (the same keys, the same clipped runs)
// and the same predicate decides.  Plain, not fast.
template <int D>
void cluster_host(const double* xyz, int64_t N, const gicp_cluster& c, const double (&mn)[3], const double (&mx)[3], int32_t* labels,
                  int32_t* sizes, int64_t* n_clusters, double* out_xyz, int64_t* out_index, int64_t* M_out) {
    double leaf, cmin[3];
    int32_t bits[3];
    int64_t cmax[3];
    ror_key_bits(D, mn, mx, c.radius, leaf, cmin, bits, cmax, "cluster");
    const std::vector<std::pair<uint64_t, int64_t>> ks = host_keys<D>(xyz, nullptr, N, leaf, cmin, bits);
    std::vector<int32_t> parent((size_t)N);
    for (int64_t i = 0; i < N; ++i) parent[i] = (int32_t)i;
    auto find = [&](int32_t x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    };
    const double r2 = c.radius * c.radius;
    for (int64_t j = 0; j < N; ++j) {
        const int64_t i = ks[j].second;
        host_runs<D>(ks, ks[j].first, bits, cmax, [&](int64_t b, int64_t e) {
            for (int64_t t = b > j ? b : j + 1; t < e; ++t) {
                if (!ror_near(filter_d2<D>(xyz + i * D, xyz + ks[t].second * D), r2)) continue;
                const int32_t ra = find((int32_t)i), rb = find((int32_t)ks[t].second);
                if (ra != rb) parent[ra > rb ? ra : rb] = ra > rb ? rb : ra;   // the larger root below the smaller
            }
        });
    }
    // a root is its cluster's smallest row: numbering the roots as they come numbers the clusters
    std::vector<int32_t> lab((size_t)N), sz;
    for (int64_t i = 0; i < N; ++i) {
        const int32_t r = find((int32_t)i);
        if (r == i) {
            lab[i] = (int32_t)sz.size();
            sz.push_back(0);
        }
        ++sz[lab[i] = lab[r]];
    }
    int64_t M = 0;
    for (int64_t i = 0; i < N; ++i) M += cluster_keeps(sz[lab[i]], c.min_size, c.max_size) ? 1 : 0;
    check_cluster_result(M, N, (int64_t)sz.size(), c);   // (a refused call writes nothing)
    M = 0;
    for (int64_t i = 0; i < N; ++i) {
        if (labels) labels[i] = lab[i];
        if (!cluster_keeps(sz[lab[i]], c.min_size, c.max_size)) continue;
        if (out_xyz)
            for (int a = 0; a < D; ++a) out_xyz[M * D + a] = xyz[i * D + a];
        if (out_index) out_index[M] = i;
        ++M;
    }
    if (sizes)
        for (size_t k = 0; k < sz.size(); ++k) sizes[k] = sz[k];
    if (n_clusters) *n_clusters = (int64_t)sz.size();
    if (M_out) *M_out = M;
}
}  // namespace

void cluster_points_host(const double* xyz, int64_t N, int dim, const gicp_cluster* c, int32_t* labels, int32_t* sizes,
                         int64_t* n_clusters, double* out_xyz, int64_t* out_index, int64_t* M_out) {
    double mn[3], mx[3];
    check_cluster_args(xyz, N, dim, c, mn, mx);
    if (dim == 3) cluster_host<3>(xyz, N, *c, mn, mx, labels, sizes, n_clusters, out_xyz, out_index, M_out);
    else cluster_host<2>(xyz, N, *c, mn, mx, labels, sizes, n_clusters, out_xyz, out_index, M_out);
}

// ---- what every entry point checks the same way ----

void check_cloud_args(const double* xyz, int64_t n, int dim) {
    if (!xyz || n <= 0 || (dim != 2 && dim != 3)) throw Fail{GICP_E_INVALID, "cloud must be a non-empty N x 2 or N x 3 array"};
    if (n > (int64_t)0x7FFFFFFF - 64) throw Fail{GICP_E_INVALID, "cloud too large (> 2^31 points)"};
}

void check_shard(int shard, int nshards) {
    if (nshards < 1 || shard < 0 || shard >= nshards) throw Fail{GICP_E_INVALID, "bad shard / nshards"};
}

// The exception in flight (call inside a catch block) as a GICP_E_* code and its text; the callers add their prefix.
// ---- registration report ----

// H = G^T H_z G and b = -G^T g of the pass's statistics `st` (layout DESIGN.md §4) at pose T, for the left
// perturbation T' = Exp(xi) T: dz = G xi with z = (vec R row-major, t), dR = [w]x R, dt = w x t + v (2-D:
// dR = w J2 R, dt = w J2 t + v).  H [n][n] row-major, b [n], n = 6 (3-D) or 3 (2-D).
void information(int dim, const double* st, const double* T, double* H, double* b) {
    if (dim != 2 && dim != 3) throw Fail{GICP_E_INVALID, "dim must be 2 or 3"};
    if (!st || !T || !H || !b) throw Fail{GICP_E_INVALID, "stats, T, H and b must not be NULL"};
    const int d = dim, n1 = d + 1, ns = d * (d + 1) / 2, nz = d * d + d, n = d == 3 ? 6 : 3, nw = n - d;
    for (int k = 0; k < n1 * n1; ++k)
        if (!std::isfinite(T[k])) throw Fail{GICP_E_INVALID, "pose contains non-finite values"};
    const auto sym = [d](int a, int c) {
        if (a > c) std::swap(a, c);
        return a * d - a * (a - 1) / 2 + (c - a);
    };
    const double* A = st;
    const double* B = A + ns * ns;
    const double* C = B + ns * d;
    const double* g = C + ns;   // gR [d][d], then gt [d]: g in z's order
    double Hz[12][12];
    for (int a = 0; a < d; ++a)
        for (int i = 0; i < d; ++i) {
            for (int c = 0; c < d; ++c) {
                for (int j = 0; j < d; ++j) Hz[a * d + i][c * d + j] = A[sym(a, c) * ns + sym(i, j)];
                Hz[a * d + i][d * d + c] = Hz[d * d + c][a * d + i] = B[sym(a, c) * d + i];
            }
        }
    for (int a = 0; a < d; ++a)
        for (int c = 0; c < d; ++c) Hz[d * d + a][d * d + c] = C[sym(a, c)];
    // G [nz][n]: E[k][a][c] = ([e_k]x)_ac, the generator of axis k (2-D: the one generator J2)
    double G[12][6] = {};
    for (int k = 0; k < nw; ++k) {
        double E[3][3] = {};
        if (d == 2) {
            E[0][1] = -1.0;
            E[1][0] = 1.0;
        } else {
            const int u = (k + 1) % 3, v = (k + 2) % 3;   // e_k x e_u = e_v
            E[v][u] = 1.0;
            E[u][v] = -1.0;
        }
        for (int a = 0; a < d; ++a) {
            for (int i = 0; i < d; ++i) {
                double s = 0.0;
                for (int c = 0; c < d; ++c) s += E[a][c] * T[c * n1 + i];
                G[a * d + i][k] = s;
            }
            double s = 0.0;
            for (int c = 0; c < d; ++c) s += E[a][c] * T[c * n1 + d];
            G[d * d + a][k] = s;
        }
    }
    for (int a = 0; a < d; ++a) G[d * d + a][nw + a] = 1.0;
    double HG[12][6];
    for (int i = 0; i < nz; ++i)
        for (int k = 0; k < n; ++k) {
            double s = 0.0;
            for (int j = 0; j < nz; ++j) s += Hz[i][j] * G[j][k];
            HG[i][k] = s;
        }
    for (int k = 0; k < n; ++k) {
        for (int l = 0; l < n; ++l) {
            double s = 0.0;
            for (int i = 0; i < nz; ++i) s += G[i][k] * HG[i][l];
            H[k * n + l] = s;
        }
        double s = 0.0;
        for (int i = 0; i < nz; ++i) s += G[i][k] * g[i];
        b[k] = -s;
    }
}

// Eigenvalues (ascending) and unit eigenvectors (the columns of V, [n][n] row-major) of the symmetric part of A
// ([n][n] row-major, n <= 6): cyclic Jacobi in fp64.  Each rotation annihilates one off-diagonal pair with the
// stable tangent formula; the sweeps stop when every off-diagonal entry is exactly 0 or so small that its
// rotation no longer changes the diagonal (relative 2^-53), which for these orders takes under ten sweeps.
void sym_eig(int n, const double* A, double* w, double* V) {
    if (n < 1 || n > 6) throw Fail{GICP_E_INVALID, "n must be 1..6"};
    if (!A || !w || !V) throw Fail{GICP_E_INVALID, "A, w and V must not be NULL"};
    double a[6][6], v[6][6];
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            if (!std::isfinite(A[i * n + j])) throw Fail{GICP_E_INVALID, "matrix contains non-finite values"};
            a[i][j] = 0.5 * A[i * n + j] + 0.5 * A[j * n + i];
            v[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 64; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = a[p][q];
                if (apq == 0.0) continue;
                const double app = a[p][p], aqq = a[q][q];
                // negligible: |a_pq| below half an ulp of both diagonal entries
                if (std::fabs(apq) <= 0x1p-54 * std::min(std::fabs(app), std::fabs(aqq))) {
                    a[p][q] = a[q][p] = 0.0;
                    continue;
                }
                rotated = true;
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                a[p][p] = app - t * apq;
                a[q][q] = aqq + t * apq;
                a[p][q] = a[q][p] = 0.0;
                for (int k = 0; k < n; ++k) {
                    if (k != p && k != q) {
                        const double akp = a[k][p], akq = a[k][q];
                        a[k][p] = a[p][k] = c * akp - s * akq;
                        a[k][q] = a[q][k] = s * akp + c * akq;
                    }
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c * vkp - s * vkq;
                    v[k][q] = s * vkp + c * vkq;
                }
            }
        if (!rotated) break;
    }
    int order[6];
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order, order + n, [&](int x, int y) { return a[x][x] < a[y][y]; });
    for (int k = 0; k < n; ++k) {
        w[k] = a[order[k]][order[k]];
        for (int i = 0; i < n; ++i) V[i * n + k] = v[i][order[k]];
    }
}

// The degeneracy part of a report from its H: the spectra of H, its rotation block and its translation block.
void report_spectra(gicp_report* r) {
    const int d = r->dim, n = d == 3 ? 6 : 3, nw = n - d;
    sym_eig(n, r->H, r->eig, r->eigvec);
    double blk[9];
    for (int i = 0; i < nw; ++i)
        for (int j = 0; j < nw; ++j) blk[i * nw + j] = r->H[i * n + j];
    sym_eig(nw, blk, r->eig_rot, r->vec_rot);
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) blk[i * d + j] = r->H[(nw + i) * n + nw + j];
    sym_eig(d, blk, r->eig_trans, r->vec_trans);
}

// The rank of the lower order statistic of probability pi among n values: floor(pi (n - 1)), the product in fp64
int64_t quantile_rank(double pi, int64_t n) {
    const int64_t k = (int64_t)std::floor(pi * (double)(n - 1));
    return std::max<int64_t>(0, std::min(n - 1, k));
}

// what gicp_evaluate refuses of a spec (NULL: nothing asked) under the pass's d_c
void check_report_spec(const gicp_report_spec* s, double dc) {
    if (!s) return;
    if (s->n_thresholds < 0 || s->n_thresholds > GICP_REPORT_MAX)
        throw Fail{GICP_E_INVALID, "n_thresholds must be 0..GICP_REPORT_MAX"};
    if (s->n_quantiles < 0 || s->n_quantiles > GICP_REPORT_MAX)
        throw Fail{GICP_E_INVALID, "n_quantiles must be 0..GICP_REPORT_MAX"};
    for (int j = 0; j < s->n_thresholds; ++j)
        if (!(std::isfinite(s->thresholds[j]) && s->thresholds[j] >= 0.0 && s->thresholds[j] <= dc))
            throw Fail{GICP_E_INVALID, "a threshold must be finite and in [0, max_distance_correspondence] of the pass"};
    for (int j = 0; j < s->n_quantiles; ++j)
        if (!(s->quantiles[j] >= 0.0 && s->quantiles[j] <= 1.0))
            throw Fail{GICP_E_INVALID, "a quantile probability must be in [0, 1]"};
}

int current_failure(std::string& msg) {
    try {
        throw;
    } catch (const Fail& f) {
        msg = f.msg;
        return f.code;
    } catch (const std::bad_alloc&) {
        msg = "out of host memory";
        return GICP_E_NOMEM;
    } catch (...) {
        msg = "unknown error";
        return GICP_E_INVALID;
    }
}

}  // namespace gicp

// The host-only filter lives here, not in gicp_capi.cpp, so that it links without the runtime
// (tests/native/filter_check.cpp).  Its message goes to a per-thread string: it has no context to leave it in.
namespace {
thread_local std::string t_host_err;
}
namespace gicp {
// the message of a call refused before it had a context to leave it in (gicp_batch_align's argument checks)
void set_host_error(const std::string& msg) noexcept {
    try {
        t_host_err = msg;
    } catch (...) {
    }
}
}  // namespace gicp

extern "C" {

int gicp_filter_points_host(const double* xyz, int64_t N, int dim, const gicp_filter* f, double* out_xyz, int64_t* out_index,
                            int32_t* out_count, int64_t* M_out) {
    try {
        gicp::filter_points_host(xyz, N, dim, f, out_xyz, out_index, out_count, M_out);
        return GICP_OK;
    } catch (...) {
        std::string msg;
        const int rc = gicp::current_failure(msg);
        try {
            t_host_err = "gicp_filter_points_host: " + msg;
        } catch (...) {
        }
        return rc == GICP_E_NOMEM ? GICP_E_INVALID : rc;
    }
}

// the host yardstick of the k-nearest-neighbour queries: here for the same reason
int gicp_knn_host(const double* xyz, int64_t M, const double* queries, int64_t Q, int dim, int k, double max_distance,
                  int64_t* index, double* dist2, int32_t* count) {
    try {
        gicp::knn_host(xyz, M, queries, Q, dim, k, max_distance, index, dist2, count);
        return GICP_OK;
    } catch (...) {
        std::string msg;
        const int rc = gicp::current_failure(msg);
        try {
            t_host_err = "gicp_knn_host: " + msg;
        } catch (...) {
        }
        return rc == GICP_E_NOMEM ? GICP_E_INVALID : rc;
    }
}

// ... and of statistical outlier removal
int gicp_sor_points_host(const double* xyz, int64_t N, int dim, const gicp_sor* s, double* out_xyz, int64_t* out_index,
                         double* out_mean, double* out_stats, int64_t* M_out) {
    try {
        gicp::sor_points_host(xyz, N, dim, s, out_xyz, out_index, out_mean, out_stats, M_out);
        return GICP_OK;
    } catch (...) {
        std::string msg;
        const int rc = gicp::current_failure(msg);
        try {
            t_host_err = "gicp_sor_points_host: " + msg;
        } catch (...) {
        }
        return rc == GICP_E_NOMEM ? GICP_E_INVALID : rc;
    }
}

// ... and of Euclidean cluster extraction
int gicp_cluster_points_host(const double* xyz, int64_t N, int dim, const gicp_cluster* c, int32_t* labels, int32_t* sizes,
                             int64_t* n_clusters, double* out_xyz, int64_t* out_index, int64_t* M_out) {
    try {
        gicp::cluster_points_host(xyz, N, dim, c, labels, sizes, n_clusters, out_xyz, out_index, M_out);
        return GICP_OK;
    } catch (...) {
        std::string msg;
        const int rc = gicp::current_failure(msg);
        try {
            t_host_err = "gicp_cluster_points_host: " + msg;
        } catch (...) {
        }
        return rc == GICP_E_NOMEM ? GICP_E_INVALID : rc;
    }
}

const char* gicp_last_host_error(void) { return t_host_err.c_str(); }

}  // extern "C"
