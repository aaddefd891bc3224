// gicp_batch.cpp — batched registration (include/gicp_hip.h gicp_batch_align): the argument
// checks, which need neither a context nor the runtime, the two launches of gicp_batch.hip on the context's
// stream, and the problems' outcomes.  Nothing of the context but its stream and its batch buffers is touched.
#include "gicp_host.h"

namespace gicp {
namespace {

std::string nth(const char* what, long long k) { return std::string(what) + " " + std::to_string(k); }

// Everything gicp_batch_align refuses before anything runs; returns the parameters in force.
gicp_params check_batch_args(int dim, const double* xyz, const int64_t* offsets, int n_clouds,
                             const gicp_batch_problem* problems, int n_problems, const gicp_params* p,
                             const double* T_out) {
    if (dim != 2 && dim != 3) throw Fail{GICP_E_INVALID, "dim must be 2 or 3"};
    if (n_clouds < 1) throw Fail{GICP_E_INVALID, "n_clouds must be >= 1"};
    if (n_problems < 1) throw Fail{GICP_E_INVALID, "n_problems must be >= 1"};
    if (!xyz || !offsets || !problems || !T_out)
        throw Fail{GICP_E_INVALID, "xyz, offsets, problems and T_out must not be NULL"};
    const gicp_params prm = resolve(dim, p);
    const int k = prm.k_neighbors;
    if (!(dim == 2 ? (k == 6 || k == 10) : (k == 10 || k == 20)))
        throw Fail{GICP_E_INVALID, "unsupported k_neighbors for this dim (2-D: 6, 10; 3-D: 10, 20)"};
    if (offsets[0] != 0) throw Fail{GICP_E_INVALID, "offsets must start at 0"};
    const int64_t cap = batch_max_points(dim);
    for (int c = 0; c < n_clouds; ++c) {
        const int64_t n = offsets[c + 1] - offsets[c];
        if (n < 0) throw Fail{GICP_E_INVALID, "offsets do not ascend at " + nth("cloud", c)};
        if (n == 0) throw Fail{GICP_E_INVALID, nth("cloud", c) + " is empty"};
        if (n > cap)
            throw Fail{GICP_E_INVALID, nth("cloud", c) + " has " + std::to_string(n) + " points, more than gicp_batch_max_points = " +
                                           std::to_string(cap) + " (larger clouds: gicp_set_target / gicp_align)"};
    }
    for (int c = 0; c < n_clouds; ++c)
        for (int64_t i = offsets[c] * dim; i < offsets[c + 1] * dim; ++i)
            if (!std::isfinite(xyz[i]))
                throw Fail{GICP_E_INVALID, nth("cloud", c) + " contains non-finite coordinates (row " +
                                               std::to_string(i / dim - offsets[c]) + ")"};
    const int n1 = dim + 1;
    for (int b = 0; b < n_problems; ++b) {
        const gicp_batch_problem& q = problems[b];
        if (q.source < 0 || q.source >= n_clouds || q.target < 0 || q.target >= n_clouds)
            throw Fail{GICP_E_INVALID, nth("problem", b) + " names a cloud out of range (source " + std::to_string(q.source) +
                                           ", target " + std::to_string(q.target) + ", n_clouds " + std::to_string(n_clouds) + ")"};
        for (int e = 0; e < n1 * n1; ++e)
            if (!std::isfinite(q.T0[e])) throw Fail{GICP_E_INVALID, "T0 of " + nth("problem", b) + " contains non-finite values"};
    }
    return prm;
}

size_t align8(size_t n) { return (n + 7) & ~(size_t)7; }

}  // namespace

void batch_align(gicp_ctx* c, int dim, const double* xyz, const int64_t* offsets, int n_clouds,
                 const gicp_batch_problem* problems, int n_problems, const gicp_params& prm, double* T_out,
                 gicp_batch_result* res, gicp_batch_debug* dbg) {
    hipStream_t st = c->stream;
    const int64_t rows = offsets[n_clouds];
    const int n1 = dim + 1, nss = nstat(dim);
    // the work list of the covariances, the debug rows' starts, the largest cloud and the largest target
    std::vector<int2> work;
    int cap_all = 1, cap_tgt = 1;
    for (int k = 0; k < n_clouds; ++k) {
        const int n = (int)(offsets[k + 1] - offsets[k]);
        cap_all = std::max(cap_all, n);
        for (int i = 0; i < n; i += kBatchThreads) work.push_back(make_int2(k, i));
    }
    std::vector<int64_t> row0((size_t)n_problems);
    int64_t src_rows = 0;
    for (int b = 0; b < n_problems; ++b) {
        row0[b] = src_rows;
        src_rows += offsets[problems[b].source + 1] - offsets[problems[b].source];
        cap_tgt = std::max<int>(cap_tgt, (int)(offsets[problems[b].target + 1] - offsets[problems[b].target]));
    }
    // one upload for the points, one for everything else (each part 8-byte aligned)
    const size_t o_off = 0, o_row0 = o_off + sizeof(int64_t) * ((size_t)n_clouds + 1);
    const size_t o_work = o_row0 + sizeof(int64_t) * (size_t)n_problems;
    const size_t o_prob = o_work + align8(sizeof(int2) * work.size());
    const size_t meta_bytes = o_prob + sizeof(gicp_batch_problem) * (size_t)n_problems;
    static_assert(sizeof(gicp_batch_problem) % 8 == 0, "problems stay 8-byte aligned in the packed upload");
    std::vector<unsigned char> meta(meta_bytes);
    std::memcpy(meta.data() + o_off, offsets, sizeof(int64_t) * ((size_t)n_clouds + 1));
    std::memcpy(meta.data() + o_row0, row0.data(), sizeof(int64_t) * (size_t)n_problems);
    std::memcpy(meta.data() + o_work, work.data(), sizeof(int2) * work.size());
    std::memcpy(meta.data() + o_prob, problems, sizeof(gicp_batch_problem) * (size_t)n_problems);

    c->b_xyz.reserve((size_t)rows * dim);
    c->b_meta.reserve(meta_bytes);
    c->b_cov.reserve((size_t)rows);
    c->b_cnt.reserve((size_t)rows);
    c->b_out.reserve((size_t)n_problems);
    const bool want_cov = dbg && dbg->covariances, want_idx = dbg && dbg->index, want_dist = dbg && dbg->distance;
    if (want_cov) c->b_dbg_cov.reserve((size_t)rows * dim * dim);
    if (want_idx) c->b_dbg_idx.reserve((size_t)src_rows);
    if (want_dist) c->b_dbg_dist.reserve((size_t)src_rows);
    HIPCHK(hipMemcpyAsync(c->b_xyz, xyz, sizeof(double) * rows * dim, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->b_meta, meta.data(), meta_bytes, hipMemcpyHostToDevice, st));
    unsigned char* const dm = c->b_meta;
    const int64_t* const d_off = reinterpret_cast<const int64_t*>(dm + o_off);

    BatchCovArgs ca{};
    ca.xyz = c->b_xyz;
    ca.offsets = d_off;
    ca.work = reinterpret_cast<const int2*>(dm + o_work);
    ca.cap = cap_all;
    ca.min_nb = prm.min_neighbors;
    const double dn = prm.max_distance_nearest_neighbors;
    ca.dn2 = dn * dn;
    ca.eps_a = prm.epsilon;
    ca.m_scale = std::sqrt(prm.epsilon * (1.0 - prm.ratio));
    ca.cov = c->b_cov;
    ca.count = c->b_cnt;
    ca.dbg_cov = want_cov ? c->b_dbg_cov.get() : nullptr;
    HIPCHK(launch_batch_cov(ca, dim, prm.k_neighbors, (int)work.size(), st));

    BatchArgs a{};
    a.xyz = c->b_xyz;
    a.offsets = d_off;
    a.cov = c->b_cov;
    a.prob = reinterpret_cast<const gicp_batch_problem*>(dm + o_prob);
    a.row0 = reinterpret_cast<const int64_t*>(dm + o_row0);
    a.cap = cap_tgt;
    a.max_iter = prm.max_iterations;
    a.fixed = prm.fixed_iterations ? 1 : 0;
    a.cov_model = prm.cov_model;
    a.robust_kernel = prm.robust_kernel;
    a.tol = prm.tolerance;
    a.trans_eps = prm.transformation_epsilon;
    a.rot_cos = prm.rotation_epsilon;
    a.fit_eps = prm.euclidean_fitness_epsilon;
    a.rel_eps = prm.mse_relative_epsilon;
    a.dc2_max = accept_d2_max(prm.max_distance_correspondence);
    a.pl_inv = 1.0 / (prm.epsilon * (1.0 - prm.ratio));
    a.robust_c = prm.robust_scale;
    a.robust_c2 = prm.robust_scale * prm.robust_scale;
    a.out = c->b_out;
    a.dbg_index = want_idx ? c->b_dbg_idx.get() : nullptr;
    a.dbg_dist = want_dist ? c->b_dbg_dist.get() : nullptr;
    HIPCHK(launch_batch_align(a, dim, n_problems, st));

    std::vector<BatchOut> out((size_t)n_problems);
    HIPCHK(hipMemcpyAsync(out.data(), c->b_out, sizeof(BatchOut) * (size_t)n_problems, hipMemcpyDeviceToHost, st));
    std::vector<int64_t> h_idx;
    std::vector<double> h_dist;
    // (a problem that ran no pass, max_iterations < 1, wrote no debug row: those read as rejected, at infinity)
    const bool ran = prm.max_iterations > 0;
    if (want_idx && ran) {
        h_idx.resize((size_t)src_rows);
        HIPCHK(hipMemcpyAsync(h_idx.data(), c->b_dbg_idx, sizeof(int64_t) * src_rows, hipMemcpyDeviceToHost, st));
    }
    if (want_dist && ran) {
        h_dist.resize((size_t)src_rows);
        HIPCHK(hipMemcpyAsync(h_dist.data(), c->b_dbg_dist, sizeof(double) * src_rows, hipMemcpyDeviceToHost, st));
    }
    std::vector<double> h_cov;
    std::vector<int32_t> h_cnt;
    if (want_cov) {
        h_cov.resize((size_t)rows * dim * dim);
        HIPCHK(hipMemcpyAsync(h_cov.data(), c->b_dbg_cov, sizeof(double) * h_cov.size(), hipMemcpyDeviceToHost, st));
    }
    if (dbg && dbg->neighbor_counts) {
        h_cnt.resize((size_t)rows);
        HIPCHK(hipMemcpyAsync(h_cnt.data(), c->b_cnt, sizeof(int32_t) * rows, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    // nothing failed: only now are the caller's outputs written
    if (want_cov) std::memcpy(dbg->covariances, h_cov.data(), sizeof(double) * h_cov.size());
    if (!h_cnt.empty()) std::memcpy(dbg->neighbor_counts, h_cnt.data(), sizeof(int32_t) * rows);
    if (want_idx) {
        if (ran) std::memcpy(dbg->index, h_idx.data(), sizeof(int64_t) * src_rows);
        else std::fill(dbg->index, dbg->index + src_rows, (int64_t)-1);
    }
    if (want_dist) {
        if (ran) std::memcpy(dbg->distance, h_dist.data(), sizeof(double) * src_rows);
        else std::fill(dbg->distance, dbg->distance + src_rows, (double)INFINITY);
    }
    const int NS = dim * (dim + 1) / 2;
    for (int b = 0; b < n_problems; ++b) {
        const BatchOut& o = out[b];
        std::memcpy(T_out + (size_t)b * n1 * n1, o.T, sizeof(double) * n1 * n1);
        if (dbg && dbg->stats) {
            double* s = dbg->stats + (size_t)b * GICP_MAX_STATS;
            std::memcpy(s, o.stats, sizeof(double) * nss);
            std::fill(s + nss, s + GICP_MAX_STATS, 0.0);
        }
        if (!res) continue;
        // gicp_align's rule (gicp_align.cpp zero_weight): a robust pass whose weights are all 0 has an
        // identically zero quadratic, which every pose minimises -- no failure
        const double* Cw = o.stats + NS * NS + NS * dim;
        const bool zero_weight = std::all_of(Cw, Cw + NS, [](double x) { return x == 0.0; });
        gicp_batch_result r;
        std::memset(&r, 0, sizeof(r));
        // a last pass without a correspondence has no statistics to solve from (the device solve leaves the pose
        // and reports nothing, as gicp_align's does): a failed problem here
        const bool none = o.iterations > 0 && o.stats[nss - 1] == 0.0;
        r.status = none || (o.solve_fail && !(prm.robust_kernel != GICP_ROBUST_NONE && zero_weight)) ? GICP_E_INVALID : GICP_OK;
        r.iterations = o.iterations;
        r.converged = o.converged;
        r.converged_at = o.converged ? o.converged_at : -1;
        r.stop_reason = o.converged ? o.stop_reason : GICP_STOP_NONE;
        r.correspondences = (int64_t)o.stats[nss - 1];
        r.final_loss = o.loss;
        r.mse = o.mse;
        res[b] = r;
    }
}

}  // namespace gicp

extern "C" {

int gicp_batch_max_points(int dim) { return gicp::batch_max_points(dim); }

int gicp_batch_align(gicp_ctx* c, int dim, const double* xyz, const int64_t* offsets, int n_clouds,
                     const gicp_batch_problem* problems, int n_problems, const gicp_params* p, double* T_out,
                     gicp_batch_result* res, gicp_batch_debug* dbg) {
    using namespace gicp;
    const auto failed = [&](const char* stage) {   // (inside a catch block)
        std::string msg;
        int rc = current_failure(msg);
        msg = std::string("gicp_batch_align: ") + msg;
        if (stage) {
            set_host_error(msg);
            if (rc == GICP_E_NOMEM) rc = GICP_E_INVALID;
        }
        try {
            if (c) c->err = msg;
        } catch (...) {
        }
        return rc;
    };
    gicp_params prm;
    try {
        prm = check_batch_args(dim, xyz, offsets, n_clouds, problems, n_problems, p, T_out);
    } catch (...) {
        return failed("arguments");
    }
    if (!c) {
        set_host_error("gicp_batch_align: the context must not be NULL");
        return GICP_E_INVALID;
    }
    try {
        HIPCHK(hipSetDevice(c->device));
        batch_align(c, dim, xyz, offsets, n_clouds, problems, n_problems, prm, T_out, res, dbg);
        return GICP_OK;
    } catch (...) {
        return failed(nullptr);
    }
}

}  // extern "C"
