// gicp_align.cpp — the registration itself: the per-source-tile state, one pass at a pose (gicp_iterate), and
// the batched outer loop of gicp.py:116-167 with its trace, timing and diagnostics (gicp_align_trace).
#include <atomic>

#include "gicp_host.h"

namespace gicp {
namespace {

void ensure_workspace(gicp_ctx* c) {
    const int nsx = nstat_ext(3);
    const int grid = std::max(1, corr_grid(c->src.ntiles, c->shard, c->nshards));
    if ((grid + kGroupWG - 1) / kGroupWG > kMaxGroups) throw Fail{GICP_E_INVALID, "source shard too large"};
    c->d_partials.reserve((size_t)grid * nsx);
    // the fixed state block, each buffer on its own first use (tickets and the pinned mirror start zeroed)
    if (!c->d_state) c->d_state.alloc(1);
    if (!c->h_state) alloc_init(c->h_state, 1, [](IterState* h) { std::memset(h, 0, sizeof(IterState)); });
    if (!c->d_tickets) {
        const size_t nt = (size_t)(kMaxGroups + 1) * kTicketStride;
        alloc_init(c->d_tickets, nt, [&](uint32_t* d) { HIPCHK(hipMemsetAsync(d, 0, sizeof(uint32_t) * nt, c->stream)); });
    }
    if (!c->d_gpart) c->d_gpart.alloc((size_t)kMaxGroups * nsx);
}

// what a pass and the loop need before anything else: both clouds, of one dimension
void require_clouds(const gicp_ctx* c) {
    if (!c->tgt.n || !c->src.n) throw Fail{GICP_E_STATE, "set_target and set_source first"};
    if (c->tgt.dim != c->src.dim) throw Fail{GICP_E_INVALID, "source and target dimensions differ"};
}

// The head of the device state (all before IterState::stats; xchg_* = 0) for a start at the finite pose T (NULL:
// identity), uploaded on the context's stream.  prm: the loop's stopping rules and last_loss = inf
// (gicp.py:106-110); a single pass has none.
void upload_state(gicp_ctx* c, const double* T, const gicp_params* prm) {
    const int n1 = c->src.dim + 1;
    IterState& hs = *c->h_state;
    std::memset(&hs, 0, offsetof(IterState, stats));
    for (int k = 0; k < n1 * n1; ++k) hs.T[k] = T ? T[k] : ((k % (n1 + 1)) == 0 ? 1.0 : 0.0);
    if (prm) {
        hs.last_loss = INFINITY;
        hs.tol = prm->tolerance;
        hs.fixed = prm->fixed_iterations ? 1 : 0;
        hs.trans_eps = prm->transformation_epsilon;
        hs.rot_cos = prm->rotation_epsilon;
        hs.fit_eps = prm->euclidean_fitness_epsilon;
        hs.rel_eps = prm->mse_relative_epsilon;
        hs.prev_mse = INFINITY;
        hs.pairs_total = 0.0;
    }
    hs.converged_at = -1;
    HIPCHK(hipMemcpyAsync(c->d_state, &hs, offsetof(IterState, stats), hipMemcpyHostToDevice, c->stream));
}

// kernel arguments of a pass (the pose comes from the device state)
CorrArgs corr_args(gicp_ctx* c, int single_pass) {
    const int d = c->src.dim;
    CorrArgs a{};
    a.src = c->src.view();
    a.tgt = c->tgt.view();
    a.q_begin = c->q_begin;
    a.q_end = c->q_end;
    a.sh_skip = (c->nshards - 1) * kShardChunk;
    a.sh_first = c->shard * kShardChunk;
    a.unit_map = c->unit_map;
    a.state = c->d_state;
    a.tickets = c->d_tickets;
    a.gpart = c->d_gpart;
    a.single_pass = single_pass;
    const double dc = c->psrc.max_distance_correspondence;
    a.dc = dc;
    a.dc2_max = accept_d2_max(dc);
    // with certificates the screen reaches kappa past d_c, so an empty lane's radius outlasts small moves
    const double kappa = c->use_certs ? c->kappa_frac * dc : 0.0;
    a.mg = make_margin(d, c->src.rho, c->tgt.rho, dc + kappa);
    a.search2 = screen_bound(a.mg, dc + kappa);
    a.kappa = (float)kappa;
    a.empty_r = (float)dc * (1.0f + 1e-6f);
    if (c->use_certs) {
        a.cert_j = c->d_cert_j;
        a.cert_gap = c->d_cert_gap;
    }
    a.cert_pass = c->d_cert_pass;   // always valid: k_corr reads it (and hint) unconditionally, with the tile metadata
    a.hint = c->d_hint;
    a.partials = c->d_partials;
    a.count_pairs = 1;
    a.list = c->d_list;
    a.list_len = c->d_list_len;
    a.list_rcert = c->d_list_rcert;
    a.list_pass = c->d_list_pass;
    a.poses = c->d_poses;
    a.pass = ++c->pass;
    a.use_lists = c->use_lists ? 1 : 0;
    a.sparse_max = c->sparse_max;
    a.sparse_amb = c->sparse_amb;
    a.skin = (float)(c->skin_frac * dc);
    a.skin_gain = (float)c->skin_gain;
    a.skin_max = (float)dc;
    a.gap_slack = (float)std::ldexp(std::sqrt((double)a.search2) + 2.0 * c->tgt.rho + 2.0 * c->src.rho, -19);
    a.cov_model = c->psrc.cov_model;
    a.pl_inv = 1.0 / (c->ptgt.epsilon * (1.0 - c->ptgt.ratio));   // target m = sqrt(eps (1 - ratio)) n
    a.robust_kernel = c->psrc.robust_kernel;
    a.robust_c = c->psrc.robust_scale;   // (both unread with GICP_ROBUST_NONE)
    a.robust_c2 = c->psrc.robust_scale * c->psrc.robust_scale;
    if (c->peer.n > 1) a.peer = c->peer;   // (the exchange's sequence number is counted on the device)
    return a;
}

// k_corr over this shard's `grid` workgroups; with no tile in the shard one empty workgroup still takes part in
// the peer exchange, and without an exchange the statistics are just cleared
void launch_pass(gicp_ctx* c, CorrArgs& a, int d, int grid) {
    if (grid > 0) {
        HIPCHK(launch_corr(a, d, grid, c->stream));
    } else if (a.peer.n > 1) {
        a.q_end = 0;
        HIPCHK(launch_corr(a, d, 1, c->stream));
    } else {
        HIPCHK(hipMemsetAsync(c->d_state->stats, 0, sizeof(double) * nstat_ext(d), c->stream));
    }
}

void allreduce_stats(gicp_ctx* c) {
    const int nsx = nstat_ext(c->src.dim);
    if (c->peer.n > 1) return;   // summed inside k_corr
    if (c->hook) {   // host exchange: statistics out, the caller's sum over ranks back in
        HIPCHK(hipMemcpyAsync(c->h_xchg, c->d_state->stats, sizeof(double) * nsx, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (c->hook(c->h_xchg, nsx, c->hook_user) != 0) throw Fail{GICP_E_COMM, "host all-reduce hook failed"};
        HIPCHK(hipMemcpyAsync(c->d_state->stats, c->h_xchg, sizeof(double) * nsx, hipMemcpyHostToDevice, c->stream));
        return;
    }
    if (!c->comm) return;
    ncclResult_t r = ncclAllReduce(c->d_state->stats, c->d_state->stats, nsx, ncclFloat64, ncclSum, c->comm, c->stream);
    if (r != ncclSuccess) throw Fail{GICP_E_COMM, std::string("ncclAllReduce: ") + ncclGetErrorString(r)};
}

// det(W) rows of other shards stay NaN (never selected); one shard writes every row
void fill_other_shards_det(gicp_ctx* c) {
    if (c->nshards > 1) HIPCHK(hipMemsetAsync(c->d_dbg_det, 0xFF, sizeof(double) * c->src.n, c->stream));
}

// solve_fail = 2 is the device's report that the peer exchange gave up waiting
void check_peer_timeout(int solve_fail) {
    if (solve_fail == 2) throw Fail{GICP_E_COMM, "peer exchange timed out (a rank did not arrive)"};
}

// the diagnostics of the last pass (gicp_pass_info), from the extended statistics `ext` = stats + nstat(d)
void record_pass_info(gicp_ctx* c, const double* ext) {
    c->last_amb = ext[0];
    c->last_pairs = ext[1];
    c->last_rebuilds = ext[2];
    c->last_sq = ext[3];
    c->last_gproved = ext[4];
    c->last_walked = ext[5];
}

#if defined(GICP_STAMPS) || defined(GICP_TIMELINE)
// Diagnostic build: per wave 8 phase-cycle slots (7 = rows scanned) + 8 event counters.
void print_stamps(const unsigned long long* d_stamps, size_t nst) {
    constexpr int W = 20;
    std::vector<unsigned long long> hs(nst);
    HIPCHK(hipMemcpy(hs.data(), d_stamps, nst * 8, hipMemcpyDeviceToHost));
    if (const char* f = std::getenv("GICP_STAMPS_DUMP")) {   // raw [waves][20] u64 for offline analysis
        static int seq = 0;
        const std::string path = std::string(f) + "." + std::to_string(seq++);
        if (FILE* fp = std::fopen(path.c_str(), "wb")) {
            std::fwrite(hs.data(), 8, hs.size(), fp);
            std::fclose(fp);
        }
    }
    std::vector<std::pair<double, size_t>> byc;
    double tot[W] = {0}, all = 0;
    for (size_t w = 0; w < nst / W; ++w) {
        double r = 0;
        for (int k = 0; k < 7; ++k) r += (double)hs[w * W + k];
        if (r <= 0) continue;
        byc.push_back({r, w});
        all += r;
        for (int k = 0; k < W; ++k) tot[k] += (double)hs[w * W + k];
    }
    if (byc.empty()) return;
    std::sort(byc.begin(), byc.end());
    const size_t nw = byc.size(), n1 = std::max<size_t>(1, nw / 100);
    static const char* nm[W] = {"setup", "trav", "stage", "scan", "fb", "epi", "red", "rows",
                                "visits", "scanned", "chunks", "list", "listlen", "blktests", "candblk", "fbtiles",
                                "t0", "t1", "hwid", "xcc"};
    auto row = [&](const char* tag, size_t b, size_t e) {
        double m[W] = {0};
        for (size_t i = b; i < e; ++i)
            for (int k = 0; k < W; ++k) m[k] += (double)hs[byc[i].second * W + k] / (double)(e - b);
        std::fprintf(stderr, "[stamps] %-9s", tag);
        for (int k = 0; k < 16; ++k) std::fprintf(stderr, " %s %.6g", nm[k], m[k]);
        std::fprintf(stderr, "\n");
    };
    row("all", 0, nw);
    row("median1%", nw / 2 - n1 / 2, nw / 2 - n1 / 2 + n1);
    row("slowest1%", nw - n1, nw);
    for (size_t i = nw - std::min<size_t>(nw, 4); i < nw; ++i) {
        char tag[32];
        std::snprintf(tag, sizeof tag, "w%zu", byc[i].second);
        row(tag, i, i + 1);
    }
    std::fprintf(stderr, "[stamps] wave cycles p50 %.0f p90 %.0f p99 %.0f p999 %.0f max %.0f\n", byc[nw / 2].first,
                 byc[nw * 9 / 10].first, byc[nw * 99 / 100].first, byc[nw * 999 / 1000].first, byc.back().first);
    std::fprintf(stderr, "[stamps] waves %zu, mean cycles/wave %.0f:", nw, all / (double)nw);
    for (int k = 0; k < 7; ++k) std::fprintf(stderr, " %s %.1f%%", nm[k], 100.0 * tot[k] / std::max(1.0, all));
    std::fprintf(stderr, "\n");
}
#endif

// per-point debug outputs of a pass (gicp_debug) and the det(W) record of the top-k, grow-only
void ensure_dbg(gicp_ctx* c) {
    const size_t n = (size_t)c->src.n;
    c->d_dbg_idx.reserve(n);
    c->d_dbg_w.reserve(n * 9);
    c->d_dbg_dist.reserve(n);
    c->d_dbg_det.reserve(n);
    c->d_top_tgt.reserve(n);
}

constexpr int kTopBlocks = 256;   // stage-1 blocks of the top-k of det(W)

void ensure_top_scratch(gicp_ctx* c) {
    if (!c->d_top_v) c->d_top_v.alloc((size_t)kTopBlocks * 16 + 16);
    if (!c->d_top_i) c->d_top_i.alloc((size_t)kTopBlocks * 16);
    if (!c->d_top_out) c->d_top_out.alloc(32);
}

}  // namespace

// Per-source-tile state that refers to target tiles (hints, candidate lists, heavy schedule):
// reset whenever either cloud changes.
void reset_tile_state(gicp_ctx* c) {
    const int nt = std::max(1, c->src.ntiles);
    if (!c->d_hint) return;
    // hints -1, lists empty, certificates none (cert_pass -1) and no last match (cert_j -1: k_corr's per-lane
    // search cap) -- one launch (five memsets were five queue operations, ~40 us of a C5 frame)
    HIPCHK(launch_reset_tiles(c->d_hint, c->d_list_len, c->d_list_rcert, c->d_cert_pass, nt, c->d_cert_j,
                              c->d_cert_j ? std::max<int64_t>(1, c->src.n) : 0, c->d_poses, c->stream));
    c->pass = 0;
}

void set_shard(gicp_ctx* c, int shard, int nshards) {
    check_shard(shard, nshards);
    if (c->src.cov_nshards > 1 && (c->src.cov_nshards != nshards || c->src.cov_shard != shard))
        throw Fail{GICP_E_INVALID, "the source's covariances were computed for another shard"};
    c->shard = shard;
    c->nshards = nshards;
    c->q_begin = 0;   // k_corr maps this rank's units onto the cloud's (interleaved chunks)
    c->q_end = c->src.ntiles;
    const int nt = std::max(1, c->src.ntiles);
    c->d_hint.reserve(nt);
    c->d_list.reserve((size_t)nt * kListMax);
    c->d_list_len.reserve(nt);
    c->d_list_pass.reserve(nt);
    c->d_list_rcert.reserve(nt);
    if (!c->d_poses) c->d_poses.alloc((size_t)kPoseRing * 12);
    c->d_cert_j.reserve((size_t)std::max<int64_t>(1, c->src.n));
    c->d_cert_gap.reserve((size_t)std::max<int64_t>(1, c->src.n));
    c->d_cert_pass.reserve(nt);
    reset_tile_state(c);
}

// Top-k of the last pass's det(W) (k_top1 / k_top2) and its copy into the pinned c->h_top, enqueued on
// the library's stream (the caller synchronises).
void top_enqueue(gicp_ctx* c, int k) {
    ensure_top_scratch(c);
    if (!c->h_top) c->h_top.alloc(32 + 16);   // 32 int64, then 16 double
    double* ov = c->d_top_v + (size_t)kTopBlocks * 16;
    HIPCHK(launch_top_weights(c->d_dbg_det, c->d_top_tgt, c->src.perm, c->src.n, k, c->d_top_v, c->d_top_i, kTopBlocks,
                              ov, c->d_top_out, c->d_top_out + 16, c->stream));
    HIPCHK(hipMemcpyAsync(c->h_top, c->d_top_out, sizeof(int64_t) * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(c->h_top + 32, ov, sizeof(double) * 16, hipMemcpyDeviceToHost, c->stream));
}

// One pass at pose T: statistics (all-reduced) into c->h_stats.  keep_on_device: the pass writes index, weight
// and distance of every row into d_dbg_idx / d_dbg_w / d_dbg_dist and none is copied out (gicp_evaluate).
void run_pass(gicp_ctx* c, const double* T, gicp_debug* dbg, bool keep_on_device) {
    require_clouds(c);
    const int d = c->src.dim;
    for (int k = 0; k < (d + 1) * (d + 1); ++k)
        if (!std::isfinite(T[k])) throw Fail{GICP_E_INVALID, "pose contains non-finite values"};
    ensure_workspace(c);
    hipStream_t st = c->stream;
    upload_state(c, T, nullptr);
    CorrArgs a = corr_args(c, 1);
    c->top_ready = false;
    if (keep_on_device || (dbg && (dbg->index || dbg->weight || dbg->distance || dbg->want_top_weights))) {
        ensure_dbg(c);
        a.dbg_index = keep_on_device || dbg->index ? c->d_dbg_idx : nullptr;
        a.dbg_weight = keep_on_device || dbg->weight ? c->d_dbg_w : nullptr;
        a.dbg_dist = keep_on_device || dbg->distance ? c->d_dbg_dist : nullptr;
        if (dbg && dbg->want_top_weights) {
            fill_other_shards_det(c);
            a.dbg_det = c->d_dbg_det;
            a.top_tgt = c->d_top_tgt;
        }
    }
    const int nsx = nstat_ext(d);
    const int grid = corr_grid(c->src.ntiles, c->shard, c->nshards);
#if defined(GICP_STAMPS) || defined(GICP_TIMELINE)
    const size_t nst = (size_t)std::max(1, grid) * kCorrWaves * 20;
    c->d_stamps.reserve(nst);
    unsigned long long* const d_stamps = c->d_stamps;
    HIPCHK(hipMemsetAsync(d_stamps, 0, nst * 8, st));
    a.stamps = d_stamps;
#endif
    launch_pass(c, a, d, grid);
    allreduce_stats(c);
    HIPCHK(hipMemcpyAsync(c->h_stats, c->d_state->stats, sizeof(double) * nsx, hipMemcpyDeviceToHost, st));
    c->top_cached_k = 0;
    if (a.dbg_det && c->src.n > 0) {   // the top-k in the same stream sync as the pass
        top_enqueue(c, c->top_k_pref);
        c->top_cached_k = c->top_k_pref;
    }
    if (dbg) {
        const size_t n = (size_t)c->src.n;
        if (dbg->index) HIPCHK(hipMemcpyAsync(dbg->index, c->d_dbg_idx, sizeof(int64_t) * n, hipMemcpyDeviceToHost, st));
        if (dbg->weight)
            HIPCHK(hipMemcpyAsync(dbg->weight, c->d_dbg_w, sizeof(double) * n * d * d, hipMemcpyDeviceToHost, st));
        if (dbg->distance)
            HIPCHK(hipMemcpyAsync(dbg->distance, c->d_dbg_dist, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    if (a.peer.n > 1) {
        int fail = 0;
        HIPCHK(hipMemcpy(&fail, &c->d_state->solve_fail, sizeof(int), hipMemcpyDeviceToHost));
        check_peer_timeout(fail);
    }
#if defined(GICP_STAMPS) || defined(GICP_TIMELINE)
    print_stamps(d_stamps, nst);
#endif
    record_pass_info(c, c->h_stats + nstat(d));
    c->top_ready = a.dbg_det != nullptr;
}

// The report of one pass at pose T: run_pass with its per-point outputs kept on the device, the
// overlap table and the quantiles reduced there (gicp_eval.hip), H, b and the spectra on the host from the pass's
// statistics.  p's d_c, cov_model and robust kernel hold for this pass alone.
void evaluate(gicp_ctx* c, const double* T, const gicp_params* p, const gicp_report_spec* spec, gicp_report* out) {
    require_clouds(c);
    if (c->nshards > 1) throw Fail{GICP_E_STATE, "gicp_evaluate needs an unsharded source (nshards == 1)"};
    if (c->comm || c->hook || c->peer.n > 1)
        throw Fail{GICP_E_STATE, "gicp_evaluate needs a context without a communicator, host hook or peer exchange"};
    if (!out) throw Fail{GICP_E_INVALID, "out must not be NULL"};
    const int d = c->src.dim, n1 = d + 1;
    // the values in force come back whatever happens below
    struct Restore {
        gicp_params& live;
        const gicp_params saved;
        ~Restore() {
            live.max_distance_correspondence = saved.max_distance_correspondence;
            live.cov_model = saved.cov_model;
            live.robust_kernel = saved.robust_kernel;
            live.robust_scale = saved.robust_scale;
        }
    } restore{c->psrc, c->psrc};
    const gicp_params prm = p ? resolve(d, p) : c->psrc;
    check_report_spec(spec, prm.max_distance_correspondence);
    double Tid[16];
    for (int k = 0; k < n1 * n1; ++k) Tid[k] = T ? T[k] : ((k % (n1 + 1)) == 0 ? 1.0 : 0.0);
    c->psrc.max_distance_correspondence = prm.max_distance_correspondence;
    c->psrc.cov_model = prm.cov_model;
    c->psrc.robust_kernel = prm.robust_kernel;
    c->psrc.robust_scale = prm.robust_scale;
    run_pass(c, Tid, nullptr, true);

    gicp_report r;
    std::memset(&r, 0, sizeof(r));
    const double* st = c->h_stats;
    r.dim = d;
    r.n_thresholds = spec ? spec->n_thresholds : 0;
    r.n_quantiles = spec ? spec->n_quantiles : 0;
    r.n_source = c->src.n;
    r.n_matched = (int64_t)st[nstat(d) - 1];
    r.sum_sq = c->last_sq;
    r.loss = st[nstat(d) - 2];
    information(d, st, Tid, r.H, r.b);
    report_spectra(&r);
    for (int j = 0; j < GICP_REPORT_MAX; ++j) r.dist_q[j] = r.white_q[j] = std::nan("");
    const int nq = r.n_matched > 0 ? r.n_quantiles : 0;   // no accepted row: every quantile stays NaN
    if (r.n_thresholds > 0 || nq > 0) {
        const size_t N = (size_t)c->src.n;
        EvalArgs a{};
        a.idx = c->d_dbg_idx;
        a.dist = c->d_dbg_dist;
        a.w = c->d_dbg_w;
        a.src_xyz = c->src.rec;
        a.src_inv = c->src.inv;
        a.tgt_xyz = c->tgt.rec;
        a.tgt_inv = c->tgt.inv;
        a.n = c->src.n;
        a.m = c->tgt.n;
        a.dim = d;
        a.nthr = r.n_thresholds;
        a.nq = nq;
        for (int i = 0; i < d; ++i) {
            for (int k = 0; k < d; ++k) a.R[i * 3 + k] = Tid[i * n1 + k];
            a.t[i] = Tid[i * n1 + d];
        }
        for (int j = 0; j < a.nthr; ++j) a.thr[j] = spec->thresholds[j];
        for (int j = 0; j < nq; ++j)
            a.rank[j] = a.rank[kEvalMax + j] = (unsigned long long)quantile_rank(spec->quantiles[j], r.n_matched);
        if (nq > 0) c->d_eval_keys.reserve(2 * N);
        c->d_eval_part.reserve((N + kEvalBlock - 1) / kEvalBlock * kEvalMax);
        if (!c->d_eval_sel) c->d_eval_sel.alloc(1);
        if (!c->d_eval_hist) c->d_eval_hist.alloc((size_t)kSelQueries * kSelBins);
        if (!c->d_eval_out) c->d_eval_out.alloc(kEvalOutWords);
        if (!c->h_eval_out) c->h_eval_out.alloc(kEvalOutWords);
        a.keys = c->d_eval_keys;
        a.part = c->d_eval_part;
        a.sel = c->d_eval_sel;
        a.hist = c->d_eval_hist;
        a.out = c->d_eval_out;
        HIPCHK(launch_eval(a, c->stream));
        HIPCHK(hipMemcpyAsync(c->h_eval_out, c->d_eval_out, sizeof(unsigned long long) * kEvalOutWords, hipMemcpyDeviceToHost,
                              c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        const unsigned long long* w = c->h_eval_out;
        for (int j = 0; j < a.nthr; ++j) {
            r.inliers[j] = (int64_t)w[kEvalOutCnt + j];
            std::memcpy(&r.inlier_sum_sq[j], &w[kEvalOutSum + j], sizeof(double));
        }
        for (int j = 0; j < nq; ++j) {
            std::memcpy(&r.dist_q[j], &w[kEvalOutKey + j], sizeof(double));
            std::memcpy(&r.white_q[j], &w[kEvalOutKey + kEvalMax + j], sizeof(double));
        }
    }
    *out = r;
}

void align_trace(gicp_ctx* c, const double* T0, const gicp_params* p, double* T_out, gicp_result* res, gicp_trace* trace) {
    require_clouds(c);
    const int d = c->src.dim, n1 = d + 1;
    gicp_params prm = p ? resolve(d, p) : c->psrc;
    c->psrc.max_distance_correspondence = prm.max_distance_correspondence;
    c->psrc.cov_model = prm.cov_model;
    c->psrc.robust_kernel = prm.robust_kernel;
    c->psrc.robust_scale = prm.robust_scale;
    ensure_workspace(c);
    hipStream_t st = c->stream;
    // per-iteration trace rows (gicp_trace): pose + loss from k_solve, top-k rows after k_corr
    const int HS = n1 * n1 + 1;
    const int tk = trace ? trace->top_k : 0;
    if (trace) {
        if (trace->capacity < std::max(0, prm.max_iterations))
            throw Fail{GICP_E_INVALID, "gicp_trace.capacity < max_iterations"};
        if (tk < 0 || tk > 16) throw Fail{GICP_E_INVALID, "gicp_trace.top_k must be 0..16"};
        const size_t rows = (size_t)std::max(1, prm.max_iterations);
        c->d_hist.reserve(rows * HS);
        if (tk > 0) {
            ensure_dbg(c);
            ensure_top_scratch(c);
            c->d_trace_top.reserve(rows * 32);
            c->d_trace_det.reserve(rows * 16);
            fill_other_shards_det(c);
        }
    }
    c->top_ready = false;
    for (int k = 0; T0 && k < n1 * n1; ++k)
        if (!std::isfinite(T0[k])) throw Fail{GICP_E_INVALID, "T0 contains non-finite values"};
    upload_state(c, T0, &prm);
    IterState& hs = *c->h_state;
    const int grid = corr_grid(c->src.ntiles, c->shard, c->nshards);
    const bool timing = res != nullptr && prm.timing_stride >= 0;   // < 0: no timing events
    const auto t0 = std::chrono::steady_clock::now();
    double corr_ms = 0.0;
    int enq = 0, samples = 0;
    // Timing events are recorded around every kEvStride-th k_corr only: an event pair around
    // every launch inserts a few microseconds of queue work per iteration.
    const int kEvStride = prm.timing_stride > 0 ? std::min(prm.timing_stride, (int)gicp_ctx::kMaxBatch) : 8;
    const int kEvOffset = std::max(0, prm.timing_offset) % kEvStride;
    c->iter_ms.assign((size_t)std::max(0, prm.max_iterations), -1.f);
#ifdef GICP_TAIL
    // diagnostic build: one tail record per iteration (gicp_internal.h kTailWords), dumped raw to
    // $GICP_TAIL_DUMP.<call> after the loop
    static std::atomic<int> tail_seq{0};   // dump file counter (process-wide)
    const char* tail_path = std::getenv("GICP_TAIL_DUMP");
    const size_t ntail = (size_t)std::max(1, prm.max_iterations) * kTailWords;
    unsigned long long* d_tail = nullptr;
    if (tail_path) {   // the context's own buffer, on its device
        c->d_tail.reserve(ntail);
        d_tail = c->d_tail;
        std::vector<unsigned long long> init(ntail, 0ull);
        for (size_t k = 0; k < ntail; k += kTailWords) init[k] = ~0ull;
        HIPCHK(hipMemcpyAsync(d_tail, init.data(), ntail * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
    }
#endif
    // Iterations are enqueued in batches with no host sync inside a batch: each is k_corr (pose
    // from the device state, statistics reduced in-launch) [+ RCCL all-reduce] + k_solve.
    // After convergence the remaining launches of a batch exit at once.
    // A host exchange synchronises every iteration anyway: batches of one, so the loop stops at the
    // converged iteration without launching more.  Otherwise the first batch is as long as the last
    // converging align on this context ran (a sequence of similar registrations -- odometry frames --
    // then pays one host sync per call instead of two or three; a shorter registration pays a few
    // launches that exit at once), later batches 8.
    const int first_batch = std::max(8, std::min((int)gicp_ctx::kMaxBatch, c->batch_hint));
    while (enq < prm.max_iterations) {
        const int B = std::min(prm.max_iterations - enq,
                               c->hook ? 1 : prm.fixed_iterations ? (int)gicp_ctx::kMaxBatch
                                                                  : enq == 0 ? first_batch : 8);
        for (int b = 0; b < B; ++b) {
            const int it = enq + b;
            CorrArgs a = corr_args(c, 0);
            if (it < c->moving_iters) a.unit_map = c->moving_map;
#ifdef GICP_TAIL
            if (tail_path) a.tail = d_tail + (size_t)it * kTailWords;
#endif
            if (tk > 0) {   // det(W) of every point, for this iteration's top-k rows (gicp.py:170)
                a.dbg_det = c->d_dbg_det;
                a.top_tgt = c->d_top_tgt;
            }
            // k_corr's final workgroup runs the solve too whenever it holds the sums the solve needs: with
            // no exchange (one rank, or bench.py --shard-sim's lone shard: the peer-exchange launch shape
            // without the exchange) and with the in-kernel peer exchange; RCCL and the host hook sit
            // between k_corr and k_solve
            const bool peer = a.peer.n > 1;
            const bool fuse = c->fuse_solve && (peer || (grid > 0 && !c->hook && !c->comm));
            double* const hist = trace ? c->d_hist + (size_t)it * HS : nullptr;
            if (fuse) {
                a.fuse_solve = 1;
                a.hist = hist;
            }
            const bool ev = timing && it % kEvStride == kEvOffset;
            if (ev) HIPCHK(hipEventRecord(c->ev[2 * b], st));
            launch_pass(c, a, d, grid);
            if (ev) HIPCHK(hipEventRecord(c->ev[2 * b + 1], st));
            if (tk > 0)   // launched after convergence too (the pass exited at once): rows >= iter are ignored
                HIPCHK(launch_top_weights(c->d_dbg_det, c->d_top_tgt, c->src.perm, c->src.n, tk, c->d_top_v,
                                          c->d_top_i, kTopBlocks, c->d_trace_det + (size_t)it * 16,
                                          c->d_trace_top + (size_t)it * 32, c->d_trace_top + (size_t)it * 32 + 16,
                                          st));
            if (!fuse) {
                allreduce_stats(c);
                HIPCHK(launch_solve(c->d_state, d, st, hist));
            }
        }
        enq += B;
        HIPCHK(hipMemcpyAsync(&hs, c->d_state, sizeof(IterState), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (timing)
            for (int b = 0; b < B; ++b) {
                if ((enq - B + b) % kEvStride != kEvOffset) continue;
                if (enq - B + b >= hs.iter) break;   // launched after convergence: exited at once
                float ms = 0.f;
                HIPCHK(hipEventElapsedTime(&ms, c->ev[2 * b], c->ev[2 * b + 1]));
                c->iter_ms[enq - B + b] = ms;
                corr_ms += ms;
                ++samples;
            }
        if (hs.converged) break;
    }
    const auto t1 = std::chrono::steady_clock::now();
    if (!prm.fixed_iterations && hs.converged) c->batch_hint = hs.iter;
    c->iter_ms.resize((size_t)std::max(0, std::min(hs.iter, prm.max_iterations)));
#ifdef GICP_TAIL
    if (tail_path) {
        std::vector<unsigned long long> h(ntail);
        HIPCHK(hipMemcpyAsync(h.data(), d_tail, ntail * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const std::string path = std::string(tail_path) + "." + std::to_string(tail_seq++);
        if (FILE* fp = std::fopen(path.c_str(), "wb")) {
            std::fwrite(h.data(), 8, h.size(), fp);
            std::fclose(fp);
        }
    }
#endif
    if (trace && hs.iter > 0) {   // the rows of the iterations executed, in one copy per array
        const int ni = std::min(hs.iter, prm.max_iterations);
        std::vector<double> hist((size_t)ni * HS);
        HIPCHK(hipMemcpyAsync(hist.data(), c->d_hist, sizeof(double) * hist.size(), hipMemcpyDeviceToHost, st));
        std::vector<int64_t> ttop;
        std::vector<double> tdet;
        if (tk > 0) {
            ttop.resize((size_t)ni * 32);
            tdet.resize((size_t)ni * 16);
            HIPCHK(hipMemcpyAsync(ttop.data(), c->d_trace_top, sizeof(int64_t) * ttop.size(), hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(tdet.data(), c->d_trace_det, sizeof(double) * tdet.size(), hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
        for (int k = 0; k < ni; ++k) {
            if (trace->poses) std::memcpy(trace->poses + (size_t)k * n1 * n1, &hist[(size_t)k * HS], sizeof(double) * n1 * n1);
            if (trace->losses) trace->losses[k] = hist[(size_t)k * HS + n1 * n1];
            for (int r = 0; r < tk; ++r) {
                if (trace->top_src) trace->top_src[(size_t)k * tk + r] = ttop[(size_t)k * 32 + r];
                if (trace->top_tgt) trace->top_tgt[(size_t)k * tk + r] = ttop[(size_t)k * 32 + 16 + r];
                if (trace->top_det) trace->top_det[(size_t)k * tk + r] = tdet[(size_t)k * 16 + r];
            }
        }
    }
    check_peer_timeout(hs.solve_fail);
    // A robust kernel can give every correspondence w = 0 (GICP_ROBUST_TUKEY with every residual beyond c):
    // the pass's quadratic is identically zero, the solve finds its translation block sum w W not positive
    // definite and leaves the pose where it was.  Every pose minimises that quadratic: not an error.
    const auto zero_weight = [&] {
        const int NS = d * (d + 1) / 2;
        const double* Cw = hs.stats_solved + NS * NS + NS * d;   // sum w W
        return std::all_of(Cw, Cw + NS, [](double x) { return x == 0.0; });
    };
    if (hs.solve_fail && !(prm.robust_kernel != GICP_ROBUST_NONE && zero_weight()))
        throw Fail{GICP_E_INVALID, "pose solve failed (degenerate statistics)"};
    std::memcpy(T_out, hs.T, sizeof(double) * n1 * n1);
    if (res) {
        gicp_result r;
        std::memset(&r, 0, sizeof(r));
        const int ns = nstat(d);
        r.iterations = hs.iter;
        r.converged = hs.converged;
        r.converged_at = hs.converged ? hs.converged_at : -1;
        r.final_loss = hs.loss;
        r.correspondences = (int64_t)hs.stats_solved[ns - 1];
        r.ambiguous = (int32_t)hs.stats_solved[ns];
        r.pairs_evaluated = (int64_t)hs.stats_solved[ns + 1];
        record_pass_info(c, hs.stats_solved + ns);
        r.wall_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        // kernel time of the iterations actually executed (after convergence launches exit at once)
        r.corr_kernel_ms = samples ? corr_ms / samples * hs.iter : 0.0;
        r.reduce_ms = 0.0;
        r.stop_reason = hs.converged ? hs.stop_reason : GICP_STOP_NONE;
        r.pairs_total = hs.pairs_total;
        r.corr_kernel_ms_sampled = corr_ms;
        r.corr_samples = samples;
        r.mse = hs.mse;
        if (hs.xchg_n > 0.0) {   // wall-clock ticks -> us
            const double us = 1e3 / wall_clock_khz(c);
            r.exchange_us_mean = hs.xchg_sum / hs.xchg_n * us;
            r.exchange_us_min = hs.xchg_min * us;
        }
        *res = r;
    }
}

}  // namespace gicp
