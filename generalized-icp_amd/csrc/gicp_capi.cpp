// gicp_capi.cpp — the C-ABI of libgicp_hip.so (include/gicp_hip.h): argument checks, the exception boundary and
// a call into the unit that does the work (gicp_build.cpp, gicp_align.cpp, gicp_exchange.cpp, gicp_hostmath.cpp).
//
// A context owns one GPU: device copies of both clouds (Morton-sorted tile index, per-point surface
// covariances), the per-iteration workspace, an optional statistics exchange, and the outer loop of
// gicp.py:116-167.
#include <functional>
#include <new>

#include "gicp_host.h"

using namespace gicp;

// the four functions gicp_mem.h's buffers reach the runtime through
namespace gicp {
void* dev_alloc(size_t bytes) {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, bytes));
    return p;
}
void dev_free(void* p) noexcept { quiet(hipFree(p)); }
void* pinned_alloc(size_t bytes) {
    void* p = nullptr;
    HIPCHK(hipHostMalloc(&p, bytes));
    return p;
}
void pinned_free(void* p) noexcept { quiet(hipHostFree(p)); }
}  // namespace gicp

namespace {

int guard_impl(gicp_ctx* c, const char* where, const std::function<void()>& body) {
    try {
        if (c) HIPCHK(hipSetDevice(c->device));
        body();
        return GICP_OK;
    } catch (...) {
        std::string msg;
        const int rc = current_failure(msg);
        if (c) c->err = std::string(where) + ": " + msg;
        return rc;
    }
}

// a host-only entry point's body: no context, no HIP call (and no message: running out of memory is, like
// everything else that is no Fail, GICP_E_INVALID here)
int host_guard(const std::function<void()>& body) {
    try {
        body();
        return GICP_OK;
    } catch (...) {
        std::string msg;
        const int rc = current_failure(msg);
        return rc == GICP_E_NOMEM ? GICP_E_INVALID : rc;
    }
}

Cloud& need_cloud(gicp_ctx* c, int which, bool cov = false) {
    Cloud& cl = which == 0 ? c->tgt : c->src;
    if (!cl.n || (cov && !cl.cov_ready)) throw Fail{GICP_E_STATE, "cloud not set"};
    return cl;
}

VoxelMap& need_map(gicp_ctx* c) {
    if (!c->map.set) throw Fail{GICP_E_STATE, "no map: call gicp_map_reset first"};
    return c->map;
}

// what gicp_deskew and gicp_deskew_host refuse alike, and the twist of the motion M
void check_sweep_args(const double* xyz, const double* stamps, int64_t N, int dim, const double* M, double ref,
                      const double* out, double* xi) {
    check_cloud_args(xyz, N, dim);
    if (!stamps) throw Fail{GICP_E_INVALID, "a sweep needs stamps (stamps is NULL)"};
    if (!out) throw Fail{GICP_E_INVALID, "out must not be NULL"};
    double mn[3], mx[3];
    scan_bounds(xyz, N, dim, mn, mx);   // (the finiteness test)
    scan_stamps(stamps, N, ref);
    motion_twist(dim, M, xi);
}

}  // namespace

extern "C" {

int gicp_version(void) { return 108; }

int gicp_stats_size(int dim) { return (dim == 2 || dim == 3) ? nstat(dim == 2 ? 2 : 3) : GICP_E_INVALID; }

void gicp_default_params(int dim, gicp_params* out) {
    if (out) default_params(dim == 2 ? 2 : 3, out);
}

const char* gicp_strerror(int code) {
    switch (code) {
        case GICP_OK: return "ok";
        case GICP_E_INVALID: return "invalid argument";
        case GICP_E_HIP: return "HIP runtime error";
        case GICP_E_STATE: return "call out of order";
        case GICP_E_COMM: return "RCCL error";
        case GICP_E_NOMEM: return "out of memory";
        default: return "unknown error";
    }
}

int gicp_create(gicp_ctx** out, int device) {
    if (!out) return GICP_E_INVALID;
    *out = nullptr;
    gicp_ctx* c = new (std::nothrow) gicp_ctx();
    if (!c) return GICP_E_NOMEM;
    c->device = device;
    if (const char* e = std::getenv("GICP_NO_LISTS")) c->use_lists = !(e[0] == '1');
    if (const char* e = std::getenv("GICP_SKIN")) c->skin_frac = std::max(0.0, std::atof(e));
    if (const char* e = std::getenv("GICP_SKIN_GAIN")) c->skin_gain = std::max(0.0, std::atof(e));
    if (const char* e = std::getenv("GICP_NO_CERTS")) c->use_certs = !(e[0] == '1');
    if (const char* e = std::getenv("GICP_NO_GRAPH")) c->use_graph = !(e[0] == '1');
    if (const char* e = std::getenv("GICP_FUSE_SOLVE")) c->fuse_solve = !(e[0] == '0');
    if (const char* e = std::getenv("GICP_UNIT_MAP")) c->unit_map = std::max(0, std::atoi(e));
    if (const char* e = std::getenv("GICP_MOVING_MAP")) c->moving_map = std::max(0, std::atoi(e));
    if (const char* e = std::getenv("GICP_MOVING_ITERS")) c->moving_iters = std::max(0, std::atoi(e));
    if (const char* e = std::getenv("GICP_SRC_TILE")) {
        const int v = std::atoi(e);
        c->src_tile = v == 16 || v == 32 ? v : kTile;
    }
    if (const char* e = std::getenv("GICP_CERT_KAPPA")) c->kappa_frac = std::max(0.0, std::atof(e));
    if (const char* e = std::getenv("GICP_SPARSE_WALK")) c->sparse_max = std::max(0, std::min(64, std::atoi(e)));
    if (const char* e = std::getenv("GICP_SPARSE_AMB")) c->sparse_amb = std::max(0, std::min(64, std::atoi(e)));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        delete c;
        return GICP_E_HIP;
    }
    if (device < 0 || device >= ndev) {
        delete c;
        return GICP_E_INVALID;
    }
    const int rc = guard_impl(c, "gicp_create", [&] {
        HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        for (auto& e : c->ev) HIPCHK(hipEventCreate(&e));
    });
    if (rc != GICP_OK) {
        gicp_destroy(c);
        return rc;
    }
    *out = c;
    return GICP_OK;
}

void gicp_destroy(gicp_ctx* c) {
    if (!c) return;
    for (auto& g : c->stg) g.stop();             // staged builds still running finish first
    quiet(hipSetDevice(c->device));
    if (c->stream) quiet(hipStreamSynchronize(c->stream));
    drop_comm(c);
    for (auto& p : c->peer_open)
        if (p) quiet(hipIpcCloseMemHandle(p));
    if (c->d_peer_area) dev_free(c->d_peer_area);   // (the one buffer that is no DevBuf: see gicp_ctx)
    // a staged build that failed may have left work enqueued on its stream (it synchronises only on success)
    for (auto& g : c->stg)
        if (g.stream) {
            quiet(hipStreamSynchronize(g.stream));
            quiet(hipStreamDestroy(g.stream));
        }
    for (auto& e : c->ev)
        if (e) quiet(hipEventDestroy(e));
    if (c->stream) quiet(hipStreamDestroy(c->stream));
    delete c;   // every stream is idle and gone: the buffers release themselves
}

const char* gicp_last_error(const gicp_ctx* c) { return c ? c->err.c_str() : "null context"; }

int gicp_comm_unique_id(char out[GICP_COMM_ID_BYTES]) {
    if (!out) return GICP_E_INVALID;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return GICP_E_COMM;
    static_assert(sizeof(id) == GICP_COMM_ID_BYTES, "ncclUniqueId size");
    std::memcpy(out, &id, sizeof(id));
    return GICP_OK;
}

int gicp_comm_init(gicp_ctx* c, int nranks, int rank, const char id[GICP_COMM_ID_BYTES]) {
    if (!c || !id || nranks < 1 || rank < 0 || rank >= nranks) return GICP_E_INVALID;
    return guard_impl(c, "gicp_comm_init", [&] { comm_init(c, nranks, rank, id); });
}

int gicp_comm_ranks(gicp_ctx* c, int* nranks, int* rank, int* kind) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_comm_ranks", [&] { comm_ranks(c, nranks, rank, kind); });
}

int gicp_set_target(gicp_ctx* c, const double* xyz, int64_t M, int dim, const gicp_params* p) {
    return gicp_set_target_sweep(c, xyz, M, dim, p, nullptr);
}

int gicp_set_target_sweep(gicp_ctx* c, const double* xyz, int64_t M, int dim, const gicp_params* p, const gicp_sweep* sw) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_set_target", [&] {
        c->ptgt = resolve(dim, p);
        c->top_ready = false;
        BuildSpec spec = target_spec(c, c->stream);
        take_sweep(spec, sw, dim);
        build_cloud(c->tgt, xyz, M, dim, c->ptgt, c->bs, spec);
        if (c->src.n) reset_tile_state(c);
    });
}

int gicp_set_source(gicp_ctx* c, const double* xyz, int64_t N, int dim, const gicp_params* p, int shard,
                    int nshards) {
    return gicp_set_source_sweep(c, xyz, N, dim, p, shard, nshards, nullptr);
}

int gicp_set_source_sweep(gicp_ctx* c, const double* xyz, int64_t N, int dim, const gicp_params* p, int shard,
                          int nshards, const gicp_sweep* sw) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_set_source", [&] {
        check_shard(shard, nshards);
        c->psrc = resolve(dim, p);
        c->top_ready = false;
        BuildSpec spec = source_spec(c, shard, nshards);
        take_sweep(spec, sw, dim);
        build_cloud(c->src, xyz, N, dim, c->psrc, c->bs, spec);
        set_shard(c, shard, nshards);
        HIPCHK(hipStreamSynchronize(c->stream));
    });
}

int gicp_target_to_source(gicp_ctx* c, int shard, int nshards) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_target_to_source", [&] {
        if (!c->tgt.n) throw Fail{GICP_E_STATE, "no target to promote"};
        std::swap(c->src, c->tgt);   // the old source's buffers are kept for the next target
        c->top_ready = false;
        c->tgt.unset();
        c->psrc = c->ptgt;
        set_shard(c, shard, nshards);   // (its resets are stream-ordered before the next registration: no host sync)
    });
}

int gicp_get_covariances(gicp_ctx* c, int which, double* out) {
    if (!c || !out || (which != 0 && which != 1)) return GICP_E_INVALID;
    return guard_impl(c, "gicp_get_covariances", [&] {
        const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};   // (R = I: R m = m exactly)
        const double I2[4] = {1, 0, 0, 1};
        Cloud& cl = need_cloud(c, which, true);
        copy_covariances(c, cl, cl.dim == 3 ? I : I2, out);
    });
}

int gicp_get_graph(gicp_ctx* c, int64_t* index, double* radius) {
    if (!c) return GICP_E_INVALID;
    static_assert(GICP_GRAPH_K == kGraphK, "graph width");
    return guard_impl(c, "gicp_get_graph", [&] {
        Cloud& cl = c->tgt;
        if (!cl.n || !cl.graph_ready) throw Fail{GICP_E_STATE, "no target graph (set_target first; GICP_NO_GRAPH unset)"};
        const int64_t n = cl.n;
        std::vector<uint4> nbq((size_t)n * 8);
        std::vector<int32_t> nbi((size_t)n * kGraphK), perm(n);
        HIPCHK(hipMemcpyAsync(nbq.data(), cl.nbq, sizeof(uint4) * n * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(nbi.data(), cl.nbi, sizeof(int32_t) * n * kGraphK, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(perm.data(), cl.perm, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int64_t i = 0; i < n; ++i) {
            const int64_t o = perm[i];
            if (radius) {
                float r;
                std::memcpy(&r, &nbq[(size_t)i * 8].x, sizeof(float));
                radius[o] = r;
            }
            if (index)
                for (int k = 0; k < kGraphK; ++k) {
                    const int t = nbi[(size_t)i * kGraphK + k];
                    index[o * kGraphK + k] = t >= 0 ? (int64_t)perm[t] : -1;
                }
        }
    });
}

int gicp_get_neighbor_counts(gicp_ctx* c, int which, int32_t* out) {
    if (!c || !out || (which != 0 && which != 1)) return GICP_E_INVALID;
    return guard_impl(c, "gicp_get_neighbor_counts", [&] {
        Cloud& cl = need_cloud(c, which);
        std::vector<int32_t> cnt(cl.n), perm(cl.n);
        HIPCHK(hipMemcpyAsync(cnt.data(), cl.ncount, sizeof(int32_t) * cl.n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(perm.data(), cl.perm, sizeof(int32_t) * cl.n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int64_t i = 0; i < cl.n; ++i) out[perm[i]] = cnt[i];
    });
}

int gicp_iterate(gicp_ctx* c, const double* T, double* stats, gicp_debug* dbg) {
    if (!c || !T || !stats) return GICP_E_INVALID;
    return guard_impl(c, "gicp_iterate", [&] {
        run_pass(c, T, dbg);
        std::memcpy(stats, c->h_stats, sizeof(double) * nstat(c->src.dim));
    });
}

int gicp_pass_info(gicp_ctx* c, double out[GICP_PASS_INFO]) {
    if (!c || !out) return GICP_E_INVALID;
    out[0] = c->last_amb;
    out[1] = c->last_pairs;
    out[2] = c->last_rebuilds;
    out[3] = c->last_sq;
    out[4] = c->last_gproved;
    out[5] = c->last_walked;
    return GICP_OK;
}

int gicp_top_weights(gicp_ctx* c, int k, int64_t* src_out, int64_t* tgt_out, double* det_out) {
    if (!c || k < 1 || k > 16) return GICP_E_INVALID;
    return guard_impl(c, "gicp_top_weights", [&] {
        if (!c->top_ready) throw Fail{GICP_E_STATE, "no pass with want_top_weights since the last cloud change"};
        if (c->top_cached_k != k) {   // not computed with the pass: now (and for this k from the next pass on)
            top_enqueue(c, k);
            HIPCHK(hipStreamSynchronize(c->stream));
            c->top_cached_k = c->top_k_pref = k;
        }
        const double* hv = reinterpret_cast<const double*>(c->h_top + 32);
        for (int r = 0; r < k; ++r) {
            if (src_out) src_out[r] = c->h_top[r];
            if (tgt_out) tgt_out[r] = c->h_top[16 + r];
            if (det_out) det_out[r] = hv[r];
        }
    });
}

int gicp_solve_pose(int dim, const double* stats, const double* T_k, double* T_out, double* loss_out) {
    if ((dim != 2 && dim != 3) || !stats || !T_k || !T_out) return GICP_E_INVALID;
    try {
        return solve_pose(dim, stats, T_k, T_out, loss_out) == 0 ? GICP_OK : GICP_E_INVALID;
    } catch (...) {
        return GICP_E_INVALID;
    }
}

// ---- the registration report ----

int gicp_evaluate(gicp_ctx* c, const double* T, const gicp_params* p, const gicp_report_spec* spec, gicp_report* out) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_evaluate", [&] { evaluate(c, T, p, spec, out); });
}

int gicp_information(int dim, const double* stats, const double* T, double* H, double* b) {
    return host_guard([&] { information(dim, stats, T, H, b); });
}

int gicp_sym_eig(int n, const double* A, double* w, double* V) {
    return host_guard([&] { sym_eig(n, A, w, V); });
}

int gicp_align(gicp_ctx* c, const double* T0, const gicp_params* p, double* T_out, gicp_result* res) {
    return gicp_align_trace(c, T0, p, T_out, res, nullptr);
}

int gicp_align_trace(gicp_ctx* c, const double* T0, const gicp_params* p, double* T_out, gicp_result* res,
                     gicp_trace* trace) {
    if (!c || !T_out) return GICP_E_INVALID;
    return guard_impl(c, "gicp_align", [&] { align_trace(c, T0, p, T_out, res, trace); });
}

int gicp_stage_target(gicp_ctx* c, const double* xyz, int64_t M, int dim, const gicp_params* p) {
    return gicp_stage_target_ex(c, xyz, M, dim, p, 0);
}

int gicp_stage_target_ex(gicp_ctx* c, const double* xyz, int64_t M, int dim, const gicp_params* p, int flags) {
    return gicp_stage_target_sweep(c, xyz, M, dim, p, flags, nullptr);
}

int gicp_stage_target_sweep(gicp_ctx* c, const double* xyz, int64_t M, int dim, const gicp_params* p, int flags,
                            const gicp_sweep* sw) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_stage_target", [&] {
        if (c->stg_count >= GICP_MAX_STAGED)
            throw Fail{GICP_E_STATE, "GICP_MAX_STAGED staged targets are pending (gicp_commit_target or gicp_cancel_stage first)"};
        // (the size limit is the build's to refuse, when the slot is committed)
        if (!xyz || M <= 0 || (dim != 2 && dim != 3)) throw Fail{GICP_E_INVALID, "cloud must be a non-empty N x 2 or N x 3 array"};
        if (flags & ~GICP_STAGE_BORROW) throw Fail{GICP_E_INVALID, "unknown gicp_stage_target_ex flags"};
        if (sw) {   // a sweep no build would take is refused here, with no slot used
            if (!sw->stamps) throw Fail{GICP_E_INVALID, "a sweep needs stamps (gicp_sweep.stamps is NULL)"};
            double xi[6];
            motion_twist(dim, sw->motion, xi);
        }
        stage_target(c, xyz, M, dim, p, flags, sw);
    });
}

int gicp_commit_target(gicp_ctx* c, int shard, int nshards) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_commit_target", [&] {
        if (!c->stg_count) throw Fail{GICP_E_STATE, "no staged target (gicp_stage_target first)"};
        commit_target(c, shard, nshards);
    });
}

int gicp_cancel_stage(gicp_ctx* c) {
    if (!c) return GICP_E_INVALID;
    cancel_stage(c);
    return GICP_OK;
}

int gicp_reset_cache(gicp_ctx* c) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_reset_cache", [&] {
        reset_tile_state(c);
        HIPCHK(hipStreamSynchronize(c->stream));
    });
}

int gicp_iteration_times(gicp_ctx* c, float* out, int n) {
    if (!c || (!out && n > 0) || n < 0) return GICP_E_INVALID;
    const int m = std::min(n, (int)c->iter_ms.size());
    for (int i = 0; i < m; ++i) out[i] = c->iter_ms[i];
    return m;
}

int gicp_set_allreduce(gicp_ctx* c, gicp_allreduce_fn fn, void* user) {
    return gicp_set_allreduce_ranks(c, fn, user, 1, 0);
}

int gicp_set_allreduce_ranks(gicp_ctx* c, gicp_allreduce_fn fn, void* user, int nranks, int rank) {
    if (!c || nranks < 1 || rank < 0 || rank >= nranks) return GICP_E_INVALID;
    return guard_impl(c, "gicp_set_allreduce", [&] { set_allreduce(c, fn, user, nranks, rank); });
}

int gicp_peer_export(gicp_ctx* c, char handle[GICP_PEER_HANDLE_BYTES]) {
    if (!c || !handle) return GICP_E_INVALID;
    return guard_impl(c, "gicp_peer_export", [&] { peer_export(c, handle); });
}

int gicp_peer_init(gicp_ctx* c, int nranks, int rank, const char* handles, double timeout_s) {
    if (!c || !handles || nranks < 2 || nranks > GICP_MAX_PEERS || rank < 0 || rank >= nranks || !(timeout_s > 0.0))
        return GICP_E_INVALID;
    return guard_impl(c, "gicp_peer_init", [&] { peer_init(c, nranks, rank, handles, timeout_s); });
}

int gicp_peer_close(gicp_ctx* c) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_peer_close", [&] { close_peers(c); });
}

const char* gicp_build_info(void) {
#ifndef GICP_SRC_HASH
#define GICP_SRC_HASH "unknown"
#endif
#ifndef GICP_GIT_REV
#define GICP_GIT_REV "unknown"
#endif
    return "src=" GICP_SRC_HASH ";git=" GICP_GIT_REV ";built=" __DATE__ " " __TIME__ ";arch=gfx950";
}

int gicp_rotated_covariances(gicp_ctx* c, int which, const double* R, double* out) {
    if (!c || !R || !out || (which != 0 && which != 1)) return GICP_E_INVALID;
    return guard_impl(c, "gicp_rotated_covariances", [&] {
        Cloud& cl = need_cloud(c, which, true);
        for (int k = 0; k < cl.dim * cl.dim; ++k)
            if (!std::isfinite(R[k])) throw Fail{GICP_E_INVALID, "R contains non-finite values"};
        copy_covariances(c, cl, R, out);
    });
}

int gicp_set_voxel(gicp_ctx* c, double leaf, int min_points) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_set_voxel", [&] {
        if (!std::isfinite(leaf) || leaf < 0.0) throw Fail{GICP_E_INVALID, "leaf must be finite and >= 0 (0 turns the filter off)"};
        if (min_points < 1) throw Fail{GICP_E_INVALID, "min_points must be >= 1"};
        c->voxel_leaf = leaf;
        c->voxel_min = min_points;
    });
}

int gicp_voxel_downsample(gicp_ctx* c, const double* xyz, int64_t N, int dim, double leaf, int min_points,
                          double* out_xyz, int32_t* out_count, int64_t* M_out) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_voxel_downsample", [&] {
        check_cloud_args(xyz, N, dim);
        if (!out_xyz || !M_out) throw Fail{GICP_E_INVALID, "out_xyz and M_out must not be NULL"};
        if (!std::isfinite(leaf) || leaf <= 0.0) throw Fail{GICP_E_INVALID, "leaf must be finite and > 0"};
        if (min_points < 1) throw Fail{GICP_E_INVALID, "min_points must be >= 1"};
        *M_out = 0;
        voxel_downsample(c, xyz, N, dim, leaf, min_points, out_xyz, out_count, M_out);
    });
}

// ---- input filters; gicp_filter_points_host lives in gicp_hostmath.cpp ----

int gicp_set_filter(gicp_ctx* c, const gicp_filter* f) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_set_filter", [&] {
        gicp_filter v{};
        if (f) {
            check_filter(*f);
            v = *f;
            v.pad = 0;
        }
        c->filt = v;
    });
}

int gicp_filter_points(gicp_ctx* c, const double* xyz, int64_t N, int dim, const gicp_filter* f, double* out_xyz,
                       int64_t* out_index, int32_t* out_count, int64_t* M_out) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_filter_points", [&] {
        check_filter_args(xyz, N, dim, f, out_xyz, M_out);
        *M_out = 0;
        filter_points(c, xyz, N, dim, *f, out_xyz, out_index, out_count, M_out);
    });
}

// ---- exact k-nearest-neighbour queries; gicp_knn_host lives in gicp_hostmath.cpp ----

int gicp_knn_max_k(void) { return kKnnMaxK; }

int gicp_knn(gicp_ctx* c, int which, const double* queries, int64_t Q, int dim, int k, double max_distance, int64_t* index,
             double* dist2, int32_t* count) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_knn", [&] {
        if (which != 0 && which != 1) throw Fail{GICP_E_INVALID, "which must be 0 (target) or 1 (source)"};
        check_knn_args(queries, Q, dim, k, max_distance);
        const Cloud& cl = need_cloud(c, which);
        if (queries && dim != cl.dim) throw Fail{GICP_E_INVALID, "queries must have the cloud's dim"};
        knn_query(c, &cl, nullptr, 0, queries, Q, cl.dim, k, max_distance, index, dist2, count);
    });
}

int gicp_knn_points(gicp_ctx* c, const double* xyz, int64_t M, const double* queries, int64_t Q, int dim, int k,
                    double max_distance, int64_t* index, double* dist2, int32_t* count) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_knn_points", [&] {
        check_cloud_args(xyz, M, dim);
        check_knn_args(queries, Q, dim, k, max_distance);
        knn_query(c, nullptr, xyz, M, queries, Q, dim, k, max_distance, index, dist2, count);
    });
}

// ---- statistical outlier removal; gicp_sor_points_host lives in gicp_hostmath.cpp ----

int gicp_sor_max_k(void) { return kSorMaxK; }

int gicp_set_sor(gicp_ctx* c, const gicp_sor* s) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_set_sor", [&] {
        gicp_sor v{};
        if (s && s->k != 0) {
            check_sor(*s);
            v = *s;
            v.pad = 0;
        }
        c->sor = v;
    });
}

int gicp_sor_points(gicp_ctx* c, const double* xyz, int64_t N, int dim, const gicp_sor* s, double* out_xyz, int64_t* out_index,
                    double* out_mean, double* out_stats, int64_t* M_out) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_sor_points", [&] {
        double mn[3], mx[3];
        check_sor_args(xyz, N, dim, s, M_out, mn, mx);   // (the one scan of the cloud: finiteness and bounds)
        sor_points(c, xyz, N, dim, mn, mx, *s, out_xyz, out_index, out_mean, out_stats, M_out);
    });
}

// ---- Euclidean cluster extraction; gicp_cluster_points_host lives in gicp_hostmath.cpp ----

int gicp_set_cluster(gicp_ctx* c, const gicp_cluster* cl) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_set_cluster", [&] {
        gicp_cluster v{};
        if (cl && cl->radius != 0.0) {
            check_cluster(*cl);
            v = *cl;
        }
        c->cluster = v;
    });
}

int gicp_cluster_points(gicp_ctx* c, const double* xyz, int64_t N, int dim, const gicp_cluster* cl, int32_t* labels, int32_t* sizes,
                        int64_t* n_clusters, double* out_xyz, int64_t* out_index, int64_t* M_out) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_cluster_points", [&] {
        double mn[3], mx[3];
        check_cluster_args(xyz, N, dim, cl, mn, mx);   // (the one scan of the cloud: finiteness and bounds)
        cluster_points(c, xyz, N, dim, mn, mx, *cl, labels, sizes, n_clusters, out_xyz, out_index, M_out);
    });
}

int gicp_cloud_size(gicp_ctx* c, int which, int64_t* n) {
    if (!c || !n || (which != 0 && which != 1)) return GICP_E_INVALID;
    *n = (which == 0 ? c->tgt : c->src).n;
    return GICP_OK;
}

int gicp_get_points(gicp_ctx* c, int which, double* out) {
    if (!c || !out || (which != 0 && which != 1)) return GICP_E_INVALID;
    return guard_impl(c, "gicp_get_points", [&] { copy_points(c, need_cloud(c, which), out); });
}

// ---- motion compensation ----

int gicp_motion_twist(int dim, const double* M, double* xi) {
    return host_guard([&] { motion_twist(dim, M, xi); });
}

int gicp_deskew_host(const double* xyz, const double* stamps, int64_t N, int dim, const double* M, double ref,
                     double* out) {
    return host_guard([&] {
        double xi[6];
        check_sweep_args(xyz, stamps, N, dim, M, ref, out, xi);
        deskew_host(xyz, stamps, N, dim, xi, ref, out);
    });
}

int gicp_deskew(gicp_ctx* c, const double* xyz, const double* stamps, int64_t N, int dim, const double* M, double ref,
                double* out) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_deskew", [&] {
        double xi[6];
        check_sweep_args(xyz, stamps, N, dim, M, ref, out, xi);
        deskew_cloud(c, xyz, stamps, N, dim, xi, ref, out);
    });
}

// ---- the local voxel map ----

int gicp_map_reset(gicp_ctx* c, int dim, double leaf, double max_range) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_map_reset", [&] {
        if (dim != 2 && dim != 3) throw Fail{GICP_E_INVALID, "dim must be 2 or 3"};
        if (!std::isfinite(leaf) || leaf <= 0.0) throw Fail{GICP_E_INVALID, "leaf must be finite and > 0"};
        if (!std::isfinite(max_range) || max_range <= 0.0) throw Fail{GICP_E_INVALID, "max_range must be finite and > 0"};
        int bits = 0;
        const int64_t R = map_window_cells(dim, leaf, max_range, bits);
        VoxelMap& mp = c->map;   // (buffers are kept: grow-only)
        mp.set = true;
        mp.dim = dim;
        mp.leaf = leaf;
        mp.R = R;
        mp.bits = bits;
        mp.rows = 0;
    });
}

int gicp_map_insert(gicp_ctx* c, int which, const double* T) {
    if (!c || !T || (which != 0 && which != 1)) return GICP_E_INVALID;
    return guard_impl(c, "gicp_map_insert", [&] {
        VoxelMap& mp = need_map(c);
        Cloud& cl = need_cloud(c, which);
        if (cl.dim != mp.dim) throw Fail{GICP_E_INVALID, "the cloud's dimension differs from the map's"};
        map_insert(c, &cl, nullptr, cl.n, T);
    });
}

int gicp_map_insert_points(gicp_ctx* c, const double* xyz, int64_t n, int dim, const double* T) {
    if (!c || !T) return GICP_E_INVALID;
    return guard_impl(c, "gicp_map_insert_points", [&] {
        VoxelMap& mp = need_map(c);
        check_cloud_args(xyz, n, dim);
        if (dim != mp.dim) throw Fail{GICP_E_INVALID, "the cloud's dimension differs from the map's"};
        double mn[3], mx[3];
        scan_bounds(xyz, n, dim, mn, mx);   // (the finiteness test)
        map_insert(c, nullptr, xyz, n, T);
    });
}

int gicp_map_size(gicp_ctx* c, int64_t* rows) {
    if (!c || !rows) return GICP_E_INVALID;
    *rows = c->map.set ? c->map.rows : 0;
    return GICP_OK;
}

int gicp_map_get(gicp_ctx* c, int32_t* cells, double* centroids, int32_t* counts) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_map_get", [&] {
        VoxelMap& mp = need_map(c);
        const int64_t m = mp.rows;
        if (m == 0) return;
        const int d = mp.dim;
        std::vector<double> sums;
        std::vector<int32_t> cl;
        if (centroids || counts) {
            sums.resize((size_t)m * 4);
            HIPCHK(hipMemcpyAsync(sums.data(), mp.sums[mp.cur], sizeof(double) * m * 4, hipMemcpyDeviceToHost, c->stream));
        }
        if (cells) {
            cl.resize((size_t)m * 3);
            HIPCHK(hipMemcpyAsync(cl.data(), mp.cells[mp.cur], sizeof(int32_t) * m * 3, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int64_t i = 0; i < m; ++i)
            for (int a = 0; a < d; ++a) {
                if (cells) cells[i * d + a] = cl[i * 3 + a];
                if (centroids) centroids[i * d + a] = sums[i * 4 + a] / sums[i * 4 + 3];   // (correctly rounded, as the device's)
            }
        if (counts)
            for (int64_t i = 0; i < m; ++i) counts[i] = (int32_t)sums[i * 4 + 3];
    });
}

int gicp_map_to_target(gicp_ctx* c, const gicp_params* p, int min_points) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_map_to_target", [&] {
        VoxelMap& mp = need_map(c);
        if (min_points < 1) throw Fail{GICP_E_INVALID, "min_points must be >= 1"};
        if (mp.rows <= 0) throw Fail{GICP_E_INVALID, "the map is empty"};
        map_to_target(c, p, min_points);
    });
}

}  // extern "C"
