// gicp_capi.cpp — the C-ABI of libgicp_hip.so (include/gicp_hip.h).
//
// Owns one GPU per context: device copies of both clouds (Morton-sorted tile index,
// per-point surface covariances), the per-iteration workspace, an optional RCCL
// communicator for the statistics all-reduce, and the outer loop of gicp.py:116-167.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/gicp_hip.h"
#include "gicp_internal.h"
#include "gicp_mem.h"
#include "gicp_sweep.h"

namespace gicp {
hipError_t launch_morton(const double*, int64_t, int, const DevCloud&, uint32_t*, int32_t*, hipStream_t);
hipError_t launch_build_tiles(const double*, int, int32_t*, TileInfo*, TileBox*, int, double*, float4*, int32_t*,
                              unsigned*, hipStream_t);
hipError_t launch_build_blocks(const TileInfo*, int, BlockInfo*, int, int, hipStream_t);
hipError_t launch_knn_cov(const CovArgs&, int, int, bool, hipStream_t);
hipError_t launch_corr(const CorrArgs&, int, int, hipStream_t);
hipError_t launch_solve(IterState*, int, hipStream_t, double*);
hipError_t launch_peer_probe(const PeerArgs&, double*, hipStream_t);
hipError_t launch_reset_tiles(int32_t*, int32_t*, float*, int32_t*, int, int32_t*, int64_t, hipStream_t);
hipError_t launch_graph_pack(const GraphArgs&, hipStream_t);
hipError_t launch_rotate_cov(const double4*, const int32_t*, int64_t, int, const double*, double*, hipStream_t);
hipError_t launch_top_weights(const double*, const int64_t*, const int32_t*, int64_t, int, double*, int64_t*, int, double*, int64_t*,
                              int64_t*, hipStream_t);
hipError_t voxel_temp_bytes(int64_t, int, size_t*, hipStream_t);
hipError_t launch_voxel(const VoxelArgs&, hipStream_t);
hipError_t launch_points_out(const double*, const int32_t*, int64_t, int, double*, hipStream_t);
hipError_t launch_deskew(const SweepArgs&, hipStream_t);
hipError_t launch_map_insert(const VoxelArgs&, const MapArgs&, hipStream_t);
hipError_t launch_map_centroids(const double*, int64_t, int, int, int32_t*, int32_t*, void*, size_t, double*,
                                unsigned long long*, hipStream_t);
int corr_grid(int q_tiles, int shard, int nshards);
int solve_pose(int d, const double* st, const double* Tk, double* Tout, double* loss_out);
}  // namespace gicp

using namespace gicp;

namespace {

// a failing HIP call is reported to the caller (the exception) and its error cleared from HIP's
// per-thread last error here, so it cannot fail a later call's first launch check
#define HIPCHK(x)                                                                                  \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            (void)hipGetLastError();                                                               \
            throw Fail{GICP_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)};               \
        }                                                                                          \
    } while (0)

// a HIP call whose failure is deliberately ignored (teardown): its error must not linger either
inline void quiet(hipError_t e) {
    if (e != hipSuccess) (void)hipGetLastError();
}

}  // namespace

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

// A few persistent host threads for the tiling (spawning threads per cloud costs tens of us each,
// which a 100k-point frame of a stream cannot afford).  run(n, fn) calls fn(0 .. n-1) on the workers
// and the calling thread and returns when all are done; one caller at a time.
class WorkerPool {
public:
    explicit WorkerPool(int workers) {
        for (int i = 0; i < workers; ++i) th_.emplace_back([this] { loop(); });
    }
    ~WorkerPool() {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    void run(int tasks, std::function<void(int)> fn) {
        std::unique_lock<std::mutex> lk(m_);
        job_ = std::move(fn);
        ntasks_ = tasks;
        next_ = done_ = 0;
        ++gen_;
        lk.unlock();
        cv_.notify_all();
        work();
        lk.lock();
        done_cv_.wait(lk, [&] { return done_ == ntasks_ && active_ == 0; });
    }

private:
    void work() {
        for (;;) {
            int k;
            {
                std::lock_guard<std::mutex> g(m_);
                if (next_ >= ntasks_) return;
                k = next_++;
            }
            job_(k);
            std::lock_guard<std::mutex> g(m_);
            if (++done_ == ntasks_) done_cv_.notify_all();
        }
    }
    void loop() {
        std::unique_lock<std::mutex> lk(m_);
        long seen = 0;
        for (;;) {
            cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
            if (stop_) return;
            seen = gen_;
            ++active_;
            lk.unlock();
            work();
            lk.lock();
            if (--active_ == 0) done_cv_.notify_all();
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_cv_;
    std::function<void(int)> job_;
    int ntasks_ = 0, next_ = 0, done_ = 0, active_ = 0;
    long gen_ = 0;
    bool stop_ = false;
};

// One indexed cloud on the device.
struct Cloud {
    int dim = 0;
    int64_t n = 0;
    int ntiles = 0, nblocks = 0, level = 0, bits = 0;   // level: tile extent-cap step k (cap 2^(1 + k/4) cells)
    double lo[3] = {0, 0, 0};
    double scale = 1.0;
    float rho = 0.f;
    // the buffers are grow-only and move with the cloud: a swap of two clouds swaps them, and the side that
    // is then cleared (n = 0) keeps its buffers as spares for the next build
    DevBuf<double> xyz64;
    DevBuf<float4> rel32;
    DevBuf<double4> cov;
    DevBuf<int32_t> perm, inv, ncount;
    DevBuf<TileInfo> tiles;
    DevBuf<BlockInfo> blocks;
    DevBuf<uint32_t> tile_code;
    DevBuf<TileBox> boxes;            // the walk's compact tile records (k_build_tiles)
    DevBuf<int32_t> seed_tab;         // Morton seed lookup (DevCloud::seed_tab), built on the host
    int seed_shift = 0;
    DevBuf<uint4> nbq;                // neighbour graph (targets only): packed rows (line A)
    DevBuf<uint4> nbx;                // ... their last entries
    DevBuf<int32_t> nbi;              // ... and their sorted indices
    bool graph_ready = false;
    bool cov_ready = false;
    int cov_shard = 0, cov_nshards = 1;  // whose tiles' covariances were computed (build_cloud)

    void reserve_points(int64_t np) {
        xyz64.reserve((size_t)np * 4);
        rel32.reserve((size_t)np);
        cov.reserve((size_t)np);
        perm.reserve((size_t)np);
        inv.reserve((size_t)np);
        ncount.reserve((size_t)np);
    }
    void reserve_tiles(int nt, int nb) {
        tiles.reserve((size_t)nt);
        blocks.reserve((size_t)nb + (nb + kBlockTiles - 1) / kBlockTiles);   // + super-blocks
        tile_code.reserve((size_t)nt);
        boxes.reserve((size_t)nt);
    }
    DevCloud view() const {
        DevCloud v{};
        v.xyz64 = xyz64;
        v.rel32 = rel32;
        v.cov = cov;
        v.perm = perm;
        v.tiles = tiles;
        v.blocks = blocks;
        v.tile_code = tile_code;
        v.boxes = boxes;
        v.seed_tab = seed_tab;
        v.seed_shift = seed_shift;
        v.nbq = graph_ready ? nbq.get() : nullptr;
        v.nbx = graph_ready ? nbx.get() : nullptr;
        v.nbi = graph_ready ? nbi.get() : nullptr;
        v.n = n;
        v.ntiles = ntiles;
        v.nblocks = nblocks;
        for (int a = 0; a < 3; ++a) v.lo[a] = lo[a];
        v.scale = scale;
        v.bits = bits;
        v.dim = dim;
        return v;
    }
};

// Scratch of one cloud build (grow-only): the synchronous builds and the staged one (which runs on
// its own stream and host thread while the current target is registered) each own one.
struct BuildScratch {
    DevBuf<double> s_in;
    DevBuf<uint32_t> s_codes, s_codes2;
    DevBuf<int32_t> s_idx;
    DevBuf<unsigned char> s_sort;
    DevBuf<float4> g_nb;              // graph build scratch
    DevBuf<float2> g_nbh;
    DevBuf<int32_t> d_amb;            // covariance-kernel diagnostics counter
    int tile_k_hint[4] = {0, 0, 0, 0};  // last tile extent-cap step per dimension (tiling warm start)
    PinnedBuf<double> h_pinned;       // pinned host copy of the input (staged builds)
    // voxel filter (gicp_voxel.hip): the raw cloud, keys and indices before and after the sort, head flags,
    // voxel ids, per-wave carries, per-voxel centroids and counts, the kept counts, rocPRIM scratch, results
    DevBuf<double> v_raw;
    DevBuf<uint64_t> v_keys, v_keys2;
    DevBuf<int32_t> v_idx, v_idx2, v_flag, v_vid, v_cnt, v_ocnt;
    DevBuf<double> v_cfirst, v_clast, v_cent;
    DevBuf<int2> v_cmeta;
    DevBuf<unsigned char> v_tmp;
    DevBuf<unsigned long long> v_res;
    DevBuf<double> w_stamps;          // the stamps of a sweep (gicp_sweep.hip)
    std::unique_ptr<WorkerPool> pool;  // tiling threads (lazily started)
    WorkerPool& workers() {
        if (!pool) {
            const unsigned hc = std::max(1u, std::thread::hardware_concurrency());
            pool.reset(new WorkerPool((int)std::min(7u, hc > 1 ? hc - 1 : 0u)));
        }
        return *pool;
    }
};

// The local voxel map (gicp_map_*): rows (cell, sums, count) in key order, double-buffered --
// an insert reads buffer `cur` and writes the other -- and grow-only like the build scratch.
struct VoxelMap {
    bool set = false;                 // gicp_map_reset was called
    int dim = 0;
    double leaf = 0.0;
    int64_t R = 0;                    // half-width of the window in cells
    int bits = 0;                     // key bits per axis: ceil(log2(2 R + 1))
    int64_t rows = 0;
    int cur = 0;
    DevBuf<int32_t> cells[2];         // [rows][3]
    DevBuf<double> sums[2];           // [rows][4]
    DevBuf<double> pts;               // [n][dim] the scan being inserted, original order
    DevBuf<double> vals;              // [rows + n][4] staged values of an insert
};

// How a cloud is built (build_cloud / build_core); the defaults are a plain synchronous build.
struct BuildSpec {
    bool graph = false;               // also the neighbour graph (targets: k_corr's graph descent)
    bool staged = false;              // runs beside a registration: one k_knn_cov wave per tile
    // the covariances are computed for that shard's tiles only (a sharded source: every rank needs the whole
    // cloud's index for the neighbourhoods, but only its own tiles' covariances); the other rows read NaN
    int cov_shard = 0, cov_nshards = 1;
    int tile_points = kTile;          // points per tile at most (64; a source may take 32 or 16: GICP_SRC_TILE)
    // leaf > 0: the uploaded cloud is first reduced to one centroid per voxel holding >= voxel_min points (the
    // voxel filter, on the device), and the index is built over those centroids in key order
    double voxel_leaf = 0.0;
    int voxel_min = 1;
    // sweep: the uploaded cloud is first de-skewed on the device, point i moved by
    // Exp((stamps[i] - ref) Log(motion)); the filter and the index then see the de-skewed points and their bounds.
    // The twist is taken from `motion` ((dim+1)^2 row-major) once the build has begun, so a motion it refuses
    // leaves the cloud NOT SET
    bool sweep = false;
    const double* stamps = nullptr;   // [n] host, read during the build
    double motion[16] = {};
    double ref = 0.0;
    hipStream_t stream = nullptr;
};

// GICP_VERBOSE=1: the time of each phase of a build, printed with the cloud's figures when it is done.
// tick() synchronises the stream, so it does nothing unless verbose.
struct BuildLog {
    hipStream_t st;
    bool verbose = std::getenv("GICP_VERBOSE") && std::getenv("GICP_VERBOSE")[0] == '1';
    std::chrono::steady_clock::time_point prev = std::chrono::steady_clock::now();
    std::string text;
    explicit BuildLog(hipStream_t s) : st(s) {}
    void tick(const char* what) {
        if (!verbose) return;
        HIPCHK(hipStreamSynchronize(st));
        const auto t = std::chrono::steady_clock::now();
        char b[64];
        std::snprintf(b, sizeof b, " %s %.1f", what, std::chrono::duration<double, std::milli>(t - prev).count());
        text += b;
        prev = t;
    }
};

}  // namespace

struct gicp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    Cloud tgt, src;
    gicp_params ptgt{}, psrc{};
    int shard = 0, nshards = 1, q_begin = 0, q_end = 0;
    // Every device and pinned buffer below owns itself (gicp_mem.h): delete c releases them.  The reserved ones
    // are grow-only (a frame stream allocates once); the fixed ones are allocated on first use.
    DevBuf<int32_t> d_hint;
    DevBuf<double> d_partials;
    DevBuf<IterState> d_state;
    PinnedBuf<IterState> h_state;     // pinned mirror
    DevBuf<uint32_t> d_tickets;
    DevBuf<double> d_gpart;
    double h_stats[80];
    DevBuf<int64_t> d_dbg_idx;
    DevBuf<double> d_dbg_w, d_dbg_dist;
    DevBuf<double> d_dbg_det;         // det(W) per source point (gicp_top_weights)
    bool top_ready = false;           // the last pass recorded det(W)
    // the top-k of that pass, computed inside the pass (same stream sync) for k = top_k_pref, the k the
    // last gicp_top_weights call asked for: [0, 16) source, [16, 32) target indices, then 16 det values
    int top_k_pref = 5, top_cached_k = 0;
    PinnedBuf<int64_t> h_top;         // 32 int64 + 16 double
    DevBuf<double> d_top_v;           // top-k scratch: stage-1 candidates and outputs
    DevBuf<int64_t> d_top_i;
    DevBuf<int64_t> d_top_tgt;        // [N] sorted order: target of each correspondence (with det(W))
    DevBuf<int64_t> d_top_out;
    // per-source-tile candidate lists
    DevBuf<int32_t> d_list, d_list_len, d_list_pass;
    DevBuf<float> d_list_rcert;
    DevBuf<double> d_poses;
    // per-source-point nearest-neighbour certificates
    DevBuf<int32_t> d_cert_j;
    DevBuf<float> d_cert_gap;
    DevBuf<int32_t> d_cert_pass;
    bool use_certs = true;            // GICP_NO_CERTS=1: every pass walks every lane
    bool use_graph = true;            // GICP_NO_GRAPH=1: no target neighbour graph, no graph descent
    bool fuse_solve = true;           // GICP_FUSE_SOLVE=0: the solve as its own k_solve launch even with no exchange
    int unit_map = 0;                 // k_corr workgroup -> unit map (CorrArgs::unit_map, GICP_UNIT_MAP)
    int moving_map = 8;               // ... for the first moving_iters iterations of an align (GICP_MOVING_MAP)
    int moving_iters = 5;             // (GICP_MOVING_ITERS)
    int src_tile = kTile;             // source points per tile at most: 64, 32 or 16 (GICP_SRC_TILE)
    double kappa_frac = 0.002;        // certificate gap resolved by the walk, fraction of d_c (GICP_CERT_KAPPA)
    int sparse_max = 4;               // CorrArgs::sparse_max (GICP_SPARSE_WALK; 0: sparse waves walk like the rest)
    int sparse_amb = 2;               // CorrArgs::sparse_amb (GICP_SPARSE_AMB; 0: every fp64 re-resolution wave-wide)
    // cloud-build scratch (synchronous builds) and per-source-tile arrays, grow-only (a frame stream
    // allocates once)
    BuildScratch bs;
    // voxel filter of every later cloud build (gicp_set_voxel): leaf 0 = off
    double voxel_leaf = 0.0;
    int voxel_min = 1;
    VoxelMap map;                     // local voxel map (gicp_map_reset)
    // staged targets (gicp_stage_target / gicp_commit_target): a ring of GICP_MAX_STAGED slots, each
    // built into its own cloud on its own stream by a host thread while the current target is
    // registered; commits take them in staging order
    // Each slot owns a persistent build thread (started on first use): a thread per staged frame cost
    // tens of microseconds of the caller's time per frame.  state: 0 idle, 1 build queued or running,
    // 2 built (rc / err hold the outcome); the caller waits for state != 1 before it takes the slot.
    struct Staged {
        Cloud cl;
        BuildScratch bs;
        hipStream_t stream = nullptr;
        std::thread th;
        std::mutex m;
        std::condition_variable cv;
        int state = 0;
        bool quit = false;
        const double* xyz = nullptr;   // the slot's pinned copy, or the caller's buffer (GICP_STAGE_BORROW)
        int64_t M = 0;
        int dim = 0;
        int device = 0;
        BuildSpec spec;                // graph, the context's filter setting when the build was staged, this stream
        gicp_params p{};
        int rc = GICP_OK;
        std::string err;
        void wait_idle() {
            std::unique_lock<std::mutex> lk(m);
            cv.wait(lk, [&] { return state != 1; });
        }
        void stop() {
            if (!th.joinable()) return;
            {
                std::lock_guard<std::mutex> g(m);
                quit = true;
            }
            cv.notify_all();
            th.join();
        }
    };
    Staged stg[GICP_MAX_STAGED];
    int stg_head = 0, stg_count = 0;
    int pass = 0;
    bool use_lists = true;
    double skin_frac = 0.2;           // candidate-list skin as a fraction of d_c (GICP_SKIN)
    double skin_gain = 1.0;           // adaptive skin: multiple of the tile's last displacement (GICP_SKIN_GAIN)
    double last_rebuilds = 0.0;
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
    gicp_allreduce_fn hook = nullptr;  // host statistics exchange (gicp_set_allreduce)
    void* hook_user = nullptr;
    PinnedBuf<double> h_xchg;         // exchange buffer of the hook
    // in-kernel peer exchange (gicp_peer_export / gicp_peer_init)
    // This rank's exchange area: uncached device memory (hipExtMallocWithFlags) that other processes map through
    // IPC, so it is no DevBuf.  A raw pointer, set only once the area is zeroed, with one free in gicp_destroy.
    double* d_peer_area = nullptr;
    void* peer_open[kMaxPeers] = {};  // the peers' areas as opened here (closed by gicp_peer_close)
    PeerArgs peer{};                  // n > 1 while the peer exchange is on
    DevBuf<uint64_t> d_peer_ctr;      // the device's exchange counter (PeerArgs::ctr)
    double peer_timeout_s = 10.0;
    DevBuf<double> d_probe;
    DevBuf<double*> d_peer_ptrs;      // device copy of the areas' addresses (PeerArgs::area)
    std::vector<float> iter_ms;       // sampled k_corr time per iteration of the last align (-1: not sampled)
    DevBuf<double> d_rot;             // gicp_rotated_covariances output
    // gicp_align_trace: per-iteration rows recorded on the device ([iter][(d+1)^2 + 1] pose + loss;
    // top-k rows [iter][16] source, target, det), copied out once after the loop
    DevBuf<double> d_hist;
    DevBuf<int64_t> d_trace_top;      // [iter][16] source, then [iter][16] target
    DevBuf<double> d_trace_det;       // [iter][16]
    DevBuf<unsigned long long> d_tail;     // GICP_TAIL diagnostic build: [iter][kTailWords] (on this context's device)
    DevBuf<unsigned long long> d_stamps;   // GICP_STAMPS / GICP_TIMELINE diagnostic builds: [wave][20]
    static constexpr int kMaxBatch = 64;
    hipEvent_t ev[2 * kMaxBatch] = {};
    int batch_hint = 0;               // iterations the last converging align ran: its first batch next time
    // diagnostics of the last pass
    double last_amb = 0.0, last_pairs = 0.0, last_sq = 0.0, last_gproved = 0.0, last_walked = 0.0;
    float last_corr_ms = 0.f, last_reduce_ms = 0.f;
    bool timing = false;
};

namespace {

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

// Cut the Morton-sorted points into tiles: runs of <= 64 consecutive points whose bounding box (in
// Morton grid cells) stays within an extent cap E.  E is the smallest cap (steps of 2^(1/4)) whose
// tile count stays <= 1.35x the minimum ceil(n/64): tiles are as compact as that budget allows, and
// the cap bounds the largest tile, which sets both the widest query wave and the loosest box.
void build_tile_table(const std::vector<uint32_t>& codes, int dim, int bits, std::vector<int32_t>& start,
                      std::vector<int32_t>& count, std::vector<uint32_t>& first_code, int& cap_out, int k_hint,
                      WorkerPool& pool, int maxp = kTile) {
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
    auto cap_of = [](int k) { return (int)(2.0 * std::pow(2.0, k / 4.0)); };
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

// Build the device index of a cloud and the per-point covariances of all its tiles (a source shard
// is a set of interleaved chunks, and the whole-cloud pass costs ~1 ms at 1M points).
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

// doubles from the ordered-integer form gicp_voxel.hip reduces min / max in
double dec_ordered(unsigned long long e) {
    const unsigned long long b = (e >> 63) ? (e & 0x7FFFFFFFFFFFFFFFull) : ~e;
    double v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}

struct VoxelOut {
    int64_t M = 0;                  // voxels kept
    double mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};   // bounds of their centroids
};

// The filter's scratch for va.n rows sorted on va.end_bit key bits, reserved (grow-only) and entered into va;
// centroids: also the per-voxel centroids and counts (the map's inserts store sums instead).
void voxel_scratch(BuildScratch& bs, VoxelArgs& va, bool centroids, hipStream_t st) {
    const int64_t n = va.n;
    const size_t nw = (size_t)((n + kWave - 1) / kWave);
    bs.v_keys.reserve((size_t)n);
    bs.v_keys2.reserve((size_t)n);
    bs.v_idx.reserve((size_t)n);
    bs.v_idx2.reserve((size_t)n);
    bs.v_flag.reserve((size_t)n);
    bs.v_vid.reserve((size_t)n);
    if (centroids) {
        bs.v_cnt.reserve((size_t)n);
        bs.v_ocnt.reserve((size_t)n);
        bs.v_cent.reserve((size_t)n * 3);
    }
    bs.v_cfirst.reserve(nw * 4);
    bs.v_clast.reserve(nw * 4);
    bs.v_cmeta.reserve(nw);
    if (!bs.v_res) bs.v_res.alloc((size_t)kVoxelRes);
    size_t tmp_bytes = 0;
    HIPCHK(voxel_temp_bytes(n, va.end_bit, &tmp_bytes, st));
    bs.v_tmp.reserve(tmp_bytes + 16);
    va.keys = bs.v_keys;
    va.keys_s = bs.v_keys2;
    va.idx = bs.v_idx;
    va.idx_s = bs.v_idx2;
    va.flag = bs.v_flag;
    va.vid1 = bs.v_vid;
    va.cfirst = bs.v_cfirst;
    va.clast = bs.v_clast;
    va.cmeta = bs.v_cmeta;
    va.cent = centroids ? bs.v_cent : nullptr;
    va.cnt = centroids ? bs.v_cnt : nullptr;
    va.tmp = bs.v_tmp;
    va.tmp_bytes = tmp_bytes;
    va.out_cnt = centroids ? bs.v_ocnt : nullptr;
    va.res = bs.v_res;
}

// The voxel filter (gicp_voxel.hip) of the device cloud d_raw [n][dim] with host bounds mn / mx:
// centroids of the voxels holding >= min_points points into d_out [M][dim] in key order, their counts into
// bs.v_ocnt.  One stream sync; the result words (centroid bounds, M) are all that returns to the host.
VoxelOut voxel_filter(BuildScratch& bs, const double* d_raw, int64_t n, int dim, const double (&mn)[3],
                      const double (&mx)[3], double leaf, int min_points, double* d_out, hipStream_t st) {
    VoxelArgs va{};
    va.raw = d_raw;
    va.n = n;
    va.dim = dim;
    va.min_points = min_points;
    va.leaf = leaf;
    // the lowest cell per axis and the key bits: division by a positive leaf is monotone, so every point's
    // cell lies in [floor(min / leaf), floor(max / leaf)], computed here as the device computes it
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
        va.cmin[a] = c0;
        uint64_t r = (uint64_t)range - 1;
        int bits = 0;
        while (r) ++bits, r >>= 1;
        va.bits[a] = bits;
        total += bits;
    }
    va.end_bit = std::max(1, total);
    voxel_scratch(bs, va, true, st);
    va.out_xyz = d_out;
    HIPCHK(launch_voxel(va, st));
    unsigned long long res[kVoxelRes];
    HIPCHK(hipMemcpyAsync(res, bs.v_res, sizeof res, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    VoxelOut vo;
    vo.M = (int64_t)res[6];
    if (vo.M <= 0) {
        char b[128];
        std::snprintf(b, sizeof b, "voxel filter: none of the %lld voxels holds min_points = %d points", (long long)res[7],
                      min_points);
        throw Fail{GICP_E_INVALID, b};
    }
    for (int a = 0; a < dim; ++a) {
        vo.mn[a] = dec_ordered(res[a]);
        vo.mx[a] = dec_ordered(res[3 + a]);
    }
    return vo;
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

// the finiteness test of a sweep's stamps and reference stamp (v - v is NaN for NaN and +-inf)
void scan_stamps(const double* stamps, int64_t n, double ref) {
    if (!std::isfinite(ref)) throw Fail{GICP_E_INVALID, "sweep reference stamp is not finite"};
    double acc = 0.0;
    for (int64_t i = 0; i < n; ++i) acc += stamps[i] - stamps[i];
    if (!(acc == 0.0)) throw Fail{GICP_E_INVALID, "sweep contains non-finite stamps"};
}

template <int D>
void deskew_host(const double* xyz, const double* stamps, int64_t n, const double* xi, double ref, double* out) {
    for (int64_t i = 0; i < n; ++i) sweep_point<D>(xi, stamps[i] - ref, xyz + i * D, out + i * D);
}

// De-skew the device cloud d_pts [n][dim] in place on `st` (gicp_sweep.hip): the host stamps are uploaded into
// bs.w_stamps, the ordered-integer bounds of the result land in bs.v_res[0..5] (deskew_decode decodes them).
void deskew_launch(BuildScratch& bs, double* d_pts, const double* stamps, int64_t n, int dim, const double* xi, double ref,
                   hipStream_t st) {
    bs.w_stamps.reserve((size_t)n);
    if (!bs.v_res) bs.v_res.alloc((size_t)kVoxelRes);
    HIPCHK(hipMemcpyAsync(bs.w_stamps, stamps, sizeof(double) * n, hipMemcpyHostToDevice, st));
    SweepArgs sa{};
    sa.pts = d_pts;
    sa.stamps = bs.w_stamps;
    sa.n = n;
    sa.dim = dim;
    for (int k = 0; k < (dim == 3 ? 6 : 3); ++k) sa.xi[k] = xi[k];
    sa.ref = ref;
    sa.res = bs.v_res;
    HIPCHK(launch_deskew(sa, st));
}

// the exact bounds of the de-skewed points, decoded from the result words (synchronised by the caller)
void deskew_decode(const unsigned long long* res, int dim, double (&mn)[3], double (&mx)[3]) {
    for (int a = 0; a < 3; ++a) mn[a] = mx[a] = 0.0;
    for (int a = 0; a < dim; ++a) {
        mn[a] = dec_ordered(res[a]);
        mx[a] = dec_ordered(res[3 + a]);
        // (finite stamps times a finite twist can still overflow; a NaN coordinate decodes as a NaN bound)
        if (!std::isfinite(mn[a]) || !std::isfinite(mx[a]))
            throw Fail{GICP_E_INVALID, "de-skewed cloud is not finite (stamps too large for the motion)"};
    }
}

void build_core(Cloud& cl, int64_t n, int dim, const double (&mn)[3], const double (&mx)[3], const gicp_params& p,
                BuildScratch& bs, const BuildSpec& spec, BuildLog& log);

// The host front of a cloud build: the bounds and finiteness scan, the upload and (spec.voxel_leaf > 0) the
// voxel filter; build_core does the rest from the device buffer bs.s_in and the bounds.
void build_cloud(Cloud& cl, const double* xyz, int64_t n, int dim, const gicp_params& p, BuildScratch& bs,
                 const BuildSpec& spec) {
    if (!xyz || n <= 0 || (dim != 2 && dim != 3)) throw Fail{GICP_E_INVALID, "cloud must be a non-empty N x 2 or N x 3 array"};
    if (n > (int64_t)0x7FFFFFFF - 64) throw Fail{GICP_E_INVALID, "cloud too large (> 2^31 points)"};
    if (spec.sweep && !spec.stamps) throw Fail{GICP_E_INVALID, "a sweep needs stamps (gicp_sweep.stamps is NULL)"};
    hipStream_t st = spec.stream;
    BuildLog log(st);
    cl.n = 0;   // buffers are kept (grow-only) and reused
    cl.cov_ready = false;
    cl.graph_ready = false;
    cl.dim = dim;
    cl.bits = dim == 3 ? 10 : 16;
    double mn[3], mx[3];
    scan_bounds(xyz, n, dim, mn, mx);
    double xi[6];
    if (spec.sweep) {
        scan_stamps(spec.stamps, n, spec.ref);
        motion_twist(dim, spec.motion, xi);
    }
    log.tick("host-scan");
    bs.s_in.reserve((size_t)n * dim);
    // A sweep is de-skewed in place where it was uploaded; the filter and the index then take the device's
    // exact bounds of the de-skewed points (one stream sync) in place of the host scan's.
    auto deskew = [&](double* d_pts) {
        deskew_launch(bs, d_pts, spec.stamps, n, dim, xi, spec.ref, st);
        unsigned long long res[kVoxelRes];
        HIPCHK(hipMemcpyAsync(res, bs.v_res, sizeof res, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        deskew_decode(res, dim, mn, mx);
        log.tick("deskew");
    };
    // (a staged build passes its pinned copy: the H2D copy is then asynchronous)
    if (spec.voxel_leaf > 0.0) {
        bs.v_raw.reserve((size_t)n * dim);
        HIPCHK(hipMemcpyAsync(bs.v_raw, xyz, sizeof(double) * n * dim, hipMemcpyHostToDevice, st));
        if (spec.sweep) deskew(bs.v_raw);
        const VoxelOut vo = voxel_filter(bs, bs.v_raw, n, dim, mn, mx, spec.voxel_leaf, spec.voxel_min, bs.s_in, st);
        n = vo.M;
        for (int a = 0; a < 3; ++a) mn[a] = vo.mn[a], mx[a] = vo.mx[a];
        log.tick("voxel");
    } else {
        HIPCHK(hipMemcpyAsync(bs.s_in, xyz, sizeof(double) * n * dim, hipMemcpyHostToDevice, st));
        if (spec.sweep) deskew(bs.s_in);
    }
    build_core(cl, n, dim, mn, mx, p, bs, spec, log);
}

// The core of a cloud build: the n points in bs.s_in ([n][dim], device) with bounds mn / mx -> Morton sort,
// tiles, blocks, covariances and (graph) the neighbour graph.
void build_core(Cloud& cl, int64_t n, int dim, const double (&mn)[3], const double (&mx)[3], const gicp_params& p,
                BuildScratch& bs, const BuildSpec& spec, BuildLog& log) {
    hipStream_t st = spec.stream;
    const bool graph = spec.graph;
    const int tile_points = spec.tile_points;
    // a build that fails part-way (an unsupported k_neighbors, a HIP error) leaves the cloud NOT SET: cl.n is
    // raised below, before the covariances exist, and every entry point tells a usable cloud by cl.n alone
    struct Unset {
        Cloud& cl;
        bool done = false;
        ~Unset() {
            if (done) return;
            cl.n = 0;
            cl.cov_ready = false;
            cl.graph_ready = false;
        }
    } unset{cl};
    double ext = 0.0;
    for (int a = 0; a < dim; ++a) ext = std::max(ext, mx[a] - mn[a]);
    ext = ext * (1.0 + 1e-9) + 1e-12 * (1.0 + std::fabs(mn[0]));
    for (int a = 0; a < 3; ++a) cl.lo[a] = a < dim ? mn[a] : 0.0;
    cl.scale = std::ldexp(1.0, cl.bits) / ext;

    {
        cl.reserve_points(n);
        bs.s_codes.reserve((size_t)n);
        bs.s_codes2.reserve((size_t)n);
        bs.s_idx.reserve((size_t)n);
        if (!bs.d_amb)
            alloc_init(bs.d_amb, 4, [&](int32_t* d) { HIPCHK(hipMemsetAsync(d, 0, sizeof(int32_t) * 4, st)); });
        double* d_in = bs.s_in;
        uint32_t *d_codes = bs.s_codes, *d_codes_s = bs.s_codes2;
        int32_t *d_idx = bs.s_idx, *d_perm = cl.perm;   // (raw pointers: rocPRIM deduces its iterator types)
        DevCloud fr = cl.view();
        HIPCHK(launch_morton(d_in, n, dim, fr, d_codes, d_idx, st));
        size_t tmp_bytes = 0;
        const unsigned end_bit = (unsigned)(dim * cl.bits);
        HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, d_codes, d_codes_s, d_idx, d_perm, (size_t)n, 0, end_bit,
                                         st));
        bs.s_sort.reserve(tmp_bytes + 16);
        HIPCHK(rocprim::radix_sort_pairs(bs.s_sort.get(), tmp_bytes, d_codes, d_codes_s, d_idx, d_perm, (size_t)n, 0,
                                         end_bit, st));
        log.tick("upload+sort");
        std::vector<uint32_t> codes(n);
        HIPCHK(hipMemcpyAsync(codes.data(), d_codes_s, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        log.tick("codes-d2h");
        std::vector<int32_t> tstart, tcount;
        std::vector<uint32_t> tcode;
        // (the extent-cap hint is kept for full-size tiles, the stream's case)
        build_tile_table(codes, dim, cl.bits, tstart, tcount, tcode, cl.level,
                         tile_points == kTile ? bs.tile_k_hint[dim & 3] : 0, bs.workers(), tile_points);
        if (tile_points == kTile) bs.tile_k_hint[dim & 3] = cl.level;
        log.tick("tiling");
        cl.ntiles = (int)tstart.size();
        cl.nblocks = (cl.ntiles + kBlockTiles - 1) / kBlockTiles;
        std::vector<TileInfo> ti(cl.ntiles);
        std::memset(ti.data(), 0, sizeof(TileInfo) * ti.size());
        for (int t = 0; t < cl.ntiles; ++t) {
            ti[t].start = tstart[t];
            ti[t].count = tcount[t];
        }
        cl.reserve_tiles(cl.ntiles, cl.nblocks);
        cl.n = n;
        unsigned* d_rho = reinterpret_cast<unsigned*>(d_codes);  // reuse scratch
        HIPCHK(hipMemsetAsync(d_rho, 0, sizeof(unsigned), st));
        HIPCHK(hipMemcpyAsync(cl.tiles, ti.data(), sizeof(TileInfo) * cl.ntiles, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(cl.tile_code, tcode.data(), sizeof(uint32_t) * cl.ntiles, hipMemcpyHostToDevice, st));
        // Morton seed lookup (DevCloud::seed_tab): 2^sb buckets of the code's top bits, about 4 per tile
        std::vector<int32_t> seed;
        {
            const int code_bits = dim * cl.bits;
            int sb = 2;
            while ((1 << sb) < 4 * cl.ntiles && sb < 20) ++sb;
            sb = std::min(sb, code_bits);
            cl.seed_shift = code_bits - sb;
            const size_t nb = (size_t)1 << sb;
            seed.resize(nb + 1);
            int t = 0;   // last tile whose first code <= p << shift (0 if none)
            for (size_t p = 0; p < nb; ++p) {
                const uint64_t lim = (uint64_t)p << cl.seed_shift;
                while (t + 1 < cl.ntiles && (uint64_t)tcode[t + 1] <= lim) ++t;
                seed[p] = t;
            }
            seed[nb] = cl.ntiles - 1;
            cl.seed_tab.reserve(nb + 1);
            HIPCHK(hipMemcpyAsync(cl.seed_tab, seed.data(), sizeof(int32_t) * (nb + 1), hipMemcpyHostToDevice, st));
        }
        HIPCHK(launch_build_tiles(d_in, dim, cl.perm, cl.tiles, cl.boxes, cl.ntiles, cl.xyz64, cl.rel32, cl.inv, d_rho, st));
        HIPCHK(launch_build_blocks(cl.tiles, cl.ntiles, cl.blocks, cl.nblocks, dim, st));
        unsigned rho_bits = 0;
        HIPCHK(hipMemcpyAsync(&rho_bits, d_rho, sizeof(unsigned), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        std::memcpy(&cl.rho, &rho_bits, sizeof(float));
        log.tick("tiles");

        // surface covariances (gicp.py:19-35), of this rank's tiles when sharded
        const int qb = 0, qe = shard_tile_count(cl.ntiles, spec.cov_shard, spec.cov_nshards);
        CovArgs ca{};
        ca.cl = cl.view();
        ca.q_begin = qb;
        ca.q_end = qe;
        ca.sh_n = spec.cov_nshards;
        ca.sh_r = spec.cov_shard;
        if (spec.cov_nshards > 1) HIPCHK(hipMemsetAsync(cl.cov, 0xFF, sizeof(double4) * n, st));   // NaN: not computed
        const double dn = p.max_distance_nearest_neighbors;
        ca.mg = make_margin(dim, cl.rho, cl.rho, dn);
        ca.search2 = screen_bound(ca.mg, dn);
        ca.dn2 = dn * dn;
        ca.eps_a = p.epsilon;
        ca.m_scale = std::sqrt(p.epsilon * (1.0 - p.ratio));
        ca.min_nb = p.min_neighbors;
        ca.cov_out = cl.cov;
        ca.count_out = cl.ncount;
        ca.amb_counter = bs.d_amb;
        // waves per query tile: a synchronous build of a small cloud is split by sub-tile (the walk of its
        // longest wave bounds it); a staged build keeps one wave per tile -- it runs beside a registration,
        // whose k_corr the split's idle lanes would slow (C5, 500 frames: 1050 vs 960 frames/s) -- and so
        // does a cloud whose tiles alone fill the GPU (GICP_BUILD_SPLIT = 1 / 4 forces either)
        static const int split_env = [] {
            const char* e = std::getenv("GICP_BUILD_SPLIT");
            return e ? std::atoi(e) : 0;
        }();
        ca.split = split_env == 1 || split_env == kSub ? split_env : (!spec.staged && cl.ntiles <= 8192 ? kSub : 1);
        // the target neighbour graph (k_corr's graph descent) comes out of the covariances'
        // own two walks (k_knn_cov<D, K, true>), then one pass packs the rows
        GraphArgs ga{};
        if (graph) {
            cl.nbq.reserve((size_t)n * 8);
            cl.nbx.reserve((size_t)n * 3);
            cl.nbi.reserve((size_t)n * kGraphK);
            bs.g_nb.reserve((size_t)n * kGraphK);   // unpacked rows (scratch)
            bs.g_nbh.reserve((size_t)n);
            ga.cl = cl.view();
            ga.split = ca.split;
            ga.mg = ca.mg;
            ga.search2 = ca.search2;
            ga.nb = bs.g_nb;
            ga.nbh = bs.g_nbh;
            ga.nbq = cl.nbq;
            ga.nbx = cl.nbx;
            ga.nbi = cl.nbi;
            ca.g_nb = bs.g_nb;
            ca.g_nbh = bs.g_nbh;
        }
        HIPCHK(hipMemsetAsync(cl.ncount, 0, sizeof(int32_t) * n, st));
        hipError_t e = launch_knn_cov(ca, dim, p.k_neighbors, graph, st);
        if (e == hipErrorInvalidValue) throw Fail{GICP_E_INVALID, "unsupported k_neighbors for this dim (2-D: 6, 10; 3-D: 10, 20)"};
        HIPCHK(e);
        if (graph) HIPCHK(launch_graph_pack(ga, st));
        HIPCHK(hipStreamSynchronize(st));
        cl.cov_ready = true;
        cl.cov_shard = spec.cov_shard;
        cl.cov_nshards = spec.cov_nshards;
        cl.graph_ready = graph;
        log.tick(graph ? "covariances+graph" : "covariances");
        if (log.verbose)
            std::fprintf(stderr, "[gicp] cloud n=%lld tiles=%d (%.2fx min) extent cap=%d cells rho=%.4f | ms:%s\n",
                         (long long)n, cl.ntiles, cl.ntiles / std::ceil(n / 64.0), cl.level, cl.rho, log.text.c_str());
    }
    unset.done = true;
}

// One insert into the local voxel map: the n points in mp.pts ([n][dim], device, original row
// order, sensor frame) are moved by T (sensor -> world, (dim+1)^2 row-major), the window is re-centred on T's
// translation, and rows and points are merged into the map's other buffer.  One stream sync; only the result
// words return to the host.
void map_insert_core(VoxelMap& mp, BuildScratch& bs, int64_t n, const double* T, hipStream_t st) {
    const int d = mp.dim;
    for (int k = 0; k < (d + 1) * (d + 1); ++k)
        if (!std::isfinite(T[k])) throw Fail{GICP_E_INVALID, "T contains non-finite values"};
    if (mp.rows + n > (int64_t)0x7FFFFFFF - 64) throw Fail{GICP_E_INVALID, "map and scan together hold more than 2^31 rows"};
    MapArgs ma{};
    for (int a = 0; a < d; ++a) {
        for (int b = 0; b < d; ++b) ma.R[a * 3 + b] = T[a * (d + 1) + b];
        ma.t[a] = T[a * (d + 1) + d];
        const double c = std::floor(ma.t[a] / mp.leaf);   // the centre cell
        if (!(std::fabs(c) + (double)mp.R < 2147483648.0)) {
            char b[160];
            std::snprintf(b, sizeof b, "map window leaves the int32 cell range: axis %d is centred on cell %.6g with a half-width of %lld cells",
                          a, c, (long long)mp.R);
            throw Fail{GICP_E_INVALID, b};
        }
        ma.lo[a] = (int64_t)c - mp.R;
    }
    const int64_t N = mp.rows + n;
    const int nb = mp.cur ^ 1;
    mp.cells[nb].reserve((size_t)N * 3);
    mp.sums[nb].reserve((size_t)N * 4);
    mp.vals.reserve((size_t)N * 4);
    VoxelArgs va{};
    va.n = N;
    va.dim = d;
    va.min_points = 1;
    va.leaf = mp.leaf;
    va.end_bit = std::max(1, d * mp.bits);
    voxel_scratch(bs, va, false, st);
    ma.cells_old = mp.cells[mp.cur];
    ma.sums_old = mp.sums[mp.cur];
    ma.m_old = mp.rows;
    ma.pts = mp.pts;
    ma.n = n;
    ma.dim = d;
    ma.leaf = mp.leaf;
    ma.span = 2 * mp.R;
    ma.bits = mp.bits;
    ma.vals = mp.vals;
    ma.cells_new = mp.cells[nb];
    ma.sums_new = mp.sums[nb];
    HIPCHK(launch_map_insert(va, ma, st));
    unsigned long long res[kVoxelRes];
    HIPCHK(hipMemcpyAsync(res, bs.v_res, sizeof res, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    mp.rows = (int64_t)res[6];
    mp.cur = nb;
}

// a target built on `st` under the context's settings: with the graph unless switched off, through the voxel filter
BuildSpec target_spec(const gicp_ctx* c, hipStream_t st) {
    BuildSpec spec;
    spec.graph = c->use_graph && c->use_certs;
    spec.voxel_leaf = c->voxel_leaf;
    spec.voxel_min = c->voxel_min;
    spec.stream = st;
    return spec;
}

// the optional sweep of a build (NULL: a plain cloud)
void take_sweep(BuildSpec& spec, const gicp_sweep* sw, int dim) {
    if (!sw) return;
    spec.sweep = true;
    spec.stamps = sw->stamps;
    spec.ref = sw->ref;
    if (dim == 2 || dim == 3) std::memcpy(spec.motion, sw->motion, sizeof(double) * (dim + 1) * (dim + 1));
}

VoxelMap& need_map(gicp_ctx* c) {
    if (!c->map.set) throw Fail{GICP_E_STATE, "no map: call gicp_map_reset first"};
    return c->map;
}

// Per-source-tile state that refers to target tiles (hints, candidate lists, heavy schedule):
// reset whenever either cloud changes.
void reset_tile_state(gicp_ctx* c) {
    const int nt = std::max(1, c->src.ntiles);
    if (!c->d_hint) return;
    // hints -1, lists empty, certificates none (cert_pass -1) and no last match (cert_j -1: k_corr's per-lane
    // search cap) -- one launch (five memsets were five queue operations, ~40 us of a C5 frame)
    HIPCHK(launch_reset_tiles(c->d_hint, c->d_list_len, c->d_list_rcert, c->d_cert_pass, nt, c->d_cert_j,
                              c->d_cert_j ? std::max<int64_t>(1, c->src.n) : 0, c->stream));
    c->pass = 0;
}

void set_shard(gicp_ctx* c, int shard, int nshards) {
    if (nshards < 1 || shard < 0 || shard >= nshards) throw Fail{GICP_E_INVALID, "bad shard / nshards"};
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

// The largest double x with sqrt(x) <= dc (sqrt correctly rounded, as on the device), so the accept
// test of gicp.py:136, !(distance > d_c) with distance = sqrt(d2), is exactly d2 <= accept_d2_max(d_c)
double accept_d2_max(double dc) {
    if (!(dc >= 0.0) || std::isinf(dc)) return dc;   // d_c = +inf accepts everything; NaN nothing
    double x = dc * dc;
    while (std::sqrt(x) > dc) x = std::nextafter(x, 0.0);
    while (std::sqrt(std::nextafter(x, INFINITY)) <= dc) x = std::nextafter(x, INFINITY);
    return x;
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

// One pass at pose T: statistics (all-reduced) into c->h_stats.
void run_pass(gicp_ctx* c, const double* T, gicp_debug* dbg) {
    if (!c->tgt.n || !c->src.n) throw Fail{GICP_E_STATE, "set_target and set_source first"};
    if (c->tgt.dim != c->src.dim) throw Fail{GICP_E_INVALID, "source and target dimensions differ"};
    const int d = c->src.dim, n1 = d + 1;
    for (int k = 0; k < n1 * n1; ++k)
        if (!std::isfinite(T[k])) throw Fail{GICP_E_INVALID, "pose contains non-finite values"};
    ensure_workspace(c);
    hipStream_t st = c->stream;
    IterState& hs = *c->h_state;
    std::memset(&hs, 0, offsetof(IterState, stats));
    for (int k = 0; k < n1 * n1; ++k) hs.T[k] = T[k];
    hs.converged_at = -1;
    HIPCHK(hipMemcpyAsync(c->d_state, &hs, offsetof(IterState, stats), hipMemcpyHostToDevice, st));
    CorrArgs a = corr_args(c, 1);
    c->top_ready = false;
    if (dbg && (dbg->index || dbg->weight || dbg->distance || dbg->want_top_weights)) {
        ensure_dbg(c);
        a.dbg_index = dbg->index ? c->d_dbg_idx : nullptr;
        a.dbg_weight = dbg->weight ? c->d_dbg_w : nullptr;
        a.dbg_dist = dbg->distance ? c->d_dbg_dist : nullptr;
        if (dbg->want_top_weights) {   // rows of other shards stay NaN (never selected); one shard writes every row
            if (c->nshards > 1) HIPCHK(hipMemsetAsync(c->d_dbg_det, 0xFF, sizeof(double) * c->src.n, st));
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
    if (grid > 0) {
        HIPCHK(launch_corr(a, d, grid, st));
    } else if (a.peer.n > 1) {   // no tile in this shard: one empty workgroup still takes part in the exchange
        a.q_end = 0;
        HIPCHK(launch_corr(a, d, 1, st));
    } else {
        HIPCHK(hipMemsetAsync(c->d_state->stats, 0, sizeof(double) * nsx, st));
    }
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
        if (fail == 2) throw Fail{GICP_E_COMM, "peer exchange timed out (a rank did not arrive)"};
    }
#if defined(GICP_STAMPS) || defined(GICP_TIMELINE)
    print_stamps(d_stamps, nst);
#endif
    const int ns = nstat(d);
    c->last_amb = c->h_stats[ns];
    c->last_pairs = c->h_stats[ns + 1];
    c->last_rebuilds = c->h_stats[ns + 2];
    c->last_sq = c->h_stats[ns + 3];
    c->last_gproved = c->h_stats[ns + 4];
    c->last_walked = c->h_stats[ns + 5];
    c->top_ready = a.dbg_det != nullptr;
}

}  // namespace

namespace {
// drop the peer exchange: unmap the peers' areas (this rank's own area stays, re-exportable)
void close_peers(gicp_ctx* c) {
    bool any = c->peer.n > 1;
    for (void* p : c->peer_open) any = any || p != nullptr;
    if (any) quiet(hipStreamSynchronize(c->stream));   // no launch of ours still uses the mappings
    for (auto& p : c->peer_open) {
        if (p) quiet(hipIpcCloseMemHandle(p));
        p = nullptr;
    }
    c->peer = PeerArgs{};
}

int guard_impl(gicp_ctx* c, const char* where, const std::function<void()>& body) {
    try {
        if (c) HIPCHK(hipSetDevice(c->device));
        body();
        return GICP_OK;
    } catch (const Fail& f) {
        if (c) c->err = std::string(where) + ": " + f.msg;
        return f.code;
    } catch (const std::bad_alloc&) {
        if (c) c->err = std::string(where) + ": out of host memory";
        return GICP_E_NOMEM;
    } catch (...) {
        if (c) c->err = std::string(where) + ": unknown error";
        return GICP_E_INVALID;
    }
}
}  // namespace

extern "C" {

int gicp_version(void) { return 102; }

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
    if (c->comm) ncclCommDestroy(c->comm);
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
    return guard_impl(c, "gicp_comm_init", [&] {
        if (c->comm) {
            ncclCommDestroy(c->comm);
            c->comm = nullptr;
        }
        c->hook = nullptr;   // one exchange per context
        close_peers(c);
        // a one-rank communicator is created too: the all-reduce then runs (as an identity) on the
        // same stream path as a multi-GPU job, which is how the one-GPU tests exercise it
        ncclUniqueId uid;
        std::memcpy(&uid, id, sizeof(uid));
        ncclResult_t r = ncclCommInitRank(&c->comm, nranks, uid, rank);
        if (r != ncclSuccess) throw Fail{GICP_E_COMM, std::string("ncclCommInitRank: ") + ncclGetErrorString(r)};
        c->nranks = nranks;
        c->rank = rank;
    });
}

int gicp_comm_ranks(gicp_ctx* c, int* nranks, int* rank, int* kind) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_comm_ranks", [&] {
        int n = 1, r = 0, k = 0;
        if (c->peer.n > 1) {
            n = c->peer.n;
            r = c->peer.rank;
            k = 3;
        } else if (c->comm) {
            ncclResult_t e = ncclCommCount(c->comm, &n);
            if (e == ncclSuccess) e = ncclCommUserRank(c->comm, &r);
            if (e != ncclSuccess) throw Fail{GICP_E_COMM, std::string("ncclCommCount: ") + ncclGetErrorString(e)};
            k = 1;
        } else if (c->hook) {
            n = c->nranks;
            r = c->rank;
            k = 2;
        }
        if (nranks) *nranks = n;
        if (rank) *rank = r;
        if (kind) *kind = k;
    });
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
        if (nshards < 1 || shard < 0 || shard >= nshards) throw Fail{GICP_E_INVALID, "bad shard / nshards"};
        c->psrc = resolve(dim, p);
        c->top_ready = false;
        BuildSpec spec;
        spec.cov_shard = shard;
        spec.cov_nshards = nshards;
        spec.tile_points = c->src_tile;
        spec.voxel_leaf = c->voxel_leaf;
        spec.voxel_min = c->voxel_min;
        spec.stream = c->stream;
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
        c->tgt.n = 0;
        c->tgt.cov_ready = false;
        c->psrc = c->ptgt;
        set_shard(c, shard, nshards);   // (its resets are stream-ordered before the next registration: no host sync)
    });
}

int gicp_get_covariances(gicp_ctx* c, int which, double* out) {
    if (!c || !out || (which != 0 && which != 1)) return GICP_E_INVALID;
    return guard_impl(c, "gicp_get_covariances", [&] {
        Cloud& cl = which == 0 ? c->tgt : c->src;
        if (!cl.n || !cl.cov_ready) throw Fail{GICP_E_STATE, "cloud not set"};
        // a I - m m^T expanded on the device in original order (k_rotate_cov with R = I: R m = m
        // exactly), then one copy of the n x d x d result
        const int d = cl.dim;
        const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        const double I2[4] = {1, 0, 0, 1};
        const size_t m = (size_t)cl.n * d * d;
        c->d_rot.reserve(m);
        HIPCHK(launch_rotate_cov(cl.cov, cl.perm, cl.n, d, d == 3 ? I : I2, c->d_rot, c->stream));
        HIPCHK(hipMemcpyAsync(out, c->d_rot, sizeof(double) * m, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
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
        Cloud& cl = which == 0 ? c->tgt : c->src;
        if (!cl.n) throw Fail{GICP_E_STATE, "cloud not set"};
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

int gicp_align(gicp_ctx* c, const double* T0, const gicp_params* p, double* T_out, gicp_result* res) {
    return gicp_align_trace(c, T0, p, T_out, res, nullptr);
}

int gicp_align_trace(gicp_ctx* c, const double* T0, const gicp_params* p, double* T_out, gicp_result* res,
                     gicp_trace* trace) {
    if (!c || !T_out) return GICP_E_INVALID;
    return guard_impl(c, "gicp_align", [&] {
        if (!c->tgt.n || !c->src.n) throw Fail{GICP_E_STATE, "set_target and set_source first"};
        if (c->tgt.dim != c->src.dim) throw Fail{GICP_E_INVALID, "source and target dimensions differ"};
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
                // rows of other shards stay NaN (never selected); one shard writes every row
                if (c->nshards > 1) HIPCHK(hipMemsetAsync(c->d_dbg_det, 0xFF, sizeof(double) * c->src.n, st));
            }
        }
        c->top_ready = false;
        // device state: T0, last_loss = inf (gicp.py:106-110)
        IterState& hs = *c->h_state;
        std::memset(&hs, 0, offsetof(IterState, stats));
        for (int k = 0; k < n1 * n1; ++k) hs.T[k] = T0 ? T0[k] : ((k % (n1 + 1)) == 0 ? 1.0 : 0.0);
        for (int k = 0; k < n1 * n1; ++k)
            if (!std::isfinite(hs.T[k])) throw Fail{GICP_E_INVALID, "T0 contains non-finite values"};
        hs.last_loss = INFINITY;
        hs.tol = prm.tolerance;
        hs.fixed = prm.fixed_iterations ? 1 : 0;
        hs.trans_eps = prm.transformation_epsilon;
        hs.rot_cos = prm.rotation_epsilon;
        hs.fit_eps = prm.euclidean_fitness_epsilon;
        hs.rel_eps = prm.mse_relative_epsilon;
        hs.prev_mse = INFINITY;
        hs.pairs_total = 0.0;
        hs.converged_at = -1;
        HIPCHK(hipMemcpyAsync(c->d_state, &hs, offsetof(IterState, stats), hipMemcpyHostToDevice, st));   // (xchg_* = 0)
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
                if (grid > 0) {
                    HIPCHK(launch_corr(a, d, grid, st));
                } else if (peer) {   // no tile in this shard: one empty workgroup takes part in the exchange
                    a.q_end = 0;
                    HIPCHK(launch_corr(a, d, 1, st));
                } else {
                    HIPCHK(hipMemsetAsync(c->d_state->stats, 0, sizeof(double) * nstat_ext(d), st));
                }
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
        if (hs.solve_fail == 2) throw Fail{GICP_E_COMM, "peer exchange timed out (a rank did not arrive)"};
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
            c->last_amb = hs.stats_solved[ns];
            c->last_pairs = hs.stats_solved[ns + 1];
            c->last_rebuilds = hs.stats_solved[ns + 2];
            c->last_sq = hs.stats_solved[ns + 3];
            c->last_gproved = hs.stats_solved[ns + 4];
            c->last_walked = hs.stats_solved[ns + 5];
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
                int khz = 0;
                HIPCHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device));
                const double us = 1e3 / (khz > 0 ? khz : 100000);
                r.exchange_us_mean = hs.xchg_sum / hs.xchg_n * us;
                r.exchange_us_min = hs.xchg_min * us;
            }
            *res = r;
        }
    });
}

namespace {
// the slot's build thread: waits for a queued build, runs it on the slot's stream, reports state 2
void staged_worker(gicp_ctx::Staged* gp) {
    for (;;) {
        {
            std::unique_lock<std::mutex> lk(gp->m);
            gp->cv.wait(lk, [&] { return gp->quit || gp->state == 1; });
            if (gp->state != 1) return;   // quit with nothing queued
        }
        int rc = GICP_OK;
        std::string err;
        try {
            HIPCHK(hipSetDevice(gp->device));
            build_cloud(gp->cl, gp->xyz, gp->M, gp->dim, gp->p, gp->bs, gp->spec);
        } catch (const Fail& f) {
            rc = f.code;
            err = f.msg;
        } catch (const std::bad_alloc&) {
            rc = GICP_E_NOMEM;
            err = "out of host memory";
        } catch (...) {
            rc = GICP_E_INVALID;
            err = "unknown error";
        }
        {
            std::lock_guard<std::mutex> g(gp->m);
            gp->rc = rc;
            gp->err = err;
            gp->state = 2;
        }
        gp->cv.notify_all();
    }
}
}  // namespace

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
        if (!xyz || M <= 0 || (dim != 2 && dim != 3)) throw Fail{GICP_E_INVALID, "cloud must be a non-empty N x 2 or N x 3 array"};
        if (flags & ~GICP_STAGE_BORROW) throw Fail{GICP_E_INVALID, "unknown gicp_stage_target_ex flags"};
        if (sw) {   // a sweep no build would take is refused here, with no slot used
            if (!sw->stamps) throw Fail{GICP_E_INVALID, "a sweep needs stamps (gicp_sweep.stamps is NULL)"};
            double xi[6];
            motion_twist(dim, sw->motion, xi);
        }
        gicp_ctx::Staged& g = c->stg[(c->stg_head + c->stg_count) % GICP_MAX_STAGED];
        g.wait_idle();   // (a slot is only reused after its commit or cancel; a build never runs here)
        const gicp_params prm = resolve(dim, p);
        if (!g.stream) HIPCHK(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
        const double* src = xyz;
        const double* stamps = sw ? sw->stamps : nullptr;
        if (!(flags & GICP_STAGE_BORROW)) {
            // (the stamps of a sweep lie behind the points in the same pinned buffer)
            const size_t need = (size_t)M * dim + (sw ? (size_t)M : 0);
            // grow-only pinned staging buffer (allocated here, not in the worker), with headroom from the first
            // allocation on: need / 8
            if (need > g.bs.h_pinned.capacity()) g.bs.h_pinned.alloc(need + need / 8);
            // the caller's scan is copied into the slot's pinned buffer before this call returns (the caller
            // may refill its buffer at once): 16 fixed chunks on the calling thread's tiling pool (a 100k-point
            // frame, 2.4 MB, in ~0.06 ms instead of one thread's ~0.3 ms)
            const size_t total = sizeof(double) * (size_t)M * dim;
            char* dst = reinterpret_cast<char*>(g.bs.h_pinned.get());
            const char* srcb = reinterpret_cast<const char*>(xyz);
            constexpr int kChunks = 16;
            c->bs.workers().run(kChunks, [&](int k) {
                const size_t b0 = total * k / kChunks, b1 = total * (k + 1) / kChunks;
                std::memcpy(dst + b0, srcb + b0, b1 - b0);
            });
            src = g.bs.h_pinned;
            if (sw) {
                double* ds = g.bs.h_pinned.get() + (size_t)M * dim;
                std::memcpy(ds, sw->stamps, sizeof(double) * (size_t)M);
                stamps = ds;
            }
        }
        if (!g.th.joinable()) g.th = std::thread(staged_worker, &g);
        {
            std::lock_guard<std::mutex> lk(g.m);
            g.xyz = src;
            g.M = M;
            g.dim = dim;
            g.device = c->device;
            g.spec = target_spec(c, g.stream);
            g.spec.staged = true;
            take_sweep(g.spec, sw, dim);
            g.spec.stamps = stamps;
            g.p = prm;
            g.rc = GICP_OK;
            g.err.clear();
            g.state = 1;
        }
        g.cv.notify_all();
        ++c->stg_count;
    });
}

int gicp_commit_target(gicp_ctx* c, int shard, int nshards) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_commit_target", [&] {
        if (!c->stg_count) throw Fail{GICP_E_STATE, "no staged target (gicp_stage_target first)"};
        gicp_ctx::Staged& g = c->stg[c->stg_head];
        g.wait_idle();
        c->stg_head = (c->stg_head + 1) % GICP_MAX_STAGED;
        --c->stg_count;
        {
            std::lock_guard<std::mutex> lk(g.m);
            g.state = 0;
            g.xyz = nullptr;
        }
        if (g.rc != GICP_OK) throw Fail{g.rc, "staged build: " + g.err};
        if (nshards < 1 || shard < 0 || shard >= nshards) throw Fail{GICP_E_INVALID, "bad shard / nshards"};
        // the current target (index + covariances) becomes the source, as robot-visualization.py:250
        // swaps scans, and the staged cloud the target; the old source's buffers wait in the slot
        if (c->tgt.n) {
            std::swap(c->src, c->tgt);
            c->psrc = c->ptgt;
        }
        std::swap(c->tgt, g.cl);
        g.cl.n = 0;
        g.cl.cov_ready = false;
        g.cl.graph_ready = false;
        c->ptgt = g.p;
        c->top_ready = false;
        if (c->src.n) set_shard(c, shard, nshards);   // (stream-ordered resets: no host sync)
    });
}

int gicp_cancel_stage(gicp_ctx* c) {
    if (!c) return GICP_E_INVALID;
    for (auto& g : c->stg) {
        g.wait_idle();
        std::lock_guard<std::mutex> lk(g.m);
        g.state = 0;
        g.xyz = nullptr;
    }
    c->stg_head = c->stg_count = 0;
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
    return guard_impl(c, "gicp_set_allreduce", [&] {
        if (fn) close_peers(c);
        if (fn && !c->h_xchg) c->h_xchg.alloc(80);
        if (fn && c->comm) {   // one exchange per context: the hook replaces the communicator
            HIPCHK(hipStreamSynchronize(c->stream));
            ncclCommDestroy(c->comm);
            c->comm = nullptr;
        }
        c->hook = fn;
        c->hook_user = fn ? user : nullptr;
        if (!c->comm) {   // what gicp_comm_ranks reports for the hook
            c->nranks = fn ? nranks : 1;
            c->rank = fn ? rank : 0;
        }
    });
}

int gicp_peer_export(gicp_ctx* c, char handle[GICP_PEER_HANDLE_BYTES]) {
    if (!c || !handle) return GICP_E_INVALID;
    return guard_impl(c, "gicp_peer_export", [&] {
        static_assert(sizeof(hipIpcMemHandle_t) + sizeof(uint64_t) == GICP_PEER_HANDLE_BYTES, "IPC handle + counter");
        if (!c->d_peer_area) {   // uncached: peers' stores and this rank's polling meet in memory
            double* area = nullptr;   // published only once it is zeroed
            HIPCHK(hipExtMallocWithFlags(reinterpret_cast<void**>(&area), sizeof(double) * kPeerAreaDoubles,
                                         hipDeviceMallocUncached));
            try {
                HIPCHK(hipMemset(area, 0, sizeof(double) * kPeerAreaDoubles));
                HIPCHK(hipDeviceSynchronize());
            } catch (...) {
                dev_free(area);
                throw;
            }
            c->d_peer_area = area;
        }
        if (!c->d_peer_ctr) alloc_init(c->d_peer_ctr, 1, [](uint64_t* d) { HIPCHK(hipMemset(d, 0, sizeof(uint64_t))); });
        hipIpcMemHandle_t h;
        HIPCHK(hipIpcGetMemHandle(&h, c->d_peer_area));
        uint64_t seq = 0;   // this rank's exchange counter (its launches have finished: stream sync)
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(&seq, c->d_peer_ctr, sizeof(seq), hipMemcpyDeviceToHost));
        std::memcpy(handle, &h, sizeof(h));
        std::memcpy(handle + sizeof(h), &seq, sizeof(seq));
    });
}

int gicp_peer_init(gicp_ctx* c, int nranks, int rank, const char* handles, double timeout_s) {
    if (!c || !handles || nranks < 2 || nranks > GICP_MAX_PEERS || rank < 0 || rank >= nranks || !(timeout_s > 0.0))
        return GICP_E_INVALID;
    return guard_impl(c, "gicp_peer_init", [&] {
        if (!c->d_peer_area || !c->d_peer_ctr) throw Fail{GICP_E_STATE, "gicp_peer_export first"};
        close_peers(c);
        PeerArgs p{};
        p.n = nranks;
        p.rank = rank;
        p.own = c->d_peer_area;
        p.ctr = c->d_peer_ctr;
        // every rank starts at the largest counter any rank exported: above every flag left in any area
        uint64_t seq0 = 0;
        for (int r = 0; r < nranks; ++r) {
            uint64_t v = 0;
            std::memcpy(&v, handles + (size_t)r * GICP_PEER_HANDLE_BYTES + sizeof(hipIpcMemHandle_t), sizeof(v));
            seq0 = std::max(seq0, v);
        }
        HIPCHK(hipMemcpy(c->d_peer_ctr, &seq0, sizeof(seq0), hipMemcpyHostToDevice));
        double* area[kMaxPeers] = {};
        try {
            for (int r = 0; r < nranks; ++r) {
                if (r == rank) {
                    area[r] = c->d_peer_area;
                    continue;
                }
                hipIpcMemHandle_t h;
                std::memcpy(&h, handles + (size_t)r * GICP_PEER_HANDLE_BYTES, sizeof(h));
                void* ptr = nullptr;
                const hipError_t e = hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess);
                if (e != hipSuccess) {
                    (void)hipGetLastError();
                    throw Fail{GICP_E_COMM, std::string("hipIpcOpenMemHandle(rank ") + std::to_string(r) + "): " +
                                                hipGetErrorString(e)};
                }
                c->peer_open[r] = ptr;
                area[r] = static_cast<double*>(ptr);
            }
            if (!c->d_peer_ptrs) c->d_peer_ptrs.alloc(kMaxPeers);
            HIPCHK(hipMemcpy(c->d_peer_ptrs, area, sizeof(area), hipMemcpyHostToDevice));
            p.area = c->d_peer_ptrs;
            int khz = 0;
            HIPCHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device));
            p.timeout = (uint64_t)(timeout_s * (khz > 0 ? khz : 100000) * 1e3);
            // the probe: kPeerProbeRounds full-slot exchanges checked bit for bit, which every rank runs now
            if (!c->d_probe) c->d_probe.alloc(2);
            HIPCHK(launch_peer_probe(p, c->d_probe, c->stream));
            double got[2] = {0, 0};
            HIPCHK(hipMemcpyAsync(got, c->d_probe, sizeof(got), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            if (got[0] != (double)kPeerProbeRounds || got[1] != 0.0)
                throw Fail{GICP_E_COMM, got[0] < 0.0 ? std::string("peer exchange probe failed (a rank did not arrive)")
                                                     : "peer exchange probe failed (" + std::to_string((int)got[1]) +
                                                           " of " + std::to_string(kPeerSlot * kPeerProbeRounds) +
                                                           " summed values wrong after " +
                                                           std::to_string((int)got[0]) + " rounds)"};
        } catch (...) {
            close_peers(c);
            throw;
        }
        // the peer exchange replaces any other exchange of this context
        if (c->comm) {
            ncclCommDestroy(c->comm);
            c->comm = nullptr;
        }
        c->hook = nullptr;
        c->peer = p;
        c->peer_timeout_s = timeout_s;
        c->nranks = nranks;
        c->rank = rank;
    });
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
        Cloud& cl = which == 0 ? c->tgt : c->src;
        if (!cl.n || !cl.cov_ready) throw Fail{GICP_E_STATE, "cloud not set"};
        const int d = cl.dim;
        for (int k = 0; k < d * d; ++k)
            if (!std::isfinite(R[k])) throw Fail{GICP_E_INVALID, "R contains non-finite values"};
        const size_t m = (size_t)cl.n * d * d;
        c->d_rot.reserve(m);
        HIPCHK(launch_rotate_cov(cl.cov, cl.perm, cl.n, d, R, c->d_rot, c->stream));
        HIPCHK(hipMemcpyAsync(out, c->d_rot, sizeof(double) * m, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
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
        if (!xyz || N <= 0 || (dim != 2 && dim != 3)) throw Fail{GICP_E_INVALID, "cloud must be a non-empty N x 2 or N x 3 array"};
        if (N > (int64_t)0x7FFFFFFF - 64) throw Fail{GICP_E_INVALID, "cloud too large (> 2^31 points)"};
        if (!out_xyz || !M_out) throw Fail{GICP_E_INVALID, "out_xyz and M_out must not be NULL"};
        if (!std::isfinite(leaf) || leaf <= 0.0) throw Fail{GICP_E_INVALID, "leaf must be finite and > 0"};
        if (min_points < 1) throw Fail{GICP_E_INVALID, "min_points must be >= 1"};
        *M_out = 0;
        double mn[3], mx[3];
        scan_bounds(xyz, N, dim, mn, mx);
        BuildScratch& bs = c->bs;
        hipStream_t st = c->stream;
        bs.v_raw.reserve((size_t)N * dim);
        bs.s_in.reserve((size_t)N * dim);
        HIPCHK(hipMemcpyAsync(bs.v_raw, xyz, sizeof(double) * N * dim, hipMemcpyHostToDevice, st));
        const VoxelOut vo = voxel_filter(bs, bs.v_raw, N, dim, mn, mx, leaf, min_points, bs.s_in, st);
        HIPCHK(hipMemcpyAsync(out_xyz, bs.s_in, sizeof(double) * vo.M * dim, hipMemcpyDeviceToHost, st));
        if (out_count) HIPCHK(hipMemcpyAsync(out_count, bs.v_ocnt, sizeof(int32_t) * vo.M, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        *M_out = vo.M;
    });
}

int gicp_cloud_size(gicp_ctx* c, int which, int64_t* n) {
    if (!c || !n || (which != 0 && which != 1)) return GICP_E_INVALID;
    *n = (which == 0 ? c->tgt : c->src).n;
    return GICP_OK;
}

int gicp_get_points(gicp_ctx* c, int which, double* out) {
    if (!c || !out || (which != 0 && which != 1)) return GICP_E_INVALID;
    return guard_impl(c, "gicp_get_points", [&] {
        Cloud& cl = which == 0 ? c->tgt : c->src;
        if (!cl.n) throw Fail{GICP_E_STATE, "cloud not set"};
        const size_t m = (size_t)cl.n * cl.dim;
        c->d_rot.reserve(m);
        HIPCHK(launch_points_out(cl.xyz64, cl.perm, cl.n, cl.dim, c->d_rot, c->stream));
        HIPCHK(hipMemcpyAsync(out, c->d_rot, sizeof(double) * m, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    });
}

// ---- motion compensation ----

namespace {
// a host-only entry point's body: no context, no HIP call
int host_guard(const std::function<void()>& body) {
    try {
        body();
        return GICP_OK;
    } catch (const Fail& f) {
        return f.code;
    } catch (...) {
        return GICP_E_INVALID;
    }
}

void check_sweep_args(const double* xyz, const double* stamps, int64_t N, int dim, const double* out) {
    if (!xyz || N <= 0 || (dim != 2 && dim != 3)) throw Fail{GICP_E_INVALID, "cloud must be a non-empty N x 2 or N x 3 array"};
    if (N > (int64_t)0x7FFFFFFF - 64) throw Fail{GICP_E_INVALID, "cloud too large (> 2^31 points)"};
    if (!stamps) throw Fail{GICP_E_INVALID, "a sweep needs stamps (stamps is NULL)"};
    if (!out) throw Fail{GICP_E_INVALID, "out must not be NULL"};
}
}  // namespace

int gicp_motion_twist(int dim, const double* M, double* xi) {
    return host_guard([&] { motion_twist(dim, M, xi); });
}

int gicp_deskew_host(const double* xyz, const double* stamps, int64_t N, int dim, const double* M, double ref,
                     double* out) {
    return host_guard([&] {
        check_sweep_args(xyz, stamps, N, dim, out);
        double mn[3], mx[3], xi[6];
        scan_bounds(xyz, N, dim, mn, mx);   // (the finiteness test)
        scan_stamps(stamps, N, ref);
        motion_twist(dim, M, xi);
        if (dim == 3) deskew_host<3>(xyz, stamps, N, xi, ref, out);
        else deskew_host<2>(xyz, stamps, N, xi, ref, out);
    });
}

int gicp_deskew(gicp_ctx* c, const double* xyz, const double* stamps, int64_t N, int dim, const double* M, double ref,
                double* out) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_deskew", [&] {
        check_sweep_args(xyz, stamps, N, dim, out);
        double mn[3], mx[3], xi[6];
        scan_bounds(xyz, N, dim, mn, mx);   // (the finiteness test)
        scan_stamps(stamps, N, ref);
        motion_twist(dim, M, xi);
        BuildScratch& bs = c->bs;
        hipStream_t st = c->stream;
        bs.s_in.reserve((size_t)N * dim);
        HIPCHK(hipMemcpyAsync(bs.s_in, xyz, sizeof(double) * N * dim, hipMemcpyHostToDevice, st));
        deskew_launch(bs, bs.s_in, stamps, N, dim, xi, ref, st);
        unsigned long long res[kVoxelRes];
        HIPCHK(hipMemcpyAsync(out, bs.s_in, sizeof(double) * N * dim, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(res, bs.v_res, sizeof res, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        deskew_decode(res, dim, mn, mx);   // (refuses a result that is not finite)
    });
}

int gicp_map_reset(gicp_ctx* c, int dim, double leaf, double max_range) {
    if (!c) return GICP_E_INVALID;
    return guard_impl(c, "gicp_map_reset", [&] {
        if (dim != 2 && dim != 3) throw Fail{GICP_E_INVALID, "dim must be 2 or 3"};
        if (!std::isfinite(leaf) || leaf <= 0.0) throw Fail{GICP_E_INVALID, "leaf must be finite and > 0"};
        if (!std::isfinite(max_range) || max_range <= 0.0) throw Fail{GICP_E_INVALID, "max_range must be finite and > 0"};
        const double R = std::ceil(max_range / leaf);
        const double lim = dim == 3 ? 2097152.0 : 2147483648.0;   // 2^21, 2^31 cells per axis (the filter's limits)
        if (!(2.0 * R + 1.0 <= lim)) {
            char b[160];
            std::snprintf(b, sizeof b, "map window too wide: %.6g cells of leaf %g per axis (at most 2^%d per axis in %d-D)",
                          2.0 * R + 1.0, leaf, dim == 3 ? 21 : 31, dim);
            throw Fail{GICP_E_INVALID, b};
        }
        VoxelMap& mp = c->map;   // (buffers are kept: grow-only)
        mp.set = true;
        mp.dim = dim;
        mp.leaf = leaf;
        mp.R = (int64_t)R;
        uint64_t r = (uint64_t)(2 * mp.R);
        mp.bits = 0;
        while (r) ++mp.bits, r >>= 1;
        mp.rows = 0;
    });
}

int gicp_map_insert(gicp_ctx* c, int which, const double* T) {
    if (!c || !T || (which != 0 && which != 1)) return GICP_E_INVALID;
    return guard_impl(c, "gicp_map_insert", [&] {
        VoxelMap& mp = need_map(c);
        Cloud& cl = which == 0 ? c->tgt : c->src;
        if (!cl.n) throw Fail{GICP_E_STATE, "cloud not set"};
        if (cl.dim != mp.dim) throw Fail{GICP_E_INVALID, "the cloud's dimension differs from the map's"};
        mp.pts.reserve((size_t)cl.n * cl.dim);
        HIPCHK(launch_points_out(cl.xyz64, cl.perm, cl.n, cl.dim, mp.pts, c->stream));
        map_insert_core(mp, c->bs, cl.n, T, c->stream);
    });
}

int gicp_map_insert_points(gicp_ctx* c, const double* xyz, int64_t n, int dim, const double* T) {
    if (!c || !T) return GICP_E_INVALID;
    return guard_impl(c, "gicp_map_insert_points", [&] {
        VoxelMap& mp = need_map(c);
        if (!xyz || n <= 0 || (dim != 2 && dim != 3)) throw Fail{GICP_E_INVALID, "cloud must be a non-empty N x 2 or N x 3 array"};
        if (n > (int64_t)0x7FFFFFFF - 64) throw Fail{GICP_E_INVALID, "cloud too large (> 2^31 points)"};
        if (dim != mp.dim) throw Fail{GICP_E_INVALID, "the cloud's dimension differs from the map's"};
        double mn[3], mx[3];
        scan_bounds(xyz, n, dim, mn, mx);   // (the finiteness test)
        mp.pts.reserve((size_t)n * dim);
        HIPCHK(hipMemcpyAsync(mp.pts, xyz, sizeof(double) * n * dim, hipMemcpyHostToDevice, c->stream));
        map_insert_core(mp, c->bs, n, T, c->stream);
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
        const int dim = mp.dim;
        const int64_t m = mp.rows;
        BuildScratch& bs = c->bs;
        hipStream_t st = c->stream;
        BuildLog log(st);
        bs.s_in.reserve((size_t)m * dim);
        bs.v_flag.reserve((size_t)m);
        bs.v_idx.reserve((size_t)m);
        if (!bs.v_res) bs.v_res.alloc((size_t)kVoxelRes);
        size_t tmp_bytes = 0;
        HIPCHK(voxel_temp_bytes(m, 1, &tmp_bytes, st));
        bs.v_tmp.reserve(tmp_bytes + 16);
        HIPCHK(launch_map_centroids(mp.sums[mp.cur], m, dim, min_points, bs.v_flag, bs.v_idx, bs.v_tmp, tmp_bytes, bs.s_in,
                                    bs.v_res, st));
        unsigned long long res[kVoxelRes];
        HIPCHK(hipMemcpyAsync(res, bs.v_res, sizeof res, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const int64_t M = (int64_t)res[6];
        if (M <= 0) {
            char b[128];
            std::snprintf(b, sizeof b, "map: none of the %lld voxels holds min_points = %d points", (long long)m, min_points);
            throw Fail{GICP_E_INVALID, b};
        }
        double mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
        for (int a = 0; a < dim; ++a) {
            mn[a] = dec_ordered(res[a]);
            mx[a] = dec_ordered(res[3 + a]);
        }
        log.tick("map-centroids");
        c->ptgt = resolve(dim, p);
        c->top_ready = false;
        Cloud& cl = c->tgt;
        cl.n = 0;   // buffers are kept (grow-only) and reused
        cl.cov_ready = false;
        cl.graph_ready = false;
        cl.dim = dim;
        cl.bits = dim == 3 ? 10 : 16;
        build_core(cl, M, dim, mn, mx, c->ptgt, bs, target_spec(c, st), log);   // (the centroids are not filtered again)
        if (c->src.n) reset_tile_state(c);
    });
}

}  // extern "C"
