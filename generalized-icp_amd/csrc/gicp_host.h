// gicp_host.h — what the host units of libgicp_hip.so share (gicp_capi.cpp, gicp_build.cpp, gicp_align.cpp,
// gicp_exchange.cpp): the HIP error macro, the kernel launchers, the clouds, the context.  Private to those
// files; no .hip file includes it.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "gicp_cluster.h"
#include "gicp_filter.h"
#include "gicp_hostmath.h"
#include "gicp_sor.h"
#include "gicp_sweep.h"

namespace gicp {
hipError_t launch_morton(const double*, int64_t, int, const DevCloud&, uint32_t*, int32_t*, hipStream_t);
hipError_t launch_build_tiles(const double*, int, int32_t*, TileInfo*, TileBox*, int, PointRec*, float4*, int32_t*,
                              unsigned*, hipStream_t);
hipError_t launch_build_blocks(const TileInfo*, int, BlockInfo*, int, int, hipStream_t);
hipError_t launch_knn_cov(const CovArgs&, int, int, bool, hipStream_t);
hipError_t launch_corr(const CorrArgs&, int, int, hipStream_t);
hipError_t launch_solve(IterState*, int, hipStream_t, double*);
hipError_t launch_peer_probe(const PeerArgs&, double*, hipStream_t);
hipError_t launch_reset_tiles(int32_t*, int32_t*, float*, int32_t*, int, int32_t*, int64_t, double*, hipStream_t);
hipError_t launch_graph_pack(const GraphArgs&, hipStream_t);
hipError_t launch_rotate_cov(const PointRec*, double, const int32_t*, int64_t, int, const double*, double*, hipStream_t);
hipError_t launch_top_weights(const double*, const int64_t*, const int32_t*, int64_t, int, double*, int64_t*, int, double*, int64_t*,
                              int64_t*, hipStream_t);
hipError_t voxel_temp_bytes(int64_t, int, size_t*, hipStream_t);
hipError_t launch_voxel(const VoxelArgs&, hipStream_t);
hipError_t launch_crop(const CropArgs&, hipStream_t);
hipError_t launch_ror(const VoxelArgs&, const RorArgs&, hipStream_t);
hipError_t launch_points_out(const PointRec*, const int32_t*, int64_t, int, double*, hipStream_t);
hipError_t launch_deskew(const SweepArgs&, hipStream_t);
hipError_t launch_eval(const EvalArgs&, hipStream_t);
hipError_t launch_map_insert(const VoxelArgs&, const MapArgs&, hipStream_t);
hipError_t launch_map_centroids(const double*, int64_t, int, int, int32_t*, int32_t*, void*, size_t, double*,
                                unsigned long long*, hipStream_t);
hipError_t launch_batch_cov(const BatchCovArgs&, int, int, int, hipStream_t);
hipError_t launch_batch_align(const BatchArgs&, int, int, hipStream_t);
int batch_max_points(int dim);
hipError_t launch_knn_query(const KnnArgs&, hipStream_t);
hipError_t launch_sor(const SorArgs&, hipStream_t);
hipError_t launch_cluster(const VoxelArgs&, const ClusterArgs&, hipStream_t);
size_t sor_part_count(int64_t n);
int corr_grid(int q_tiles, int shard, int nshards);
int solve_pose(int d, const double* st, const double* Tk, double* Tout, double* loss_out);

// a failing HIP call is reported to the caller (the exception) and its error cleared from HIP's
// per-thread last error here, so it cannot fail a later call's first launch check
#define HIPCHK(x)                                                                                  \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            (void)hipGetLastError();                                                               \
            throw gicp::Fail{GICP_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)};         \
        }                                                                                          \
    } while (0)

// a HIP call whose failure is deliberately ignored (teardown): its error must not linger either
inline void quiet(hipError_t e) {
    if (e != hipSuccess) (void)hipGetLastError();
}

// One indexed cloud on the device.
struct Cloud {
    int dim = 0;
    int64_t n = 0;
    int ntiles = 0, nblocks = 0, level = 0, bits = 0;   // level: tile extent-cap step k (cap 2^(1 + k/4) cells)
    double lo[3] = {0, 0, 0};
    double scale = 1.0;
    float rho = 0.f;
    double bb_lo[3] = {0, 0, 0}, bb_hi[3] = {0, 0, 0};   // exact bounds of the indexed points (the kNN screen's d_max)
    // the epsilon the cloud was built with (a of C = a I - m m^T for every surface point, DevCloud::eps_a): it
    // belongs to the cloud, not to the context's current parameters, and moves with it through every swap
    double eps_a = 0.0;
    // the buffers are grow-only and move with the cloud: a swap of two clouds swaps them, and the side that
    // is then cleared (n = 0) keeps its buffers as spares for the next build
    DevBuf<PointRec> rec;             // positions and covariances, one 48-B record per point
    DevBuf<float4> rel32;
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

    // NOT SET: every entry point tells a usable cloud by n alone; the buffers are kept (grow-only) and reused
    void unset() {
        n = 0;
        cov_ready = false;
        graph_ready = false;
    }
    void reserve_points(int64_t np) {
        rec.reserve((size_t)np);
        rel32.reserve((size_t)np);
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
        v.rec = rec;
        v.rel32 = rel32;
        v.eps_a = eps_a;
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
    // input filters (gicp_filter.hip): two clouds the stages alternate between, the points in key order, keep
    // flags and their scan, the original row of each survivor after each stage, the counts (one-shot only); the
    // keys, the sort's scratch and the result words are the voxel filter's
    DevBuf<double> f_pts[2], f_packed;
    DevBuf<int32_t> f_keep, f_pos, f_idx[2], f_cnt;
    // statistical outlier removal (gicp_sor.hip): the index of the stage's rows (index only) and the
    // self-query's answers, the means, the trees' partials, the sums and result doubles, the survivors and their rows
    Cloud o_cl;
    DevBuf<int64_t> o_idx;
    DevBuf<double> o_d2, o_mean, o_part, o_stats, o_pts;
    DevBuf<int32_t> o_cnt, o_rows;
    // Euclidean cluster extraction (gicp_cluster.hip): the forest, the sizes by root, the root flags
    // and their scan, labels and sizes by cluster, the survivors and their rows; keys, sort, packed points, keep
    // flags and result words are the input filters'
    DevBuf<int32_t> c_parent, c_size, c_root, c_cid, c_labels, c_sizes, c_rows;
    DevBuf<double> c_pts;
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
    // the input filters, run after the de-skew and before the voxel filter; all-zero: off
    gicp_filter filter{};
    // statistical outlier removal, run after the input filters and before the voxel filter; k = 0: off
    gicp_sor sor{};
    // Euclidean cluster extraction, run after statistical outlier removal and before the voxel filter;
    // radius = 0: off
    gicp_cluster cluster{};
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
        std::snprintf(b, sizeof b, " %s %.3f", what, std::chrono::duration<double, std::milli>(t - prev).count());
        text += b;
        prev = t;
    }
};

}  // namespace gicp

struct gicp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    gicp::Cloud tgt, src;
    gicp_params ptgt{}, psrc{};
    int shard = 0, nshards = 1, q_begin = 0, q_end = 0;
    // Every device and pinned buffer below owns itself (gicp_mem.h): delete c releases them.  The reserved ones
    // are grow-only (a frame stream allocates once); the fixed ones are allocated on first use.
    gicp::DevBuf<int32_t> d_hint;
    gicp::DevBuf<double> d_partials;
    gicp::DevBuf<gicp::IterState> d_state;
    gicp::PinnedBuf<gicp::IterState> h_state;     // pinned mirror
    gicp::DevBuf<uint32_t> d_tickets;
    gicp::DevBuf<double> d_gpart;
    double h_stats[80];
    gicp::DevBuf<int64_t> d_dbg_idx;
    gicp::DevBuf<double> d_dbg_w, d_dbg_dist;
    gicp::DevBuf<double> d_dbg_det;   // det(W) per source point (gicp_top_weights)
    bool top_ready = false;           // the last pass recorded det(W)
    // the top-k of that pass, computed inside the pass (same stream sync) for k = top_k_pref, the k the
    // last gicp_top_weights call asked for: [0, 16) source, [16, 32) target indices, then 16 det values
    int top_k_pref = 5, top_cached_k = 0;
    gicp::PinnedBuf<int64_t> h_top;   // 32 int64 + 16 double
    gicp::DevBuf<double> d_top_v;     // top-k scratch: stage-1 candidates and outputs
    gicp::DevBuf<int64_t> d_top_i;
    gicp::DevBuf<int64_t> d_top_tgt;  // [N] sorted order: target of each correspondence (with det(W))
    gicp::DevBuf<int64_t> d_top_out;
    // per-source-tile candidate lists
    gicp::DevBuf<int32_t> d_list, d_list_len, d_list_pass;
    gicp::DevBuf<float> d_list_rcert;
    gicp::DevBuf<double> d_poses;
    // per-source-point nearest-neighbour certificates
    gicp::DevBuf<int32_t> d_cert_j;
    gicp::DevBuf<float> d_cert_gap;
    gicp::DevBuf<int32_t> d_cert_pass;
    bool use_certs = true;            // GICP_NO_CERTS=1: every pass walks every lane
    bool use_graph = true;            // GICP_NO_GRAPH=1: no target neighbour graph, no graph descent
    bool fuse_solve = true;           // GICP_FUSE_SOLVE=0: the solve as its own k_solve launch even with no exchange
    int unit_map = 0;                 // k_corr workgroup -> unit map (CorrArgs::unit_map, GICP_UNIT_MAP)
    int moving_map = 8;               // ... for the first moving_iters iterations of an align (GICP_MOVING_MAP)
    int moving_iters = 5;             // (GICP_MOVING_ITERS)
    int src_tile = gicp::kTile;       // source points per tile at most: 64, 32 or 16 (GICP_SRC_TILE)
    double kappa_frac = 0.002;        // certificate gap resolved by the walk, fraction of d_c (GICP_CERT_KAPPA)
    int sparse_max = 4;               // CorrArgs::sparse_max (GICP_SPARSE_WALK; 0: sparse waves walk like the rest)
    int sparse_amb = 2;               // CorrArgs::sparse_amb (GICP_SPARSE_AMB; 0: every fp64 re-resolution wave-wide)
    // cloud-build scratch (synchronous builds) and per-source-tile arrays, grow-only (a frame stream
    // allocates once)
    gicp::BuildScratch bs;
    // voxel filter of every later cloud build (gicp_set_voxel): leaf 0 = off
    double voxel_leaf = 0.0;
    int voxel_min = 1;
    gicp_filter filt{};               // input filters of every later cloud build (gicp_set_filter): all-zero = off
    gicp_sor sor{};                   // statistical outlier removal of every later cloud build (gicp_set_sor): k = 0 = off
    gicp_cluster cluster{};           // cluster extraction of every later cloud build (gicp_set_cluster): radius = 0 = off
    gicp::VoxelMap map;               // local voxel map (gicp_map_reset)
    // staged targets (gicp_stage_target / gicp_commit_target): a ring of GICP_MAX_STAGED slots, each
    // built into its own cloud on its own stream by a host thread while the current target is
    // registered; commits take them in staging order
    // Each slot owns a persistent build thread (started on first use): a thread per staged frame cost
    // tens of microseconds of the caller's time per frame.  state: 0 idle, 1 build queued or running,
    // 2 built (rc / err hold the outcome); the caller waits for state != 1 before it takes the slot.
    struct Staged {
        gicp::Cloud cl;
        gicp::BuildScratch bs;
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
        gicp::BuildSpec spec;          // graph, the context's filter setting when the build was staged, this stream
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
    gicp::PinnedBuf<double> h_xchg;   // exchange buffer of the hook
    // in-kernel peer exchange (gicp_peer_export / gicp_peer_init)
    // This rank's exchange area: uncached device memory (hipExtMallocWithFlags) that other processes map through
    // IPC, so it is no DevBuf.  A raw pointer, set only once the area is zeroed, with one free in gicp_destroy.
    double* d_peer_area = nullptr;
    void* peer_open[gicp::kMaxPeers] = {};  // the peers' areas as opened here (closed by gicp_peer_close)
    gicp::PeerArgs peer{};            // n > 1 while the peer exchange is on
    gicp::DevBuf<uint64_t> d_peer_ctr;      // the device's exchange counter (PeerArgs::ctr)
    double peer_timeout_s = 10.0;
    gicp::DevBuf<double> d_probe;
    gicp::DevBuf<double*> d_peer_ptrs;      // device copy of the areas' addresses (PeerArgs::area)
    std::vector<float> iter_ms;       // sampled k_corr time per iteration of the last align (-1: not sampled)
    gicp::DevBuf<double> d_rot;       // gicp_rotated_covariances output
    // gicp_evaluate: the two key arrays [2][N], the per-workgroup sums of the overlap table, the
    // select's state and histograms, the result words and their pinned mirror
    gicp::DevBuf<unsigned long long> d_eval_keys;
    gicp::DevBuf<double> d_eval_part;
    gicp::DevBuf<gicp::SelState> d_eval_sel;
    gicp::DevBuf<uint32_t> d_eval_hist;
    gicp::DevBuf<unsigned long long> d_eval_out;
    gicp::PinnedBuf<unsigned long long> h_eval_out;
    // gicp_align_trace: per-iteration rows recorded on the device ([iter][(d+1)^2 + 1] pose + loss;
    // top-k rows [iter][16] source, target, det), copied out once after the loop
    gicp::DevBuf<double> d_hist;
    gicp::DevBuf<int64_t> d_trace_top;      // [iter][16] source, then [iter][16] target
    gicp::DevBuf<double> d_trace_det;       // [iter][16]
    gicp::DevBuf<unsigned long long> d_tail;     // GICP_TAIL diagnostic build: [iter][kTailWords] (on this context's device)
    gicp::DevBuf<unsigned long long> d_stamps;   // GICP_STAMPS / GICP_TIMELINE diagnostic builds: [wave][20]
    // gicp_batch_align: all clouds' points, the packed offsets / work list / problems / debug row
    // starts, the covariances and counts of every row, the problems' outcomes, the optional debug outputs
    gicp::DevBuf<double> b_xyz, b_dbg_cov, b_dbg_dist;
    gicp::DevBuf<unsigned char> b_meta;
    gicp::DevBuf<double4> b_cov;
    gicp::DevBuf<int32_t> b_cnt;
    gicp::DevBuf<gicp::BatchOut> b_out;
    gicp::DevBuf<int64_t> b_dbg_idx;
    // gicp_knn / gicp_knn_points: the index of an external query set and of a one-shot database
    // (index only: no covariances, no graph), and the answers before they are copied out; all grow-only
    gicp::Cloud knn_q, knn_db;
    gicp::DevBuf<int64_t> knn_idx;
    gicp::DevBuf<double> knn_d2;
    gicp::DevBuf<int32_t> knn_cnt;
    static constexpr int kMaxBatch = 64;
    hipEvent_t ev[2 * kMaxBatch] = {};
    int batch_hint = 0;               // iterations the last converging align ran: its first batch next time
    // diagnostics of the last pass
    double last_amb = 0.0, last_pairs = 0.0, last_sq = 0.0, last_gproved = 0.0, last_walked = 0.0;
    float last_corr_ms = 0.f, last_reduce_ms = 0.f;
    bool timing = false;
};

namespace gicp {

// gicp_build.cpp: cloud builds (synchronous and staged), the voxel filter, the de-skew, the local map
void build_cloud(Cloud& cl, const double* xyz, int64_t n, int dim, const gicp_params& p, BuildScratch& bs,
                 const BuildSpec& spec);
BuildSpec target_spec(const gicp_ctx* c, hipStream_t st);
BuildSpec source_spec(const gicp_ctx* c, int shard, int nshards);
void take_sweep(BuildSpec& spec, const gicp_sweep* sw, int dim);
void copy_covariances(gicp_ctx* c, Cloud& cl, const double* R, double* out);
void copy_points(gicp_ctx* c, Cloud& cl, double* out);
void voxel_downsample(gicp_ctx* c, const double* xyz, int64_t N, int dim, double leaf, int min_points, double* out_xyz,
                      int32_t* out_count, int64_t* M_out);
void filter_points(gicp_ctx* c, const double* xyz, int64_t N, int dim, const gicp_filter& f, double* out_xyz, int64_t* out_index,
                   int32_t* out_count, int64_t* M_out);
void sor_points(gicp_ctx* c, const double* xyz, int64_t N, int dim, const double (&mn)[3], const double (&mx)[3], const gicp_sor& s,
                double* out_xyz, int64_t* out_index, double* out_mean, double* out_stats, int64_t* M_out);
void cluster_points(gicp_ctx* c, const double* xyz, int64_t N, int dim, const double (&mn)[3], const double (&mx)[3],
                    const gicp_cluster& cl, int32_t* labels, int32_t* sizes, int64_t* n_clusters, double* out_xyz, int64_t* out_index,
                    int64_t* M_out);
void deskew_cloud(gicp_ctx* c, const double* xyz, const double* stamps, int64_t N, int dim, const double* xi, double ref,
                  double* out);
void knn_query(gicp_ctx* c, const Cloud* resident, const double* xyz, int64_t M, const double* queries, int64_t Q, int dim,
               int k, double max_distance, int64_t* index, double* dist2, int32_t* count);
void map_insert(gicp_ctx* c, const Cloud* cl, const double* xyz, int64_t n, const double* T);
void map_to_target(gicp_ctx* c, const gicp_params* p, int min_points);
void stage_target(gicp_ctx* c, const double* xyz, int64_t M, int dim, const gicp_params* p, int flags, const gicp_sweep* sw);
void commit_target(gicp_ctx* c, int shard, int nshards);
void cancel_stage(gicp_ctx* c);

// gicp_align.cpp: the per-source-tile state, one pass, the batched loop, the report of a pass
void reset_tile_state(gicp_ctx* c);
void set_shard(gicp_ctx* c, int shard, int nshards);
void top_enqueue(gicp_ctx* c, int k);
void run_pass(gicp_ctx* c, const double* T, gicp_debug* dbg, bool keep_on_device = false);
void evaluate(gicp_ctx* c, const double* T, const gicp_params* p, const gicp_report_spec* spec, gicp_report* out);
void align_trace(gicp_ctx* c, const double* T0, const gicp_params* p, double* T_out, gicp_result* res, gicp_trace* trace);

// gicp_batch.cpp: batched registration
void batch_align(gicp_ctx* c, int dim, const double* xyz, const int64_t* offsets, int n_clouds,
                 const gicp_batch_problem* problems, int n_problems, const gicp_params& prm, double* T_out,
                 gicp_batch_result* res, gicp_batch_debug* dbg);

// gicp_exchange.cpp: the three statistics exchanges (RCCL, host hook, IPC peers); one per context
void drop_comm(gicp_ctx* c);
void close_peers(gicp_ctx* c);
int wall_clock_khz(gicp_ctx* c);
void comm_init(gicp_ctx* c, int nranks, int rank, const char* id);
void comm_ranks(gicp_ctx* c, int* nranks, int* rank, int* kind);
void set_allreduce(gicp_ctx* c, gicp_allreduce_fn fn, void* user, int nranks, int rank);
void peer_export(gicp_ctx* c, char* handle);
void peer_init(gicp_ctx* c, int nranks, int rank, const char* handles, double timeout_s);

}  // namespace gicp
