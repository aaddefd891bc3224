// gicp_internal.h — device data layout shared by the HIP kernels and the host context.
//
// Every cloud (target and source) is stored Morton-sorted and cut into TILES of at most
// 64 consecutive points that never cross a grid cell of the chosen Morton level, so a
// tile is spatially compact (radius bounded by the cell).  64 consecutive tiles form a
// BLOCK.  Both carry an fp64 centre and fp32 half-extents; points are kept twice:
// fp64 (exact epilogue, fp64 fallback) and fp32 relative to their tile centre (the
// distance screen).  See DESIGN.md §3.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gicp_hip.h"

namespace gicp {

constexpr int kWave = 64;          // CDNA wavefront
constexpr int kTile = 64;          // points per tile (= one wave of queries)
constexpr int kBlockTiles = 64;    // tiles per block (= one wave of tile tests)
constexpr int kWavesPerWG = 4;     // 256-thread workgroups, each wave independent
#ifndef GICP_CORR_WAVES
#define GICP_CORR_WAVES 4
#endif
constexpr int kCorrWaves = GICP_CORR_WAVES;       // waves per k_corr workgroup

constexpr int kListMax = 64;       // candidate target tiles kept per source tile
constexpr int kPoseRing = 64;      // passes a list stays usable for
#ifndef GICP_SUB_TILES
#define GICP_SUB_TILES 4
#endif
// sub-tiles per tile (finer culling of the row scan).  8 (8-row sub-tiles) screens 27-38 % fewer
// rows on the 1M bench but ran 2 % slower: twice the sub-box tests, and the tile metadata no longer
// fits k_corr's scalar registers (44 SGPRs spilled)
constexpr int kSub = GICP_SUB_TILES;
constexpr int kSubRows = 64 / kSub;    // rows per sub-tile (a multiple of 4: the scan's row group)
// target neighbour graph: each target point's kGraphK nearest other target points
constexpr int kGraphK = 20;
#ifndef GICP_GRAPH_HOPS
#define GICP_GRAPH_HOPS 4
#endif
constexpr int kGraphHops = GICP_GRAPH_HOPS;   // descent steps a k_corr lane may take before it walks
// error bound of the descent's fp32 distances, per metre of the coordinates involved (2^-19: the
// relative-to-node arithmetic errs by a few 2^-24 per operation)
constexpr float kGraphErr = 1.9073486328125e-06f;
// graph row layout (DevCloud::nbq / nbx): entries per 128-B line and per first half-line, and the index delta
// that marks an entry whose sorted-index delta does not fit 16 bits
constexpr int kGraphLineA = 15;
constexpr int kGraphHalf = 7;
constexpr int kGraphFar = -32768;
static_assert(2 + 2 * kGraphLineA == 32 && 2 + 2 * kGraphHalf == 16, "header + entries fill the line and its half");
static_assert(2 * (kGraphK - kGraphLineA) == 10, "the remaining entries fill 40 B of the 48-B record");

struct __attribute__((aligned(16))) TileInfo {
    double c[3];      // fp64 centre (midpoint of the fp64 AABB)
    float h[3];       // half-extents: max |rel32| over the tile's points, per axis
    int32_t start;    // first sorted point
    int32_t count;    // 1..64
    float radius;     // max |rel32| norm
    float sc[3][kSub];  // sub-tile box centres (rows kSubRows g ..) relative to c, fp32, axis-major
    float sh[3][kSub];  // sub-tile box half-extents (cover every rel32 of the sub-tile), axis-major
};

// The walk's view of a tile: what k_corr's candidate tests read for every tile of a candidate block (or
// list), 48 B so a wave's 64 records are three coalesced 16-B loads per lane (TileInfo is 144 B apart)
struct __attribute__((aligned(16))) TileBox {
    double c[3];      // = TileInfo::c
    float h[3];       // = TileInfo::h
    int32_t start;    // = TileInfo::start (any n < 2^31)
    int32_t count;    // = TileInfo::count
    int32_t pad;
};
static_assert(sizeof(TileBox) == 48, "TileBox is three 16-B words");

struct __attribute__((aligned(16))) BlockInfo {
    double c[3];
    float h[3];
    int32_t first;    // first tile
    int32_t ntiles;   // 1..64
    float pad;
};

// One point of an indexed cloud: its fp64 position and the m of its covariance C = a I - m m^T, 48 B, so a
// record is three 16-B loads (16-B aligned; two of every three records straddle a 128-B line).  In 2-D z = m2 = 0.
// `a` is not stored: it is the cloud's epsilon (DevCloud::eps_a) for a point with a surface covariance and 1 for
// an isolated one (C = I, m = 0), which m0 marks with kRecIsolated; a row whose covariance was not computed (another
// shard's) has every bit of m set (kRecNotComputed) and decodes as NaN.  Both marks are NaNs, which no computed m0
// is, so "m0 is a NaN" tells a marked row (decode_cov); a surface point with m = 0 (ratio = 1) is not marked.
struct __attribute__((aligned(16))) PointRec {
    double x, y, z;
    double m0, m1, m2;
};
static_assert(sizeof(PointRec) == 48, "a point record is three 16-B words");
constexpr unsigned long long kRecIsolated = 0x7FF8000000000001ull;      // m0 of an isolated point (m1 = m2 = +0)
constexpr unsigned long long kRecNotComputed = 0xFFFFFFFFFFFFFFFFull;   // m0, m1, m2 of a row that was not computed

// Device view of one indexed cloud (all pointers device memory, sorted order).
struct DevCloud {
    const PointRec* rec;      // [n]     x y z m0 m1 m2
    const float4* rel32;      // [n]     x y z 0 relative to the tile centre
    double eps_a;             // the epsilon the cloud was built with: a of every surface covariance
    const int32_t* perm;      // [n]     sorted -> original index
    const TileInfo* tiles;    // [ntiles]
    const BlockInfo* blocks;  // [nblocks] blocks of 64 tiles, then [ceil(nblocks / 64)] super-blocks of 64 blocks
    const uint32_t* tile_code;// [ntiles] Morton code of each tile's first point
    const TileBox* boxes;     // [ntiles] the walk's compact tile records
    // Morton seed lookup: seed_tab[p] = the last tile whose first code <= p << seed_shift (0 if none),
    // p < 2^seed_bits, seed_tab[2^seed_bits] = ntiles - 1: the tile of code c lies in
    // [seed_tab[c >> seed_shift], seed_tab[(c >> seed_shift) + 1]] (a few binary steps instead of log2 ntiles)
    const int32_t* seed_tab;
    int32_t seed_shift;
    // neighbour graph (target only; null when not built), DESIGN.md §3c.  Row i: dword 0 r(i) (fp32: every
    // target t != i with |x_t - x_i| < r is in the row), dword 1 the scale s, then kGraphK entries nearest-first,
    // two dwords each: (x_t - x_i) / s as 3 int16 rounded to nearest (|error| <= s / 2 per axis) and the
    // sorted-index delta t - i as a fourth int16 (kGraphFar when it does not fit: nbi holds it), so a descent
    // step needs no index read.  Entries 0 .. kGraphLineA - 1 fill the 128-B line nbq[i] (its first half holds
    // the header and entries 0 .. kGraphHalf - 1), the rest the 48-B record nbx[i].  An unused entry repeats
    // the last real one (offset and delta 0 in an empty row).  nbi[i][k] = sorted index of entry k (-1 unused).
    const uint4* nbq;         // [n][8]
    const uint4* nbx;         // [n][3]
    const int32_t* nbi;       // [n][kGraphK]
    int64_t n;
    int32_t ntiles;
    int32_t nblocks;
    double lo[3];             // Morton frame: code_a = (x_a - lo_a) * scale
    double scale;
    int32_t bits;             // bits per axis (10 for 3-D, 16 for 2-D)
    int32_t dim;
};

// A record's position alone: one 16-B and one 8-B load, nothing read past z
struct RecPos {
    double x, y, z;
};
__device__ __forceinline__ RecPos rec_pos(const PointRec* r) {
    const double2 xy = *reinterpret_cast<const double2*>(r);
    return RecPos{xy.x, xy.y, r->z};
}
// ... and the whole record as its three 16-B words: (x, y), (z, m0), (m1, m2)
struct RecWords {
    double2 xy, zm, mm;
};
__device__ __forceinline__ RecWords rec_words(const PointRec* r) {
    const double2* const p = reinterpret_cast<const double2*>(r);
    return RecWords{p[0], p[1], p[2]};
}

// (a, m0) of a record's covariance from the words stored (PointRec): the values k_knn_cov computed, bit for bit.
// m1 and m2 are what the record holds.  A marked row's m1 is +0 (isolated: a = 1, m = 0) or a NaN (not computed:
// a and m0 take it, so the row reads NaN as the stored words do).
__device__ __forceinline__ void decode_cov(double eps_a, double m0, double m1, double& a, double& m0d) {
    const bool marked = m0 != m0;
    a = marked ? (m1 != m1 ? m1 : 1.0) : eps_a;
    m0d = marked ? m1 : m0;
}

// Error bound of the fp32 distance screen: |d2_f32 - d2_f64| <= a sqrt(d2) + b + c d2.
struct Margin {
    float a, b, c;
};

struct GraphArgs {
    DevCloud cl;
    int32_t split;            // waves per query tile (1, or kSub: one wave per 16-row sub-tile), see CovArgs
    float search2;            // fp32 screen bound (d_n^2 + margins): the graph's neighbourhood cap
    Margin mg;
    float4* nb;               // [n][kGraphK] scratch: x_t - x_i fp32, t as the w bits
    float2* nbh;              // [n] scratch: (r, count)
    uint4* nbq;               // [n][8] out (packed rows: header and entries 0 .. kGraphLineA - 1)
    uint4* nbx;               // [n][3] out (entries kGraphLineA .. kGraphK - 1)
    int32_t* nbi;             // [n][kGraphK] out
};

struct CovArgs {
    DevCloud cl;
    int32_t q_begin, q_end;   // query tiles, counted within this rank's shard (all tiles when sh_n = 1)
    // source shards (the k_corr split, gicp_internal.h kShardChunk): this rank's query tile t is the cloud's
    // tile ((t / 64) sh_n + sh_r) 64 + t % 64 -- a rank computes the covariances of its own tiles only
    int32_t sh_n, sh_r;
    // waves per query tile: 1 (the tile's 64 points, one per lane), or kSub (one wave per 16-row sub-tile,
    // its box the sub-box: a small cloud -- a 100k stream frame is ~1.7k tiles, a third of one wave per
    // SIMD -- is bound by its longest neighbourhood walk, which the smaller box shortens)
    int32_t split;
    float search2;            // fp32 screen bound (d_n^2 + margins)
    double dn2;               // d_n^2, fp64, strict
    Margin mg;
    double eps_a;             // epsilon (a of C = a I - m m^T)
    double m_scale;           // sqrt(epsilon (1 - ratio))
    int32_t min_nb;           // minimum neighbours for a surface covariance
    PointRec* rec_out;        // [n] sorted: the cloud's records, whose m this kernel writes
    int32_t* count_out;       // [n] sorted
    int32_t* amb_counter;     // diagnostics (may be null)
    float4* g_nb;             // k_knn_cov<D, K, true>: the graph rows (GraphArgs::nb), [n][kGraphK]
    float2* g_nbh;            // ... and (r, count) per point (GraphArgs::nbh)
};

// Device-resident state of the outer loop (gicp.py:106-110,155-167): the pose every pass reads,
// the convergence bookkeeping k_solve updates, and the last pass's statistics.
struct IterState {
    double T[16];             // current pose (d+1)^2 row-major (gicp.py:107,166)
    double loss;              // min_loss of the last inner solve (gicp.py:154)
    double last_loss;         // gicp.py:110,165
    double tol;               // gicp.py:78 tolerance
    int32_t converged;        // 1 once |last_loss - min_loss| < tolerance (gicp.py:160)
    int32_t converged_at;     // iteration index of that test, -1 if none
    int32_t iter;             // outer iterations executed
    int32_t fixed;            // 1: never stop on tolerance (benchmark mode)
    int32_t solve_fail;
    int32_t stop_reason;      // GICP_STOP_*
    // PCL-style criteria (include/gicp_hip.h gicp_params; <= 0 disables), checked after the update
    double trans_eps;         // |dt|^2 <= trans_eps and cos(angle) >= rot_cos of the increment
    double rot_cos;
    double fit_eps;           // |mse - prev_mse| < fit_eps
    double rel_eps;           // |mse - prev_mse| / prev_mse < rel_eps
    double prev_mse;          // +inf before the first pass
    double mse;               // mean squared correspondence distance of the last solved pass
    double pairs_total;       // distance pairs screened, summed over the passes k_solve consumed
    // peer exchange timing (diagnostic, wall-clock ticks of the final workgroup's exchange, this call): in the
    // header, so the host's one upload of the header at the start of a call also clears them
    double xchg_sum, xchg_min, xchg_n;
    double stats[80];         // statistics of the last pass (summed over ranks when a communicator is set)
    double stats_solved[80];  // copy of the statistics the last k_solve consumed (reporting)
};

constexpr int kGroupWG = 64;       // workgroups per first-level reduction group
// grids of at most this many units reduce in one level: the final workgroup sums every unit's partial itself
// (its loads cover 81 units per round trip, k_corr sum_rows), one ticket and one round trip of stores fewer;
// beyond it the one ticket's queue (every unit on one counter) and a third round trip of loads cost more
#ifndef GICP_FLAT_UNITS
#define GICP_FLAT_UNITS 128
#endif
constexpr int kFlatUnits = GICP_FLAT_UNITS;
// Source shards are interleaved in chunks of kShardChunk units (a unit = kCorrWaves source tiles,
// one k_corr workgroup): rank r of G reduces global chunks r, r + G, r + 2G, ...  Contiguous Morton
// ranges left the ranks unbalanced (the registration's far walls are the heavy tiles: one rank of 8
// took 1.7x another's k_corr time), and every rank waits for the slowest at the all-reduce.  A chunk
// of 64 tiles is still one compact region, so an XCD's L2 keeps its locality.
constexpr int kShardChunk = 16;
constexpr int kMaxGroups = 4096;   // ticket counters available
// one 128-B line per ticket counter: agent-scope atomics on one line serialise at the memory side, so tickets
// sharing a line made the groups' last arrivers queue behind each other (625 units: 2.8 us for the group ticket)
constexpr int kTicketStride = 32;

// In-kernel peer exchange of the statistics (include/gicp_hip.h gicp_peer_init).  Each rank
// owns an exchange area in fine-grained (uncached) device memory, mapped into every peer by IPC:
//   uint64 flag[2][kMaxPeers]              sequence number of the launch whose slot last arrived
//   double slot[2][kMaxPeers][kPeerSlot]   rank p's statistics of that launch
// indexed [parity of the exchange's sequence number][sending rank].  The sequence number counts the
// exchanges that actually happen (a launch that exits at once after convergence takes none): it is kept on
// the device (PeerArgs::ctr, the last number this rank wrote flags for) and advanced by the final workgroup
// as it exchanges, so consecutive exchanges always alternate parity.  Two parities then suffice: a rank
// writes exchange s + 1's slot only after its exchange s read every slot of s (stream order), and exchange
// s + 2's only after every rank wrote s + 1's flag, i.e. after every rank finished reading s.  gicp_peer_init
// starts every rank's counter at the maximum over the ranks (carried in the exported handles), so no flag
// left in any area by earlier exchanges (a timed-out one included) can pass for a new one.
constexpr int kMaxPeers = GICP_MAX_PEERS;
constexpr int kPeerSlot = 80;
constexpr int kPeerFlagWords = 2 * kMaxPeers;   // doubles before the slots
constexpr int kPeerProbeRounds = 8;             // full-slot exchanges gicp_peer_init's probe runs (both parities)
constexpr size_t kPeerAreaDoubles = kPeerFlagWords + (size_t)2 * kMaxPeers * kPeerSlot;
struct PeerArgs {
    double* const* area;       // device array [n]: rank p's area as mapped here (area[rank] = this rank's own)
    double* own;               // = area[rank]
    int32_t n;                 // ranks (0: no peer exchange)
    int32_t rank;
    uint64_t* ctr;             // device word: the sequence number of this rank's last exchange (flags written)
    uint64_t timeout;          // wall-clock ticks (wall_clock64) a rank waits for its peers
};

struct CorrArgs {
    DevCloud src, tgt;
    int32_t q_begin, q_end;   // k_corr: q_begin unused (0), q_end = the cloud's tile count
    // source shards (interleaved by kShardChunk units): this rank's unit u is the cloud's unit
    // u + (u / kShardChunk) sh_skip + sh_first, sh_skip = (G - 1) kShardChunk, sh_first = r kShardChunk
    int32_t sh_skip, sh_first;
    // workgroup -> unit map: 0 = XCD stripes (XCD x takes the contiguous eighth x), C > 0 = chunks of C
    // units dealt round-robin to the XCDs (1 = identity)
    int32_t unit_map;
    IterState* state;         // pose in, statistics out
    uint32_t* tickets;        // [(kMaxGroups + 1) kTicketStride] arrival counters (one per line), zero between
                              // launches (self-resetting)
    double* gpart;            // [kMaxGroups][nstat_ext] group partials
    int32_t single_pass;      // 1: run even if state->converged (gicp_iterate)
    float search2;            // fp32 screen bound (d_c^2 + margins)
    float gap_slack;          // rounding slack S of the box tests (search radius + 2 rho_t, x 2^-19)
    double dc;                // d_c, fp64, inclusive (distance > d_c rejects)
    double dc2_max;           // the largest double x with sqrt(x) <= d_c: "sqrt(d2) > d_c" <=> d2 > dc2_max
    Margin mg;
    int32_t* hint;            // [src.ntiles] best target tile of the previous pass
    double* partials;         // [gridDim.x][nstat_ext] workgroup partials
    int64_t* dbg_index;       // [N] original order (nullable)
    double* dbg_weight;       // [N][dim][dim] (nullable)
    double* dbg_dist;         // [N] (nullable)
    double* dbg_det;          // [N] det(W), 0 if rejected, sorted order (nullable; gicp_top_weights)
    int64_t* top_tgt;         // [N] with dbg_det, sorted order: original target index of the correspondence, -1 rejected
    int32_t cov_model;        // GICP_COV_* (include/gicp_hip.h)
    double pl_inv;            // 1 / (epsilon (1 - ratio)): n n^T = m m^T * pl_inv (point-to-plane)
    int32_t count_pairs;      // 1: accumulate evaluated pairs (diagnostic)
    // per-source-tile candidate lists (certified): built by a full walk with the
    // search radius inflated by `skin`, reused while the tile's displacement since the build pose
    // plus the wave's final search radius stays within the certified radius
    int32_t* list;            // [src.ntiles][kListMax] target tiles
    int32_t* list_len;        // [src.ntiles]
    float* list_rcert;        // [src.ntiles] certified radius (0: invalid)
    int32_t* list_pass;       // [src.ntiles] pass the list was built in
    double* poses;            // [kPoseRing][12] pose of each pass (R row-major, t)
    int32_t pass;             // this pass's id (monotonic per source cloud)
    int32_t use_lists;        // 0: always full walk (no lists)
    // a wave with 1 .. sparse_max walking lanes searches lane-parallel, one walking lane at a time (the candidate
    // tiles' rows kSparseGroup tiles per memory round trip) instead of one visit per tile; 0: never
    int32_t sparse_max;
    // a wave with 1 .. sparse_amb lanes the fp32 screen left ambiguous re-resolves them lane-parallel, one at a
    // time (its candidate tiles from the box hierarchy, a tile's rows one per lane, exact fp64), else wave-wide
    // with a walk (GICP_SPARSE_AMB; 0: always wave-wide)
    int32_t sparse_amb;
    float skin;
    // a tile rebuilding its list while the pose still moves uses skin' = min(max(skin, skin_gain x its
    // displacement over the last pass), skin_max): the list then outlasts a step of the same size
    float skin_gain, skin_max;
    // per-source-point nearest-neighbour certificates, sorted source order; null: off
    int32_t* cert_j;          // [src.n] sorted target index of the certified nearest, -1: none within R
    float* cert_gap;          // [src.n] runner-up gap (found) or empty radius R (none), relative to cert_pass
    int32_t* cert_pass;       // [src.ntiles] pass the tile's certificates refer to (-1: none)
    float kappa;              // runner-up gap the walk resolves (m); 0 without certificates
    float empty_r;            // d_c (fp32, rounded up): a lane with no target within R - delta > empty_r stays rejected
    unsigned long long* stamps;  // [waves][16] phase cycles + counters (STAMPS diagnostic build only; else null)
    // 1: the final workgroup also runs the inner solve + pose update (what k_solve does), when no exchange
    // of the statistics between ranks comes between them; `hist` = this iteration's gicp_trace row or null
    int32_t fuse_solve;
    double* hist;
    PeerArgs peer;            // n > 1: the final workgroup exchanges the statistics with its peers in-kernel
    // GICP_TAIL diagnostic build: this launch's tail record ([kTailWords] realtime stamps, 100 MHz), else null
    unsigned long long* tail;
    // robust kernel of the pass (include/gicp_hip.h GICP_ROBUST_*): read by the k_corr<D, true>
    // instantiations only, which launch_corr picks when robust_kernel != 0.  Last in the struct, so every
    // other argument keeps its kernel-argument offset
    int32_t robust_kernel;
    double robust_c, robust_c2;   // robust_scale and its square
};
// GICP_TAIL record of one k_corr launch: [0] workgroup 0's start, [1] the final workgroup's partial stored,
// then the final workgroup: [2] its group ticket won, [3] group sum stored, [4] final ticket won, [5] final
// sum in LDS, [6] peer exchange done, [7] statistics stored, [8] solve done; [9..15] how lanes' searches
// ended (counts over the launch): [9] lanes that descended the target graph, [10..13] lanes the descent proved
// at the start node's local minimum / at a row entry of the start node / after a hop / by an exactly resolved
// near tie, [14] walking lanes, [15] walking waves
constexpr int kTailWords = 16;

// Voxel-grid filter (gicp_voxel.hip): the cell of a point is c_a = floor(x_a / leaf) on an
// absolute grid; its key packs c_a - cmin_a, bits[a] bits per axis, x most significant, so ascending keys are
// the lexicographic order of the cells.  All pointers device memory; the scratch arrays hold n entries.
constexpr int kVoxelRes = 8;       // result words: ordered-integer min[3], max[3] of the kept centroids, M, voxels
struct VoxelArgs {
    const double* raw;        // [n][dim] the unfiltered cloud
    int64_t n;
    int32_t dim;
    int32_t min_points;       // voxels with fewer points are dropped
    double leaf;
    double cmin[3];           // floor(min_a / leaf): the lowest cell per axis
    int32_t bits[3];          // key bits per axis (0 when the axis spans one cell)
    int32_t end_bit;          // bits the sort covers (>= 1)
    uint64_t *keys, *keys_s;  // [n] keys, unsorted and sorted
    int32_t *idx, *idx_s;     // [n] original indices (idx: later the scan of the keep flags)
    int32_t* flag;            // [n] head flags (later the keep flags)
    int32_t* vid1;            // [n] voxel id + 1 of each sorted point
    double* cfirst;           // [ceil(n / 64)][4] per-wave carries: the sum before the wave's first head ...
    double* clast;            // [ceil(n / 64)][4] ... and of its final segment
    int2* cmeta;              // [ceil(n / 64)] (the wave holds a head, voxel of its final segment)
    double* cent;             // [n][3] centroid per voxel
    int32_t* cnt;             // [n] points per voxel
    void* tmp;                // rocPRIM scratch (voxel_temp_bytes)
    size_t tmp_bytes;
    double* out_xyz;          // [M][dim] kept centroids in key order
    int32_t* out_cnt;         // [M] their counts
    unsigned long long* res;  // [kVoxelRes]
};

// Local voxel map (gicp_voxel.hip): rows (cell, coordinate sums, count) of the filter's absolute
// grid in ascending lexicographic order of the cells, kept inside a cube window of 2 R + 1 cells per axis.  One
// insert sorts the map's rows (0 .. m_old - 1) and the posed scan's points (m_old .. m_old + n - 1) together by
// the cell relative to the window's lowest corner, `bits` bits per axis, x most significant; a row outside the
// window takes the key kMapInvalid, which no row inside it can have (2 R + 1 is odd, so the x field of a valid
// key is never all ones; R = 0 sorts on one bit, which only the invalid key sets).
constexpr uint64_t kMapInvalid = ~0ull;
struct MapArgs {
    const int32_t* cells_old; // [m_old][3] the map's rows before the insert
    const double* sums_old;   // [m_old][4] sum x, y, z of the merged points and their number (an exact integer)
    int64_t m_old;
    const double* pts;        // [n][dim] the scan in its original row order, sensor frame
    int64_t n;
    int32_t dim;
    double leaf;
    double R[9], t[3];        // sensor -> world (R[a * 3 + b]; 2-D uses a, b < 2)
    int64_t lo[3];            // the window's lowest cell per axis
    int64_t span;             // 2 R: the highest relative cell
    int32_t bits;             // key bits per axis (0 when R = 0)
    double* vals;             // [m_old + n][4] staged rows: (sx, sy, sz, count) or (x, y, z, 1)
    int32_t* cells_new;       // [rows][3] out
    double* sums_new;         // [m_old + n][4] out (the row after the last valid one takes the dropped rows' sum)
};

// Registration report (gicp_eval.hip): from the per-point outputs a pass left on the device
// (index, distance, weight: original source order) the overlap table and two arrays of 64-bit keys -- the bit
// patterns of dist_i and of the whitened residual s_i, all ones for a rejected row -- then an exact radix select of
// up to kEvalMax ranks per key array, kSelBits bits per round from the top.  All pointers device memory.
constexpr int kEvalMax = GICP_REPORT_MAX;
constexpr int kEvalBlock = 256;                 // rows per workgroup of k_eval_values
constexpr int kSelBits = 8;                     // digit width of the select: 8 rounds over a 64-bit key
constexpr int kSelBins = 1 << kSelBits;
constexpr int kSelRounds = 64 / kSelBits;
constexpr int kSelQueries = 2 * kEvalMax;       // query q: key array q / kEvalMax, rank slot q % kEvalMax
// result words (8 bytes each): inlier counts, their sums of dist^2 (fp64), the selected keys of both arrays
constexpr int kEvalOutCnt = 0, kEvalOutSum = kEvalMax, kEvalOutKey = 2 * kEvalMax, kEvalOutWords = 4 * kEvalMax;
struct SelState {
    unsigned long long prefix[kSelQueries];     // the key bits found so far (the rounds' digits, top first)
    unsigned long long rank[kSelQueries];       // the rank wanted among the keys that carry that prefix
    int32_t slot[kSelQueries];                  // the first query of the same array with the same prefix: its histogram serves
};
struct EvalArgs {
    const int64_t* idx;       // [n] matched target row, -1 rejected (CorrArgs::dbg_index)
    const double* dist;       // [n] (CorrArgs::dbg_dist)
    const double* w;          // [n][dim][dim] (CorrArgs::dbg_weight)
    const PointRec* src_xyz;  // the clouds' sorted point records (DevCloud::rec) ...
    const int32_t* src_inv;   // ... and original -> sorted row
    const PointRec* tgt_xyz;
    const int32_t* tgt_inv;
    int64_t n, m;             // source and target rows
    int32_t dim;
    int32_t nthr, nq;         // thresholds; ranks per key array (0: no keys are written, no select runs)
    double R[9], t[3];        // the pass's pose (R[a * 3 + b]; 2-D uses a, b < 2)
    double thr[kEvalMax];
    unsigned long long rank[kSelQueries];
    unsigned long long* keys; // [2][n]
    double* part;             // [ceil(n / kEvalBlock)][kEvalMax] per-workgroup sums of dist^2
    SelState* sel;
    uint32_t* hist;           // [kSelQueries][kSelBins]
    unsigned long long* out;  // [kEvalOutWords]
};

// Batched registration (gicp_batch.hip): many small cloud pairs in one launch.  All clouds lie
// concatenated in their input order (no index is built: the searches are brute force in LDS), cloud c the rows
// offsets[c] .. offsets[c + 1].  All pointers device memory.
constexpr int kBatchMaxPoints = 2048;   // largest cloud: its fp64 points, with the workgroup's fixed LDS, fit 64 KB
constexpr int kBatchThreads = 256;
constexpr int kBatchRows = 64;          // source rows per chunk of the statistics reduction
struct BatchCovArgs {
    const double* xyz;        // [rows][dim]
    const int64_t* offsets;   // [n_clouds + 1]
    const int2* work;         // [grid] (cloud, first query row within it): kBatchThreads query rows per workgroup
    int32_t cap;              // LDS rows: the largest cloud of the batch
    int32_t min_nb;
    double dn2, eps_a, m_scale;   // as CovArgs
    double4* cov;             // [rows] (a, m0, m1, m2): C = a I - m m^T
    int32_t* count;           // [rows]
    double* dbg_cov;          // [rows][dim][dim] (nullable)
};
// what a problem's workgroup leaves behind
struct BatchOut {
    double T[16];
    double loss, mse;
    int32_t iterations, converged, converged_at, stop_reason, solve_fail, pad;
    double stats[80];         // the statistics its last solve consumed (IterState::stats_solved)
};
struct BatchArgs {
    const double* xyz;
    const int64_t* offsets;
    const double4* cov;
    const gicp_batch_problem* prob;   // [grid]
    const int64_t* row0;      // [grid] first row of the problem in dbg_index / dbg_dist
    int32_t cap;              // LDS rows of the target: the largest target of the batch
    int32_t max_iter, fixed;
    int32_t cov_model, robust_kernel;
    double tol, trans_eps, rot_cos, fit_eps, rel_eps;   // as IterState
    double dc2_max, pl_inv, robust_c, robust_c2;        // as CorrArgs
    BatchOut* out;            // [grid]
    int64_t* dbg_index;       // (nullable)
    double* dbg_dist;         // (nullable)
};

// Exact k-nearest-neighbour queries (gicp_knn.hip): the query cloud qc (indexed in its own frame, or
// the database itself: a self-query) against the database db.  All pointers device memory.
constexpr int kKnnMaxK = 32;
struct KnnArgs {
    DevCloud qc, db;
    int32_t self;             // 1: qc is db (a wave's seed tile is its own tile)
    int32_t k;                // 1 .. K of the instantiation launched
    float search2;            // fp32 screen bound of max_distance (max_distance^2 + margins); +inf: no limit
    double maxd2;             // max_distance^2, fp64, inclusive; +inf: no limit
    Margin mg;
    int64_t* index;           // [Q][k] original database rows, -1 padded; rows in original query order
    double* dist2;            // [Q][k] exact d2, +inf padded
    int32_t* count;           // [Q]
};

constexpr int nstat(int D) {
    return (D * (D + 1) / 2) * (D * (D + 1) / 2) + (D * (D + 1) / 2) * D + (D * (D + 1) / 2) + D * D + D + 2;
}
// partials carry extra diagnostics: ambiguous count, pairs evaluated, list rebuilds, sum |r|^2
// ... and lanes proved by the graph descent, waves that walked (GICP_PASS_INFO)
constexpr int nstat_ext(int D) { return nstat(D) + 6; }
static_assert(nstat_ext(3) <= 80, "IterState::stats holds the extended statistics");

// Each launcher reports hipGetLastError() after its launches.  HIP's last error is per thread and shared
// with every other HIP user on it (torch, RCCL, the caller): one such user's failed call left there must not
// fail this library's launch check, so each launcher clears it first.
inline void clear_foreign_error() { (void)hipGetLastError(); }
// workgroups of 256 threads that cover n rows
inline unsigned grid256(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace gicp
