// gicp_build.cpp — everything that makes a cloud on the device: the build and its front (upload, de-skew, input
// filters, voxel filter), the copies out of a cloud, the local voxel map, and the ring of staged targets with its threads.
#include <rocprim/device/device_radix_sort.hpp>

#include "gicp_host.h"

namespace gicp {
namespace {

struct VoxelOut {
    int64_t M = 0;                  // voxels kept
    double mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};   // bounds of their centroids
};

// The result words (bs.v_res) of what the caller has enqueued on `st`, after the one stream sync of its path:
// callers enqueue their own copies out first.
void read_result_words(BuildScratch& bs, unsigned long long (&res)[kVoxelRes], hipStream_t st) {
    HIPCHK(hipMemcpyAsync(res, bs.v_res, sizeof res, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
}

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
    va.end_bit = voxel_key_bits(dim, mn, mx, leaf, va.cmin, va.bits);
    voxel_scratch(bs, va, true, st);
    va.out_xyz = d_out;
    HIPCHK(launch_voxel(va, st));
    unsigned long long res[kVoxelRes];
    read_result_words(bs, res, st);
    VoxelOut vo;
    vo.M = (int64_t)res[6];
    if (vo.M <= 0) {
        char b[128];
        std::snprintf(b, sizeof b, "voxel filter: none of the %lld voxels holds min_points = %d points", (long long)res[7],
                      min_points);
        throw Fail{GICP_E_INVALID, b};
    }
    decode_bounds(res, dim, vo.mn, vo.mx);
    return vo;
}

struct FilterOut {
    double* pts = nullptr;          // the survivors [M][dim], rows in their order
    const int32_t* idx = nullptr;   // the row of each in the input (tracked; null otherwise)
    int64_t M = 0;
    double mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};   // their exact bounds
};

bool filter_on(const gicp_filter& f) { return filter_crops(f) || f.radius > 0.0; }

// The input filters (gicp_filter.hip) of the device cloud d_in [n][dim] with bounds mn / mx: the
// crop, then radius outlier removal among its survivors.  The last stage in force writes to d_last when given
// (else, as every other stage, to a buffer of the scratch).  track: also the input row of each survivor;
// d_cnt: [n] device, prefilled -1, takes the exact count of every row the crop kept (and makes the count kernel
// count to the end).  One stream sync per stage in force; the result words (bounds, M) are all that returns.
FilterOut filter_stages(BuildScratch& bs, double* d_in, int64_t n, int dim, const double (&mn)[3], const double (&mx)[3],
                        const gicp_filter& f, double* d_last, bool track, int32_t* d_cnt, hipStream_t st) {
    FilterOut fo;
    fo.pts = d_in;
    fo.M = n;
    for (int a = 0; a < 3; ++a) fo.mn[a] = mn[a], fo.mx[a] = mx[a];
    const bool crop = filter_crops(f), ror = f.radius > 0.0;
    if (!crop && !ror) return fo;
    bs.f_keep.reserve((size_t)n);
    bs.f_pos.reserve((size_t)n);
    if (!bs.v_res) bs.v_res.alloc((size_t)kVoxelRes);
    auto dest = [&](int k, bool last) -> double* {
        if (last && d_last) return d_last;
        bs.f_pts[k].reserve((size_t)n * dim);
        return bs.f_pts[k];
    };
    auto index = [&](int k) -> int32_t* {
        if (!track) return nullptr;
        bs.f_idx[k].reserve((size_t)n);
        return bs.f_idx[k];
    };
    unsigned long long res[kVoxelRes];
    if (crop) {
        size_t tmp_bytes = 0;
        HIPCHK(voxel_temp_bytes(n, 1, &tmp_bytes, st));
        bs.v_tmp.reserve(tmp_bytes + 16);
        CropArgs ca{};
        ca.in = d_in;
        ca.n = n;
        ca.dim = dim;
        for (int a = 0; a < 3; ++a) ca.center[a] = a < dim ? f.center[a] : 0.0;
        ca.lo2 = f.min_range * f.min_range;
        ca.hi2 = f.max_range * f.max_range;
        ca.keep = bs.f_keep;
        ca.pos1 = bs.f_pos;
        ca.tmp = bs.v_tmp;
        ca.tmp_bytes = tmp_bytes;
        ca.out = dest(0, !ror);
        ca.idx_out = index(0);
        ca.res = bs.v_res;
        HIPCHK(launch_crop(ca, st));
        read_result_words(bs, res, st);
        fo.M = (int64_t)res[6];
        if (fo.M <= 0) fail_filter_empty(0, n, f);
        decode_bounds(res, dim, fo.mn, fo.mx);
        fo.pts = ca.out;
        fo.idx = ca.idx_out;
    }
    if (ror) {
        const int64_t m = fo.M;
        VoxelArgs va{};
        RorArgs ra{};
        va.raw = fo.pts;
        va.n = m;
        va.dim = dim;
        va.min_points = 1;
        va.end_bit = ror_key_bits(dim, fo.mn, fo.mx, f.radius, va.leaf, va.cmin, va.bits, ra.cmax);
        bs.v_keys.reserve((size_t)m);
        bs.v_keys2.reserve((size_t)m);
        bs.v_idx.reserve((size_t)m);
        bs.v_idx2.reserve((size_t)m);
        bs.f_packed.reserve((size_t)m * dim);
        size_t tmp_bytes = 0;
        HIPCHK(voxel_temp_bytes(m, va.end_bit, &tmp_bytes, st));
        bs.v_tmp.reserve(tmp_bytes + 16);
        va.keys = bs.v_keys;
        va.keys_s = bs.v_keys2;
        va.idx = bs.v_idx;
        va.idx_s = bs.v_idx2;
        va.tmp = bs.v_tmp;
        va.tmp_bytes = tmp_bytes;
        va.res = bs.v_res;
        ra.r2 = f.radius * f.radius;
        ra.min_neighbors = f.min_neighbors;
        ra.full = d_cnt ? 1 : 0;
        ra.packed = bs.f_packed;
        ra.keep = bs.f_keep;
        ra.pos1 = bs.f_pos;
        ra.idx_in = fo.idx;
        ra.cnt_out = d_cnt;
        ra.out = dest(1, true);
        ra.idx_out = index(1);
        HIPCHK(launch_ror(va, ra, st));
        read_result_words(bs, res, st);
        fo.M = (int64_t)res[6];
        if (fo.M <= 0) fail_filter_empty(1, m, f);
        decode_bounds(res, dim, fo.mn, fo.mx);
        fo.pts = ra.out;
        fo.idx = ra.idx_out;
    }
    return fo;
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
    decode_bounds(res, dim, mn, mx);
    // (finite stamps times a finite twist can still overflow; a NaN coordinate decodes as a NaN bound)
    for (int a = 0; a < dim; ++a)
        if (!std::isfinite(mn[a]) || !std::isfinite(mx[a]))
            throw Fail{GICP_E_INVALID, "de-skewed cloud is not finite (stamps too large for the motion)"};
}

// a build begins: the cloud is NOT SET until build_core has finished
void begin_build(Cloud& cl, int dim) {
    cl.unset();
    cl.dim = dim;
    cl.bits = dim == 3 ? 10 : 16;
}

// a build that fails part-way (an unsupported k_neighbors, a HIP error) leaves the cloud NOT SET: cl.n is
// raised by build_index, before the covariances exist, and every entry point tells a usable cloud by cl.n alone
struct Unset {
    Cloud& cl;
    bool done = false;
    ~Unset() {
        if (!done) cl.unset();
    }
};

// The index of a cloud alone: the n points in bs.s_in ([n][dim], device; or in `pts` when given) with bounds
// mn / mx -> Morton sort, tiles, boxes, blocks, rho.  What the searches need of a database or a query set (gicp_knn:
// no covariances, no graph); build_core goes on from here.
void build_index(Cloud& cl, int64_t n, int dim, const double (&mn)[3], const double (&mx)[3], BuildScratch& bs,
                 const BuildSpec& spec, BuildLog& log, const double* pts = nullptr) {
    hipStream_t st = spec.stream;
    const int tile_points = spec.tile_points;
    for (int a = 0; a < 3; ++a) cl.bb_lo[a] = a < dim ? mn[a] : 0.0, cl.bb_hi[a] = a < dim ? mx[a] : 0.0;
    double ext = 0.0;
    for (int a = 0; a < dim; ++a) ext = std::max(ext, mx[a] - mn[a]);
    ext = ext * (1.0 + 1e-9) + 1e-12 * (1.0 + std::fabs(mn[0]));
    for (int a = 0; a < 3; ++a) cl.lo[a] = a < dim ? mn[a] : 0.0;
    cl.scale = std::ldexp(1.0, cl.bits) / ext;

    cl.reserve_points(n);
    bs.s_codes.reserve((size_t)n);
    bs.s_codes2.reserve((size_t)n);
    bs.s_idx.reserve((size_t)n);
    const double* d_in = pts ? pts : bs.s_in.get();
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
    std::vector<int32_t> seed;   // (lives until the stream sync below)
    cl.seed_shift = build_seed_table(tcode, dim * cl.bits, seed);
    cl.seed_tab.reserve(seed.size());
    HIPCHK(hipMemcpyAsync(cl.seed_tab, seed.data(), sizeof(int32_t) * seed.size(), hipMemcpyHostToDevice, st));
    HIPCHK(launch_build_tiles(d_in, dim, cl.perm, cl.tiles, cl.boxes, cl.ntiles, cl.rec, cl.rel32, cl.inv, d_rho, st));
    HIPCHK(launch_build_blocks(cl.tiles, cl.ntiles, cl.blocks, cl.nblocks, dim, st));
    unsigned rho_bits = 0;
    HIPCHK(hipMemcpyAsync(&rho_bits, d_rho, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::memcpy(&cl.rho, &rho_bits, sizeof(float));
    log.tick("tiles");
}

// Statistical outlier removal (gicp_sor.hip) of the device cloud d_in [m][dim] with bounds mn / mx:
// an index-only build of the rows into the scratch's own cloud, the self-query for k + 1 neighbours, the means, the
// two tree sums, the flags, the compaction into d_out (never d_in).  track: also the input row of each
// survivor; stats [3] (nullable): mu, sigma, thr.  The means stay
// in bs.o_mean.  One stream sync beyond the index build's two; the result words and doubles are all that returns.
// The tiling's warm-start hint is put back, so the build that follows starts as it would have.
FilterOut sor_stage(BuildScratch& bs, const double* d_in, int64_t m, int dim, const double (&mn)[3], const double (&mx)[3],
                    const gicp_sor& s, double* d_out, bool track, double* stats, BuildLog& log,
                    hipStream_t st) {
    check_sor_rows(m);
    check_sor_extent(dim, mn, mx);
    Cloud& cl = bs.o_cl;
    {
        const int hint = bs.tile_k_hint[dim & 3];
        BuildLog ilog(st);   // (the index's own phases are not the build's)
        ilog.verbose = false;
        BuildSpec spec;
        spec.stream = st;
        begin_build(cl, dim);
        Unset unset{cl};
        build_index(cl, m, dim, mn, mx, bs, spec, ilog, d_in);
        bs.tile_k_hint[dim & 3] = hint;
        unset.done = true;
    }
    log.tick("sor-index");
    const int kk = s.k + 1;
    bs.o_idx.reserve((size_t)m * kk);
    bs.o_d2.reserve((size_t)m * kk);
    bs.o_cnt.reserve((size_t)m);
    KnnArgs ka{};
    ka.qc = cl.view();
    ka.db = ka.qc;
    ka.self = 1;
    ka.k = kk;
    double diag2 = 0.0;   // d_max of the screen's margin: the diagonal of the bounding box
    for (int a = 0; a < dim; ++a) {
        const double e = cl.bb_hi[a] - cl.bb_lo[a];
        diag2 += e * e;
    }
    ka.mg = make_margin(dim, cl.rho, cl.rho, std::sqrt(diag2) * (1.0 + 1e-9));
    ka.maxd2 = INFINITY;
    ka.search2 = INFINITY;
    ka.index = bs.o_idx;
    ka.dist2 = bs.o_d2;
    ka.count = bs.o_cnt;
    HIPCHK(launch_knn_query(ka, st));
    log.tick("sor-query");
    bs.o_mean.reserve((size_t)m);
    bs.o_part.reserve(sor_part_count(m));
    bs.o_stats.reserve((size_t)kSorStats + 2);
    bs.f_keep.reserve((size_t)m);
    bs.f_pos.reserve((size_t)m);
    if (track) bs.o_rows.reserve((size_t)m);
    if (!bs.v_res) bs.v_res.alloc((size_t)kVoxelRes);
    size_t tmp_bytes = 0;
    HIPCHK(voxel_temp_bytes(m, 1, &tmp_bytes, st));
    bs.v_tmp.reserve(tmp_bytes + 16);
    SorArgs sa{};
    sa.in = d_in;
    sa.n = m;
    sa.dim = dim;
    sa.k = s.k;
    sa.std_ratio = s.std_ratio;
    sa.d2 = bs.o_d2;
    sa.cnt = bs.o_cnt;
    sa.mean = bs.o_mean;
    sa.part = bs.o_part;
    sa.stats = bs.o_stats;
    sa.sums = bs.o_stats.get() + kSorStats;
    sa.keep = bs.f_keep;
    sa.pos1 = bs.f_pos;
    sa.tmp = bs.v_tmp;
    sa.tmp_bytes = tmp_bytes;
    sa.out = d_out;
    sa.idx_out = track ? bs.o_rows.get() : nullptr;
    sa.res = bs.v_res;
    HIPCHK(launch_sor(sa, st));
    double hs[kSorStats];
    unsigned long long res[kVoxelRes];
    HIPCHK(hipMemcpyAsync(hs, bs.o_stats, sizeof hs, hipMemcpyDeviceToHost, st));
    read_result_words(bs, res, st);
    FilterOut fo;
    fo.M = (int64_t)res[6];
    log.tick("sor-reduce");
    check_sor_result(hs[0], fo.M, m, s);
    decode_bounds(res, dim, fo.mn, fo.mx);
    fo.pts = d_out;
    fo.idx = sa.idx_out;
    if (stats)
        for (int a = 0; a < 3; ++a) stats[a] = hs[1 + a];
    return fo;
}

// Euclidean cluster extraction (gicp_cluster.hip) of the device cloud d_in [m][dim] with bounds mn /
// mx: the grid of radius outlier removal at edge c.radius, the components in one pass, labels, sizes and the decision,
// the compaction of the kept clusters' rows into d_out (never d_in).  track: also the input row of each survivor.
// The labels stay in bs.c_labels, the sizes in bs.c_sizes.  One stream sync; the result words (bounds, M, C) are all
// that returns.
FilterOut cluster_stage(BuildScratch& bs, const double* d_in, int64_t m, int dim, const double (&mn)[3], const double (&mx)[3],
                        const gicp_cluster& c, double* d_out, bool track, int64_t* n_clusters, BuildLog& log, hipStream_t st) {
    VoxelArgs va{};
    ClusterArgs ca{};
    va.raw = d_in;
    va.n = m;
    va.dim = dim;
    va.min_points = 1;
    va.end_bit = ror_key_bits(dim, mn, mx, c.radius, va.leaf, va.cmin, va.bits, ca.cmax, "cluster");
    bs.v_keys.reserve((size_t)m);
    bs.v_keys2.reserve((size_t)m);
    bs.v_idx.reserve((size_t)m);
    bs.v_idx2.reserve((size_t)m);
    bs.f_packed.reserve((size_t)m * dim);
    bs.f_keep.reserve((size_t)m);
    bs.f_pos.reserve((size_t)m);
    bs.c_parent.reserve((size_t)m);
    bs.c_size.reserve((size_t)m);
    bs.c_root.reserve((size_t)m);
    bs.c_cid.reserve((size_t)m);
    bs.c_labels.reserve((size_t)m);
    bs.c_sizes.reserve((size_t)m);
    if (track) bs.c_rows.reserve((size_t)m);
    if (!bs.v_res) bs.v_res.alloc((size_t)kVoxelRes);
    size_t tmp_bytes = 0;
    HIPCHK(voxel_temp_bytes(m, va.end_bit, &tmp_bytes, st));
    bs.v_tmp.reserve(tmp_bytes + 16);
    va.keys = bs.v_keys;
    va.keys_s = bs.v_keys2;
    va.idx = bs.v_idx;
    va.idx_s = bs.v_idx2;
    va.tmp = bs.v_tmp;
    va.tmp_bytes = tmp_bytes;
    va.res = bs.v_res;
    ca.r2 = c.radius * c.radius;
    ca.min_size = c.min_size;
    ca.max_size = c.max_size;
    ca.packed = bs.f_packed;
    ca.parent = bs.c_parent;
    ca.size = bs.c_size;
    ca.root = bs.c_root;
    ca.cid1 = bs.c_cid;
    ca.labels = bs.c_labels;
    ca.sizes = bs.c_sizes;
    ca.keep = bs.f_keep;
    ca.pos1 = bs.f_pos;
    ca.out = d_out;
    ca.idx_out = track ? bs.c_rows.get() : nullptr;
    HIPCHK(launch_cluster(va, ca, st));
    unsigned long long res[kVoxelRes];
    read_result_words(bs, res, st);
    log.tick("cluster");
    FilterOut fo;
    fo.M = (int64_t)res[6];
    check_cluster_result(fo.M, m, (int64_t)res[7], c);
    decode_bounds(res, dim, fo.mn, fo.mx);
    fo.pts = d_out;
    fo.idx = ca.idx_out;
    if (n_clusters) *n_clusters = (int64_t)res[7];
    return fo;
}

// The core of a cloud build: the index (build_index), then covariances and (graph) the neighbour graph.
void build_core(Cloud& cl, int64_t n, int dim, const double (&mn)[3], const double (&mx)[3], const gicp_params& p,
                BuildScratch& bs, const BuildSpec& spec, BuildLog& log) {
    hipStream_t st = spec.stream;
    const bool graph = spec.graph;
    Unset unset{cl};
    if (!bs.d_amb)
        alloc_init(bs.d_amb, 4, [&](int32_t* d) { HIPCHK(hipMemsetAsync(d, 0, sizeof(int32_t) * 4, st)); });
    build_index(cl, n, dim, mn, mx, bs, spec, log);

    // surface covariances (gicp.py:19-35), of this rank's tiles when sharded
    const int qb = 0, qe = shard_tile_count(cl.ntiles, spec.cov_shard, spec.cov_nshards);
    cl.eps_a = p.epsilon;   // remembered by the cloud: its records do not store a
    CovArgs ca{};
    ca.cl = cl.view();
    ca.q_begin = qb;
    ca.q_end = qe;
    ca.sh_n = spec.cov_nshards;
    ca.sh_r = spec.cov_shard;
    // (every record's m was marked "not computed" by k_build_tiles: the rows of another shard stay so)
    const double dn = p.max_distance_nearest_neighbors;
    ca.mg = make_margin(dim, cl.rho, cl.rho, dn);
    ca.search2 = screen_bound(ca.mg, dn);
    ca.dn2 = dn * dn;
    ca.eps_a = p.epsilon;
    ca.m_scale = std::sqrt(p.epsilon * (1.0 - p.ratio));
    ca.min_nb = p.min_neighbors;
    ca.rec_out = cl.rec;
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
        ma.lo[a] = map_window_lo(a, ma.t[a], mp.leaf, mp.R);
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
    read_result_words(bs, res, st);
    mp.rows = (int64_t)res[6];
    mp.cur = nb;
}

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
        } catch (...) {
            rc = current_failure(err);
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

// The host front of a cloud build: the bounds and finiteness scan, the upload and (spec.voxel_leaf > 0) the
// voxel filter; build_core does the rest from the device buffer bs.s_in and the bounds.
void build_cloud(Cloud& cl, const double* xyz, int64_t n, int dim, const gicp_params& p, BuildScratch& bs,
                 const BuildSpec& spec) {
    check_cloud_args(xyz, n, dim);
    if (spec.sweep && !spec.stamps) throw Fail{GICP_E_INVALID, "a sweep needs stamps (gicp_sweep.stamps is NULL)"};
    hipStream_t st = spec.stream;
    BuildLog log(st);
    begin_build(cl, dim);
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
        read_result_words(bs, res, st);
        deskew_decode(res, dim, mn, mx);
        log.tick("deskew");
    };
    // (a staged build passes its pinned copy: the H2D copy is then asynchronous)
    const bool sor = spec.sor.k > 0, cluster = spec.cluster.radius > 0.0;
    if (filter_on(spec.filter) || sor || cluster) {
        // upload, de-skew, crop, radius outlier removal, statistical outlier removal, cluster extraction, voxel filter,
        // index: every stage hands the next one its survivors and their exact bounds on the device; the last input
        // filter writes where the index reads
        const bool voxel = spec.voxel_leaf > 0.0;
        bs.v_raw.reserve((size_t)n * dim);
        HIPCHK(hipMemcpyAsync(bs.v_raw, xyz, sizeof(double) * n * dim, hipMemcpyHostToDevice, st));
        log.tick("upload");
        if (spec.sweep) deskew(bs.v_raw);
        FilterOut fo = filter_stages(bs, bs.v_raw, n, dim, mn, mx, spec.filter, voxel || sor || cluster ? nullptr : bs.s_in.get(),
                                     false, nullptr, st);
        log.tick("filter");
        if (sor) {
            const bool more = voxel || cluster;
            if (more) bs.o_pts.reserve((size_t)fo.M * dim);
            fo = sor_stage(bs, fo.pts, fo.M, dim, fo.mn, fo.mx, spec.sor, more ? bs.o_pts.get() : bs.s_in.get(), false, nullptr,
                           log, st);
        }
        if (cluster) {
            if (voxel) bs.c_pts.reserve((size_t)fo.M * dim);
            fo = cluster_stage(bs, fo.pts, fo.M, dim, fo.mn, fo.mx, spec.cluster, voxel ? bs.c_pts.get() : bs.s_in.get(), false,
                               nullptr, log, st);
        }
        n = fo.M;
        for (int a = 0; a < 3; ++a) mn[a] = fo.mn[a], mx[a] = fo.mx[a];
        if (voxel) {
            const VoxelOut vo = voxel_filter(bs, fo.pts, n, dim, mn, mx, spec.voxel_leaf, spec.voxel_min, bs.s_in, st);
            n = vo.M;
            for (int a = 0; a < 3; ++a) mn[a] = vo.mn[a], mx[a] = vo.mx[a];
            log.tick("voxel");
        }
    } else if (spec.voxel_leaf > 0.0) {
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

// a target built on `st` under the context's settings: with the graph unless switched off, through the voxel filter
BuildSpec target_spec(const gicp_ctx* c, hipStream_t st) {
    BuildSpec spec;
    spec.graph = c->use_graph && c->use_certs;
    spec.voxel_leaf = c->voxel_leaf;
    spec.voxel_min = c->voxel_min;
    spec.filter = c->filt;
    spec.sor = c->sor;
    spec.cluster = c->cluster;
    spec.stream = st;
    return spec;
}

// ... and a source on the context's stream: this shard's covariances, the source's tile size, the same filter
BuildSpec source_spec(const gicp_ctx* c, int shard, int nshards) {
    BuildSpec spec;
    spec.cov_shard = shard;
    spec.cov_nshards = nshards;
    spec.tile_points = c->src_tile;
    spec.voxel_leaf = c->voxel_leaf;
    spec.voxel_min = c->voxel_min;
    spec.filter = c->filt;
    spec.sor = c->sor;
    spec.cluster = c->cluster;
    spec.stream = c->stream;
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

// a I - m m^T rotated by R and expanded on the device in original order (k_rotate_cov), then one copy of the
// n x d x d result
void copy_covariances(gicp_ctx* c, Cloud& cl, const double* R, double* out) {
    const int d = cl.dim;
    const size_t m = (size_t)cl.n * d * d;
    c->d_rot.reserve(m);
    HIPCHK(launch_rotate_cov(cl.rec, cl.eps_a, cl.perm, cl.n, d, R, c->d_rot, c->stream));
    HIPCHK(hipMemcpyAsync(out, c->d_rot, sizeof(double) * m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
}

void copy_points(gicp_ctx* c, Cloud& cl, double* out) {
    const size_t m = (size_t)cl.n * cl.dim;
    c->d_rot.reserve(m);
    HIPCHK(launch_points_out(cl.rec, cl.perm, cl.n, cl.dim, c->d_rot, c->stream));
    HIPCHK(hipMemcpyAsync(out, c->d_rot, sizeof(double) * m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
}

void voxel_downsample(gicp_ctx* c, const double* xyz, int64_t N, int dim, double leaf, int min_points, double* out_xyz,
                      int32_t* out_count, int64_t* M_out) {
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
}

// gicp_filter_points: the one-shot of the input filters, host in, host out
void filter_points(gicp_ctx* c, const double* xyz, int64_t N, int dim, const gicp_filter& f, double* out_xyz, int64_t* out_index,
                   int32_t* out_count, int64_t* M_out) {
    double mn[3], mx[3];
    scan_bounds(xyz, N, dim, mn, mx);
    if (!filter_on(f)) {   // the identity
        std::memcpy(out_xyz, xyz, sizeof(double) * N * dim);
        for (int64_t i = 0; i < N; ++i) {
            if (out_index) out_index[i] = i;
            if (out_count) out_count[i] = 0;
        }
        *M_out = N;
        return;
    }
    BuildScratch& bs = c->bs;
    hipStream_t st = c->stream;
    bs.v_raw.reserve((size_t)N * dim);
    HIPCHK(hipMemcpyAsync(bs.v_raw, xyz, sizeof(double) * N * dim, hipMemcpyHostToDevice, st));
    const bool counts = out_count && f.radius > 0.0;
    if (counts) {
        bs.f_cnt.reserve((size_t)N);
        HIPCHK(hipMemsetAsync(bs.f_cnt, 0xFF, sizeof(int32_t) * N, st));   // -1: removed by the crop
    }
    const bool track = out_index || out_count;
    const FilterOut fo = filter_stages(bs, bs.v_raw, N, dim, mn, mx, f, nullptr, track, counts ? bs.f_cnt.get() : nullptr, st);
    std::vector<int32_t> idx(track ? (size_t)fo.M : 0);
    HIPCHK(hipMemcpyAsync(out_xyz, fo.pts, sizeof(double) * fo.M * dim, hipMemcpyDeviceToHost, st));
    if (track) HIPCHK(hipMemcpyAsync(idx.data(), fo.idx, sizeof(int32_t) * fo.M, hipMemcpyDeviceToHost, st));
    if (counts) HIPCHK(hipMemcpyAsync(out_count, bs.f_cnt, sizeof(int32_t) * N, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (out_index)
        for (int64_t m = 0; m < fo.M; ++m) out_index[m] = idx[m];
    if (out_count && !counts) {   // the crop alone: 0 for a kept row, -1 for a removed one
        for (int64_t i = 0; i < N; ++i) out_count[i] = -1;
        for (int64_t m = 0; m < fo.M; ++m) out_count[idx[m]] = 0;
    }
    *M_out = fo.M;
}

// gicp_sor_points: the one-shot of statistical outlier removal, host in, host out; every output may be null
void sor_points(gicp_ctx* c, const double* xyz, int64_t N, int dim, const double (&mn)[3], const double (&mx)[3], const gicp_sor& s,
                double* out_xyz, int64_t* out_index, double* out_mean, double* out_stats, int64_t* M_out) {
    BuildScratch& bs = c->bs;
    hipStream_t st = c->stream;
    bs.v_raw.reserve((size_t)N * dim);
    bs.o_pts.reserve((size_t)N * dim);
    HIPCHK(hipMemcpyAsync(bs.v_raw, xyz, sizeof(double) * N * dim, hipMemcpyHostToDevice, st));
    double stats[3];
    BuildLog log(st);
    log.verbose = false;   // (nothing prints a one-shot's phases: no synchronisation for them)
    const FilterOut fo = sor_stage(bs, bs.v_raw, N, dim, mn, mx, s, bs.o_pts, out_index != nullptr, stats, log, st);
    std::vector<int32_t> idx(out_index ? (size_t)fo.M : 0);
    if (out_xyz) HIPCHK(hipMemcpyAsync(out_xyz, fo.pts, sizeof(double) * fo.M * dim, hipMemcpyDeviceToHost, st));
    if (out_index) HIPCHK(hipMemcpyAsync(idx.data(), fo.idx, sizeof(int32_t) * fo.M, hipMemcpyDeviceToHost, st));
    if (out_mean) HIPCHK(hipMemcpyAsync(out_mean, bs.o_mean, sizeof(double) * N, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (out_index)
        for (int64_t m = 0; m < fo.M; ++m) out_index[m] = idx[m];
    if (out_stats)
        for (int a = 0; a < 3; ++a) out_stats[a] = stats[a];
    *M_out = fo.M;
}

// gicp_cluster_points: the one-shot of Euclidean cluster extraction, host in, host out; every output may be null.
// The stage's synchronisation brings the result words; a decision that keeps no row is refused there, before any
// output is written.
void cluster_points(gicp_ctx* c, const double* xyz, int64_t N, int dim, const double (&mn)[3], const double (&mx)[3],
                    const gicp_cluster& cl, int32_t* labels, int32_t* sizes, int64_t* n_clusters, double* out_xyz, int64_t* out_index,
                    int64_t* M_out) {
    BuildScratch& bs = c->bs;
    hipStream_t st = c->stream;
    bs.v_raw.reserve((size_t)N * dim);
    bs.c_pts.reserve((size_t)N * dim);
    HIPCHK(hipMemcpyAsync(bs.v_raw, xyz, sizeof(double) * N * dim, hipMemcpyHostToDevice, st));
    BuildLog log(st);
    log.verbose = false;   // (nothing prints a one-shot's phases: no synchronisation for them)
    int64_t C = 0;
    const FilterOut fo = cluster_stage(bs, bs.v_raw, N, dim, mn, mx, cl, bs.c_pts, out_index != nullptr, &C, log, st);
    std::vector<int32_t> idx(out_index ? (size_t)fo.M : 0);
    if (labels) HIPCHK(hipMemcpyAsync(labels, bs.c_labels, sizeof(int32_t) * N, hipMemcpyDeviceToHost, st));
    if (sizes) HIPCHK(hipMemcpyAsync(sizes, bs.c_sizes, sizeof(int32_t) * C, hipMemcpyDeviceToHost, st));
    if (out_xyz) HIPCHK(hipMemcpyAsync(out_xyz, fo.pts, sizeof(double) * fo.M * dim, hipMemcpyDeviceToHost, st));
    if (out_index) HIPCHK(hipMemcpyAsync(idx.data(), fo.idx, sizeof(int32_t) * fo.M, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (out_index)
        for (int64_t m = 0; m < fo.M; ++m) out_index[m] = idx[m];
    if (n_clusters) *n_clusters = C;
    if (M_out) *M_out = fo.M;
}

// gicp_knn / gicp_knn_points: the k nearest database rows of every query, host out.  The database
// is the resident cloud, or (resident == nullptr) the M host points xyz, indexed into the context's scratch cloud;
// the queries are the database's own rows (queries == nullptr) or the Q host points `queries`, indexed in their
// own frame into a second scratch cloud.  Index-only builds on the context's stream with its synchronous scratch;
// the tiling's warm-start hint is put back, so a later build of the context's starts as it would have.
// Everything that can refuse (the finiteness scans) comes before the first write.
void knn_query(gicp_ctx* c, const Cloud* resident, const double* xyz, int64_t M, const double* queries, int64_t Q, int dim,
               int k, double max_distance, int64_t* index, double* dist2, int32_t* count) {
    BuildScratch& bs = c->bs;
    hipStream_t st = c->stream;
    double dmn[3], dmx[3], qmn[3], qmx[3];
    if (!resident) scan_bounds(xyz, M, dim, dmn, dmx);
    if (queries) scan_bounds(queries, Q, dim, qmn, qmx);
    auto index_only = [&](Cloud& cl, const double* pts, int64_t n, const double (&mn)[3], const double (&mx)[3]) {
        const int hint = bs.tile_k_hint[dim & 3];
        BuildLog log(st);
        BuildSpec spec;
        spec.stream = st;
        begin_build(cl, dim);
        Unset unset{cl};
        bs.s_in.reserve((size_t)n * dim);
        HIPCHK(hipMemcpyAsync(bs.s_in, pts, sizeof(double) * n * dim, hipMemcpyHostToDevice, st));
        build_index(cl, n, dim, mn, mx, bs, spec, log);
        bs.tile_k_hint[dim & 3] = hint;
        unset.done = true;
    };
    if (!resident) index_only(c->knn_db, xyz, M, dmn, dmx);
    const Cloud& db = resident ? *resident : c->knn_db;
    if (queries) index_only(c->knn_q, queries, Q, qmn, qmx);
    const Cloud& qc = queries ? c->knn_q : db;
    // d_max of the screen's margin: the diagonal of the union of the two clouds' bounding boxes
    double diag2 = 0.0;
    for (int a = 0; a < dim; ++a) {
        const double e = std::max(db.bb_hi[a], qc.bb_hi[a]) - std::min(db.bb_lo[a], qc.bb_lo[a]);
        diag2 += e * e;
    }
    const int64_t nq = qc.n;
    c->knn_idx.reserve((size_t)nq * k);
    c->knn_d2.reserve((size_t)nq * k);
    c->knn_cnt.reserve((size_t)nq);
    KnnArgs ka{};
    ka.qc = qc.view();
    ka.db = db.view();
    ka.self = queries ? 0 : 1;
    ka.k = k;
    // (under a limit no pair further apart than it matters, as d_n bounds k_knn_cov's)
    const bool limited = max_distance > 0.0;
    const double diag = std::sqrt(diag2) * (1.0 + 1e-9);
    ka.mg = make_margin(dim, qc.rho, db.rho, limited ? std::min(diag, max_distance) : diag);
    ka.maxd2 = limited ? max_distance * max_distance : INFINITY;
    ka.search2 = INFINITY;
    if (limited) {
        const float s2 = screen_bound(ka.mg, max_distance);
        if (s2 < 3.0e38f) ka.search2 = s2;   // (a limit beyond the fp32 screen's range limits the exact phase alone)
    }
    ka.index = c->knn_idx;
    ka.dist2 = c->knn_d2;
    ka.count = c->knn_cnt;
    HIPCHK(launch_knn_query(ka, st));
    if (index) HIPCHK(hipMemcpyAsync(index, c->knn_idx, sizeof(int64_t) * nq * k, hipMemcpyDeviceToHost, st));
    if (dist2) HIPCHK(hipMemcpyAsync(dist2, c->knn_d2, sizeof(double) * nq * k, hipMemcpyDeviceToHost, st));
    if (count) HIPCHK(hipMemcpyAsync(count, c->knn_cnt, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
}

// gicp_deskew: the sweep xyz with twist xi, de-skewed on the device into `out` (host)
void deskew_cloud(gicp_ctx* c, const double* xyz, const double* stamps, int64_t N, int dim, const double* xi, double ref,
                  double* out) {
    BuildScratch& bs = c->bs;
    hipStream_t st = c->stream;
    bs.s_in.reserve((size_t)N * dim);
    HIPCHK(hipMemcpyAsync(bs.s_in, xyz, sizeof(double) * N * dim, hipMemcpyHostToDevice, st));
    deskew_launch(bs, bs.s_in, stamps, N, dim, xi, ref, st);
    unsigned long long res[kVoxelRes];
    HIPCHK(hipMemcpyAsync(out, bs.s_in, sizeof(double) * N * dim, hipMemcpyDeviceToHost, st));
    read_result_words(bs, res, st);
    double mn[3], mx[3];
    deskew_decode(res, dim, mn, mx);   // (refuses a result that is not finite)
}

// an insert of the cloud cl (its points go back to their original order on the device) or of the n host points xyz
void map_insert(gicp_ctx* c, const Cloud* cl, const double* xyz, int64_t n, const double* T) {
    VoxelMap& mp = c->map;
    mp.pts.reserve((size_t)n * mp.dim);
    if (cl) HIPCHK(launch_points_out(cl->rec, cl->perm, cl->n, cl->dim, mp.pts, c->stream));
    else HIPCHK(hipMemcpyAsync(mp.pts, xyz, sizeof(double) * n * mp.dim, hipMemcpyHostToDevice, c->stream));
    map_insert_core(mp, c->bs, n, T, c->stream);
}

void map_to_target(gicp_ctx* c, const gicp_params* p, int min_points) {
    VoxelMap& mp = c->map;
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
    read_result_words(bs, res, st);
    const int64_t M = (int64_t)res[6];
    if (M <= 0) {
        char b[128];
        std::snprintf(b, sizeof b, "map: none of the %lld voxels holds min_points = %d points", (long long)m, min_points);
        throw Fail{GICP_E_INVALID, b};
    }
    double mn[3], mx[3];
    decode_bounds(res, dim, mn, mx);
    log.tick("map-centroids");
    c->ptgt = resolve(dim, p);
    c->top_ready = false;
    begin_build(c->tgt, dim);
    build_core(c->tgt, M, dim, mn, mx, c->ptgt, bs, target_spec(c, st), log);   // (the centroids are not filtered again)
    if (c->src.n) reset_tile_state(c);
}

// ---- the ring of staged targets ----

void stage_target(gicp_ctx* c, const double* xyz, int64_t M, int dim, const gicp_params* p, int flags, const gicp_sweep* sw) {
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
}

void commit_target(gicp_ctx* c, int shard, int nshards) {
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
    check_shard(shard, nshards);
    // the current target (index + covariances) becomes the source, as robot-visualization.py:250
    // swaps scans, and the staged cloud the target; the old source's buffers wait in the slot
    if (c->tgt.n) {
        std::swap(c->src, c->tgt);
        c->psrc = c->ptgt;
    }
    std::swap(c->tgt, g.cl);
    g.cl.unset();
    c->ptgt = g.p;
    c->top_ready = false;
    if (c->src.n) set_shard(c, shard, nshards);   // (stream-ordered resets: no host sync)
}

void cancel_stage(gicp_ctx* c) {
    for (auto& g : c->stg) {
        g.wait_idle();
        std::lock_guard<std::mutex> lk(g.m);
        g.state = 0;
        g.xyz = nullptr;
    }
    c->stg_head = c->stg_count = 0;
}

}  // namespace gicp
