/*
 * gicp_hip.h — C-ABI of libgicp_hip.so, the MI355X (gfx950) GICP engine.
 *
 * The drop-in boundary for the reference's only public surface,
 *   gicp(source_points, target_points, max_iterations=100, tolerance=1e-6,
 *        max_distance_correspondence=150, max_distance_nearest_neighbors=50)
 *   (/root/reference/python-implementation/gicp.py:78, returns gicp.py:174)
 * and apply_transformation(cloud, T) (gicp.py:176-177).  The Python module
 * generalized-icp_amd/gicp/__init__.py binds these entry points with ctypes
 * and restores the reference's signature and 7-tuple; INTEGRATION.md shows
 * the binding.
 *
 * Conventions
 *   - Host buffers are caller-owned, fp64, row-major (N x dim); device
 *     buffers are library-owned.  No torch / HIP types cross this boundary.
 *   - Every int-returning call returns GICP_OK (0) or a negative GICP_E_*;
 *     gicp_last_error() then describes the failure.  No C++ exception
 *     crosses the boundary.  After GICP_E_HIP / GICP_E_NOMEM from an
 *     allocation the context stays usable and the failed call may be
 *     repeated: a buffer that could not be allocated is left empty, never
 *     half-built, and is allocated again then.
 *   - HIP is initialised lazily inside gicp_create(), never at load time, so
 *     the library is safe to load before fork() (robot-visualization.py:199
 *     runs gicp() in a forked worker).
 *   - One context = one GPU = one host thread; one process per GPU.  Ranks
 *     of a multi-GPU job share the per-iteration statistics through an RCCL
 *     all-reduce (gicp_comm_init) -- or a host reducer (gicp_set_allreduce) --
 *     between the correspondence pass and the pose solve; every rank then runs
 *     the same device solve (k_solve) on bit-identical sums, so no pose
 *     broadcast is needed.
 */
#ifndef GICP_HIP_H
#define GICP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GICP_OK 0
#define GICP_E_INVALID (-1)   /* bad argument (shape, dim, NULL, range) */
#define GICP_E_HIP (-2)       /* HIP runtime failure */
#define GICP_E_STATE (-3)     /* call out of order (e.g. align before set_target) */
#define GICP_E_COMM (-4)      /* RCCL failure */
#define GICP_E_NOMEM (-5)     /* host or device allocation failed */

#define GICP_COMM_ID_BYTES 128
#define GICP_MAX_STATS 74     /* statistics per pass, dim 3 (dim 2: 26); a multi-GPU exchange carries these
                                 plus the GICP_PASS_INFO diagnostics: 80 fp64 (dim 2: 32) */

typedef struct gicp_ctx gicp_ctx;

/* Keyword arguments of gicp() (gicp.py:78) and the constants gicp.py
 * hard-codes (epsilon gicp.py:5, 0.1 ratio gicp.py:11, k = 6 gicp.py:24). */
typedef struct gicp_params {
    int32_t max_iterations;                 /* gicp.py:78, default 100 */
    int32_t k_neighbors;                    /* 0 -> 6 for dim 2 (gicp.py:24), 20 for dim 3 */
    double tolerance;                       /* |delta loss| < tolerance stops, gicp.py:155-162 */
    double max_distance_correspondence;     /* d_c, inclusive (gicp.py:136), default 150 */
    double max_distance_nearest_neighbors;  /* d_n, strict (KDTree distance_upper_bound, gicp.py:24), default 50 */
    double epsilon;                         /* 100 (gicp.py:5) */
    double ratio;                           /* 0.1 (gicp.py:11) */
    int32_t fixed_iterations;               /* 1: never stop on tolerance (benchmark mode) */
    int32_t min_neighbors;                  /* 0 -> dim (2-D: > 1 neighbour, gicp.py:27) */
    int32_t timing_stride;                  /* gicp_align times every n-th correspondence launch with HIP
                                               events (0 -> 8; 1 = every launch, adds queue work;
                                               < 0: no events, corr_kernel_ms 0) ... */
    int32_t timing_offset;                  /* ... starting at launch timing_offset (< stride) */
    /* --- additions beyond gicp.py; zero = the reference's behaviour --- */
    int32_t cov_model;                      /* GICP_COV_* : which covariances weight a correspondence
                                               (presentation/main.typ:446-455) */
    double transformation_epsilon;          /* > 0: PCL-style stop when the iteration's increment has
                                               |dt|^2 <= this and cos(angle) >= rotation threshold
                                               (presentation/main.typ:773-776) */
    double rotation_epsilon;                /* cosine threshold of that test; 0 -> 1 - transformation_epsilon
                                               (PCL's default when its rotation epsilon is unset) */
    double euclidean_fitness_epsilon;       /* > 0: stop when |MSE - previous MSE| < this, MSE = mean squared
                                               correspondence distance of the pass (presentation/main.typ:776) */
    double mse_relative_epsilon;            /* > 0: stop when |MSE - previous| / previous < this (PCL: 1e-5) */
    /* --- robust kernel (M-estimator weights); zero = plain least squares --- */
    int32_t robust_kernel;                  /* GICP_ROBUST_* : per-correspondence weight w of the pass */
    int32_t pad_robust;                     /* explicit padding, ignored */
    double robust_scale;                    /* c of the kernel, in units of the whitened residual
                                               s = sqrt(r^T W r); finite and > 0 unless robust_kernel is 0
                                               (then ignored) */
} gicp_params;

/* gicp_params.robust_kernel.  For an accepted correspondence of a pass at pose T_k, with r = q - (R s + t),
 * W the weight of the pass's cov_model (all three models), e = max(r^T W r, 0), s = sqrt(e) the whitened
 * residual and c = robust_scale, the pass uses W~ = w W wherever it used W: in the statistics A, B, C, gR,
 * gt and c0 (c0 becomes sum w r^T W r, the surrogate the stopping rule watches), in gicp_debug.weight, and
 * in det(W) of gicp_top_weights and the trace's top-k rows.  The correspondence itself (gicp_debug.index
 * stays >= 0 even where GICP_ROBUST_TUKEY gives w = 0), gicp_debug.distance, the count and the sum of
 * |r|^2 (gicp_pass_info out[3], gicp_result.mse, gicp_result.correspondences) are unchanged.  The inner
 * solve minimises sum w_i r_i(T)^T W_i r_i(T) with the weights frozen at T_k: iteratively re-weighted
 * least squares, one re-weighting per outer iteration.  A pass in which every w is 0 (GICP_ROBUST_TUKEY with
 * every residual beyond c) has an identically zero quadratic: gicp_align leaves the pose where it is, with
 * loss 0, and goes on; gicp_solve_pose on such statistics reports GICP_E_INVALID, as for any statistics whose
 * translation block is not positive definite.
 * c is in units of the WHITENED residual: metres for GICP_COV_POINT_TO_POINT (W = I, s = |r|); for
 * GICP_COV_PLANE_TO_PLANE with the reference's epsilon = 100 and ratio = 0.1, about |r . n| / sqrt(20) (two
 * aligned surfaces: the normal direction carries 1 / (2 epsilon ratio)); for GICP_COV_POINT_TO_PLANE,
 * |r . n| (metres along the target normal). */
#define GICP_ROBUST_NONE 0            /* w = 1 (robust_scale ignored) */
#define GICP_ROBUST_HUBER 1           /* w = 1 if s <= c, else c / s */
#define GICP_ROBUST_CAUCHY 2          /* w = 1 / (1 + e / c^2) */
#define GICP_ROBUST_GEMAN_MCCLURE 3   /* w = (c^2 / (c^2 + e))^2 */
#define GICP_ROBUST_TUKEY 4           /* w = (1 - e / c^2)^2 if e < c^2, else 0 */

/* gicp_params.cov_model (the GICP paper's three instances, presentation/main.typ:446-455) */
#define GICP_COV_PLANE_TO_PLANE 0   /* W = inv(R C_s R^T + C_t), both surface covariances (gicp.py:143-145) */
#define GICP_COV_POINT_TO_POINT 1   /* C_s = 0, C_t = I: W = I (standard ICP) */
#define GICP_COV_POINT_TO_PLANE 2   /* C_s = 0, C_t = P^-1: W = n_t n_t^T (projection on the target normal) */

/* gicp_result.stop_reason */
#define GICP_STOP_NONE 0            /* max_iterations reached (or fixed_iterations) */
#define GICP_STOP_LOSS 1            /* |delta loss| < tolerance, gicp.py:160 (the update is NOT applied) */
#define GICP_STOP_TRANSFORM 2       /* transformation_epsilon test (the update IS applied, as PCL does) */
#define GICP_STOP_ABS_MSE 3         /* euclidean_fitness_epsilon test (update applied) */
#define GICP_STOP_REL_MSE 4         /* mse_relative_epsilon test (update applied) */

/* What gicp_align() reports (the reference only prints "Converged at iteration", gicp.py:161). */
typedef struct gicp_result {
    int32_t iterations;        /* outer iterations executed (each = correspondences + solve) */
    int32_t converged;         /* 1 if a stopping criterion ended the loop (which: stop_reason) */
    int32_t converged_at;      /* iteration index printed by gicp.py:161, -1 if none */
    int32_t ambiguous;         /* points re-resolved in fp64 in the last pass (diagnostic) */
    double final_loss;         /* min_loss of the last inner solve */
    int64_t correspondences;   /* accepted correspondences in the last pass, all ranks */
    double wall_ms;            /* host wall time of the iteration loop */
    double corr_kernel_ms;     /* correspondence-kernel time: mean HIP-event duration of the sampled launches
                                  (gicp_params.timing_stride / timing_offset) x iterations executed */
    double reduce_ms;          /* sum of HIP-event durations of partial-reduce + all-reduce */
    int64_t pairs_evaluated;   /* source x target distance evaluations in the last pass (if counted) */
    int32_t stop_reason;       /* GICP_STOP_* */
    int32_t pad;
    double mse;                /* mean squared correspondence distance of the last pass */
    double pairs_total;        /* distance pairs screened over all passes of this call, all ranks */
    double corr_kernel_ms_sampled;  /* sum of the event-timed correspondence launches ... */
    int32_t corr_samples;           /* ... and how many there were */
    int32_t pad2;
    double exchange_us_mean;        /* peer exchange (gicp_peer_init): mean / minimum time the final workgroup spent */
    double exchange_us_min;         /* in the exchange per launch of this call (its stores to every rank's arrival) */
} gicp_result;

/* Optional caller-allocated per-point outputs of one pass, ORIGINAL source
 * order, this rank's shard only (other rows untouched).  Any pointer may be NULL. */
typedef struct gicp_debug {
    int64_t* index;      /* [N] target index of the correspondence, -1 if rejected (gicp.py:136-138) */
    double* weight;      /* [N, dim, dim] W_i = inv(R C_s R^T + C_t), zeros if rejected (gicp.py:143-145);
                            with a robust kernel w_i W_i (GICP_ROBUST_*) */
    double* distance;    /* [N] fp64 distance to the nearest target point (gicp.py:133) */
    int32_t want_top_weights;  /* 1: the pass also keeps det(W) on the device for gicp_top_weights */
} gicp_debug;

/* ---- library ------------------------------------------------------------ */
int gicp_version(void);                          /* 100 * major + minor; 101: gicp_params grew by robust_kernel,
                                                    pad_robust, robust_scale (appended); 102: motion
                                                    compensation (gicp_sweep, gicp_deskew, gicp_*_sweep); 103: the
                                                    registration report (gicp_evaluate, gicp_information,
                                                    gicp_sym_eig); 104: the input filters (gicp_filter,
                                                    gicp_filter_points[_host], gicp_set_filter); 105: batched
                                                    registration (gicp_batch_align, gicp_batch_max_points); 106:
                                                    exact k-nearest-neighbour queries (gicp_knn, gicp_knn_points,
                                                    gicp_knn_host, gicp_knn_max_k); 107: statistical outlier
                                                    removal (gicp_sor, gicp_sor_points[_host], gicp_set_sor,
                                                    gicp_sor_max_k); 108: Euclidean cluster extraction
                                                    (gicp_cluster, gicp_cluster_points[_host], gicp_set_cluster) */
int gicp_stats_size(int dim);                    /* 26 (dim 2) or 74 (dim 3) */
void gicp_default_params(int dim, gicp_params* out);
const char* gicp_strerror(int code);

/* ---- context ------------------------------------------------------------ */
int gicp_create(gicp_ctx** out, int device);     /* lazily initialises HIP on `device` */
void gicp_destroy(gicp_ctx* ctx);
const char* gicp_last_error(const gicp_ctx* ctx);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI ---------------------- */
int gicp_comm_unique_id(char out[GICP_COMM_ID_BYTES]);   /* rank 0, then broadcast out-of-band */
int gicp_comm_init(gicp_ctx* ctx, int nranks, int rank, const char id[GICP_COMM_ID_BYTES]);
/* The exchange this context's statistics go through, read back from the communicator itself
 * (ncclCommCount / ncclCommUserRank): *nranks = 1 and *rank = 0 without one; with a host hook
 * (gicp_set_allreduce_ranks) the values it was given, else 1 / 0; with the peer exchange
 * (gicp_peer_init) its nranks / rank.  *kind: 0 none, 1 RCCL, 2 host hook, 3 peer exchange.  Any
 * output may be NULL. */
int gicp_comm_ranks(gicp_ctx* ctx, int* nranks, int* rank, int* kind);

/* In-kernel peer exchange (replaces the collective on the per-iteration path).  Every rank
 * exports one small exchange area of its own device memory (fine-grained, uncached) as an IPC handle
 * (gicp_peer_export), the handles are all-gathered out of band, and gicp_peer_init maps the peers' areas.
 * From then on the final workgroup of each correspondence launch writes this rank's statistics into its
 * slot of every rank's area, raises the exchange's sequence number there, waits (bounded by `timeout_s`)
 * until every rank's slot of this exchange has arrived in its own area, sums them in rank order -- the
 * same bits on every rank -- and runs the pose solve in the same launch: no collective and no second kernel
 * per iteration.  The sequence number counts the exchanges that happen (launches that exit at once after
 * convergence take none) and lives on the device; an exported handle carries this rank's current number
 * after the 64-byte IPC handle, and gicp_peer_init starts every rank at the maximum, so the ranks agree
 * again after a timed-out exchange.  gicp_peer_init is collective (every rank, same order of calls) and
 * proves the path with one probe exchange before it returns.  It first closes this context's previous peer
 * exchange; on success it replaces RCCL / the host hook, on failure (GICP_E_COMM) the context is left with
 * no peer exchange and its RCCL communicator / hook as they were.  A timed-out exchange inside gicp_align
 * fails the call with GICP_E_COMM.  `handles` holds nranks x GICP_PEER_HANDLE_BYTES bytes in rank order
 * (this rank's entry is not opened).  Ranks of one GPU (several processes) and of several GPUs (xGMI) use
 * the same protocol.  gicp_comm_ranks reports kind 3. */
#define GICP_PEER_HANDLE_BYTES 72
#define GICP_MAX_PEERS 16
int gicp_peer_export(gicp_ctx* ctx, char handle[GICP_PEER_HANDLE_BYTES]);
int gicp_peer_init(gicp_ctx* ctx, int nranks, int rank, const char* handles, double timeout_s);
int gicp_peer_close(gicp_ctx* ctx);   /* back to no exchange (RCCL / hook as set before are dropped by init) */

/* Build provenance of this library: "src=<first 16 hex of sha256 over the sources>;git=<rev>;built=<date
 * time>;arch=gfx950".  The source hash covers csrc/{gicp_index.hip, gicp_cov.hip, gicp_corr.hip, gicp_extras.hip,
 * gicp_capi.cpp, gicp_solver.cpp, gicp_cg.cpp, gicp_hostmath.cpp, gicp_build.cpp, gicp_align.cpp, gicp_exchange.cpp,
 * gicp_voxel.hip, gicp_sweep.hip, gicp_eval.hip, gicp_filter.hip, gicp_batch.hip, gicp_batch.cpp, gicp_knn.hip, gicp_sor.hip,
 * gicp_cluster.hip, gicp_internal.h,
 * gicp_mem.h, gicp_sweep.h, gicp_filter.h, gicp_cov_dev.h, gicp_solver.h, gicp_solve_dev.h, gicp_hostmath.h,
 * gicp_host.h}, include/gicp_hip.h and csrc/{gicp_wave_dev.h, gicp_search_dev.h, gicp_stats_dev.h,
 * gicp_bounds_dev.h, gicp_sor.h, gicp_cluster.h, gicp_runs_dev.h}, concatenated in that order (the Makefile's SRCS, then its HEADERS), so
 * a caller can prove the loaded library was compiled from the sources beside it. */
const char* gicp_build_info(void);

/* ---- clouds -------------------------------------------------------------- */
/* Target cloud (gicp.py:101,104): builds the tile index and the per-point
 * surface covariances once; reusable across gicp_align calls.
 * A failed build leaves no half-built cloud: after gicp_set_target, gicp_set_source or gicp_map_to_target
 * has failed once the build of the cloud began (non-finite coordinates, an unsupported k_neighbors, a HIP
 * error), that cloud is NOT SET -- gicp_cloud_size gives 0, and gicp_iterate, gicp_align,
 * gicp_get_covariances, gicp_get_neighbor_counts and gicp_get_graph report GICP_E_STATE -- until a later
 * build of it succeeds; the other cloud is untouched, and results after the good rebuild are those of a
 * fresh context.  (A call refused for its arguments before the build began leaves the cloud as it was.) */
int gicp_set_target(gicp_ctx* ctx, const double* xyz, int64_t M, int dim, const gicp_params* p);
/* Source cloud (gicp.py:100,111): the whole cloud is uploaded and indexed (its
 * covariance neighbourhoods need every point); this rank reduces only the
 * source tiles of shard `shard` of `nshards`: the cloud's Morton-ordered
 * tiles in chunks of 64, dealt round-robin (chunks shard, shard + nshards, ...;
 * gicp/distributed.py shard_tiles states the same split), and computes the
 * covariances of those tiles only (with nshards > 1, gicp_get_covariances /
 * gicp_rotated_covariances of the source give NaN rows for the other shards'
 * points: merge them across ranks). */
int gicp_set_source(gicp_ctx* ctx, const double* xyz, int64_t N, int dim, const gicp_params* p,
                    int shard, int nshards);
/* Promote the current target (index + covariances) to be the next source,
 * as robot-visualization.py:250 swaps scans; then set a new target. */
int gicp_target_to_source(gicp_ctx* ctx, int shard, int nshards);

/* Pipelined frame stream (robot-visualization.py:239-252): build the NEXT
 * targets -- pinned copy, upload, Morton sort, tiling, covariances, neighbour graph -- each on its own
 * stream from a host thread while the current target is registered (gicp_align on the library's stream
 * runs concurrently).  Up to GICP_MAX_STAGED builds may be pending; commits take them in staging
 * order.  `xyz` is copied into a pinned buffer of the slot before gicp_stage_target returns: the caller may
 * reuse or refill it at once.
 * gicp_commit_target waits for the oldest build, then promotes: current target -> source (as
 * gicp_target_to_source), staged cloud -> target.  gicp_cancel_stage waits for and drops them all. */
#define GICP_MAX_STAGED 2
int gicp_stage_target(gicp_ctx* ctx, const double* xyz, int64_t M, int dim, const gicp_params* p);
/* gicp_stage_target with flags.  GICP_STAGE_BORROW: no copy -- the build reads the caller's `xyz` on its
 * own thread, so the caller must keep that buffer alive and unmodified until the staged target is committed
 * (gicp_commit_target) or dropped (gicp_cancel_stage); for callers that own their frames (a stream held in
 * memory), it saves the ~0.06 ms copy of a 100k frame on the calling thread. */
#define GICP_STAGE_BORROW 1
int gicp_stage_target_ex(gicp_ctx* ctx, const double* xyz, int64_t M, int dim, const gicp_params* p, int flags);
int gicp_commit_target(gicp_ctx* ctx, int shard, int nshards);
int gicp_cancel_stage(gicp_ctx* ctx);

/* Surface covariances C = a I - m m^T of the last set_target/set_source,
 * original order, [n, dim, dim] (gicp.py:104 target_cov_matrices, :111
 * initial_source_cov_matrices).  which: 0 = target, 1 = source. */
int gicp_get_covariances(gicp_ctx* ctx, int which, double* out);
/* The target's neighbour graph (built by gicp_set_target unless GICP_NO_GRAPH=1):
 * index[M][GICP_GRAPH_K] original indices of up to GICP_GRAPH_K other target points (-1 pads),
 * radius[M] such that every target within distance < radius[i] of point i is in row i (0: the
 * row certifies nothing).  Original order.  Either output may be NULL. */
#define GICP_GRAPH_K 20
int gicp_get_graph(gicp_ctx* ctx, int64_t* index, double* radius);
/* Neighbour count (incl. self, < d_n, capped at k) per point, original order. */
int gicp_get_neighbor_counts(gicp_ctx* ctx, int which, int32_t* out);

/* ---- the hot path -------------------------------------------------------- */
/* One pass at pose T ((dim+1)^2, row-major): correspondences + Mahalanobis
 * weights + normal-equation statistics (gicp.py:119-145 plus everything
 * loss()/grad_loss() need, gicp.py:52-76).  `stats` receives
 * gicp_stats_size(dim) doubles, summed over all ranks when a communicator is
 * set.  Layout: see DESIGN.md §4 (A, B, C, gR, gt, c0, count). */
int gicp_iterate(gicp_ctx* ctx, const double* T, double* stats, gicp_debug* dbg);

/* Per-pass diagnostics of the last gicp_iterate / gicp_align pass, summed over ranks:
 * out[0] walking lanes whose fp32 screen was ambiguous, re-resolved in fp64 (a near tie that the graph
 * descent resolves in fp64 from its row counts in out[4], not here), out[1] distance pairs screened,
 * out[2] candidate-list rebuilds, out[3] sum of squared correspondence distances |q - (R s + t)|^2 (PCL's
 * MSE numerator), out[4] points whose nearest target the graph descent proved, out[5] source tiles that
 * walked. */
#define GICP_PASS_INFO 6
int gicp_pass_info(gicp_ctx* ctx, double out[GICP_PASS_INFO]);

/* The drop-in's visualisation extras (gicp.py:169-172) without copying per-point arrays: the k
 * accepted source points of the last gicp_iterate pass with the largest det(W) (W as in
 * gicp_debug.weight; rejected points have det 0), ascending by det as np.argsort(...)[-k:] yields
 * them, ties broken towards the larger original index (the last k of a stable argsort).  Needs a
 * preceding gicp_iterate whose gicp_debug had want_top_weights = 1.  src_out[k]: original source
 * indices; tgt_out[k]: their matched target indices (-1 if rejected); det_out[k]: det(W).  Any
 * output may be NULL.  1 <= k <= 16; slots beyond the shard's point count are -1 / 0.  The pass
 * itself computes the top-k for the k of the previous call (default 5), so that call returns without
 * touching the device; another k costs one more launch and stream sync. */
int gicp_top_weights(gicp_ctx* ctx, int k, int64_t* src_out, int64_t* tgt_out, double* det_out);

/* Host solve of the inner problem (gicp.py:148-154): minimise
 * c0 - 2 g^T dz + dz^T H dz over SE(dim), dz = z(T) - z(T_k), starting at T_k.
 * Pure host code, no GPU needed.  Writes T_out and the minimum. */
int gicp_solve_pose(int dim, const double* stats, const double* T_k, double* T_out, double* loss_out);

/* 2-D inner solve of gicp.py:148-154 as the reference runs it: scipy.optimize.fmin_cg (SciPy 1.15.3:
 * Polak-Ribiere+ CG, gtol 1e-5, maxiter 600, Wolfe line search dcsrch then wolfe2, c1 1e-4, c2 0.4),
 * restated natively (csrc/gicp_cg.cpp), on the closed form of the loss from one pass's 2-D statistics
 * (gicp_iterate's 26 values at pose T_k, 3x3): minimises over the offset x = (tx, ty, theta) from x0
 * (gicp.py:151).  Writes xopt[3], *fopt (gicp.py:153-154; may be NULL) and counts[4] = {nfev, ngev,
 * warnflag, iterations} (may be NULL).  Pure host code, no GPU needed.  Replaces the reference's
 * fmin_cg call at gicp.py:152 (the fast mode's host inner solve). */
int gicp_cg_inner_2d(const double* stats, const double* T_k, const double* x0, double* xopt, double* fopt,
                     int32_t* counts);

/* The whole outer loop (gicp.py:116-167) on the GPU: per iteration the correspondence pass
 * (k_corr), the statistics exchange when sharded, the pose solve + convergence test (k_solve).
 * T0 = NULL starts at the identity; p = NULL means the parameters the source was set with.  The
 * max_distance_correspondence, cov_model, robust_kernel and robust_scale of the last gicp_align stay in
 * force for later gicp_iterate calls, until the next build of the source cloud (gicp_set_source,
 * gicp_target_to_source, gicp_commit_target) brings its own; caches built under the old values change no
 * result.  (A robust_kernel outside GICP_ROBUST_*, or one other than GICP_ROBUST_NONE with a robust_scale
 * that is not finite and > 0, is GICP_E_INVALID here and wherever a gicp_params is taken.) */
int gicp_align(gicp_ctx* ctx, const double* T0, const gicp_params* p, double* T_out, gicp_result* res);

/* What the drop-in's 7-tuple needs from each iteration of that loop (gicp.py:108,121,154,167-172),
 * recorded on the device while it runs and copied out once at the end.  Caller-allocated; row k is
 * iteration k (rows >= gicp_result.iterations are untouched).  Any array may be NULL. */
typedef struct gicp_trace {
    int32_t capacity;   /* rows the arrays hold: >= gicp_params.max_iterations */
    int32_t top_k;      /* 0: no top-k rows; 1..16: the pass's k largest det(W) (gicp_top_weights order) */
    double* poses;      /* [capacity][(dim+1)^2] the pose iteration k's pass ran at (T_k, row-major) */
    double* losses;     /* [capacity] min_loss of iteration k's inner solve (gicp.py:154) */
    int64_t* top_src;   /* [capacity][top_k] original source indices (-1 pads) */
    int64_t* top_tgt;   /* [capacity][top_k] their matched target indices (-1: rejected) */
    double* top_det;    /* [capacity][top_k] det(W) */
} gicp_trace;
/* gicp_align plus the trace (trace = NULL is gicp_align).  With top_k the pass also records det(W)
 * on the device and two small launches per iteration select the rows (gicp.py:170-172); with a
 * shard (nshards > 1) the rows cover this rank's shard only -- merge them across ranks by
 * (det, source index). */
int gicp_align_trace(gicp_ctx* ctx, const double* T0, const gicp_params* p, double* T_out, gicp_result* res,
                     gicp_trace* trace);

/* Drop every pose-dependent cache of the current clouds (candidate lists, nearest-neighbour
 * certificates, last matches, seed tiles): the next pass starts cold, as after a fresh
 * gicp_set_source.  Results never depend on the caches (they are exact); only the time does. */
int gicp_reset_cache(gicp_ctx* ctx);

/* Per-iteration correspondence-kernel time (ms, HIP events) of the last gicp_align: out[i] for
 * iteration i, -1 where that launch was not sampled (gicp_params.timing_stride / timing_offset).
 * Returns the number of iterations written (<= n), or a negative GICP_E_*. */
int gicp_iteration_times(gicp_ctx* ctx, float* out, int n);

/* Host statistics exchange, for a job whose ranks talk over something other than RCCL (e.g. a
 * gloo process group, or ranks sharing one GPU, which RCCL refuses).  When set, every pass
 * copies its statistics (n = gicp_stats_size(dim) + GICP_PASS_INFO doubles) to a host buffer,
 * calls fn(buf, n, user), which must replace buf by the sum over ranks and return 0, and copies
 * the sum back before the pose solve -- in gicp_iterate and inside gicp_align's loop (which then
 * synchronises once per iteration).  Replaces an RCCL communicator on the same context.
 * fn = NULL removes the hook. */
typedef int (*gicp_allreduce_fn)(double* buf, int n, void* user);
int gicp_set_allreduce(gicp_ctx* ctx, gicp_allreduce_fn fn, void* user);
/* gicp_set_allreduce that also records the job's (nranks, rank), which gicp_comm_ranks then reports
 * for the hook (e.g. the device threads of one gicp(devices=[...]) call). */
int gicp_set_allreduce_ranks(gicp_ctx* ctx, gicp_allreduce_fn fn, void* user, int nranks, int rank);

/* The source covariances rotated by R (dim x dim, row-major): R C_s R^T = a I - (R m)(R m)^T per
 * point, computed on the device (gicp.py:120-121 all_source_cov_matrices, rotated instead of
 * recomputed), ORIGINAL order, [n, dim, dim].  which: 0 = target, 1 = source. */
int gicp_rotated_covariances(gicp_ctx* ctx, int which, const double* R, double* out);

/* ---- voxel-grid downsampling -------------------------------------------------------
 * One centroid per occupied cell of an ABSOLUTE grid of edge `leaf`: the cell of a point is
 * floor(x_a / leaf) per axis (fp64, correctly rounded division: NumPy's np.floor(x / leaf) bit for bit),
 * so a voxel is the same region of space in every frame of a stream.  A centroid is the fp64 sum of the
 * cell's points divided by their number; the summation order is a fixed function of the input (no
 * floating-point atomics), so the output is bit-identical from call to call and context to context.
 * Voxels with fewer than min_points points are dropped.  The survivors come in ascending lexicographic
 * order of their cells (c_x, c_y[, c_z]) -- the order of np.unique(cells, axis=0).  The cloud may span at
 * most 2^21 cells per axis in 3-D and 2^31 in 2-D.
 *
 * One-shot, host in, host out: out_xyz [N][dim] and out_count [N] (may be NULL) are caller-allocated for
 * the worst case; *M_out receives the number of voxels kept (their rows come first).  GICP_E_INVALID for
 * a leaf that is not finite or <= 0, min_points < 1, non-finite input, a cell range too wide, and when no
 * voxel reaches min_points. */
int gicp_voxel_downsample(gicp_ctx* ctx, const double* xyz, int64_t N, int dim, double leaf, int min_points,
                          double* out_xyz, int32_t* out_count, int64_t* M_out);
/* Context setting: leaf > 0 filters every later gicp_set_target / gicp_set_source / gicp_stage_target[_ex]
 * cloud on the device, after its upload and before its index is built (only the centroids' bounds and their
 * number return to the host); leaf = 0, the default, is off.  A staged build uses the setting in force when
 * it was staged, on its own stream; GICP_STAGE_BORROW still reads the caller's raw frame in place.  With a
 * sharded source every rank filters the whole cloud (the filter is deterministic: the ranks agree).
 * With a filter set, "original order" and "original index" of a cloud, everywhere in this header
 * (gicp_debug.index, gicp_top_weights, gicp_get_covariances, gicp_get_graph, ...), mean the rows of the
 * FILTERED cloud in the order above; gicp_cloud_size and gicp_get_points return their number and the rows.
 * GICP_E_INVALID for leaf < 0 or not finite, or min_points < 1. */
int gicp_set_voxel(gicp_ctx* ctx, double leaf, int min_points);
int gicp_cloud_size(gicp_ctx* ctx, int which, int64_t* n);      /* points the indexed cloud holds (0: not set) */
int gicp_get_points(gicp_ctx* ctx, int which, double* out);     /* [n][dim], the cloud's original order */

/* ---- motion compensation: de-skewing a sweep -----------------------------------------
 * A SWEEP is a cloud p_i (N x dim, fp64) with one stamp tau_i per point (fp64), a motion M and a reference
 * stamp ref.  M is a (dim+1)^2 row-major rigid transform: the sensor pose one stamp unit later, expressed in
 * the sensor frame now, M = P(tau)^-1 P(tau + 1) for sensor -> world poses P.  Stamps in [0, 1) make M the
 * motion over the sweep, stamps in seconds the motion per second: the library does not care which.  With the
 * twist xi = Log(M) the de-skewed cloud is
 *     p'_i = Exp((tau_i - ref) xi) p_i,
 * the point as seen from the sensor frame at stamp ref, under constant twist.  Twist layout: 3-D
 * (w_x, w_y, w_z, v_x, v_y, v_z), 2-D (w, v_x, v_y).  Per point, with s = tau_i - ref, phi = s w, u = s v:
 * p' = R(phi) p + V(phi) u (Rodrigues' formula and its integral); the coefficients switch to their series
 * below |phi| = 0.1, so the small-angle behaviour is sound ((1 - cos t) / t^2 evaluated naively is 0 at 1e-8).
 * xi is computed once on the host in fp64, the per-point map runs in fp64, and the same function
 * (csrc/gicp_sweep.h) serves the device kernel and gicp_deskew_host.  Rows keep their order: "original order"
 * and "original index" mean what they mean without a sweep.  s = 0 or xi = 0 returns the input.  The last row
 * of M is not read.
 * GICP_E_INVALID for: a non-finite M, ref, stamp or coordinate; max|R^T R - I| > 1e-9 or det R <= 0; a rotation
 * of more than a quarter turn per stamp unit ((tr R - 1) / 2 < 0 in 3-D, R_00 < 0 in 2-D: no constant-velocity
 * sweep, and Log stays well conditioned); stamps == NULL; a de-skewed cloud that is not finite.
 *
 * gicp_motion_twist and gicp_deskew_host are host only, as gicp_solve_pose: no HIP call, no context.
 * gicp_deskew is the one-shot on the device, host in, host out (out [N][dim] caller-allocated; the context's
 * clouds are untouched).  Its output is bit-identical from call to call and context to context, and to the
 * rows a build with the same sweep indexes.
 * The *_sweep builds are gicp_set_target, gicp_set_source and gicp_stage_target_ex with a sweep (sweep = NULL:
 * exactly those calls): the cloud is de-skewed on the device after its upload, before the voxel filter (if
 * set) and the index, which take the device's exact bounds of the de-skewed points (one more stream
 * synchronisation).  Only the scan and its stamps cross to the device.  gicp_get_points returns the de-skewed
 * rows (with a filter: their centroids), and gicp_map_insert of the cloud merges them.  A sharded source
 * de-skews the whole cloud on every rank.  gicp_stage_target_sweep copies the stamps with the points; with
 * GICP_STAGE_BORROW it reads them in place, under the same lifetime rule.  A sweep refused once the build has
 * begun (a non-finite stamp, a motion that is not rigid) leaves that cloud NOT SET, as any failed build. */
typedef struct gicp_sweep {
    const double* stamps;   /* [N], one per point */
    double ref;             /* reference stamp: the de-skewed points are in the sensor frame at this stamp */
    double motion[16];      /* M, (dim+1)^2 values used */
} gicp_sweep;
int gicp_motion_twist(int dim, const double* M, double* xi);   /* xi[6] (3-D) or xi[3] (2-D) = Log(M), and the checks */
int gicp_deskew_host(const double* xyz, const double* stamps, int64_t N, int dim, const double* M, double ref,
                     double* out);
int gicp_deskew(gicp_ctx* ctx, const double* xyz, const double* stamps, int64_t N, int dim, const double* M,
                double ref, double* out);
int gicp_set_target_sweep(gicp_ctx* ctx, const double* xyz, int64_t M, int dim, const gicp_params* p,
                          const gicp_sweep* sweep);
int gicp_set_source_sweep(gicp_ctx* ctx, const double* xyz, int64_t N, int dim, const gicp_params* p, int shard,
                          int nshards, const gicp_sweep* sweep);
int gicp_stage_target_sweep(gicp_ctx* ctx, const double* xyz, int64_t M, int dim, const gicp_params* p, int flags,
                            const gicp_sweep* sweep);

/* ---- input filters: range crop and radius outlier removal -----------------------------
 * What a LiDAR front end runs before registration, on the device.  Two stages, in this order:
 *   1. CROP.  Keep p iff d2(p, center) >= min_range * min_range (min_range > 0) and d2(p, center) <=
 *      max_range * max_range (max_range > 0); a range of 0 sets no limit.
 *   2. RADIUS OUTLIER REMOVAL among the crop's survivors only.  For survivor i,
 *      count_i = #{ j != i, j a survivor : d2(p_i, p_j) <= radius * radius } -- the bound is inclusive, as d_c
 *      is, and coincident other rows count -- and i is kept iff count_i >= min_neighbors.  One pass, not iterated.
 * All arithmetic is fp64 and every product and every sum is rounded on its own (no FMA):
 *   d2(a, b) = ((dx * dx + dy * dy) + dz * dz),  dx = a_x - b_x,  the z term dropped in 2-D,
 * the same bits in either direction, and the bits NumPy's expression gives.  The same functions
 * (csrc/gicp_filter.h) serve the device kernels and gicp_filter_points_host.  Survivors keep their original
 * relative order.  A filter with every field 0 is the identity.  No floating-point atomics: the output is
 * bit-identical from call to call and context to context.
 * GICP_E_INVALID for: a non-finite field; a negative range or radius; min_range > max_range with max_range > 0;
 * min_neighbors < 1 with radius > 0; non-finite input; a stage that leaves no row (the message names the stage);
 * a cropped cloud that spans more than 2^21 (3-D) or 2^31 (2-D) cells of edge `radius` on an axis (the message
 * names the axis and suggests a max_range) or lies beyond 2^35 such cells from the origin.
 *
 * One-shot, host in, host out: out_xyz [N][dim], out_index [N] (may be NULL) and out_count [N] (may be NULL) are
 * caller-allocated; *M_out receives the number of rows kept (they come first).  out_index: the original row of
 * each kept row, ascending.  out_count, per INPUT row: the exact count_i, -1 where the crop removed the row (0
 * for every kept row when radius is 0).  With out_count == NULL a point stops counting at min_neighbors; the
 * kept set is the same.  The context's clouds and its gicp_set_filter setting are untouched.
 * gicp_filter_points_host is host only, as gicp_deskew_host: no HIP call, no context -- a plain cell-bucketed
 * loop, the CPU yardstick, not a fast path.  Its message is gicp_last_host_error()'s (per thread).
 *
 * Context setting (gicp_set_filter; NULL or all-zero: off, the default): filters every later gicp_set_target /
 * gicp_set_source / gicp_stage_target[_ex] cloud and their *_sweep forms on the device -- after the upload and
 * the de-skew, so `center` is in the de-skewed sensor frame, and before the voxel filter (if set) and the index,
 * which take the device's exact bounds of the survivors (one stream synchronisation per stage in force; only
 * result words return to the host).  A staged build uses the setting in force when it was staged, on its own
 * stream; GICP_STAGE_BORROW still reads the caller's raw frame in place.  With a sharded source every rank
 * filters the whole cloud.  With a filter set, "original order" and "original index" of a cloud, everywhere in
 * this header, mean the rows of the FILTERED cloud; gicp_cloud_size and gicp_get_points return their number and
 * the rows.  A filter that fails after the build began (no survivor, a grid too wide) leaves that cloud NOT
 * SET, as any failed build. */
typedef struct gicp_filter {
    double center[3];      /* crop centre, in the frame of the cloud (the sensor origin; 2-D uses two) */
    double min_range;      /* >= 0; keep d2(p, c) >= min_range * min_range   (0: no lower limit) */
    double max_range;      /* >= 0; keep d2(p, c) <= max_range * max_range   (0: no upper limit) */
    double radius;         /* > 0: radius outlier removal on the cropped cloud; 0: off */
    int32_t min_neighbors; /* >= 1 when radius > 0 */
    int32_t pad;
} gicp_filter;
int gicp_filter_points(gicp_ctx* ctx, const double* xyz, int64_t N, int dim, const gicp_filter* f, double* out_xyz,
                       int64_t* out_index, int32_t* out_count, int64_t* M_out);
int gicp_filter_points_host(const double* xyz, int64_t N, int dim, const gicp_filter* f, double* out_xyz,
                            int64_t* out_index, int32_t* out_count, int64_t* M_out);
const char* gicp_last_host_error(void);   /* of this thread's last failed gicp_filter_points_host, gicp_knn_host, gicp_sor_points_host or gicp_cluster_points_host, or refused gicp_batch_align ("" if none) */
int gicp_set_filter(gicp_ctx* ctx, const gicp_filter* f);

/* ---- local voxel map ----------------------------------------------------------------
 * A device-resident set of voxels of the same absolute grid as the filter above, in the WORLD frame: each
 * holds its integer cell (int32 per axis), the fp64 sums of the coordinates of every point ever merged into
 * it, and their int32 number; its centroid is sum / count (one correctly rounded division), computed when
 * the map is read or made the target.  The map lives inside a cube window of |cell_a - c_a| <= R cells per
 * axis, R = ceil(max_range / leaf), re-centred by every insert.
 *
 * An insert takes T = sensor -> world, (dim+1)^2 row-major, and
 *   1. moves every point to the world frame as ((R_a0 x + R_a1 y) + R_a2 z) + t_a, each product and sum
 *      rounded on its own (no FMA; the z term is dropped in 2-D), so NumPy's
 *      R[a,0]*x + R[a,1]*y + R[a,2]*z + t[a] gives the same bits;
 *   2. re-centres the window on the cell c = floor(t_a / leaf): voxels outside it are dropped and forgotten
 *      (a region entered again starts from count 0), new points outside it are discarded;
 *   3. merges the new points into the voxels inside it: a voxel's new sum is its stored sum first, then its
 *      new points in the scan's row order, added in a tree that depends on their sorted positions alone (no
 *      floating-point atomics: the same inserts give the same bits on every call, context and GPU);
 *   4. keeps the rows in ascending lexicographic order of their cells.
 * One stream synchronisation per insert; only a few result words return to the host.
 *
 * gicp_map_reset creates or empties the map.  GICP_E_INVALID for a dim other than 2 or 3, a leaf or
 * max_range that is not finite and > 0, and a window of more than 2^21 (3-D) / 2^31 (2-D) cells per axis.
 * gicp_map_insert merges the context's target (which = 0) or source (1) cloud as it is indexed -- with
 * gicp_set_voxel in force, the filtered cloud -- without host traffic; gicp_map_insert_points a host cloud.
 * GICP_E_STATE before gicp_map_reset or for a cloud that is not set; GICP_E_INVALID for a T or points that are
 * not finite, a dimension other than the map's, and a window that would leave the int32 cell range
 * (|c_a| + R >= 2^31; the message names the axis).
 * gicp_map_get copies the rows out in key order: cells [rows][dim], centroids [rows][dim], counts [rows];
 * any may be NULL.
 * gicp_map_to_target makes the centroids of the voxels holding >= min_points points, in key order, the
 * target cloud (index, covariances and graph built as by gicp_set_target, no host copy of the points).  It
 * leaves the source and any staged targets alone and resets the pose-dependent caches.  GICP_E_INVALID for
 * min_points < 1, an empty map, and when no voxel reaches min_points (the target is then unchanged). */
int gicp_map_reset(gicp_ctx* ctx, int dim, double leaf, double max_range);
int gicp_map_insert(gicp_ctx* ctx, int which, const double* T);
int gicp_map_insert_points(gicp_ctx* ctx, const double* xyz, int64_t n, int dim, const double* T);
int gicp_map_size(gicp_ctx* ctx, int64_t* rows);                /* 0 before gicp_map_reset */
int gicp_map_get(gicp_ctx* ctx, int32_t* cells, double* centroids, int32_t* counts);
int gicp_map_to_target(gicp_ctx* ctx, const gicp_params* p, int min_points);

/* ---- registration report -------------------------------------------------------------
 * One pass at pose T and, from it, what a consumer needs to judge the registration; no per-point array
 * reaches the host.  The pass accepts a set of source points; for each accepted point i
 *     p_i = R s_i + t,  q_i its match,  r_i = q_i - p_i,
 *     W~_i the weight the pass used (cov_model and robust kernel in force: exactly gicp_debug.weight),
 *     dist_i = gicp_debug.distance.
 *
 * Information matrix.  Left perturbation T' = Exp(xi) T, twist layout as gicp_sweep: 3-D
 * (w_x, w_y, w_z, v_x, v_y, v_z), 2-D (w, v_x, v_y).  J_i = d r_i / d xi = [ [p_i]x , -I ] (2-D:
 * [ -J2 p_i , -I ], J2 = [[0,-1],[1,0]]), H = sum J_i^T W~_i J_i, b = sum J_i^T W~_i r_i; the Gauss-Newton step
 * is -H^-1 b and the frozen-weight loss is c0 + 2 b^T xi + xi^T H xi to second order.  Both follow from the pass's
 * statistics with no per-point work: with H_z, g of DESIGN.md §4 and dz = G xi (dR = [w]x R, dt = w x t + v),
 * H = G^T H_z G and b = -G^T g (gicp_information).  n = 6 (3-D) or 3 (2-D); H is n x n row-major.
 *
 * Degeneracy.  Eigenvalues ascending and eigenvectors (columns, n x n row-major) of three matrices: H (mixed
 * units: radians and metres), its rotation block H_ww (3 x 3; 2-D: 1 x 1) and its translation block H_vv (dim x
 * dim).  All three are defined for a singular H too (no Schur complement is taken).  gicp_sym_eig is a cyclic
 * Jacobi iteration in fp64 on (A + A^T) / 2.
 *
 * Overlap table.  Up to GICP_REPORT_MAX thresholds tau_j, each finite with 0 <= tau_j <= d_c of the pass (the
 * search is exact only up to d_c): inliers[j] = #{i accepted : dist_i <= tau_j} (inclusive, as d_c is) and
 * inlier_sum_sq[j] = sum of dist_i^2 over them.  Fitness is inliers[j] / n_source, the inlier RMSE
 * sqrt(inlier_sum_sq[j] / inliers[j]).  The sums are added in an order fixed by the cloud's size (no
 * floating-point atomics): bit-identical from call to call and from context to context.
 *
 * Quantiles.  Up to GICP_REPORT_MAX probabilities pi_j in [0, 1]; the statistic is the lower order statistic:
 * of the n accepted values sorted ascending the one at index floor(pi_j (n - 1)), the product in fp64
 * (np.quantile(v, pi, method="lower")), exact, of two value sets: dist_q of the distances dist_i, white_q of the
 * whitened residuals s_i = sqrt(max(r_i^T W~_i r_i, 0)) -- the unit of robust_scale when the pass runs with
 * GICP_ROBUST_NONE.  With n = 0 every quantile is NaN, the counts are 0 and H, b and the eigenvalues are 0:
 * not an error.
 *
 * gicp_evaluate: T = NULL is the identity; p = NULL means the values in force; otherwise p's
 * max_distance_correspondence, cov_model, robust_kernel and robust_scale are used FOR THIS PASS ALONE and the
 * values in force are restored afterwards (unlike gicp_align, whose values stay).  spec = NULL: no thresholds,
 * no quantiles.  It counts as a pass (gicp_pass_info describes it) and uses and updates the pose-dependent
 * caches as gicp_iterate does; they change no result.  One stream synchronisation more than gicp_iterate.
 * GICP_E_STATE: clouds not set, a sharded source (nshards > 1), or a communicator, host hook or peer exchange
 * set (quantiles do not sum over ranks).  GICP_E_INVALID: a non-finite T, a count < 0 or > GICP_REPORT_MAX, a
 * threshold or probability out of range, out == NULL.
 * gicp_information and gicp_sym_eig are host only, as gicp_solve_pose: no HIP call, no context.  gicp_evaluate
 * calls exactly these two on the pass's statistics. */
#define GICP_REPORT_MAX 8
typedef struct gicp_report_spec {
    int32_t n_thresholds, n_quantiles;
    double thresholds[GICP_REPORT_MAX];
    double quantiles[GICP_REPORT_MAX];
} gicp_report_spec;
typedef struct gicp_report {
    int32_t dim;               /* 2 or 3; n = 3 or 6 below */
    int32_t n_thresholds, n_quantiles;   /* as asked */
    int32_t pad;
    int64_t n_source;          /* rows of the source cloud */
    int64_t n_matched;         /* accepted correspondences: the statistics' count */
    double sum_sq;             /* sum |r_i|^2 (gicp_pass_info out[3]) */
    double loss;               /* c0 = sum r_i^T W~_i r_i */
    double H[36], b[6];        /* n x n row-major, n */
    double eig[6], eigvec[36]; /* of H: ascending; eigvec[i * n + k] = component i of eigenvector k */
    double eig_rot[3], vec_rot[9];       /* of H_ww (3 x 3; 2-D: 1 x 1) */
    double eig_trans[3], vec_trans[9];   /* of H_vv (dim x dim) */
    int64_t inliers[GICP_REPORT_MAX];
    double inlier_sum_sq[GICP_REPORT_MAX];
    double dist_q[GICP_REPORT_MAX], white_q[GICP_REPORT_MAX];
} gicp_report;
int gicp_evaluate(gicp_ctx* ctx, const double* T, const gicp_params* p, const gicp_report_spec* spec,
                  gicp_report* out);
/* H [n][n] and b [n] from `stats` (gicp_iterate's output at pose T, (dim+1)^2 row-major) */
int gicp_information(int dim, const double* stats, const double* T, double* H, double* b);
/* A [n][n] row-major, 1 <= n <= 6 (only (A + A^T) / 2 is used) -> w[n] ascending, V[n][n] with column k the
 * unit eigenvector of w[k].  GICP_E_INVALID for n out of range, a NULL pointer or a non-finite entry. */
int gicp_sym_eig(int n, const double* A, double* w_ascending, double* V_columns_row_major);

/* ---- batched registration: many small cloud pairs in one launch ----
 * A particle filter, a multi-start search over yaw, a fleet, loop-closure candidates: hundreds of registrations
 * of clouds of a few hundred points each.  One such pair keeps a few wavefronts busy and a gicp_align call is
 * launch and synchronisation latency; gicp_batch_align runs ONE workgroup per problem, persistent over the
 * problem's whole outer loop (nearest neighbours by exact fp64 brute force over the target held in LDS, the
 * statistics reduced in a fixed order, the pose solve and the stopping rules of gicp_align on the device), so a
 * batch costs two launches and one synchronisation however many problems it holds.
 *
 * Clouds: `xyz` holds all clouds concatenated, [offsets[n_clouds]][dim]; cloud c is rows offsets[c] ..
 * offsets[c + 1] (offsets[0] = 0), of 1 .. gicp_batch_max_points(dim) points.  Many problems may name the same
 * cloud: a multi-start search is one pair with n_problems different T0.  One gicp_params serves the whole batch
 * (NULL: the defaults of `dim`); k_neighbors, max_distance_nearest_neighbors, epsilon, ratio and min_neighbors give
 * the surface covariances of every cloud (computed once per cloud, the semantics of gicp_set_target's), the rest
 * is gicp_align's.  The context's voxel and filter settings (gicp_set_voxel, gicp_set_filter) do NOT apply to
 * batch clouds: they are registered as given.
 *
 * A problem's outputs depend on its two clouds, its T0 and the parameters alone: the same bits whatever else is
 * in the batch, at any position, batch size, call history or context.  Correspondences are exact: the nearest
 * target by d2 = ((dx*dx + dy*dy) + dz*dz), every operation rounded on its own, equal distances to the lower
 * row, accepted iff sqrt(d2) <= max_distance_correspondence.
 *
 * GICP_E_INVALID, before anything runs, with the outputs untouched and a message that names the cloud or
 * problem (gicp_last_error, and gicp_last_host_error for this thread): a dim other than 2 or 3; n_clouds < 1 or
 * n_problems < 1; a NULL xyz, offsets, problems or T_out; offsets that do not start at 0 or do not ascend; an
 * empty or oversized cloud; a cloud number out of range; non-finite points or T0; the parameter errors
 * gicp_align and gicp_set_target refuse (cov_model, robust kernel and scale, k_neighbors).  These checks come
 * before the context is looked at, so they need no GPU; a NULL context is GICP_E_INVALID after them.
 * A problem whose pose solve fails, or whose last pass accepted no correspondence, does not fail the call: it
 * reports status GICP_E_INVALID, keeps the pose it had (T0 when its first solve failed), and the others are
 * unaffected.  A GICP_ROBUST_TUKEY pass that gives every
 * correspondence weight 0 is no failure (gicp_align's rule).
 *
 * The call runs on the context's stream and leaves the context's clouds, voxel map, caches, settings and
 * statistics exchange exactly as they were; its device buffers are the context's own (grow-only). */
typedef struct gicp_batch_problem {
    int32_t source, target;    /* cloud numbers */
    double T0[16];             /* the start pose, (dim+1)^2 row-major in the first entries */
} gicp_batch_problem;
typedef struct gicp_batch_result {
    int32_t status;            /* GICP_OK, or GICP_E_INVALID: this problem's pose solve failed (degenerate
                                  statistics, e.g. no correspondence) */
    int32_t iterations, converged, converged_at, stop_reason, pad;   /* as gicp_result */
    int64_t correspondences;
    double final_loss, mse;    /* as gicp_result */
} gicp_batch_result;
typedef struct gicp_batch_debug {        /* all optional, caller-allocated */
    double* covariances;       /* [rows of all clouds][dim][dim], cloud after cloud, input order */
    int32_t* neighbor_counts;  /* [rows of all clouds] */
    int64_t* index;            /* per problem, its source's rows: target row within its target cloud, -1 rejected;
                                  problem b starts at the sum of the source sizes of problems < b */
    double* distance;          /* same layout: distance to the nearest target row (accepted or not) */
    double* stats;             /* [n_problems][GICP_MAX_STATS], the first gicp_stats_size(dim) used: the last pass
                                  each problem ran */
} gicp_batch_debug;
int gicp_batch_max_points(int dim);   /* largest cloud a batch takes (2048); GICP_E_INVALID for a dim other than 2, 3 */
int gicp_batch_align(gicp_ctx* ctx, int dim, const double* xyz, const int64_t* offsets, int n_clouds,
                     const gicp_batch_problem* problems, int n_problems, const gicp_params* p,
                     double* T_out /* [n_problems][(dim+1)^2] */, gicp_batch_result* res /* [n_problems], may be NULL */,
                     gicp_batch_debug* dbg /* may be NULL */);

/* ---- exact k-nearest-neighbour queries ------------------------------------------------
 * The k nearest rows of a database cloud P (M rows) to each query point q, from the index the engine builds for
 * every cloud, 1 <= k <= gicp_knn_max_k().
 *   DISTANCE  d2(q, p) = ((dx * dx + dy * dy) + dz * dz) in fp64, dx = p_x - q_x, every product and every sum
 *             rounded on its own (no FMA), the z term dropped in 2-D: the bits NumPy's expression gives.
 *   ORDER     rows are ordered by (d2, original index), ascending: exactly equal distances go to the SMALLER
 *             original index.  The result is the first k rows of that order.  (The library's own rule; a KD-tree's
 *             choice at exact ties follows its traversal.)
 *   LIMIT     max_distance must be finite and >= 0; 0 sets no limit, otherwise only rows with
 *             d2 <= max_distance * max_distance (the product rounded once, the bound inclusive) are kept.
 *   OUTPUT    per query, in the caller's query order: index[k] the original rows (int64, padded with -1), dist2[k]
 *             their exact d2 (fp64, padded with +inf), count the number of real entries (int32).  Any of the three
 *             may be NULL.  The same inputs give the same bits on every call, context and GPU.
 * gicp_knn asks the resident cloud `which` (0 target, 1 source): its rows and indices are those of
 * gicp_get_points (the filtered cloud under gicp_set_voxel / gicp_set_filter; source shards do not matter).
 * queries == NULL is a SELF-QUERY: the queries are the cloud's own rows in original order (Q and dim are ignored),
 * so a row is its own neighbour at d2 = 0 and, among coincident rows, the lowest index comes first.  Nothing of the
 * context is used or changed beyond that cloud's index: not its staged targets, pose-dependent caches or filter
 * settings; an align gives the same bits with or without such calls around it.
 * gicp_knn_points is the one-shot: it indexes xyz (no covariances, no graph) into scratch and answers; the
 * context's clouds are untouched.  gicp_knn_host is host only (no HIP call, no context): a brute force over all
 * pairs, the CPU yardstick; its message is gicp_last_host_error()'s.
 * GICP_E_INVALID for: k outside 1 .. gicp_knn_max_k(); a dim other than 2 or 3, or other than the cloud's; Q < 1 or
 * M < 1; a non-finite query or point; a max_distance that is negative or not finite.  GICP_E_STATE when the
 * resident cloud is not set.  A refused call writes nothing.  The call is synchronous on the context's stream (one
 * stream synchronisation for a self-query of a resident cloud; indexing a query set or a one-shot database adds
 * the two of an index build each); scratch is grow-only. */
int gicp_knn_max_k(void);   /* 32 */
int gicp_knn(gicp_ctx* ctx, int which, const double* queries, int64_t Q, int dim, int k, double max_distance,
             int64_t* index /* [Q][k] */, double* dist2 /* [Q][k] */, int32_t* count /* [Q] */);
int gicp_knn_points(gicp_ctx* ctx, const double* xyz, int64_t M, const double* queries, int64_t Q, int dim, int k,
                    double max_distance, int64_t* index, double* dist2, int32_t* count);
int gicp_knn_host(const double* xyz, int64_t M, const double* queries, int64_t Q, int dim, int k, double max_distance,
                  int64_t* index, double* dist2, int32_t* count);

/* ---- statistical outlier removal -----------------------------------------------------
 * Removes the rows whose mean distance to their k nearest neighbours is large against the cloud's own statistic
 * (PCL's StatisticalOutlierRemoval, Open3D's remove_statistical_outlier), defined to the bit.
 * Input: M >= 2 rows, finite, dim 2 or 3, and a gicp_sor with k in 1 .. gicp_sor_max_k() (= gicp_knn_max_k() - 1
 * = 31) and std_ratio finite and >= 0.
 * Every operation below is fp64 and rounded on its own: no FMA, a correctly rounded sqrt, a correctly rounded
 * division.
 *   1. MEAN NEIGHBOUR DISTANCE.  n_i = min(k, M - 1).  Take the n_i smallest values of d2(p_i, p_j) over j != i,
 *      d2 the expression of the k-nearest-neighbour queries above; coincident other rows count, at 0.
 *      mean_i = (sum of sqrt(d2)) / n_i, the sum sequential in ascending order of d2, then one division.  Only the
 *      multiset of d2 values enters, so the result does not depend on how exact ties are ordered.  (On the device: a
 *      self-query for k + 1 rows with entry 0 dropped -- entry 0 is always a zero, the row itself or a coincident
 *      row of lower index.)
 *   2. TREE SUM T(v) of a vector in original row order: pad with +0.0 to the next power of two, replace v by
 *      v[0::2] + v[1::2] until one value is left.  All summands here are >= 0, so padding equals carrying the odd
 *      element.  (A wave's xor-butterfly over 64 consecutive rows, then (w0 + w1) + (w2 + w3) per 256 aligned rows,
 *      then the same tree over the partials, is this tree.)
 *   3. CLOUD STATISTICS.  mu = T(mean) / M;  dev_i = mean_i - mu;  sigma = sqrt(T(dev_i * dev_i) / (M - 1)) -- the
 *      two-pass sample deviation.
 *   4. DECISION.  thr = mu + std_ratio * sigma, the product first.  Keep i iff mean_i <= thr: the bound is
 *      inclusive, like every bound in this library.  One pass, not iterated.  Survivors keep their relative order.
 * The same functions (csrc/gicp_sor.h) serve the device kernels and gicp_sor_points_host.  No floating-point
 * atomics: the output is bit-identical from call to call, context to context, and to the host's.
 * GICP_E_INVALID, with the stage named in the message ("sor: ..."), for: k out of range; std_ratio negative or not
 * finite; M < 2; non-finite input; a T(mean) that is not finite; a stage that leaves no row (possible with
 * std_ratio = 0 when all means are equal and mu rounds below them).  Rows whose bounding box has a squared diagonal
 * that fp64 does not hold (coordinates about 1e154 apart) are refused before anything runs, by the device and the
 * host function alike: only there can a d2 overflow, so T(mean) is finite for every cloud that passes.
 *
 * One-shot, host in, host out (gicp_sor_points): out_xyz [N][dim], out_index [N], out_mean [N] (per INPUT row) and
 * out_stats [3] (mu, sigma, thr) are caller-allocated and any of them may be NULL; *M_out receives the number of
 * rows kept (they come first in out_xyz and out_index; out_index: the original row of each, ascending).  The
 * context's clouds and settings are untouched.  gicp_sor_points_host is host only (no HIP call, no context): a
 * brute force through the same search as gicp_knn_host, the CPU yardstick; its message is gicp_last_host_error()'s.
 *
 * Context setting (gicp_set_sor; NULL or k = 0: off, the default): every later cloud build runs
 *   upload -> de-skew -> crop -> radius outlier removal -> STATISTICAL OUTLIER REMOVAL -> voxel filter -> index
 * on the device.  The stage works on the survivors of the stages before it (M above is their number, "original
 * row order" theirs) and hands the next stage its survivors and their exact bounds on the device; it costs one
 * stream synchronisation beyond those of its own index build, and only result words return to the host.  A staged
 * build uses the setting in force when it was staged, on its own stream and scratch; GICP_STAGE_BORROW still reads
 * the caller's frame in place.  With a sharded source every rank filters the whole cloud.  A failure after the
 * build began leaves that cloud NOT SET.  "Original order" of a cloud means the rows of the filtered cloud, as for
 * the other filters.  With the setting off a build is what it was without this section. */
typedef struct gicp_sor {
    int32_t k;         /* neighbours of the mean, 1 .. gicp_sor_max_k(); 0: off (gicp_set_sor only) */
    int32_t pad;
    double std_ratio;  /* finite, >= 0 */
} gicp_sor;
int gicp_sor_max_k(void);   /* 31 */
int gicp_sor_points(gicp_ctx* ctx, const double* xyz, int64_t N, int dim, const gicp_sor* s, double* out_xyz,
                    int64_t* out_index, double* out_mean /* [N], per input row */,
                    double* out_stats /* [3]: mu, sigma, thr */, int64_t* M_out);
int gicp_sor_points_host(const double* xyz, int64_t N, int dim, const gicp_sor* s, double* out_xyz, int64_t* out_index,
                         double* out_mean, double* out_stats, int64_t* M_out);
int gicp_set_sor(gicp_ctx* ctx, const gicp_sor* s);

/* ---- Euclidean cluster extraction ------------------------------------------------------
 * The connected components of the graph "rows within `radius` of each other" (PCL's EuclideanClusterExtraction,
 * Open3D's cluster_dbscan with min_points 1), and the rows of the clusters whose size lies in given limits: what
 * removes a clump of returns that are each other's neighbours, which both outlier filters above keep, and what finds
 * objects.  Defined to the bit.
 * Input: N >= 1 rows, finite, dim 2 or 3, and a gicp_cluster.
 *   1. EDGES.  i ~ j (i != j) iff d2(p_i, p_j) <= radius * radius: d2 the expression of the input filters above, fp64
 *      with every product and sum rounded on its own (no FMA), the squared radius one rounded product, the bound
 *      inclusive.  Coincident rows are adjacent.  Hence a row is a singleton exactly when radius outlier removal's
 *      count_i at the same radius is 0.
 *   2. CLUSTERS.  The connected components of that graph.  Only the set partition is defined; nothing depends on
 *      the order in which anything is traversed.
 *   3. NUMBERING.  Clusters are numbered 0 .. C - 1 in ascending order of their smallest original row.  labels[i]
 *      (int32, per input row) is the number of row i's cluster, sizes[c] (int32) the row count of cluster c.  Every
 *      row has a label, whether its cluster is kept or not.
 *   4. DECISION.  A cluster is kept iff min_size <= size and (max_size == 0 or size <= max_size).  Kept rows keep
 *      their relative order.
 *   5. DETERMINISM.  Integer atomics only, no floating-point atomics: the output is bit-identical from call to
 *      call, context to context, and to the host function's.
 * GICP_E_INVALID, with the stage named in the message ("cluster: ..."), for: a radius that is not finite or is <= 0
 * (gicp_set_cluster takes 0 as off); min_size < 1; max_size < 0 or 0 < max_size < min_size; N < 1 or N >= 2^31 - 64;
 * non-finite input; a cloud spanning more than 2^21 (3-D) or 2^31 (2-D) cells of edge `radius` on an axis (the
 * message names the axis), or lying beyond 2^35 such cells from the origin -- the limits of radius outlier removal,
 * whose grid this is; a decision that keeps no row.  A refused call writes nothing.
 *
 * One-shot, host in, host out (gicp_cluster_points): labels [N], sizes [N] (the first C entries are written; N is the
 * worst case), n_clusters, out_xyz [N][dim], out_index [N] and M_out are caller-allocated and any of them may be
 * NULL; *M_out receives the number of rows kept (they come first in out_xyz and out_index; out_index: the original
 * row of each, ascending).  The context's clouds and settings are untouched.  gicp_cluster_points_host is host only
 * (no HIP call, no context): a union-find over the pairs the same grid proposes, the CPU yardstick; its message is
 * gicp_last_host_error()'s.  The device makes ONE lock-free pass over the edges whatever the shape of the components:
 * there are no rounds to count.
 *
 * Context setting (gicp_set_cluster; NULL or radius = 0: off, the default): every later cloud build runs
 *   upload -> de-skew -> crop -> radius outlier removal -> statistical outlier removal -> CLUSTER EXTRACTION ->
 *   voxel filter -> index
 * on the device.  The stage works on the survivors of the stages before it (N above is their number, "original row"
 * theirs), keeps the rows of the kept clusters and hands the next stage these rows and their exact bounds on the
 * device; it costs one stream synchronisation, in which only result words return to the host.  A staged build uses
 * the setting in force when it was staged, on its own stream and scratch; GICP_STAGE_BORROW still reads the
 * caller's frame in place.  With a sharded source every rank filters the whole cloud.  A failure after the build
 * began leaves that cloud NOT SET.  With the setting off a build is what it was without this section. */
typedef struct gicp_cluster {
    double radius;      /* finite, > 0; 0: off (gicp_set_cluster only) */
    int32_t min_size;   /* >= 1 */
    int32_t max_size;   /* 0: no upper limit, else >= min_size */
} gicp_cluster;
int gicp_cluster_points(gicp_ctx* ctx, const double* xyz, int64_t N, int dim, const gicp_cluster* c,
                        int32_t* labels /* [N] */, int32_t* sizes /* [N] worst case */, int64_t* n_clusters,
                        double* out_xyz /* [N][dim] */, int64_t* out_index /* [N] */, int64_t* M_out);
int gicp_cluster_points_host(const double* xyz, int64_t N, int dim, const gicp_cluster* c, int32_t* labels, int32_t* sizes,
                             int64_t* n_clusters, double* out_xyz, int64_t* out_index, int64_t* M_out);
int gicp_set_cluster(gicp_ctx* ctx, const gicp_cluster* c);

#ifdef __cplusplus
}
#endif
#endif /* GICP_HIP_H */
