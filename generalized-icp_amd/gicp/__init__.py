"""MI355X-native GICP — drop-in for msi-se/generalized-icp's ``gicp.py``.

``from gicp import gicp, apply_transformation`` works as with the reference
(python-implementation/gicp.py:78, :176; imported that way by
visualization.py:7 and robot-visualization.py:6).  The per-iteration hot path
(correspondences, Mahalanobis weights, normal-equation statistics) and the
per-point surface covariances run in hand-written HIP kernels for gfx950
behind the C-ABI of ``libgicp_hip.so``; this module is the thin host layer.

There is no CPU fallback: without the built library or a GPU the engine
raises.  HIP is initialised on the first call, not at import (the reference
calls gicp() from a forked worker, robot-visualization.py:199).
"""
from __future__ import annotations

import ctypes as C
from collections.abc import Sequence

import numpy as np

from . import _lib
from ._lib import Debug, Params, Report, ReportSpec, Result, Trace, check, dptr

__all__ = ["gicp", "apply_transformation", "Engine", "RotatedCovariances", "expand_stats", "stats_size",
           "default_params", "last_result", "voxel_downsample", "filter_points", "filter_points_host", "deskew", "deskew_host", "motion_twist", "information",
           "sym_eig", "align_batch", "multistart", "batch_max_points", "pick_start", "knn", "knn_host", "knn_max_k", "sor_points", "sor_points_host",
           "sor_max_k", "cluster_points", "cluster_points_host"]


def stats_size(dim):
    ns = dim * (dim + 1) // 2
    return ns * ns + ns * dim + ns + dim * dim + dim + 2


def default_params(dim, **kw):
    """gicp_params with the reference defaults (gicp.py:5, :11, :24, :78), overridden by kw.
    robust_kernel takes a name of _lib.ROBUST_KERNELS or its GICP_ROBUST_* code."""
    p = Params()
    _lib.load().gicp_default_params(dim, C.byref(p))
    for k, v in kw.items():
        if v is not None:
            setattr(p, k, _robust_code(v) if k == "robust_kernel" else v)
    return p


def _robust_code(kernel):
    """GICP_ROBUST_* code of a robust kernel given by name or by code (None: none)."""
    if kernel is None:
        return 0
    if isinstance(kernel, str):
        if kernel not in _lib.ROBUST_KERNELS:
            raise ValueError(f"robust_kernel must be one of {sorted(_lib.ROBUST_KERNELS)}, got {kernel!r}")
        return _lib.ROBUST_KERNELS[kernel]
    return int(kernel)


def _sym_pairs(d):
    return [(a, b) for a in range(d) for b in range(a, d)]


def expand_stats(st, d):
    """(H, g, c0, count) of  f(z) = c0 - 2 g.(z - z_k) + (z - z_k)^T H (z - z_k),  z = (vec R, t).

    Layout of ``st``: A[ab][ij] = sum W_ab s_i s_j, B[ab][i] = sum W_ab s_i,
    C[ab] = sum W_ab, gR[a][i] = sum (W r_k)_a s_i, gt[a] = sum (W r_k)_a, c0, count."""
    st = np.asarray(st, dtype=np.float64)
    P = _sym_pairs(d)
    ns = len(P)
    pos = {}
    for k, (a, b) in enumerate(P):
        pos[(a, b)] = pos[(b, a)] = k
    o = 0
    A = st[o:o + ns * ns].reshape(ns, ns); o += ns * ns
    B = st[o:o + ns * d].reshape(ns, d); o += ns * d
    Cc = st[o:o + ns]; o += ns
    gR = st[o:o + d * d].reshape(d, d); o += d * d
    gt = st[o:o + d]; o += d
    nz = d * d + d
    H = np.zeros((nz, nz))
    for a in range(d):
        for i in range(d):
            for b in range(d):
                for j in range(d):
                    H[a * d + i, b * d + j] = A[pos[(a, b)], pos[(i, j)]]
                H[a * d + i, d * d + b] = H[d * d + b, a * d + i] = B[pos[(a, b)], i]
        for b in range(d):
            H[d * d + a, d * d + b] = Cc[pos[(a, b)]]
    return H, np.concatenate([gR.ravel(), gt]), float(st[o]), float(st[o + 1])


# 2-D: z6 = (R00, R01, R10, R11, tx, ty) = L (tx, ty, cos th, sin th)
_L2 = np.array([[0, 0, 1, 0], [0, 0, 0, -1], [0, 0, 0, 1], [0, 0, 1, 0], [1, 0, 0, 0], [0, 1, 0, 0]], dtype=np.float64)


def _rot2(theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, -s], [s, c]])


def _offset_to_T(x):
    """gicp.py:42-50."""
    T = np.eye(3)
    T[:2, :2] = _rot2(x[2])
    T[:2, 2] = x[:2]
    return T


def apply_transformation(cloud, T):
    """gicp.py:176-177 (any dimension: x -> R x + t)."""
    T = np.asarray(T)
    d = T.shape[0] - 1
    return np.dot(np.asarray(cloud)[:, :d], T[:d, :d].T) + T[:d, d]


class Engine:
    """One GPU context of libgicp_hip.so (clouds stay resident between calls)."""

    def __init__(self, device=0):
        self._lib = _lib.load()
        self._ctx = C.c_void_p()
        rc = self._lib.gicp_create(C.byref(self._ctx), int(device))
        if rc == _lib.GICP_E_INVALID:
            raise ValueError(f"gicp_create(device={device}): no such GPU")
        if rc != _lib.GICP_OK:
            raise _lib.GicpError(rc, f"gicp_create(device={device}): {self._lib.gicp_strerror(rc).decode()}")
        self.device = device
        self.dim = None
        self.n_src = self.n_tgt = 0
        self.generation = 0        # bumped whenever the source cloud changes (lazy covariance views)
        self._staged = []          # (shape, params, borrowed array or None) of the staged targets, oldest first
        self._hook = None          # keeps the ctypes callback of set_allreduce alive
        self._hook_fn = None       # (fn, nranks, rank) of that hook, to restore it after a gicp() call
        self.voxel = (0.0, 1)      # (voxel_size, min_points) of set_voxel; size 0: no filter
        self.filter = _NO_FILTER   # the keywords of set_filter in force (all zero: no filter)
        self.sor = (0, 0.0)        # (k, std_ratio) of set_sor; k 0: off
        self.cluster = (0.0, 1, 0)  # (radius, min_size, max_size) of set_cluster; radius 0: off
        self.map_dim = None        # dimension of the local voxel map (map_reset)

    def close(self):
        if self._ctx:
            self._lib.gicp_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _cloud(pts):
        a = np.ascontiguousarray(np.asarray(pts, dtype=np.float64))
        if a.ndim != 2 or a.shape[1] not in (2, 3) or a.shape[0] < 1:
            raise ValueError(f"point cloud must be a non-empty N x 2 or N x 3 array, got shape {a.shape}")
        return a

    def comm_init(self, nranks, rank, uid: bytes):
        check(self._lib.gicp_comm_init(self._ctx, nranks, rank, uid), self._ctx, "gicp_comm_init")

    def comm_ranks(self):
        """(nranks, rank, kind) of the statistics exchange, read back from the RCCL communicator
        (gicp_comm_ranks); kind is 'none', 'rccl' or 'hook'."""
        n, r, k = C.c_int(), C.c_int(), C.c_int()
        check(self._lib.gicp_comm_ranks(self._ctx, C.byref(n), C.byref(r), C.byref(k)), self._ctx, "gicp_comm_ranks")
        return n.value, r.value, {0: "none", 1: "rccl", 2: "hook", 3: "peer"}[k.value]

    def peer_export(self) -> bytes:
        """This rank's exchange area as an IPC handle (gicp_peer_export): all-gather it, then peer_init."""
        buf = C.create_string_buffer(_lib.PEER_HANDLE_BYTES)
        check(self._lib.gicp_peer_export(self._ctx, buf), self._ctx, "gicp_peer_export")
        return buf.raw

    def peer_init(self, nranks, rank, handles, timeout=10.0):
        """Map the peers' exchange areas (handles in rank order) and prove the path with one probe
        exchange (gicp_peer_init, collective): from then on every pass sums the statistics over the
        ranks inside its own launch.  Raises GicpError (code GICP_E_COMM) when the path does not work."""
        if len(handles) != nranks or any(len(h) != _lib.PEER_HANDLE_BYTES for h in handles):
            raise ValueError(f"need {nranks} handles of {_lib.PEER_HANDLE_BYTES} bytes")
        blob = b"".join(handles)
        check(self._lib.gicp_peer_init(self._ctx, int(nranks), int(rank), blob, float(timeout)), self._ctx,
              "gicp_peer_init")

    def peer_close(self):
        check(self._lib.gicp_peer_close(self._ctx), self._ctx, "gicp_peer_close")

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
        check(_lib.load().gicp_comm_unique_id(buf), None, "gicp_comm_unique_id")
        return buf.raw

    @staticmethod
    def _sweep(a, stamps, motion, ref):
        """(gicp_sweep, the stamps array it points into) of the cloud `a`."""
        d = a.shape[1]
        st = np.ascontiguousarray(np.asarray(stamps, dtype=np.float64))
        if st.shape != (a.shape[0],):
            raise ValueError(f"stamps must hold one value per point ({a.shape[0]}), got shape {st.shape}")
        if motion is None:
            raise ValueError("a sweep needs its motion (stamps given, motion None)")
        M = np.asarray(motion, dtype=np.float64)
        if M.shape != (d + 1, d + 1):
            raise ValueError(f"motion must be {d + 1} x {d + 1}, got shape {M.shape}")
        sw = _lib.Sweep()
        sw.stamps = dptr(st)
        sw.ref = float(ref)
        for k, v in enumerate(M.ravel()):
            sw.motion[k] = v
        return sw, st

    def set_target(self, pts, params=None, stamps=None, motion=None, ref=0.0):
        """Index `pts` as the target.  With `stamps` (one per point) the cloud is a sweep: it is de-skewed on
        the device by the rigid `motion` per stamp unit to the reference stamp `ref` before it is filtered and
        indexed (gicp_set_target_sweep; see `deskew`)."""
        a = self._cloud(pts)
        p = params or default_params(a.shape[1])
        if stamps is None:
            rc = self._lib.gicp_set_target(self._ctx, dptr(a), a.shape[0], a.shape[1], C.byref(p))
        else:
            sw, _keep = self._sweep(a, stamps, motion, ref)
            rc = self._lib.gicp_set_target_sweep(self._ctx, dptr(a), a.shape[0], a.shape[1], C.byref(p), C.byref(sw))
        check(rc, self._ctx, "gicp_set_target")
        self.n_tgt, self.dim = a.shape
        if self._reduces():
            self.n_tgt = self.cloud_size("target")

    def set_source(self, pts, params=None, shard=0, nshards=1, stamps=None, motion=None, ref=0.0):
        """Index `pts` as the source; `stamps`, `motion`, `ref` as in set_target (gicp_set_source_sweep)."""
        a = self._cloud(pts)
        p = params or default_params(a.shape[1])
        if stamps is None:
            rc = self._lib.gicp_set_source(self._ctx, dptr(a), a.shape[0], a.shape[1], C.byref(p), shard, nshards)
        else:
            sw, _keep = self._sweep(a, stamps, motion, ref)
            rc = self._lib.gicp_set_source_sweep(self._ctx, dptr(a), a.shape[0], a.shape[1], C.byref(p), shard, nshards,
                                                 C.byref(sw))
        check(rc, self._ctx, "gicp_set_source")
        self.n_src, self.dim = a.shape
        if self._reduces():
            self.n_src = self.cloud_size("source")
        self.generation += 1

    def target_to_source(self, shard=0, nshards=1):
        check(self._lib.gicp_target_to_source(self._ctx, shard, nshards), self._ctx, "gicp_target_to_source")
        self.n_src = self.n_tgt
        self.n_tgt = 0
        self.generation += 1

    MAX_STAGED = 2   # GICP_MAX_STAGED

    def stage_target(self, pts, params=None, borrow=False, stamps=None, motion=None, ref=0.0):
        """Build `pts` as a coming target on its own stream while the current one is registered
        (gicp_stage_target; up to MAX_STAGED pending); commit_target makes the oldest current.  The
        library copies `pts` before this call returns, so the caller may reuse the array at once --
        unless borrow=True (GICP_STAGE_BORROW): then the build reads the array itself (no copy on this
        thread) and the caller must not modify it until commit_target / cancel_stage (this object keeps
        a reference until then).  `stamps`, `motion`, `ref` as in set_target (gicp_stage_target_sweep); the
        stamps are copied or borrowed with the points."""
        a = self._cloud(pts)
        p = params or default_params(a.shape[1])
        flags = _lib.GICP_STAGE_BORROW if borrow else 0
        st = None
        if stamps is None:
            rc = self._lib.gicp_stage_target_ex(self._ctx, dptr(a), a.shape[0], a.shape[1], C.byref(p), flags)
        else:
            sw, st = self._sweep(a, stamps, motion, ref)
            rc = self._lib.gicp_stage_target_sweep(self._ctx, dptr(a), a.shape[0], a.shape[1], C.byref(p), flags,
                                                   C.byref(sw))
        check(rc, self._ctx, "gicp_stage_target")
        self._staged.append((a.shape, p, (a, st) if borrow else None, self._reduces()))

    def commit_target(self, shard=0, nshards=1):
        """Wait for the oldest staged target; the current target becomes the source, the staged one the target."""
        rc = self._lib.gicp_commit_target(self._ctx, shard, nshards)
        staged = self._staged.pop(0) if (self._staged and rc != _lib.GICP_E_STATE) else None   # slot consumed
        check(rc, self._ctx, "gicp_commit_target")
        if self.n_tgt:
            self.n_src = self.n_tgt
            self.generation += 1
        self.n_tgt, self.dim = staged[0]
        if staged[3]:   # staged with a voxel or input filter set: the target holds the filtered cloud
            self.n_tgt = self.cloud_size("target")

    def cancel_stage(self):
        """Wait for and drop every staged target."""
        self._lib.gicp_cancel_stage(self._ctx)
        self._staged = []

    def set_voxel(self, voxel_size, min_points=1):
        """Voxel-grid filter of every cloud set or staged from now on (gicp_set_voxel): each is reduced on
        the device to one centroid per occupied cell of the absolute grid floor(x / voxel_size), cells
        with fewer than min_points points dropped, before its index is built.  voxel_size None or 0 turns
        the filter off.  With a filter, every per-point output of this engine (covariances,
        neighbor_counts, graph, iterate's index / weight / distance, the top weights) refers to the rows of
        the FILTERED clouds, which points() returns: ascending lexicographic order of the cells."""
        size = 0.0 if voxel_size is None else float(voxel_size)
        check(self._lib.gicp_set_voxel(self._ctx, size, int(min_points)), self._ctx, "gicp_set_voxel")
        self.voxel = (size, int(min_points))

    def _reduces(self):
        """A filter of the builds is in force (set_voxel, set_filter): a cloud then holds fewer rows than its input."""
        return self.voxel[0] > 0 or _filter_on(self.filter) or self.sor[0] > 0 or self.cluster[0] > 0

    def set_sor(self, k, std_ratio=1.0):
        """Statistical outlier removal of every cloud set or staged from now on (gicp_set_sor), on the
        device, after the input filters and before the voxel filter: a row is kept iff the mean distance to its k
        nearest neighbours is at most mu + std_ratio sigma, mu and sigma the mean and the sample deviation of those
        means over the cloud (gicp.sor_points has the definition).  k None or 0 turns it off.  With it, every
        per-point output of this engine refers to the rows of the FILTERED clouds, which points() returns: the
        input's rows that survive, in their order.  Engine.sor holds the setting as (k, std_ratio)."""
        k = 0 if k is None else int(k)
        s = _lib.Sor(k, 0, float(std_ratio) if k else 0.0)
        check(self._lib.gicp_set_sor(self._ctx, C.byref(s)), self._ctx, "gicp_set_sor")
        self.sor = (s.k, s.std_ratio)

    def sor_points(self, points, k, std_ratio=1.0, return_index=False, return_mean=False, return_stats=False):
        """gicp.sor_points on this engine's GPU (gicp_sor_points); the engine's clouds and settings are untouched."""
        a = self._cloud(points)
        return _sor_call(lambda *args: check(self._lib.gicp_sor_points(self._ctx, *args), self._ctx, "gicp_sor_points"),
                         a, k, std_ratio, return_index, return_mean, return_stats)

    def set_cluster(self, radius, min_size=1, max_size=0):
        """Euclidean cluster extraction of every cloud set or staged from now on (gicp_set_cluster), on
        the device, after statistical outlier removal and before the voxel filter: the rows within `radius` of each
        other form the edges of a graph, its connected components are the clusters, and the rows of the clusters
        with min_size <= size (and size <= max_size unless max_size is 0) are kept (gicp.cluster_points has the
        definition).  radius None or 0 turns it off.  With it, every per-point output of this engine refers to the
        rows of the FILTERED clouds, which points() returns: the input's rows that survive, in their order.
        Engine.cluster holds the setting as (radius, min_size, max_size)."""
        radius = 0.0 if radius is None else float(radius)
        c = _lib.Cluster(radius, int(min_size) if radius else 1, int(max_size) if radius else 0)
        check(self._lib.gicp_set_cluster(self._ctx, C.byref(c)), self._ctx, "gicp_set_cluster")
        self.cluster = (c.radius, c.min_size, c.max_size)

    def cluster_points(self, points, radius, min_size=1, max_size=0, return_index=False, return_labels=False, return_sizes=False):
        """gicp.cluster_points on this engine's GPU (gicp_cluster_points); the engine's clouds and settings are
        untouched."""
        a = self._cloud(points)
        return _cluster_call(lambda *args: check(self._lib.gicp_cluster_points(self._ctx, *args), self._ctx, "gicp_cluster_points"),
                             a, radius, min_size, max_size, return_index, return_labels, return_sizes)

    def set_filter(self, center=None, min_range=0.0, max_range=0.0, radius=0.0, min_neighbors=1):
        """Input filters of every cloud set or staged from now on (gicp_set_filter), on the device,
        after the de-skew and before the voxel filter: a range crop about `center` (None: the origin, the sensor
        of a scan in its own frame) keeping min_range <= |p - center| <= max_range (0: no limit), then radius
        outlier removal among the crop's survivors, keeping a point with at least min_neighbors others within
        `radius` (0: off).  Every argument at its default turns the filters off.  With a filter, every per-point
        output of this engine refers to the rows of the FILTERED clouds, which points() returns: the input's
        rows that survive, in their order.  Engine.filter holds the setting as these keywords."""
        kw = _filter_kw(center, min_range, max_range, radius, min_neighbors)
        f = _filter_struct(kw, None)
        check(self._lib.gicp_set_filter(self._ctx, C.byref(f)), self._ctx, "gicp_set_filter")
        self.filter = kw

    def filter_points(self, points, center=None, min_range=0.0, max_range=0.0, radius=0.0, min_neighbors=1,
                      return_index=False, return_counts=False):
        """gicp.filter_points on this engine's GPU (gicp_filter_points); the engine's clouds and its set_filter
        setting are untouched."""
        a = self._cloud(points)
        f = _filter_struct(_filter_kw(center, min_range, max_range, radius, min_neighbors), a.shape[1])
        return _filter_call(lambda *args: check(self._lib.gicp_filter_points(self._ctx, *args), self._ctx,
                                                "gicp_filter_points"), a, f, return_index, return_counts)

    def voxel_downsample(self, points, voxel_size, min_points=1, return_counts=False):
        """gicp.voxel_downsample on this engine's GPU (gicp_voxel_downsample); the engine's clouds and its
        set_voxel setting are untouched."""
        a = self._cloud(points)
        out = np.empty_like(a)
        cnt = np.empty(a.shape[0], dtype=np.int32)
        m = C.c_int64()
        check(self._lib.gicp_voxel_downsample(self._ctx, dptr(a), a.shape[0], a.shape[1], float(voxel_size),
                                              int(min_points), dptr(out), cnt.ctypes.data_as(C.POINTER(C.c_int32)),
                                              C.byref(m)), self._ctx, "gicp_voxel_downsample")
        out = out[:m.value].copy()
        return (out, cnt[:m.value].copy()) if return_counts else out

    def deskew(self, points, stamps, motion, ref=0.0):
        """gicp.deskew on this engine's GPU (gicp_deskew); the engine's clouds are untouched."""
        a = self._cloud(points)
        _, st = self._sweep(a, stamps, motion, ref)   # (the shape checks)
        M = np.ascontiguousarray(np.asarray(motion, dtype=np.float64))
        out = np.empty_like(a)
        check(self._lib.gicp_deskew(self._ctx, dptr(a), dptr(st), a.shape[0], a.shape[1], dptr(M), float(ref),
                                    dptr(out)), self._ctx, "gicp_deskew")
        return out

    def knn(self, queries=None, k=1, max_distance=None, which="target", squared=False):
        """The k nearest rows of the resident cloud `which` to every query (gicp_knn), exact: fp64
        d2 = ((dx*dx + dy*dy) + dz*dz), rows ordered by (d2, original index), so exactly equal distances go to the
        smaller index.  `queries` Q x dim, or None for a self-query (the cloud's own rows, each its own neighbour
        at distance 0).  max_distance None or 0: no limit, else only rows with d2 <= max_distance**2.  Returns
        (index [Q, k] int64 padded with -1, distance [Q, k] float64 padded with inf; squared=True: d2 itself).
        Indices refer to `Engine.points(which)`.  The engine's clouds, caches and settings are untouched."""
        w = 0 if which == "target" else 1
        if queries is None:
            q, nq, dim = None, self.cloud_size(which), 0
        else:
            q = _knn_array(queries, "queries")
            nq, dim = q.shape
        return _knn_call(lambda *args: check(self._lib.gicp_knn(self._ctx, w, *args), self._ctx, "gicp_knn"),
                         q, nq, dim, k, max_distance, squared)

    def knn_points(self, points, queries=None, k=1, max_distance=None, squared=False):
        """gicp.knn on this engine's GPU (gicp_knn_points); the engine's clouds are untouched."""
        a = _knn_array(points, "points")
        if queries is None:
            q, nq = None, a.shape[0]
        else:
            q = _knn_array(queries, "queries")
            nq = q.shape[0]
            if q.shape[1] != a.shape[1]:
                raise ValueError(f"queries must be Q x {a.shape[1]} as the points, got shape {q.shape}")
        return _knn_call(lambda *args: check(self._lib.gicp_knn_points(self._ctx, dptr(a), a.shape[0], *args), self._ctx,
                                             "gicp_knn_points"), q, nq, a.shape[1], k, max_distance, squared)

    def cloud_size(self, which="target"):
        """Points the indexed cloud holds (gicp_cloud_size): the input's length, with set_filter the rows that
        survive, with a voxel filter the number of voxels kept."""
        n = C.c_int64()
        check(self._lib.gicp_cloud_size(self._ctx, 0 if which == "target" else 1, C.byref(n)), self._ctx,
              "gicp_cloud_size")
        return int(n.value)

    def points(self, which="target"):
        """The indexed cloud's points in its original order (gicp_get_points): the input rows, with set_filter
        the surviving rows in their order, with a voxel filter the centroids -- what every per-point output refers to."""
        n = self.cloud_size(which)
        out = np.empty((n, self.dim))
        check(self._lib.gicp_get_points(self._ctx, 0 if which == "target" else 1, dptr(out)), self._ctx,
              "gicp_get_points")
        return out

    # ---- local voxel map (gicp_map_*) ----
    def map_reset(self, voxel_size, max_range, dim=None):
        """Create or empty the engine's local voxel map (gicp_map_reset): voxels of the absolute grid
        floor(x / voxel_size) in the world frame, kept within ceil(max_range / voxel_size) cells of the last
        inserted pose's cell on every axis.  dim defaults to the engine's clouds' dimension (3 before any)."""
        d = int(dim if dim is not None else (self.dim or 3))
        check(self._lib.gicp_map_reset(self._ctx, d, float(voxel_size), float(max_range)), self._ctx, "gicp_map_reset")
        self.map_dim = d

    def map_insert(self, T=None, which="source", points=None):
        """Merge a cloud posed at T (sensor -> world, identity if None) into the map: the engine's indexed
        `which` cloud straight from the device (with set_voxel in force, the filtered cloud), or the host
        array `points`.  The window is re-centred on T's translation; what leaves it is forgotten."""
        d = self.map_dim or self.dim or 3
        T = np.eye(d + 1) if T is None else np.ascontiguousarray(np.asarray(T, dtype=np.float64))
        if points is not None:
            a = self._cloud(points)
            if T.shape != (a.shape[1] + 1,) * 2:
                raise ValueError(f"T must be {a.shape[1] + 1} x {a.shape[1] + 1}")
            check(self._lib.gicp_map_insert_points(self._ctx, dptr(a), a.shape[0], a.shape[1], dptr(T)), self._ctx,
                  "gicp_map_insert_points")
            return
        if T.shape != (d + 1, d + 1):
            raise ValueError(f"T must be {d + 1} x {d + 1}")
        check(self._lib.gicp_map_insert(self._ctx, 0 if which == "target" else 1, dptr(T)), self._ctx, "gicp_map_insert")

    def map_size(self):
        """Voxels the map holds (gicp_map_size)."""
        n = C.c_int64()
        check(self._lib.gicp_map_size(self._ctx, C.byref(n)), self._ctx, "gicp_map_size")
        return int(n.value)

    def map_get(self):
        """The map's rows in ascending lexicographic order of the cells (gicp_map_get):
        (cells int32 [M, d], centroids [M, d], counts int32 [M])."""
        m = self.map_size()
        d = self.map_dim or self.dim or 3
        cells = np.empty((m, d), dtype=np.int32)
        cent = np.empty((m, d))
        cnt = np.empty(m, dtype=np.int32)
        p32 = C.POINTER(C.c_int32)
        check(self._lib.gicp_map_get(self._ctx, cells.ctypes.data_as(p32), dptr(cent), cnt.ctypes.data_as(p32)), self._ctx,
              "gicp_map_get")
        return cells, cent, cnt

    def map_to_target(self, params=None, min_points=1):
        """The centroids of the map's voxels holding at least min_points points become the target
        (gicp_map_to_target), in the order of map_get; the source is left alone."""
        d = self.map_dim or self.dim or 3
        p = params or default_params(d)
        check(self._lib.gicp_map_to_target(self._ctx, C.byref(p), int(min_points)), self._ctx, "gicp_map_to_target")
        self.dim = d
        self.n_tgt = self.cloud_size("target")

    def covariances(self, which="target"):
        w = 0 if which == "target" else 1
        n = self.n_tgt if w == 0 else self.n_src
        out = np.empty((n, self.dim, self.dim))
        check(self._lib.gicp_get_covariances(self._ctx, w, dptr(out)), self._ctx, "gicp_get_covariances")
        return out

    def rotated_covariances(self, R, which="source"):
        """R C Rᵀ of every point on the device (gicp_rotated_covariances), original order."""
        w = 0 if which == "target" else 1
        n = self.n_tgt if w == 0 else self.n_src
        R = np.ascontiguousarray(np.asarray(R, dtype=np.float64))
        if R.shape != (self.dim, self.dim):
            raise ValueError(f"R must be {self.dim} x {self.dim}")
        out = np.empty((n, self.dim, self.dim))
        check(self._lib.gicp_rotated_covariances(self._ctx, w, dptr(R), dptr(out)), self._ctx,
              "gicp_rotated_covariances")
        return out

    def graph(self):
        """The target neighbour graph (gicp_get_graph): (index [M, 20] original ids with -1 pads,
        radius [M]: every target nearer than radius[i] to point i is in row i)."""
        idx = np.empty((self.n_tgt, _lib.GRAPH_K), dtype=np.int64)
        rad = np.empty(self.n_tgt)
        check(self._lib.gicp_get_graph(self._ctx, idx.ctypes.data_as(C.POINTER(C.c_int64)), dptr(rad)), self._ctx,
              "gicp_get_graph")
        return idx, rad

    def reset_cache(self):
        """Forget the pose-dependent caches (lists, certificates, last matches): the next pass starts cold."""
        check(self._lib.gicp_reset_cache(self._ctx), self._ctx, "gicp_reset_cache")

    def iteration_times(self):
        """Sampled k_corr time (ms) per iteration of the last align; NaN where not sampled."""
        buf = (C.c_float * 4096)()
        m = self._lib.gicp_iteration_times(self._ctx, buf, 4096)
        check(min(m, 0), self._ctx, "gicp_iteration_times")
        t = np.array(buf[:m], dtype=np.float64)
        t[t < 0] = np.nan
        return t

    def set_allreduce(self, fn, nranks=1, rank=0):
        """Host statistics exchange (gicp_set_allreduce_ranks): fn(buf) gets this rank's statistics as a
        float64 array and must return (or write in place) the sum over ranks; (nranks, rank) is what
        comm_ranks() then reports.  None removes it."""
        if fn is None:
            check(self._lib.gicp_set_allreduce(self._ctx, None, None), self._ctx, "gicp_set_allreduce")
            self._hook = None
            self._hook_fn = None
            return

        def _cb(buf, n, _user):
            try:
                a = np.ctypeslib.as_array(buf, shape=(n,))
                r = fn(a)
                if r is not None and r is not a:
                    a[:] = np.asarray(r, dtype=np.float64)
                return 0
            except Exception:   # an exception must not cross the C boundary
                import traceback
                traceback.print_exc()
                return -1

        cb = _lib.ALLREDUCE_FN(_cb)
        check(self._lib.gicp_set_allreduce_ranks(self._ctx, C.cast(cb, C.c_void_p), None, int(nranks), int(rank)),
              self._ctx, "gicp_set_allreduce")
        self._hook = cb
        self._hook_fn = (fn, int(nranks), int(rank))

    def neighbor_counts(self, which="target"):
        w = 0 if which == "target" else 1
        n = self.n_tgt if w == 0 else self.n_src
        out = np.empty(n, dtype=np.int32)
        check(self._lib.gicp_get_neighbor_counts(self._ctx, w, out.ctypes.data_as(C.POINTER(C.c_int32))), self._ctx,
              "gicp_get_neighbor_counts")
        return out

    def iterate(self, T, debug=False):
        """One pass at pose T -> statistics (and per-point index / W / distance if debug)."""
        T = np.ascontiguousarray(np.asarray(T, dtype=np.float64))
        st = np.empty(stats_size(self.dim))
        dbg = None
        out = None
        if debug:
            n, d = self.n_src, self.dim
            out = dict(index=np.empty(n, dtype=np.int64), weight=np.empty((n, d, d)), distance=np.empty(n))
            dbg = Debug(out["index"].ctypes.data_as(C.POINTER(C.c_int64)), dptr(out["weight"]), dptr(out["distance"]))
        check(self._lib.gicp_iterate(self._ctx, dptr(T), dptr(st), C.byref(dbg) if dbg else None), self._ctx,
              "gicp_iterate")
        return (st, out) if debug else st

    def evaluate(self, T=None, params=None, thresholds=(), quantiles=()):
        """One pass at pose T (None: identity) and its report (gicp_evaluate), reduced on the
        device: a dict with the information matrix 'H' (6 x 6; 2-D 3 x 3, twist (omega, v), left perturbation)
        and 'b', the spectra 'eig'/'eigvec' of H, 'eig_rot'/'vec_rot' and 'eig_trans'/'vec_trans' of its blocks
        (ascending, eigenvectors in columns), per threshold 'inliers', 'inlier_sum_sq', 'fitness' and
        'inlier_rmse', the lower order statistics 'dist_q' and 'white_q' keyed by probability, and 'n_source',
        'n_matched', 'sum_sq', 'loss'.  params (None: the values in force) gives d_c, cov_model and the robust
        kernel of this pass alone."""
        spec, thr, qs = _report_spec(thresholds, quantiles)
        Tp = None if T is None else np.ascontiguousarray(np.asarray(T, dtype=np.float64))
        rep = Report()
        check(self._lib.gicp_evaluate(self._ctx, None if Tp is None else dptr(Tp), C.byref(params) if params else None,
                                      C.byref(spec), C.byref(rep)), self._ctx, "gicp_evaluate")
        return _report_dict(rep, thr, qs)

    def pass_info(self):
        """Diagnostics of the last pass: walking lanes the fp32 screen left ambiguous (re-resolved in fp64),
        pairs screened, list rebuilds, sum |r|^2, lanes proved by the graph descent (its near ties, resolved
        in fp64 from the row, included), source tiles that walked."""
        out = np.empty(_lib.PASS_INFO)
        check(self._lib.gicp_pass_info(self._ctx, dptr(out)), self._ctx, "gicp_pass_info")
        return dict(ambiguous=out[0], pairs=out[1], list_rebuilds=out[2], sum_sq=out[3], graph_proved=out[4],
                    walked_tiles=out[5])

    def iterate_top(self, T, k=5):
        """One pass at pose T keeping det(W) on the device, then its top-k on the device
        (gicp.py:170 `np.argsort(det(W))[-k:]`): (statistics, src_idx[k], tgt_idx[k], det[k])."""
        T = np.ascontiguousarray(np.asarray(T, dtype=np.float64))
        st = np.empty(stats_size(self.dim))
        dbg = Debug(None, None, None, 1)
        check(self._lib.gicp_iterate(self._ctx, dptr(T), dptr(st), C.byref(dbg)), self._ctx, "gicp_iterate")
        si = np.empty(k, dtype=np.int64)
        ti = np.empty(k, dtype=np.int64)
        dt = np.empty(k)
        p64 = C.POINTER(C.c_int64)
        check(self._lib.gicp_top_weights(self._ctx, k, si.ctypes.data_as(p64), ti.ctypes.data_as(p64), dptr(dt)),
              self._ctx, "gicp_top_weights")
        return st, si, ti, dt

    def align(self, T0=None, params=None, trace=False, top_k=0):
        """The whole outer loop (gicp.py:116-167) natively; returns (T, result dict), plus with
        trace=True a dict of per-iteration rows recorded on the device (gicp_align_trace): 'poses'
        [iters, d+1, d+1] (the pose each pass ran at), 'losses' [iters], and with top_k > 0 the
        pass's top_k largest det(W): 'top_src', 'top_tgt' [iters, top_k] original indices, 'top_det'."""
        d = self.dim
        T0 = np.eye(d + 1) if T0 is None else np.ascontiguousarray(np.asarray(T0, dtype=np.float64))
        Tout = np.empty((d + 1, d + 1))
        res = Result()
        p = params or default_params(d)
        if trace:
            cap = max(1, int(p.max_iterations))
            rows = dict(poses=np.zeros((cap, d + 1, d + 1)), losses=np.zeros(cap),
                        top_src=np.full((cap, max(top_k, 1)), -1, dtype=np.int64),
                        top_tgt=np.full((cap, max(top_k, 1)), -1, dtype=np.int64),
                        top_det=np.zeros((cap, max(top_k, 1))))
            p64 = C.POINTER(C.c_int64)
            tr = Trace(cap, int(top_k), dptr(rows["poses"]), dptr(rows["losses"]),
                       rows["top_src"].ctypes.data_as(p64), rows["top_tgt"].ctypes.data_as(p64), dptr(rows["top_det"]))
            check(self._lib.gicp_align_trace(self._ctx, dptr(T0), C.byref(p), dptr(Tout), C.byref(res), C.byref(tr)),
                  self._ctx, "gicp_align_trace")
        else:
            check(self._lib.gicp_align(self._ctx, dptr(T0), C.byref(p), dptr(Tout), C.byref(res)), self._ctx,
                  "gicp_align")
        r = res.as_dict()
        r.pop("pad", None)
        r.pop("pad2", None)
        r["stop_reason"] = _lib.STOP_REASONS.get(r["stop_reason"], r["stop_reason"])
        if not trace:
            return Tout, r
        n = min(int(r["iterations"]), int(p.max_iterations))
        out = {k: v[:n] for k, v in rows.items()}
        if not top_k:
            for k in ("top_src", "top_tgt", "top_det"):
                out.pop(k)
        return Tout, r, out

    def align_batch(self, clouds, pairs, T0=None, params=None, debug=False):
        """Many small registrations in one launch (gicp_batch_align): `clouds` a list of N x 2 or
        N x 3 arrays of one dimension, each of 1 .. batch_max_points(dim) rows; `pairs` a list of (source, target)
        cloud numbers (a cloud may serve many pairs); T0 None (identity), one pose, or one per pair.  One
        gicp_params serves the batch; the engine's clouds, caches, voxel and filter settings are neither used nor
        changed.  Returns (T [B, d+1, d+1], results): per pair a dict of status (0, or GICP_E_INVALID = -1 when
        its pose solve failed: it keeps the pose it had, the others are unaffected), iterations, converged,
        converged_at, stop_reason (named as Engine.align names it), correspondences, final_loss, mse.  With
        debug=True also a dict: per cloud 'covariances' and 'neighbor_counts', per pair 'index', 'distance'
        (of the last pass it ran) and 'stats'.  A pair's outputs do not depend on what else is in the batch."""
        cl = [self._cloud(c) for c in clouds]
        if not cl:
            raise ValueError("align_batch: clouds must not be empty")
        d = cl[0].shape[1]
        if any(c.shape[1] != d for c in cl):
            raise ValueError("align_batch: all clouds must have one dimension")
        pr = np.asarray(list(pairs), dtype=np.int64).reshape(-1, 2) if len(pairs) else np.empty((0, 2), np.int64)
        B = len(pr)
        if B < 1:
            raise ValueError("align_batch: pairs must not be empty")
        if T0 is None:
            T0 = np.eye(d + 1)
        T0 = np.asarray(T0, dtype=np.float64)
        if T0.shape == (d + 1, d + 1):
            T0 = np.broadcast_to(T0, (B, d + 1, d + 1))
        if T0.shape != (B, d + 1, d + 1):
            raise ValueError(f"align_batch: T0 must be None, one {d + 1} x {d + 1} pose or one per pair, got shape {T0.shape}")
        if pr.min() < -2 ** 31 or pr.max() >= 2 ** 31:
            raise ValueError("align_batch: a cloud number is out of range")
        xyz = np.ascontiguousarray(np.concatenate(cl, axis=0))
        off = np.zeros(len(cl) + 1, dtype=np.int64)
        np.cumsum([len(c) for c in cl], out=off[1:])
        probs = (_lib.BatchProblem * B)()
        raw = np.frombuffer(probs, dtype=np.dtype([("source", np.int32), ("target", np.int32), ("T0", np.float64, 16)]))
        raw["source"], raw["target"] = pr[:, 0], pr[:, 1]
        raw["T0"][:] = 0.0
        raw["T0"][:, :(d + 1) ** 2] = T0.reshape(B, -1)
        Tout = np.empty((B, d + 1, d + 1))
        res = (_lib.BatchResult * B)()
        p = params or default_params(d)
        dbg = out = None
        if debug:
            rows = int(off[-1])
            ok = (pr >= 0).all() and (pr < len(cl)).all()     # (else the call is refused before it writes)
            nsrc = np.array([len(cl[s]) for s in pr[:, 0]], dtype=np.int64) if ok else np.zeros(B, np.int64)
            out = dict(cov=np.empty((rows, d, d)), cnt=np.empty(rows, dtype=np.int32),
                       index=np.empty(max(1, int(nsrc.sum())), dtype=np.int64), distance=np.empty(max(1, int(nsrc.sum()))),
                       stats=np.empty((B, _lib.MAX_STATS)))
            dbg = _lib.BatchDebug(dptr(out["cov"]), out["cnt"].ctypes.data_as(C.POINTER(C.c_int32)),
                                  out["index"].ctypes.data_as(C.POINTER(C.c_int64)), dptr(out["distance"]), dptr(out["stats"]))
        check(self._lib.gicp_batch_align(self._ctx, d, dptr(xyz), off.ctypes.data_as(C.POINTER(C.c_int64)), len(cl), probs, B,
                                         C.byref(p), dptr(Tout), res, C.byref(dbg) if dbg else None), self._ctx,
              "gicp_batch_align")
        results = []
        for r in res:
            e = {k: getattr(r, k) for k, _ in r._fields_ if k != "pad"}
            e["stop_reason"] = _lib.STOP_REASONS.get(e["stop_reason"], e["stop_reason"])
            results.append(e)
        if not debug:
            return Tout, results
        ps = np.concatenate([[0], np.cumsum(nsrc)])
        ns = stats_size(d)
        return Tout, results, dict(
            covariances=[out["cov"][off[c]:off[c + 1]] for c in range(len(cl))],
            neighbor_counts=[out["cnt"][off[c]:off[c + 1]] for c in range(len(cl))],
            index=[out["index"][ps[b]:ps[b + 1]] for b in range(B)],
            distance=[out["distance"][ps[b]:ps[b + 1]] for b in range(B)],
            stats=[out["stats"][b, :ns] for b in range(B)])


def batch_max_points(dim):
    """The largest cloud align_batch takes (gicp_batch_max_points)."""
    n = _lib.load().gicp_batch_max_points(int(dim))
    if n < 0:
        raise ValueError("batch_max_points: dim must be 2 or 3")
    return n


def align_batch(clouds, pairs, T0=None, params=None, debug=False, device=0, **params_kw):
    """Engine.align_batch on the process's engine of `device`; params_kw are gicp_params fields over the defaults
    (or over `params`), e.g. max_distance_correspondence=20.0."""
    cl = [Engine._cloud(c) for c in clouds]
    if params_kw:
        if not cl:
            raise ValueError("align_batch: clouds must not be empty")
        base = {k: getattr(params, k) for k, _ in Params._fields_} if params is not None else {}
        base.update(params_kw)
        params = default_params(cl[0].shape[1], **base)
    return _engine(int(device)).align_batch(cl, pairs, T0, params, debug)


def pick_start(results):
    """multistart's choice among a list of result dicts: the start with the most correspondences among those
    with status == 0, ties to the smaller mse, then to the lower index; None when every start failed."""
    best = None
    for i, r in enumerate(results):
        if r["status"] != 0:
            continue
        key = (-int(r["correspondences"]), float(r["mse"]))
        if best is None or key < best[0]:
            best = (key, i)
    return None if best is None else best[1]


def multistart(source, target, T0s, **kw):
    """One pair registered from len(T0s) start poses in one launch (a multi-start search over yaw when odometry
    is lost): returns (best, T [B, d+1, d+1], results) with `best` = pick_start(results).  kw as align_batch's."""
    T0s = np.asarray(T0s, dtype=np.float64)
    if T0s.ndim != 3 or len(T0s) < 1:
        raise ValueError(f"multistart: T0s must be B >= 1 poses [B, d+1, d+1], got shape {T0s.shape}")
    T, results = align_batch([source, target], [(0, 1)] * len(T0s), T0s, **kw)[:2]
    return pick_start(results), T, results


def _report_spec(thresholds, quantiles):
    """gicp_report_spec of the two sequences (their lengths are the library's to refuse)."""
    thr = [float(v) for v in thresholds]
    qs = [float(v) for v in quantiles]
    spec = ReportSpec()
    spec.n_thresholds, spec.n_quantiles = len(thr), len(qs)
    for k, v in enumerate(thr[:_lib.REPORT_MAX]):
        spec.thresholds[k] = v
    for k, v in enumerate(qs[:_lib.REPORT_MAX]):
        spec.quantiles[k] = v
    return spec, thr, qs


def _report_dict(rep, thr, qs):
    """The gicp_report as a dict: arrays shaped n x n, the two ratios of the overlap table, quantiles keyed by
    probability."""
    d = int(rep.dim)
    n, nw = (6, 3) if d == 3 else (3, 1)
    nt, nq = int(rep.n_thresholds), int(rep.n_quantiles)
    arr = lambda f, k: np.array(f[:k], dtype=np.float64)
    inl = np.array(rep.inliers[:nt], dtype=np.int64)
    ssq = arr(rep.inlier_sum_sq, nt)
    with np.errstate(invalid="ignore", divide="ignore"):
        fitness = inl / float(rep.n_source) if rep.n_source else np.full(nt, np.nan)
        rmse = np.where(inl > 0, np.sqrt(ssq / np.maximum(inl, 1)), np.nan)
    return dict(
        dim=d, n_source=int(rep.n_source), n_matched=int(rep.n_matched), sum_sq=float(rep.sum_sq), loss=float(rep.loss),
        H=arr(rep.H, n * n).reshape(n, n), b=arr(rep.b, n),
        eig=arr(rep.eig, n), eigvec=arr(rep.eigvec, n * n).reshape(n, n),
        eig_rot=arr(rep.eig_rot, nw), vec_rot=arr(rep.vec_rot, nw * nw).reshape(nw, nw),
        eig_trans=arr(rep.eig_trans, d), vec_trans=arr(rep.vec_trans, d * d).reshape(d, d),
        thresholds=np.array(thr[:nt]), inliers=inl, inlier_sum_sq=ssq, fitness=fitness, inlier_rmse=rmse,
        quantiles=np.array(qs[:nq]),
        dist_q={qs[k]: float(rep.dist_q[k]) for k in range(nq)},
        white_q={qs[k]: float(rep.white_q[k]) for k in range(nq)})


def information(stats, T):
    """(H, b) of a pass's statistics at pose T for the left perturbation T' = Exp(xi) T, xi = (omega, v): the
    Gauss-Newton Hessian sum J^T W J and sum J^T W r, J = [[p]x, -I] (gicp_information, host only).  H is 6 x 6
    (2-D: 3 x 3)."""
    T = np.ascontiguousarray(np.asarray(T, dtype=np.float64))
    d = T.shape[0] - 1
    st = np.ascontiguousarray(np.asarray(stats, dtype=np.float64))
    if T.shape != (d + 1, d + 1) or d not in (2, 3) or st.shape != (stats_size(d),):
        raise ValueError("information: T must be 3 x 3 or 4 x 4 and stats the statistics of that dimension")
    n = 6 if d == 3 else 3
    H = np.empty((n, n))
    b = np.empty(n)
    check(_lib.load().gicp_information(d, dptr(st), dptr(T), dptr(H), dptr(b)), None, "gicp_information")
    return H, b


def sym_eig(A):
    """(w, V) of the symmetric part of A (order <= 6): eigenvalues ascending, V[:, k] the unit eigenvector of
    w[k] (gicp_sym_eig: cyclic Jacobi in fp64, host only)."""
    A = np.ascontiguousarray(np.asarray(A, dtype=np.float64))
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("sym_eig: A must be square")
    n = A.shape[0]
    w = np.empty(n)
    V = np.empty((n, n))
    check(_lib.load().gicp_sym_eig(n, dptr(A), dptr(w), dptr(V)), None, "gicp_sym_eig")
    return w, V


def solve_pose(stats, T_k):
    """Host minimiser of the inner problem from the statistics (gicp_solve_pose)."""
    T_k = np.ascontiguousarray(np.asarray(T_k, dtype=np.float64))
    d = T_k.shape[0] - 1
    st = np.ascontiguousarray(np.asarray(stats, dtype=np.float64))
    out = np.empty_like(T_k)
    loss = C.c_double()
    check(_lib.load().gicp_solve_pose(d, dptr(st), dptr(T_k), dptr(out), C.byref(loss)), None, "gicp_solve_pose")
    return out, loss.value


def _cg_inner(stats, offset, T_k):
    """2-D reference inner solve (gicp.py:148-154): fmin_cg's algorithm (SciPy 1.15.3, restated natively in
    gicp_cg_inner_2d, bit-identical to scipy's own on the same objective: tests/test_cg_native.py) on the
    closed form of the loss from the pass's 26 statistics.  Returns (xopt, fopt)."""
    st = np.ascontiguousarray(stats, dtype=np.float64)
    Tk = np.ascontiguousarray(T_k, dtype=np.float64)
    x0 = np.ascontiguousarray(offset, dtype=np.float64)
    if st.shape != (stats_size(2),) or Tk.shape != (3, 3) or x0.shape != (3,):
        raise ValueError("2-D statistics (26), a 3x3 pose and a 3-vector offset expected")
    x = np.zeros(3)
    fopt = C.c_double()
    check(_lib.load().gicp_cg_inner_2d(dptr(st), dptr(Tk), dptr(x0), dptr(x), C.byref(fopt), None), None,
          "gicp_cg_inner_2d")
    return x, fopt.value


def _loss_2d(x, s, q, W):
    """The reference's loss (gicp.py:52-58) on GPU-produced correspondences q and weights W."""
    r = q - s @ _rot2(x[2]).T - x[:2]
    wr = np.sum(W * r[:, None, :], axis=2)
    return np.sum(r * wr)


def _grad_2d(x, s, q, W):
    """The reference's gradient (gicp.py:60-76)."""
    r = q - s @ _rot2(x[2]).T - x[:2]
    wr = np.sum(W * r[:, None, :], axis=2)
    g = np.zeros(3)
    g[:2] = -2 * np.sum(wr, axis=0)
    dR = np.array([[-np.sin(x[2]), -np.cos(x[2])], [np.cos(x[2]), -np.sin(x[2])]])
    g[2] = np.sum(-2 * (wr.T @ s) * dR)
    return g


def _cg_inner_faithful(src, q, W, offset):
    """fmin_cg on the per-point loss exactly as gicp.py:148-154 evaluates it."""
    from scipy.optimize import fmin_cg

    out = fmin_cg(f=lambda x: _loss_2d(x, src, q, W), x0=offset, fprime=lambda x: _grad_2d(x, src, q, W),
                  disp=False, full_output=True)
    return out[0], out[1]


_ENGINES = {}
_LAST_RESULT = None


def last_result():
    """The gicp_result of the last gicp() call that ran its loop on the device (mode='fast',
    inner='newton'; the first device's): iterations, wall_ms (the library's own wall time of the loop,
    without the clouds' setup and the 7-tuple's assembly), stop reason, ...  None before such a call."""
    return None if _LAST_RESULT is None else dict(_LAST_RESULT)

# 2-D clouds up to this size default to mode='faithful' (scipy fmin_cg on the reference's per-point
# loss, which copies N x 2 x 2 weights to the host every iteration); larger ones to mode='fast'
FAITHFUL_MAX_POINTS = 5000


class RotatedCovariances(Sequence):
    """all_source_cov_matrices of the fast path (gicp.py:120-121,174), held lazily: element k is
    R_k C_s,i R_kᵀ for every source point (rigid invariance), R_k the rotation of
    iteration k.  Only the initial covariances and the rotations are stored; an element is computed
    on the host when read (always the same formula, so a re-read is bit-identical whatever the engine
    did meanwhile), and the last two elements read are kept, so the reference's per-point access
    `all_source_cov_matrices[step][i]` (visualization.py:158) costs one computation per step.  Holds no
    engine: picklable (e.g. through the multiprocessing Queue of robot-visualization.py:153,166).
    Behaves as the reference's list for len / indexing / iteration."""

    _CACHE = 2

    def __init__(self, init_cov, rotations=()):
        self._init = init_cov
        self._R = [np.array(R, dtype=np.float64) for R in rotations]
        self._cache = {}
        self.computed = 0   # elements materialised so far (a test bounds it)

    def append_rotation(self, R):
        self._R.append(np.array(R, dtype=np.float64))

    def __len__(self):
        return len(self._R)

    def _one(self, k):
        hit = self._cache.get(k)
        if hit is not None:
            return hit
        R = self._R[k]
        out = np.matmul(np.matmul(R, self._init), R.T)
        self.computed += 1
        if len(self._cache) >= self._CACHE:
            self._cache.pop(next(iter(self._cache)))
        self._cache[k] = out
        return out

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self._one(i) for i in range(len(self._R))[k]]
        k = range(len(self._R))[k]   # negative indices, IndexError as a list
        return self._one(k)

    def __getstate__(self):
        return {"init": self._init, "R": self._R}

    def __setstate__(self, st):
        self._init = st["init"]
        self._R = st["R"]
        self._cache = {}
        self.computed = 0

    def __repr__(self):
        return f"RotatedCovariances({len(self)} iterations x {len(self._init)} points)"


_NO_FILTER = dict(center=None, min_range=0.0, max_range=0.0, radius=0.0, min_neighbors=1)


def _filter_kw(center, min_range, max_range, radius, min_neighbors):
    """The keywords of Engine.set_filter, normalised (None: the default of each)."""
    return dict(center=None if center is None else tuple(float(v) for v in np.asarray(center, dtype=np.float64).ravel()),
                min_range=0.0 if min_range is None else float(min_range),
                max_range=0.0 if max_range is None else float(max_range),
                radius=0.0 if radius is None else float(radius), min_neighbors=int(min_neighbors))


def _filter_on(kw):
    return kw["min_range"] > 0 or kw["max_range"] > 0 or kw["radius"] > 0


def _filter_struct(kw, dim):
    """gicp_filter of the keywords; dim: the cloud's dimension the centre must have (None: 2 or 3 values)."""
    f = _lib.Filter()
    c = kw["center"]
    if c is not None:
        if len(c) not in ((2, 3) if dim is None else (dim,)):
            raise ValueError(f"center must hold {'2 or 3' if dim is None else dim} values, got {len(c)}")
        for k, v in enumerate(c):
            f.center[k] = v
    f.min_range, f.max_range, f.radius = kw["min_range"], kw["max_range"], kw["radius"]
    f.min_neighbors = kw["min_neighbors"]
    return f


def _filter_call(call, a, f, return_index, return_counts):
    """One one-shot filter call (device or host) on the cloud `a`: the kept rows, then what was asked for."""
    out = np.empty_like(a)
    idx = np.empty(a.shape[0], dtype=np.int64) if return_index else None
    cnt = np.empty(a.shape[0], dtype=np.int32) if return_counts else None
    m = C.c_int64()
    call(dptr(a), a.shape[0], a.shape[1], C.byref(f), dptr(out),
         idx.ctypes.data_as(C.POINTER(C.c_int64)) if return_index else None,
         cnt.ctypes.data_as(C.POINTER(C.c_int32)) if return_counts else None, C.byref(m))
    res = (out[:m.value].copy(),)
    if return_index:
        res += (idx[:m.value].copy(),)
    if return_counts:
        res += (cnt,)
    return res[0] if len(res) == 1 else res


def _engine(device):
    eng = _ENGINES.get(device)
    if eng is None:
        eng = _ENGINES[device] = Engine(device)
    return eng


def voxel_downsample(points, voxel_size, min_points=1, return_counts=False, device=0):
    """Voxel-grid downsampling on the GPU (gicp_voxel_downsample): one centroid per occupied cell of the
    absolute grid floor(x / voxel_size), cells with fewer than min_points points dropped, in ascending
    lexicographic order of the cells (the order of np.unique(cells, axis=0)).  N x 2 or N x 3 in, M x dim
    out; with return_counts also the int32 number of points behind each centroid.  Deterministic: the same
    input gives the same bits on every call and every GPU.  Raises ValueError for a voxel_size that is
    not finite and positive, non-finite points, a cloud spanning more than 2^21 (3-D) / 2^31 (2-D) cells
    along an axis, and when no cell reaches min_points."""
    return _engine(int(device)).voxel_downsample(points, voxel_size, min_points, return_counts)


def filter_points(points, center=None, min_range=0.0, max_range=0.0, radius=0.0, min_neighbors=1, return_index=False,
                  return_counts=False, device=0):
    """Range crop and radius outlier removal on the GPU (gicp_filter_points): keep the rows of
    `points` (N x 2 or N x 3) with min_range <= |p - center| <= max_range (0: no limit; center None: the origin),
    then, among those, the rows with at least min_neighbors others within `radius` (inclusive; 0: off).  The
    decisions are those of the fp64 expression d2 = ((dx*dx + dy*dy) + dz*dz) against the squared bounds, every
    operation rounded on its own, so NumPy's restatement gives the same rows.  Returns the kept rows in their
    order; with return_index also their int64 rows in `points`; with return_counts also, per INPUT row, the int32
    number of neighbours (-1 where the crop removed the row; 0 for kept rows without a radius).  Deterministic.
    Raises ValueError for non-finite input or fields, negative ranges, min_range > max_range > 0,
    min_neighbors < 1 with a radius, a stage that leaves no row, and a cropped cloud spanning more than 2^21
    (3-D) / 2^31 (2-D) cells of edge radius along an axis (crop far returns with max_range first)."""
    return _engine(int(device)).filter_points(points, center, min_range, max_range, radius, min_neighbors, return_index,
                                              return_counts)


def filter_points_host(points, center=None, min_range=0.0, max_range=0.0, radius=0.0, min_neighbors=1, return_index=False,
                       return_counts=False):
    """`filter_points` computed on the host by the same predicates (gicp_filter_points_host; no GPU needed): the
    CPU yardstick, a plain loop."""
    a = Engine._cloud(points)
    f = _filter_struct(_filter_kw(center, min_range, max_range, radius, min_neighbors), a.shape[1])
    lib = _lib.load()

    def call(*args):
        rc = lib.gicp_filter_points_host(*args)
        if rc != _lib.GICP_OK:   # (host only: the message is the thread's, there is no context)
            raise ValueError(lib.gicp_last_host_error().decode())

    return _filter_call(call, a, f, return_index, return_counts)


def _sor_call(call, a, k, std_ratio, return_index, return_mean, return_stats):
    """One one-shot statistical-outlier-removal call (device or host) on the cloud `a`."""
    s = _lib.Sor(int(k), 0, float(std_ratio))
    out = np.empty_like(a)
    idx = np.empty(a.shape[0], dtype=np.int64) if return_index else None
    mean = np.empty(a.shape[0], dtype=np.float64) if return_mean else None
    stats = np.empty(3, dtype=np.float64) if return_stats else None
    m = C.c_int64()
    call(dptr(a), a.shape[0], a.shape[1], C.byref(s), dptr(out),
         idx.ctypes.data_as(C.POINTER(C.c_int64)) if return_index else None,
         dptr(mean) if return_mean else None, dptr(stats) if return_stats else None, C.byref(m))
    res = (out[:m.value].copy(),)
    if return_index:
        res += (idx[:m.value].copy(),)
    if return_mean:
        res += (mean,)
    if return_stats:
        res += (dict(mu=float(stats[0]), sigma=float(stats[1]), threshold=float(stats[2])),)
    return res[0] if len(res) == 1 else res


def sor_max_k():
    """The largest k of `sor_points` (gicp_sor_max_k): knn_max_k() - 1."""
    return int(_lib.load().gicp_sor_max_k())


def sor_points(points, k, std_ratio=1.0, return_index=False, return_mean=False, return_stats=False, device=0):
    """Statistical outlier removal on the GPU (gicp_sor_points): keep the rows of `points` (N x 2 or
    N x 3, N >= 2) whose mean distance to their k nearest other rows is at most mu + std_ratio sigma, where mu is the
    mean and sigma the sample deviation of those means over the cloud.  Defined to the bit (include/gicp_hip.h): fp64,
    every operation rounded on its own, the mean a sequential sum of the roots of the ascending d2 and one division,
    mu and sigma from pairwise tree sums in row order, the bound inclusive -- NumPy's restatement gives the same rows.
    Returns the kept rows in their order; with return_index also their int64 rows in `points`; with return_mean also,
    per INPUT row, the float64 mean neighbour distance; with return_stats also dict(mu, sigma, threshold).
    Deterministic.  Raises ValueError for k outside 1..sor_max_k(), a negative or non-finite std_ratio, fewer than 2
    rows, non-finite input, and a call that leaves no row."""
    return _engine(int(device)).sor_points(points, k, std_ratio, return_index, return_mean, return_stats)


def sor_points_host(points, k, std_ratio=1.0, return_index=False, return_mean=False, return_stats=False):
    """`sor_points` computed on the host by the same functions over a brute-force search (gicp_sor_points_host; no
    GPU needed): the CPU yardstick, quadratic in the number of rows."""
    a = Engine._cloud(points)
    lib = _lib.load()

    def call(*args):
        rc = lib.gicp_sor_points_host(*args)
        if rc != _lib.GICP_OK:   # (host only: the message is the thread's, there is no context)
            raise ValueError(lib.gicp_last_host_error().decode())

    return _sor_call(call, a, k, std_ratio, return_index, return_mean, return_stats)


def _cluster_call(call, a, radius, min_size, max_size, return_index, return_labels, return_sizes):
    """One one-shot cluster-extraction call (device or host) on the cloud `a`."""
    c = _lib.Cluster(float(radius), int(min_size), int(max_size))
    n = a.shape[0]
    out = np.empty_like(a)
    idx = np.empty(n, dtype=np.int64) if return_index else None
    labels = np.empty(n, dtype=np.int32) if return_labels else None
    sizes = np.empty(n, dtype=np.int32) if return_sizes else None
    m, nc = C.c_int64(), C.c_int64()
    i32 = C.POINTER(C.c_int32)
    call(dptr(a), n, a.shape[1], C.byref(c), labels.ctypes.data_as(i32) if return_labels else None,
         sizes.ctypes.data_as(i32) if return_sizes else None, C.byref(nc), dptr(out),
         idx.ctypes.data_as(C.POINTER(C.c_int64)) if return_index else None, C.byref(m))
    res = (out[:m.value].copy(),)
    if return_index:
        res += (idx[:m.value].copy(),)
    if return_labels:
        res += (labels,)
    if return_sizes:
        res += (sizes[:nc.value].copy(),)
    return res[0] if len(res) == 1 else res


def cluster_points(points, radius, min_size=1, max_size=0, return_index=False, return_labels=False, return_sizes=False,
                   device=0):
    """Euclidean cluster extraction on the GPU (gicp_cluster_points): rows i != j of `points` (N x 2 or
    N x 3, N >= 1) are adjacent iff d2 = ((dx*dx + dy*dy) + dz*dz) <= radius*radius in fp64, every operation rounded on
    its own and the bound inclusive (coincident rows are adjacent); the clusters are the connected components,
    numbered 0 .. C - 1 in ascending order of their smallest row; a cluster is kept iff min_size <= size and
    (max_size == 0 or size <= max_size).  Defined to the bit (include/gicp_hip.h): the host function and a NumPy /
    SciPy restatement give the same arrays.  Returns the rows of the kept clusters in their order; with return_index
    also their int64 rows in `points`; with return_labels also, per INPUT row, the int32 number of its cluster (kept
    or not); with return_sizes also the int32 sizes of the C clusters.  Deterministic.  Raises ValueError for a radius
    that is not finite and > 0, min_size < 1, max_size below min_size (0: no limit), non-finite input, a cloud spanning
    more than 2^21 (3-D) / 2^31 (2-D) cells of edge radius on an axis, and a decision that keeps no row."""
    return _engine(int(device)).cluster_points(points, radius, min_size, max_size, return_index, return_labels, return_sizes)


def cluster_points_host(points, radius, min_size=1, max_size=0, return_index=False, return_labels=False, return_sizes=False):
    """`cluster_points` computed on the host by a union-find over the same grid and predicate
    (gicp_cluster_points_host; no GPU needed): the CPU yardstick."""
    a = Engine._cloud(points)
    lib = _lib.load()

    def call(*args):
        rc = lib.gicp_cluster_points_host(*args)
        if rc != _lib.GICP_OK:   # (host only: the message is the thread's, there is no context)
            raise ValueError(lib.gicp_last_host_error().decode())

    return _cluster_call(call, a, radius, min_size, max_size, return_index, return_labels, return_sizes)


def _knn_array(a, name):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if a.ndim != 2:
        raise ValueError(f"{name} must be a 2-D array of rows, got shape {a.shape}")
    return a


def _knn_call(call, q, nq, dim, k, max_distance, squared):
    """One kNN entry point: `call` takes (queries, Q, dim, k, max_distance, index, dist2, count) after its own
    leading arguments and raises if the library refuses; the outputs are allocated once the sizes are plausible."""
    k = int(k)
    rows = max(int(nq), 1) if 1 <= k <= knn_max_k() else 1
    idx = np.empty((rows, max(k, 1)), dtype=np.int64)
    d2 = np.empty((rows, max(k, 1)))
    call(dptr(q) if q is not None else None, int(nq), int(dim), k, 0.0 if max_distance is None else float(max_distance),
         idx.ctypes.data_as(C.POINTER(C.c_int64)), dptr(d2), None)
    return idx, (d2 if squared else np.sqrt(d2))


def knn_max_k():
    """The largest k of `knn` (gicp_knn_max_k)."""
    return int(_lib.load().gicp_knn_max_k())


def knn(points, queries=None, k=1, max_distance=None, squared=False, device=0):
    """Exact k nearest neighbours on the GPU (gicp_knn_points): for every row of `queries` (Q x dim;
    None: the rows of `points` themselves) the k rows of `points` (M x 2 or M x 3) nearest to it.  The distance is
    the fp64 expression d2 = ((dx*dx + dy*dy) + dz*dz), every operation rounded on its own; rows are ordered by
    (d2, row), so exactly equal distances go to the smaller row -- the library's own rule, not a KD-tree's.
    max_distance None or 0: no limit, else only rows with d2 <= max_distance**2 count.  Returns (index [Q, k] int64
    padded with -1, distance [Q, k] float64 padded with inf); squared=True returns d2 itself.  Deterministic.
    Raises ValueError for k outside 1..knn_max_k(), non-finite input, an empty array and a negative or non-finite
    max_distance."""
    return _engine(int(device)).knn_points(points, queries, k, max_distance, squared)


def knn_host(points, queries=None, k=1, max_distance=None):
    """`knn` computed on the host by a brute force over all pairs (gicp_knn_host; no GPU needed): the CPU
    yardstick.  Returns (index, d2): always the squared distances."""
    a = _knn_array(points, "points")
    q = None if queries is None else _knn_array(queries, "queries")
    if q is not None and q.shape[1] != a.shape[1]:
        raise ValueError(f"queries must be Q x {a.shape[1]} as the points, got shape {q.shape}")
    lib = _lib.load()

    def call(*args):
        rc = lib.gicp_knn_host(dptr(a), a.shape[0], *args)
        if rc != _lib.GICP_OK:   # (host only: the message is the thread's, there is no context)
            raise ValueError(lib.gicp_last_host_error().decode())

    return _knn_call(call, q, a.shape[0] if q is None else q.shape[0], a.shape[1], k, max_distance, True)


def deskew(points, stamps, motion, ref=0.0, device=0):
    """Motion compensation of a sweep on the GPU (gicp_deskew): `points` (N x 2 or N x 3) were
    measured one by one while the sensor moved, point i at stamp `stamps[i]`; `motion` is the rigid
    (dim+1) x (dim+1) transform of the sensor over one stamp unit, expressed in the sensor frame,
    P(tau)^-1 P(tau + 1).  Returns the points as seen from the sensor frame at stamp `ref` under constant twist:
    p'_i = Exp((stamps[i] - ref) Log(motion)) p_i, in fp64, rows in their order.  Deterministic: the same bits
    on every call and GPU, and the rows Engine.set_target(..., stamps=, motion=, ref=) indexes.  Raises
    ValueError for non-finite input, a motion that is not rigid (max|R^T R - I| > 1e-9) or that rotates by more
    than a quarter turn per stamp unit."""
    return _engine(int(device)).deskew(points, stamps, motion, ref)


def motion_twist(motion):
    """The twist Log(motion) of a rigid (dim+1) x (dim+1) motion (gicp_motion_twist, host only): 3-D
    (w_x, w_y, w_z, v_x, v_y, v_z), 2-D (w, v_x, v_y); ValueError for a motion `deskew` would refuse."""
    M = np.ascontiguousarray(np.asarray(motion, dtype=np.float64))
    if M.ndim != 2 or M.shape[0] != M.shape[1] or M.shape[0] not in (3, 4):
        raise ValueError(f"motion must be 3 x 3 or 4 x 4, got shape {M.shape}")
    d = M.shape[0] - 1
    xi = np.empty(3 if d == 2 else 6)
    check(_lib.load().gicp_motion_twist(d, dptr(M), dptr(xi)), None, "gicp_motion_twist")
    return xi


def deskew_host(points, stamps, motion, ref=0.0):
    """`deskew` computed on the host by the same per-point function (gicp_deskew_host; no GPU needed)."""
    a = Engine._cloud(points)
    _sw, st = Engine._sweep(a, stamps, motion, ref)
    M = np.ascontiguousarray(np.asarray(motion, dtype=np.float64))
    out = np.empty_like(a)
    check(_lib.load().gicp_deskew_host(dptr(a), dptr(st), a.shape[0], a.shape[1], dptr(M), float(ref), dptr(out)), None,
          "gicp_deskew_host")
    return out


def _devices(device, devices):
    """The GPUs a gicp() call runs on: [device], or the distinct entries of `devices`."""
    if devices is None:
        return [int(device)]
    devs = [int(x) for x in devices]
    if not devs:
        raise ValueError("devices must name at least one GPU")
    if len(set(devs)) != len(devs):
        raise ValueError(f"devices lists a GPU more than once: {devs}")
    return devs


class _ThreadSum:
    """Statistics exchange of a multi-device gicp() call (one host thread per GPU): every rank's
    buffer in, the sum in rank order out -- the same bits on every rank, so every device's solve and
    convergence test agree.  A failing rank aborts the barrier and the others raise instead of waiting."""

    def __init__(self, world, timeout=300.0):
        import threading
        self.world = world
        self.slots = [None] * world
        self.bar = threading.Barrier(world, timeout=timeout)

    def __call__(self, rank, buf):
        self.slots[rank] = np.array(buf, dtype=np.float64)
        self.bar.wait()
        total = self.slots[0].copy()
        for r in range(1, self.world):
            total += self.slots[r]
        self.bar.wait()
        return total

    def abort(self):
        self.bar.abort()


def _run_ranks(engines, fn):
    """fn(rank, engine) on one thread per engine (ctypes releases the GIL inside the library);
    returns the results in rank order, re-raising the first failure."""
    if len(engines) == 1:
        return [fn(0, engines[0])]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(len(engines)) as ex:
        futs = [ex.submit(fn, r, e) for r, e in enumerate(engines)]
        return [f.result() for f in futs]


def _merge_top(rows, k=5):
    """The k largest det(W) over the ranks' top-k rows, ascending as np.argsort(det)[-k:] orders them
    (equal dets: larger original index last).  rows: [(src, tgt, det), ...] per rank."""
    src = np.concatenate([r[0] for r in rows])
    tgt = np.concatenate([r[1] for r in rows])
    det = np.concatenate([r[2] for r in rows])
    ok = src >= 0
    src, tgt, det = src[ok], tgt[ok], det[ok]
    order = np.lexsort((src, det))[-k:]
    return src[order], tgt[order], det[order]


def pcl_stop(T_old, T_new, mse, prev_mse, transformation_epsilon=0.0, rotation_epsilon=0.0,
             euclidean_fitness_epsilon=0.0, mse_relative_epsilon=0.0):
    """PCL-style stopping test after an update (the criteria the reference's ROS experiment set,
    presentation/main.typ:773-776; same order and semantics as k_solve): the increment
    dT = T_new T_old^-1 with |dt|^2 <= transformation_epsilon and cos(angle) >= rotation threshold
    (1 - transformation_epsilon when rotation_epsilon is 0), else |mse - prev| < euclidean_fitness_epsilon,
    else |mse - prev| / prev < mse_relative_epsilon.  Returns 'transform' / 'abs_mse' / 'rel_mse' / None."""
    d = T_old.shape[0] - 1
    dR = T_new[:d, :d] @ T_old[:d, :d].T
    dt = T_new[:d, d] - dR @ T_old[:d, d]
    tr = float(np.trace(dR))
    cosang = 0.5 * (tr - 1.0) if d == 3 else 0.5 * tr
    rot_cos = rotation_epsilon if rotation_epsilon > 0 else 1.0 - transformation_epsilon
    dm = abs(mse - prev_mse)
    if transformation_epsilon > 0 and cosang >= rot_cos and float(dt @ dt) <= transformation_epsilon:
        return "transform"
    if euclidean_fitness_epsilon > 0 and dm < euclidean_fitness_epsilon:
        return "abs_mse"
    if mse_relative_epsilon > 0 and np.isfinite(prev_mse) and dm / prev_mse < mse_relative_epsilon:
        return "rel_mse"
    return None


def gicp(source_points, target_points, max_iterations=100, tolerance=1e-6, max_distance_correspondence=150,
         max_distance_nearest_neighbors=50, *, full_output=True, mode=None, inner=None, k_neighbors=None, device=0,
         devices=None, verbose=True, T0=None, method="plane_to_plane", transformation_epsilon=0.0,
         rotation_epsilon=0.0, euclidean_fitness_epsilon=0.0, mse_relative_epsilon=0.0, voxel_size=None,
         voxel_min_points=1, robust_kernel=None, robust_scale=None, min_range=None, max_range=None, outlier_radius=None,
         outlier_min_neighbors=1, filter_center=None, sor_k=None, sor_std_ratio=1.0, cluster_radius=None,
         cluster_min_size=1, cluster_max_size=0):
    """Drop-in for gicp.py:78 — returns the same 7-tuple (gicp.py:174):

    (T, all_transformations, initial_source_cov_matrices, target_cov_matrices,
     highest_weight_points_source, highest_weight_points_target, all_source_cov_matrices)

    2-D and 3-D clouds (T is 3x3 or 4x4).

    mode='faithful' (default for 2-D clouds of <= FAITHFUL_MAX_POINTS source points): every
      iteration the GPU recomputes the source covariances on the transformed source
      (gicp.py:120) and produces the correspondences and weights; scipy's fmin_cg then
      minimises the reference's own per-point loss on them (gicp.py:148-154), so the
      inexact inner stop follows the reference's trajectory.
    mode='fast' (3-D default, and larger 2-D clouds): source covariances are
      rotated (rigid invariance), the GPU reduces the loss to its sufficient
      statistics in one pass, and the inner problem is solved from them -- exactly by
      Newton on SO(d) (inner='newton', the 3-D default: the whole loop then runs on the
      device in one gicp_align_trace call, the 7-tuple's per-iteration rows recorded there),
      or by conjugate gradients on the closed form (inner='cg', the 2-D default, host loop): the
      native gicp_cg_inner_2d, a C++ restatement of SciPy 1.15.3's fmin_cg pinned bit for bit
      against scipy's own on the same closed form (tests/test_cg_native.py).
    full_output=False skips the per-point visualisation extras (the three
    lists come back empty), which is what large clouds want.  In 'fast' mode the
    top-5 det(W) points are selected on the GPU (no per-point copy) and
    all_source_cov_matrices is a RotatedCovariances view (computed when read).

    device / devices: the GPU, or a list of distinct GPUs; with several, every GPU holds
      both clouds and reduces its shard of the source, one host thread drives each, and the
      statistics are summed over them every iteration in device order (the same sum on every
      GPU, so all take the same step).  mode='faithful' runs on the first listed GPU.
    method: 'plane_to_plane' (GICP, the reference), 'point_to_point' (ICP: C_s = 0,
      C_t = I) or 'point_to_plane' (C_s = 0, C_t = P^-1), presentation/main.typ:446-455.
    transformation_epsilon / rotation_epsilon / euclidean_fitness_epsilon /
      mse_relative_epsilon: optional PCL-style stopping criteria (see pcl_stop), tested
      after the update; 0 disables each.  tolerance=0 disables the reference's rule.
    voxel_size / voxel_min_points: None (default) registers the clouds as given.  Otherwise both are
      first reduced on the device to one centroid per voxel_size cell holding at least voxel_min_points
      points (voxel_downsample), and every per-point member of the 7-tuple -- the covariance arrays, the
      highest-weight points, all_source_cov_matrices -- refers to the FILTERED clouds, whose lengths
      differ from the inputs'.
    min_range / max_range / outlier_radius / outlier_min_neighbors / filter_center: all None (default) registers
      the clouds as given.  Otherwise both clouds first pass the input filters on the device
      (Engine.set_filter: a range crop about filter_center, None the origin, then radius outlier removal), before
      the voxel filter if voxel_size is given, and every per-point member of the 7-tuple -- the covariance
      arrays, the highest-weight points, all_source_cov_matrices -- refers to the FILTERED clouds.
    sor_k / sor_std_ratio: sor_k None (default) registers the clouds as given.  Otherwise both clouds pass
      statistical outlier removal on the device (Engine.set_sor) after the input filters and before the voxel
      filter, and every per-point member of the 7-tuple refers to the FILTERED clouds.
    cluster_radius / cluster_min_size / cluster_max_size: cluster_radius None (default) registers the clouds as
      given.  Otherwise both clouds pass Euclidean cluster extraction on the device (Engine.set_cluster) after
      statistical outlier removal and before the voxel filter: only the rows of the clusters whose size lies in
      the limits stay, and every per-point member of the 7-tuple refers to the FILTERED clouds.
    robust_kernel / robust_scale: None (default) is plain least squares.  'huber', 'cauchy',
      'geman_mcclure' ('gm') or 'tukey' (or the GICP_ROBUST_* code) weights every accepted
      correspondence of a pass by the kernel's w(s / robust_scale), s = sqrt(r^T W r) the whitened residual
      at the pass's pose (include/gicp_hip.h): iteratively re-weighted least squares, so a moved object or
      a structure seen in one cloud only no longer pulls the pose.  robust_scale is in units of s: metres
      for 'point_to_point', about |r . n| / sqrt(20) for 'plane_to_plane'.  mode='fast' only (either inner
      solver, one or several devices; the default mode of a call that names a kernel); the reference has no
      such weights, so mode='faithful' refuses it.
    """
    src = Engine._cloud(source_points)
    tgt = Engine._cloud(target_points)
    d = src.shape[1]
    if tgt.shape[1] != d:
        raise ValueError("source and target must have the same dimension")
    robust = _robust_code(robust_kernel)
    if mode is None:
        mode = "faithful" if d == 2 and len(src) <= FAITHFUL_MAX_POINTS and not robust else "fast"
    if mode not in ("faithful", "fast") or (mode == "faithful" and d != 2):
        raise ValueError("mode must be 'fast', or 'faithful' for 2-D clouds")
    inner = ("cg" if d == 2 else "newton") if inner is None else inner
    if inner not in ("cg", "newton") or (inner == "cg" and d != 2):
        raise ValueError("inner must be 'newton', or 'cg' for 2-D clouds")
    if method not in _lib.COV_MODELS:
        raise ValueError(f"method must be one of {sorted(set(_lib.COV_MODELS))}")
    if robust and mode == "faithful":
        raise ValueError("robust_kernel needs mode='fast': mode='faithful' replays the reference, which has no such weights")
    if robust and not (robust_scale is not None and np.isfinite(robust_scale) and robust_scale > 0):
        raise ValueError(f"robust_scale must be finite and > 0 with a robust kernel, got {robust_scale!r}")
    devs = _devices(device, devices)
    if mode == "faithful":
        devs = devs[:1]
    engines = [_engine(x) for x in devs]
    G = len(engines)
    p = default_params(d, max_iterations=int(max_iterations), tolerance=float(tolerance),
                       max_distance_correspondence=float(max_distance_correspondence),
                       max_distance_nearest_neighbors=float(max_distance_nearest_neighbors), k_neighbors=k_neighbors,
                       cov_model=_lib.COV_MODELS[method], robust_kernel=robust,
                       robust_scale=None if robust_scale is None else float(robust_scale))
    pcl = dict(transformation_epsilon=float(transformation_epsilon), rotation_epsilon=float(rotation_epsilon),
               euclidean_fitness_epsilon=float(euclidean_fitness_epsilon),
               mse_relative_epsilon=float(mse_relative_epsilon))

    def build(r, e):
        e.set_target(tgt, p)
        e.set_source(src, p, shard=r, nshards=G)

    filt = None
    if not (min_range is None and max_range is None and outlier_radius is None):
        filt = _filter_kw(filter_center, min_range, max_range, outlier_radius, outlier_min_neighbors)
    if voxel_size is None and filt is None and sor_k is None and cluster_radius is None:
        _run_ranks(engines, build)
        eng = engines[0]
    else:   # the engines are shared between calls: the settings last for this call's builds only
        prev_voxel = [e.voxel for e in engines]
        prev_filter = [e.filter for e in engines]
        prev_sor = [e.sor for e in engines]
        prev_cluster = [e.cluster for e in engines]
        try:
            for e in engines:
                if voxel_size is not None:
                    e.set_voxel(voxel_size, voxel_min_points)
                if filt is not None:
                    e.set_filter(**filt)
                if sor_k is not None:
                    e.set_sor(sor_k, sor_std_ratio)
                if cluster_radius is not None:
                    e.set_cluster(cluster_radius, cluster_min_size, cluster_max_size)
            _run_ranks(engines, build)
            eng = engines[0]
            # the host side of the loops (highest-weight points, the faithful mode's moved source) works on
            # the clouds the engine registers
            src, tgt = eng.points("source"), eng.points("target")
        finally:
            for e, v, f, s, cl in zip(engines, prev_voxel, prev_filter, prev_sor, prev_cluster):
                e.set_voxel(*v)
                e.set_filter(**f)
                e.set_sor(*s)
                e.set_cluster(*cl)
    target_cov = eng.covariances("target")
    init_src_cov = eng.covariances("source")
    for e in engines[1:]:   # each device computed its own shard's source covariances (NaN elsewhere)
        other = e.covariances("source")
        miss = np.isnan(init_src_cov[:, 0, 0])
        init_src_cov[miss] = other[miss]
    T = np.eye(d + 1) if T0 is None else np.array(T0, dtype=np.float64)
    if mode == "fast" and inner == "newton":
        for k, v in pcl.items():
            setattr(p, k, v)
        return _device_loop(engines, src, tgt, T, p, full_output, verbose, init_src_cov, target_cov)
    return _host_loop(engines, src, tgt, T, T0, p, pcl, mode, inner, full_output, verbose, init_src_cov, target_cov)


def _device_loop(engines, src, tgt, T, p, full_output, verbose, init_src_cov, target_cov):
    """gicp.py:116-172 as ONE gicp_align_trace call per GPU: the loop, the solve and the convergence
    test run on the device; the per-iteration rows the 7-tuple needs (poses, top-5 det(W)) are recorded
    there and copied out once."""
    d = src.shape[1]
    G = len(engines)
    k = 5 if full_output else 0
    xchg = _ThreadSum(G) if G > 1 else None
    if xchg is not None:   # installing this call's hook would tear down an RCCL communicator or peer exchange
        own = [e.comm_ranks()[2] for e in engines]
        if any(k in ("rccl", "peer") for k in own):
            raise ValueError(f"gicp(devices=...): the cached engines carry their own statistics exchange ({own}); "
                             "a multi-device call needs engines without one (close it, or use distributed.align)")
    prev = [e._hook_fn for e in engines]   # a hook the caller installed on the cached engines
    if xchg is not None:
        for r, e in enumerate(engines):
            e.set_allreduce(lambda buf, r=r: xchg(r, buf), nranks=G, rank=r)

    def run(r, e):
        try:
            return e.align(T, p, trace=True, top_k=k)
        except BaseException:
            if xchg is not None:
                xchg.abort()
            raise

    try:
        outs = _run_ranks(engines, run)
    finally:
        if xchg is not None:   # restore what was there before this call
            for e, h in zip(engines, prev):
                e.set_allreduce(*h) if h is not None else e.set_allreduce(None)
    T_fin, res, tr = outs[0]
    global _LAST_RESULT
    _LAST_RESULT = dict(res)
    iters = int(res["iterations"])
    poses = tr["poses"]
    loss_stop = bool(res["converged"]) and res["stop_reason"] == "loss"
    if res["converged"] and verbose:
        if loss_stop:
            print("Converged at iteration", res["converged_at"])                 # gicp.py:161
        else:
            print("Converged at iteration", res["converged_at"], f"({res['stop_reason']})")
    all_T = [T] + [poses[i].copy() for i in range(1, iters)]
    if iters > 0 and not loss_stop:                                            # gicp.py:166-167
        all_T.append(T_fin)
    hw_s, hw_t = [], []
    all_src_cov = []
    if full_output:
        all_src_cov = RotatedCovariances(init_src_cov, [poses[i][:d, :d] for i in range(iters)])   # gicp.py:121
        for i in range(iters - 1 if loss_stop else iters):                      # gicp.py:169-172
            rows = [(o[2]["top_src"][i], o[2]["top_tgt"][i], o[2]["top_det"][i]) for o in outs]
            top_s, top_t, _ = _merge_top(rows) if G > 1 else rows[0]
            hw_s.append(apply_transformation(src[top_s[top_s >= 0]], poses[i]))
            hw_t.append(_targets(tgt, top_s, top_t, d))
    return T_fin, all_T, init_src_cov, target_cov, hw_s, hw_t, all_src_cov


def _targets(tgt, top_s, top_t, d):
    """corresponding_target_points rows of the selected points (gicp.py:140; zeros where rejected)."""
    ok = top_s >= 0
    qt = np.zeros((int(ok.sum()), d))
    m = top_t[ok] >= 0
    qt[m] = tgt[top_t[ok][m]]
    return qt


def _host_loop(engines, src, tgt, T, T0, p, pcl, mode, inner, full_output, verbose, init_src_cov, target_cov):
    """gicp.py:116-172 with the inner solve on the host: faithful mode, and fast mode with inner='cg'."""
    d = src.shape[1]
    G = len(engines)
    eng = engines[0]
    use_pcl = any(v > 0 for k, v in pcl.items() if k != "rotation_epsilon")
    prev_mse = np.inf
    all_T = [T]
    offset = np.array([T[0, 2], T[1, 2], np.arctan2(T[1, 0], T[0, 0])]) if d == 2 else None
    last = np.inf
    hw_s, hw_t = [], []
    all_src_cov = [] if (mode == "faithful" or not full_output) else RotatedCovariances(init_src_cov)
    eye = np.eye(d + 1)
    moved_source = False   # faithful mode: the engine holds a transformed copy of the source
    for it in range(int(p.max_iterations)):
        if mode == "faithful":
            moved = apply_transformation(src, T)                   # gicp.py:119
            if it > 0 or T0 is not None:
                eng.set_source(moved, p)                           # gicp.py:120, on the GPU
                moved_source = True
            cs = eng.covariances("source") if moved_source else init_src_cov
            if full_output:
                all_src_cov.append(cs)
            _, dbg = eng.iterate(eye, debug=True)                  # gicp.py:124-145 on the moved cloud
            idx = dbg["index"]
            q = np.zeros_like(src)
            q[idx >= 0] = tgt[idx[idx >= 0]]
            if inner == "cg":
                new_offset, min_loss = _cg_inner_faithful(src, q, dbg["weight"], offset)
                T_new = _offset_to_T(new_offset)
            else:
                T_new, min_loss = _newton_from_points(src, q, dbg["weight"], idx, T)
                new_offset = None
        else:
            if full_output:                                        # gicp.py:170 on the device
                outs = _run_ranks(engines, lambda r, e: e.iterate_top(T, 5))
                top_s, top_t, _ = _merge_top([o[1:] for o in outs]) if G > 1 else outs[0][1:]
                all_src_cov.append_rotation(T[:d, :d])            # gicp.py:120-121, read lazily
            else:
                outs = [(o,) for o in _run_ranks(engines, lambda r, e: e.iterate(T))]
            st = outs[0][0].copy()
            for o in outs[1:]:                                     # rank order: deterministic
                st += o[0]
            if inner == "cg":
                new_offset, min_loss = _cg_inner(st, offset, T)
                T_new = _offset_to_T(new_offset)
            else:
                T_new, min_loss = solve_pose(st, T)
                new_offset = None
        if abs(last - min_loss) < p.tolerance:                     # gicp.py:155-162
            if verbose:
                print("Converged at iteration", it)
            break
        last = min_loss
        if full_output:                                            # gicp.py:169-172
            if mode == "faithful":
                idx = dbg["index"]
                q = np.zeros_like(src)
                q[idx >= 0] = tgt[idx[idx >= 0]]
                top = np.argsort(np.linalg.det(dbg["weight"]))[-5:]
                hw_s.append(moved[top])
                hw_t.append(q[top])
            else:
                hw_s.append(apply_transformation(src[top_s[top_s >= 0]], T))   # gicp.py:119,171: the 5 rows only
                hw_t.append(_targets(tgt, top_s, top_t, d))
        offset = new_offset
        stop = None
        if use_pcl:                                                # PCL-style criteria, after the update
            sum_sq = sum(e.pass_info()["sum_sq"] for e in engines)
            cnt = float(np.sum(dbg["index"] >= 0)) if mode == "faithful" else float(st[-1])
            mse = sum_sq / cnt if cnt > 0 else 0.0
            stop = pcl_stop(T, T_new, mse, prev_mse, **pcl)
            prev_mse = mse
        T = T_new
        all_T.append(T)
        if stop is not None:
            if verbose:
                print("Converged at iteration", it, f"({stop})")
            break
    if moved_source:
        eng.set_source(src, p)   # leave the engine holding the untransformed source
    return T, all_T, init_src_cov, target_cov, hw_s, hw_t, all_src_cov


def _newton_from_points(src, q, W, idx, T):
    """Exact inner minimiser for the faithful path: statistics of the given (q, W) at T, then the host solve."""
    d = src.shape[1]
    ok = idx >= 0
    s, qq, WW = src[ok], q[ok], W[ok]
    r = qq - s @ T[:d, :d].T - T[:d, d]
    wr = np.einsum("nab,nb->na", WW, r)
    P = _sym_pairs(d)
    ws = np.stack([WW[:, a, b] for a, b in P], axis=1)
    ss = np.stack([s[:, i] * s[:, j] for i, j in P], axis=1)
    st = np.concatenate([np.einsum("np,nq->pq", ws, ss).ravel(), np.einsum("np,ni->pi", ws, s).ravel(), ws.sum(0),
                         np.einsum("na,ni->ai", wr, s).ravel(), wr.sum(0), [np.sum(r * wr)], [float(ok.sum())]])
    return solve_pose(st, T)
