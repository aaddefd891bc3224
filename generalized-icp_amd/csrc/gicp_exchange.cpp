// gicp_exchange.cpp — the three ways ranks sum their statistics, one per context: an RCCL communicator, a host
// hook, and the in-kernel peer exchange over IPC-mapped areas.  (The sum itself: allreduce_stats
// in gicp_align.cpp and k_corr.)
#include "gicp_host.h"

namespace gicp {

void drop_comm(gicp_ctx* c) {
    if (c->comm) ncclCommDestroy(c->comm);
    c->comm = nullptr;
}

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

// the device's wall clock (the peer exchange's time-out and timings count its ticks)
int wall_clock_khz(gicp_ctx* c) {
    int khz = 0;
    HIPCHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device));
    return khz > 0 ? khz : 100000;
}

void comm_init(gicp_ctx* c, int nranks, int rank, const char* id) {
    drop_comm(c);
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
}

void comm_ranks(gicp_ctx* c, int* nranks, int* rank, int* kind) {
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
}

void set_allreduce(gicp_ctx* c, gicp_allreduce_fn fn, void* user, int nranks, int rank) {
    if (fn) close_peers(c);
    if (fn && !c->h_xchg) c->h_xchg.alloc(80);
    if (fn && c->comm) {   // one exchange per context: the hook replaces the communicator
        HIPCHK(hipStreamSynchronize(c->stream));
        drop_comm(c);
    }
    c->hook = fn;
    c->hook_user = fn ? user : nullptr;
    if (!c->comm) {   // what gicp_comm_ranks reports for the hook
        c->nranks = fn ? nranks : 1;
        c->rank = fn ? rank : 0;
    }
}

void peer_export(gicp_ctx* c, char* handle) {
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
}

void peer_init(gicp_ctx* c, int nranks, int rank, const char* handles, double timeout_s) {
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
        p.timeout = (uint64_t)(timeout_s * wall_clock_khz(c) * 1e3);
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
    drop_comm(c);
    c->hook = nullptr;
    c->peer = p;
    c->peer_timeout_s = timeout_s;
    c->nranks = nranks;
    c->rank = rank;
}

}  // namespace gicp
