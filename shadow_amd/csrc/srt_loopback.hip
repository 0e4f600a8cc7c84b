// srt_loopback.hip -- the loopback interface: what a host's sockets hand to
// 127.0.0.1 at one instant is popped in the qdisc's order by relay_loopback's
// forward task, pushed back into the same interface, looked up in the loopback
// interface's own associations and counted in the tracker's LOCAL records
// (host/host.rs:307-310, 988-1002; network/relay/mod.rs:110-135, 200-272;
// host/network/network_interface.c:140-202, 205-370; host/tracker.c:188-284).
// The step -- the instants, the two sort keys, the lookup, the counters, the
// flags, the range checks -- is srt_loopback_step.h, compiled here for the
// device and for the host-only instance alike.  The table is the srt_deliver
// instance's, uploaded by srt_deliver_run's own path (srt::deliver_table); the
// heartbeat is srt_tracker's (srt::counters_heartbeat).
//
// Device form, one launch a run on the plan's stream; only heartbeat, tasks
// and status wait for it.  A group of L lanes owns one host and walks its span
// twice:
//   (1) arrivals: lane l takes packets b + l, b + l + L, ... with coalesced
//       loads; the begin of a packet's instant is a max-scan of the instants'
//       first indices across the group's lanes, carried along the walk; the
//       packet's key is one pass over the earlier packets of its instant
//       (L1 / L2 hits: the lanes of a group read the same few lines).  Keys and
//       instants go to the per-packet scratch; the time-order and socket checks
//       and the tasks are reduced across the group;
//   (2) after a workgroup barrier, unless the host is flagged: a packet's place
//       is its instant's begin plus the keys of the instant that sort before
//       its own; the lane looks the packet up, writes the five outputs at that
//       place, adds to the two slot records with 64-bit atomics and keeps the
//       host's twenty sums in registers.  They are reduced across the group and
//       its first lane adds them to the host's records with ordinary loads and
//       stores: no other lane of the launch has those records.
// So a packet's records are read from HBM once and an instant of any length
// needs no LDS window; its cost is quadratic in its length, shared by L lanes.
// L is 64 (a wave a host) when the batch averages more than 16 packets a host,
// else 8 (eight hosts a wave).  No kernel adds to a call-wide counter: the
// run's counts are kept a host and summed by srt_loopback_status.
// Every value is written with ordinary stores or vector atomics from plain C++.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "srt_internal.h"
#include "srt_loopback_step.h"
#include "srt_stage.h"

namespace {

static_assert(sizeof(srt_trk_counters) == 80 && sizeof(srt_trk_meta) == 16 && sizeof(srt_rx_meta) == 16 &&
                  sizeof(srt_out_pkt) == 32 && sizeof(loopb::State) == 24 && sizeof(loopb::HostSt) == 16,
              "record layouts");

using stage::BT;
using stage::ST;
using stage::set_err;

template <uint32_t L>
__global__ __launch_bounds__(BT) void loopback_run_kernel(const loopb::Ctx c) {
    const stage::Group<L> G(c.n_hosts);
    const uint32_t l = G.l;
    const bool own = G.own();
    const uint32_t h = own ? (uint32_t)G.g : 0u;
    uint32_t b = 0, e = 0;
    uint64_t last = loopb::NONE;
    if (own) {
        relay::segment(c.host_ptr, loopb::walked(c), h, b, e);
        last = c.hs[h].last_ns;
    }
    // (1) every lane of the wave takes every step: the shuffles are over whole groups
    uint32_t bits = 0, n_tasks = 0, carry = b;
    for (uint32_t i = b + l; __any(i < e); i += L) {
        uint32_t gb = 0;
        if (i < e) {
            const uint32_t a = loopb::arrival(c, b, i, last);
            bits |= a & loopb::F_HOST;
            n_tasks += (a & loopb::A_TASK) != 0;
            if (a & loopb::A_GROUP) gb = i;
        }
#pragma unroll
        for (uint32_t off = 1; off < L; off <<= 1) {
            const uint32_t o = __shfl_up(gb, off, L);
            if (l >= off && o > gb) gb = o;
        }
        if (carry > gb) gb = carry;  // the instant began in an earlier step
        carry = __shfl(gb, L - 1, L);
        if (i < e) loopb::key_store(c, gb, i, e);
    }
    bits = stage::group_or<L>(bits);
    n_tasks = stage::group_add<L>(n_tasks);
    if (own && l == 0) loopb::scan_done(c, h, b, e, bits, n_tasks);
    __threadfence();
    __syncthreads();  // the keys and instants of the workgroup's hosts are written
    // (2)
    tracker::Acc in, out;
    tracker::acc_zero(in);
    tracker::acc_zero(out);
    uint32_t miss = 0;
    for (uint32_t i = b + l; i < e; i += L) {
        if (bits) loopb::emit_flagged(c, i);
        else miss += loopb::emit(c, h, b, e, i, in, out);
    }
    stage::group_sum<L>(in.v);  // every lane is here
    stage::group_sum<L>(out.v);
    miss = stage::group_add<L>(miss);
    if (own && l == 0) loopb::emit_done(c, h, in, out, bits ? 0 : e - b, miss);
}

// srt_loopback_status: the hosts' counts of the last run, summed by one workgroup
__global__ __launch_bounds__(ST) void loopback_sum_kernel(const loopb::Ctx c) {
    __shared__ uint64_t wsum[2][ST / 64];
    const uint32_t t = threadIdx.x;
    unsigned long long rx = 0, miss = 0;
    for (uint32_t h = t; h < c.n_hosts; h += ST) rx += c.cnt_recv[h], miss += c.cnt_miss[h];
    for (uint32_t off = 32; off > 0; off >>= 1) rx += __shfl_xor(rx, off), miss += __shfl_xor(miss, off);
    if ((t & 63) == 0) wsum[0][t >> 6] = rx, wsum[1][t >> 6] = miss;
    __syncthreads();
    if (t == 0) {
        uint64_t a = 0, b = 0;
        for (uint32_t w = 0; w < ST / 64; ++w) a += wsum[0][w], b += wsum[1][w];
        c.st->n_received = a;
        c.st->n_no_socket = b;
    }
}

}  // namespace

struct srt_loopback {
    srt_plan *plan = nullptr;  // nullptr: host-only
    uint32_t n_hosts = 0, n_slots = 0;
    void *mem = nullptr;       // device form: everything but the scratch in one allocation; host-only: h_mem
    void *scratch = nullptr;   // 16 bytes a packet of the largest batch seen
    size_t scratch_cap = 0;    // packets
    size_t rec_bytes = 0;      // the four record arrays, contiguous from node_in
    std::vector<uint64_t> h_mem, h_scratch;
    std::vector<srt_trk_counters> stage;  // device form: the records on the host, for the heartbeat
    std::vector<loopb::HostSt> h_hs;      // device form: the hosts' words on the host, for srt_loopback_tasks
    loopb::Ctx base;
};

namespace srt {
// srt_init: loads this unit's code object (srt::preload_kernels)
hipError_t preload_loopback() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&loopback_sum_kernel));
}
}  // namespace srt

extern "C" void srt_loopback_destroy(srt_loopback *lb) {
    if (!lb) return;
    if (lb->plan) {
        (void)stage::use_device(lb->plan);
        (void)hipStreamSynchronize(lb->plan->stream);
        (void)hipFree(lb->mem);
        (void)hipFree(lb->scratch);
    }
    delete lb;
}

extern "C" srt_status srt_loopback_create(srt_plan *plan, uint32_t n_hosts, uint32_t qdisc, uint32_t max_sockets,
                                          uint32_t n_slots, srt_loopback **out, srt_err *err) {
    stage::begin(err);
    if (!out) return stage::null_argument(err);
    *out = nullptr;
    if (n_hosts >= 0x80000000u || n_slots >= 0x80000000u || qdisc > SRT_QDISC_RR || !max_sockets) {
        set_err(err, SRT_ERR_INVALID, "loopback: n_hosts, n_slots (below 2^31), qdisc or max_sockets out of range");
        return SRT_ERR_INVALID;
    }
    srt_loopback *lb = new (std::nothrow) srt_loopback;
    if (!lb) return SRT_ERR_OOM;
    lb->plan = plan;
    lb->n_hosts = n_hosts;
    lb->n_slots = n_slots;
    // state; the hosts' and the slots' records; the hosts' words; the hosts' two counts
    const size_t head = 32, recs = 2 * ((size_t)n_hosts + n_slots);
    lb->rec_bytes = recs * sizeof(srt_trk_counters);
    const size_t bytes = head + lb->rec_bytes + 24 * (size_t)n_hosts;
    bool ok = true;
    if (!plan) {
        try {
            lb->h_mem.assign(bytes / 8 + 1, 0);
        } catch (const std::bad_alloc &) {
            ok = false;
        }
        lb->mem = lb->h_mem.data();
    } else {
        try {
            lb->stage.resize(recs + 1);
            lb->h_hs.resize((size_t)n_hosts + 1);
        } catch (const std::bad_alloc &) {
            ok = false;
        }
        if (ok) {
            srt::init_wait();
            ok = stage::use_device(plan);
            ok = ok && hipMalloc(&lb->mem, bytes + 8) == hipSuccess;
            ok = ok && hipMemset(lb->mem, 0, bytes + 8) == hipSuccess;
            if (!ok) {
                (void)hipGetLastError();
                (void)hipFree(lb->mem);
            }
        }
    }
    if (!ok) {
        delete lb;
        set_err(err, SRT_ERR_OOM, "loopback: allocation failed");
        return SRT_ERR_OOM;
    }
    loopb::Ctx &c = lb->base;
    std::memset(&c, 0, sizeof c);
    char *p = static_cast<char *>(lb->mem);
    c.st = reinterpret_cast<loopb::State *>(p);
    c.node_in = reinterpret_cast<srt_trk_counters *>(p + head);
    c.node_out = c.node_in + n_hosts;
    c.slot_in = c.node_out + n_hosts;
    c.slot_out = c.slot_in + n_slots;
    c.hs = reinterpret_cast<loopb::HostSt *>(p + head + lb->rec_bytes);
    c.cnt_recv = reinterpret_cast<uint32_t *>(c.hs + n_hosts);
    c.cnt_miss = c.cnt_recv + n_hosts;
    c.n_hosts = n_hosts;
    c.n_slots = n_slots;
    c.max_sockets = max_sockets;
    c.qdisc = qdisc;
    // no host has seen an instant yet: last_ns NONE, tasks 0
    if (!plan) {
        for (uint32_t h = 0; h < n_hosts; ++h) c.hs[h].last_ns = loopb::NONE;
    } else {
        for (uint32_t h = 0; h < n_hosts; ++h) lb->h_hs[h] = loopb::HostSt{loopb::NONE, 0};
        if (n_hosts && hipMemcpy(c.hs, lb->h_hs.data(), 16 * (size_t)n_hosts, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(lb->mem);
            delete lb;
            set_err(err, SRT_ERR_HIP, "loopback: device initialisation failed");
            return SRT_ERR_HIP;
        }
    }
    *out = lb;
    return SRT_OK;
}

extern "C" srt_status srt_loopback_run(srt_loopback *lb, srt_deliver *dl, const srt_out_pkt *d_pkts,
                                       const uint32_t *d_host_ptr, uint64_t n_pkts, const srt_rx_meta *d_rx_meta,
                                       const srt_trk_meta *d_trk_meta, uint32_t *d_out_index, uint32_t *d_out_socket,
                                       uint64_t *d_out_recv_ns, uint32_t *d_out_user, uint32_t *d_out_status,
                                       srt_err *err) {
    stage::begin(err);
    if (!lb || !dl || !d_host_ptr ||
        (n_pkts && (!d_pkts || !d_rx_meta || !d_out_index || !d_out_socket || !d_out_recv_ns || !d_out_user ||
                    !d_out_status)))
        return stage::null_argument(err);
    if (n_pkts >= 0x80000000ull) {
        set_err(err, SRT_ERR_INVALID, "more than 2^31-1 packets in one batch");
        return SRT_ERR_INVALID;
    }
    loopb::Ctx c = lb->base;
    srt_plan *dl_plan = nullptr;
    uint32_t dl_hosts = 0;
    const srt_status up = srt::deliver_table(dl, &dl_plan, &dl_hosts, &c.table, &c.mask, err);
    if (up != SRT_OK) return up;
    if (dl_plan != lb->plan || dl_hosts != lb->n_hosts) {
        set_err(err, SRT_ERR_INVALID, "loopback: the deliver instance is of another plan or another n_hosts");
        return SRT_ERR_INVALID;
    }
    const uint32_t n = (uint32_t)n_pkts;
    if (n > lb->scratch_cap) {  // the scratch grows with the largest batch seen
        if (lb->plan) {
            (void)hipStreamSynchronize(lb->plan->stream);
            (void)hipFree(lb->scratch);
            lb->scratch = nullptr;
            lb->scratch_cap = 0;
            if (hipMalloc(&lb->scratch, (size_t)n * 16) != hipSuccess) {
                (void)hipGetLastError();
                set_err(err, SRT_ERR_OOM, "hipMalloc(loopback scratch) failed");
                return SRT_ERR_OOM;
            }
        } else {
            try {
                lb->h_scratch.resize((size_t)n * 2);
            } catch (const std::bad_alloc &) {
                set_err(err, SRT_ERR_OOM, "loopback: host allocation failed");
                return SRT_ERR_OOM;
            }
            lb->scratch = lb->h_scratch.data();
        }
        lb->scratch_cap = n;
    }
    c.key = static_cast<uint64_t *>(lb->scratch);
    c.grp = reinterpret_cast<uint32_t *>(c.key + lb->scratch_cap);
    c.gend = c.grp + lb->scratch_cap;
    c.n_pkts = n;
    c.pkts = d_pkts;
    c.host_ptr = d_host_ptr;
    c.rx_meta = d_rx_meta;
    c.trk_meta = d_trk_meta;
    c.out_index = d_out_index;
    c.out_socket = d_out_socket;
    c.out_recv_ns = d_out_recv_ns;
    c.out_user = d_out_user;
    c.out_status = d_out_status;
    if (!lb->plan) {
        loopb::host_run(c);
        return SRT_OK;
    }
    if (!c.n_hosts) return SRT_OK;
    hipStream_t s = lb->plan->stream;
    const bool wide = stage::wide(n_pkts, c.n_hosts);
    stage::launch_grouped(loopback_run_kernel<64>, loopback_run_kernel<8>, wide, stage::host_blocks(c.n_hosts, wide),
                          BT, s, c);
    return stage::launched(err, "loopback");
}

extern "C" srt_status srt_loopback_heartbeat(srt_loopback *lb, const uint32_t *hosts, uint32_t n_sel_hosts,
                                             const uint32_t *slots, uint32_t n_sel_slots,
                                             srt_trk_counters *out_node_in, srt_trk_counters *out_node_out,
                                             srt_trk_counters *out_slot_in, srt_trk_counters *out_slot_out,
                                             srt_err *err) {
    stage::begin(err);
    if (!lb) return stage::null_argument(err);
    return srt::counters_heartbeat(lb->plan, "loopback", lb->base.node_in, lb->rec_bytes, lb->stage.data(),
                                   lb->n_hosts, lb->n_slots, hosts, n_sel_hosts, slots, n_sel_slots, out_node_in,
                                   out_node_out, out_slot_in, out_slot_out, err);
}

extern "C" srt_status srt_loopback_tasks(srt_loopback *lb, uint64_t *out_tasks, srt_err *err) {
    stage::begin(err);
    if (!lb || (lb->n_hosts && !out_tasks)) return stage::null_argument(err);
    const loopb::HostSt *hs = lb->base.hs;
    if (lb->plan && lb->n_hosts) {
        if (!stage::use_device(lb->plan)) return SRT_ERR_HIP;
        hipStream_t s = lb->plan->stream;
        if (hipMemcpyAsync(lb->h_hs.data(), lb->base.hs, 16 * (size_t)lb->n_hosts, hipMemcpyDeviceToHost, s) !=
                hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) {
            (void)hipGetLastError();
            set_err(err, SRT_ERR_HIP, "loopback: stream failed");
            return SRT_ERR_HIP;
        }
        hs = lb->h_hs.data();
    }
    for (uint32_t h = 0; h < lb->n_hosts; ++h) out_tasks[h] = hs[h].tasks;
    return SRT_OK;
}

extern "C" srt_status srt_loopback_status(srt_loopback *lb, uint32_t *flags, uint64_t *n_received,
                                          uint64_t *n_no_socket, srt_err *err) {
    stage::begin(err);
    if (!lb) return stage::null_argument(err);
    loopb::State w;
    if (!lb->plan) {
        w = *lb->base.st;
        lb->base.st->flags = 0;
    } else {
        if (!stage::use_device(lb->plan)) return SRT_ERR_HIP;
        hipLaunchKernelGGL(loopback_sum_kernel, dim3(1), dim3(ST), 0, lb->plan->stream, lb->base);
        const srt_status st = stage::read_status(lb->plan, &w, lb->base.st, sizeof w, err, "loopback");
        if (st != SRT_OK) return st;
    }
    const uint32_t f = w.flags & 7u;
    if (flags) *flags = f;
    if (n_received) *n_received = w.n_received;
    if (n_no_socket) *n_no_socket = w.n_no_socket;
    if (!f) return SRT_OK;
    if (err) {
        err->code = SRT_ERR_INVALID;
        std::snprintf(err->msg, sizeof err->msg, "loopback:%s%s%s",
                      f & loopb::F_TIME_ORDER ? " a ready_ns below its host's previous arrival (the host's span is not run);" : "",
                      f & loopb::F_BAD_SOCKET ? " a socket is not below max_sockets (the host's span is not run);" : "",
                      f & loopb::F_BAD_SLOT ? " a socket slot is not below n_slots (counted at its host only);" : "");
    }
    return SRT_ERR_INVALID;
}
