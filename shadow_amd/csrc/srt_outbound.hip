// srt_outbound.hip -- batched outbound relay stage: each source host's
// interface qdisc over its sockets and its upload rate limit, for one
// scheduling window.
//
// Reference: a socket with data notifies the host (host/host.rs:988-1002),
// which queues the socket at the interface (host/network/network_interface.c:
// 344-370) and wakes relay_inet_out; the relay drains the interface in the
// qdisc's order (network_interface.c:205-340, network_queuing_disciplines.c)
// under a TokenBucket sized from bandwidth_up (host.rs:299-302,
// network/relay/mod.rs:200-287, relay/token_bucket.rs) and pushes every packet
// into the router, which calls Worker::send_packet at that moment
// (network/router/mod.rs:49-55, 74-77).  The per-host step -- sockets, qdisc,
// bucket, relay loop, event order, carry-over -- is srt_outbound_step.h,
// compiled here for the device and for the host-only instance alike.
//
// Out of scope: how sockets produce packets and the CPU-delay model.  The
// loopback relay is srt_loopback.hip; a local packet pushed back into this
// interface is resolved with srt_deliver_lookup_flat (srt_deliver.hip), its
// order among the call's local packets staying the caller's.
//
// Device form, two launches a call on the plan's stream:
//   (1) preset: one thread a batch packet: status 0, send_ns and send_rank
//       UINT64_MAX; the call's late count and pending count zeroed;
//   (2) step: one lane owns one source host (a wave 64 consecutive hosts).
//       The batch is grouped by host already, so the wave's packets are one
//       contiguous span: it is copied into LDS with coalesced loads as 32-byte
//       records whose last word becomes the per-socket link (a span over 2,048
//       packets is walked from HBM instead, its links in an HBM array).  The
//       per-socket cursors and the qdisc's socket array sit in HBM / L2; for
//       max_sockets <= 16 the wave copies its 64 hosts' (12 bytes a socket)
//       into LDS for the call and writes them back at its end.  LDS a
//       workgroup: 64 KB of window + 12 KB of cursors and socket queues =
//       76 KB, two workgroups a CU.  Each lane loads its 96-byte state record,
//       walks its arrivals in time order against its pending forward task and
//       stores the state back; the ring in HBM is read only when earlier calls
//       left packets in it and written only for packets still queued at
//       until_ns.  The wave runs as long as its busiest host.  The step is
//       instantiated for the four combinations of window and cursors in LDS or
//       not, so that every on-chip access is an LDS instruction.
// Every value is written with ordinary stores from plain C++.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "srt_internal.h"
#include "srt_outbound_step.h"
#include "srt_stage.h"

namespace {

using outb::CUR_LDS;
using outb::LDS_BYTES;
using outb::WIN_CAP;
using stage::set_err;
static_assert(sizeof(outb::Rec) == 32 && sizeof(outb::Cur) == 8 && sizeof(outb::RingEl) == 32 &&
              sizeof(srt_out_pkt) == 32 && sizeof(srt_outbound_late) == 32, "record layouts");

__global__ __launch_bounds__(256) void outbound_preset_kernel(uint32_t n_pkts, uint32_t *__restrict__ status,
                                                              uint64_t *__restrict__ send_ns,
                                                              uint64_t *__restrict__ send_rank,
                                                              uint32_t *__restrict__ late_count,
                                                              unsigned long long *__restrict__ pending) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        *late_count = 0;
        *pending = 0;
    }
    if (i >= n_pkts) return;
    status[i] = 0;
    send_ns[i] = outb::NONE;
    send_rank[i] = outb::NONE;
}

template <bool WIN, bool CL>
__device__ __forceinline__ void run_host(const outb::Ctx &c, uint32_t h, uint32_t s0, uint32_t n) {
    outb::Run<WIN, CL> r(c, h);
    r.win0 = s0, r.win_n = n;
    r.run();
}

__global__ __launch_bounds__(64) void outbound_step_kernel(const outb::Ctx c) {
    using outb::outb_lds;
    outb::Rec *win = reinterpret_cast<outb::Rec *>(outb_lds);
    outb::Cur *lcur = reinterpret_cast<outb::Cur *>(outb_lds + outb::LDS_CUR_OFF);
    uint32_t *lq = reinterpret_cast<uint32_t *>(outb_lds + outb::LDS_Q_OFF);
    const uint32_t h0 = blockIdx.x * 64, h = h0 + threadIdx.x;
    const uint32_t h1 = min(h0 + 64, c.n_hosts);
    const uint32_t lim = min(c.host_ptr[c.n_hosts], c.n_pkts);
    const uint32_t s0 = min(c.host_ptr[h0], lim), s1 = min(c.host_ptr[h1], lim);
    const uint32_t n = s1 > s0 ? s1 - s0 : 0;
    const bool staged = n <= WIN_CAP;
    if (staged)
        for (uint32_t i = threadIdx.x; i < n; i += 64) {
            const srt_out_pkt p = c.pkts[s0 + i];
            outb::Rec r;
            r.ready = p.ready_ns, r.prio = p.priority, r.size = p.total_size, r.socket = p.socket, r.flags = p.flags;
            r.link = outb::NIL;
            win[i] = r;
        }
    // the wave's cursors and socket queues: one contiguous span of (h1 - h0) * max_sockets entries
    const bool cur_lds = c.max_sockets <= CUR_LDS;
    const uint32_t n_cur = cur_lds ? (h1 - h0) * c.max_sockets : 0;
    const uint64_t cur0 = (uint64_t)h0 * c.max_sockets;
    for (uint32_t i = threadIdx.x; i < n_cur; i += 64) {
        lcur[i] = c.cur[cur0 + i];
        lq[i] = c.sockq[cur0 + i];
    }
    __syncthreads();
    if (h < c.n_hosts) {
        if (staged) {
            if (cur_lds) run_host<true, true>(c, h, s0, n);
            else run_host<true, false>(c, h, s0, n);
        } else {
            if (cur_lds) run_host<false, true>(c, h, s0, n);
            else run_host<false, false>(c, h, s0, n);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_cur; i += 64) {
        c.cur[cur0 + i] = lcur[i];
        c.sockq[cur0 + i] = lq[i];
    }
}

// srt_outbound_cached_seq: one thread a host
__global__ __launch_bounds__(256) void outbound_cached_seq_kernel(const outb::Host *__restrict__ hosts, uint32_t n_hosts,
                                                                  uint64_t *__restrict__ seq) {
    const uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h < n_hosts) seq[h] = outb::cached_seq_of(hosts[h]);
}

}  // namespace

struct srt_outbound {
    srt_plan *plan = nullptr;  // nullptr: host-only
    uint32_t n = 0, cap = 0, max_sockets = 0, qdisc = 0;
    // device form: device memory; host-only form: the vectors below
    outb::Host *hosts = nullptr;
    outb::RingEl *ring = nullptr;
    outb::Cur *cur = nullptr;
    uint32_t *sockq = nullptr;
    uint32_t *link = nullptr;
    size_t link_cap = 0;
    // [0] SRT_OUTBOUND_* bits, [1] the late count when the caller passes none, [2..3] u64 packets pending
    uint32_t *flags = nullptr;
    uint64_t base = 0, prev_until = 0;
    std::vector<outb::Host> h_hosts;
    std::vector<outb::RingEl> h_ring;
    std::vector<outb::Cur> h_cur;
    std::vector<uint32_t> h_sockq, h_link;
    alignas(8) uint32_t h_flags[4] = {0, 0, 0, 0};
};

namespace srt {
// srt_init: loads this unit's code object (srt::preload_kernels)
hipError_t preload_outbound() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&outbound_step_kernel));
}
}  // namespace srt

extern "C" void srt_outbound_destroy(srt_outbound *ob) {
    if (!ob) return;
    if (ob->plan) {
        (void)stage::use_device(ob->plan);
        (void)hipStreamSynchronize(ob->plan->stream);
        (void)hipFree(ob->hosts);
        (void)hipFree(ob->ring);
        (void)hipFree(ob->cur);
        (void)hipFree(ob->sockq);
        (void)hipFree(ob->link);
        (void)hipFree(ob->flags);
    }
    delete ob;
}

extern "C" srt_status srt_outbound_create(srt_plan *plan, uint32_t n_hosts, const uint64_t *bw_up_bytes_per_s,
                                          uint32_t qdisc, uint32_t max_sockets, uint32_t queue_cap,
                                          srt_outbound **out, srt_err *err) {
    stage::begin(err);
    if (!out || (n_hosts && !bw_up_bytes_per_s)) return stage::null_argument(err);
    *out = nullptr;
    if (qdisc > SRT_QDISC_RR || !max_sockets || max_sockets >= 0x80000000u || queue_cap >= 0x7ffffffeu) {
        set_err(err, SRT_ERR_INVALID, "outbound: qdisc, max_sockets or queue_cap out of range");
        return SRT_ERR_INVALID;
    }
    srt_outbound *ob = new (std::nothrow) srt_outbound;
    if (!ob) return SRT_ERR_OOM;
    ob->plan = plan;
    ob->n = n_hosts;
    ob->cap = queue_cap;
    ob->max_sockets = max_sockets;
    ob->qdisc = qdisc;
    const size_t n_ring = (size_t)n_hosts * queue_cap + 1, n_cur = (size_t)n_hosts * max_sockets + 1;
    try {
        ob->h_hosts.assign(n_hosts, outb::Host{});
        if (!plan) {
            ob->h_ring.resize(n_ring);
            ob->h_cur.assign(n_cur, outb::Cur{outb::NIL, outb::NIL});
            ob->h_sockq.assign(n_cur, 0);
        }
    } catch (const std::bad_alloc &) {
        delete ob;
        set_err(err, SRT_ERR_OOM, "outbound: host allocation failed");
        return SRT_ERR_OOM;
    }
    for (uint32_t h = 0; h < n_hosts; ++h) {
        outb::Host &s = ob->h_hosts[h];
        // create_token_bucket (relay/mod.rs:277-287)
        s.refill = relay::bucket_refill(bw_up_bytes_per_s[h]);
        s.capacity = relay::sat_add(s.refill, relay::MTU);
        s.balance = s.capacity;
        s.task_ns = outb::NONE;
    }
    if (!plan) {
        ob->hosts = ob->h_hosts.data();
        ob->ring = ob->h_ring.data();
        ob->cur = ob->h_cur.data();
        ob->sockq = ob->h_sockq.data();
        ob->flags = ob->h_flags;
        *out = ob;
        return SRT_OK;
    }
    srt::init_wait();
    bool ok = stage::use_device(plan);
    ok = ok && hipMalloc(&ob->hosts, ((size_t)n_hosts + 1) * sizeof(outb::Host)) == hipSuccess &&
         hipMalloc(&ob->ring, n_ring * sizeof(outb::RingEl)) == hipSuccess &&
         hipMalloc(&ob->cur, n_cur * sizeof(outb::Cur)) == hipSuccess &&
         hipMalloc(&ob->sockq, n_cur * 4) == hipSuccess && hipMalloc(&ob->flags, 16) == hipSuccess;
    ok = ok && hipMemcpy(ob->hosts, ob->h_hosts.data(), (size_t)n_hosts * sizeof(outb::Host),
                         hipMemcpyHostToDevice) == hipSuccess &&
         hipMemset(ob->cur, 0xff, n_cur * sizeof(outb::Cur)) == hipSuccess &&  // every cursor NIL
         hipMemset(ob->sockq, 0, n_cur * 4) == hipSuccess && hipMemset(ob->flags, 0, 16) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        ob->plan = nullptr;  // frees below without the stream
        (void)hipFree(ob->hosts);
        (void)hipFree(ob->ring);
        (void)hipFree(ob->cur);
        (void)hipFree(ob->sockq);
        (void)hipFree(ob->flags);
        delete ob;
        set_err(err, SRT_ERR_OOM, "outbound: device allocation failed");
        return SRT_ERR_OOM;
    }
    (void)hipFuncSetAttribute((const void *)outbound_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)LDS_BYTES);
    *out = ob;
    return SRT_OK;
}

extern "C" srt_status srt_outbound_run(srt_outbound *ob, const srt_out_pkt *d_pkts, const uint32_t *d_host_ptr,
                                       uint64_t n_pkts, uint64_t until_ns, uint64_t bootstrap_end_ns,
                                       uint32_t *d_status, uint64_t *d_send_ns, uint64_t *d_send_rank,
                                       srt_outbound_late *d_late, uint32_t late_cap, uint32_t *d_late_count,
                                       uint64_t *seq_base, srt_err *err) {
    stage::begin(err);
    if (!ob || !d_host_ptr || (late_cap && !d_late) ||
        (n_pkts && (!d_pkts || !d_status || !d_send_ns || !d_send_rank)))
        return stage::null_argument(err);
    if (n_pkts >= 0x80000000ull) {
        set_err(err, SRT_ERR_INVALID, "more than 2^31-1 packets in one batch");
        return SRT_ERR_INVALID;
    }
    if (until_ns < ob->prev_until) {
        set_err(err, SRT_ERR_INVALID, "outbound: until_ns earlier than the previous call's");
        return SRT_ERR_INVALID;
    }
    const uint32_t n = (uint32_t)n_pkts;
    if (ob->plan && !stage::use_device(ob->plan)) return SRT_ERR_HIP;
    if (n > ob->link_cap) {  // the links grow with the largest batch seen
        if (ob->plan) {
            (void)hipStreamSynchronize(ob->plan->stream);
            (void)hipFree(ob->link);
            ob->link = nullptr;
            ob->link_cap = 0;
            if (hipMalloc(&ob->link, (size_t)n * 4) != hipSuccess) {
                set_err(err, SRT_ERR_OOM, "hipMalloc(outbound links) failed");
                return SRT_ERR_OOM;
            }
        } else {
            try {
                ob->h_link.resize(n);
            } catch (const std::bad_alloc &) {
                set_err(err, SRT_ERR_OOM, "outbound: host allocation failed");
                return SRT_ERR_OOM;
            }
            ob->link = ob->h_link.data();
        }
        ob->link_cap = n;
    }
    outb::Ctx c;
    c.hosts = ob->hosts;
    c.ring = ob->ring;
    c.cur = ob->cur;
    c.sockq = ob->sockq;
    c.pkts = d_pkts;
    c.link = ob->link;
    c.host_ptr = d_host_ptr;
    c.status = d_status;
    c.send_ns = d_send_ns;
    c.send_rank = d_send_rank;
    c.late = d_late;
    c.late_count = d_late_count ? d_late_count : ob->flags + 1;
    c.flags = ob->flags;
    c.pending = reinterpret_cast<unsigned long long *>(ob->flags + 2);
    c.base = ob->base;
    c.until = until_ns;
    c.boot_end = bootstrap_end_ns;
    c.prev_until = ob->prev_until;
    c.n_hosts = ob->n;
    c.ring_cap = ob->cap;
    c.late_cap = late_cap;
    c.n_pkts = n;
    c.max_sockets = ob->max_sockets;
    c.qdisc = ob->qdisc;
    c.pad[0] = c.pad[1] = 0;
    if (ob->plan) {
        hipStream_t s = ob->plan->stream;
        hipLaunchKernelGGL(outbound_preset_kernel, dim3(n / 256 + 1), dim3(256), 0, s, n, d_status, d_send_ns,
                           d_send_rank, c.late_count, c.pending);
        if (ob->n)
            hipLaunchKernelGGL(outbound_step_kernel, dim3((ob->n + 63) / 64), dim3(64), LDS_BYTES, s, c);
        if (stage::launched(err, "outbound") != SRT_OK) return SRT_ERR_HIP;
    } else {
        *c.late_count = 0;
        *c.pending = 0;
        for (uint32_t i = 0; i < n; ++i) {
            d_status[i] = 0;
            d_send_ns[i] = outb::NONE;
            d_send_rank[i] = outb::NONE;
        }
        for (uint32_t h = 0; h < ob->n; ++h) {
            outb::Run<false> r(c, h);
            r.run();
        }
    }
    if (seq_base) *seq_base = ob->base;
    ob->base += n_pkts;
    ob->prev_until = until_ns;
    return SRT_OK;
}

namespace {
// the stream drained; the flags and the pending count (16 bytes) on the host,
// and every host's state record when `states`
srt_status pull(srt_outbound *ob, bool states, uint32_t *flags, uint64_t *pending, srt_err *err) {
    uint32_t w[4] = {0, 0, 0, 0};
    if (!ob->plan) {
        std::memcpy(w, ob->h_flags, sizeof w);
    } else {
        if (!stage::use_device(ob->plan)) return SRT_ERR_HIP;
        hipStream_t s = ob->plan->stream;
        if (hipMemcpyAsync(w, ob->flags, sizeof w, hipMemcpyDeviceToHost, s) != hipSuccess ||
            (states && ob->n &&
             hipMemcpyAsync(ob->h_hosts.data(), ob->hosts, (size_t)ob->n * sizeof(outb::Host), hipMemcpyDeviceToHost,
                            s) != hipSuccess) ||
            hipStreamSynchronize(s) != hipSuccess) {
            set_err(err, SRT_ERR_HIP, "outbound: stream failed");
            return SRT_ERR_HIP;
        }
    }
    *flags = w[0];
    std::memcpy(pending, w + 2, 8);
    return SRT_OK;
}
}  // namespace

extern "C" srt_status srt_outbound_status(srt_outbound *ob, uint32_t *flags, uint64_t *n_pending, srt_err *err) {
    stage::begin(err);
    if (!ob) return stage::null_argument(err);
    uint32_t f = 0;
    uint64_t pending = 0;
    const srt_status st = pull(ob, false, &f, &pending, err);
    if (st != SRT_OK) return st;
    if (f) {
        if (ob->plan) (void)hipMemsetAsync(ob->flags, 0, 4, ob->plan->stream);
        else ob->h_flags[0] = 0;
    }
    if (n_pending) *n_pending = pending;
    if (flags) *flags = f & 63u;
    if (!f) return SRT_OK;
    const char *msg = f & outb::F_BAD_SOCKET        ? "outbound: a packet's socket is not below max_sockets (not taken)"
                      : f & outb::F_TIME_REGRESSION ? "outbound: an arrival earlier than the previous call's until_ns"
                      : f & outb::F_RING_OVERFLOW   ? "outbound: a host's ring overflowed (its results are invalid)"
                      : f & outb::F_LATE_OVERFLOW   ? "outbound: more late records than late_cap"
                      : f & outb::F_AFTER_UNTIL     ? "outbound: an arrival at or after until_ns was not taken"
                                                    : "outbound: a packet larger than its host's token bucket holds";
    set_err(err, SRT_ERR_INVALID, msg);
    return SRT_ERR_INVALID;
}

extern "C" srt_status srt_outbound_state(srt_outbound *ob, srt_outbound_host_state *out, srt_err *err) {
    stage::begin(err);
    if (!ob || (ob->n && !out)) return stage::null_argument(err);
    uint32_t f = 0;
    uint64_t pending = 0;
    const srt_status st = pull(ob, true, &f, &pending, err);
    if (st != SRT_OK) return st;
    for (uint32_t h = 0; h < ob->n; ++h) {
        const outb::Host &s = ob->h_hosts[h];
        srt_outbound_host_state &o = out[h];
        o.balance = s.balance;
        o.last_refill_ns = s.last_refill;
        o.task_ns = s.task_ns;
        o.tasks_scheduled = s.tasks;
        o.sent_total = s.sent;
        o.queue_len = s.ring_len;
        o.cached = s.cached;
        o.overflow = s.overflow;
    }
    return SRT_OK;
}

extern "C" srt_status srt_outbound_cached_seq(srt_outbound *ob, uint64_t *d_seq, srt_err *err) {
    stage::begin(err);
    if (!ob || (ob->n && !d_seq)) return stage::null_argument(err);
    if (!ob->n) return SRT_OK;
    if (!ob->plan) {
        for (uint32_t h = 0; h < ob->n; ++h) d_seq[h] = outb::cached_seq_of(ob->hosts[h]);
        return SRT_OK;
    }
    if (!stage::use_device(ob->plan)) return SRT_ERR_HIP;
    hipLaunchKernelGGL(outbound_cached_seq_kernel, dim3((ob->n + 255) / 256), dim3(256), 0, ob->plan->stream, ob->hosts,
                       ob->n, d_seq);
    return stage::launched(err, "outbound");
}
