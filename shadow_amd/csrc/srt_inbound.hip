// srt_inbound.hip -- batched inbound router stage: each destination host's
// CoDel queue and download rate limit, for one scheduling window.
//
// Reference: the packet events srt_packet_events ordered run at their
// destination host, where each pushes its packet into the host's upstream
// Router, a CoDelQueue (src/main/network/router/mod.rs:57-61,
// router/codel_queue.rs), and the host's relay_inet_in drains that queue into
// the network interface under a TokenBucket sized from bandwidth_down
// (network/relay/mod.rs:200-287, relay/token_bucket.rs, host/host.rs:303-305,
// 855-858, 977-979).  The per-host step itself -- queue, bucket, relay loop,
// event order -- is srt_inbound_step.h, compiled here for the device and for
// the host-only instance alike.
//
// Out of scope: the CPU-delay model that reschedules events (host.rs:820-848),
// the loopback relay (the outbound relay is srt_outbound.hip), and what the
// socket does with the packet (the interface's receive side is srt_deliver.hip).
//
// Device form, two launches a call on the plan's stream:
//   (1) stage: one thread a position of order[]: the gathers behind it
//       (deliver time, size) done once into 16-byte records in group order,
//       and every batch packet's outputs preset (status 0, forward UINT64_MAX);
//   (2) step: one lane owns one destination host (a wave 64 consecutive
//       hosts).  The wave copies its hosts' records -- one contiguous span of
//       the stream -- into LDS with coalesced loads (a span over 5,120 records
//       is walked from HBM instead); each lane loads its 128-byte state
//       record, walks its records in time order against its pending forward
//       task, and stores the state back.  The ring in HBM is read only when
//       earlier calls left packets in it and written only for packets still
//       queued at until_ns.  Group sizes differ between the hosts of a wave;
//       the wave runs as long as its busiest host (accepted).
// Every value is written with ordinary stores from plain C++.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "srt_inbound_step.h"
#include "srt_internal.h"
#include "srt_stage.h"

namespace {

using stage::set_err;

constexpr uint32_t F_BAD_ORDER = 32;  // order[] / dst_ptr[] out of range (internal, reported as invalid)

__host__ __device__ __forceinline__ void stage_one(uint64_t i, const uint32_t *order, uint32_t n_sent,
                                                   const uint64_t *deliver, const uint32_t *size, uint32_t n_pkts,
                                                   inb::Rec *rec, uint32_t *status, uint64_t *forward,
                                                   uint32_t *flags) {
    status[i] = 0;
    forward[i] = inb::NONE;
    if (i < n_sent) {
        uint32_t p = order[i];
        inb::Rec r;
        if (p < n_pkts) {
            r.ts = deliver[p];
            r.size = size[p];
        } else {
            inb::raise(flags, F_BAD_ORDER);
            p = 0;
            r.ts = inb::NONE;
            r.size = 0;
        }
        r.idx = p;
        rec[i] = r;
    }
}

__global__ __launch_bounds__(256) void inbound_stage_kernel(const uint32_t *__restrict__ order,
                                                            const uint32_t *__restrict__ dst_ptr, uint32_t n_hosts,
                                                            const uint64_t *__restrict__ deliver,
                                                            const uint32_t *__restrict__ size, uint32_t n_pkts,
                                                            inb::Rec *__restrict__ rec, uint32_t *__restrict__ status,
                                                            uint64_t *__restrict__ forward,
                                                            uint32_t *__restrict__ late_count,
                                                            uint32_t *__restrict__ flags,
                                                            unsigned long long *__restrict__ pending) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        *late_count = 0;
        *pending = 0;
    }
    if (i >= n_pkts) return;
    const uint32_t n_sent = min(dst_ptr[n_hosts], n_pkts);
    stage_one(i, order, n_sent, deliver, size, n_pkts, rec, status, forward, flags);
}

// Records a wave may hold in LDS (80 KB: two workgroups share a CU's 160 KB): its 64 hosts' groups
// are one contiguous span of the staged stream.
constexpr uint32_t WIN_CAP = 5120;

__global__ __launch_bounds__(64) void inbound_step_kernel(const inb::Ctx c) {
    extern __shared__ inb::Rec inb_window[];
    const uint32_t h0 = blockIdx.x * 64, h = h0 + threadIdx.x;
    const uint32_t h1 = min(h0 + 64, c.n_hosts);
    const uint32_t lim = min(c.dst_ptr[c.n_hosts], c.n_pkts);
    const uint32_t s0 = min(c.dst_ptr[h0], lim), s1 = min(c.dst_ptr[h1], lim);
    const uint32_t n = s1 > s0 ? s1 - s0 : 0;
    const bool staged = n <= c.win_cap;
    if (staged)
        for (uint32_t i = threadIdx.x; i < n; i += 64) inb_window[i] = c.rec[s0 + i];
    __syncthreads();
    if (h >= c.n_hosts) return;
    if (staged) {
        inb::Run<true> r(c, h);
        r.win0 = s0;
        r.win_n = n;
        r.run();
    } else {
        inb::Run<false> r(c, h);
        r.run();
    }
}

__global__ __launch_bounds__(256) void inbound_law_kernel(const uint64_t *__restrict__ counts, uint64_t n,
                                                          const uint64_t *__restrict__ tab,
                                                          uint64_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = tab ? inb::law_increment(tab, counts[i]) : inb::law_increment_f64(counts[i]);
}

}  // namespace

struct srt_inbound {
    srt_plan *plan = nullptr;  // nullptr: host-only
    uint32_t n = 0, cap = 0;
    // device form: device memory; host-only form: the vectors below
    inb::Host *hosts = nullptr;
    inb::RingEl *ring = nullptr;
    inb::Rec *rec = nullptr;
    size_t rec_cap = 0;
    // [0] SRT_INBOUND_* bits, [1] the late count when the caller passes none, [2..3] u64 packets pending
    uint32_t *flags = nullptr;
    uint64_t *law_tab = nullptr;
    uint64_t base = 0, prev_until = 0;
    std::vector<inb::Host> h_hosts;
    std::vector<inb::RingEl> h_ring;
    std::vector<inb::Rec> h_rec;
    std::vector<uint64_t> h_law;
    alignas(8) uint32_t h_flags[4] = {0, 0, 0, 0};
};

namespace srt {
// srt_init: loads this unit's code object (srt::preload_kernels)
hipError_t preload_inbound() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&inbound_step_kernel));
}
}  // namespace srt

extern "C" void srt_inbound_destroy(srt_inbound *ib) {
    if (!ib) return;
    if (ib->plan) {
        (void)stage::use_device(ib->plan);
        (void)hipStreamSynchronize(ib->plan->stream);
        (void)hipFree(ib->hosts);
        (void)hipFree(ib->ring);
        (void)hipFree(ib->rec);
        (void)hipFree(ib->flags);
        (void)hipFree(ib->law_tab);
    }
    delete ib;
}

extern "C" srt_status srt_inbound_create(srt_plan *plan, uint32_t n_hosts, const uint64_t *bw_down_bytes_per_s,
                                         uint32_t queue_cap, srt_inbound **out, srt_err *err) {
    stage::begin(err);
    if (!out || (n_hosts && !bw_down_bytes_per_s)) return stage::null_argument(err);
    *out = nullptr;
    srt_inbound *ib = new (std::nothrow) srt_inbound;
    if (!ib) return SRT_ERR_OOM;
    ib->plan = plan;
    ib->n = n_hosts;
    ib->cap = queue_cap;
    try {
        ib->h_hosts.assign(n_hosts, inb::Host{});
        ib->h_law.resize(inb::LAW_TABLE);
        if (!plan) ib->h_ring.resize((size_t)n_hosts * queue_cap + 1);
    } catch (const std::bad_alloc &) {
        delete ib;
        set_err(err, SRT_ERR_OOM, "inbound: host allocation failed");
        return SRT_ERR_OOM;
    }
    for (uint32_t h = 0; h < n_hosts; ++h) {
        inb::Host &s = ib->h_hosts[h];
        // create_token_bucket (relay/mod.rs:277-287)
        s.refill = bw_down_bytes_per_s[h] / 1000 ? bw_down_bytes_per_s[h] / 1000 : 1;
        s.capacity = inb::sat_add(s.refill, inb::MTU);
        s.balance = s.capacity;
        s.interval_end = s.drop_next = s.task_ns = inb::NONE;
    }
    // the control law's increments for small counts, evaluated by the host
    for (uint32_t k = 0; k < inb::LAW_TABLE; ++k) ib->h_law[k] = inb::law_increment_f64(k);
    if (!plan) {
        ib->hosts = ib->h_hosts.data();
        ib->ring = ib->h_ring.data();
        ib->law_tab = ib->h_law.data();
        ib->flags = ib->h_flags;
        *out = ib;
        return SRT_OK;
    }
    srt::init_wait();
    const size_t ring_bytes = ((size_t)n_hosts * queue_cap + 1) * sizeof(inb::RingEl);
    const size_t host_bytes = ((size_t)n_hosts + 1) * sizeof(inb::Host);
    bool ok = stage::use_device(plan);
    ok = ok && hipMalloc(&ib->hosts, host_bytes) == hipSuccess && hipMalloc(&ib->ring, ring_bytes) == hipSuccess &&
         hipMalloc(&ib->flags, 16) == hipSuccess && hipMalloc(&ib->law_tab, 8 * inb::LAW_TABLE) == hipSuccess;
    ok = ok && hipMemcpy(ib->hosts, ib->h_hosts.data(), (size_t)n_hosts * sizeof(inb::Host), hipMemcpyHostToDevice) ==
                   hipSuccess &&
         hipMemcpy(ib->law_tab, ib->h_law.data(), 8 * inb::LAW_TABLE, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemset(ib->flags, 0, 16) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        ib->plan = nullptr;  // frees below without the stream
        (void)hipFree(ib->hosts);
        (void)hipFree(ib->ring);
        (void)hipFree(ib->flags);
        (void)hipFree(ib->law_tab);
        delete ib;
        set_err(err, SRT_ERR_OOM, "inbound: device allocation failed");
        return SRT_ERR_OOM;
    }
    (void)hipFuncSetAttribute((const void *)inbound_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(WIN_CAP * sizeof(inb::Rec)));
    *out = ib;
    return SRT_OK;
}

extern "C" srt_status srt_inbound_run(srt_inbound *ib, const uint32_t *d_order, const uint32_t *d_dst_ptr,
                                      const uint64_t *d_deliver, const uint32_t *d_total_size, uint64_t n_pkts,
                                      uint64_t until_ns, uint64_t bootstrap_end_ns, uint32_t *d_status,
                                      uint64_t *d_forward_ns, srt_inbound_late *d_late, uint32_t late_cap,
                                      uint32_t *d_late_count, uint64_t *seq_base, srt_err *err) {
    stage::begin(err);
    if (!ib || !d_dst_ptr || (late_cap && !d_late) ||
        (n_pkts && (!d_order || !d_deliver || !d_total_size || !d_status || !d_forward_ns)))
        return stage::null_argument(err);
    if (n_pkts >= 0xffffffffull) {
        set_err(err, SRT_ERR_INVALID, "more than 2^32-2 packets in one batch");
        return SRT_ERR_INVALID;
    }
    if (until_ns < ib->prev_until) {
        set_err(err, SRT_ERR_INVALID, "inbound: until_ns earlier than the previous call's");
        return SRT_ERR_INVALID;
    }
    const uint32_t n = (uint32_t)n_pkts;
    if (ib->plan && !stage::use_device(ib->plan)) return SRT_ERR_HIP;
    if (n > ib->rec_cap) {  // the staged records grow with the largest batch seen
        if (ib->plan) {
            (void)hipStreamSynchronize(ib->plan->stream);
            (void)hipFree(ib->rec);
            ib->rec = nullptr;
            ib->rec_cap = 0;
            if (hipMalloc(&ib->rec, (size_t)n * sizeof(inb::Rec)) != hipSuccess) {
                set_err(err, SRT_ERR_OOM, "hipMalloc(inbound records) failed");
                return SRT_ERR_OOM;
            }
        } else {
            try {
                ib->h_rec.resize(n);
            } catch (const std::bad_alloc &) {
                set_err(err, SRT_ERR_OOM, "inbound: host allocation failed");
                return SRT_ERR_OOM;
            }
            ib->rec = ib->h_rec.data();
        }
        ib->rec_cap = n;
    }
    inb::Ctx c;
    c.hosts = ib->hosts;
    c.ring = ib->ring;
    c.rec = ib->rec;
    c.dst_ptr = d_dst_ptr;
    c.status = d_status;
    c.forward = d_forward_ns;
    c.late = d_late;
    c.late_count = d_late_count ? d_late_count : ib->flags + 1;
    c.flags = ib->flags;
    c.pending = reinterpret_cast<unsigned long long *>(ib->flags + 2);
    c.law_tab = ib->law_tab;
    c.base = ib->base;
    c.until = until_ns;
    c.boot_end = bootstrap_end_ns;
    c.prev_until = ib->prev_until;
    c.n_hosts = ib->n;
    c.ring_cap = ib->cap;
    c.late_cap = late_cap;
    c.n_pkts = n;
    c.win_cap = WIN_CAP;
    c.pad = 0;
    if (ib->plan) {
        hipStream_t s = ib->plan->stream;
        hipLaunchKernelGGL(inbound_stage_kernel, dim3(n / 256 + 1), dim3(256), 0, s, d_order, d_dst_ptr, ib->n,
                           d_deliver, d_total_size, n, ib->rec, d_status, d_forward_ns, c.late_count, ib->flags,
                           c.pending);
        if (ib->n)
            hipLaunchKernelGGL(inbound_step_kernel, dim3((ib->n + 63) / 64), dim3(64),
                               WIN_CAP * sizeof(inb::Rec), s, c);
        if (stage::launched(err, "inbound") != SRT_OK) return SRT_ERR_HIP;
    } else {
        *c.late_count = 0;
        *c.pending = 0;
        const uint32_t n_sent = d_dst_ptr[ib->n] < n ? d_dst_ptr[ib->n] : n;
        for (uint32_t i = 0; i < n; ++i)
            stage_one(i, d_order, n_sent, d_deliver, d_total_size, n, ib->rec, d_status, d_forward_ns, ib->flags);
        for (uint32_t h = 0; h < ib->n; ++h) {
            inb::Run<false> r(c, h);
            r.run();
        }
    }
    if (seq_base) *seq_base = ib->base;
    ib->base += n_pkts;
    ib->prev_until = until_ns;
    return SRT_OK;
}

namespace {
// the stream drained; the flags and the pending count (16 bytes) on the host,
// and every host's state record when `states`
srt_status pull(srt_inbound *ib, bool states, uint32_t *flags, uint64_t *pending, srt_err *err) {
    uint32_t w[4] = {0, 0, 0, 0};
    if (!ib->plan) {
        std::memcpy(w, ib->h_flags, sizeof w);
    } else {
        if (!stage::use_device(ib->plan)) return SRT_ERR_HIP;
        hipStream_t s = ib->plan->stream;
        if (hipMemcpyAsync(w, ib->flags, sizeof w, hipMemcpyDeviceToHost, s) != hipSuccess ||
            (states && ib->n &&
             hipMemcpyAsync(ib->h_hosts.data(), ib->hosts, (size_t)ib->n * sizeof(inb::Host), hipMemcpyDeviceToHost,
                            s) != hipSuccess) ||
            hipStreamSynchronize(s) != hipSuccess) {
            set_err(err, SRT_ERR_HIP, "inbound: stream failed");
            return SRT_ERR_HIP;
        }
    }
    *flags = w[0];
    std::memcpy(pending, w + 2, 8);
    return SRT_OK;
}
}  // namespace

extern "C" srt_status srt_inbound_status(srt_inbound *ib, uint32_t *flags, uint64_t *n_pending, srt_err *err) {
    stage::begin(err);
    if (!ib) return stage::null_argument(err);
    uint32_t f = 0;
    uint64_t pending = 0;
    const srt_status st = pull(ib, false, &f, &pending, err);
    if (st != SRT_OK) return st;
    if (f) {
        if (ib->plan) (void)hipMemsetAsync(ib->flags, 0, 4, ib->plan->stream);
        else ib->h_flags[0] = 0;
    }
    if (n_pending) *n_pending = pending;
    if (flags) *flags = f & 31u;
    if (!f) return SRT_OK;
    const char *msg = f & F_BAD_ORDER                ? "inbound: order[] or dst_ptr[] out of range"
                      : f & inb::F_TIME_REGRESSION ? "inbound: an arrival earlier than the previous call's until_ns"
                      : f & inb::F_RING_OVERFLOW   ? "inbound: a host's ring overflowed (its results are invalid)"
                      : f & inb::F_LATE_OVERFLOW   ? "inbound: more late records than late_cap"
                      : f & inb::F_AFTER_UNTIL     ? "inbound: an arrival at or after until_ns was not taken"
                                                   : "inbound: a packet larger than its host's token bucket holds";
    set_err(err, SRT_ERR_INVALID, msg);
    return SRT_ERR_INVALID;
}

extern "C" srt_status srt_inbound_state(srt_inbound *ib, srt_inbound_host_state *out, srt_err *err) {
    stage::begin(err);
    if (!ib || (ib->n && !out)) return stage::null_argument(err);
    uint32_t f = 0;
    uint64_t pending = 0;
    const srt_status st = pull(ib, true, &f, &pending, err);
    if (st != SRT_OK) return st;
    for (uint32_t h = 0; h < ib->n; ++h) {
        const inb::Host &s = ib->h_hosts[h];
        srt_inbound_host_state &o = out[h];
        o.balance = s.balance;
        o.last_refill_ns = s.last_refill;
        o.interval_end_ns = s.interval_end;
        o.drop_next_ns = s.drop_next;
        o.current_drop_count = s.cur_drops;
        o.previous_drop_count = s.prev_drops;
        o.queue_len = s.ring_len;
        o.bytes_stored = s.bytes_stored;
        o.task_ns = s.task_ns;
        o.tasks_scheduled = s.tasks;
        o.mode = s.mode;
        o.cached = s.cached;
        o.overflow = s.overflow;
        o.reserved0 = 0;
    }
    return SRT_OK;
}

extern "C" srt_status srt_inbound_control_law(srt_inbound *ib, const uint64_t *counts, uint64_t n, int use_table,
                                              uint64_t *increments, srt_err *err) {
    stage::begin(err);
    if (!ib || (n && (!counts || !increments))) return stage::null_argument(err);
    if (!n) return SRT_OK;
    if (!ib->plan) {
        for (uint64_t i = 0; i < n; ++i)
            increments[i] = use_table ? inb::law_increment(ib->law_tab, counts[i]) : inb::law_increment_f64(counts[i]);
        return SRT_OK;
    }
    if (!stage::use_device(ib->plan)) return SRT_ERR_HIP;
    hipStream_t s = ib->plan->stream;
    uint64_t *d = nullptr;
    if (hipMalloc(&d, 16 * n) != hipSuccess) {
        set_err(err, SRT_ERR_OOM, "hipMalloc(control law) failed");
        return SRT_ERR_OOM;
    }
    hipError_t e = hipMemcpyAsync(d, counts, 8 * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(inbound_law_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s,
                           (const uint64_t *)d, n, use_table ? (const uint64_t *)ib->law_tab : nullptr, d + n);
        e = hipMemcpyAsync(increments, d + n, 8 * n, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d);
    if (e != hipSuccess) {
        set_err(err, SRT_ERR_HIP, "inbound: control law kernel failed");
        return SRT_ERR_HIP;
    }
    return SRT_OK;
}
