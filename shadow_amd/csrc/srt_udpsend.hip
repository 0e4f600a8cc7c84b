// srt_udpsend.hip -- the UDP send side for one window: every host's sockets'
// send buffers and its outbound relay in one fused step, a lane a host, in front
// of srt_sendbatch_run: UdpSocket::sendmsg (host/descriptor/socket/inet/udp.rs:
// 327-475), pull_out_packet (:170-195), MessageBuffer (:1056-1134), the SO_SNDBUF
// rule (:874-899), shutdown and close, Host::get_next_packet_priority
// (host/host.rs:715-720), and the relay of srt_outbound.hip.  The per-host step --
// checks, buffer, priority draw, qdisc, bucket, relay loop, wake-ups, event order,
// carry-over and every range check -- is srt_udpsend_step.h, compiled here for the
// device and for the host-only instance alike.
//
// Out of scope: TCP, payload bytes, the implicit bind, the CPU-delay model, the
// loopback interface (srt_loopback.hip).
//
// Device form, on the plan's stream; only status and state wait for it.
//   config: the steps sorted stably by target on the host, one launch: the first
//           step of a target applies the target's run in list order.
//   run, two launches:
//     (1) preset: a grid-stride pass: a call's 32-byte staged record (the form
//         the step reads and links), d_results preset with the call's user,
//         status 0, send_ns and send_rank UINT64_MAX; d_first_writable_ns
//         UINT64_MAX a slot; the call's counts zeroed;
//     (2) step: one lane owns one host (a wave 64 consecutive hosts).  The calls
//         are grouped by host, so the wave's are one contiguous span: it is
//         copied into LDS with coalesced loads when it is at most 1,536 records
//         (a longer span is walked in device memory).  The hosts' slots are one
//         contiguous span too: at most 320, their 88-byte state records and qdisc
//         entries are copied into LDS for the call and written back at its end
//         (more stay in device memory).  LDS a workgroup: 48 KB + 27.5 KB +
//         1.25 KB = 78,592 bytes, two workgroups a CU.  Each lane loads its
//         112-byte host record, walks its calls in time order against its pending
//         forward task, and stores the record back; a slot's ring is read only
//         when an earlier call left messages in it and written only for messages
//         still queued at until_ns.  The wave runs as long as its busiest host.
//         The step is instantiated for the four combinations, so that every
//         on-chip access is an LDS instruction.
// Every value is written with ordinary stores or vector atomics from plain C++.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <vector>

#include "srt_internal.h"
#include "srt_stage.h"
#include "srt_udpsend_step.h"

namespace {

static_assert(sizeof(udps::Sock) == udps::SOCK_BYTES && sizeof(udps::Host) == 112 && sizeof(udps::Rec) == 32 &&
                  sizeof(udps::RingEl) == 32 && sizeof(udps::State) == 64 && sizeof(srt_udp_send) == 40 &&
                  sizeof(srt_udpsend_result) == 40 && sizeof(srt_udpsend_late) == 48 && sizeof(srt_udpsend_op) == 16 &&
                  sizeof(srt_udpsend_socket_state) == 48 && sizeof(srt_udpsend_host_state) == 64,
              "record layouts");
static_assert(udps::LDS_BYTES <= 80 * 1024 && udps::LDS_SOCK_OFF % 16 == 0 && udps::LDS_Q_OFF % 8 == 0,
              "two workgroups share a CU's 160 KB");

using stage::BT;
using stage::set_err;
using udps::LDS_BYTES;
using udps::SLOT_LDS;
using udps::WIN_CAP;

constexpr uint32_t OPS_MIN = 1024;  // configuration steps a launch takes, at least

__global__ __launch_bounds__(BT) void udpsend_config_kernel(const udps::Ctx c) {
    for (uint64_t i : stage::grid_stride(c.n_ops)) udps::config_at(c, (uint32_t)i);
}

__global__ __launch_bounds__(BT) void udpsend_preset_kernel(const udps::Ctx c) {
    if (blockIdx.x == 0 && threadIdx.x == 0) udps::preset_words(c);
    for (uint64_t i : stage::grid_stride(c.n_calls)) udps::preset_call(c, (uint32_t)i);
    for (uint64_t x : stage::grid_stride(c.n_sockets)) c.first_writable[x] = udps::NONE;
}

template <bool WIN, bool SL>
__device__ __forceinline__ void run_host(const udps::Ctx &c, uint32_t h, uint32_t k0, uint32_t n, uint32_t sp0) {
    udps::Run<WIN, SL> r(c, h);
    r.win0 = k0, r.win_n = n, r.sp0 = sp0;
    r.run();
}

__global__ __launch_bounds__(64) void udpsend_step_kernel(const udps::Ctx c) {
    using udps::udps_lds;
    const uint32_t h0 = blockIdx.x * 64, h = h0 + threadIdx.x;
    const uint32_t h1 = min(h0 + 64, c.n_hosts);
    const uint32_t lim = min(c.host_ptr[c.n_hosts], c.n_calls);
    const uint32_t k0 = min(c.host_ptr[h0], lim), k1 = min(c.host_ptr[h1], lim);
    const uint32_t n = k1 > k0 ? k1 - k0 : 0;
    const bool staged = n <= WIN_CAP;
    if (staged) {
        const uint4 *src = reinterpret_cast<const uint4 *>(c.rec + k0);  // 32-byte records: two 16-byte words each
        uint4 *dst = reinterpret_cast<uint4 *>(udps_lds);
        for (uint32_t i = threadIdx.x; i < 2 * n; i += 64) dst[i] = src[i];
    }
    // the wave's slots: one contiguous span of the slot records and of the qdisc arrays
    const uint32_t sp0 = min(c.socket_ptr[h0], c.n_sockets), sp1 = min(c.socket_ptr[h1], c.n_sockets);
    const uint32_t n_sl = sp1 > sp0 ? sp1 - sp0 : 0;
    const bool sl = n_sl <= SLOT_LDS;
    uint64_t *l_sock = reinterpret_cast<uint64_t *>(udps_lds + udps::LDS_SOCK_OFF);
    uint32_t *l_q = reinterpret_cast<uint32_t *>(udps_lds + udps::LDS_Q_OFF);
    constexpr uint32_t SW = udps::SOCK_BYTES / 8;
    if (sl) {
        const uint64_t *src = reinterpret_cast<const uint64_t *>(c.socks + sp0);
        for (uint32_t i = threadIdx.x; i < SW * n_sl; i += 64) l_sock[i] = src[i];
        for (uint32_t i = threadIdx.x; i < n_sl; i += 64) l_q[i] = c.sockq[sp0 + i];
    }
    __syncthreads();
    if (h < c.n_hosts) {
        if (staged) {
            if (sl) run_host<true, true>(c, h, k0, n, sp0);
            else run_host<true, false>(c, h, k0, n, sp0);
        } else {
            if (sl) run_host<false, true>(c, h, k0, n, sp0);
            else run_host<false, false>(c, h, k0, n, sp0);
        }
    }
    __syncthreads();
    if (sl) {
        uint64_t *dst = reinterpret_cast<uint64_t *>(c.socks + sp0);
        for (uint32_t i = threadIdx.x; i < SW * n_sl; i += 64) dst[i] = l_sock[i];
        for (uint32_t i = threadIdx.x; i < n_sl; i += 64) c.sockq[sp0 + i] = l_q[i];
    }
}

// srt_udpsend_cached_seq: one thread a host
__global__ __launch_bounds__(BT) void udpsend_cached_seq_kernel(const udps::Host *__restrict__ hosts, uint32_t n_hosts,
                                                                uint64_t *__restrict__ seq) {
    const uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h < n_hosts) seq[h] = udps::cached_seq_of(hosts[h]);
}

}  // namespace

struct srt_udpsend {
    srt_plan *plan = nullptr;  // nullptr: host-only
    uint32_t n_hosts = 0, n_sockets = 0, ring_cap = 0, ops_cap = 0, call_no = 0;
    uint64_t base = 0, prev_until = 0;
    void *mem = nullptr;  // device form: everything but the staged records in one allocation; host-only: h_mem
    udps::Rec *rec = nullptr;
    size_t rec_cap = 0;
    srt_udpsend_op *d_ops = nullptr;
    std::vector<uint64_t> h_mem;
    std::vector<udps::Rec> h_rec;
    std::vector<udps::Host> h_hosts;
    std::vector<udps::Sock> h_socks;
    std::vector<srt_udpsend_op> h_sorted;
    std::vector<uint32_t> h_order;
    udps::Ctx base_ctx;
};

namespace srt {
// srt_init: loads this unit's code object (srt::preload_kernels)
hipError_t preload_udpsend() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&udpsend_step_kernel));
}
}  // namespace srt

extern "C" uint32_t srt_udpsend_window_bytes(void) { return LDS_BYTES; }

extern "C" void srt_udpsend_destroy(srt_udpsend *us) {
    if (!us) return;
    if (us->plan) {
        (void)stage::use_device(us->plan);
        (void)hipStreamSynchronize(us->plan->stream);
        (void)hipFree(us->mem);
        (void)hipFree(us->rec);
    }
    delete us;
}

extern "C" srt_status srt_udpsend_create(srt_plan *plan, uint32_t n_hosts, const uint32_t *socket_ptr,
                                         const uint32_t *host_ip_be, const uint64_t *bw_up_bytes_per_s, uint32_t qdisc,
                                         uint32_t ring_cap, uint32_t late_cap_hint, srt_udpsend **out, srt_err *err) {
    stage::begin(err);
    if (!out || !socket_ptr || (n_hosts && (!host_ip_be || !bw_up_bytes_per_s))) return stage::null_argument(err);
    *out = nullptr;
    bool ok = n_hosts < 0x80000000u && ring_cap < 0x7fffffffu && late_cap_hint < 0x80000000u && qdisc <= SRT_QDISC_RR &&
              socket_ptr[0] == 0;
    for (uint32_t h = 0; ok && h < n_hosts; ++h)
        ok = socket_ptr[h] <= socket_ptr[h + 1] &&
             (uint64_t)(socket_ptr[h + 1] - socket_ptr[h]) * ((uint64_t)ring_cap + 1) < 0x80000000ull;
    ok = ok && socket_ptr[n_hosts] < 0x80000000u;
    if (!ok) {
        set_err(err, SRT_ERR_INVALID,
                "udpsend: qdisc, n_hosts, late_cap_hint or a host's slots * (ring_cap + 1) (below 2^31) out of range, or "
                "socket_ptr not 0-based, nondecreasing and below 2^31");
        return SRT_ERR_INVALID;
    }
    srt_udpsend *us = new (std::nothrow) srt_udpsend;
    if (!us) return SRT_ERR_OOM;
    const uint32_t n_sockets = socket_ptr[n_hosts];
    us->plan = plan;
    us->n_hosts = n_hosts;
    us->n_sockets = n_sockets;
    us->ring_cap = ring_cap;
    us->ops_cap = std::max(n_sockets + n_hosts, OPS_MIN);
    // the call-wide words; the hosts; the slots; the rings; the qdisc arrays; socket_ptr; the steps
    const size_t hosts = sizeof(udps::Host) * (size_t)n_hosts, socks = sizeof(udps::Sock) * (size_t)n_sockets,
                 ring = sizeof(udps::RingEl) * (size_t)n_sockets * ((size_t)ring_cap + 1), sockq = 4 * (size_t)n_sockets,
                 sptr = 4 * ((size_t)n_hosts + 1), ops = 16 * (size_t)us->ops_cap;
    const auto up16 = [](size_t v) { return (v + 15) / 16 * 16; };
    const size_t hosts_at = 64, ring_at = up16(hosts_at + hosts), socks_at = ring_at + ring, ops_at = up16(socks_at + socks),
                 sockq_at = ops_at + ops, sptr_at = sockq_at + up16(sockq), bytes = sptr_at + up16(sptr);
    try {
        us->h_hosts.assign(n_hosts, udps::Host{});
        us->h_socks.assign(n_sockets, udps::Sock{});
        for (uint32_t x = 0; x < n_sockets; ++x) udps::sock_init(us->h_socks[x]);
        for (uint32_t h = 0; h < n_hosts; ++h) {
            udps::Host &s = us->h_hosts[h];
            // create_token_bucket (relay/mod.rs:277-287)
            s.refill = relay::bucket_refill(bw_up_bytes_per_s[h]);
            s.capacity = relay::sat_add(s.refill, relay::MTU);
            s.balance = s.capacity;
            s.task_ns = udps::NONE;
            s.next_priority = 1;  // host.rs:262
            s.ip = host_ip_be[h];
        }
        if (!plan) us->h_mem.assign(bytes / 8 + 2, 0);
    } catch (const std::bad_alloc &) {
        ok = false;
    }
    if (ok && !plan) {
        us->mem = us->h_mem.data();
    } else if (ok) {
        srt::init_wait();
        ok = stage::use_device(plan);
        ok = ok && hipMalloc(&us->mem, bytes + 16) == hipSuccess;
        ok = ok && hipMemset(us->mem, 0, bytes + 16) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            (void)hipFree(us->mem);
        }
    }
    if (!ok) {
        delete us;
        set_err(err, SRT_ERR_OOM, "udpsend: allocation failed");
        return SRT_ERR_OOM;
    }
    udps::Ctx &c = us->base_ctx;
    std::memset(&c, 0, sizeof c);
    char *p = static_cast<char *>(us->mem);
    c.st = reinterpret_cast<udps::State *>(p);
    c.hosts = reinterpret_cast<udps::Host *>(p + hosts_at);
    c.ring = reinterpret_cast<udps::RingEl *>(p + ring_at);
    c.socks = reinterpret_cast<udps::Sock *>(p + socks_at);
    us->d_ops = reinterpret_cast<srt_udpsend_op *>(p + ops_at);
    c.sockq = reinterpret_cast<uint32_t *>(p + sockq_at);
    uint32_t *sp = reinterpret_cast<uint32_t *>(p + sptr_at);
    c.socket_ptr = sp;
    c.n_hosts = n_hosts;
    c.n_sockets = n_sockets;
    c.ring_cap = ring_cap;
    c.qdisc = qdisc;
    if (!plan) {
        if (n_hosts) std::memcpy(c.hosts, us->h_hosts.data(), hosts);
        if (n_sockets) std::memcpy(c.socks, us->h_socks.data(), socks);
        std::memcpy(sp, socket_ptr, sptr);
    } else {
        bool up = (!n_hosts || hipMemcpy(c.hosts, us->h_hosts.data(), hosts, hipMemcpyHostToDevice) == hipSuccess) &&
                  (!n_sockets || hipMemcpy(c.socks, us->h_socks.data(), socks, hipMemcpyHostToDevice) == hipSuccess) &&
                  hipMemcpy(sp, socket_ptr, sptr, hipMemcpyHostToDevice) == hipSuccess;
        up = up && hipFuncSetAttribute((const void *)udpsend_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)LDS_BYTES) == hipSuccess;
        if (!up) {
            (void)hipGetLastError();
            (void)hipFree(us->mem);
            delete us;
            set_err(err, SRT_ERR_HIP, "udpsend: device initialisation failed, or the step kernel's LDS was refused");
            return SRT_ERR_HIP;
        }
    }
    *out = us;
    return SRT_OK;
}

extern "C" srt_status srt_udpsend_config(srt_udpsend *us, const srt_udpsend_op *ops, uint64_t n, srt_err *err) {
    stage::begin(err);
    if (!us || (n && !ops)) return stage::null_argument(err);
    if (n >= 0x80000000ull) {
        set_err(err, SRT_ERR_INVALID, "udpsend: more than 2^31-1 configuration steps in one call");
        return SRT_ERR_INVALID;
    }
    for (uint64_t i = 0; i < n; ++i) {
        const bool host_op = ops[i].op == SRT_UDPSEND_SET_NEXT_PRIORITY;
        if (ops[i].op < SRT_UDPSEND_OPEN || ops[i].op > SRT_UDPSEND_SET_NEXT_PRIORITY ||
            ops[i].slot >= (host_op ? us->n_hosts : us->n_sockets)) {
            set_err(err, SRT_ERR_INVALID,
                    "udpsend: a configuration step's slot is not below n_sockets (its host not below n_hosts) or its op is "
                    "unknown (nothing was changed)");
            return SRT_ERR_INVALID;
        }
    }
    if (!n) return SRT_OK;
    udps::Ctx c = us->base_ctx;
    if (!us->plan) {
        c.ops = ops;
        c.n_ops = (uint32_t)n;
        udps::host_config(c);
        return SRT_OK;
    }
    // steps on different targets commute: sorted stably by target, a target's steps are one run of the list.  The
    // sorted copy is the instance's: the stream is waited for first, so the previous call's copy has left it.
    if (!stage::use_device(us->plan)) return SRT_ERR_HIP;
    hipStream_t s = us->plan->stream;
    (void)hipStreamSynchronize(s);
    try {
        us->h_order.resize(n);
        us->h_sorted.resize(n);
    } catch (const std::bad_alloc &) {
        set_err(err, SRT_ERR_OOM, "udpsend: host allocation failed");
        return SRT_ERR_OOM;
    }
    const auto key = [ops](uint32_t a) {
        return (uint64_t)(ops[a].op == SRT_UDPSEND_SET_NEXT_PRIORITY) << 32 | ops[a].slot;
    };
    std::iota(us->h_order.begin(), us->h_order.end(), 0u);
    std::stable_sort(us->h_order.begin(), us->h_order.end(), [&key](uint32_t a, uint32_t b) { return key(a) < key(b); });
    for (uint64_t i = 0; i < n; ++i) us->h_sorted[i] = ops[us->h_order[i]];
    c.ops = us->d_ops;
    // a launch takes ops_cap steps; a target's run cut by a launch's end goes on in the next, in stream order
    for (uint64_t at = 0; at < n; at += us->ops_cap) {
        const uint64_t m = std::min<uint64_t>(us->ops_cap, n - at);
        if (hipMemcpyAsync(us->d_ops, us->h_sorted.data() + at, 16 * m, hipMemcpyHostToDevice, s) != hipSuccess) {
            (void)hipGetLastError();
            set_err(err, SRT_ERR_HIP, "udpsend: copying the configuration steps failed");
            return SRT_ERR_HIP;
        }
        c.n_ops = (uint32_t)m;
        hipLaunchKernelGGL(udpsend_config_kernel, dim3(stage::strided_blocks(m, stage::LATE_BLOCKS)), dim3(BT), 0, s, c);
    }
    return stage::launched(err, "udpsend");
}

extern "C" srt_status srt_udpsend_run(srt_udpsend *us, const uint32_t *d_call_host_ptr, const srt_udp_send *d_calls,
                                      uint64_t n_calls, uint64_t until_ns, uint64_t bootstrap_end_ns,
                                      srt_udpsend_result *d_results, uint32_t *d_pds_status, uint64_t *d_send_ns,
                                      uint64_t *d_send_rank, srt_outbound_late *d_late, uint32_t late_cap,
                                      uint32_t *d_late_count, srt_udpsend_late *d_late_results,
                                      uint32_t late_results_cap, uint32_t *d_late_results_count,
                                      uint64_t *d_first_writable_ns, uint64_t *seq_base, srt_err *err) {
    stage::begin(err);
    if (!us || !d_call_host_ptr || (us->n_sockets && !d_first_writable_ns) || (late_cap && !d_late) ||
        (late_results_cap && !d_late_results) ||
        (n_calls && (!d_calls || !d_results || !d_pds_status || !d_send_ns || !d_send_rank)))
        return stage::null_argument(err);
    if (n_calls >= 0x80000000ull || late_cap >= 0x80000000u || late_results_cap >= 0x80000000u) {
        set_err(err, SRT_ERR_INVALID, "udpsend: more than 2^31-1 calls, late packets or late results in one call");
        return SRT_ERR_INVALID;
    }
    if (until_ns < us->prev_until) {
        set_err(err, SRT_ERR_INVALID, "udpsend: until_ns earlier than the previous call's");
        return SRT_ERR_INVALID;
    }
    const uint32_t n = (uint32_t)n_calls;
    if (us->plan && !stage::use_device(us->plan)) return SRT_ERR_HIP;
    if (n > us->rec_cap) {  // the staged records grow with the largest list seen
        if (us->plan) {
            (void)hipStreamSynchronize(us->plan->stream);
            (void)hipFree(us->rec);
            us->rec = nullptr;
            us->rec_cap = 0;
            if (hipMalloc(&us->rec, (size_t)n * sizeof(udps::Rec)) != hipSuccess) {
                (void)hipGetLastError();
                set_err(err, SRT_ERR_OOM, "hipMalloc(udpsend records) failed");
                return SRT_ERR_OOM;
            }
        } else {
            try {
                us->h_rec.resize(n);
            } catch (const std::bad_alloc &) {
                set_err(err, SRT_ERR_OOM, "udpsend: host allocation failed");
                return SRT_ERR_OOM;
            }
            us->rec = us->h_rec.data();
        }
        us->rec_cap = n;
    }
    if (!++us->call_no) us->call_no = 1;  // 0 is "never" in a slot's record
    udps::Ctx c = us->base_ctx;
    c.rec = us->rec;
    c.calls = d_calls;
    c.host_ptr = d_call_host_ptr;
    c.results = d_results;
    c.status = d_pds_status;
    c.send_ns = d_send_ns;
    c.send_rank = d_send_rank;
    c.late = d_late;
    c.late_cap = late_cap;
    c.late_count = d_late_count ? d_late_count : &c.st->own_late_count;
    c.late_res = d_late_results;
    c.late_res_cap = late_results_cap;
    c.late_res_count = d_late_results_count ? d_late_results_count : &c.st->own_late_res_count;
    c.first_writable = d_first_writable_ns;
    c.base = us->base;
    c.until = until_ns;
    c.boot_end = bootstrap_end_ns;
    c.prev_until = us->prev_until;
    c.n_calls = n;
    c.call_no = us->call_no;
    if (!us->plan) {
        udps::host_run(c);
    } else {
        hipStream_t s = us->plan->stream;
        const uint64_t items = std::max<uint64_t>(std::max<uint64_t>(n, us->n_sockets), 1);
        hipLaunchKernelGGL(udpsend_preset_kernel, dim3(stage::strided_blocks(items, stage::NOTE_BLOCKS)), dim3(BT), 0, s,
                           c);
        if (us->n_hosts)
            hipLaunchKernelGGL(udpsend_step_kernel, dim3((us->n_hosts + 63) / 64), dim3(64), LDS_BYTES, s, c);
        if (stage::launched(err, "udpsend") != SRT_OK) return SRT_ERR_HIP;
    }
    if (seq_base) *seq_base = us->base;
    us->base += n_calls;
    us->prev_until = until_ns;
    return SRT_OK;
}

extern "C" srt_status srt_udpsend_status(srt_udpsend *us, uint32_t *flags, uint64_t *n_pending, uint64_t *n_accepted,
                                         uint64_t *n_would_block, uint64_t *n_armed, srt_err *err) {
    stage::begin(err);
    if (!us) return stage::null_argument(err);
    udps::State w;
    if (!us->plan) {
        w = *us->base_ctx.st;
        us->base_ctx.st->flags = 0;
    } else {
        if (!stage::use_device(us->plan)) return SRT_ERR_HIP;
        const srt_status st = stage::read_status(us->plan, &w, us->base_ctx.st, sizeof w, err, "udpsend");
        if (st != SRT_OK) return st;
    }
    const uint32_t f = w.flags & udps::F_ALL;
    if (flags) *flags = f;
    if (n_pending) *n_pending = w.pending;
    if (n_accepted) *n_accepted = w.n_acc;
    if (n_would_block) *n_would_block = w.n_wb;
    if (n_armed) *n_armed = w.n_arm;
    if (!f) return SRT_OK;
    if (err) {
        err->code = SRT_ERR_INVALID;
        std::snprintf(err->msg, sizeof err->msg, "udpsend:%s%s%s%s%s%s%s%s%s%s%s%s",
                      f & udps::F_RING_OVERFLOW ? " ring overflow;" : "", f & udps::F_LATE_OVERFLOW ? " late overflow;" : "",
                      f & udps::F_LATE_RESULT_OVERFLOW ? " late result overflow;" : "",
                      f & udps::F_TIME_REGRESSION ? " time regression;" : "", f & udps::F_CALL_ORDER ? " call order;" : "",
                      f & udps::F_AFTER_UNTIL ? " after until;" : "", f & udps::F_OVERSIZE ? " oversize;" : "",
                      f & udps::F_BAD_SOCKET ? " bad socket;" : "", f & udps::F_UNBOUND ? " unbound;" : "",
                      f & udps::F_LOOPBACK ? " loopback;" : "", f & udps::F_ARMED_TWICE ? " armed twice;" : "",
                      f & udps::F_REOPEN_BUSY ? " reopen busy;" : "");
    }
    return SRT_ERR_INVALID;
}

extern "C" srt_status srt_udpsend_state(srt_udpsend *us, srt_udpsend_host_state *hosts, srt_udpsend_socket_state *socks,
                                        srt_err *err) {
    stage::begin(err);
    if (!us) return stage::null_argument(err);
    const udps::Host *hh = us->base_ctx.hosts;
    const udps::Sock *ss = us->base_ctx.socks;
    if (us->plan) {
        if (!stage::use_device(us->plan)) return SRT_ERR_HIP;
        hipStream_t s = us->plan->stream;
        if ((us->n_hosts && hipMemcpyAsync(us->h_hosts.data(), hh, sizeof(udps::Host) * (size_t)us->n_hosts,
                                           hipMemcpyDeviceToHost, s) != hipSuccess) ||
            (us->n_sockets && hipMemcpyAsync(us->h_socks.data(), ss, sizeof(udps::Sock) * (size_t)us->n_sockets,
                                             hipMemcpyDeviceToHost, s) != hipSuccess) ||
            hipStreamSynchronize(s) != hipSuccess) {
            (void)hipGetLastError();
            set_err(err, SRT_ERR_HIP, "udpsend: stream failed");
            return SRT_ERR_HIP;
        }
        hh = us->h_hosts.data();
        ss = us->h_socks.data();
    }
    for (uint32_t h = 0; hosts && h < us->n_hosts; ++h) {
        const udps::Host &s = hh[h];
        srt_udpsend_host_state &o = hosts[h];
        o.balance = s.balance;
        o.last_refill_ns = s.last_refill;
        o.task_ns = s.task_ns;
        o.tasks_scheduled = s.tasks;
        o.sent_total = s.sent;
        o.queue_len = s.n_queued;
        o.cached = s.cached;
        o.overflow = s.overflow;
        o.next_priority = s.next_priority;
    }
    for (uint32_t x = 0; socks && x < us->n_sockets; ++x) {
        const udps::Sock &s = ss[x];
        srt_udpsend_socket_state &o = socks[x];
        o.len_bytes = s.len_bytes;
        o.soft_limit = s.soft_limit;
        o.armed_seq = s.armed_seq;
        o.n_msgs = s.n_msgs;
        o.bound_ip_be = s.bind_ip;
        o.peer_ip_be = s.peer_ip;
        o.bound_port_be = s.bind_port;
        o.peer_port_be = s.peer_port;
        o.open = (s.bits & udps::B_OPEN) != 0;
        o.shut_wr = (s.bits & udps::B_SHUT_WR) != 0;
        o.bound = (s.bits & udps::B_BOUND) != 0;
        o.has_peer = (s.bits & udps::B_PEER) != 0;
        o.overflow = (s.bits & udps::B_OVERFLOW) != 0;
        o.reserved0 = 0;
        o.reserved1 = 0;
    }
    return SRT_OK;
}

extern "C" srt_status srt_udpsend_cached_seq(srt_udpsend *us, uint64_t *d_seq, srt_err *err) {
    stage::begin(err);
    if (!us || (us->n_hosts && !d_seq)) return stage::null_argument(err);
    if (!us->n_hosts) return SRT_OK;
    if (!us->plan) {
        for (uint32_t h = 0; h < us->n_hosts; ++h) d_seq[h] = udps::cached_seq_of(us->base_ctx.hosts[h]);
        return SRT_OK;
    }
    if (!stage::use_device(us->plan)) return SRT_ERR_HIP;
    hipLaunchKernelGGL(udpsend_cached_seq_kernel, dim3((us->n_hosts + BT - 1) / BT), dim3(BT), 0, us->plan->stream,
                       us->base_ctx.hosts, us->n_hosts, d_seq);
    return stage::launched(err, "udpsend");
}
