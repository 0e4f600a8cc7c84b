// srt_udprecv.hip -- UDP sockets' receive buffers and reads for one window, a
// lane a socket slot, behind srt_deliver_run: UdpSocket::push_in_packet
// (host/descriptor/socket/inet/udp.rs:108-168), recvmsg (:477-572),
// MessageBuffer (:1056-1134) and the SO_RCVBUF rule (:900-925).  The per-slot
// step -- buffer, peer, reads, the blocked read, the ring and its range checks --
// is srt_udprecv_step.h, compiled here for the device and for the host-only
// instance alike.
//
// Out of scope: TCP sockets, the send buffer, shutdown(2), the CPU-delay model.
//
// Device form, on the plan's stream; only status and state wait for it.
//   note:   one launch, a copy of the round's metas into the ring.
//   config: the steps sorted stably by slot on the host, one launch: the first
//           step of a slot applies the slot's run in list order.
//   run, two launches:
//     (1) stage: a grid-stride pass over the delivery records and the reads: the
//         gathers behind a record (status, socket, forward time, the note by
//         tag, whether the slot is open here) done once into a 32-byte record in
//         list order, d_rx_status preset to deliver's status, d_results preset,
//         a read no walk owns answered -EBADF, *d_late_count zeroed;
//     (2) step: one lane owns one slot (a wave 64 consecutive slots).  The
//         slots' hosts are consecutive, so their staged records are one
//         contiguous span of the list, and so are their reads: the wave copies
//         them into LDS with coalesced loads: the records if they fit the
//         window, the reads if they fit what is left (a list that does not is
//         walked in device memory instead).  Each lane loads its 88-byte state, walks
//         its host's sub-span picking out its own records and reads, merged by
//         time, and stores the state back.  The ring is read only when an
//         earlier call left messages in it and written only for messages still
//         buffered at the end.  A lane re-reads its host's whole sub-span: LDS
//         reads proportional to records per host, the time bound of inbound's
//         per-host walk, and no dependent trip to device memory per packet
//         (DESIGN.md 3.5).
//   status: the slots' counts summed by one launch of one workgroup.
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
#include "srt_udprecv_step.h"

namespace {

static_assert(sizeof(udprecv::Sock) == 88 && sizeof(udprecv::Msg) == 32 && sizeof(udprecv::Rec) == 32 &&
                  sizeof(udprecv::State) == 32 && sizeof(srt_udp_meta) == 16 && sizeof(srt_udp_read) == 24 &&
                  sizeof(srt_udp_result) == 56 && sizeof(srt_udp_late) == 64 && sizeof(srt_udprecv_op) == 16 &&
                  sizeof(srt_udprecv_socket_state) == 48,
              "record layouts");

using stage::BT;
using stage::ST;
using stage::set_err;

// Bytes of staged records and reads a wave may hold in LDS (80 KB: two workgroups share a CU's 160 KB)
constexpr uint32_t WIN_BYTES = 80 * 1024;
constexpr uint32_t OPS_MIN = 1024;  // configuration steps a launch takes, at least

__global__ __launch_bounds__(BT) void udprecv_note_kernel(const udprecv::Ctx c) {
    for (uint64_t i = (uint64_t)c.note_first + (uint64_t)blockIdx.x * BT + threadIdx.x; i < c.note_n;
         i += (uint64_t)gridDim.x * BT)
        udprecv::note_store(c, (uint32_t)i);
}

__global__ __launch_bounds__(BT) void udprecv_config_kernel(const udprecv::Ctx c) {
    for (uint64_t i : stage::grid_stride(c.n_ops)) udprecv::config_at(c, (uint32_t)i);
}

__global__ __launch_bounds__(BT) void udprecv_stage_kernel(const udprecv::Ctx c) {
    const uint32_t lim = udprecv::walked(c), rlim = udprecv::reads_walked(c);
    if (blockIdx.x == 0 && threadIdx.x == 0) *c.late_count = 0;
    for (uint64_t k : stage::grid_stride(lim)) udprecv::stage_record(c, (uint32_t)k);
    for (uint64_t r : stage::grid_stride(c.n_reads)) udprecv::stage_read(c, (uint32_t)r, rlim);
}

__global__ __launch_bounds__(64) void udprecv_step_kernel(const udprecv::Ctx c) {
    extern __shared__ __attribute__((aligned(16))) char udprecv_window[];
    const uint32_t s0 = blockIdx.x * 64, slot = s0 + threadIdx.x;
    const uint32_t s1 = min(s0 + 64, c.n_sockets);  // s0 < n_sockets: the grid is sized to the slots
    const uint32_t lim = udprecv::walked(c), rlim = udprecv::reads_walked(c);
    // the wave's hosts, hence its spans of the two lists
    const uint32_t ha = c.socks[s0].host, hb = c.socks[s1 - 1].host;
    const uint32_t k0 = min(c.out_host_ptr[ha], lim), k1 = max(min(c.out_host_ptr[hb + 1], lim), k0);
    uint32_t r0 = 0, r1 = 0;
    if (c.read_host_ptr) r0 = min(c.read_host_ptr[ha], rlim), r1 = max(min(c.read_host_ptr[hb + 1], rlim), r0);
    const uint32_t n = k1 - k0, nr = r1 - r0;
    // the two lists are staged one by one: the records if they fit the window, the reads if they fit what is left
    const uint64_t rec_bytes = (uint64_t)n * sizeof(udprecv::Rec), rd_bytes = (uint64_t)nr * sizeof(srt_udp_read);
    const bool in_rec = rec_bytes <= c.win_bytes;
    const bool in_rd = rd_bytes <= c.win_bytes - (in_rec ? rec_bytes : 0);
    udprecv::Rec *w_rec = reinterpret_cast<udprecv::Rec *>(udprecv_window);
    srt_udp_read *w_rd = reinterpret_cast<srt_udp_read *>(udprecv_window + (in_rec ? rec_bytes : 0));
    if (in_rec) {
        const uint4 *src = reinterpret_cast<const uint4 *>(c.rec + k0);  // 32-byte records: two 16-byte words each
        uint4 *dst = reinterpret_cast<uint4 *>(w_rec);
        for (uint32_t i = threadIdx.x; i < 2 * n; i += 64) dst[i] = src[i];
    }
    if (in_rd) {
        const uint64_t *rs = reinterpret_cast<const uint64_t *>(c.reads + r0);  // 24-byte reads: three words each
        uint64_t *rd = reinterpret_cast<uint64_t *>(w_rd);
        for (uint32_t i = threadIdx.x; i < 3 * nr; i += 64) rd[i] = rs[i];
    }
    __syncthreads();
    if (slot >= c.n_sockets) return;
    const auto walk = [&](udprecv::Rec *rec, const srt_udp_read *rd, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) {
        const udprecv::Win w{rec, rd, a0, a1, b0, b1};
        udprecv::Walk wk(c, w, slot);
        wk.run(lim, rlim);
    };
    // one call site a combination, so each walk knows which of its lists are in LDS
    if (in_rec && in_rd) walk(w_rec, w_rd, k0, k1, r0, r1);
    else if (in_rec) walk(w_rec, c.reads, k0, k1, 0, rlim);
    else if (in_rd) walk(c.rec, w_rd, 0, lim, r0, r1);
    else walk(c.rec, c.reads, 0, lim, 0, rlim);
}

// srt_udprecv_status: the slots' counts, summed by one workgroup
__global__ __launch_bounds__(ST) void udprecv_sum_kernel(const udprecv::Ctx c) {
    __shared__ uint64_t wsum[3][ST / 64];
    const uint32_t t = threadIdx.x;
    unsigned long long a = 0, b = 0, d = 0;
    for (uint32_t x = t; x < c.n_sockets; x += ST) a += c.socks[x].n_proc, b += c.socks[x].n_buf, d += c.socks[x].n_drop;
    for (uint32_t off = 32; off > 0; off >>= 1)
        a += __shfl_xor(a, off), b += __shfl_xor(b, off), d += __shfl_xor(d, off);
    if ((t & 63) == 0) wsum[0][t >> 6] = a, wsum[1][t >> 6] = b, wsum[2][t >> 6] = d;
    __syncthreads();
    if (t == 0) {
        uint64_t x = 0, y = 0, z = 0;
        for (uint32_t w = 0; w < ST / 64; ++w) x += wsum[0][w], y += wsum[1][w], z += wsum[2][w];
        c.st->n_proc = x;
        c.st->n_buf = y;
        c.st->n_drop = z;
    }
}

}  // namespace

struct srt_udprecv {
    srt_plan *plan = nullptr;  // nullptr: host-only
    uint32_t n_hosts = 0, n_sockets = 0, ring_cap = 0, ops_cap = 0;
    uint64_t note_cap = 0, note_end = 0, read_base = 0, prev_until = 0;
    void *mem = nullptr;  // device form: everything but the staged records in one allocation; host-only: h_mem
    udprecv::Rec *rec = nullptr;
    size_t rec_cap = 0;
    srt_udprecv_op *d_ops = nullptr;
    uint32_t *own_late_count = nullptr;  // for a caller that passes none
    std::vector<uint64_t> h_mem;
    std::vector<udprecv::Rec> h_rec;
    std::vector<udprecv::Sock> h_socks;    // state(): the copy on the host
    std::vector<srt_udprecv_op> h_sorted;  // config(): the steps in slot order
    std::vector<uint32_t> h_order;
    udprecv::Ctx base;
};

namespace srt {
// srt_init: loads this unit's code object (srt::preload_kernels)
hipError_t preload_udprecv() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&udprecv_step_kernel));
}
}  // namespace srt

extern "C" uint32_t srt_udprecv_window_bytes(void) { return WIN_BYTES; }

extern "C" void srt_udprecv_destroy(srt_udprecv *ur) {
    if (!ur) return;
    if (ur->plan) {
        (void)stage::use_device(ur->plan);
        (void)hipStreamSynchronize(ur->plan->stream);
        (void)hipFree(ur->mem);
        (void)hipFree(ur->rec);
    }
    delete ur;
}

extern "C" srt_status srt_udprecv_create(srt_plan *plan, uint32_t n_hosts, const uint32_t *socket_ptr, uint32_t ring_cap,
                                         uint64_t note_cap, uint32_t late_cap_hint, srt_udprecv **out, srt_err *err) {
    stage::begin(err);
    if (!out || !socket_ptr) return stage::null_argument(err);
    *out = nullptr;
    bool ok = n_hosts < 0x80000000u && ring_cap < 0x80000000u && late_cap_hint < 0x80000000u &&
              note_cap <= (1ull << 31) && socket_ptr[0] == 0;
    for (uint32_t h = 0; ok && h < n_hosts; ++h) ok = socket_ptr[h] <= socket_ptr[h + 1];
    ok = ok && socket_ptr[n_hosts] < 0x80000000u;
    if (!ok) {
        set_err(err, SRT_ERR_INVALID,
                "udprecv: n_hosts, ring_cap, late_cap_hint (below 2^31), note_cap (at most 2^31) out of range, or "
                "socket_ptr not 0-based, nondecreasing and below 2^31");
        return SRT_ERR_INVALID;
    }
    srt_udprecv *ur = new (std::nothrow) srt_udprecv;
    if (!ur) return SRT_ERR_OOM;
    const uint32_t n_sockets = socket_ptr[n_hosts];
    ur->plan = plan;
    ur->n_hosts = n_hosts;
    ur->n_sockets = n_sockets;
    ur->ring_cap = ring_cap;
    ur->note_cap = note_cap;
    ur->ops_cap = std::max(n_sockets, OPS_MIN);
    // state words; the late count of a caller that passes none; the slots; the rings; the note ring; the steps
    const size_t head = 32 + 16, socks = sizeof(udprecv::Sock) * (size_t)n_sockets,
                 ring = sizeof(udprecv::Msg) * (size_t)n_sockets * ring_cap, note = 16 * (size_t)note_cap,
                 ops = 16 * (size_t)ur->ops_cap;
    const size_t socks_at = head, ring_at = (socks_at + socks + 15) / 16 * 16, note_at = ring_at + ring,
                 ops_at = note_at + note, bytes = ops_at + ops;
    try {
        ur->h_socks.assign(n_sockets, udprecv::Sock{});
        for (uint32_t h = 0; h < n_hosts; ++h)
            for (uint32_t x = socket_ptr[h]; x < socket_ptr[h + 1]; ++x) {
                udprecv::sock_reset(ur->h_socks[x], 0, 0);
                ur->h_socks[x].host = h;
            }
        if (!plan) ur->h_mem.assign(bytes / 8 + 2, 0);
    } catch (const std::bad_alloc &) {
        ok = false;
    }
    if (ok && !plan) {
        ur->mem = ur->h_mem.data();
    } else if (ok) {
        srt::init_wait();
        ok = stage::use_device(plan);
        ok = ok && hipMalloc(&ur->mem, bytes + 16) == hipSuccess;
        ok = ok && hipMemset(ur->mem, 0, bytes + 16) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            (void)hipFree(ur->mem);
        }
    }
    if (!ok) {
        delete ur;
        set_err(err, SRT_ERR_OOM, "udprecv: allocation failed");
        return SRT_ERR_OOM;
    }
    udprecv::Ctx &c = ur->base;
    std::memset(&c, 0, sizeof c);
    char *p = static_cast<char *>(ur->mem);
    c.st = reinterpret_cast<udprecv::State *>(p);
    ur->own_late_count = reinterpret_cast<uint32_t *>(p + 32);
    c.socks = reinterpret_cast<udprecv::Sock *>(p + socks_at);
    c.ring = reinterpret_cast<udprecv::Msg *>(p + ring_at);
    c.note_ring = reinterpret_cast<srt_udp_meta *>(p + note_at);
    ur->d_ops = reinterpret_cast<srt_udprecv_op *>(p + ops_at);
    c.n_hosts = n_hosts;
    c.n_sockets = n_sockets;
    c.ring_cap = ring_cap;
    c.note_cap = note_cap;
    c.win_bytes = WIN_BYTES;
    if (!plan) {
        if (n_sockets) std::memcpy(c.socks, ur->h_socks.data(), socks);
    } else {
        if (n_sockets && hipMemcpy(c.socks, ur->h_socks.data(), socks, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(ur->mem);
            delete ur;
            set_err(err, SRT_ERR_HIP, "udprecv: device initialisation failed");
            return SRT_ERR_HIP;
        }
        if (hipFuncSetAttribute((const void *)udprecv_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)WIN_BYTES) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(ur->mem);
            delete ur;
            set_err(err, SRT_ERR_HIP, "udprecv: the step kernel's LDS window was refused");
            return SRT_ERR_HIP;
        }
    }
    *out = ur;
    return SRT_OK;
}

extern "C" srt_status srt_udprecv_config(srt_udprecv *ur, const srt_udprecv_op *ops, uint64_t n, srt_err *err) {
    stage::begin(err);
    if (!ur || (n && !ops)) return stage::null_argument(err);
    if (n >= 0x80000000ull) {
        set_err(err, SRT_ERR_INVALID, "udprecv: more than 2^31-1 configuration steps in one call");
        return SRT_ERR_INVALID;
    }
    for (uint64_t i = 0; i < n; ++i)
        if (ops[i].slot >= ur->n_sockets || ops[i].op < SRT_UDPRECV_OPEN || ops[i].op > SRT_UDPRECV_SET_RCVBUF) {
            set_err(err, SRT_ERR_INVALID,
                    "udprecv: a configuration step's slot is not below n_sockets or its op is unknown (nothing was changed)");
            return SRT_ERR_INVALID;
        }
    if (!n) return SRT_OK;
    udprecv::Ctx c = ur->base;
    if (!ur->plan) {
        c.ops = ops;
        c.n_ops = (uint32_t)n;
        udprecv::host_config(c);
        return SRT_OK;
    }
    // steps on different slots commute: sorted stably by slot, a slot's steps are one run of the list.  The
    // sorted copy is the instance's: the stream is waited for first, so the previous call's copy has left it.
    if (!stage::use_device(ur->plan)) return SRT_ERR_HIP;
    hipStream_t s = ur->plan->stream;
    (void)hipStreamSynchronize(s);
    try {
        ur->h_order.resize(n);
        ur->h_sorted.resize(n);
    } catch (const std::bad_alloc &) {
        set_err(err, SRT_ERR_OOM, "udprecv: host allocation failed");
        return SRT_ERR_OOM;
    }
    std::iota(ur->h_order.begin(), ur->h_order.end(), 0u);
    std::stable_sort(ur->h_order.begin(), ur->h_order.end(),
                     [ops](uint32_t a, uint32_t b) { return ops[a].slot < ops[b].slot; });
    for (uint64_t i = 0; i < n; ++i) ur->h_sorted[i] = ops[ur->h_order[i]];
    c.ops = ur->d_ops;
    // a launch takes ops_cap steps; a slot's run cut by a launch's end goes on in the next, in stream order
    for (uint64_t at = 0; at < n; at += ur->ops_cap) {
        const uint64_t m = std::min<uint64_t>(ur->ops_cap, n - at);
        if (hipMemcpyAsync(ur->d_ops, ur->h_sorted.data() + at, 16 * m, hipMemcpyHostToDevice, s) != hipSuccess) {
            (void)hipGetLastError();
            set_err(err, SRT_ERR_HIP, "udprecv: copying the configuration steps failed");
            return SRT_ERR_HIP;
        }
        c.n_ops = (uint32_t)m;
        hipLaunchKernelGGL(udprecv_config_kernel, dim3(stage::strided_blocks(m, stage::LATE_BLOCKS)), dim3(BT), 0, s, c);
    }
    return stage::launched(err, "udprecv");
}

extern "C" srt_status srt_udprecv_note(srt_udprecv *ur, const srt_udp_meta *d_meta, uint64_t n_pkts, uint64_t tag_base,
                                       srt_err *err) {
    stage::begin(err);
    if (!ur || (n_pkts && !d_meta)) return stage::null_argument(err);
    if (n_pkts >= 0x80000000ull || tag_base < ur->note_end || tag_base + n_pkts < tag_base) {
        set_err(err, SRT_ERR_INVALID,
                "udprecv: more than 2^31-1 packets in one note, or tag_base below the previous note's end");
        return SRT_ERR_INVALID;
    }
    ur->note_end = tag_base + n_pkts;
    if (!n_pkts || !ur->note_cap) return SRT_OK;
    udprecv::Ctx c = ur->base;
    c.note_in = d_meta;
    c.note_n = (uint32_t)n_pkts;
    c.note_first = n_pkts > ur->note_cap ? (uint32_t)(n_pkts - ur->note_cap) : 0u;
    c.note_first_mod = (tag_base + c.note_first) % ur->note_cap;
    if (!ur->plan) {
        udprecv::host_note(c);
        return SRT_OK;
    }
    if (!stage::use_device(ur->plan)) return SRT_ERR_HIP;
    hipLaunchKernelGGL(udprecv_note_kernel, dim3(stage::strided_blocks(n_pkts - c.note_first, stage::NOTE_BLOCKS)),
                       dim3(BT), 0, ur->plan->stream, c);
    return stage::launched(err, "udprecv");
}

extern "C" srt_status srt_udprecv_run(srt_udprecv *ur, const uint32_t *d_out_host_ptr, const uint32_t *d_out_socket,
                                      const uint64_t *d_out_forward_ns, const uint64_t *d_out_tag,
                                      const uint32_t *d_out_status, uint64_t out_cap, const uint32_t *d_read_host_ptr,
                                      const srt_udp_read *d_reads, uint64_t n_reads, uint64_t *read_seq_base,
                                      uint64_t until_ns, uint32_t *d_rx_status, srt_udp_result *d_results,
                                      srt_udp_late *d_late, uint32_t late_cap, uint32_t *d_late_count,
                                      uint64_t *d_first_readable_ns, srt_err *err) {
    stage::begin(err);
    if (!ur || !d_out_host_ptr || (ur->n_sockets && !d_first_readable_ns) || (late_cap && !d_late) ||
        (out_cap && (!d_out_socket || !d_out_forward_ns || !d_out_tag || !d_out_status || !d_rx_status)) ||
        (n_reads && (!d_read_host_ptr || !d_reads || !d_results)))
        return stage::null_argument(err);
    if (n_reads >= 0x80000000ull || late_cap >= 0x80000000u) {
        set_err(err, SRT_ERR_INVALID, "udprecv: more than 2^31-1 reads or late records in one call");
        return SRT_ERR_INVALID;
    }
    if (until_ns < ur->prev_until) {
        set_err(err, SRT_ERR_INVALID, "udprecv: until_ns earlier than the previous call's");
        return SRT_ERR_INVALID;
    }
    const uint64_t cap = out_cap < 0xffffffffull ? out_cap : 0xffffffffull;  // positions are u32
    if (ur->plan && !stage::use_device(ur->plan)) return SRT_ERR_HIP;
    if (cap > ur->rec_cap) {  // the staged records grow with the largest out_cap seen
        if (ur->plan) {
            (void)hipStreamSynchronize(ur->plan->stream);
            (void)hipFree(ur->rec);
            ur->rec = nullptr;
            ur->rec_cap = 0;
            if (hipMalloc(&ur->rec, (size_t)cap * sizeof(udprecv::Rec)) != hipSuccess) {
                (void)hipGetLastError();
                set_err(err, SRT_ERR_OOM, "hipMalloc(udprecv records) failed");
                return SRT_ERR_OOM;
            }
        } else {
            try {
                ur->h_rec.resize(cap);
            } catch (const std::bad_alloc &) {
                set_err(err, SRT_ERR_OOM, "udprecv: host allocation failed");
                return SRT_ERR_OOM;
            }
            ur->rec = ur->h_rec.data();
        }
        ur->rec_cap = cap;
    }
    udprecv::Ctx c = ur->base;
    c.rec = ur->rec;
    c.note_end = ur->note_end;
    c.note_end_mod = ur->note_cap ? ur->note_end % ur->note_cap : 0;
    c.out_host_ptr = d_out_host_ptr;
    c.out_socket = d_out_socket;
    c.out_forward = d_out_forward_ns;
    c.out_tag = d_out_tag;
    c.out_status = d_out_status;
    c.out_cap = cap;
    c.read_host_ptr = n_reads ? d_read_host_ptr : nullptr;
    c.reads = d_reads;
    c.n_reads = (uint32_t)n_reads;
    c.read_seq_base = ur->read_base;
    c.prev_until = ur->prev_until;
    c.until = until_ns;
    c.rx_status = d_rx_status;
    c.results = d_results;
    c.late = d_late;
    c.late_cap = late_cap;
    c.late_count = d_late_count ? d_late_count : ur->own_late_count;
    c.first_readable = d_first_readable_ns;
    if (!ur->plan) {
        udprecv::host_run(c);
    } else {
        hipStream_t s = ur->plan->stream;
        const uint64_t items = std::max<uint64_t>(std::max<uint64_t>(cap, n_reads), 1);
        hipLaunchKernelGGL(udprecv_stage_kernel, dim3(stage::strided_blocks(items, stage::NOTE_BLOCKS)), dim3(BT), 0, s,
                           c);
        if (c.n_sockets)
            hipLaunchKernelGGL(udprecv_step_kernel, dim3((c.n_sockets + 63) / 64), dim3(64), WIN_BYTES, s, c);
        if (stage::launched(err, "udprecv") != SRT_OK) return SRT_ERR_HIP;
    }
    if (read_seq_base) *read_seq_base = ur->read_base;
    ur->read_base += n_reads;
    ur->prev_until = until_ns;
    return SRT_OK;
}

extern "C" srt_status srt_udprecv_status(srt_udprecv *ur, uint32_t *flags, uint64_t *n_processed, uint64_t *n_buffered,
                                         uint64_t *n_dropped, srt_err *err) {
    stage::begin(err);
    if (!ur) return stage::null_argument(err);
    udprecv::State w;
    if (!ur->plan) {
        const udprecv::Ctx &c = ur->base;
        c.st->n_proc = c.st->n_buf = c.st->n_drop = 0;
        for (uint32_t x = 0; x < c.n_sockets; ++x)
            c.st->n_proc += c.socks[x].n_proc, c.st->n_buf += c.socks[x].n_buf, c.st->n_drop += c.socks[x].n_drop;
        w = *c.st;
        c.st->flags = 0;
    } else {
        if (!stage::use_device(ur->plan)) return SRT_ERR_HIP;
        hipLaunchKernelGGL(udprecv_sum_kernel, dim3(1), dim3(ST), 0, ur->plan->stream, ur->base);
        const srt_status st = stage::read_status(ur->plan, &w, ur->base.st, sizeof w, err, "udprecv");
        if (st != SRT_OK) return st;
    }
    const uint32_t f = w.flags & 63u;
    if (flags) *flags = f;
    if (n_processed) *n_processed = w.n_proc;
    if (n_buffered) *n_buffered = w.n_buf;
    if (n_dropped) *n_dropped = w.n_drop;
    if (!f) return SRT_OK;
    if (err) {
        err->code = SRT_ERR_INVALID;
        std::snprintf(err->msg, sizeof err->msg, "udprecv:%s%s%s%s%s%s",
                      f & udprecv::F_RING_OVERFLOW ? " ring overflow (socket marked);" : "",
                      f & udprecv::F_LATE_OVERFLOW ? " more late records than late_cap;" : "",
                      f & udprecv::F_NOTE_OVERRUN ? " note overrun (record skipped, socket marked);" : "",
                      f & udprecv::F_BAD_SOCKET ? " bad socket in a read (-EBADF);" : "",
                      f & udprecv::F_READ_ORDER ? " read out of order or window (not taken);" : "",
                      f & udprecv::F_ARMED_TWICE ? " armed twice (-EWOULDBLOCK);" : "");
    }
    return SRT_ERR_INVALID;
}

extern "C" srt_status srt_udprecv_state(srt_udprecv *ur, srt_udprecv_socket_state *out, srt_err *err) {
    stage::begin(err);
    if (!ur || (ur->n_sockets && !out)) return stage::null_argument(err);
    const udprecv::Sock *socks = ur->base.socks;
    if (ur->plan) {
        if (!stage::use_device(ur->plan)) return SRT_ERR_HIP;
        hipStream_t s = ur->plan->stream;
        if ((ur->n_sockets && hipMemcpyAsync(ur->h_socks.data(), socks, sizeof(udprecv::Sock) * (size_t)ur->n_sockets,
                                             hipMemcpyDeviceToHost, s) != hipSuccess) ||
            hipStreamSynchronize(s) != hipSuccess) {
            (void)hipGetLastError();
            set_err(err, SRT_ERR_HIP, "udprecv: stream failed");
            return SRT_ERR_HIP;
        }
        socks = ur->h_socks.data();
    }
    for (uint32_t x = 0; x < ur->n_sockets; ++x) {
        const udprecv::Sock &s = socks[x];
        srt_udprecv_socket_state &o = out[x];
        o.len_bytes = s.len_bytes;
        o.soft_limit = s.soft_limit;
        o.last_read_recv_ns = s.last_read_recv_ns;
        o.armed_seq = s.armed_seq;
        o.n_msgs = s.n_msgs;
        o.peer_ip_be = s.peer_ip;
        o.peer_port_be = s.peer_port;
        o.open = s.open;
        o.overflow = s.overflow;
        o.reserved = 0;
    }
    return SRT_OK;
}
