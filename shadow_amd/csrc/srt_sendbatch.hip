// srt_sendbatch.hip -- the send-batch gather: from srt_outbound_run's results
// (send_ns and send_rank per batch packet, the late list) to what
// srt_packet_batch takes, srt_pkt records grouped by source host, each host's in
// send order.  The step -- rank to position, the log rule, the range checks --
// is srt_sendbatch_step.h, compiled here for the device and for the host-only
// instance alike.  No sort: a host's ranks of one outbound call are one
// contiguous run (see the header).
//
// Device form, four launches a call on the plan's stream (three without a late
// list):
//   (1) count: a group of L lanes owns one source host and walks its segment of
//       send_rank with coalesced loads; count and smallest rank are reduced
//       across the group's lanes and stored, every host's, so the arrays need no
//       reset.  L is 64 (a wave a host) when the batch averages more than 16
//       packets a host, else 8 (eight hosts a wave).  The meta of a packet
//       without a rank goes to the log here;
//   (2) late: one thread a late record (grid-stride), 64-bit atomics onto the
//       same two arrays;
//   (3) scan: one workgroup; each thread sums a contiguous chunk of the hosts'
//       counts, the sums are scanned across the workgroup, the chunk's bases
//       stored.  It also stores n_sent and raises OUT_OVERFLOW;
//   (4) scatter: the same groups as (1) over the batch, and, in further
//       workgroups, one thread a late record: the range checks, then the
//       24-byte record, user and seq.
// Scratch: 12 bytes a host (count, smallest rank), owned by the instance.
// Every value is written with ordinary stores from plain C++.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "srt_internal.h"
#include "srt_sendbatch_step.h"
#include "srt_stage.h"

namespace {

static_assert(sizeof(srt_send_meta) == 16 && sizeof(srt_pkt) == 24 && sizeof(srt_outbound_late) == 32,
              "record layouts");

using stage::BT;
using stage::ST;
using stage::set_err;

template <uint32_t L>
__global__ __launch_bounds__(BT) void sendbatch_count_kernel(const sendb::Ctx c) {
    const stage::Group<L> G(c.n_hosts);
    uint32_t n = 0;
    uint64_t mn = sendb::NONE;
    if (G.own()) {
        uint32_t b, e;
        sendb::segment(c, (uint32_t)G.g, b, e);
        for (uint32_t i = b + G.l; i < e; i += L) {
            const uint64_t rank = c.send_rank[i];
            if (rank == sendb::NONE) {
                sendb::log_keep(c, i);
            } else {
                ++n;
                mn = rank < mn ? rank : mn;
            }
        }
    }
    // every lane is here: the group's lanes hold its partial counts and minima (one fused walk of the lanes:
    // two separate reductions schedule differently)
    for (uint32_t off = L / 2; off > 0; off >>= 1) {
        n += __shfl_xor(n, off);
        const unsigned long long o = __shfl_xor((unsigned long long)mn, off);
        mn = o < mn ? o : mn;
    }
    if (G.own() && G.l == 0) {
        c.cnt[G.g] = n;
        c.first[G.g] = mn;
    }
}

__global__ __launch_bounds__(BT) void sendbatch_late_kernel(const sendb::Ctx c) {
    for (uint64_t k : stage::grid_stride(sendb::late_n(c))) sendb::count_late(c, (uint32_t)k);
}

__global__ __launch_bounds__(ST) void sendbatch_scan_kernel(const sendb::Ctx c) {
    stage::scan_hosts<ST>(
        c.n_hosts, [&](uint32_t h) { return c.cnt[h]; },
        [&](uint32_t h, uint64_t run) {
            const uint32_t n = c.cnt[h];
            c.out_host_ptr[h] = sendb::host_base(c, run);
            return n;
        },
        [&](uint64_t total) { sendb::scan_end(c, total); });
}

template <uint32_t L>
__global__ __launch_bounds__(BT) void sendbatch_scatter_kernel(const sendb::Ctx c, uint32_t host_blocks) {
    if (blockIdx.x < host_blocks) {
        const stage::Group<L> G(c.n_hosts);
        if (!G.own()) return;
        const uint32_t h = (uint32_t)G.g;
        uint32_t b, e;
        sendb::segment(c, h, b, e);
        if (b + G.l >= e) return;
        const sendb::HostRun hr = sendb::host_run(c, h);
        for (uint32_t i = b + G.l; i < e; i += L) sendb::scatter_batch(c, hr, h, i);
    } else {
        for (uint64_t k : stage::grid_stride(sendb::late_n(c), host_blocks)) sendb::scatter_late(c, (uint32_t)k);
    }
}

}  // namespace

struct srt_sendbatch {
    srt_plan *plan = nullptr;  // nullptr: host-only
    uint32_t n = 0;
    uint64_t log_cap = 0;
    // device form: device memory; host-only form: the vectors below
    srt_send_meta *log = nullptr;
    uint32_t *cnt = nullptr;
    uint64_t *first = nullptr;
    uint32_t *flags = nullptr;  // [0] SRT_SENDBATCH_* bits, [2..3] u64 n_sent of the last call
    std::vector<srt_send_meta> h_log;
    std::vector<uint32_t> h_cnt;
    std::vector<uint64_t> h_first;
    alignas(8) uint32_t h_flags[4] = {0, 0, 0, 0};
};

namespace srt {
// srt_init: loads this unit's code object (srt::preload_kernels)
hipError_t preload_sendbatch() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&sendbatch_scan_kernel));
}
}  // namespace srt

extern "C" void srt_sendbatch_destroy(srt_sendbatch *sb) {
    if (!sb) return;
    if (sb->plan) {
        (void)stage::use_device(sb->plan);
        (void)hipStreamSynchronize(sb->plan->stream);
        (void)hipFree(sb->log);
        (void)hipFree(sb->cnt);
        (void)hipFree(sb->first);
        (void)hipFree(sb->flags);
    }
    delete sb;
}

extern "C" srt_status srt_sendbatch_create(srt_plan *plan, uint32_t n_hosts, uint64_t log_cap, srt_sendbatch **out,
                                           srt_err *err) {
    stage::begin(err);
    if (!out) return stage::null_argument(err);
    *out = nullptr;
    if (n_hosts == 0xffffffffu || log_cap > (1ull << 40)) {
        set_err(err, SRT_ERR_INVALID, "sendbatch: n_hosts or log_cap out of range");
        return SRT_ERR_INVALID;
    }
    srt_sendbatch *sb = new (std::nothrow) srt_sendbatch;
    if (!sb) return SRT_ERR_OOM;
    sb->plan = plan;
    sb->n = n_hosts;
    sb->log_cap = log_cap;
    const size_t n_log = (size_t)log_cap + 1, n_host = (size_t)n_hosts + 1;
    if (!plan) {
        try {
            sb->h_log.assign(n_log, srt_send_meta{0, 0, 0, 0});
            sb->h_cnt.assign(n_host, 0);
            sb->h_first.assign(n_host, sendb::NONE);
        } catch (const std::bad_alloc &) {
            delete sb;
            set_err(err, SRT_ERR_OOM, "sendbatch: host allocation failed");
            return SRT_ERR_OOM;
        }
        sb->log = sb->h_log.data();
        sb->cnt = sb->h_cnt.data();
        sb->first = sb->h_first.data();
        sb->flags = sb->h_flags;
        *out = sb;
        return SRT_OK;
    }
    srt::init_wait();
    bool ok = stage::use_device(plan);
    ok = ok && hipMalloc(&sb->log, n_log * sizeof(srt_send_meta)) == hipSuccess &&
         hipMalloc(&sb->cnt, n_host * 4) == hipSuccess && hipMalloc(&sb->first, n_host * 8) == hipSuccess &&
         hipMalloc(&sb->flags, 16) == hipSuccess;
    ok = ok && hipMemset(sb->log, 0, n_log * sizeof(srt_send_meta)) == hipSuccess &&
         hipMemset(sb->cnt, 0, n_host * 4) == hipSuccess && hipMemset(sb->first, 0xff, n_host * 8) == hipSuccess &&
         hipMemset(sb->flags, 0, 16) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        (void)hipFree(sb->log);
        (void)hipFree(sb->cnt);
        (void)hipFree(sb->first);
        (void)hipFree(sb->flags);
        delete sb;
        set_err(err, SRT_ERR_OOM, "sendbatch: device allocation failed");
        return SRT_ERR_OOM;
    }
    *out = sb;
    return SRT_OK;
}

extern "C" srt_status srt_sendbatch_run(srt_sendbatch *sb, const uint32_t *d_host_ptr, uint64_t n_pkts,
                                        const srt_send_meta *d_meta, const uint64_t *d_send_ns,
                                        const uint64_t *d_send_rank, uint64_t seq_base,
                                        const srt_outbound_late *d_late, uint32_t late_cap,
                                        const uint32_t *d_late_count, srt_pkt *d_out_pkts, uint32_t *d_out_host_ptr,
                                        uint32_t *d_out_user, uint64_t *d_out_seq, uint64_t out_cap, srt_err *err) {
    stage::begin(err);
    if (!sb || !d_host_ptr || !d_out_host_ptr || (n_pkts && (!d_meta || !d_send_ns || !d_send_rank)) ||
        (late_cap && (!d_late || !d_late_count)) || (out_cap && (!d_out_pkts || !d_out_user || !d_out_seq)))
        return stage::null_argument(err);
    if (n_pkts >= 0x80000000ull || late_cap >= 0x80000000u) {
        set_err(err, SRT_ERR_INVALID, "more than 2^31-1 packets in one batch or late list");
        return SRT_ERR_INVALID;
    }
    sendb::Ctx c;
    c.host_ptr = d_host_ptr;
    c.meta = d_meta;
    c.send_ns = d_send_ns;
    c.send_rank = d_send_rank;
    c.late = d_late;
    c.late_count = late_cap ? d_late_count : nullptr;
    c.log = sb->log;
    c.cnt = sb->cnt;
    c.first = sb->first;
    c.out_pkts = d_out_pkts;
    c.out_host_ptr = d_out_host_ptr;
    c.out_user = d_out_user;
    c.out_seq = d_out_seq;
    c.flags = sb->flags;
    c.seq_base = seq_base;
    c.log_cap = sb->log_cap;
    c.out_cap = out_cap < 0xffffffffull ? out_cap : 0xffffffffull;  // positions are u32
    c.end_mod = sb->log_cap ? (seq_base + n_pkts) % sb->log_cap : 0;
    c.n_hosts = sb->n;
    c.n_pkts = (uint32_t)n_pkts;
    c.late_cap = late_cap;
    c.pad = 0;
    if (!sb->plan) {
        for (uint32_t h = 0; h < c.n_hosts; ++h) {
            uint32_t b, e, n = 0;
            uint64_t mn = sendb::NONE;
            sendb::segment(c, h, b, e);
            for (uint32_t i = b; i < e; ++i) {
                const uint64_t rank = c.send_rank[i];
                if (rank == sendb::NONE) {
                    sendb::log_keep(c, i);
                } else {
                    ++n;
                    mn = rank < mn ? rank : mn;
                }
            }
            c.cnt[h] = n;
            c.first[h] = mn;
        }
        const uint32_t n_late = sendb::late_n(c);
        for (uint32_t k = 0; k < n_late; ++k) sendb::count_late(c, k);
        uint64_t run = 0;
        for (uint32_t h = 0; h < c.n_hosts; ++h) {
            c.out_host_ptr[h] = sendb::host_base(c, run);
            run += c.cnt[h];
        }
        sendb::scan_end(c, run);
        for (uint32_t h = 0; h < c.n_hosts; ++h) {
            uint32_t b, e;
            sendb::segment(c, h, b, e);
            const sendb::HostRun hr = sendb::host_run(c, h);
            for (uint32_t i = b; i < e; ++i) sendb::scatter_batch(c, hr, h, i);
        }
        for (uint32_t k = 0; k < n_late; ++k) sendb::scatter_late(c, k);
        return SRT_OK;
    }
    if (!stage::use_device(sb->plan)) return SRT_ERR_HIP;
    hipStream_t s = sb->plan->stream;
    const bool wide = stage::wide(n_pkts, c.n_hosts);
    const uint32_t host_blocks = stage::host_blocks(c.n_hosts, wide);
    const uint32_t late_blocks = stage::strided_blocks(late_cap, stage::LATE_BLOCKS);
    if (host_blocks)
        stage::launch_grouped(sendbatch_count_kernel<64>, sendbatch_count_kernel<8>, wide, host_blocks, BT, s, c);
    if (late_blocks) hipLaunchKernelGGL(sendbatch_late_kernel, dim3(late_blocks), dim3(BT), 0, s, c);
    hipLaunchKernelGGL(sendbatch_scan_kernel, dim3(1), dim3(ST), 0, s, c);
    if (host_blocks + late_blocks)
        stage::launch_grouped(sendbatch_scatter_kernel<64>, sendbatch_scatter_kernel<8>, wide,
                              host_blocks + late_blocks, BT, s, c, host_blocks);
    return stage::launched(err, "sendbatch");
}

extern "C" srt_status srt_sendbatch_status(srt_sendbatch *sb, uint32_t *flags, uint64_t *n_sent, srt_err *err) {
    stage::begin(err);
    if (!sb) return stage::null_argument(err);
    uint32_t w[4] = {0, 0, 0, 0};
    if (!sb->plan) {
        std::memcpy(w, sb->h_flags, sizeof w);
        sb->h_flags[0] = 0;
    } else {
        if (!stage::use_device(sb->plan)) return SRT_ERR_HIP;
        const srt_status st = stage::read_status(sb->plan, w, sb->flags, sizeof w, err, "sendbatch");
        if (st != SRT_OK) return st;
    }
    const uint32_t f = w[0] & 15u;
    if (flags) *flags = f;
    if (n_sent) std::memcpy(n_sent, w + 2, 8);
    if (!f) return SRT_OK;
    if (err) {
        err->code = SRT_ERR_INVALID;
        std::snprintf(err->msg, sizeof err->msg, "sendbatch:%s%s%s%s",
                      f & sendb::F_OUT_OVERFLOW ? " more sent packets than out_cap (nothing past it written);" : "",
                      f & sendb::F_RANK_GAP ? " a host's ranks are not one contiguous run;" : "",
                      f & sendb::F_LOG_OVERRUN ? " a late packet's seq is older than the log holds;" : "",
                      f & sendb::F_BAD_HOST ? " a late record's src_host is not below n_hosts (skipped);" : "");
    }
    return SRT_ERR_INVALID;
}
