// srt_tracker.hip -- the tracker's heartbeat byte counters of the internet
// interface (host/tracker.c:188-284, 582-627): per host and per socket slot, in
// and out, what tracker_addOutputBytes adds in networkinterface_pop and
// tracker_addInputBytes in networkinterface_push, kept on the device between
// heartbeats.  The step -- the classes, the pop-time rule of the output side,
// the note ring and seq log rules, the range checks -- is srt_tracker_step.h,
// compiled here for the device and for the host-only instance alike.
//
// Device form, on the plan's stream; only heartbeat and status wait for it.
//   note: one launch, a copy of the round's metas into the ring.
//   tx, two launches (one without a late list):
//     (1) late: one thread a late record (grid-stride): the remembered seq of
//         its host, the log, 64-bit atomics on the host's record and the slot's;
//     (2) hosts: a group of L lanes owns one source host and walks its segment
//         of d_status / d_meta with coalesced loads; every lane keeps the ten
//         sums of its packets in registers, a popped packet adds to its socket
//         slot with two or three 64-bit atomics, a packet that stays queued has
//         its meta written to the seq log.  The group's first lane takes the
//         host's cached packet (rules 3 and 4), the sums are reduced across
//         the group's lanes and that lane adds them to the host's record with
//         ordinary loads and stores: no other lane of the launch has that
//         record.  L is 64 (a wave a host) when the batch averages more than
//         16 packets a host, else 8 (eight hosts a wave).
//   rx: one launch of the same geometry over srt_deliver_run's list, bounded by
//       min(d_out_host_ptr[n_hosts], out_cap) on the device; L from out_cap.
//   rx_flat: one thread a record, atomics on the host's record and the slot's.
// The launches of one stream run in order, so a record's atomic adds (late,
// flat) and its plain read-modify-write (the hosts' walk) never overlap.  No
// kernel adds to a call-wide counter: the packets counted are kept a host and
// srt_tracker_status, which synchronises anyway, sums them with one launch.
// Every value is written with ordinary stores or vector atomics from plain C++.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "srt_internal.h"
#include "srt_tracker_step.h"
#include "srt_stage.h"

namespace {

static_assert(sizeof(srt_trk_counters) == 80 && sizeof(srt_trk_meta) == 16 && sizeof(tracker::State) == 24 &&
                  sizeof(srt_outbound_late) == 32,
              "record layouts");

using stage::BT;
using stage::ST;
using stage::set_err;

__global__ __launch_bounds__(BT) void tracker_note_kernel(const tracker::Ctx c) {
    for (uint64_t i = (uint64_t)c.note_first + (uint64_t)blockIdx.x * BT + threadIdx.x; i < c.note_n;
         i += (uint64_t)gridDim.x * BT)
        tracker::note_store(c, (uint32_t)i);
}

__global__ __launch_bounds__(BT) void tracker_late_kernel(const tracker::Ctx c) {
    for (uint64_t k : stage::grid_stride(tracker::late_n(c))) tracker::tx_late(c, (uint32_t)k);
}

template <uint32_t L>
__global__ __launch_bounds__(BT) void tracker_tx_kernel(const tracker::Ctx c) {
    const stage::Group<L> G(c.n_hosts);
    tracker::Acc a;
    tracker::acc_zero(a);
    if (G.own()) {
        uint32_t b, e;
        tracker::segment(c.host_ptr, tracker::tx_walked(c), (uint32_t)G.g, b, e);
        for (uint32_t i = b + G.l; i < e; i += L) tracker::tx_batch(c, i, a);
        if (G.l == 0) tracker::tx_cached(c, (uint32_t)G.g, a);
    }
    stage::group_sum<L>(a.v);  // every lane is here
    if (G.own() && G.l == 0) tracker::host_merge(c.node_out + G.g, c.cnt_tx + G.g, a);
}

template <uint32_t L>
__global__ __launch_bounds__(BT) void tracker_rx_kernel(const tracker::Ctx c) {
    const stage::Group<L> G(c.n_hosts);
    tracker::Acc a;
    tracker::acc_zero(a);
    if (G.own()) {
        uint32_t b, e;
        tracker::segment(c.out_host_ptr, tracker::rx_walked(c), (uint32_t)G.g, b, e);
        for (uint32_t p = b + G.l; p < e; p += L) tracker::rx_record(c, p, a);
    }
    stage::group_sum<L>(a.v);
    if (G.own() && G.l == 0) tracker::host_merge(c.node_in + G.g, c.cnt_rx + G.g, a);
}

__global__ __launch_bounds__(BT) void tracker_flat_kernel(const tracker::Ctx c) {
    for (uint64_t k : stage::grid_stride(c.f_n)) tracker::rx_flat(c, (uint32_t)k);
}

// srt_tracker_status: the hosts' counts of packets, summed by one workgroup
__global__ __launch_bounds__(ST) void tracker_sum_kernel(const tracker::Ctx c) {
    __shared__ uint64_t wsum[2][ST / 64];
    const uint32_t t = threadIdx.x;
    unsigned long long tx = 0, rx = 0;
    for (uint32_t h = t; h < c.n_hosts; h += ST) tx += c.cnt_tx[h], rx += c.cnt_rx[h];
    for (uint32_t off = 32; off > 0; off >>= 1) tx += __shfl_xor(tx, off), rx += __shfl_xor(rx, off);
    if ((t & 63) == 0) wsum[0][t >> 6] = tx, wsum[1][t >> 6] = rx;
    __syncthreads();
    if (t == 0) {
        uint64_t a = 0, b = 0;
        for (uint32_t w = 0; w < ST / 64; ++w) a += wsum[0][w], b += wsum[1][w];
        c.st->n_tx = a;
        c.st->n_rx = b;
    }
}

}  // namespace

struct srt_tracker {
    srt_plan *plan = nullptr;  // nullptr: host-only
    uint32_t n_hosts = 0, n_sockets = 0;
    uint64_t note_cap = 0, log_cap = 0;
    uint64_t note_end = 0;
    void *mem = nullptr;  // device form: everything in one allocation; host-only: h_mem
    size_t rec_bytes = 0;  // the four record arrays, contiguous from node_in
    std::vector<uint64_t> h_mem;
    std::vector<srt_trk_counters> stage;  // device form: the records on the host, for the heartbeat
    tracker::Ctx base;
};

namespace srt {
// srt_init: loads this unit's code object (srt::preload_kernels)
hipError_t preload_tracker() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&tracker_sum_kernel));
}
}  // namespace srt

extern "C" void srt_tracker_destroy(srt_tracker *trk) {
    if (!trk) return;
    if (trk->plan) {
        (void)stage::use_device(trk->plan);
        (void)hipStreamSynchronize(trk->plan->stream);
        (void)hipFree(trk->mem);
    }
    delete trk;
}

extern "C" srt_status srt_tracker_create(srt_plan *plan, uint32_t n_hosts, uint32_t n_sockets, uint64_t note_cap,
                                         uint64_t log_cap, srt_tracker **out, srt_err *err) {
    stage::begin(err);
    if (!out) return stage::null_argument(err);
    *out = nullptr;
    if (n_hosts >= 0x80000000u || n_sockets >= 0x80000000u || note_cap > (1ull << 31) || log_cap > (1ull << 31)) {
        set_err(err, SRT_ERR_INVALID,
                "tracker: n_hosts, n_sockets (below 2^31), note_cap or log_cap (at most 2^31) out of range");
        return SRT_ERR_INVALID;
    }
    srt_tracker *trk = new (std::nothrow) srt_tracker;
    if (!trk) return SRT_ERR_OOM;
    trk->plan = plan;
    trk->n_hosts = n_hosts;
    trk->n_sockets = n_sockets;
    trk->note_cap = note_cap;
    trk->log_cap = log_cap;
    // state; the hosts' and the slots' records; the ring; the log; the hosts' counts and remembered seqs
    const size_t head = 32, recs = 2 * ((size_t)n_hosts + n_sockets);
    trk->rec_bytes = recs * sizeof(srt_trk_counters);
    const size_t words = 24 * (size_t)n_hosts, bytes = head + trk->rec_bytes + words + 16 * (size_t)(note_cap + log_cap);
    bool ok = true;
    if (!plan) {
        try {
            trk->h_mem.assign(bytes / 8 + 1, 0);
        } catch (const std::bad_alloc &) {
            ok = false;
        }
        trk->mem = trk->h_mem.data();
    } else {
        try {
            trk->stage.resize(recs + 1);
        } catch (const std::bad_alloc &) {
            ok = false;
        }
        if (ok) {
            srt::init_wait();
            ok = stage::use_device(plan);
            ok = ok && hipMalloc(&trk->mem, bytes + 8) == hipSuccess;
            ok = ok && hipMemset(trk->mem, 0, bytes + 8) == hipSuccess;
            if (!ok) {
                (void)hipGetLastError();
                (void)hipFree(trk->mem);
            }
        }
    }
    if (!ok) {
        delete trk;
        set_err(err, SRT_ERR_OOM, "tracker: allocation failed");
        return SRT_ERR_OOM;
    }
    tracker::Ctx &c = trk->base;
    std::memset(&c, 0, sizeof c);
    char *p = static_cast<char *>(trk->mem);
    c.st = reinterpret_cast<tracker::State *>(p);
    c.node_in = reinterpret_cast<srt_trk_counters *>(p + head);
    c.node_out = c.node_in + n_hosts;
    c.sock_in = c.node_out + n_hosts;
    c.sock_out = c.sock_in + n_sockets;
    c.ring = reinterpret_cast<srt_trk_meta *>(p + head + trk->rec_bytes);  // 16-byte aligned
    c.log = c.ring + note_cap;
    c.cnt_tx = reinterpret_cast<uint64_t *>(c.log + log_cap);
    c.cnt_rx = c.cnt_tx + n_hosts;
    c.remembered = c.cnt_rx + n_hosts;
    c.n_hosts = n_hosts;
    c.n_sockets = n_sockets;
    c.note_cap = note_cap;
    c.log_cap = log_cap;
    // no host holds a cached packet yet
    if (!plan) {
        for (uint32_t h = 0; h < n_hosts; ++h) c.remembered[h] = tracker::NONE;
    } else if (n_hosts && hipMemset(c.remembered, 0xff, 8 * (size_t)n_hosts) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(trk->mem);
        delete trk;
        set_err(err, SRT_ERR_HIP, "tracker: device initialisation failed");
        return SRT_ERR_HIP;
    }
    *out = trk;
    return SRT_OK;
}

extern "C" srt_status srt_tracker_tx(srt_tracker *trk, const uint64_t *d_cached_seq, const uint32_t *d_host_ptr,
                                     uint64_t n_pkts, const srt_trk_meta *d_meta, const uint32_t *d_status,
                                     uint64_t seq_base, const srt_outbound_late *d_late, uint32_t late_cap,
                                     const uint32_t *d_late_count, srt_err *err) {
    stage::begin(err);
    if (!trk || !d_host_ptr || (trk->n_hosts && !d_cached_seq) || (n_pkts && (!d_meta || !d_status)) ||
        (late_cap && (!d_late || !d_late_count)))
        return stage::null_argument(err);
    if (n_pkts >= 0x80000000ull || late_cap >= 0x80000000u || seq_base + n_pkts < seq_base) {
        set_err(err, SRT_ERR_INVALID, "more than 2^31-1 packets in one batch or late list");
        return SRT_ERR_INVALID;
    }
    tracker::Ctx c = trk->base;
    c.base_mod = trk->log_cap ? seq_base % trk->log_cap : 0;
    c.end_mod = trk->log_cap ? (seq_base + n_pkts) % trk->log_cap : 0;
    c.cached_seq = d_cached_seq;
    c.host_ptr = d_host_ptr;
    c.status = d_status;
    c.meta = d_meta;
    c.late = d_late;
    c.late_count = late_cap ? d_late_count : nullptr;
    c.late_cap = late_cap;
    c.seq_base = seq_base;
    c.n_pkts = (uint32_t)n_pkts;
    if (!trk->plan) {
        tracker::host_tx(c);
        return SRT_OK;
    }
    if (!stage::use_device(trk->plan)) return SRT_ERR_HIP;
    hipStream_t s = trk->plan->stream;
    if (late_cap)
        hipLaunchKernelGGL(tracker_late_kernel, dim3(stage::strided_blocks(late_cap, stage::LATE_BLOCKS)), dim3(BT), 0,
                           s, c);
    if (c.n_hosts) {
        const bool wide = stage::wide(n_pkts, c.n_hosts);
        stage::launch_grouped(tracker_tx_kernel<64>, tracker_tx_kernel<8>, wide, stage::host_blocks(c.n_hosts, wide),
                              BT, s, c);
    }
    return stage::launched(err, "tracker");
}

extern "C" srt_status srt_tracker_note(srt_tracker *trk, const srt_trk_meta *d_meta, uint64_t n_pkts,
                                       uint64_t tag_base, srt_err *err) {
    stage::begin(err);
    if (!trk || (n_pkts && !d_meta)) return stage::null_argument(err);
    if (n_pkts >= 0x80000000ull || tag_base < trk->note_end || tag_base + n_pkts < tag_base) {
        set_err(err, SRT_ERR_INVALID, "tracker: more than 2^31-1 packets in one note, or tag_base below the previous note's end");
        return SRT_ERR_INVALID;
    }
    trk->note_end = tag_base + n_pkts;
    if (!n_pkts || !trk->note_cap) return SRT_OK;
    tracker::Ctx c = trk->base;
    c.note_in = d_meta;
    c.note_n = (uint32_t)n_pkts;
    c.note_first = n_pkts > trk->note_cap ? (uint32_t)(n_pkts - trk->note_cap) : 0u;
    c.note_first_mod = (tag_base + c.note_first) % trk->note_cap;
    if (!trk->plan) {
        tracker::host_note(c);
        return SRT_OK;
    }
    if (!stage::use_device(trk->plan)) return SRT_ERR_HIP;
    hipLaunchKernelGGL(tracker_note_kernel, dim3(stage::strided_blocks(n_pkts - c.note_first, stage::NOTE_BLOCKS)),
                       dim3(BT), 0, trk->plan->stream, c);
    return stage::launched(err, "tracker");
}

extern "C" srt_status srt_tracker_rx(srt_tracker *trk, const uint32_t *d_out_host_ptr, const uint32_t *d_out_socket,
                                     const uint64_t *d_out_tag, const uint32_t *d_out_status, uint64_t out_cap,
                                     srt_err *err) {
    stage::begin(err);
    if (!trk || !d_out_host_ptr || (out_cap && (!d_out_socket || !d_out_tag || !d_out_status)))
        return stage::null_argument(err);
    tracker::Ctx c = trk->base;
    c.note_end = trk->note_end;
    c.note_end_mod = trk->note_cap ? trk->note_end % trk->note_cap : 0;
    c.out_host_ptr = d_out_host_ptr;
    c.out_socket = d_out_socket;
    c.out_tag = d_out_tag;
    c.out_status = d_out_status;
    c.out_cap = out_cap < 0xffffffffull ? out_cap : 0xffffffffull;  // positions are u32
    if (!trk->plan) {
        tracker::host_rx(c);
        return SRT_OK;
    }
    if (!c.n_hosts) return SRT_OK;
    if (!stage::use_device(trk->plan)) return SRT_ERR_HIP;
    hipStream_t s = trk->plan->stream;
    const bool wide = stage::wide(out_cap, c.n_hosts);
    stage::launch_grouped(tracker_rx_kernel<64>, tracker_rx_kernel<8>, wide, stage::host_blocks(c.n_hosts, wide), BT, s,
                          c);
    return stage::launched(err, "tracker");
}

extern "C" srt_status srt_tracker_rx_flat(srt_tracker *trk, const uint32_t *d_host, const uint32_t *d_socket,
                                          const srt_trk_meta *d_meta, uint64_t n, srt_err *err) {
    stage::begin(err);
    if (!trk || (n && (!d_host || !d_socket || !d_meta))) return stage::null_argument(err);
    if (n >= 0x80000000ull) {
        set_err(err, SRT_ERR_INVALID, "more than 2^31-1 records in one call");
        return SRT_ERR_INVALID;
    }
    if (!n) return SRT_OK;
    tracker::Ctx c = trk->base;
    c.f_host = d_host;
    c.f_socket = d_socket;
    c.f_meta = d_meta;
    c.f_n = (uint32_t)n;
    if (!trk->plan) {
        tracker::host_rx_flat(c);
        return SRT_OK;
    }
    if (!stage::use_device(trk->plan)) return SRT_ERR_HIP;
    hipLaunchKernelGGL(tracker_flat_kernel, dim3(stage::strided_blocks(n, stage::LATE_BLOCKS)), dim3(BT), 0,
                       trk->plan->stream, c);
    return stage::launched(err, "tracker");
}

namespace srt {
// tracker_heartbeat over the four contiguous record arrays at `recs` (hosts in, hosts out, slots in,
// slots out; device memory with a plan, whose `stage` then takes the copy on the host)
srt_status counters_heartbeat(srt_plan *plan, const char *who, srt_trk_counters *recs, size_t rec_bytes,
                              srt_trk_counters *stage, uint32_t n_hosts, uint32_t n_sockets, const uint32_t *hosts,
                              uint32_t n_sel_hosts, const uint32_t *sockets, uint32_t n_sel_sockets,
                              srt_trk_counters *out_node_in, srt_trk_counters *out_node_out,
                              srt_trk_counters *out_sock_in, srt_trk_counters *out_sock_out, srt_err *err) {
    char msg[160];
    const uint32_t nh = hosts ? n_sel_hosts : n_hosts, ns = sockets ? n_sel_sockets : n_sockets;
    for (uint32_t k = 0; hosts && k < nh; ++k)
        if (hosts[k] >= n_hosts) {
            std::snprintf(msg, sizeof msg, "%s: a selected host is not below n_hosts (nothing was cleared)", who);
            set_err(err, SRT_ERR_INVALID, msg);
            return SRT_ERR_INVALID;
        }
    for (uint32_t k = 0; sockets && k < ns; ++k)
        if (sockets[k] >= n_sockets) {
            std::snprintf(msg, sizeof msg, "%s: a selected socket slot is not below n_sockets (nothing was cleared)", who);
            set_err(err, SRT_ERR_INVALID, msg);
            return SRT_ERR_INVALID;
        }
    // the four record arrays as the host sees them: the instance's own memory, or the staged copy
    srt_trk_counters *dev = recs;
    const bool all = !hosts && !sockets;
    if (plan) {
        if (!stage::use_device(plan)) return SRT_ERR_HIP;
        hipStream_t s = plan->stream;
        recs = stage;
        if ((rec_bytes && hipMemcpyAsync(recs, dev, rec_bytes, hipMemcpyDeviceToHost, s) != hipSuccess) ||
            hipStreamSynchronize(s) != hipSuccess) {
            (void)hipGetLastError();
            std::snprintf(msg, sizeof msg, "%s: stream failed", who);
            set_err(err, SRT_ERR_HIP, msg);
            return SRT_ERR_HIP;
        }
    }
    srt_trk_counters *node_in = recs, *node_out = node_in + n_hosts, *sock_in = node_out + n_hosts,
                     *sock_out = sock_in + n_sockets;
    for (uint32_t k = 0; k < nh; ++k) {
        const uint32_t h = hosts ? hosts[k] : k;
        if (out_node_in) out_node_in[k] = node_in[h];
        if (out_node_out) out_node_out[k] = node_out[h];
    }
    for (uint32_t k = 0; k < ns; ++k) {
        const uint32_t x = sockets ? sockets[k] : k;
        if (out_sock_in) out_sock_in[k] = sock_in[x];
        if (out_sock_out) out_sock_out[k] = sock_out[x];
    }
    // tracker.c:607-619: the selected records start the next interval at zero
    const srt_trk_counters zero = {};
    for (uint32_t k = 0; k < nh; ++k) node_in[hosts ? hosts[k] : k] = node_out[hosts ? hosts[k] : k] = zero;
    for (uint32_t k = 0; k < ns; ++k) sock_in[sockets ? sockets[k] : k] = sock_out[sockets ? sockets[k] : k] = zero;
    if (plan && rec_bytes && (nh || ns)) {
        // the stream is idle: the cleared copy goes back whole (everything selected: a memset)
        hipStream_t s = plan->stream;
        const hipError_t e = all ? hipMemsetAsync(dev, 0, rec_bytes, s)
                                 : hipMemcpyAsync(dev, recs, rec_bytes, hipMemcpyHostToDevice, s);
        if (e != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
            (void)hipGetLastError();
            std::snprintf(msg, sizeof msg, "%s: clearing the records failed", who);
            set_err(err, SRT_ERR_HIP, msg);
            return SRT_ERR_HIP;
        }
    }
    return SRT_OK;
}
}  // namespace srt

extern "C" srt_status srt_tracker_heartbeat(srt_tracker *trk, const uint32_t *hosts, uint32_t n_sel_hosts,
                                            const uint32_t *sockets, uint32_t n_sel_sockets,
                                            srt_trk_counters *out_node_in, srt_trk_counters *out_node_out,
                                            srt_trk_counters *out_sock_in, srt_trk_counters *out_sock_out,
                                            srt_err *err) {
    stage::begin(err);
    if (!trk) return stage::null_argument(err);
    return srt::counters_heartbeat(trk->plan, "tracker", trk->base.node_in, trk->rec_bytes, trk->stage.data(),
                                   trk->n_hosts, trk->n_sockets, hosts, n_sel_hosts, sockets, n_sel_sockets,
                                   out_node_in, out_node_out, out_sock_in, out_sock_out, err);
}

extern "C" srt_status srt_tracker_status(srt_tracker *trk, uint32_t *flags, uint64_t *n_tx_counted,
                                         uint64_t *n_rx_counted, srt_err *err) {
    stage::begin(err);
    if (!trk) return stage::null_argument(err);
    tracker::State w;
    if (!trk->plan) {
        const tracker::Ctx &c = trk->base;
        c.st->n_tx = c.st->n_rx = 0;
        for (uint32_t h = 0; h < c.n_hosts; ++h) c.st->n_tx += c.cnt_tx[h], c.st->n_rx += c.cnt_rx[h];
        w = *c.st;
        c.st->flags = 0;
    } else {
        if (!stage::use_device(trk->plan)) return SRT_ERR_HIP;
        hipLaunchKernelGGL(tracker_sum_kernel, dim3(1), dim3(ST), 0, trk->plan->stream, trk->base);
        const srt_status st = stage::read_status(trk->plan, &w, trk->base.st, sizeof w, err, "tracker");
        if (st != SRT_OK) return st;
    }
    const uint32_t f = w.flags & 15u;
    if (flags) *flags = f;
    if (n_tx_counted) *n_tx_counted = w.n_tx;
    if (n_rx_counted) *n_rx_counted = w.n_rx;
    if (!f) return SRT_OK;
    if (err) {
        err->code = SRT_ERR_INVALID;
        std::snprintf(err->msg, sizeof err->msg, "tracker:%s%s%s%s",
                      f & tracker::F_LOG_OVERRUN ? " a late or cached packet's seq is older than the log holds (not counted);" : "",
                      f & tracker::F_NOTE_OVERRUN ? " a placeholder record or a tag the note ring does not hold (skipped);" : "",
                      f & tracker::F_BAD_SOCKET ? " a socket slot is not below n_sockets (counted at its host only);" : "",
                      f & tracker::F_BAD_HOST ? " a record's host is not below n_hosts (skipped);" : "");
    }
    return SRT_ERR_INVALID;
}

extern "C" int srt_tracker_counter_string(const srt_trk_counters *c, char *buf, size_t cap) {
    if (!c || (cap && !buf)) return -1;
    const unsigned long long packets =
        c->packets_control + c->packets_control_retrans + c->packets_data + c->packets_data_retrans;
    const unsigned long long bytes = c->bytes_control_header + c->bytes_control_header_retrans + c->bytes_data_header +
                                     c->bytes_data_header_retrans + c->bytes_data_payload +
                                     c->bytes_data_payload_retrans;
    return std::snprintf(buf, cap, "%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu", packets, bytes,
                         (unsigned long long)c->packets_control, (unsigned long long)c->bytes_control_header,
                         (unsigned long long)c->packets_control_retrans,
                         (unsigned long long)c->bytes_control_header_retrans, (unsigned long long)c->packets_data,
                         (unsigned long long)c->bytes_data_header, (unsigned long long)c->bytes_data_payload,
                         (unsigned long long)c->packets_data_retrans, (unsigned long long)c->bytes_data_header_retrans,
                         (unsigned long long)c->bytes_data_payload_retrans);
}
