// srt_sendbatch_step.h -- the send-batch gather between the outbound relay
// stage and the send decision, written once for the host and the device
// (srt_sendbatch.hip compiles it for both).
//
// Within one srt_outbound_run call every send rank a host hands out comes from
// one per-host counter (outb::Host::sent), batch packets and late packets
// alike, so a host's ranks of a call are one contiguous run [first, first +
// count) and a packet's place in the grouped send batch is
//   host_base[h] + (rank - first[h]).
// The step is therefore: per host the count and the smallest rank of its
// forwarded non-local packets (its batch segment, plus the late records naming
// it), an exclusive scan of the counts over the hosts, and a scatter.  No sort.
//
// The log.  What srt_pkt needs beyond the outbound stage's outputs (srt_send_meta)
// is kept for packets that stay in the stage: a ring of log_cap records addressed
// by seq % log_cap.  A call writes batch packet i (seq = seq_base + i) iff its
// send_rank is UINT64_MAX and n_pkts - i <= log_cap, and a late packet's seq is
// read back iff seq_base + n_pkts - seq <= log_cap: the distance from the end of
// the call's sequence range.  A slot read by that rule belongs to a seq at least
// seq_base + n_pkts - log_cap, so no write of the same call (all below seq_base +
// n_pkts) can land on it, and of two batch packets of a call that share a slot
// only the newer is written: the rule does not depend on the order of writes.
//
// Every write is preceded by its range check: rank - first < count, position <
// out_cap, src_host < n_hosts.
#ifndef SRT_SENDBATCH_STEP_H
#define SRT_SENDBATCH_STEP_H

#include <stdint.h>

#include "../../include/srt.h"

#include "srt_relay_common.h"

namespace sendb {

using relay::NONE;
using relay::raise;

constexpr uint32_t F_OUT_OVERFLOW = SRT_SENDBATCH_OUT_OVERFLOW, F_RANK_GAP = SRT_SENDBATCH_RANK_GAP,
                   F_LOG_OVERRUN = SRT_SENDBATCH_LOG_OVERRUN, F_BAD_HOST = SRT_SENDBATCH_BAD_HOST;

struct Ctx {
    const uint32_t *host_ptr;
    const srt_send_meta *meta;
    const uint64_t *send_ns;
    const uint64_t *send_rank;
    const srt_outbound_late *late;
    const uint32_t *late_count;  // nullptr: no late list
    srt_send_meta *log;
    uint32_t *cnt;    // [n_hosts] forwarded non-local packets of the host in this call
    uint64_t *first;  // [n_hosts] their smallest rank
    srt_pkt *out_pkts;
    uint32_t *out_host_ptr;
    uint32_t *out_user;
    uint64_t *out_seq;
    uint32_t *flags;  // [0] SRT_SENDBATCH_* bits, [2..3] u64 n_sent
    uint64_t seq_base, log_cap, out_cap;
    uint64_t end_mod;  // (seq_base + n_pkts) % log_cap (0 without a log)
    uint32_t n_hosts, n_pkts, late_cap, pad;
};

SRT_HD uint32_t late_n(const Ctx &c) { return relay::late_n(c.late_count, c.late_cap); }

// host h's segment of the batch
SRT_HD void segment(const Ctx &c, uint32_t h, uint32_t &b, uint32_t &e) {
    relay::segment(c.host_ptr, relay::walked(c.host_ptr, c.n_hosts, c.n_pkts), h, b, e);
}

// the log slot of the seq that lies `a` before the end of the call's range, 0 <= a <= log_cap
SRT_HD uint64_t log_slot(const Ctx &c, uint64_t a) { return c.end_mod >= a ? c.end_mod - a : c.end_mod + (c.log_cap - a); }

// batch packet i stays in the stage (or is local): its meta goes to the log
SRT_HD void log_keep(const Ctx &c, uint32_t i) {
    const uint64_t a = (uint64_t)c.n_pkts - i;
    if (a <= c.log_cap) c.log[log_slot(c, a)] = c.meta[i];
}

// one late record joins its host's count and smallest rank
SRT_HD void count_late(const Ctx &c, uint32_t k) {
    const uint64_t rank = c.late[k].send_rank;
    const uint32_t h = c.late[k].src_host;
    if (rank == NONE) return;  // a local packet: never reaches the send decision
    if (h >= c.n_hosts) {
        raise(c.flags, F_BAD_HOST);
        return;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(&c.cnt[h], 1u);
    atomicMin(reinterpret_cast<unsigned long long *>(&c.first[h]), (unsigned long long)rank);
#else
    ++c.cnt[h];
    if (rank < c.first[h]) c.first[h] = rank;
#endif
}

// the scan's output for a host whose packets begin at `prefix` of `total` sent
SRT_HD uint32_t host_base(const Ctx &c, uint64_t prefix) { return relay::host_base(prefix, c.out_cap); }

SRT_HD void scan_end(const Ctx &c, uint64_t total) {
    c.out_host_ptr[c.n_hosts] = host_base(c, total);
    c.flags[2] = (uint32_t)total;
    c.flags[3] = (uint32_t)(total >> 32);
    if (total > c.out_cap) raise(c.flags, F_OUT_OVERFLOW);
}

// a host's run of the call: where its packets begin in the output, how many, their smallest rank
struct HostRun {
    uint64_t first;
    uint32_t cnt, base;
};
SRT_HD HostRun host_run(const Ctx &c, uint32_t h) {
    HostRun r;
    r.first = c.first[h], r.cnt = c.cnt[h], r.base = c.out_host_ptr[h];
    return r;
}

// rank -> position, the range checks, the record
SRT_HD void emit(const Ctx &c, const HostRun &hr, uint32_t h, uint64_t rank, uint64_t send_ns, const srt_send_meta &m,
                 uint64_t seq) {
    const uint64_t d = rank - hr.first;
    if (d >= hr.cnt) {
        raise(c.flags, F_RANK_GAP);
        return;
    }
    const uint64_t pos = (uint64_t)hr.base + d;
    if (pos >= c.out_cap) return;  // OUT_OVERFLOW, raised by the scan
    srt_pkt p;
    p.src_host = h;
    p.src_row = m.src_row;
    p.dst_row = m.dst_row;
    p.payload_size = m.payload_size;
    p.t_ns = send_ns;
    c.out_pkts[pos] = p;
    c.out_user[pos] = m.user;
    c.out_seq[pos] = seq;
}

SRT_HD void scatter_batch(const Ctx &c, const HostRun &hr, uint32_t h, uint32_t i) {
    const uint64_t rank = c.send_rank[i];
    if (rank != NONE) emit(c, hr, h, rank, c.send_ns[i], c.meta[i], c.seq_base + i);
}

SRT_HD void scatter_late(const Ctx &c, uint32_t k) {
    const srt_outbound_late r = c.late[k];
    if (r.send_rank == NONE || r.src_host >= c.n_hosts) return;  // local; BAD_HOST was raised by the count
    const uint64_t a = c.seq_base + c.n_pkts - r.seq;
    srt_send_meta m;
    if (a <= c.log_cap) {
        m = c.log[log_slot(c, a)];
    } else {
        raise(c.flags, F_LOG_OVERRUN);
        m.src_row = m.dst_row = m.payload_size = 0;
        m.user = 0xffffffffu;
    }
    emit(c, host_run(c, r.src_host), r.src_host, r.send_rank, r.send_ns, m, r.seq);
}

}  // namespace sendb
#endif
