// srt_tracker_step.h -- the tracker's heartbeat byte counters for the internet
// interface (host/tracker.c:24-48 the Counters record, :188-212
// _tracker_updateCounters, :214-284 tracker_addInputBytes / addOutputBytes,
// :400-433 the counter string, :582-627 the heartbeat and its memset), written
// once for the host and the device (srt_tracker.hip compiles it for both).
//
// Counters: ten u64 a record in the reference's print order; a packet with
// payload > 0 is data, else control, SRT_TRK_RETRANS (PDS_SND_TCP_RETRANSMITTED)
// selects the retransmit class.  Kept per host and per socket slot, in and out,
// REMOTE only: on the internet interface no packet has the loopback address, an
// SRT_OUT_LOCAL packet included.  The LOCAL counters are the loopback
// interface's: srt_loopback_step.h, which uses the classes and record helpers
// below.
//
// Output side (networkinterface_pop, network_interface.c:310-340): a packet is
// counted in the call in which the interface popped it, forwarded or not:
//   1. a batch packet whose status has SND_INTERFACE_SENT;
//   2. a late record, unless its seq is the one remembered as its host's cached
//      packet at the end of the previous call (counted when it was popped);
//   3. the packet the relay holds cached at the end of this call, if its seq is
//      below seq_base and differs from the remembered one (queued earlier,
//      popped and held in this call: neither in the batch nor in the late list);
//   4. the remembered seq becomes the cached seq, or none.
// Rule 2 reads the remembered seqs before rule 4 writes them: the late records
// are taken first.  Metas of batch packets not popped go to the seq log (seq %
// log_cap) under srt_sendbatch's rule: batch packet i is written iff n_pkts - i
// <= log_cap, a seq below seq_base is read iff seq_base + n_pkts - seq <=
// log_cap, both distances from the end of the call's range, so a slot read is
// never one the same call writes.
//
// Input side (networkinterface_push, :140-202): a delivery record is counted iff
// a socket took it.  Its meta comes from the note ring by tag (tag % note_cap; a
// tag is readable iff tag < note_end && note_end - tag <= note_cap).
//
// Every write is preceded by its range check: host < n_hosts, slot < n_sockets,
// late index < the late list's length, ring and log distances.
#ifndef SRT_TRACKER_STEP_H
#define SRT_TRACKER_STEP_H

#include <stdint.h>

#include "../../include/srt.h"

#include "srt_relay_common.h"

namespace tracker {

using relay::NONE;
using relay::raise;

constexpr uint32_t F_LOG_OVERRUN = SRT_TRACKER_LOG_OVERRUN, F_NOTE_OVERRUN = SRT_TRACKER_NOTE_OVERRUN,
                   F_BAD_SOCKET = SRT_TRACKER_BAD_SOCKET, F_BAD_HOST = SRT_TRACKER_BAD_HOST;
constexpr uint32_t NO_SOCKET = 0xffffffffu;
constexpr uint32_t N_CTR = 10;  // u64 words of srt_trk_counters

// the words a call leaves behind, 24 bytes
struct State {
    uint32_t flags;  // SRT_TRACKER_* bits since the last status call
    uint32_t pad;
    uint64_t n_tx, n_rx;  // packets counted since create (device form: summed from the hosts' words by status)
};

struct Ctx {
    State *st;
    srt_trk_counters *node_in, *node_out;  // [n_hosts]
    srt_trk_counters *sock_in, *sock_out;  // [n_sockets]
    uint64_t *cnt_tx, *cnt_rx;             // [n_hosts] packets counted since create
    uint64_t *remembered;                  // [n_hosts] the cached seq at the end of the previous tx call, or NONE
    srt_trk_meta *ring, *log;
    uint64_t note_cap, note_end, note_end_mod;  // note_end % note_cap (0 without a ring)
    uint64_t log_cap, base_mod, end_mod;        // seq_base % log_cap, (seq_base + n_pkts) % log_cap
    uint32_t n_hosts, n_sockets;
    // note
    const srt_trk_meta *note_in;
    uint64_t note_first_mod;  // ring slot of note packet note_first
    uint32_t note_first, note_n;
    // tx
    const uint64_t *cached_seq;
    const uint32_t *host_ptr, *status;
    const srt_trk_meta *meta;
    const srt_outbound_late *late;
    const uint32_t *late_count;  // nullptr: no late list
    uint64_t seq_base;
    uint32_t n_pkts, late_cap;
    // rx
    const uint32_t *out_host_ptr, *out_socket, *out_status;
    const uint64_t *out_tag;
    uint64_t out_cap;
    // rx_flat
    const uint32_t *f_host, *f_socket;
    const srt_trk_meta *f_meta;
    uint32_t f_n;
};

// a lane's ten sums; every index is a constant, so they stay in registers
struct Acc {
    uint64_t v[N_CTR];
};

SRT_HD void acc_zero(Acc &a) {
#pragma unroll
    for (uint32_t j = 0; j < N_CTR; ++j) a.v[j] = 0;
}

// _tracker_updateCounters (tracker.c:188-212)
SRT_HD void acc_add(Acc &a, const srt_trk_meta &m) {
    const bool data = m.payload_size > 0, rt = (m.flags & SRT_TRK_RETRANS) != 0;
    const uint64_t c0 = !data && !rt, c1 = !data && rt, d0 = data && !rt, d1 = data && rt;
    const uint64_t hd = m.header_size, pl = m.payload_size;
    a.v[0] += c0, a.v[1] += c0 ? hd : 0;
    a.v[2] += c1, a.v[3] += c1 ? hd : 0;
    a.v[4] += d0, a.v[5] += d0 ? hd : 0, a.v[6] += d0 ? pl : 0;
    a.v[7] += d1, a.v[8] += d1 ? hd : 0, a.v[9] += d1 ? pl : 0;
}

SRT_HD uint64_t acc_packets(const Acc &a) { return a.v[0] + a.v[2] + a.v[4] + a.v[7]; }

SRT_HD void add64(uint64_t *p, uint64_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)n);
#else
    *p += n;
#endif
}

// one packet into a record that other lanes add to as well: two or three adds
SRT_HD void rec_add(srt_trk_counters *rec, const srt_trk_meta &m) {
    uint64_t *w = reinterpret_cast<uint64_t *>(rec);
    const bool data = m.payload_size > 0, rt = (m.flags & SRT_TRK_RETRANS) != 0;
    const uint32_t at = data ? (rt ? 7u : 4u) : (rt ? 2u : 0u);
    add64(w + at, 1);
    add64(w + at + 1, m.header_size);
    if (data) add64(w + at + 2, m.payload_size);
}

// the sums of one host's walk into its record: the one writer of this record in this launch
SRT_HD void rec_merge(srt_trk_counters *rec, const Acc &a) {
    uint64_t *w = reinterpret_cast<uint64_t *>(rec);
#pragma unroll
    for (uint32_t j = 0; j < N_CTR; ++j)
        if (a.v[j]) w[j] += a.v[j];
}

// the packet's socket slot; a slot the instance does not have is counted at the host only
SRT_HD void sock_add(const Ctx &c, srt_trk_counters *socks, uint32_t slot, const srt_trk_meta &m) {
    if (!c.n_sockets) return;
    if (slot >= c.n_sockets) {
        raise(&c.st->flags, F_BAD_SOCKET);
        return;
    }
    rec_add(socks + slot, m);
}

// ---- the note ring (srt_deliver's rule)
SRT_HD void note_store(const Ctx &c, uint32_t i) {
    if (i < c.note_first || i >= c.note_n) return;  // older than the ring holds after this note
    uint64_t s = c.note_first_mod + (i - c.note_first);  // below 2 * note_cap
    if (s >= c.note_cap) s -= c.note_cap;
    c.ring[s] = c.note_in[i];
}

SRT_HD bool note_read(const Ctx &c, uint64_t tag, srt_trk_meta &m) {
    const uint64_t a = c.note_end - tag;
    if (tag >= c.note_end || a > c.note_cap) return false;
    m = c.ring[c.note_end_mod >= a ? c.note_end_mod - a : c.note_end_mod + (c.note_cap - a)];
    return true;
}

// ---- the seq log
SRT_HD void log_put(const Ctx &c, uint32_t i, const srt_trk_meta &m) {
    if ((uint64_t)(c.n_pkts - i) > c.log_cap) return;
    c.log[(c.base_mod + i) % c.log_cap] = m;
}

// the meta of a packet of an earlier call; false: the log does not hold it (flagged)
SRT_HD bool log_get(const Ctx &c, uint64_t seq, srt_trk_meta &m) {
    const uint64_t end = c.seq_base + c.n_pkts, a = end - seq;
    if (seq >= c.seq_base || a > c.log_cap) {
        raise(&c.st->flags, F_LOG_OVERRUN);
        return false;
    }
    m = c.log[c.end_mod >= a ? c.end_mod - a : c.end_mod + (c.log_cap - a)];
    return true;
}

// ---- the walks
using relay::segment;

SRT_HD uint32_t tx_walked(const Ctx &c) { return relay::walked(c.host_ptr, c.n_hosts, c.n_pkts); }

SRT_HD uint32_t rx_walked(const Ctx &c) {
    return c.out_host_ptr[c.n_hosts] < c.out_cap ? c.out_host_ptr[c.n_hosts] : (uint32_t)c.out_cap;
}

SRT_HD uint32_t late_n(const Ctx &c) { return relay::late_n(c.late_count, c.late_cap); }

// rule 1, and the log for the packets that stay queued
SRT_HD void tx_batch(const Ctx &c, uint32_t i, Acc &a) {
    const srt_trk_meta m = c.meta[i];
    if (c.status[i] & SRT_PDS_SND_INTERFACE_SENT) {
        acc_add(a, m);
        sock_add(c, c.sock_out, m.socket_slot, m);
    } else {
        log_put(c, i, m);
    }
}

// rules 3 and 4, once a host
SRT_HD void tx_cached(const Ctx &c, uint32_t h, Acc &a) {
    const uint64_t cs = c.cached_seq[h];
    srt_trk_meta m;
    if (cs != NONE && cs < c.seq_base && cs != c.remembered[h] && log_get(c, cs, m)) {
        acc_add(a, m);
        sock_add(c, c.sock_out, m.socket_slot, m);
    }
    c.remembered[h] = cs;
}

// rule 2: late record k, any order, before the hosts' walk of the same call
SRT_HD void tx_late(const Ctx &c, uint32_t k) {
    const srt_outbound_late r = c.late[k];
    const uint32_t h = r.src_host;
    if (h >= c.n_hosts) {
        raise(&c.st->flags, F_BAD_HOST);
        return;
    }
    srt_trk_meta m;
    if (r.seq == c.remembered[h] || !log_get(c, r.seq, m)) return;
    rec_add(c.node_out + h, m);
    add64(c.cnt_tx + h, 1);
    sock_add(c, c.sock_out, m.socket_slot, m);
}

// delivery record p: counted iff a socket took it
SRT_HD void rx_record(const Ctx &c, uint32_t p, Acc &a) {
    const uint32_t sock = c.out_socket[p];
    if (!(c.out_status[p] & SRT_PDS_RCV_INTERFACE_RECEIVED)) {  // a placeholder: never looked up
        raise(&c.st->flags, F_NOTE_OVERRUN);
        return;
    }
    if (sock == NO_SOCKET) return;  // RCV_INTERFACE_DROPPED
    srt_trk_meta m;
    if (!note_read(c, c.out_tag[p], m)) {
        raise(&c.st->flags, F_NOTE_OVERRUN);
        return;
    }
    acc_add(a, m);
    sock_add(c, c.sock_in, sock, m);
}

// ungrouped record k
SRT_HD void rx_flat(const Ctx &c, uint32_t k) {
    const uint32_t h = c.f_host[k], sock = c.f_socket[k];
    if (h >= c.n_hosts) {
        raise(&c.st->flags, F_BAD_HOST);
        return;
    }
    if (sock == NO_SOCKET) return;
    const srt_trk_meta m = c.f_meta[k];
    rec_add(c.node_in + h, m);
    add64(c.cnt_rx + h, 1);
    sock_add(c, c.sock_in, sock, m);
}

// a host's sums join its record and its count of packets
SRT_HD void host_merge(srt_trk_counters *rec, uint64_t *cnt, const Acc &a) {
    const uint64_t n = acc_packets(a);
    if (!n) return;
    rec_merge(rec, a);
    *cnt += n;
}

// ---- the host-only form: the same step, one packet after the other
inline void host_note(const Ctx &c) {
    for (uint32_t i = c.note_first; i < c.note_n; ++i) note_store(c, i);
}

inline void host_tx(const Ctx &c) {
    const uint32_t n_late = late_n(c), lim = tx_walked(c);
    for (uint32_t k = 0; k < n_late; ++k) tx_late(c, k);
    for (uint32_t h = 0; h < c.n_hosts; ++h) {
        uint32_t b, e;
        segment(c.host_ptr, lim, h, b, e);
        Acc a;
        acc_zero(a);
        for (uint32_t i = b; i < e; ++i) tx_batch(c, i, a);
        tx_cached(c, h, a);
        host_merge(c.node_out + h, c.cnt_tx + h, a);
    }
}

inline void host_rx(const Ctx &c) {
    const uint32_t lim = rx_walked(c);
    for (uint32_t h = 0; h < c.n_hosts; ++h) {
        uint32_t b, e;
        segment(c.out_host_ptr, lim, h, b, e);
        Acc a;
        acc_zero(a);
        for (uint32_t p = b; p < e; ++p) rx_record(c, p, a);
        host_merge(c.node_in + h, c.cnt_rx + h, a);
    }
}

inline void host_rx_flat(const Ctx &c) {
    for (uint32_t k = 0; k < c.f_n; ++k) rx_flat(c, k);
}

}  // namespace tracker
#endif
