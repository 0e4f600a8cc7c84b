// srt_deliver_step.h -- the interface's receive stage behind the inbound
// router (networkinterface_push, host/network/network_interface.c:140-202, as
// Relay::forward_until_blocked calls it, network/relay/mod.rs:260-270), written
// once for the host and the device (srt_deliver.hip compiles it for both).
//
// Which packets: those of one srt_inbound_run call whose status has
// RELAY_FORWARDED -- batch packets and late records alike.  Order: grouped by
// destination host, each host's late packets by ascending seq, then its batch
// packets by ascending position in the window (the CoDel queue is a FIFO and
// the window is in final order).  So a host's count is late + batch, its base
// an exclusive scan over the hosts, a batch packet's place base + late count +
// its rank among the forwarded packets of its segment.  No global sort: only a
// host's late run is ordered, by seq.
//
// Lookup: the host's socket associations as they stand at the call, the
// specific key (protocol, local port, peer ip, peer port) first, then the
// wildcard (protocol, local port, 0, 0); fields are compared verbatim as
// integers.  The table is open addressing with linear probing over 16-byte
// slots, built on the host (table_build) and probed by the same function on
// both sides; a load of at most 1/2 keeps a free slot behind every chain.
//
// The note ring keeps each pushed packet's srt_rx_meta under its flight tag
// (tag % note_cap); a tag is readable iff tag < note_end && note_end - tag <=
// note_cap.  The seq log keeps {tag, meta} of packets that stay in the inbound
// stage (seq % log_cap) under srt_sendbatch's rule: batch packet i is written
// iff walked - i <= log_cap, a late seq is read iff seq_base + n_pkts - seq <=
// log_cap, both distances from the end of the call's range (walked <= n_pkts),
// so a slot read is never one the same call writes.
//
// Every write is preceded by its range check: position < out_cap, dst_host <
// n_hosts, late index < the late list's length, ring and log distances.
#ifndef SRT_DELIVER_STEP_H
#define SRT_DELIVER_STEP_H

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/srt.h"

#include "srt_relay_common.h"

namespace deliver {

using relay::raise;

constexpr uint32_t F_OUT_OVERFLOW = SRT_DELIVER_OUT_OVERFLOW, F_LOG_OVERRUN = SRT_DELIVER_LOG_OVERRUN,
                   F_NOTE_OVERRUN = SRT_DELIVER_NOTE_OVERRUN, F_BAD_HOST = SRT_DELIVER_BAD_HOST;
constexpr uint32_t NO_SOCKET = 0xffffffffu;  // also a free slot's host
constexpr uint32_t RECEIVED = SRT_PDS_RCV_INTERFACE_RECEIVED, DROPPED = SRT_PDS_RCV_INTERFACE_DROPPED;
constexpr uint32_t SORT_CAP = 256;  // seqs of a host's late run held at once for ranking (FL_CAP of the flight sort)

// one association, one probe: 16 bytes
struct alignas(16) Slot {
    uint32_t host;     // NO_SOCKET: free
    uint32_t peer_ip;  // network byte order, verbatim
    uint32_t ports;    // local_port_be | peer_port_be << 16
    uint32_t sock;     // socket | (protocol == SRT_PROTO_UDP) << 31
};

// a packet that stays in the inbound stage, 32 bytes
struct LogRec {
    uint64_t tag;
    srt_rx_meta meta;
    uint32_t valid;  // 0: its tag was not readable in the note ring when it was logged
    uint32_t pad;
};

// the words a call leaves behind, 24 bytes
struct State {
    uint32_t flags;  // SRT_DELIVER_* bits since the last status call
    uint32_t pad;
    uint64_t n_delivered;  // the last run's delivered packets (the true count on OUT_OVERFLOW)
    uint64_t n_no_socket;  // of those written, the ones no socket took
};

struct Ctx {
    State *st;
    const Slot *table;
    uint32_t mask;  // slots - 1
    uint32_t n_hosts;
    srt_rx_meta *ring;
    LogRec *log;
    uint64_t note_cap, note_end, note_end_mod;  // note_end % note_cap (0 without a ring)
    uint64_t log_cap, base_mod, end_mod;        // seq_base % log_cap, (seq_base + n_pkts) % log_cap
    uint32_t *cnt;    // [n_hosts] forwarded batch packets of the host in this call; after the scan (device
                      // form): its written packets that no socket took
    uint32_t *nlate;  // [n_hosts] its forwarded late records
    uint32_t *lfill;  // [n_hosts] of those, the ones placed so far
    // note
    const srt_rx_meta *note_in;
    uint64_t note_first_mod;  // ring slot of note packet note_first
    uint32_t note_first, note_n;
    // run
    const uint32_t *dst_ptr, *status;
    const uint64_t *tag, *forward_ns;
    const srt_inbound_late *late;
    const uint32_t *late_count;  // nullptr: no late list
    uint64_t seq_base, out_cap;
    uint32_t n_pkts, late_cap;
    uint32_t *out_host_ptr, *out_socket, *out_user, *out_status;
    uint64_t *out_forward_ns, *out_tag;
};

// ---- the association table
SRT_HD uint32_t hash_key(uint32_t host, uint32_t peer_ip, uint32_t ports, uint32_t udp) {
    uint32_t h = host * 0x9E3779B1u ^ peer_ip * 0x85EBCA77u ^ ports * 0xC2B2AE3Du ^ udp;
    h ^= h >> 16, h *= 0x85EBCA6Bu, h ^= h >> 13, h *= 0xC2B2AE35u, h ^= h >> 16;
    return h;
}

SRT_HD uint32_t ports_word(uint16_t local_port_be, uint16_t peer_port_be) {
    return (uint32_t)local_port_be | (uint32_t)peer_port_be << 16;
}

// one key: at most mask + 1 slots, a free slot ends the chain
SRT_HD uint32_t probe(const Slot *table, uint32_t mask, uint32_t host, uint32_t peer_ip, uint32_t ports, uint32_t udp) {
    uint32_t at = hash_key(host, peer_ip, ports, udp) & mask;
    for (uint32_t n = 0; n <= mask; ++n, at = (at + 1) & mask) {
        const Slot s = table[at];
        if (s.host == NO_SOCKET) return NO_SOCKET;
        if (s.host == host && s.peer_ip == peer_ip && s.ports == ports && s.sock >> 31 == udp) return s.sock & 0x7fffffffu;
    }
    return NO_SOCKET;
}

// networkinterface_push's two lookups (network_interface.c:157-173); a protocol no association can
// have matches nothing
SRT_HD uint32_t lookup(const Slot *table, uint32_t mask, uint32_t host, const srt_rx_meta &m) {
    if (m.protocol != SRT_PROTO_TCP && m.protocol != SRT_PROTO_UDP) return NO_SOCKET;
    const uint32_t udp = m.protocol == SRT_PROTO_UDP;
    const uint32_t s = probe(table, mask, host, m.peer_ip_be, ports_word(m.local_port_be, m.peer_port_be), udp);
    if (s != NO_SOCKET || (m.peer_ip_be == 0 && m.peer_port_be == 0)) return s;
    return probe(table, mask, host, 0, ports_word(m.local_port_be, 0), udp);
}

// a slot for every association, keys in the caller's order; slots is a power of two, at least 2 * n
inline void table_build(Slot *table, uint32_t slots, const srt_assoc *a, size_t n, uint32_t *max_probe, uint32_t *wrapped) {
    const uint32_t mask = slots - 1;
    for (uint32_t i = 0; i < slots; ++i) table[i] = Slot{NO_SOCKET, 0, 0, 0};
    *max_probe = 0, *wrapped = 0;
    for (size_t k = 0; k < n; ++k) {
        const uint32_t udp = a[k].protocol == SRT_PROTO_UDP, ports = ports_word(a[k].local_port_be, a[k].peer_port_be);
        const uint32_t home = hash_key(a[k].host, a[k].peer_ip_be, ports, udp) & mask;
        uint32_t at = home, len = 1;
        while (table[at].host != NO_SOCKET) at = (at + 1) & mask, ++len;
        table[at] = Slot{a[k].host, a[k].peer_ip_be, ports, a[k].socket | udp << 31};
        if (len > *max_probe) *max_probe = len;
        if (at < home) *wrapped = 1;
    }
}

// ---- the note ring
SRT_HD void note_store(const Ctx &c, uint32_t i) {
    if (i < c.note_first || i >= c.note_n) return;  // older than the ring holds after this note
    uint64_t s = c.note_first_mod + (i - c.note_first);  // below 2 * note_cap
    if (s >= c.note_cap) s -= c.note_cap;
    c.ring[s] = c.note_in[i];
}

SRT_HD bool note_read(const Ctx &c, uint64_t tag, srt_rx_meta &m) {
    const uint64_t a = c.note_end - tag;
    if (tag >= c.note_end || a > c.note_cap) return false;
    m = c.ring[c.note_end_mod >= a ? c.note_end_mod - a : c.note_end_mod + (c.note_cap - a)];
    return true;
}

// ---- the walk
SRT_HD uint32_t walked(const Ctx &c) { return relay::walked(c.dst_ptr, c.n_hosts, c.n_pkts); }

// host h's segment of the window of `lim` walked packets
SRT_HD void segment(const Ctx &c, uint32_t lim, uint32_t h, uint32_t &b, uint32_t &e) {
    relay::segment(c.dst_ptr, lim, h, b, e);
}

SRT_HD bool forwarded(uint32_t status) { return (status & SRT_PDS_RELAY_FORWARDED) != 0; }

SRT_HD uint32_t late_n(const Ctx &c) { return relay::late_n(c.late_count, c.late_cap); }

// batch packet i of a window of `lim` walked packets is not forwarded: if it stays in the stage
// (enqueued, neither forwarded nor dropped) its tag and meta go to the log
SRT_HD void log_keep(const Ctx &c, uint32_t lim, uint32_t i, uint32_t status) {
    if (!(status & SRT_PDS_ROUTER_ENQUEUED) || (status & (SRT_PDS_RELAY_FORWARDED | SRT_PDS_ROUTER_DROPPED))) return;
    if ((uint64_t)(lim - i) > c.log_cap) return;
    LogRec r;
    r.tag = c.tag[i];
    r.valid = note_read(c, r.tag, r.meta);
    r.pad = 0;
    if (!r.valid) {
        raise(&c.st->flags, F_NOTE_OVERRUN);
        r.meta = srt_rx_meta{0, 0, 0, 0, 0xffffffffu};
    }
    c.log[(c.base_mod + i) % c.log_cap] = r;
}

// one late record joins its host's count
SRT_HD void count_late(const Ctx &c, uint32_t k) {
    if (!forwarded(c.late[k].status)) return;  // a router drop
    const uint32_t h = c.late[k].dst_host;
    if (h >= c.n_hosts) {
        raise(&c.st->flags, F_BAD_HOST);
        return;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(&c.nlate[h], 1u);
#else
    ++c.nlate[h];
#endif
}

// the scan's output for a host whose packets begin at `prefix`
SRT_HD uint32_t host_base(const Ctx &c, uint64_t prefix) { return relay::host_base(prefix, c.out_cap); }

SRT_HD void scan_end(const Ctx &c, uint64_t total) {
    c.out_host_ptr[c.n_hosts] = host_base(c, total);
    c.st->n_delivered = total;
    c.st->n_no_socket = 0;
    if (total > c.out_cap) raise(&c.st->flags, F_OUT_OVERFLOW);
}

// the record at `pos`: the lookup with what the table holds now; 1: no socket took it
SRT_HD uint32_t emit(const Ctx &c, uint32_t h, uint64_t pos, uint64_t tag, uint64_t forward_ns, uint32_t status,
                     bool known, const srt_rx_meta &m) {
    if (pos >= c.out_cap) return 0;  // OUT_OVERFLOW, raised by the scan
    uint32_t sock = NO_SOCKET, user = 0xffffffffu, miss = 0;
    if (known) {
        sock = lookup(c.table, c.mask, h, m);
        user = m.user;
        miss = sock == NO_SOCKET;
        status |= miss ? RECEIVED | DROPPED : RECEIVED;  // network_interface.c:151, 191
    }
    c.out_socket[pos] = sock;
    c.out_forward_ns[pos] = forward_ns;
    c.out_tag[pos] = tag;
    c.out_user[pos] = user;
    c.out_status[pos] = status;
    return miss;
}

// forwarded batch packet i of host h goes to `pos`
SRT_HD uint32_t emit_batch(const Ctx &c, uint32_t h, uint32_t i, uint64_t pos) {
    if (pos >= c.out_cap) return 0;
    const uint64_t tag = c.tag[i];
    srt_rx_meta m;
    const bool known = note_read(c, tag, m);
    if (!known) raise(&c.st->flags, F_NOTE_OVERRUN);
    return emit(c, h, pos, tag, c.forward_ns[i], c.status[i], known, m);
}

// late record k takes a place in its host's late run: its index waits in out_user
SRT_HD void place_late(const Ctx &c, uint32_t k) {
    if (!forwarded(c.late[k].status)) return;
    const uint32_t h = c.late[k].dst_host;
    if (h >= c.n_hosts) return;  // BAD_HOST was raised by the count
    const uint64_t pos = (uint64_t)c.out_host_ptr[h] + relay::take_slot(&c.lfill[h]);
    if (pos < c.out_cap) c.out_user[pos] = k;
}

// the part of host h's late run that lies inside the output
SRT_HD uint32_t late_run(const Ctx &c, uint32_t h, uint64_t &b) {
    b = c.out_host_ptr[h];
    const uint64_t room = c.out_cap - b;  // b <= out_cap
    return (uint32_t)(c.nlate[h] < room ? c.nlate[h] : room);
}

SRT_HD uint64_t late_seq(const Ctx &c, uint32_t k, uint32_t n_late) { return k < n_late ? c.late[k].seq : ~0ull; }

// late record k is number `pos` of the output
SRT_HD uint32_t emit_late(const Ctx &c, uint32_t h, uint64_t pos, uint32_t k, uint32_t n_late) {
    if (pos >= c.out_cap || k >= n_late) return 0;
    const srt_inbound_late r = c.late[k];
    const uint64_t end = c.seq_base + c.n_pkts, a = end - r.seq;
    if (r.seq >= end || a > c.log_cap) {
        raise(&c.st->flags, F_LOG_OVERRUN);
        return emit(c, h, pos, ~0ull, r.forward_ns, r.status, false, srt_rx_meta{0, 0, 0, 0, 0});
    }
    const LogRec g = c.log[c.end_mod >= a ? c.end_mod - a : c.end_mod + (c.log_cap - a)];
    if (!g.valid) raise(&c.st->flags, F_NOTE_OVERRUN);
    return emit(c, h, pos, g.tag, r.forward_ns, r.status, g.valid != 0, g.meta);
}

// ---- the host-only form: the same step, one packet after the other
inline void host_note(const Ctx &c) {
    for (uint32_t i = c.note_first; i < c.note_n; ++i) note_store(c, i);
}

inline void host_run(const Ctx &c) {
    const uint32_t lim = walked(c), n_late = late_n(c);
    for (uint32_t h = 0; h < c.n_hosts; ++h) {
        uint32_t b, e, n = 0;
        segment(c, lim, h, b, e);
        for (uint32_t i = b; i < e; ++i) {
            const uint32_t st = c.status[i];
            if (forwarded(st)) ++n;
            else log_keep(c, lim, i, st);
        }
        c.cnt[h] = n, c.nlate[h] = 0, c.lfill[h] = 0;
    }
    for (uint32_t k = 0; k < n_late; ++k) count_late(c, k);
    uint64_t run = 0;
    for (uint32_t h = 0; h < c.n_hosts; ++h) {
        c.out_host_ptr[h] = host_base(c, run);
        run += (uint64_t)c.cnt[h] + c.nlate[h];
    }
    scan_end(c, run);
    uint64_t miss = 0;
    for (uint32_t h = 0; h < c.n_hosts; ++h) {
        uint32_t b, e;
        segment(c, lim, h, b, e);
        uint64_t pos = (uint64_t)c.out_host_ptr[h] + c.nlate[h];
        for (uint32_t i = b; i < e; ++i)
            if (forwarded(c.status[i])) miss += emit_batch(c, h, i, pos++);
    }
    for (uint32_t k = 0; k < n_late; ++k) place_late(c, k);
    std::vector<uint32_t> idx;
    for (uint32_t h = 0; h < c.n_hosts; ++h) {
        uint64_t b;
        const uint32_t m = late_run(c, h, b);
        if (!m) continue;
        idx.assign(c.out_user + b, c.out_user + b + m);
        // equal seqs (a caller error) stay in placing order, as the device ranks them
        std::stable_sort(idx.begin(), idx.end(),
                         [&](uint32_t x, uint32_t y) { return late_seq(c, x, n_late) < late_seq(c, y, n_late); });
        for (uint32_t j = 0; j < m; ++j) miss += emit_late(c, h, b + j, idx[j], n_late);
    }
    relay::add_pending(reinterpret_cast<unsigned long long *>(&c.st->n_no_socket), miss);
}

}  // namespace deliver
#endif
