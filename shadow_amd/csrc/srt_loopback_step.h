// srt_loopback_step.h -- one host's loopback interface for one call: the
// relay, the receive and the tracker's local counters, written once for the
// host and the device (srt_loopback.hip compiles it for both).
//
// Reference:
//   notify   host/host.rs:988-1002 -> networkinterface_wantsSend
//            (host/network/network_interface.c:344-370) and Relay::notify
//            (network/relay/mod.rs:110-135: an Idle relay schedules its forward
//            task with delay 0, one host event id)
//   task     relay/mod.rs:200-272 with RateLimit::Unlimited (host.rs:307-310):
//            no bucket, no cached packet, every packet local; the task pops
//            until the interface is empty (network_interface.c:205-340 over
//            network_queuing_disciplines.c) and pushes each packet back into
//            the same interface at the task's time
//   push     network_interface.c:140-202: RCV_INTERFACE_RECEIVED, the specific
//            then the wildcard key of the loopback interface's own table
//            (deliver::lookup), tracker_addInputBytes iff a socket took it
//   counters host/tracker.c:188-284, the local records (tracker classes and
//            record helpers: srt_tracker_step.h)
//
// The stage keeps the event-order contract of srt_outbound_step.h: at equal
// times every arrival runs before the forward task.  So the interface is empty
// between instants, an instant is a run of equal ready_ns in a host's span, and
// within one instant both qdisc orders are sort keys of the packets (distinct
// priorities):
//   FIFO  ascending running maximum of the priority along the packet's socket,
//         ties (inside one socket only) in arrival order;
//   RR    ascending (rank of the packet within its socket, arrival index of
//         that socket's first packet).
// A packet's key needs the earlier packets of its instant only; its place is
// its instant's begin plus the number of the instant's packets that sort
// before it.  Every packet of a host that is not flagged is received, so a
// host's output span is its input span.
//
// Per-packet scratch (the instance's, grows to the largest batch): the key,
// the begin of the packet's instant and, at that begin, the instant's end.
// Every write is preceded by its range check: a place lies in the host's span,
// a slot below n_slots.
#ifndef SRT_LOOPBACK_STEP_H
#define SRT_LOOPBACK_STEP_H

#include <stdint.h>

#include "../../include/srt.h"

#include "srt_deliver_step.h"
#include "srt_relay_common.h"
#include "srt_tracker_step.h"

namespace loopb {

using relay::NONE;
using relay::raise;
using tracker::Acc;

constexpr uint32_t F_TIME_ORDER = SRT_LOOPBACK_TIME_ORDER, F_BAD_SOCKET = SRT_LOOPBACK_BAD_SOCKET,
                   F_BAD_SLOT = SRT_LOOPBACK_BAD_SLOT;
constexpr uint32_t F_HOST = F_TIME_ORDER | F_BAD_SOCKET;  // these flag the host: its span is not run
constexpr uint32_t A_GROUP = 1u << 8, A_TASK = 1u << 9;   // arrival(): first of its instant in this call; starts a task
constexpr uint32_t NO_SOCKET = 0xffffffffu;
constexpr uint32_t RECEIVED = SRT_PDS_SND_INTERFACE_SENT | SRT_PDS_RELAY_FORWARDED | SRT_PDS_RCV_INTERFACE_RECEIVED;

// the words a call leaves behind, 24 bytes
struct State {
    uint32_t flags;  // SRT_LOOPBACK_* bits since the last status call
    uint32_t pad;
    uint64_t n_received, n_no_socket;  // the last run's (device form: summed from the hosts' words by status)
};

// what a host carries between calls, 16 bytes
struct HostSt {
    uint64_t last_ns;  // the last instant seen (NONE: none yet)
    uint64_t tasks;    // forward tasks scheduled so far: each took one host event id
};

struct Ctx {
    State *st;
    HostSt *hs;                                // [n_hosts]
    uint32_t *cnt_recv, *cnt_miss;             // [n_hosts] the last run's received packets, and those no socket took
    srt_trk_counters *node_in, *node_out;      // [n_hosts] the local records
    srt_trk_counters *slot_in, *slot_out;      // [n_slots]
    uint64_t *key;                             // [n_pkts] scratch
    uint32_t *grp, *gend;                      // [n_pkts] scratch
    const deliver::Slot *table;                // the loopback interface's associations
    uint32_t mask;
    uint32_t n_hosts, n_slots, max_sockets, qdisc, n_pkts;
    const srt_out_pkt *pkts;
    const uint32_t *host_ptr;
    const srt_rx_meta *rx_meta;
    const srt_trk_meta *trk_meta;  // nullptr: nothing is counted
    uint32_t *out_index, *out_socket, *out_user, *out_status;
    uint64_t *out_recv_ns;
};

SRT_HD uint32_t walked(const Ctx &c) { return relay::walked(c.host_ptr, c.n_hosts, c.n_pkts); }

// The socket-has-data event of packet i of the span beginning at b, `last` being the host's last
// instant of the earlier calls: F_* bits of what is wrong with it, A_GROUP when it is the first of
// its instant in this call, A_TASK when it finds the relay Idle.  An instant continued from an
// earlier call is a group of its own (its packets pop after everything that call held) and takes
// no further event id.
SRT_HD uint32_t arrival(const Ctx &c, uint32_t b, uint32_t i, uint64_t last) {
    const uint64_t ready = c.pkts[i].ready_ns;
    const uint64_t prev = i > b ? c.pkts[i - 1].ready_ns : last;
    const bool has_prev = i > b || last != NONE;
    uint32_t a = 0;
    if (i == b || ready != prev) a |= A_GROUP;
    if (!has_prev || ready != prev) a |= A_TASK;
    if (has_prev && ready < prev) a |= F_TIME_ORDER;
    if (c.pkts[i].socket >= c.max_sockets) a |= F_BAD_SOCKET;
    return a;
}

// packet i of the instant beginning at gb: its key, its instant, and the instant's end when it is the last
SRT_HD void key_store(const Ctx &c, uint32_t gb, uint32_t i, uint32_t e) {
    const srt_out_pkt p = c.pkts[i];
    uint64_t mx = p.priority;
    uint32_t rank = 0, first = i;
#pragma unroll 4
    for (uint32_t j = gb; j < i; ++j) {
        const uint32_t sj = c.pkts[j].socket;
        const uint64_t pj = c.pkts[j].priority;
        if (sj != p.socket) continue;
        mx = pj > mx ? pj : mx;
        if (!rank) first = j;
        ++rank;
    }
    c.key[i] = c.qdisc == SRT_QDISC_FIFO ? mx : (uint64_t)rank << 32 | first;
    c.grp[i] = gb;
    if (i + 1 >= e || c.pkts[i + 1].ready_ns != p.ready_ns) c.gend[gb] = i + 1;
}

// the end of one host's arrivals: a flagged host keeps its state
SRT_HD void scan_done(const Ctx &c, uint32_t h, uint32_t b, uint32_t e, uint32_t bits, uint32_t n_tasks) {
    if (bits & F_HOST) {
        raise(&c.st->flags, bits & F_HOST);
        return;
    }
    if (e == b) return;
    HostSt s = c.hs[h];
    s.last_ns = c.pkts[e - 1].ready_ns;
    s.tasks += n_tasks;
    c.hs[h] = s;
}

// the packet's slot record; a slot the instance does not have is counted at the host only
SRT_HD void slot_add(const Ctx &c, srt_trk_counters *slots, uint32_t slot, const srt_trk_meta &m) {
    if (!c.n_slots) return;
    if (slot >= c.n_slots) {
        raise(&c.st->flags, F_BAD_SLOT);
        return;
    }
    tracker::rec_add(slots + slot, m);
}

// Packet i of host h's span [b, e): popped at its place in the qdisc's order (the out counters),
// pushed back into the interface (the lookup, the in counters), written at that place.
// Returns 1 when no socket took it.
SRT_HD uint32_t emit(const Ctx &c, uint32_t h, uint32_t b, uint32_t e, uint32_t i, Acc &in, Acc &out) {
    uint32_t gb = c.grp[i];
    if (gb < b || gb > i) gb = i;  // the scratch is the step's own: only to stay inside the span
    uint32_t ge = c.gend[gb];
    if (ge <= i || ge > e) ge = i + 1;
    const uint64_t k = c.key[i];
    uint32_t r = 0;
#pragma unroll 4
    for (uint32_t j = gb; j < ge; ++j) {
        const uint64_t kj = c.key[j];
        r += (kj < k) | ((kj == k) & (j < i));
    }
    const uint32_t pos = gb + r;
    if (pos >= e) return 0;
    const srt_rx_meta rx = c.rx_meta[i];
    const uint32_t sock = deliver::lookup(c.table, c.mask, h, rx);
    const uint32_t miss = sock == NO_SOCKET;
    c.out_index[pos] = i;
    c.out_socket[pos] = sock;
    c.out_recv_ns[pos] = c.pkts[i].ready_ns;
    c.out_user[pos] = rx.user;
    c.out_status[pos] = miss ? RECEIVED | SRT_PDS_RCV_INTERFACE_DROPPED : RECEIVED;
    if (c.trk_meta) {
        const srt_trk_meta m = c.trk_meta[i];
        tracker::acc_add(out, m);  // tracker_addOutputBytes in networkinterface_pop
        slot_add(c, c.slot_out, m.socket_slot, m);
        if (!miss) {  // tracker_addInputBytes in networkinterface_push
            tracker::acc_add(in, m);
            slot_add(c, c.slot_in, sock, m);
        }
    }
    return miss;
}

// packet i of a flagged host: not run
SRT_HD void emit_flagged(const Ctx &c, uint32_t i) {
    c.out_index[i] = i;
    c.out_socket[i] = NO_SOCKET;
    c.out_recv_ns[i] = NONE;
    c.out_user[i] = c.rx_meta[i].user;
    c.out_status[i] = 0;
}

// the end of one host's run: its sums join its records (this host's one writer), its counts are the run's
SRT_HD void emit_done(const Ctx &c, uint32_t h, const Acc &in, const Acc &out, uint32_t n_recv, uint32_t n_miss) {
    tracker::rec_merge(c.node_in + h, in);
    tracker::rec_merge(c.node_out + h, out);
    c.cnt_recv[h] = n_recv;
    c.cnt_miss[h] = n_miss;
}

// ---- the host-only form: the same step, one packet after the other
inline void host_run(const Ctx &c) {
    const uint32_t lim = walked(c);
    uint64_t n_recv = 0, n_miss = 0;
    for (uint32_t h = 0; h < c.n_hosts; ++h) {
        uint32_t b, e;
        relay::segment(c.host_ptr, lim, h, b, e);
        const uint64_t last = c.hs[h].last_ns;
        uint32_t bits = 0, n_tasks = 0, gb = b;
        for (uint32_t i = b; i < e; ++i) {
            const uint32_t a = arrival(c, b, i, last);
            bits |= a & F_HOST;
            n_tasks += (a & A_TASK) != 0;
            if (a & A_GROUP) gb = i;
            key_store(c, gb, i, e);
        }
        scan_done(c, h, b, e, bits, n_tasks);
        Acc in, out;
        tracker::acc_zero(in);
        tracker::acc_zero(out);
        uint32_t miss = 0;
        for (uint32_t i = b; i < e; ++i) {
            if (bits) emit_flagged(c, i);
            else miss += emit(c, h, b, e, i, in, out);
        }
        emit_done(c, h, in, out, bits ? 0 : e - b, miss);
        n_recv += bits ? 0 : e - b;
        n_miss += miss;
    }
    c.st->n_received = n_recv;
    c.st->n_no_socket = n_miss;
}

}  // namespace loopb
#endif
