// srt_udpsend_step.h -- one host's UDP send side for one window: its sockets'
// send buffers and its outbound relay in one event loop, written once for the
// host and the device (srt_udpsend.hip compiles it for both,
// tests/asan/udpsend_check.cpp for the host alone).
//
// Reference:
//   sendmsg        host/descriptor/socket/inet/udp.rs:327-475 (the checks' order,
//                  has_space, the priority draw, the 0.0.0.0 source rewrite)
//   pop            udp.rs:170-195 pull_out_packet, :197-203 the head's priority,
//                  :1056-1134 MessageBuffer, under network_interface.c:205-370
//   relay          relay/mod.rs:200-272 with the TokenBucket of srt_relay_common.h;
//                  the loop is srt_outbound_step.h's, restated here because a pop
//                  changes a socket's buffer and may wake a blocked send
//   config         udp.rs:874-899 SO_SNDBUF, :767-788 shutdown, :229-240 close
//   event order    the list's calls of time t, the forward task of t, its
//                  wake-ups, then a further forward task of t if one was scheduled
//
// Store.  A slot's queue is the messages earlier calls left in its ring (`carry`
// of them from `ring_head`, in order) followed by a linked list of the messages
// accepted in this call.  An element of the list is named by a u32: the index of
// its call, whose staged record (Rec) holds its priority, its flags and its
// link; or RING_BIT | the slot's place in its host, which names the slot's spare
// ring element: the send an EARLIER call armed and this call woke.  A pop takes
// the carried messages first.  At the end of a call each slot still in the qdisc
// writes its queue back to the front of its ring in order, its capacity checked
// before every write.  The qdisc's slots are an array of the host's slot count:
// a circular queue for RR, a set scanned for the smallest head priority for FIFO.
// An armed send lives in its slot's state; the slots a forward task woke are
// chained through wake_next in the order of the pops.
#ifndef SRT_UDPSEND_STEP_H
#define SRT_UDPSEND_STEP_H

#include <stdint.h>

#include "../../include/srt.h"

#include "srt_relay_common.h"

namespace udps {

using relay::add_pending;
using relay::NONE;
using relay::raise;
using relay::sat_add;
using relay::take_slot;

constexpr uint32_t F_RING_OVERFLOW = SRT_UDPSEND_RING_OVERFLOW, F_LATE_OVERFLOW = SRT_UDPSEND_LATE_OVERFLOW,
                   F_TIME_REGRESSION = SRT_UDPSEND_TIME_REGRESSION, F_OVERSIZE = SRT_UDPSEND_OVERSIZE,
                   F_AFTER_UNTIL = SRT_UDPSEND_AFTER_UNTIL, F_BAD_SOCKET = SRT_UDPSEND_BAD_SOCKET,
                   F_UNBOUND = SRT_UDPSEND_UNBOUND, F_LOOPBACK = SRT_UDPSEND_LOOPBACK,
                   F_ARMED_TWICE = SRT_UDPSEND_ARMED_TWICE, F_REOPEN_BUSY = SRT_UDPSEND_REOPEN_BUSY,
                   F_LATE_RESULT_OVERFLOW = SRT_UDPSEND_LATE_RESULT_OVERFLOW, F_CALL_ORDER = SRT_UDPSEND_CALL_ORDER;
constexpr uint32_t F_ALL = 4095u;

constexpr uint32_t RING_BIT = 0x80000000u;  // element name: a slot's spare ring element
constexpr uint32_t NIL = 0xffffffffu;       // no element
constexpr int64_t E_BADF = -9, E_WOULDBLOCK = -11, E_PIPE = -32, E_DESTADDRREQ = -89, E_MSGSIZE = -90;
constexpr uint32_t DGRAM_MAX = 65507;         // CONFIG_DATAGRAM_MAX_SIZE
constexpr uint32_t HEADERS = 28;              // CONFIG_HEADER_SIZE_UDPIP
constexpr uint32_t LOCALHOST_BE = 0x0100007fu;  // 127.0.0.1 as the bytes 7f 00 00 01
constexpr uint64_t SNDBUF_MIN = 4096, SNDBUF_MAX = 1ull << 28;  // udp.rs:890, :895
constexpr uint32_t UDP_PDS = SRT_PDS_SND_CREATED;

// Sock.bits
constexpr uint16_t B_OPEN = 1, B_SHUT_WR = 2, B_BOUND = 4, B_PEER = 8, B_OVERFLOW = 16;
// RingEl.flags
constexpr uint32_t EL_LOCAL = SRT_OUT_LOCAL, EL_RAW = 2;

// Device: the workgroup's LDS, one wave's: WIN_CAP staged calls, then the state records and the qdisc
// entries of its 64 hosts' slots when they are at most SLOT_LDS (named through the shared symbol, not
// through pointers kept in the run, so that they are LDS instructions whose waits do not cover the
// outstanding stores to HBM)
constexpr uint32_t WIN_CAP = 1536;   // calls a wave may stage (48 KB)
constexpr uint32_t SLOT_LDS = 320;   // slots a wave's hosts may own for their state to sit in LDS (27.5 KB + 1.25 KB)
constexpr uint32_t SOCK_BYTES = 88;
constexpr uint32_t LDS_SOCK_OFF = WIN_CAP * 32, LDS_Q_OFF = LDS_SOCK_OFF + SLOT_LDS * SOCK_BYTES;
constexpr uint32_t LDS_BYTES = LDS_Q_OFF + SLOT_LDS * 4;
#if defined(__HIPCC__)
extern __shared__ __align__(16) unsigned char udps_lds[];
#endif

// the words a call leaves behind, 64 bytes
struct State {
    uint32_t flags;  // SRT_UDPSEND_* bits since the last status call
    uint32_t own_late_count, own_late_res_count, pad;  // for a caller that passes none
    unsigned long long pending;                         // packets in the stage after the last run
    unsigned long long n_acc, n_wb, n_arm;              // since create
    uint64_t spare[2];
};

// a staged call, 32 bytes.  `prio`: a raw arrival's priority; a UDP call's destination ip until it is
// accepted, its drawn priority from then on.  `flags`: the call's, SRT_UDPSEND_LOCAL set at acceptance.
struct alignas(16) Rec {
    uint64_t time;
    uint64_t prio;
    uint32_t slot;
    uint32_t len;
    uint32_t flags;
    uint32_t link;
};

// a message that crosses a call, 32 bytes
struct alignas(16) RingEl {
    uint64_t seq;
    uint64_t prio;
    uint32_t size;  // UDP: the payload; raw: total_size
    uint32_t flags;
    uint32_t link;  // of the spare element only
    uint32_t pad;
};

// a socket slot, 88 bytes
struct alignas(8) Sock {
    uint64_t len_bytes, soft_limit, armed_seq;
    uint32_t armed_len, armed_dst_ip, armed_flags, armed_user;  // the blocked send
    uint32_t bind_ip, peer_ip;
    uint16_t bind_port, peer_port, pad16, bits;
    uint32_t n_msgs;             // messages queued: carried and this call's
    uint32_t carry, ring_head;   // of them still in the ring, from ring_head (between calls: all, from 0)
    uint32_t head, tail;         // this call's list (between calls: NIL)
    uint32_t wake_next;          // the next slot the running forward task woke
    uint32_t fw_call;            // the call that last wrote first_writable for this slot
    uint32_t pad;
};

// per-host state, 112 bytes: outb::Host's, the counter, the address
struct alignas(16) Host {
    uint64_t balance, last_refill, refill, capacity;  // TokenBucket
    uint64_t task_ns;  // pending forward task (NONE: relay Idle)
    uint64_t tasks;    // forward tasks scheduled so far (event ids consumed)
    uint64_t sent;     // non-local packets forwarded so far: the next rank
    uint64_t cached_seq;
    uint64_t next_priority;
    uint32_t n_queued;  // messages in the slots' queues
    uint32_t cached, cached_size;
    uint32_t overflow;
    uint32_t q_head, q_len;  // the qdisc's slots: q[(q_head + k) % slots], k < q_len
    uint32_t ip;
    uint32_t cached_pds;  // SND_CREATED for a cached UDP packet
};

SRT_HD uint64_t cached_seq_of(const Host &s) { return s.cached ? s.cached_seq : NONE; }

struct Ctx {
    State *st;
    Host *hosts;
    Sock *socks;    // [n_sockets]
    RingEl *ring;   // [n_sockets][ring_cap + 1]
    uint32_t *sockq;  // [n_sockets]: host h's qdisc array is its slots' span
    const uint32_t *socket_ptr;
    Rec *rec;  // [n_calls]
    const srt_udp_send *calls;
    const uint32_t *host_ptr;
    srt_udpsend_result *results;
    uint32_t *status;
    uint64_t *send_ns;
    uint64_t *send_rank;
    srt_outbound_late *late;
    uint32_t *late_count;
    srt_udpsend_late *late_res;
    uint32_t *late_res_count;
    uint64_t *first_writable;
    const srt_udpsend_op *ops;
    uint64_t base, until, boot_end, prev_until;
    uint32_t n_hosts, n_sockets, ring_cap, n_calls;
    uint32_t late_cap, late_res_cap, qdisc, call_no;
    uint32_t n_ops, pad[3];
};

// ---- configuration
SRT_HD uint64_t sndbuf_limit(uint64_t optval) {  // udp.rs:884-895, the doubling saturating
    if (optval >= SNDBUF_MAX / 2) return SNDBUF_MAX;
    return optval * 2 > SNDBUF_MIN ? optval * 2 : SNDBUF_MIN;
}

SRT_HD void sock_init(Sock &s) {
    s.len_bytes = s.soft_limit = 0;
    s.armed_seq = NONE;
    s.armed_len = s.armed_dst_ip = s.armed_flags = s.armed_user = 0;
    s.bind_ip = s.peer_ip = 0;
    s.bind_port = s.peer_port = s.pad16 = s.bits = 0;
    s.n_msgs = s.carry = s.ring_head = 0;
    s.head = s.tail = s.wake_next = NIL;
    s.fw_call = 0;
    s.pad = 0;
}

SRT_HD void disarm(Sock &s) {
    s.armed_seq = NONE;
    s.armed_len = s.armed_dst_ip = s.armed_flags = s.armed_user = 0;
}

SRT_HD void apply_op(const Ctx &c, Sock &s, const srt_udpsend_op &op) {
    if (op.op == SRT_UDPSEND_OPEN) {
        if (s.n_msgs) {
            raise(&c.st->flags, F_REOPEN_BUSY);
            return;
        }
        const uint16_t keep = s.bits & B_OVERFLOW;
        const uint32_t fw = s.fw_call;
        sock_init(s);
        s.fw_call = fw;
        s.soft_limit = op.value;
        s.bits = B_OPEN | keep;
    } else if (!(s.bits & B_OPEN)) {
        return;
    } else if (op.op == SRT_UDPSEND_CLOSE) {
        s.bits &= (uint16_t)~B_OPEN;
        disarm(s);
    } else if (op.op == SRT_UDPSEND_BIND) {
        s.bind_ip = (uint32_t)op.value;
        s.bind_port = (uint16_t)(op.value >> 32);
        s.bits |= B_BOUND;
    } else if (op.op == SRT_UDPSEND_SET_PEER) {
        s.peer_ip = (uint32_t)op.value;
        s.peer_port = (uint16_t)(op.value >> 32);
        if (s.peer_ip || s.peer_port) s.bits |= B_PEER;
        else s.bits &= (uint16_t)~B_PEER;
    } else if (op.op == SRT_UDPSEND_SET_SNDBUF) {
        s.soft_limit = sndbuf_limit(op.value);
    } else if (op.op == SRT_UDPSEND_SHUT_WR) {
        if (s.bits & B_PEER) s.bits |= B_SHUT_WR;
    }
}

// the steps are sorted stably by (host step or not, slot): the first step of a run applies the run
SRT_HD bool same_target(const srt_udpsend_op &a, const srt_udpsend_op &b) {
    return a.slot == b.slot && (a.op == SRT_UDPSEND_SET_NEXT_PRIORITY) == (b.op == SRT_UDPSEND_SET_NEXT_PRIORITY);
}

SRT_HD void config_at(const Ctx &c, uint32_t i) {
    const srt_udpsend_op first = c.ops[i];
    if (i && same_target(c.ops[i - 1], first)) return;
    if (first.op == SRT_UDPSEND_SET_NEXT_PRIORITY) {
        if (first.slot >= c.n_hosts) return;
        uint64_t v = first.value;
        for (uint32_t k = i + 1; k < c.n_ops && same_target(c.ops[k], first); ++k) v = c.ops[k].value;
        c.hosts[first.slot].next_priority = v;
        return;
    }
    if (first.slot >= c.n_sockets) return;
    Sock s = c.socks[first.slot];
    for (uint32_t k = i; k < c.n_ops && same_target(c.ops[k], first); ++k) apply_op(c, s, c.ops[k]);
    c.socks[first.slot] = s;
}

// ---- the preset pass: call i's staged record and outputs, slot x's first_writable
SRT_HD void preset_call(const Ctx &c, uint32_t i) {
    const srt_udp_send p = c.calls[i];
    Rec r;
    r.time = p.time_ns;
    r.slot = p.slot;
    r.len = p.len;
    r.link = NIL;
    if (p.flags & SRT_UDPSEND_RAW) {
        r.prio = p.priority;
        r.flags = p.flags & (SRT_UDPSEND_RAW | SRT_UDPSEND_LOCAL);
    } else {
        r.prio = p.dst_ip_be;
        r.flags = p.flags & (SRT_UDPSEND_HAS_ADDR | SRT_UDPSEND_WAIT);
    }
    c.rec[i] = r;
    srt_udpsend_result z;
    z.complete_ns = z.priority = 0;
    z.return_val = 0;
    z.status = SRT_UDPSEND_NOT_TAKEN;
    z.src_ip_be = 0;
    z.src_port_be = z.reserved = 0;
    z.user = p.user;
    c.results[i] = z;
    c.status[i] = 0;
    c.send_ns[i] = NONE;
    c.send_rank[i] = NONE;
}

SRT_HD void preset_words(const Ctx &c) {
    *c.late_count = 0;
    *c.late_res_count = 0;
    c.st->pending = 0;
}

// one host's run over one call
// WIN: the wave staged its span of the calls in LDS; SL: and its hosts' slot records and qdisc arrays
template <bool WIN, bool SL = false>
struct Run {
    Host s;
    const Ctx c;  // by value: a reference member would keep the whole object in private memory
    uint32_t h;
    uint32_t win0, win_n;  // device: calls [win0, win0 + win_n) are held in LDS by the wave
    uint32_t sp0;          // device: the wave's first slot, LDS record 0
    uint32_t sb, ns;       // the host's slots [sb, sb + ns)
    uint32_t lo, ppos;     // calls [lo, ppos) have been taken up: the indices that are live names
    uint32_t wake_head, wake_tail;
    uint32_t n_acc, n_wb, n_arm;

    SRT_HD Run(const Ctx &ctx, uint32_t host)
        : s(ctx.hosts[host]), c(ctx), h(host), win0(0), win_n(0), sp0(0), sb(0), ns(0), lo(0), ppos(0), wake_head(NIL),
          wake_tail(NIL), n_acc(0), n_wb(0), n_arm(0) {}

    SRT_HD Rec &rec(uint32_t i) const {
#if defined(__HIP_DEVICE_COMPILE__)
        if (WIN) return reinterpret_cast<Rec *>(udps_lds)[i - win0];
#endif
        return c.rec[i];
    }
    SRT_HD Sock &sock(uint32_t slot) const {
#if defined(__HIP_DEVICE_COMPILE__)
        if (SL) return reinterpret_cast<Sock *>(udps_lds + LDS_SOCK_OFF)[slot - sp0];
#endif
        return c.socks[slot];
    }
    // entry p < ns of this host's qdisc array
    SRT_HD uint32_t &q(uint32_t p) const {
#if defined(__HIP_DEVICE_COMPILE__)
        if (SL) return reinterpret_cast<uint32_t *>(udps_lds + LDS_Q_OFF)[sb - sp0 + p];
#endif
        return c.sockq[sb + p];
    }
    SRT_HD RingEl *ring_of(uint32_t slot) const { return c.ring + (uint64_t)slot * ((uint64_t)c.ring_cap + 1); }
    SRT_HD RingEl *spare(uint32_t x) const { return ring_of(sb + (x ^ RING_BIT)) + c.ring_cap; }

    // x names an element of this host: every dereference of a stored name is preceded by this check
    SRT_HD bool live(uint32_t x) const { return x & RING_BIT ? (x ^ RING_BIT) < ns : x >= lo && x < ppos; }

    // A value loaded from the ring passes through here: it keeps the compiler from merging the
    // ring's load (HBM) and the window's (LDS) into one generic load of a selected address,
    // whose wait would cover the outstanding stores to HBM.
    template <typename T>
    SRT_HD static T from_ring(T v) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(v));
#endif
        return v;
    }

    SRT_HD uint32_t link_get(uint32_t x) const { return x & RING_BIT ? from_ring(spare(x)->link) : rec(x).link; }
    SRT_HD void link_set(uint32_t x, uint32_t v) const {
        if (x & RING_BIT) spare(x)->link = v;
        else rec(x).link = v;
    }
    // the message a live name stands for
    SRT_HD RingEl load(uint32_t x) const {
        RingEl e;
        if (x & RING_BIT) {
            const RingEl r = *spare(x);
            e.seq = from_ring(r.seq), e.prio = from_ring(r.prio), e.size = from_ring(r.size), e.flags = from_ring(r.flags);
        } else {
            const Rec r = rec(x);
            e.seq = c.base + x, e.prio = r.prio, e.size = r.len;
            e.flags = (r.flags & SRT_UDPSEND_RAW ? EL_RAW : 0u) | (r.flags & SRT_UDPSEND_LOCAL ? EL_LOCAL : 0u);
        }
        e.link = NIL, e.pad = 0;
        return e;
    }

    SRT_HD uint32_t q_slot(uint32_t k) const {
        const uint32_t p = s.q_head + k;  // both below ns (< 2^31)
        return p >= ns ? p - ns : p;
    }
    SRT_HD void q_push(uint32_t slot) {
        if (s.q_len < ns) q(q_slot(s.q_len++)) = slot;
    }

    // a packet leaves the stage: this call's by index, older ones to the late list
    SRT_HD void resolve(uint64_t seq, uint32_t status, uint64_t now, uint64_t rank) {
        if (seq >= c.base) {
            const uint64_t i = seq - c.base;
            if (i >= c.n_calls) return;
            c.status[i] = status;
            c.send_ns[i] = now;
            if (rank != NONE) c.send_rank[i] = rank;
        } else {
            const uint32_t k = take_slot(c.late_count);
            if (k < c.late_cap) {
                srt_outbound_late r;
                r.seq = seq;
                r.send_ns = now;
                r.send_rank = rank;
                r.status = status;
                r.src_host = h;
                c.late[k] = r;
            } else {
                raise(&c.st->flags, F_LATE_OVERFLOW);
            }
        }
    }

    // a call's answer: d_results[i], or a late result for a send an earlier call armed
    SRT_HD void answer(uint64_t seq, uint32_t user, uint32_t status, int64_t val, uint64_t at, uint64_t prio,
                       uint32_t src_ip, uint16_t src_port) {
        if (seq >= c.base) {
            const uint64_t i = seq - c.base;
            if (i >= c.n_calls) return;
            srt_udpsend_result &r = c.results[i];  // user, reserved: the preset pass's
            r.complete_ns = at;
            r.priority = prio;
            r.return_val = val;
            r.status = status;
            r.src_ip_be = src_ip;
            r.src_port_be = src_port;
        } else {
            const uint32_t k = take_slot(c.late_res_count);
            if (k < c.late_res_cap) {
                srt_udpsend_late l;
                l.seq = seq;
                l.result.complete_ns = at;
                l.result.priority = prio;
                l.result.return_val = val;
                l.result.status = status;
                l.result.src_ip_be = src_ip;
                l.result.src_port_be = src_port;
                l.result.reserved = 0;
                l.result.user = user;
                c.late_res[k] = l;
            } else {
                raise(&c.st->flags, F_LATE_RESULT_OVERFLOW);
            }
        }
    }

    // the message named x joins its slot's queue, the slot the qdisc unless it is in it, and the
    // relay is notified (host.rs:988-1002, Relay::notify)
    SRT_HD void enqueue(uint32_t x, uint32_t slot, uint64_t now) {
        Sock &S = sock(slot);
        link_set(x, NIL);
        if (!S.n_msgs) q_push(slot);
        const uint32_t t = S.tail;
        if (S.n_msgs > S.carry && live(t)) link_set(t, x);
        else S.head = x;
        S.tail = x;
        ++S.n_msgs;
        ++s.n_queued;
        ++n_acc;
        if (s.task_ns == NONE) {
            s.task_ns = now;
            ++s.tasks;
        }
    }

    // sendmsg from check 2 on (udp.rs:337-475) for the call `seq` on an open slot of this host.
    // x: the name its message takes if it is accepted.  false: no space, the caller blocks or refuses.
    SRT_HD bool send(uint32_t slot, uint64_t seq, uint32_t x, uint32_t len, uint32_t dst_ip, uint32_t flags,
                     uint32_t user, uint64_t now) {
        Sock &S = sock(slot);
        const uint16_t bits = S.bits;
        if (bits & B_SHUT_WR) {
            answer(seq, user, SRT_UDPSEND_DONE, E_PIPE, now, 0, 0, 0);
            return true;
        }
        if (!(flags & SRT_UDPSEND_HAS_ADDR)) {
            if (!(bits & B_PEER)) {
                answer(seq, user, SRT_UDPSEND_DONE, E_DESTADDRREQ, now, 0, 0, 0);
                return true;
            }
            dst_ip = S.peer_ip;
        }
        if (len > DGRAM_MAX) {
            answer(seq, user, SRT_UDPSEND_DONE, E_MSGSIZE, now, 0, 0, 0);
            return true;
        }
        if (!(bits & B_BOUND)) {
            raise(&c.st->flags, F_UNBOUND);
            answer(seq, user, SRT_UDPSEND_NOT_TAKEN, 0, 0, 0, 0, 0);
            return true;
        }
        const uint32_t bind_ip = S.bind_ip;
        if (dst_ip == LOCALHOST_BE || bind_ip == LOCALHOST_BE) {
            raise(&c.st->flags, F_LOOPBACK);
            answer(seq, user, SRT_UDPSEND_NOT_TAKEN, 0, 0, 0, 0, 0);
            return true;
        }
        if (!(S.len_bytes < S.soft_limit)) return false;
        const uint64_t prio = s.next_priority++;
        const uint32_t el_flags = dst_ip == s.ip ? EL_LOCAL : 0u;
        S.len_bytes += len;
        if (x & RING_BIT) {
            RingEl e;
            e.seq = seq, e.prio = prio, e.size = len, e.flags = el_flags, e.link = NIL, e.pad = 0;
            *spare(x) = e;
        } else {
            Rec &r = rec(x);
            r.prio = prio;
            if (el_flags) r.flags |= SRT_UDPSEND_LOCAL;
        }
        answer(seq, user, SRT_UDPSEND_DONE, (int64_t)len, now, prio, bind_ip ? bind_ip : s.ip, S.bind_port);
        enqueue(x, slot, now);
        return true;
    }

    // call i of the list, in order and inside the window
    SRT_HD void call(uint32_t i, const Rec &r) {
        const uint32_t slot = r.slot;
        const bool mine = slot >= sb && slot - sb < ns && slot < c.n_sockets;
        if (r.flags & SRT_UDPSEND_RAW) {
            if (!mine || (sock(slot).bits & B_OPEN)) {
                raise(&c.st->flags, F_BAD_SOCKET);  // not taken
                return;
            }
            answer(c.base + i, 0, SRT_UDPSEND_DONE, (int64_t)r.len, r.time, r.prio, 0, 0);
            enqueue(i, slot, r.time);
            return;
        }
        if (!mine || !(sock(slot).bits & B_OPEN)) {
            raise(&c.st->flags, F_BAD_SOCKET);
            answer(c.base + i, 0, SRT_UDPSEND_DONE, E_BADF, r.time, 0, 0, 0);
            return;
        }
        if (send(slot, c.base + i, i, r.len, (uint32_t)r.prio, r.flags, 0, r.time)) return;
        Sock &S = sock(slot);
        if ((r.flags & SRT_UDPSEND_WAIT) && S.armed_seq == NONE) {
            S.armed_seq = c.base + i;
            S.armed_len = r.len;
            S.armed_dst_ip = (uint32_t)r.prio;
            S.armed_flags = r.flags;
            S.armed_user = c.results[i].user;
            ++n_arm;
            answer(c.base + i, 0, SRT_UDPSEND_ARMED, 0, 0, 0, 0, 0);
        } else {
            if (r.flags & SRT_UDPSEND_WAIT) raise(&c.st->flags, F_ARMED_TWICE);
            ++n_wb;
            answer(c.base + i, 0, SRT_UDPSEND_DONE, E_WOULDBLOCK, r.time, 0, 0, 0);
        }
    }

    // the blocked send of a slot that turned writable runs again (udp.rs:465-472: blocked on WRITABLE)
    SRT_HD void wake(uint32_t slot, uint64_t now) {
        Sock &S = sock(slot);
        const uint64_t seq = S.armed_seq;
        if (seq == NONE || !(S.bits & B_OPEN)) return;
        uint32_t x = RING_BIT | (slot - sb);
        if (seq >= c.base) {
            x = (uint32_t)(seq - c.base);
            if (!live(x)) return;
        }
        const uint32_t len = S.armed_len, dst = S.armed_dst_ip, flags = S.armed_flags, user = S.armed_user;
        if (send(slot, seq, x, len, dst, flags, user, now)) disarm(S);  // else: no space after all, it blocks again
    }

    // networkinterface_pop: the next packet of the qdisc's choice; false: no slot has data
    SRT_HD bool pop(uint64_t &seq, uint32_t &size, uint32_t &flags, uint64_t now) {
        for (;;) {
            if (!s.q_len) return false;
            uint32_t k = 0;
            if (c.qdisc == SRT_QDISC_FIFO) {
                uint64_t best = 0, best_seq = 0;
                bool have = false;
                for (uint32_t j = 0; j < s.q_len; ++j) {
                    const uint32_t slot = q(q_slot(j));
                    if (slot - sb >= ns) continue;
                    const Sock &S = sock(slot);
                    uint64_t p, sq;
                    if (S.carry) {
                        if (S.ring_head >= c.ring_cap) continue;
                        const RingEl *e = ring_of(slot) + S.ring_head;
                        p = from_ring(e->prio), sq = from_ring(e->seq);
                    } else {
                        const uint32_t x = S.head;
                        if (!live(x)) continue;
                        if (x & RING_BIT) p = from_ring(spare(x)->prio), sq = from_ring(spare(x)->seq);
                        else p = rec(x).prio, sq = c.base + x;
                    }
                    // equal priorities (raw arrivals only, a caller error): in arrival order
                    if (!have || p < best || (p == best && sq < best_seq)) best = p, best_seq = sq, k = j, have = true;
                }
            }
            const uint32_t slot = q(q_slot(k));
            RingEl el;
            el.seq = 0, el.prio = 0, el.size = 0, el.flags = 0, el.link = NIL, el.pad = 0;
            bool ok = false, more = false;
            if (slot - sb < ns) {
                Sock &S = sock(slot);
                if (S.carry) {
                    if (S.ring_head < c.ring_cap) {
                        const RingEl r = ring_of(slot)[S.ring_head];
                        el.seq = from_ring(r.seq), el.size = from_ring(r.size), el.flags = from_ring(r.flags);
                        ok = true;
                    }
                    ++S.ring_head;
                    if (!--S.carry) S.ring_head = 0;
                } else {
                    const uint32_t x = S.head;
                    if (S.n_msgs && live(x)) {
                        el = load(x);
                        uint32_t nx = link_get(x);
                        if (!live(nx)) nx = NIL;
                        S.head = nx;
                        if (nx == NIL) S.tail = NIL;
                        ok = true;
                    }
                }
                if (ok && S.n_msgs) {
                    --S.n_msgs;
                } else {  // only on a host already marked: a slot that lost its messages
                    s.n_queued -= S.n_msgs < s.n_queued ? S.n_msgs : s.n_queued;
                    S.n_msgs = S.carry = S.ring_head = 0;
                    S.head = S.tail = NIL;
                }
                if (S.n_msgs == S.carry) S.head = S.tail = NIL;
                more = S.n_msgs != 0;
                if (ok && !(el.flags & EL_RAW)) {  // pull_out_packet
                    const bool had_space = S.len_bytes < S.soft_limit;
                    S.len_bytes -= el.size < S.len_bytes ? el.size : S.len_bytes;
                    if (!had_space && S.len_bytes < S.soft_limit && (S.bits & B_OPEN)) {  // turned WRITABLE
                        if (S.fw_call != c.call_no) {
                            S.fw_call = c.call_no;
                            c.first_writable[slot] = now;
                        }
                        if (S.armed_seq != NONE) {
                            const uint32_t ls = slot - sb;
                            S.wake_next = NIL;
                            if (wake_tail != NIL && wake_tail < ns) sock(sb + wake_tail).wake_next = ls;
                            else wake_head = ls;
                            wake_tail = ls;
                        }
                    }
                }
            }
            // the slot leaves the queue; with data left it goes back (RR: to the tail)
            if (c.qdisc == SRT_QDISC_FIFO) {
                if (!more) q(q_slot(k)) = q(q_slot(--s.q_len));
            } else {
                s.q_head = q_slot(1);
                --s.q_len;
                if (more) q_push(slot);
            }
            if (!ok) continue;
            if (s.n_queued) --s.n_queued;
            seq = el.seq, size = el.size, flags = el.flags;
            return true;
        }
    }

    // Relay::forward_until_blocked (relay/mod.rs:200-272) at the task's time, then the wake-ups
    SRT_HD void forward_task() {
        const uint64_t now = s.task_ns;
        s.task_ns = NONE;
        wake_head = wake_tail = NIL;
        for (;;) {
            uint64_t seq;
            uint32_t size, flags = 0;
            uint32_t st = SRT_PDS_SND_INTERFACE_SENT | SRT_PDS_RELAY_FORWARDED;
            if (s.cached) {
                seq = s.cached_seq;
                size = s.cached_size;
                s.cached = 0;
                st |= SRT_PDS_RELAY_CACHED | s.cached_pds;
            } else if (pop(seq, size, flags, now)) {
                if (!(flags & EL_RAW)) st |= UDP_PDS, size += HEADERS;
            } else {
                break;  // Idle
            }
            if (flags & EL_LOCAL) {  // pushed back into the interface: no tokens, no rank
                resolve(seq, st, now, NONE);
                continue;
            }
            uint64_t wait = 0;
            if (now >= c.boot_end &&
                !relay::bucket_remove(s.balance, s.last_refill, s.refill, s.capacity, size, now, wait)) {
                s.cached = 1;
                s.cached_seq = seq;
                s.cached_size = size;
                s.cached_pds = st & UDP_PDS;
                s.task_ns = sat_add(now, wait);
                if (size > s.capacity) {
                    // the bucket can never hold this packet (the reference would
                    // reschedule for ever): flagged, and at most one try a call
                    raise(&c.st->flags, F_OVERSIZE);
                    if (s.task_ns < c.until) s.task_ns = c.until;
                }
                ++s.tasks;
                break;  // Pending
            }
            resolve(seq, st, now, s.sent++);
        }
        // each slot is woken at most once a task: the walk ends within ns steps
        uint32_t x = wake_head;
        for (uint32_t n = ns; n && x < ns; --n) {
            const uint32_t nx = sock(sb + x).wake_next;
            wake(sb + x, now);
            x = nx;
        }
        wake_head = wake_tail = NIL;
    }

    // a slot still in the qdisc at the end of the call: its queue goes to the front of its ring in order
    SRT_HD void compact(uint32_t slot) {
        Sock &S = sock(slot);
        RingEl *r = ring_of(slot);
        uint32_t w = 0;
        for (uint32_t p = 0; p < S.carry; ++p) {  // w <= ring_head + p: a position is read before it is written
            const uint32_t from = S.ring_head + p;
            if (from >= c.ring_cap) break;
            if (from != w) r[w] = r[from];
            ++w;
        }
        uint32_t x = S.head;
        bool lost = false;
        for (uint32_t n = S.n_msgs - S.carry; n && live(x); --n) {
            const RingEl e = load(x);
            const uint32_t nx = link_get(x);
            if (w < c.ring_cap) r[w++] = e;
            else lost = true;
            x = nx;
        }
        if (lost) {
            if (!s.overflow) s.overflow = 1;
            S.bits |= B_OVERFLOW;
            raise(&c.st->flags, F_RING_OVERFLOW);
        }
        const uint32_t gone = S.n_msgs - w;
        s.n_queued -= gone < s.n_queued ? gone : s.n_queued;
        S.n_msgs = S.carry = w;
        S.ring_head = 0;
        S.head = S.tail = NIL;
    }

    SRT_HD void run() {
        // the host's slots and calls, held inside the arrays whatever the pointers say
        const uint32_t sp_b = c.socket_ptr[h] < c.n_sockets ? c.socket_ptr[h] : c.n_sockets;
        const uint32_t sp_e = c.socket_ptr[h + 1] < c.n_sockets ? c.socket_ptr[h + 1] : c.n_sockets;
        sb = sp_b, ns = sp_e > sp_b ? sp_e - sp_b : 0;
        uint32_t lim = c.host_ptr[c.n_hosts] < c.n_calls ? c.host_ptr[c.n_hosts] : c.n_calls;
        if (WIN && lim > win0 + win_n) lim = win0 + win_n;  // and inside the window
        uint32_t b = c.host_ptr[h] < lim ? c.host_ptr[h] : lim;
        if (WIN && b < win0) b = win0;
        uint32_t e = c.host_ptr[h + 1] < lim ? c.host_ptr[h + 1] : lim;
        if (e < b) e = b;
        if (s.q_head >= ns) s.q_head = 0;
        if (s.q_len > ns) s.q_len = ns;
        lo = ppos = b;
        uint64_t tmax = c.prev_until;  // the latest time of the calls taken up so far
        Rec nxt;
        nxt.time = 0;
        if (ppos < e) nxt = rec(ppos);
        for (;;) {
            if (ppos < e && nxt.time < tmax) {
                raise(&c.st->flags, nxt.time < c.prev_until ? F_TIME_REGRESSION : F_CALL_ORDER);  // not taken
                if (++ppos < e) nxt = rec(ppos);
            } else if (ppos < e && nxt.time < c.until && nxt.time <= s.task_ns) {
                const Rec x = nxt;
                const uint32_t i = ppos++;
                if (ppos < e) nxt = rec(ppos);  // in flight while this one is handled
                tmax = x.time;
                call(i, x);
            } else if (s.task_ns < c.until) {
                forward_task();
            } else {
                break;
            }
        }
        // A call at or after until_ns belongs to a later window: it is not taken and the call is flagged.
        if (ppos < e) raise(&c.st->flags, F_AFTER_UNTIL);
        if (s.n_queued) {
            for (uint32_t k = 0; k < s.q_len; ++k) {
                const uint32_t slot = q(q_slot(k));
                if (slot - sb < ns) compact(slot);
            }
            uint32_t n = 0;  // a slot that kept nothing (ring_cap 0) leaves the qdisc
            for (uint32_t k = 0; k < s.q_len; ++k) {
                const uint32_t slot = q(q_slot(k));
                if (slot - sb < ns && sock(slot).n_msgs) q(q_slot(n++)) = slot;
            }
            s.q_len = n;
        }
        if (s.cached && s.cached_seq >= c.base && s.cached_seq - c.base < c.n_calls)
            c.status[s.cached_seq - c.base] = SRT_PDS_SND_INTERFACE_SENT | SRT_PDS_RELAY_CACHED | s.cached_pds;
        add_pending(&c.st->pending, (unsigned long long)s.n_queued + s.cached);
        add_pending(&c.st->n_acc, n_acc);
        add_pending(&c.st->n_wb, n_wb);
        add_pending(&c.st->n_arm, n_arm);
        c.hosts[h] = s;
    }
};

// ---- the host-only form: the same step, one host after the other
inline void host_config(const Ctx &c) {
    for (uint32_t i = 0; i < c.n_ops; ++i) {
        const srt_udpsend_op &op = c.ops[i];
        if (op.op == SRT_UDPSEND_SET_NEXT_PRIORITY) {
            if (op.slot < c.n_hosts) c.hosts[op.slot].next_priority = op.value;
        } else if (op.slot < c.n_sockets) {
            apply_op(c, c.socks[op.slot], op);
        }
    }
}

inline void host_run(const Ctx &c) {
    preset_words(c);
    for (uint32_t i = 0; i < c.n_calls; ++i) preset_call(c, i);
    for (uint32_t x = 0; x < c.n_sockets; ++x) c.first_writable[x] = NONE;
    for (uint32_t h = 0; h < c.n_hosts; ++h) {
        Run<false> r(c, h);
        r.run();
    }
}

}  // namespace udps
#endif
