// srt_outbound_step.h -- one source host's outbound relay stage, written once
// for the host and the device (srt_outbound.hip compiles it for both).
//
// Reference:
//   notify         host/host.rs:988-1002 (notify_socket_has_packets) ->
//                  networkinterface_wantsSend (host/network/network_interface.c:
//                  344-370: the socket joins the qdisc unless it is in it) and
//                  Relay::notify (network/relay/mod.rs:110-135)
//   pop            network_interface.c:205-340 over
//                  network_queuing_disciplines.c: FIFO = the socket whose next
//                  packet has the smallest priority, RR = the head of a plain
//                  queue; the socket is put back while it has data
//   Relay          relay/mod.rs:200-272 (forward_until_blocked: the cached
//                  next_packet first, is_local and bootstrap exempt from the
//                  bucket) with the TokenBucket of srt_relay_common.h
//   event order    at equal times every arrival runs before the forward task
//
// Store.  A host's unresolved packets are its ring in HBM (carried over from
// earlier calls, compacted in arrival order) and the records of this call's
// batch.  An element is named by a u32: RING_BIT | ring position, or the batch
// index.  Every element has a u32 link, "next packet of my socket": in the ring
// record, or, for a batch packet, in the reserved word of the wave's LDS copy
// (device, span staged) or in a link array in HBM.  A packet that left its
// socket has its link set to GONE, which is how the end of the call finds the
// survivors.  Each (host, socket) has an 8-byte head / tail cursor; the
// qdisc's sockets are an array of at most max_sockets ids per host: a circular
// queue for RR, a set scanned for the smallest head priority for FIFO.  At the
// end of a call the survivors (ring first, then this call's) are written back
// to the ring compacted in arrival order and the cursors and links rebuilt on
// the new positions.  Every ring and queue write is preceded by its capacity
// check.
#ifndef SRT_OUTBOUND_STEP_H
#define SRT_OUTBOUND_STEP_H

#include <stdint.h>

#include "../../include/srt.h"

#include "srt_relay_common.h"

namespace outb {

using relay::add_pending;
using relay::NONE;
using relay::raise;
using relay::sat_add;
using relay::take_slot;

constexpr uint32_t F_RING_OVERFLOW = 1, F_LATE_OVERFLOW = 2, F_TIME_REGRESSION = 4, F_OVERSIZE = 8,
                   F_AFTER_UNTIL = 16, F_BAD_SOCKET = 32;

constexpr uint32_t RING_BIT = 0x80000000u;  // element name: a ring position
constexpr uint32_t NIL = 0xffffffffu;       // no element
constexpr uint32_t GONE = 0xfffffffeu;      // link of an element that left its socket

// Device: the workgroup's LDS, one wave's: [0, WIN_CAP) staged batch packets, then the cursors
// and the socket queues of its 64 hosts when max_sockets <= CUR_LDS (named through the shared
// symbol, not through pointers kept in the run, so that they are LDS instructions whose waits
// do not cover the outstanding stores to HBM)
constexpr uint32_t WIN_CAP = 2048;  // packets a wave may stage (64 KB)
constexpr uint32_t CUR_LDS = 16;    // sockets a host may have for the wave's cursors to sit in LDS (12 KB)
constexpr uint32_t LDS_CUR_OFF = WIN_CAP * 32, LDS_Q_OFF = LDS_CUR_OFF + 64 * CUR_LDS * 8;
constexpr uint32_t LDS_BYTES = LDS_Q_OFF + 64 * CUR_LDS * 4;
#if defined(__HIPCC__)
extern __shared__ __align__(16) unsigned char outb_lds[];
#endif

// a batch packet as the step reads it; in LDS the reserved word is the link
struct alignas(16) Rec {
    uint64_t ready;
    uint64_t prio;
    uint32_t size;
    uint32_t socket;
    uint32_t flags;
    uint32_t link;
};

struct alignas(16) RingEl {
    uint64_t seq;
    uint64_t prio;
    uint32_t size;
    uint32_t socket;
    uint32_t flags;
    uint32_t link;
};

struct Cur {
    uint32_t head, tail;
};

// per-host state, 96 bytes
struct alignas(16) Host {
    uint64_t balance, last_refill, refill, capacity;  // TokenBucket
    uint64_t task_ns;  // pending forward task (NONE: relay Idle)
    uint64_t tasks;    // forward tasks scheduled so far (event ids consumed)
    uint64_t sent;     // non-local packets forwarded so far: the next rank
    uint64_t cached_seq;
    uint32_t ring_len;  // packets in the socket queues (all in the ring between calls)
    uint32_t cached, cached_size;
    uint32_t overflow;
    uint32_t q_head, q_len;  // the qdisc's sockets: q[(q_head + k) % max_sockets], k < q_len
    uint32_t pad[2];
};

// the seq of the packet the relay holds cached between calls (srt_outbound_cached_seq)
SRT_HD uint64_t cached_seq_of(const Host &s) { return s.cached ? s.cached_seq : NONE; }

struct Ctx {
    Host *hosts;
    RingEl *ring;
    Cur *cur;        // [host][socket]
    uint32_t *sockq;  // [host][max_sockets]
    const srt_out_pkt *pkts;
    uint32_t *link;  // [n_pkts], for spans that are not staged in LDS
    const uint32_t *host_ptr;
    uint32_t *status;
    uint64_t *send_ns;
    uint64_t *send_rank;
    srt_outbound_late *late;
    uint32_t *late_count;
    uint32_t *flags;
    unsigned long long *pending;
    uint64_t base, until, boot_end, prev_until;
    uint32_t n_hosts, ring_cap, late_cap, n_pkts;
    uint32_t max_sockets, qdisc;
    uint32_t pad[2];
};

// one host's run over one call
// WIN: the wave staged its span of the batch in LDS; CL: and its hosts' cursors and socket queues
template <bool WIN, bool CL = false>
struct Run {
    Host s;
    const Ctx c;  // by value: a reference member would keep the whole object in private memory
    uint32_t h;
    uint32_t win0, win_n;  // device: batch packets [win0, win0 + win_n) are held in LDS by the wave
    Rec *win;              // that window, in a host build (tests)
    uint32_t ring0;   // ring_len at the start of the call: ring positions below it are live names
    uint32_t budget;  // pops left: the packets the host can hold this call
    uint32_t lo, ppos;  // batch packets [lo, ppos) have arrived: the batch indices that are live names

    SRT_HD Run(const Ctx &ctx, uint32_t host)
        : s(ctx.hosts[host]), c(ctx), h(host), win0(0), win_n(0), win(nullptr), ring0(0), budget(0), lo(0),
          ppos(0) {}

    SRT_HD Rec *wbase() const {
#if defined(__HIP_DEVICE_COMPILE__)
        return reinterpret_cast<Rec *>(outb_lds);
#else
        return win;
#endif
    }
    // this host's cursors and socket queue: HBM, or the wave's LDS copy (lane = host % 64)
    SRT_HD Cur *cbase() const {
#if defined(__HIP_DEVICE_COMPILE__)
        if (CL) return reinterpret_cast<Cur *>(outb_lds + LDS_CUR_OFF) + (h & 63u) * c.max_sockets;
#endif
        return c.cur + (uint64_t)h * c.max_sockets;
    }
    SRT_HD uint32_t *qbase() const {
#if defined(__HIP_DEVICE_COMPILE__)
        if (CL) return reinterpret_cast<uint32_t *>(outb_lds + LDS_Q_OFF) + (h & 63u) * c.max_sockets;
#endif
        return c.sockq + (uint64_t)h * c.max_sockets;
    }

    SRT_HD RingEl *ring_at(uint32_t x) const { return c.ring + ((uint64_t)h * c.ring_cap + (x & ~RING_BIT)); }

    SRT_HD Rec rec_at(uint32_t i) const {
        if (WIN) return wbase()[i - win0];
        const srt_out_pkt p = c.pkts[i];
        Rec r;
        r.ready = p.ready_ns, r.prio = p.priority, r.size = p.total_size, r.socket = p.socket, r.flags = p.flags;
        r.link = NIL;
        return r;
    }

    // x names an element of this host: every dereference of a stored name is preceded by this
    // check (the names are the step's own, so it fails only on a host already marked invalid)
    SRT_HD bool live(uint32_t x) const { return x & RING_BIT ? (x ^ RING_BIT) < ring0 : x >= lo && x < ppos; }

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

    SRT_HD uint32_t link_get(uint32_t x) const {
        if (x & RING_BIT) return from_ring(ring_at(x)->link);
        return WIN ? wbase()[x - win0].link : c.link[x];
    }
    SRT_HD void link_set(uint32_t x, uint32_t v) const {
        if (x & RING_BIT) ring_at(x)->link = v;
        else if (WIN) wbase()[x - win0].link = v;
        else c.link[x] = v;
    }
    SRT_HD uint64_t prio_of(uint32_t x) const {
        if (x & RING_BIT) return from_ring(ring_at(x)->prio);
        return WIN ? wbase()[x - win0].prio : c.pkts[x].priority;
    }
    // arrival order of two live elements: the ring's before the batch's, each in position order
    SRT_HD static uint32_t arrival_key(uint32_t x) { return x ^ RING_BIT; }

    SRT_HD uint32_t q_slot(uint32_t k) const {
        const uint32_t p = s.q_head + k;  // both below max_sockets (< 2^31)
        return p >= c.max_sockets ? p - c.max_sockets : p;
    }
    SRT_HD void q_push(uint32_t sock) {
        if (s.q_len < c.max_sockets) qbase()[q_slot(s.q_len++)] = sock;
    }

    // a packet leaves the stage: batch packets by index, older ones to the late list
    SRT_HD void resolve(uint64_t seq, uint32_t status, uint64_t now, uint64_t rank) {
        if (seq >= c.base) {
            const uint64_t i = seq - c.base;
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
                raise(c.flags, F_LATE_OVERFLOW);
            }
        }
    }

    // the socket-has-data event of batch packet i: the packet joins its socket's FIFO, the
    // socket the qdisc unless it is in it (a socket is in the qdisc iff it has data)
    SRT_HD void arrive(uint32_t i, uint32_t sock) {
        Cur cu = cbase()[sock];
        link_set(i, NIL);
        if (!live(cu.head) || !live(cu.tail)) {
            cu.head = cu.tail = i;
            q_push(sock);
        } else {
            link_set(cu.tail, i);
            cu.tail = i;
        }
        cbase()[sock] = cu;
        ++s.ring_len;
    }

    // networkinterface_pop: the next packet of the qdisc's choice; false: no socket has data
    SRT_HD bool pop(uint64_t &seq, uint32_t &size, uint32_t &flags) {
        if (!s.q_len) return false;
        if (!budget) {
            // more pops than packets: only host_ptr[] groups that overlap (a caller
            // error) can link a socket into a cycle; the host is marked and stops
            if (!s.overflow) {
                s.overflow = 1;
                raise(c.flags, F_RING_OVERFLOW);
            }
            for (uint32_t k = 0; k < s.q_len; ++k) {
                Cur nil;
                nil.head = nil.tail = NIL;
                cbase()[qbase()[q_slot(k)]] = nil;
            }
            s.q_len = 0;
            s.ring_len = 0;
            return false;
        }
        --budget;
        for (;;) {
            if (!s.q_len) return false;
            uint32_t k = 0;
            if (c.qdisc == SRT_QDISC_FIFO) {
                uint64_t best = 0;
                uint32_t best_x = NIL;
                for (uint32_t j = 0; j < s.q_len; ++j) {
                    const uint32_t x = cbase()[qbase()[q_slot(j)]].head;
                    if (!live(x)) continue;
                    const uint64_t p = prio_of(x);
                    if (best_x == NIL || p < best || (p == best && arrival_key(x) < arrival_key(best_x)))
                        best = p, best_x = x, k = j;
                }
            }
            const uint32_t sock = qbase()[q_slot(k)];
            Cur cu = cbase()[sock];
            const uint32_t x = cu.head;
            uint32_t nx = NIL;
            const bool ok = live(x);
            if (ok) {
                nx = link_get(x);
                link_set(x, GONE);
                if (!live(nx)) nx = NIL;
            }
            cu.head = nx;
            if (nx == NIL) cu.tail = NIL;
            cbase()[sock] = cu;
            // the socket leaves the queue; with data left it goes back (RR: to the tail)
            if (c.qdisc == SRT_QDISC_FIFO) {
                if (nx == NIL) qbase()[q_slot(k)] = qbase()[q_slot(--s.q_len)];
            } else {
                s.q_head = q_slot(1);
                --s.q_len;
                if (nx != NIL) q_push(sock);
            }
            if (!ok) continue;  // only on a host whose ring overflowed: a socket that lost its packets
            --s.ring_len;
            if (x & RING_BIT) {
                const RingEl e = *ring_at(x);
                seq = e.seq, size = e.size, flags = e.flags;
            } else {
                const Rec r = rec_at(x);
                seq = c.base + x, size = r.size, flags = r.flags;
            }
            return true;
        }
    }

    // Relay::forward_until_blocked (relay/mod.rs:200-272) at the task's time
    SRT_HD void forward_task() {
        const uint64_t now = s.task_ns;
        s.task_ns = NONE;
        for (;;) {
            uint64_t seq;
            uint32_t size, flags = 0;
            uint32_t st = SRT_PDS_SND_INTERFACE_SENT | SRT_PDS_RELAY_FORWARDED;
            if (s.cached) {
                seq = s.cached_seq;
                size = s.cached_size;
                s.cached = 0;
                st |= SRT_PDS_RELAY_CACHED;
            } else if (!pop(seq, size, flags)) {
                return;  // Idle
            }
            if (flags & SRT_OUT_LOCAL) {  // pushed back into the interface: no tokens, no rank
                resolve(seq, st, now, NONE);
                continue;
            }
            uint64_t wait = 0;
            if (now >= c.boot_end &&
                !relay::bucket_remove(s.balance, s.last_refill, s.refill, s.capacity, size, now, wait)) {
                s.cached = 1;
                s.cached_seq = seq;
                s.cached_size = size;
                s.task_ns = sat_add(now, wait);
                if (size > s.capacity) {
                    // the bucket can never hold this packet (the reference would
                    // reschedule for ever): flagged, and at most one try a call
                    raise(c.flags, F_OVERSIZE);
                    if (s.task_ns < c.until) s.task_ns = c.until;
                }
                ++s.tasks;
                return;  // Pending
            }
            resolve(seq, st, now, s.sent++);
        }
    }

    // a survivor moves to ring position w (its capacity check first) and to the tail of its socket
    SRT_HD void keep(RingEl e, uint32_t &w) {
        if (w >= c.ring_cap) {
            if (!s.overflow) {
                s.overflow = 1;
                raise(c.flags, F_RING_OVERFLOW);
            }
            return;
        }
        Cur cu = cbase()[e.socket];
        e.link = NIL;
        c.ring[(uint64_t)h * c.ring_cap + w] = e;
        if (cu.head >= GONE || (cu.tail ^ RING_BIT) >= w) cu.head = RING_BIT | w;  // first of its socket
        else ring_at(cu.tail)->link = RING_BIT | w;
        cu.tail = RING_BIT | w;
        cbase()[e.socket] = cu;
        ++w;
    }

    SRT_HD void run() {
        // the group's bounds, held inside the batch whatever host_ptr[] says
        uint32_t lim = c.host_ptr[c.n_hosts] < c.n_pkts ? c.host_ptr[c.n_hosts] : c.n_pkts;
        if (WIN && lim > win0 + win_n) lim = win0 + win_n;  // and inside the window
        uint32_t b = c.host_ptr[h] < lim ? c.host_ptr[h] : lim;
        if (WIN && b < win0) b = win0;
        uint32_t e = c.host_ptr[h + 1] < lim ? c.host_ptr[h + 1] : lim;
        if (e < b) e = b;
        ring0 = s.ring_len;
        budget = ring0 + (e - b);
        lo = ppos = b;
        Rec nxt;
        nxt.ready = 0;
        if (ppos < e) nxt = rec_at(ppos);
        for (;;) {
            if (ppos < e && nxt.ready < c.until && nxt.ready <= s.task_ns) {
                // socket-has-data event: networkinterface_wantsSend + Relay::notify
                const Rec x = nxt;
                const uint32_t i = ppos++;
                if (ppos < e) nxt = rec_at(ppos);  // in flight while this one is handled
                if (x.socket >= c.max_sockets) {
                    raise(c.flags, F_BAD_SOCKET);  // not taken
                    link_set(i, GONE);
                    continue;
                }
                if (x.ready < c.prev_until) raise(c.flags, F_TIME_REGRESSION);
                arrive(i, x.socket);
                if (s.task_ns == NONE) {
                    s.task_ns = x.ready;
                    ++s.tasks;
                }
            } else if (s.task_ns < c.until) {
                forward_task();
            } else {
                break;
            }
        }
        // An arrival at or after until_ns belongs to a later window: it is not
        // taken, its status stays 0, and the call is flagged.
        if (ppos < e) raise(c.flags, F_AFTER_UNTIL);
        // The survivors go back to the ring compacted in arrival order, and the
        // cursors and links are rebuilt on their new positions.  A host with
        // nothing queued has every cursor NIL already and touches no ring.
        if (s.ring_len) {
            for (uint32_t k = 0; k < s.q_len; ++k) {
                Cur nil;
                nil.head = nil.tail = NIL;
                cbase()[qbase()[q_slot(k)]] = nil;
            }
            uint32_t w = 0;
            for (uint32_t p = 0; p < ring0; ++p) {  // w <= p: a position is read before it is written
                const RingEl el = *ring_at(RING_BIT | p);
                if (el.link != GONE) keep(el, w);
            }
            for (uint32_t i = b; i < ppos; ++i) {
                if (link_get(i) == GONE) continue;
                const Rec x = rec_at(i);
                RingEl el;
                el.seq = c.base + i, el.prio = x.prio, el.size = x.size, el.socket = x.socket, el.flags = x.flags;
                el.link = NIL;
                keep(el, w);
            }
            if (w != s.ring_len) {  // overflow: sockets that lost every packet leave the qdisc
                uint32_t n = 0;
                for (uint32_t k = 0; k < s.q_len; ++k) {
                    const uint32_t sock = qbase()[q_slot(k)];
                    if (cbase()[sock].head < GONE) qbase()[q_slot(n++)] = sock;
                }
                s.q_len = n;
            }
            s.ring_len = w;
        }
        if (s.cached && s.cached_seq >= c.base)
            c.status[s.cached_seq - c.base] = SRT_PDS_SND_INTERFACE_SENT | SRT_PDS_RELAY_CACHED;
        add_pending(c.pending, (unsigned long long)s.ring_len + s.cached);
        c.hosts[h] = s;
    }
};

}  // namespace outb
#endif
