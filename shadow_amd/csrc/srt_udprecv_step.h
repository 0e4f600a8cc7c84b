// srt_udprecv_step.h -- a UDP socket's receive side for one window
// (host/descriptor/socket/inet/udp.rs:108-168 push_in_packet, :477-572 recvmsg,
// :900-925 SO_RCVBUF, :1056-1134 MessageBuffer), written once for the host and
// the device (srt_udprecv.hip compiles it for both, tests/asan/udprecv_check.cpp
// for the host alone).
//
// One socket slot is one sequential walk.  Its state (Sock, 88 bytes) is held in
// registers from the first event of the call to the last.  Its events are the
// delivery records of its host's sub-span whose slot is its own (pushes, at
// forward_ns, in list order) and the reads of its host's sub-span whose slot is
// its own, merged by time, pushes first at equal times.  A walk re-reads its
// host's whole sub-span to pick its own events out; the spans come through a
// window (Win): LDS on the device when the wave's hosts fit, device memory
// otherwise, plain arrays on the host.
//
// The queue of a socket inside a call is virtual: the messages earlier calls left
// in its ring (`carry`, read from the ring at its head) followed by the records
// buffered in this call and not yet read, which stay where they are: a push marks
// its staged record K_BUF, a second cursor (q) follows the marks.  Only what is
// still buffered when the walk ends is written to the ring, so a message pushed
// and read inside the call never touches it.
//
// The blocked read (SRT_UDP_WAIT): armed when it finds the queue empty, completed
// at the first instant t at which a message is buffered -- before the next event
// that is a read, or a push later than t, or the end of the walk -- and reported
// in d_results when it was armed in this call, else appended to d_late.
//
// Every write is preceded by its range check: the sub-spans are clamped to the
// window, the late list to late_cap, the ring to ring_cap.
#ifndef SRT_UDPRECV_STEP_H
#define SRT_UDPRECV_STEP_H

#include <stdint.h>

#include "../../include/srt.h"

#include "srt_relay_common.h"

namespace udprecv {

using relay::NONE;
using relay::raise;
using relay::segment;
using relay::take_slot;

constexpr uint32_t F_RING_OVERFLOW = SRT_UDPRECV_RING_OVERFLOW, F_LATE_OVERFLOW = SRT_UDPRECV_LATE_OVERFLOW,
                   F_NOTE_OVERRUN = SRT_UDPRECV_NOTE_OVERRUN, F_BAD_SOCKET = SRT_UDPRECV_BAD_SOCKET,
                   F_READ_ORDER = SRT_UDPRECV_READ_ORDER, F_ARMED_TWICE = SRT_UDPRECV_ARMED_TWICE;
constexpr uint32_t NO_SOCKET = 0xffffffffu, NO_READ = 0xffffffffu;
constexpr uint32_t PROCESSED = SRT_PDS_RCV_SOCKET_PROCESSED, DROPPED = SRT_PDS_RCV_SOCKET_DROPPED,
                   BUFFERED = SRT_PDS_RCV_SOCKET_BUFFERED;
constexpr int64_t E_WOULDBLOCK = -11, E_BADF = -9;
constexpr uint64_t RCVBUF_MIN = 2048, RCVBUF_MAX = 1ull << 28;  // udp.rs:916, :921

// a staged record's kind
constexpr uint16_t K_NONE = 0;  // not this stage's (slot is NO_SOCKET)
constexpr uint16_t K_PUSH = 1;  // a push, its meta gathered
constexpr uint16_t K_MISS = 2;  // a push whose tag the note ring does not hold
constexpr uint16_t K_BUF = 3;   // pushed and buffered in this call (set by the slot's walk)

// the words a call leaves behind, 32 bytes
struct State {
    uint32_t flags;  // SRT_UDPRECV_* bits since the last status call
    uint32_t pad;
    uint64_t n_proc, n_buf, n_drop;  // since create, summed from the slots' by status
};

// a socket slot, 88 bytes
struct Sock {
    uint64_t len_bytes, soft_limit, last_read_recv_ns, armed_seq;
    uint64_t n_proc, n_buf, n_drop;  // packets since create
    uint32_t armed_len, armed_flags, armed_user;  // the blocked read
    uint32_t ring_head, n_msgs;                   // the messages buffered across calls
    uint32_t peer_ip;
    uint32_t host;  // the slot's owner, fixed at create
    uint16_t peer_port;
    uint8_t open, overflow;
};

// a buffered message, 32 bytes
struct Msg {
    uint64_t tag, recv_ns;
    uint32_t size, src_ip, user;
    uint16_t src_port, pad;
};

// a delivery record as the walks read it, 32 bytes, in list order
struct Rec {
    uint64_t forward_ns;
    uint32_t slot;  // NO_SOCKET: passes through
    uint32_t size, src_ip, user;
    uint16_t src_port, kind;
    uint32_t status;  // deliver's
};

struct Ctx {
    State *st;
    Sock *socks;        // [n_sockets]
    Msg *ring;          // [n_sockets * ring_cap]
    Rec *rec;           // [out_cap]
    srt_udp_meta *note_ring;
    uint64_t note_cap, note_end, note_end_mod;  // note_end % note_cap (0 without a ring)
    uint32_t n_hosts, n_sockets, ring_cap;
    uint32_t win_bytes;  // the bytes of records and reads a wave holds in LDS
    // note
    const srt_udp_meta *note_in;
    uint64_t note_first_mod;
    uint32_t note_first, note_n;
    // config
    const srt_udprecv_op *ops;
    uint32_t n_ops;
    // run
    uint32_t n_reads, late_cap;
    const uint32_t *out_host_ptr, *out_socket, *out_status;
    const uint64_t *out_forward, *out_tag;
    uint64_t out_cap;
    const uint32_t *read_host_ptr;  // nullptr: no reads
    const srt_udp_read *reads;
    uint64_t read_seq_base, prev_until, until;
    uint32_t *rx_status;
    srt_udp_result *results;
    srt_udp_late *late;
    uint32_t *late_count;
    uint64_t *first_readable;
};

// ---- the note ring (srt_deliver's rule)
SRT_HD void note_store(const Ctx &c, uint32_t i) {
    if (i < c.note_first || i >= c.note_n) return;
    uint64_t s = c.note_first_mod + (i - c.note_first);  // below 2 * note_cap
    if (s >= c.note_cap) s -= c.note_cap;
    c.note_ring[s] = c.note_in[i];
}

SRT_HD bool note_read(const Ctx &c, uint64_t tag, srt_udp_meta &m) {
    const uint64_t a = c.note_end - tag;
    if (tag >= c.note_end || a > c.note_cap) return false;
    m = c.note_ring[c.note_end_mod >= a ? c.note_end_mod - a : c.note_end_mod + (c.note_cap - a)];
    return true;
}

// ---- configuration
SRT_HD uint64_t rcvbuf_limit(uint64_t optval) {  // udp.rs:910-924, the doubling saturating
    if (optval >= RCVBUF_MAX / 2) return RCVBUF_MAX;
    return optval * 2 > RCVBUF_MIN ? optval * 2 : RCVBUF_MIN;
}

SRT_HD void sock_reset(Sock &s, uint64_t limit, uint8_t open) {
    s.len_bytes = 0;
    s.soft_limit = limit;
    s.last_read_recv_ns = s.armed_seq = NONE;
    s.armed_len = s.armed_flags = s.armed_user = 0;
    s.ring_head = s.n_msgs = 0;
    s.peer_ip = 0;
    s.peer_port = 0;
    s.open = open;
    s.overflow = 0;
}

SRT_HD void apply_op(Sock &s, const srt_udprecv_op &op) {
    if (op.op == SRT_UDPRECV_OPEN) {
        sock_reset(s, op.value, 1);
    } else if (!s.open) {
        return;
    } else if (op.op == SRT_UDPRECV_CLOSE) {
        sock_reset(s, 0, 0);
    } else if (op.op == SRT_UDPRECV_SET_PEER) {
        s.peer_ip = (uint32_t)op.value;
        s.peer_port = (uint16_t)(op.value >> 32);
    } else if (op.op == SRT_UDPRECV_SET_RCVBUF) {
        s.soft_limit = rcvbuf_limit(op.value);
    }
}

// step i of a list sorted stably by slot: the first step of a slot applies the slot's run
SRT_HD void config_at(const Ctx &c, uint32_t i) {
    const uint32_t slot = c.ops[i].slot;
    if (slot >= c.n_sockets || (i && c.ops[i - 1].slot == slot)) return;
    Sock s = c.socks[slot];
    for (uint32_t k = i; k < c.n_ops && c.ops[k].slot == slot; ++k) apply_op(s, c.ops[k]);
    c.socks[slot] = s;
}

// ---- the stage pass
SRT_HD uint32_t walked(const Ctx &c) {
    return c.out_host_ptr[c.n_hosts] < c.out_cap ? c.out_host_ptr[c.n_hosts] : (uint32_t)c.out_cap;
}

SRT_HD uint32_t reads_walked(const Ctx &c) {
    if (!c.read_host_ptr) return 0;
    return c.read_host_ptr[c.n_hosts] < c.n_reads ? c.read_host_ptr[c.n_hosts] : c.n_reads;
}

// delivery record k < walked: its status copied, its staged record
SRT_HD void stage_record(const Ctx &c, uint32_t k) {
    const uint32_t status = c.out_status[k], sock = c.out_socket[k];
    c.rx_status[k] = status;
    Rec r;
    r.forward_ns = c.out_forward[k];
    r.slot = NO_SOCKET;
    r.size = r.src_ip = r.user = 0;
    r.src_port = 0;
    r.kind = K_NONE;
    r.status = status;
    if ((status & SRT_PDS_RCV_INTERFACE_RECEIVED) && sock < c.n_sockets && c.socks[sock].open) {
        r.slot = sock;
        srt_udp_meta m;
        if (note_read(c, c.out_tag[k], m)) {
            r.kind = K_PUSH;
            r.size = m.payload_size;
            r.src_ip = m.src_ip_be;
            r.src_port = m.src_port_be;
            r.user = m.user;
        } else {
            r.kind = K_MISS;
        }
    }
    c.rec[k] = r;
}

SRT_HD srt_udp_result no_result() {
    srt_udp_result z;
    z.tag = z.recv_ns = z.complete_ns = 0;
    z.return_val = 0;
    z.status = SRT_UDP_NOT_TAKEN;
    z.msg_flags = z.src_ip_be = 0;
    z.src_port_be = z.reserved = 0;
    z.user = z.read_user = 0;
    return z;
}

// read r < n_reads: its result preset; a read below rlim whose slot no walk owns is answered here
SRT_HD void stage_read(const Ctx &c, uint32_t r, uint32_t rlim) {
    srt_udp_result res = no_result();
    if (r < rlim) {
        const srt_udp_read rd = c.reads[r];
        // the read's host: the last h with read_host_ptr[h] <= r
        uint32_t lo = 0, hi = c.n_hosts;  // the answer lies in [lo, hi)
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (c.read_host_ptr[mid] <= r) lo = mid;
            else hi = mid;
        }
        bool bad = rd.slot >= c.n_sockets || !c.n_hosts;
        if (!bad) {
            const Sock &s = c.socks[rd.slot];
            bad = !s.open || s.host != lo;
        }
        if (bad) {
            raise(&c.st->flags, F_BAD_SOCKET);
            res.status = SRT_UDP_DONE;
            res.return_val = E_BADF;
            res.complete_ns = rd.time_ns;
            res.read_user = rd.user;
        }
    }
    c.results[r] = res;
}

// ---- the window a walk reads its host's sub-spans through
struct Win {
    Rec *rec;                 // record k at rec[k - rec0], k in [rec0, rec1)
    const srt_udp_read *rd;   // read j at rd[j - rd0], j in [rd0, rd1)
    uint32_t rec0, rec1, rd0, rd1;
};

SRT_HD uint32_t clampu(uint32_t v, uint32_t lo, uint32_t hi) { return v < lo ? lo : v > hi ? hi : v; }

// ---- one socket slot's walk
struct Walk {
    const Ctx &c;
    const Win &w;
    const uint32_t slot;
    Sock s;
    uint64_t first = NONE;    // the first empty -> non-empty transition
    uint64_t t_ready;         // when the queue last turned non-empty
    uint32_t carry;           // messages still in the ring, from its head
    uint32_t inwin = 0;       // buffered in this call, not yet read
    uint32_t q;               // at or before the oldest of them
    uint32_t e;               // the end of the host's records
    uint32_t armed_idx = NO_READ;  // the read armed in this call

    SRT_HD Walk(const Ctx &c_, const Win &w_, uint32_t slot_) : c(c_), w(w_), slot(slot_) {}

    SRT_HD Rec &rec(uint32_t k) const { return w.rec[k - w.rec0]; }
    SRT_HD const srt_udp_read &rd(uint32_t j) const { return w.rd[j - w.rd0]; }
    SRT_HD uint32_t n_msgs() const { return carry + inwin; }
    SRT_HD Msg *ring() const { return c.ring + (size_t)slot * c.ring_cap; }

    // the oldest message buffered in this call and not yet read; inwin > 0
    SRT_HD Msg front_here() {
        while (q < e && !(rec(q).slot == slot && rec(q).kind == K_BUF)) ++q;
        Msg m;
        m.tag = m.recv_ns = 0;
        m.size = m.src_ip = m.user = 0;
        m.src_port = m.pad = 0;
        if (q < e) {  // always: inwin counts the marks from q on
            const Rec r = rec(q);
            m.tag = c.out_tag[q];
            m.recv_ns = r.forward_ns;
            m.size = r.size;
            m.src_ip = r.src_ip;
            m.user = r.user;
            m.src_port = r.src_port;
        }
        return m;
    }

    // the front message; n_msgs() > 0
    SRT_HD Msg front() { return carry ? ring()[s.ring_head] : front_here(); }

    SRT_HD void pop() {
        if (carry) {
            --carry;
            s.ring_head = s.ring_head + 1 == c.ring_cap ? 0 : s.ring_head + 1;
        } else {
            ++q;
            --inwin;
        }
    }

    // recvmsg on a non-empty queue (udp.rs:502-545)
    SRT_HD srt_udp_result take(uint32_t len, uint32_t flags, uint64_t at, uint32_t read_user) {
        const Msg m = front();
        if (!(flags & SRT_UDP_PEEK)) {
            pop();
            s.len_bytes -= m.size;
        }
        const uint32_t copied = len < m.size ? len : m.size;
        srt_udp_result res;
        res.tag = m.tag;
        res.recv_ns = m.recv_ns;
        res.complete_ns = at;
        res.return_val = (flags & SRT_UDP_TRUNC) ? m.size : copied;
        res.status = SRT_UDP_DONE;
        res.msg_flags = copied < m.size ? SRT_UDP_MSG_TRUNC : 0;
        res.src_ip_be = m.src_ip;
        res.src_port_be = m.src_port;
        res.reserved = 0;
        res.user = m.user;
        res.read_user = read_user;
        s.last_read_recv_ns = m.recv_ns;
        return res;
    }

    // the blocked read returns at t_ready
    SRT_HD void complete() {
        const srt_udp_result res = take(s.armed_len, s.armed_flags, t_ready, s.armed_user);
        if (armed_idx != NO_READ) {
            c.results[armed_idx] = res;
        } else {
            const uint32_t k = take_slot(c.late_count);
            if (k < c.late_cap) {
                srt_udp_late l;
                l.seq = s.armed_seq;
                l.result = res;
                c.late[k] = l;
            } else {
                raise(&c.st->flags, F_LATE_OVERFLOW);
            }
        }
        s.armed_seq = NONE;
        s.armed_len = s.armed_flags = s.armed_user = 0;
        armed_idx = NO_READ;
    }

    // push_in_packet (udp.rs:108-168) for record k
    SRT_HD void push(uint32_t k) {
        const Rec r = rec(k);
        if (r.kind == K_MISS) {
            raise(&c.st->flags, F_NOTE_OVERRUN);
            s.overflow |= SRT_UDPRECV_MARK_NOTE;
            return;
        }
        uint32_t bits = PROCESSED;
        ++s.n_proc;
        if ((s.peer_ip || s.peer_port) && (r.src_ip != s.peer_ip || r.src_port != s.peer_port)) {
            bits |= DROPPED;
            ++s.n_drop;
        } else if (!(s.len_bytes < s.soft_limit)) {
            bits |= DROPPED;
            ++s.n_drop;
        } else {
            bits |= BUFFERED;
            ++s.n_buf;
            s.len_bytes += r.size;
            if (!n_msgs()) {
                t_ready = r.forward_ns;
                if (first == NONE) first = r.forward_ns;
            }
            ++inwin;
            rec(k).kind = K_BUF;
        }
        c.rx_status[k] = r.status | bits;
    }

    // recvmsg (udp.rs:477-572) for read j, which is in order
    SRT_HD void read(uint32_t j) {
        const srt_udp_read r = rd(j);
        if (n_msgs()) {
            c.results[j] = take(r.len, r.flags, r.time_ns, r.user);
            return;
        }
        srt_udp_result res = no_result();
        res.read_user = r.user;
        if ((r.flags & SRT_UDP_WAIT) && s.armed_seq == NONE) {
            s.armed_seq = c.read_seq_base + j;
            s.armed_len = r.len;
            s.armed_flags = r.flags;
            s.armed_user = r.user;
            armed_idx = j;
            res.status = SRT_UDP_ARMED;
        } else {
            if (r.flags & SRT_UDP_WAIT) raise(&c.st->flags, F_ARMED_TWICE);
            res.status = SRT_UDP_DONE;
            res.return_val = E_WOULDBLOCK;
            res.complete_ns = r.time_ns;
        }
        c.results[j] = res;
    }

    SRT_HD void run(uint32_t lim, uint32_t rlim) {
        s = c.socks[slot];
        if (s.open) {
            uint32_t i, j = 0, re = 0;
            segment(c.out_host_ptr, lim, s.host, i, e);
            i = clampu(i, w.rec0, w.rec1), e = clampu(e, i, w.rec1);
            if (c.read_host_ptr) {
                segment(c.read_host_ptr, rlim, s.host, j, re);
                j = clampu(j, w.rd0, w.rd1), re = clampu(re, j, w.rd1);
            }
            q = i;
            carry = s.n_msgs;
            t_ready = c.prev_until;
            uint64_t rmax = 0;  // the largest time of the host's earlier reads that lie in the window
            for (;;) {
                while (i < e && rec(i).slot != slot) ++i;
                bool in_win = false, in_order = false;
                uint64_t rt = 0;
                while (j < re) {
                    const srt_udp_read &r = rd(j);
                    rt = r.time_ns;
                    in_win = rt >= c.prev_until && rt < c.until;
                    if (r.slot == slot) {
                        in_order = in_win && rt >= rmax;
                        break;
                    }
                    if (in_win && rt > rmax) rmax = rt;
                    ++j;
                }
                const bool have_rec = i < e, have_rd = j < re;
                if (!have_rec && !have_rd) break;
                if (have_rd && !in_order) {
                    raise(&c.st->flags, F_READ_ORDER);
                    if (in_win && rt > rmax) rmax = rt;
                    ++j;
                    continue;
                }
                const uint64_t ft = have_rec ? rec(i).forward_ns : 0;
                if (have_rec && (!have_rd || ft <= rt)) {
                    if (s.armed_seq != NONE && n_msgs() && ft > t_ready) complete();
                    push(i);
                    ++i;
                } else {
                    if (s.armed_seq != NONE && n_msgs()) complete();
                    read(j);
                    if (rt > rmax) rmax = rt;
                    ++j;
                }
            }
            if (s.armed_seq != NONE && n_msgs()) complete();
            // what is still buffered joins the ring behind the messages carried
            uint32_t n = carry;
            while (inwin) {
                const Msg m = front_here();
                if (n < c.ring_cap) {
                    const uint32_t at = s.ring_head + n;  // below 2 * ring_cap
                    ring()[at >= c.ring_cap ? at - c.ring_cap : at] = m;
                    ++n;
                } else {
                    raise(&c.st->flags, F_RING_OVERFLOW);
                    s.overflow |= SRT_UDPRECV_MARK_RING;
                }
                ++q;
                --inwin;
            }
            s.n_msgs = n;
            c.socks[slot] = s;
        }
        c.first_readable[slot] = first;
    }
};

// ---- the host-only form: the same step, one record, one slot after the other
inline void host_note(const Ctx &c) {
    for (uint32_t i = c.note_first; i < c.note_n; ++i) note_store(c, i);
}

inline void host_config(const Ctx &c) {
    for (uint32_t i = 0; i < c.n_ops; ++i)
        if (c.ops[i].slot < c.n_sockets) apply_op(c.socks[c.ops[i].slot], c.ops[i]);
}

inline void host_run(const Ctx &c) {
    const uint32_t lim = walked(c), rlim = reads_walked(c);
    *c.late_count = 0;
    for (uint32_t k = 0; k < lim; ++k) stage_record(c, k);
    for (uint32_t r = 0; r < c.n_reads; ++r) stage_read(c, r, rlim);
    const Win w{c.rec, c.reads, 0, lim, 0, rlim};
    for (uint32_t slot = 0; slot < c.n_sockets; ++slot) {
        Walk wk(c, w, slot);
        wk.run(lim, rlim);
    }
}

}  // namespace udprecv
#endif
