// srt_flight_step.h -- the in-flight store between the event push of one round
// and the inbound stage of a later window, written once for the host and the
// device (srt_flight.hip compiles it for both).
//
// The store is one flat pool of records in structure-of-arrays form (deliver
// time, event id, tag: u64; source host, destination host, total size: u32; 36
// bytes a packet), twice: a pop reads one half and compacts the survivors into
// the other, so nothing is moved in place.  Which half is current, how far it
// is filled and the call-wide results live in State, in the memory the pool
// lives in.
//
// Push: a packet the send decision marked SENT (the test event_id_kernel
// applies) is appended at a place taken from State::len.  The counter may run
// past pool_cap: a place at or past it is not written, the packet is counted
// lost, and every reader takes min(len, pool_cap).
//
// Pop: the due set is deliver < until_ns.  Count the due packets per
// destination -- the count a packet finds is its slot in its destination's
// run, kept in `slot` -- scan the counts into w_dst_ptr, void the pop when the
// total is over out_cap, copy every due packet as one 32-byte record to
// stage[w_dst_ptr[dst] + slot] (any order within the run) and the survivors to
// the other half, then order each run by (deliver, source host, event id) -- a
// total order, event ids being unique per source host, so the output does not
// depend on the pool's order -- and write the window's arrays from it.
//
// Every write is preceded by its range check: place < pool_cap, position <
// out_cap, dst_host < n_dst_hosts.
#ifndef SRT_FLIGHT_STEP_H
#define SRT_FLIGHT_STEP_H

#include <stdint.h>

#include <algorithm>

#include "../../include/srt.h"

#include "srt_relay_common.h"

namespace flight {

using relay::raise;

constexpr uint32_t F_POOL_OVERFLOW = SRT_FLIGHT_POOL_OVERFLOW, F_OUT_OVERFLOW = SRT_FLIGHT_OUT_OVERFLOW,
                   F_BAD_HOST = SRT_FLIGHT_BAD_HOST, F_LATE_PUSH = SRT_FLIGHT_LATE_PUSH,
                   F_TIME_REGRESSION = SRT_FLIGHT_TIME_REGRESSION;

// the words a call leaves behind, 48 bytes
struct State {
    uint32_t flags;     // SRT_FLIGHT_* bits since the last status call
    uint32_t cur;       // the half pushes append to and the next pop reads
    uint32_t prev;      // the half the last pop read and its move copies from
    uint32_t is_void;   // the last pop was void
    uint64_t len;       // places handed out in the current half (may run past pool_cap)
    uint64_t prev_n;    // records the last pop walked
    uint64_t n_lost;    // packets not stored for want of room, since create
    uint64_t n_popped;  // the last pop's due count, void or not
};

// one half of the pool, or a caller's window arrays
struct Pool {
    uint64_t *deliver, *event_id, *tag;
    uint32_t *src, *dst, *size;
};

// a due packet on its way out, 32 bytes (its destination is the run it lies in)
struct Rec {
    uint64_t deliver, event_id, tag;
    uint32_t src, size;
};

struct Ctx {
    State *st;
    Pool pool;       // 2 * pool_cap records: half k begins at k * pool_cap
    uint32_t *cnt;   // [n_dst] due packets of the destination; all zero between calls
    uint32_t *slot;  // [pool_cap] a due packet's place within its destination's run
    Rec *stage;      // [pool_cap] the due packets, grouped by destination
    uint64_t pool_cap;
    uint32_t n_dst;
    uint32_t pre_flags;  // conditions the call itself found (TIME_REGRESSION)
    // push
    const uint32_t *host_ptr, *flags_in, *dst_in, *size_in;
    const uint64_t *deliver_in, *event_id_in, *tag_in;  // tag_in may be null: tag_base + batch index
    uint64_t tag_base, last_until;
    uint32_t n_src, n_pkts;
    // pop
    uint64_t until, out_cap;
    uint32_t *w_order, *w_dst_ptr;
    Pool w;
};

SRT_HD Pool half(const Ctx &c, uint32_t k) {
    const uint64_t o = (uint64_t)(k & 1u) * c.pool_cap;
    Pool p;
    p.deliver = c.pool.deliver + o, p.event_id = c.pool.event_id + o, p.tag = c.pool.tag + o;
    p.src = c.pool.src + o, p.dst = c.pool.dst + o, p.size = c.pool.size + o;
    return p;
}

SRT_HD uint64_t stored(const Ctx &c, uint64_t len) { return len < c.pool_cap ? len : c.pool_cap; }

// source host h's segment of the batch, held inside it whatever host_ptr[] says
SRT_HD void segment(const Ctx &c, uint32_t h, uint32_t &b, uint32_t &e) {
    relay::segment(c.host_ptr, relay::walked(c.host_ptr, c.n_src, c.n_pkts), h, b, e);
}

// would batch packet p go into the store?  (raises nothing: the device push counts with it first)
SRT_HD bool push_wants(const Ctx &c, uint32_t p) {
    return c.flags_in[p] == SRT_PDS_INET_SENT && c.dst_in[p] < c.n_dst;
}

// does batch packet p go into the store?  (raises BAD_HOST and LATE_PUSH)
SRT_HD bool push_takes(const Ctx &c, uint32_t p) {
    if (c.flags_in[p] != SRT_PDS_INET_SENT) return false;
    if (c.dst_in[p] >= c.n_dst) {
        raise(&c.st->flags, F_BAD_HOST);
        return false;
    }
    if (c.deliver_in[p] < c.last_until) raise(&c.st->flags, F_LATE_PUSH);
    return true;
}

// batch packet p of source host h at `place` of half `to`; false: no room
SRT_HD bool push_store(const Ctx &c, const Pool &to, uint64_t place, uint32_t h, uint32_t p) {
    if (place >= c.pool_cap) return false;
    to.deliver[place] = c.deliver_in[p];
    to.event_id[place] = c.event_id_in[p];
    to.tag[place] = c.tag_in ? c.tag_in[p] : c.tag_base + p;
    to.src[place] = h;
    to.dst[place] = c.dst_in[p];
    to.size[place] = c.size_in[p];
    return true;
}

SRT_HD void push_lost(const Ctx &c, uint64_t n) {
    if (!n) return;
    raise(&c.st->flags, F_POOL_OVERFLOW);
    relay::add_pending(reinterpret_cast<unsigned long long *>(&c.st->n_lost), n);
}

SRT_HD bool due(const Ctx &c, const Pool &from, uint64_t i) { return from.deliver[i] < c.until; }

// a due record joins its destination's count; the count it found is its slot
SRT_HD void count_due(const Ctx &c, const Pool &from, uint64_t i) {
    const uint32_t d = from.dst[i];
    if (d < c.n_dst) c.slot[i] = relay::take_slot(&c.cnt[d]);
}

// a due record goes to its place in its destination's run
SRT_HD void stage_due(const Ctx &c, const Pool &from, uint64_t i) {
    const uint32_t d = from.dst[i];
    if (d >= c.n_dst) return;
    const uint64_t pos = (uint64_t)c.w_dst_ptr[d] + c.slot[i];
    if (pos >= c.pool_cap) return;
    Rec r;
    r.deliver = from.deliver[i], r.event_id = from.event_id[i], r.tag = from.tag[i];
    r.src = from.src[i], r.size = from.size[i];
    c.stage[pos] = r;
}

// the end of the scan over the destinations: is the pop void, and the words it leaves
SRT_HD bool scan_end(const Ctx &c, uint64_t total) {
    State &s = *c.st;
    const bool is_void = total > c.out_cap;
    s.n_popped = total;
    s.is_void = is_void;
    if (c.pre_flags) raise(&s.flags, c.pre_flags);
    if (is_void) {
        raise(&s.flags, F_OUT_OVERFLOW);
    } else {
        s.prev_n = stored(c, s.len);
        s.prev = s.cur & 1u;
        s.cur = (s.cur & 1u) ^ 1u;
        s.len = 0;
    }
    return is_void;
}

// record i of `from` stays: to `place` of `to`
SRT_HD void keep(const Ctx &c, const Pool &from, const Pool &to, uint64_t i, uint64_t place) {
    if (place >= c.pool_cap) return;
    to.deliver[place] = from.deliver[i];
    to.event_id[place] = from.event_id[i];
    to.tag[place] = from.tag[i];
    to.src[place] = from.src[i];
    to.dst[place] = from.dst[i];
    to.size[place] = from.size[i];
}

// the pop order of core/work/event.rs:85-150: time, then source host id, then event id
struct Key {
    uint64_t deliver, event_id;
    uint32_t src;
};
SRT_HD Key key_of(const Rec &r) {
    Key k;
    k.deliver = r.deliver, k.event_id = r.event_id, k.src = r.src;
    return k;
}
SRT_HD bool before(const Key &a, const Key &b) {
    if (a.deliver != b.deliver) return a.deliver < b.deliver;
    if (a.src != b.src) return a.src < b.src;
    return a.event_id < b.event_id;
}
// a before b, with equal keys (a caller error) in staging order: ranks stay a permutation.  Without
// branches: the sort's inner loop runs it for every pair, and equal deliver times are the rule (the send
// decision clamps them to the round's end)
SRT_HD bool before_at(const Key &a, uint32_t ja, const Key &b, uint32_t jb) {
    const bool id = (a.event_id < b.event_id) | ((a.event_id == b.event_id) & (ja < jb));
    const bool host = (a.src < b.src) | ((a.src == b.src) & id);
    return (a.deliver < b.deliver) | ((a.deliver == b.deliver) & host);
}

// record r is number `pos` of the window
SRT_HD void emit(const Ctx &c, const Rec &r, uint64_t pos) {
    if (pos >= c.out_cap) return;
    c.w_order[pos] = (uint32_t)pos;
    c.w.deliver[pos] = r.deliver;
    c.w.size[pos] = r.size;
    c.w.src[pos] = r.src;
    c.w.event_id[pos] = r.event_id;
    c.w.tag[pos] = r.tag;
}

// ---- the host-only form: the same step, one packet after the other
inline void host_push(const Ctx &c) {
    const Pool to = half(c, c.st->cur);
    uint64_t lost = 0;
    for (uint32_t h = 0; h < c.n_src; ++h) {
        uint32_t b, e;
        segment(c, h, b, e);
        for (uint32_t i = b; i < e; ++i)
            if (push_takes(c, i) && !push_store(c, to, c.st->len++, h, i)) ++lost;
    }
    push_lost(c, lost);
}

inline void host_pop(const Ctx &c) {
    State &s = *c.st;
    {
        const Pool from = half(c, s.cur);
        const uint64_t n = stored(c, s.len);
        for (uint64_t i = 0; i < n; ++i)
            if (due(c, from, i)) count_due(c, from, i);
    }
    uint64_t total = 0;
    for (uint32_t d = 0; d < c.n_dst; ++d) {
        const uint32_t n = c.cnt[d];
        c.cnt[d] = 0;
        c.w_dst_ptr[d] = (uint32_t)total;
        total += n;
    }
    const bool is_void = scan_end(c, total);
    c.w_dst_ptr[c.n_dst] = (uint32_t)total;
    if (is_void) {
        for (uint32_t d = 0; d <= c.n_dst; ++d) c.w_dst_ptr[d] = 0;
        return;
    }
    const Pool from = half(c, s.prev), to = half(c, s.cur);
    for (uint64_t i = 0; i < s.prev_n; ++i) {
        if (due(c, from, i)) stage_due(c, from, i);
        else keep(c, from, to, i, s.len++);
    }
    for (uint32_t d = 0; d < c.n_dst; ++d) {
        const uint64_t b = c.w_dst_ptr[d], e = c.w_dst_ptr[d + 1];
        // equal keys stay in staging order, as before_at ranks them
        std::stable_sort(c.stage + b, c.stage + e,
                         [](const Rec &x, const Rec &y) { return before(key_of(x), key_of(y)); });
        for (uint64_t k = b; k < e; ++k) emit(c, c.stage[k], k);
    }
}

}  // namespace flight
#endif
