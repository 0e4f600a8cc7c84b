// srt_inbound_step.h -- one destination host's inbound router stage, written
// once for the host and the device (srt_inbound.hip compiles it for both).
//
// Reference, restated line by line, quirks included:
//   CoDelQueue     src/main/network/router/codel_queue.rs (push, pop, codel_pop,
//                  process_standing_delay, drop_from_store_mode -- which returns
//                  the next item without looking at its ok_to_drop --,
//                  drop_from_drop_mode, apply_control_law)
//   TokenBucket    src/main/network/relay/token_bucket.rs (lazy_refill,
//                  conforming_remove, compute_conforming_duration; saturating
//                  u64 arithmetic) as sized by relay/mod.rs:277-287
//   Relay          src/main/network/relay/mod.rs:110-272 (notify, forward_later,
//                  forward_until_blocked with the cached next_packet)
//   event order    core/work/event.rs:102-110: at equal times every packet
//                  event runs before any local event (the forward task)
//
// The queue of a host is its ring in HBM (packets carried over from earlier
// calls) followed by a window [qpos, ppos) of the current call's staged
// arrival records: arrivals are pushed in stream order, so the queued ones of
// this call are always a contiguous run of the stream and nothing is copied
// while the call runs.  What is still queued at the end of the call moves to
// the ring; a host that never backs up touches only its state record.
// On the device the wave first copies its 64 hosts' records -- one contiguous
// span of the stream -- into LDS with coalesced loads, so the serial loop
// reads on-chip memory; a span larger than the window is read from HBM.
#ifndef SRT_INBOUND_STEP_H
#define SRT_INBOUND_STEP_H

#include <math.h>
#include <stdint.h>

#include "../../include/srt.h"

#include "srt_relay_common.h"

#define INB_HD SRT_HD

namespace inb {

// the bucket and the saturating helpers are srt_relay_common.h's, shared with the outbound step
using relay::add_pending;
using relay::MTU;
using relay::NONE;
using relay::raise;
using relay::REFILL_NS;
using relay::sat_add;
using relay::sat_mul;
using relay::sat_sub;
using relay::take_slot;

constexpr uint64_t TARGET_NS = 10000000;    // codel_queue.rs:23
constexpr uint64_t INTERVAL_NS = 100000000;  // codel_queue.rs:28
constexpr uint32_t LAW_TABLE = 1024;        // control-law increments kept in a table

constexpr uint32_t F_RING_OVERFLOW = 1, F_LATE_OVERFLOW = 2, F_TIME_REGRESSION = 4, F_OVERSIZE = 8,
                   F_AFTER_UNTIL = 16;

// staged arrival: the gathers behind order[] done once, in group order
struct alignas(16) Rec {
    uint64_t ts;
    uint32_t size;
    uint32_t idx;  // batch index
};

struct RingEl {
    uint64_t ts;
    uint64_t seq;
    uint32_t size;
    uint32_t pad;
};

struct El {
    uint64_t ts;
    uint64_t seq;
    uint32_t size;
};

// per-host state, 128 bytes
struct Host {
    uint64_t balance, last_refill, refill, capacity;         // TokenBucket
    uint64_t interval_end, drop_next, cur_drops, prev_drops;  // CoDelQueue
    uint64_t bytes_stored;
    uint64_t task_ns;  // pending forward task (NONE: relay Idle)
    uint64_t tasks;    // forward tasks scheduled so far (event ids consumed)
    uint64_t cached_seq;
    uint32_t ring_head, ring_len;
    uint32_t mode;  // 0 Store, 1 Drop
    uint32_t cached, cached_size;
    uint32_t overflow;
    uint64_t pad;
};

struct Ctx {
    Host *hosts;
    RingEl *ring;
    const Rec *rec;
    const uint32_t *dst_ptr;
    uint32_t *status;
    uint64_t *forward;
    srt_inbound_late *late;
    uint32_t *late_count;
    uint32_t *flags;
    unsigned long long *pending;  // packets still in the stage, summed over the hosts by the call
    const uint64_t *law_tab;
    uint64_t base, until, boot_end, prev_until;
    uint32_t n_hosts, ring_cap, late_cap, n_pkts;
    uint32_t win_cap, pad;  // records a wave may hold in LDS (device)
};

// apply_control_law's increment (codel_queue.rs:288-296) in f64: the value the
// table holds for small counts and the path beyond it
INB_HD uint64_t law_increment_f64(uint64_t count) {
    const double c = count ? (double)count : 1.0;
    return (uint64_t)round(100000000.0 / sqrt(c));
}

INB_HD uint64_t law_increment(const uint64_t *tab, uint64_t count) {
    return count < LAW_TABLE ? tab[count] : law_increment_f64(count);
}

// one host's run over one call
template <bool WIN>
struct Run {
    Host s;
    const Ctx c;  // by value: a reference member would keep the whole object in private memory
    uint32_t h;
    uint32_t qpos, ppos;  // queued window of this call's stream
    uint32_t win0, win_n;  // device: records [win0, win0 + win_n) are held in LDS by the wave
    uint64_t last_ts;     // the record pushed last (the common pop needs no load)
    uint32_t last_size, last_idx;

    INB_HD Run(const Ctx &ctx, uint32_t host) : s(ctx.hosts[host]), c(ctx), h(host), qpos(0), ppos(0), win0(0), win_n(0), last_ts(0), last_size(0), last_idx(0) {}

    // staged record i: from the wave's LDS window (WIN: the whole run reads LDS
    // only, so its loads never wait for the outstanding stores), else from HBM
    INB_HD Rec rec_at(uint32_t i) const {
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (WIN) {
            extern __shared__ Rec inb_window[];
            return inb_window[i - win0];
        }
#endif
        return c.rec[i];
    }

    // a packet leaves the stage: batch packets by index, older ones to the late list
    INB_HD void resolve(uint64_t seq, uint32_t status, uint64_t forward_ns) {
        if (seq >= c.base) {
            const uint64_t i = seq - c.base;
            c.status[i] = status;
            if (forward_ns != NONE) c.forward[i] = forward_ns;
        } else {
            const uint32_t k = take_slot(c.late_count);
            if (k < c.late_cap) {
                srt_inbound_late r;
                r.seq = seq;
                r.forward_ns = forward_ns;
                r.status = status;
                r.dst_host = h;
                c.late[k] = r;
            } else {
                raise(c.flags, F_LATE_OVERFLOW);
            }
        }
    }

    INB_HD bool pop_front(El &el) {
        if (s.ring_len) {
            const RingEl e = c.ring[(uint64_t)h * c.ring_cap + s.ring_head];
            s.ring_head = s.ring_head + 1 == c.ring_cap ? 0 : s.ring_head + 1;
            --s.ring_len;
            el.ts = e.ts;
            el.seq = e.seq;
            el.size = e.size;
            return true;
        }
        if (qpos < ppos) {
            el.ts = last_ts;
            el.seq = c.base + last_idx;
            el.size = last_size;
            if (qpos + 1 != ppos) {
                const Rec x = rec_at(qpos);
                el.ts = x.ts;
                el.seq = c.base + x.idx;
                el.size = x.size;
            }
            ++qpos;
            return true;
        }
        return false;
    }

    // process_standing_delay (codel_queue.rs:233-264)
    INB_HD bool standing_delay(uint64_t now, uint64_t delay) {
        if (delay < TARGET_NS || s.bytes_stored <= MTU) {
            s.interval_end = NONE;
            return false;
        }
        if (s.interval_end != NONE) return now >= s.interval_end;
        s.interval_end = sat_add(now, INTERVAL_NS);
        return false;
    }

    // codel_pop (codel_queue.rs:205-229)
    INB_HD bool codel_pop(uint64_t now, El &el, bool &ok_to_drop) {
        if (!pop_front(el)) {
            s.interval_end = NONE;
            return false;
        }
        s.bytes_stored = sat_sub(s.bytes_stored, el.size);
        ok_to_drop = standing_delay(now, sat_sub(now, el.ts));
        return true;
    }

    INB_HD void drop(const El &el) { resolve(el.seq, SRT_PDS_ROUTER_ENQUEUED | SRT_PDS_ROUTER_DROPPED, NONE); }

    // CoDelQueue::pop (codel_queue.rs:125-202); true: `out` is dequeued
    INB_HD bool pop(uint64_t now, El &out) {
        El it;
        bool ok = false;
        if (!codel_pop(now, it, ok)) {
            s.mode = 0;
            return false;
        }
        if (!ok) {
            s.mode = 0;
            out = it;
            return true;
        }
        if (s.mode == 0) {  // drop_from_store_mode
            drop(it);
            bool ok2 = false;
            const bool has = codel_pop(now, out, ok2);
            s.mode = 1;
            const uint64_t delta = sat_sub(s.cur_drops, s.prev_drops);
            const bool recently = s.drop_next != NONE && sat_sub(now, s.drop_next) < INTERVAL_NS * 16;
            s.cur_drops = recently && delta > 1 ? delta : 1;
            s.drop_next = sat_add(now, law_increment(c.law_tab, s.cur_drops));
            s.prev_drops = s.cur_drops;
            return has;
        }
        // drop_from_drop_mode
        bool has = true;
        while (has && s.mode == 1 && s.drop_next != NONE && now >= s.drop_next) {
            drop(it);
            ++s.cur_drops;
            has = codel_pop(now, it, ok);
            if (has && ok) s.drop_next = sat_add(s.drop_next, law_increment(c.law_tab, s.cur_drops));
            else s.mode = 0;
        }
        if (has) out = it;
        return has;
    }

    // TokenBucket::conforming_remove_inner (token_bucket.rs:75-157); false: *wait
    INB_HD bool conforming_remove(uint64_t dec, uint64_t now, uint64_t &wait) {
        return relay::bucket_remove(s.balance, s.last_refill, s.refill, s.capacity, dec, now, wait);
    }

    // Relay::forward_until_blocked (relay/mod.rs:200-272) at the task's time
    INB_HD void forward_task() {
        const uint64_t now = s.task_ns;
        s.task_ns = NONE;
        for (;;) {
            El el;
            uint32_t st = SRT_PDS_ROUTER_ENQUEUED | SRT_PDS_ROUTER_DEQUEUED | SRT_PDS_RELAY_FORWARDED;
            if (s.cached) {
                el.ts = 0;
                el.seq = s.cached_seq;
                el.size = s.cached_size;
                s.cached = 0;
                st |= SRT_PDS_RELAY_CACHED;
            } else if (!pop(now, el)) {
                return;  // Idle
            }
            uint64_t wait = 0;
            if (now >= c.boot_end && !conforming_remove(el.size, now, wait)) {
                s.cached = 1;
                s.cached_seq = el.seq;
                s.cached_size = el.size;
                s.task_ns = sat_add(now, wait);
                if (el.size > s.capacity) {
                    // the bucket can never hold this packet (the reference would
                    // reschedule for ever): flagged, and at most one try a call
                    raise(c.flags, F_OVERSIZE);
                    if (s.task_ns < c.until) s.task_ns = c.until;
                }
                ++s.tasks;
                return;  // Pending
            }
            resolve(el.seq, st, now);
        }
    }

    INB_HD void run() {
        // the group's bounds, held inside the records staged by this call whatever dst_ptr[] says
        uint32_t lim = c.dst_ptr[c.n_hosts] < c.n_pkts ? c.dst_ptr[c.n_hosts] : c.n_pkts;
        if (WIN && lim > win0 + win_n) lim = win0 + win_n;  // and inside the window
        uint32_t b = c.dst_ptr[h] < lim ? c.dst_ptr[h] : lim;
        if (WIN && b < win0) b = win0;
        uint32_t e = c.dst_ptr[h + 1] < lim ? c.dst_ptr[h + 1] : lim;
        if (e < b) e = b;
        qpos = ppos = b;
        uint64_t nxt_ts = 0;
        uint32_t nxt_size = 0, nxt_idx = 0;
        if (ppos < e) {
            const Rec x = rec_at(ppos);
            nxt_ts = x.ts, nxt_size = x.size, nxt_idx = x.idx;
        }
        for (;;) {
            if (ppos < e && nxt_ts < c.until && nxt_ts <= s.task_ns) {
                // packet event: Router::push + Relay::notify
                last_ts = nxt_ts, last_size = nxt_size, last_idx = nxt_idx;
                ++ppos;
                if (ppos < e) {  // in flight while this one is handled
                    const Rec x = rec_at(ppos);
                    nxt_ts = x.ts, nxt_size = x.size, nxt_idx = x.idx;
                }
                if (last_ts < c.prev_until) raise(c.flags, F_TIME_REGRESSION);
                s.bytes_stored += last_size;
                if (s.task_ns == NONE) {
                    s.task_ns = last_ts;
                    ++s.tasks;
                }
            } else if (s.task_ns < c.until) {
                forward_task();
            } else {
                break;
            }
        }
        // An arrival at or after until_ns belongs to a later window (pushed now
        // it could overtake that window's earlier arrivals and tasks): it is
        // not taken, its status stays 0, and the call is flagged.
        if (ppos < e) raise(c.flags, F_AFTER_UNTIL);
        // what is still queued moves to the ring (the capacity check precedes every write)
        for (; qpos < ppos; ++qpos) {
            Rec x;
            x.ts = last_ts, x.size = last_size, x.idx = last_idx;
            if (qpos + 1 != ppos) x = rec_at(qpos);
            c.status[x.idx] = SRT_PDS_ROUTER_ENQUEUED;
            if (s.ring_len < c.ring_cap) {
                uint32_t t = s.ring_head + s.ring_len;
                if (t >= c.ring_cap) t -= c.ring_cap;
                RingEl r;
                r.ts = x.ts;
                r.seq = c.base + x.idx;
                r.size = x.size;
                r.pad = 0;
                c.ring[(uint64_t)h * c.ring_cap + t] = r;
                ++s.ring_len;
            } else if (!s.overflow) {
                s.overflow = 1;
                raise(c.flags, F_RING_OVERFLOW);
            }
        }
        if (s.cached && s.cached_seq >= c.base)
            c.status[s.cached_seq - c.base] = SRT_PDS_ROUTER_ENQUEUED | SRT_PDS_ROUTER_DEQUEUED | SRT_PDS_RELAY_CACHED;
        add_pending(c.pending, (unsigned long long)s.ring_len + s.cached);
        c.hosts[h] = s;
    }
};

}  // namespace inb
#endif
