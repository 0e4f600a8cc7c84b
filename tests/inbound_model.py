"""Python model of a destination host's inbound router stage: the checker for
srt_inbound (host-only and device forms).

Written from the semantics of three reference files and the event order
(not a transcription of the library's step):
  router/codel_queue.rs    CoDelQueue: TARGET 10 ms, INTERVAL 100 ms, no limit
  relay/token_bucket.rs    TokenBucket with lazy refills on a fixed schedule
  relay/mod.rs             Relay: Idle / Pending, cached next_packet, bucket of
                           max(1, bytes_per_second / 1000) per ms + CONFIG_MTU
  core/work/event.rs       equal times: packet events before the forward task

tests/golden/inbound_reference_cases.json (the reference's own unit-test
scenarios) pins the queue and the bucket here to the reference.
"""
import math
from collections import deque
from fractions import Fraction

import numpy as np

U64 = (1 << 64) - 1
MS = 1_000_000
TARGET = 10 * MS
INTERVAL = 100 * MS
MTU = 1500

ENQUEUED, DEQUEUED, DROPPED, CACHED, FORWARDED = 1 << 10, 1 << 11, 1 << 12, 1 << 21, 1 << 22


def sat(x):
    return max(0, min(U64, x))


def control_law_increment(count):
    """round(INTERVAL / sqrt(count)) in f64, half away from zero; 0 counts as 1."""
    root = math.sqrt(float(count)) if count else 1.0
    return int(Fraction(float(INTERVAL) / root) + Fraction(1, 2))  # floor of x + 1/2, exactly (x > 0)


class CoDelQueue:
    STORE, DROP = "store", "drop"

    def __init__(self):
        self.items = deque()  # (enqueue time, size, tag)
        self.bytes = 0
        self.mode = self.STORE
        self.interval_end = None
        self.drop_next = None
        self.current_drop_count = 0
        self.previous_drop_count = 0
        self.dropped = []  # tags, in drop order
        self.drop_entries = 0    # times Drop mode was entered (scenario checks)
        self.max_drop_count = 0  # highest current_drop_count seen

    def __len__(self):
        return len(self.items)

    def push(self, tag, size, now):
        self.bytes += size
        self.items.append((now, size, tag))

    # ---- the head of the queue and the standing-delay bookkeeping
    def process_standing_delay(self, now, delay):
        if delay < TARGET or self.bytes <= MTU:
            self.interval_end = None
            return False
        if self.interval_end is None:
            self.interval_end = sat(now + INTERVAL)
            return False
        return now >= self.interval_end

    def _head(self, now):
        """(tag, ok_to_drop) of the head, removed; None when empty."""
        if not self.items:
            self.interval_end = None
            return None
        ts, size, tag = self.items.popleft()
        self.bytes = sat(self.bytes - size)
        return tag, self.process_standing_delay(now, sat(now - ts))

    def should_drop(self, now):
        return self.drop_next is not None and now >= self.drop_next

    def was_dropping_recently(self, now):
        return self.drop_next is not None and sat(now - self.drop_next) < 16 * INTERVAL

    # ---- pop: the tag that is dequeued, or None
    def pop(self, now):
        head = self._head(now)
        if head is None or not head[1]:
            self.mode = self.STORE
            return None if head is None else head[0]
        tag = head[0]
        if self.mode == self.STORE:
            # one drop, into Drop mode; whatever comes next is handed out as it is
            self.dropped.append(tag)
            follower = self._head(now)
            self.mode = self.DROP
            delta = sat(self.current_drop_count - self.previous_drop_count)
            self.current_drop_count = delta if (self.was_dropping_recently(now) and delta > 1) else 1
            self.drop_next = sat(now + control_law_increment(self.current_drop_count))
            self.previous_drop_count = self.current_drop_count
            self.drop_entries += 1
            self.max_drop_count = max(self.max_drop_count, self.current_drop_count)
            return None if follower is None else follower[0]
        while head is not None and self.mode == self.DROP and self.should_drop(now):
            self.dropped.append(head[0])
            self.current_drop_count += 1
            self.max_drop_count = max(self.max_drop_count, self.current_drop_count)
            head = self._head(now)
            if head is not None and head[1]:
                self.drop_next = sat(self.drop_next + control_law_increment(self.current_drop_count))
            else:
                self.mode = self.STORE
        return None if head is None else head[0]


class TokenBucket:
    def __init__(self, capacity, refill_increment, refill_interval, last_refill=0):
        assert capacity > 0 and refill_increment > 0 and refill_interval > 0
        self.capacity, self.balance = capacity, capacity
        self.refill_increment, self.refill_interval = refill_increment, refill_interval
        self.last_refill = last_refill

    @classmethod
    def for_bandwidth(cls, bytes_per_second):
        refill = max(1, bytes_per_second // 1000)
        return cls(refill + MTU, refill, MS)

    def _refill(self, now):
        """applies the refills due by `now`; time left to the next one"""
        due = (now - self.last_refill) // self.refill_interval
        if due >= 1:
            self.balance = min(self.capacity, sat(self.balance + sat(self.refill_increment * due)))
            self.last_refill = sat(self.last_refill + sat(self.refill_interval * due))
        return self.refill_interval - (now - self.last_refill)

    def remove(self, decrement, now):
        """("ok", new balance) or ("err", time until the decrement conforms)"""
        to_next = self._refill(now)
        if decrement <= self.balance:
            self.balance -= decrement
            return "ok", self.balance
        refills = -((self.balance - decrement) // self.refill_increment)  # ceil(missing / increment)
        return "err", sat(to_next + self.refill_interval * (refills - 1))


class HostInbound:
    """router + relay_inet_in of one host"""

    def __init__(self, bytes_per_second):
        self.queue = CoDelQueue()
        self.bucket = TokenBucket.for_bandwidth(bytes_per_second)
        self.cached = None  # (tag, size): the relay's next_packet
        self.task = None    # time of the pending forward task
        self.tasks = 0
        self.sizes = {}     # tag -> size of the packets inside
        self.was_cached = set()
        self.out = []       # (tag, status, forward time or None), in resolution order
        self.last_arrival = None
        self.ties = 0             # arrivals at the time of the one before (scenario checks)
        self.on_blocked_task = 0  # arrivals exactly at the time of a blocked relay's pending task

    def arrive(self, tag, size, t):
        self.ties += t == self.last_arrival
        self.on_blocked_task += self.cached is not None and self.task == t
        self.last_arrival = t
        self.sizes[tag] = size
        self.queue.push(tag, size, t)
        if self.task is None:  # Idle relay: forward task with delay 0
            self.task, self.tasks = t, self.tasks + 1

    def _flush_drops(self):
        for tag in self.queue.dropped:
            del self.sizes[tag]
            self.out.append((tag, ENQUEUED | DROPPED, None))
        self.queue.dropped.clear()

    def run_task(self, bootstrap_end):
        now, self.task = self.task, None
        while True:
            if self.cached is not None:
                tag, self.cached = self.cached, None
            else:
                tag = self.queue.pop(now)
                self._flush_drops()
                if tag is None:
                    return
            if now >= bootstrap_end:
                verdict, val = self.bucket.remove(self.sizes[tag], now)
                if verdict == "err":
                    self.cached = tag
                    self.was_cached.add(tag)
                    self.task, self.tasks = sat(now + val), self.tasks + 1
                    return
            st = ENQUEUED | DEQUEUED | FORWARDED | (CACHED if tag in self.was_cached else 0)
            self.was_cached.discard(tag)
            del self.sizes[tag]
            self.out.append((tag, st, now))

    def advance(self, arrivals, until, bootstrap_end):
        """arrivals: [(time, tag, size)] in event order; tasks before `until` run.
        An arrival at or after `until` belongs to a later window and is not
        taken; returns how many were left."""
        i = 0
        while True:
            if i < len(arrivals) and arrivals[i][0] < until and (self.task is None or arrivals[i][0] <= self.task):
                t, tag, size = arrivals[i]
                self.arrive(tag, size, t)
                i += 1
            elif self.task is not None and self.task < until:
                self.run_task(bootstrap_end)
            else:
                return len(arrivals) - i

    def state(self):
        q, b = self.queue, self.bucket
        return dict(balance=b.balance, last_refill_ns=b.last_refill,
                    interval_end_ns=U64 if q.interval_end is None else q.interval_end,
                    drop_next_ns=U64 if q.drop_next is None else q.drop_next,
                    current_drop_count=q.current_drop_count, previous_drop_count=q.previous_drop_count,
                    queue_len=len(q), bytes_stored=q.bytes, task_ns=U64 if self.task is None else self.task,
                    tasks_scheduled=self.tasks, mode=int(q.mode == CoDelQueue.DROP), cached=int(self.cached is not None))


class InboundModel:
    """the srt_inbound calls over numpy arrays"""

    def __init__(self, bw_down_bytes_per_s):
        self.hosts = [HostInbound(int(b)) for b in bw_down_bytes_per_s]
        self.base = 0
        self.not_taken = 0  # arrivals at or after their call's until_ns (status 0, flagged by the library)

    def run(self, order, dst_ptr, deliver, total_size, until_ns, bootstrap_end_ns):
        """-> (status[n], forward_ns[n], late records sorted by seq as
        (seq, forward_ns, status, dst_host) tuples, seq base)"""
        n = len(deliver)
        status = np.zeros(n, np.uint32)
        forward = np.full(n, U64, np.uint64)
        late = []
        base = self.base
        for h, host in enumerate(self.hosts):
            grp = [int(p) for p in order[int(dst_ptr[h]):int(dst_ptr[h + 1])]]
            host.out = []
            self.not_taken += host.advance([(int(deliver[p]), base + p, int(total_size[p])) for p in grp],
                                           int(until_ns), int(bootstrap_end_ns))
            for seq, st, fwd in host.out:
                if seq >= base:
                    status[seq - base] = st
                    if fwd is not None:
                        forward[seq - base] = fwd
                else:
                    late.append((seq, U64 if fwd is None else fwd, st, h))
            for _, _, seq in host.queue.items:
                if seq >= base:
                    status[seq - base] = ENQUEUED
            if host.cached is not None and host.cached >= base:
                status[host.cached - base] = ENQUEUED | DEQUEUED | CACHED
        self.base += n
        return status, forward, sorted(late), base

    def pending(self):
        return sum(len(h.queue) + (h.cached is not None) for h in self.hosts)

    def state(self):
        return [h.state() for h in self.hosts]
