"""Python model of a source host's outbound relay stage: the checker for
srt_outbound (host-only and device forms).

Written from the semantics of the reference (not a transcription of the
library's step):
  host/host.rs:988-1002         a socket with data: the interface tracks the
                                socket unless it does already, the relay is notified
  network_interface.c:205-370   the interface's pop: FIFO takes the socket whose
                                next packet has the smallest priority, round
                                robin the head of a plain queue; a socket that
                                still has data is put back
  relay/mod.rs:110-272          Relay: Idle / Pending, cached next_packet, local
                                packets and bootstrap exempt from the bucket
  relay/token_bucket.rs         TokenBucket (tests/inbound_model.py, pinned to the
                                reference by tests/golden/inbound_reference_cases.json)
  event order                   equal times: arrivals, in list order, before the
                                forward task
"""
from collections import deque

import numpy as np

from inbound_model import MS, U64, TokenBucket, sat

INTERFACE_SENT, CACHED, FORWARDED = 1 << 7, 1 << 21, 1 << 22
FIFO, RR = 0, 1
LOCAL = 1

assert MS  # re-exported


class Packet:
    __slots__ = ("tag", "priority", "size", "local", "order", "was_cached")

    def __init__(self, tag, priority, size, local, order):
        self.tag, self.priority, self.size, self.local, self.order = tag, priority, size, local, order
        self.was_cached = False


class Interface:
    """the sockets' send queues and the queuing discipline over them"""

    def __init__(self, qdisc):
        self.qdisc = qdisc
        self.sockets = {}        # socket -> deque of its packets (only sockets with data)
        self.rr = deque()        # RR: sockets in queue order

    def __len__(self):
        return sum(len(q) for q in self.sockets.values())

    def wants_send(self, socket, packet):
        tracked = socket in self.sockets
        self.sockets.setdefault(socket, deque()).append(packet)
        if not tracked:
            self.rr.append(socket)

    def pop(self):
        if not self.sockets:
            return None
        if self.qdisc == RR:
            socket = self.rr.popleft()
        else:
            # heads only; equal priorities (a caller error) in arrival order
            socket = min(self.sockets, key=lambda s: (self.sockets[s][0].priority, self.sockets[s][0].order))
        q = self.sockets[socket]
        packet = q.popleft()
        if q:
            if self.qdisc == RR:
                self.rr.append(socket)
        else:
            del self.sockets[socket]
        return packet


class HostOutbound:
    """network interface + relay_inet_out of one host"""

    def __init__(self, bytes_per_second, qdisc):
        self.iface = Interface(qdisc)
        self.bucket = TokenBucket.for_bandwidth(bytes_per_second)
        self.cached = None   # the relay's next_packet
        self.task = None     # time of the pending forward task
        self.tasks = 0
        self.sent = 0        # non-local packets forwarded: the next rank
        self.arrivals = 0
        self.out = []        # (tag, status, send time, rank or None), in resolution order
        self.last_arrival = None
        self.ties = 0             # arrivals at the time of the one before (scenario checks)
        self.on_blocked_task = 0  # arrivals exactly at the time of a blocked relay's pending task

    def arrive(self, tag, socket, priority, size, local, t):
        self.ties += t == self.last_arrival
        self.on_blocked_task += self.cached is not None and self.task == t
        self.last_arrival = t
        self.iface.wants_send(socket, Packet(tag, priority, size, local, self.arrivals))
        self.arrivals += 1
        if self.task is None:  # Idle relay: forward task with delay 0
            self.task, self.tasks = t, self.tasks + 1

    def run_task(self, bootstrap_end):
        now, self.task = self.task, None
        while True:
            if self.cached is not None:
                p, self.cached = self.cached, None
            else:
                p = self.iface.pop()
                if p is None:
                    return
            if not p.local and now >= bootstrap_end:
                verdict, val = self.bucket.remove(p.size, now)
                if verdict == "err":
                    p.was_cached = True
                    self.cached = p
                    self.task, self.tasks = sat(now + val), self.tasks + 1
                    return
            st = INTERFACE_SENT | FORWARDED | (CACHED if p.was_cached else 0)
            rank = None
            if not p.local:
                rank, self.sent = self.sent, self.sent + 1
            self.out.append((p.tag, st, now, rank))

    def advance(self, arrivals, until, bootstrap_end):
        """arrivals: [(time, tag, socket, priority, size, local)] in list order;
        tasks before `until` run.  An arrival at or after `until` is not taken;
        returns how many were left."""
        i = 0
        while True:
            if i < len(arrivals) and arrivals[i][0] < until and (self.task is None or arrivals[i][0] <= self.task):
                t, tag, socket, priority, size, local = arrivals[i]
                self.arrive(tag, socket, priority, size, local, t)
                i += 1
            elif self.task is not None and self.task < until:
                self.run_task(bootstrap_end)
            else:
                return len(arrivals) - i

    def state(self):
        b = self.bucket
        return dict(balance=b.balance, last_refill_ns=b.last_refill, task_ns=U64 if self.task is None else self.task,
                    tasks_scheduled=self.tasks, sent_total=self.sent, queue_len=len(self.iface),
                    cached=int(self.cached is not None))


class OutboundModel:
    """the srt_outbound calls over numpy arrays"""

    def __init__(self, bw_up_bytes_per_s, qdisc, max_sockets):
        self.hosts = [HostOutbound(int(b), qdisc) for b in bw_up_bytes_per_s]
        self.max_sockets = max_sockets
        self.base = 0
        self.not_taken = 0    # arrivals at or after their call's until_ns
        self.bad_socket = 0   # packets whose socket is not below max_sockets (not taken)

    def run(self, pkts, host_ptr, until_ns, bootstrap_end_ns):
        """pkts: OUT_PKT_DTYPE records -> (status[n], send_ns[n], send_rank[n], late records sorted by seq
        as (seq, send_ns, send_rank, status, src_host) tuples, seq base)"""
        n = len(pkts)
        status = np.zeros(n, np.uint32)
        send = np.full(n, U64, np.uint64)
        rank = np.full(n, U64, np.uint64)
        late = []
        base = self.base
        for h, host in enumerate(self.hosts):
            arr = []
            for i in range(int(host_ptr[h]), int(host_ptr[h + 1])):
                p = pkts[i]
                if int(p["socket"]) >= self.max_sockets:
                    self.bad_socket += 1
                    continue
                arr.append((int(p["ready_ns"]), base + i, int(p["socket"]), int(p["priority"]), int(p["total_size"]),
                            bool(int(p["flags"]) & LOCAL)))
            host.out = []
            self.not_taken += host.advance(arr, int(until_ns), int(bootstrap_end_ns))
            for seq, st, t, r in host.out:
                r = U64 if r is None else r
                if seq >= base:
                    status[seq - base], send[seq - base], rank[seq - base] = st, t, r
                else:
                    late.append((seq, t, r, st, h))
            if host.cached is not None and host.cached.tag >= base:
                status[host.cached.tag - base] = INTERFACE_SENT | CACHED
        self.base += n
        return status, send, rank, sorted(late), base

    def pending(self):
        return sum(len(h.iface) + (h.cached is not None) for h in self.hosts)

    def state(self):
        return [h.state() for h in self.hosts]
