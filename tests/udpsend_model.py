"""Python model of a host's UDP send side: the checker for srt_udpsend (host-only
and device forms).

Written from the semantics of the reference (not a transcription of the
library's step):
  udp.rs:327-475       sendmsg: EPIPE, the destination, EMSGSIZE, the bind, has_space,
                       the priority draw, the 0.0.0.0 source rewrite, the notify
  udp.rs:170-203       pull_out_packet, peek_next_packet_priority, has_data_to_send
  udp.rs:1056-1134     MessageBuffer: a soft byte limit, has_space = len < limit
  udp.rs:874-899       SO_SNDBUF; :767-788 shutdown; :229-240 close
  host.rs:715-720      get_next_packet_priority, the counter starts at 1
  network_interface.c:205-370, relay/mod.rs:200-272   pop and forward_until_blocked, as
                       tests/outbound_model.py models them; the TokenBucket is that model's
  event order          the calls of time t, the forward task of t, its wake-ups in the
                       order of the pops, a further forward task of t if one was scheduled
"""
from collections import deque

import numpy as np

from outbound_model import CACHED, FIFO, FORWARDED, INTERFACE_SENT, RR, TokenBucket, U64, sat

assert RR == 1 and FIFO == 0

SND_CREATED = 1 << 1
HAS_ADDR, WAIT, RAW, LOCAL = 0x1, 0x10000, 0x20000, 0x40000
NOT_TAKEN, DONE, ARMED = 0, 1, 2
OPEN, CLOSE, BIND, SET_PEER, SET_SNDBUF, SHUT_WR, SET_NEXT_PRIORITY = 1, 2, 3, 4, 5, 6, 7
F_RING_OVERFLOW, F_LATE_OVERFLOW, F_TIME_REGRESSION, F_OVERSIZE, F_AFTER_UNTIL, F_BAD_SOCKET = 1, 2, 4, 8, 16, 32
F_UNBOUND, F_LOOPBACK, F_ARMED_TWICE, F_REOPEN_BUSY, F_LATE_RESULT_OVERFLOW, F_CALL_ORDER = 64, 128, 256, 512, 1024, 2048
EBADF, EWOULDBLOCK, EPIPE, EDESTADDRREQ, EMSGSIZE = 9, 11, 32, 89, 90
DGRAM_MAX, HEADERS = 65507, 28
LOCALHOST = int.from_bytes(bytes([127, 0, 0, 1]), "little")

SEND = np.dtype([("time_ns", "<u8"), ("priority", "<u8"), ("slot", "<u4"), ("len", "<u4"), ("dst_ip_be", "<u4"),
                 ("dst_port_be", "<u2"), ("reserved", "<u2"), ("flags", "<u4"), ("user", "<u4")])
RESULT = np.dtype([("complete_ns", "<u8"), ("priority", "<u8"), ("return_val", "<i8"), ("status", "<u4"),
                   ("src_ip_be", "<u4"), ("src_port_be", "<u2"), ("reserved", "<u2"), ("user", "<u4")])
LATE_RESULT = np.dtype([("seq", "<u8"), ("result", RESULT)])
LATE = np.dtype([("seq", "<u8"), ("send_ns", "<u8"), ("send_rank", "<u8"), ("status", "<u4"), ("src_host", "<u4")])
OP = np.dtype([("op", "<u4"), ("slot", "<u4"), ("value", "<u8")])
SOCK_STATE = np.dtype([("len_bytes", "<u8"), ("soft_limit", "<u8"), ("armed_seq", "<u8"), ("n_msgs", "<u4"),
                       ("bound_ip_be", "<u4"), ("peer_ip_be", "<u4"), ("bound_port_be", "<u2"), ("peer_port_be", "<u2"),
                       ("open", "u1"), ("shut_wr", "u1"), ("bound", "u1"), ("has_peer", "u1"), ("overflow", "u1"),
                       ("reserved0", "u1"), ("reserved1", "<u2")])
HOST_STATE = np.dtype([(k, "<u8") for k in ("balance", "last_refill_ns", "task_ns", "tasks_scheduled", "sent_total",
                                            "queue_len")] + [("cached", "<u4"), ("overflow", "<u4"),
                                                             ("next_priority", "<u8")])


def sndbuf_limit(optval):
    return min(max(optval * 2, 4096), 1 << 28)


class Message:
    def __init__(self, seq, priority, size, local, raw):
        self.seq, self.priority, self.size, self.local, self.raw = seq, priority, size, local, raw
        self.was_cached = False


class Socket:
    def __init__(self):
        self.open = self.shut_wr = False
        self.limit = self.len_bytes = 0
        self.bound = self.peer = None   # (ip, port)
        self.armed = None               # the blocked sendmsg: dict(seq, len, dst, flags, user)
        self.buffer = deque()           # the send buffer (or, for a slot not open here, raw packets)
        self.overflow = False

    def has_space(self):
        return self.len_bytes < self.limit


class HostSend:
    """the host's UDP sockets, its internet interface and relay_inet_out"""

    def __init__(self, model, h, slots, ip, bytes_per_second):
        self.m, self.h, self.slots, self.ip = model, h, slots, ip
        self.bucket = TokenBucket.for_bandwidth(bytes_per_second)
        self.tracked = []      # the qdisc's sockets, in the order they joined (RR: a queue)
        self.cached = None
        self.task = None
        self.tasks = self.sent = 0
        self.next_priority = 1
        self.overflow = False

    # --- sendmsg
    def checks(self, s, call):
        """checks 2 to 6: a (status, return_val) verdict, or the destination ip"""
        if s.shut_wr:
            return (DONE, -EPIPE)
        if call["flags"] & HAS_ADDR:
            dst = call["dst"]
        elif s.peer is not None:
            dst = s.peer[0]
        else:
            return (DONE, -EDESTADDRREQ)
        if call["len"] > DGRAM_MAX:
            return (DONE, -EMSGSIZE)
        if s.bound is None:
            self.m.flags |= F_UNBOUND
            return (NOT_TAKEN, 0)
        if dst == LOCALHOST or s.bound[0] == LOCALHOST:
            self.m.flags |= F_LOOPBACK
            return (NOT_TAKEN, 0)
        return dst

    def notify(self, slot, now):
        if slot not in self.tracked:
            self.tracked.append(slot)
        if self.task is None:
            self.task, self.tasks = now, self.tasks + 1

    def attempt(self, slot, call, now):
        """sendmsg from check 2 on; None: the buffer has no space"""
        s = self.m.socks[slot]
        v = self.checks(s, call)
        if isinstance(v, tuple):
            return dict(status=v[0], return_val=v[1], complete_ns=now if v[0] == DONE else 0)
        if not s.has_space():
            return None
        prio, self.next_priority = self.next_priority, self.next_priority + 1
        s.len_bytes += call["len"]
        s.buffer.append(Message(call["seq"], prio, call["len"], v == self.ip, False))
        self.m.n_acc += 1
        self.notify(slot, now)
        return dict(status=DONE, return_val=call["len"], complete_ns=now, priority=prio,
                    src_ip_be=s.bound[0] or self.ip, src_port_be=s.bound[1])

    def sendmsg(self, call):
        m, slot, now = self.m, call["slot"], call["time"]
        mine = slot in self.slots
        if call["flags"] & RAW:
            if not mine or m.socks[slot].open:
                m.flags |= F_BAD_SOCKET
                return
            m.socks[slot].buffer.append(Message(call["seq"], call["priority"], call["len"], bool(call["flags"] & LOCAL),
                                                True))
            m.n_acc += 1
            self.notify(slot, now)
            m.answer(call["seq"], dict(status=DONE, return_val=call["len"], complete_ns=now, priority=call["priority"]))
            return
        if not mine or not m.socks[slot].open:
            m.flags |= F_BAD_SOCKET
            m.answer(call["seq"], dict(status=DONE, return_val=-EBADF, complete_ns=now))
            return
        s = m.socks[slot]
        r = self.attempt(slot, call, now)
        if r is None:
            if call["flags"] & WAIT and s.armed is None:
                s.armed = call
                m.n_arm += 1
                r = dict(status=ARMED)
            else:
                if call["flags"] & WAIT:
                    m.flags |= F_ARMED_TWICE
                m.n_wb += 1
                r = dict(status=DONE, return_val=-EWOULDBLOCK, complete_ns=now)
        m.answer(call["seq"], r)

    # --- the interface and the relay
    def pop(self, now, woken):
        if not self.tracked:
            return None
        socks = self.m.socks
        if self.m.qdisc == RR:
            slot = self.tracked.pop(0)
        else:
            slot = min(self.tracked, key=lambda x: (socks[x].buffer[0].priority, socks[x].buffer[0].seq))
            self.tracked.remove(slot)
        s = socks[slot]
        p = s.buffer.popleft()
        if s.buffer:
            self.tracked.append(slot)
        if not p.raw:  # pull_out_packet
            had_space = s.has_space()
            s.len_bytes -= p.size
            if not had_space and s.has_space() and s.open:
                if self.m.first_writable[slot] == U64:
                    self.m.first_writable[slot] = now
                if s.armed is not None:
                    woken.append(slot)
        return p

    def run_task(self, boot_end, until):
        now, self.task = self.task, None
        woken = []
        while True:
            if self.cached is not None:
                p, self.cached = self.cached, None
            else:
                p = self.pop(now, woken)
                if p is None:
                    break
            size = p.size if p.raw else p.size + HEADERS
            if not p.local and now >= boot_end:
                verdict, val = self.bucket.remove(size, now)
                if verdict == "err":
                    p.was_cached = True
                    self.cached = p
                    self.task, self.tasks = sat(now + val), self.tasks + 1
                    if size > self.bucket.capacity:
                        self.m.flags |= F_OVERSIZE
                        self.task = max(self.task, until)
                    break
            st = INTERFACE_SENT | FORWARDED | (CACHED if p.was_cached else 0) | (0 if p.raw else SND_CREATED)
            rank = None
            if not p.local:
                rank, self.sent = self.sent, self.sent + 1
            self.m.resolve(p.seq, st, now, rank, self.h)
        for slot in woken:  # the blocked syscalls run again, later events of the same instant
            s = self.m.socks[slot]
            if s.armed is None or not s.open:
                continue
            r = self.attempt(slot, s.armed, now)
            if r is not None:
                call, s.armed = s.armed, None
                r["user"] = call["user"]
                self.m.answer(call["seq"], r)

    def advance(self, calls, until, boot_end):
        m = self.m
        i, tmax = 0, m.prev_until
        while True:
            if i < len(calls) and calls[i]["time"] < tmax:
                m.flags |= F_TIME_REGRESSION if calls[i]["time"] < m.prev_until else F_CALL_ORDER
                i += 1
            elif i < len(calls) and calls[i]["time"] < until and (self.task is None or calls[i]["time"] <= self.task):
                tmax = calls[i]["time"]
                self.sendmsg(calls[i])
                i += 1
            elif self.task is not None and self.task < until:
                self.run_task(boot_end, until)
            else:
                break
        if i < len(calls):
            m.flags |= F_AFTER_UNTIL


class UdpSendModel:
    """the srt_udpsend calls over numpy arrays"""

    def __init__(self, socket_ptr, host_ip_be, bw_up_bytes_per_s, qdisc, ring_cap):
        sp = [int(x) for x in socket_ptr]
        self.qdisc, self.ring_cap = qdisc, ring_cap
        self.socks = [Socket() for _ in range(sp[-1])]
        self.hosts = [HostSend(self, h, range(sp[h], sp[h + 1]), int(host_ip_be[h]), int(bw_up_bytes_per_s[h]))
                      for h in range(len(sp) - 1)]
        self.base = self.prev_until = 0
        self.flags = self.n_acc = self.n_wb = self.n_arm = 0

    def config(self, ops):
        for op, slot, value in ops:
            op, slot, value = int(op), int(slot), int(value)
            if op == SET_NEXT_PRIORITY:
                self.hosts[slot].next_priority = value
                continue
            s = self.socks[slot]
            pair = (value & 0xffffffff, (value >> 32) & 0xffff)
            if op == OPEN:
                if s.buffer:
                    self.flags |= F_REOPEN_BUSY
                    continue
                overflow = s.overflow
                s.__init__()
                s.open, s.limit, s.overflow = True, value, overflow
            elif not s.open:
                continue
            elif op == CLOSE:
                s.open, s.armed = False, None
            elif op == BIND:
                s.bound = pair
            elif op == SET_PEER:
                s.peer = pair if pair != (0, 0) else None
            elif op == SET_SNDBUF:
                s.limit = sndbuf_limit(value)
            elif op == SHUT_WR:
                if s.peer is not None:
                    s.shut_wr = True

    def answer(self, seq, r):
        if seq >= self.base:
            rec = self.results[seq - self.base]
            for k, v in r.items():
                rec[k] = v
        else:
            rec = np.zeros((), RESULT)
            for k, v in r.items():
                rec[k] = v
            self.late_results.append((seq, rec))

    def resolve(self, seq, st, now, rank, h):
        rank = U64 if rank is None else rank
        if seq >= self.base:
            i = seq - self.base
            self.status[i], self.send_ns[i], self.send_rank[i] = st, now, rank
        else:
            self.late.append((seq, now, rank, st, h))

    def run(self, calls, host_ptr, until_ns, bootstrap_end_ns):
        """calls: SEND records -> dict(results, status, send_ns, send_rank, late (sorted tuples), late_results
        (sorted by seq), first_writable, base)"""
        n = len(calls)
        self.results = np.zeros(n, RESULT)
        self.results["user"] = calls["user"]
        self.status = np.zeros(n, np.uint32)
        self.send_ns = np.full(n, U64, np.uint64)
        self.send_rank = np.full(n, U64, np.uint64)
        self.late, self.late_results = [], []
        self.first_writable = np.full(len(self.socks), U64, np.uint64)
        base = self.base
        for h, host in enumerate(self.hosts):
            mine = [dict(seq=base + i, time=int(c["time_ns"]), priority=int(c["priority"]), slot=int(c["slot"]),
                         len=int(c["len"]), dst=int(c["dst_ip_be"]), flags=int(c["flags"]), user=int(c["user"]))
                    for i, c in ((i, calls[i]) for i in range(int(host_ptr[h]), int(host_ptr[h + 1])))]
            host.advance(mine, int(until_ns), int(bootstrap_end_ns))
            if host.cached is not None and host.cached.seq >= base:
                self.status[host.cached.seq - base] = INTERFACE_SENT | CACHED | (0 if host.cached.raw else SND_CREATED)
            for slot in host.slots:  # what crosses the call: at most ring_cap messages a socket
                s = self.socks[slot]
                if len(s.buffer) > self.ring_cap:
                    while len(s.buffer) > self.ring_cap:
                        s.buffer.pop()
                    s.overflow = host.overflow = True
                    self.flags |= F_RING_OVERFLOW
                    if not s.buffer and slot in host.tracked:
                        host.tracked.remove(slot)
        self.base += n
        self.prev_until = int(until_ns)
        late_res = np.zeros(len(self.late_results), LATE_RESULT)
        for k, (seq, rec) in enumerate(sorted(self.late_results, key=lambda x: x[0])):
            late_res[k]["seq"], late_res[k]["result"] = seq, rec
        return dict(results=self.results, status=self.status, send_ns=self.send_ns, send_rank=self.send_rank,
                    late=sorted(self.late), late_results=late_res, first_writable=self.first_writable, base=base)

    def pending(self):
        return sum(len(self.socks[x].buffer) for h in self.hosts for x in h.slots) + \
            sum(h.cached is not None for h in self.hosts)

    def take_status(self):
        f, self.flags = self.flags, 0
        return (f, self.pending(), self.n_acc, self.n_wb, self.n_arm)

    def state(self):
        hosts = np.zeros(len(self.hosts), HOST_STATE)
        for k, h in enumerate(self.hosts):
            b = h.bucket
            hosts[k] = (b.balance, b.last_refill, U64 if h.task is None else h.task, h.tasks, h.sent,
                        sum(len(self.socks[x].buffer) for x in h.slots), int(h.cached is not None), int(h.overflow),
                        h.next_priority)
        socks = np.zeros(len(self.socks), SOCK_STATE)
        for k, s in enumerate(self.socks):
            b, p = s.bound or (0, 0), s.peer or (0, 0)
            socks[k] = (s.len_bytes, s.limit, U64 if s.armed is None else s.armed["seq"], len(s.buffer), b[0], p[0],
                        b[1], p[1], s.open, s.shut_wr, s.bound is not None, s.peer is not None, s.overflow, 0, 0)
        return hosts, socks
