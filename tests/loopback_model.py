"""Python model of a host's loopback interface: the checker for srt_loopback
(host-only and device forms).

A literal simulation of the reference's queues, not a restatement of the
library's sort keys:
  host/host.rs:988-1002           notify_socket_has_packets: the socket joins
                                  the interface's qdisc unless it is in it
                                  (network_interface.c:344-370) and the relay is
                                  notified; an Idle relay schedules one forward
                                  task, delay 0 (relay/mod.rs:110-135)
  network_queuing_disciplines.c   FIFO: a priority queue of sockets keyed on the
                                  priority of each socket's NEXT packet; round
                                  robin: a plain queue of sockets
  network_interface.c:205-340     pop: the qdisc's socket gives its next packet
                                  and goes back into the qdisc while it has data
  relay/mod.rs:200-272            Unlimited: the task pops until the interface
                                  is empty and pushes every packet back
  network_interface.c:140-202     push: the specific key, then the wildcard, in
                                  the loopback interface's own associations
  host/tracker.c:188-284          the local counters (tracker_model.update)
At equal times every arrival runs before the forward task (the stage's
contract), so one instant is: all its arrivals, then one task.
"""
import collections
import heapq

import numpy as np

import tracker_model as TM

U64 = (1 << 64) - 1
NONE32 = 0xFFFFFFFF
FIFO, RR = 0, 1
TCP, UDP = 1, 2
SENT, FORWARDED, RECEIVED, IF_DROPPED = 1 << 7, 1 << 22, 1 << 13, 1 << 14
TIME_ORDER, BAD_SOCKET, BAD_SLOT = 1, 2, 4


class Interface:
    """one host's loopback interface within one instant: per-socket deques and the qdisc"""

    def __init__(self, qdisc):
        self.qdisc = qdisc
        self.socks = {}  # socket -> deque of (priority, batch index)
        self.rr = collections.deque()  # round robin: sockets
        self.heap = []  # FIFO: (priority of the socket's next packet, arrival number of that packet, socket)

    def wants_send(self, sock, prio, i):
        q = self.socks.setdefault(sock, collections.deque())
        q.append((prio, i))
        if len(q) == 1:  # not in the qdisc: a socket is in it iff it has data
            if self.qdisc == RR:
                self.rr.append(sock)
            else:
                heapq.heappush(self.heap, (prio, i, sock))

    def pop(self):
        if self.qdisc == RR:
            if not self.rr:
                return None
            sock = self.rr.popleft()
        else:
            if not self.heap:
                return None
            _, _, sock = heapq.heappop(self.heap)
        q = self.socks[sock]
        _, i = q.popleft()
        if q:  # still has data: back into the qdisc
            if self.qdisc == RR:
                self.rr.append(sock)
            else:
                heapq.heappush(self.heap, (q[0][0], q[0][1], sock))
        return i


class LoopbackModel:
    def __init__(self, n_hosts, qdisc, max_sockets, n_slots):
        self.n_hosts, self.qdisc, self.max_sockets, self.n_slots = n_hosts, qdisc, max_sockets, n_slots
        self.assoc = {}  # (host, protocol, local port, peer ip, peer port) -> socket
        self.last = [None] * n_hosts
        self.tasks = [0] * n_hosts
        self.node_in, self.node_out = [TM._new() for _ in range(n_hosts)], [TM._new() for _ in range(n_hosts)]
        self.slot_in, self.slot_out = [TM._new() for _ in range(n_slots)], [TM._new() for _ in range(n_slots)]
        self.flags, self.n_received, self.n_no_socket = 0, 0, 0
        self.pop_lens = []  # packets each forward task popped (for the scenario's own assertions)

    def associate(self, recs):
        for a in recs:
            self.assoc[(int(a["host"]), int(a["protocol"]), int(a["local_port_be"]), int(a["peer_ip_be"]),
                        int(a["peer_port_be"]))] = int(a["socket"])

    def disassociate(self, recs):
        for a in recs:
            self.assoc.pop((int(a["host"]), int(a["protocol"]), int(a["local_port_be"]), int(a["peer_ip_be"]),
                            int(a["peer_port_be"])), None)

    def lookup(self, h, m):
        proto = int(m["protocol"])
        if proto not in (TCP, UDP):
            return NONE32
        s = self.assoc.get((h, proto, int(m["local_port_be"]), int(m["peer_ip_be"]), int(m["peer_port_be"])))
        if s is None:
            s = self.assoc.get((h, proto, int(m["local_port_be"]), 0, 0))
        return NONE32 if s is None else s

    def _count(self, node, slots, h, slot, m):
        hd, pl, rt = int(m["header_size"]), int(m["payload_size"]), bool(int(m["flags"]) & TM.RETRANS)
        TM.update(node[h], hd, pl, rt)
        if self.n_slots:
            if slot < self.n_slots:
                TM.update(slots[slot], hd, pl, rt)
            else:
                self.flags |= BAD_SLOT

    def run(self, pkts, host_ptr, rx_meta, trk_meta):
        """-> (index, socket, recv_ns, user, status), each n_pkts long"""
        n = len(pkts)
        idx, sock = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        recv, user, status = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        lim = min(int(host_ptr[self.n_hosts]), n)
        self.n_received = self.n_no_socket = 0
        for h in range(self.n_hosts):
            b, e = min(int(host_ptr[h]), lim), min(int(host_ptr[h + 1]), lim)
            e = max(e, b)
            # what flags the host, before anything of it runs
            bad, prev = 0, self.last[h]
            for i in range(b, e):
                t = int(pkts["ready_ns"][i])
                if prev is not None and t < prev:
                    bad |= TIME_ORDER
                if int(pkts["socket"][i]) >= self.max_sockets:
                    bad |= BAD_SOCKET
                prev = t
            if bad:
                self.flags |= bad
                for i in range(b, e):
                    idx[i], sock[i], recv[i], user[i], status[i] = i, NONE32, U64, rx_meta["user"][i], 0
                continue
            k, i = b, b
            while i < e:
                t = int(pkts["ready_ns"][i])
                iface = Interface(self.qdisc)  # empty between instants
                if self.last[h] != t:  # the relay is Idle: one forward task, one event id
                    self.tasks[h] += 1
                self.last[h] = t
                while i < e and int(pkts["ready_ns"][i]) == t:  # every arrival runs before the task
                    iface.wants_send(int(pkts["socket"][i]), int(pkts["priority"][i]), i)
                    i += 1
                popped = 0
                while True:  # the forward task
                    j = iface.pop()
                    if j is None:
                        break
                    popped += 1
                    m = None if trk_meta is None else trk_meta[j]
                    if m is not None:
                        self._count(self.node_out, self.slot_out, h, int(m["socket_slot"]), m)
                    s = self.lookup(h, rx_meta[j])
                    st = SENT | FORWARDED | RECEIVED
                    self.n_received += 1
                    if s == NONE32:
                        st |= IF_DROPPED
                        self.n_no_socket += 1
                    elif m is not None:
                        self._count(self.node_in, self.slot_in, h, s, m)
                    idx[k], sock[k], recv[k], user[k], status[k] = j, s, t, rx_meta["user"][j], st
                    k += 1
                self.pop_lens.append(popped)
            assert k == e
        return idx, sock, recv, user, status

    def heartbeat(self, hosts=None, slots=None):
        hs = range(self.n_hosts) if hosts is None else [int(h) for h in hosts]
        ss = range(self.n_slots) if slots is None else [int(s) for s in slots]
        out = (TM._records([self.node_in[h] for h in hs]), TM._records([self.node_out[h] for h in hs]),
               TM._records([self.slot_in[s] for s in ss]), TM._records([self.slot_out[s] for s in ss]))
        for h in hs:
            self.node_in[h], self.node_out[h] = TM._new(), TM._new()
        for s in ss:
            self.slot_in[s], self.slot_out[s] = TM._new(), TM._new()
        return out

    def status(self):
        f, self.flags = self.flags, 0
        return f, self.n_received, self.n_no_socket
