"""A numpy and dict model of the interface receive stage (srt_deliver), written
from the reference alone:

  networkinterface_push (host/network/network_interface.c:140-202), as
  Relay::forward_until_blocked calls it for every packet it forwards
  (network/relay/mod.rs:260-270): the packet gets PDS_RCV_INTERFACE_RECEIVED
  (:151), the socket is looked up under the specific key (protocol, destination
  port, source ip, source port) (:159-163), then under the wildcard key
  (protocol, destination port, 0, 0) (:165-171), and the packet goes to that
  socket (:189) or gets PDS_RCV_INTERFACE_DROPPED (:191).  The key is a string
  of the integers as they are (:49-61), so fields compare verbatim and a peer
  of 0:0 IS the wildcard key.  networkinterface_associate asserts that the key
  is new (:84-85); networkinterface_disassociate tolerates a missing one
  (:106-114).

The relay forwards a host's packets in the order its CoDel queue holds them, a
FIFO (router/codel_queue.rs), so per host: the packets of earlier calls by
ascending seq, then the window's by ascending position.  The lookup happens at
push time, so every packet of a call sees the associations of that call.
"""
import numpy as np

FORWARDED, ROUTER_DROPPED, ENQUEUED = 1 << 22, 1 << 12, 1 << 10
RECEIVED, IF_DROPPED = 1 << 13, 1 << 14
TCP, UDP = 1, 2
OUT_OVERFLOW, LOG_OVERRUN, NOTE_OVERRUN, BAD_HOST = 1, 2, 4, 8
NONE32, NONE64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
SORT_CAP = 256

RX_META = np.dtype([("peer_ip_be", "<u4"), ("peer_port_be", "<u2"), ("local_port_be", "<u2"), ("protocol", "<u4"),
                    ("user", "<u4")])
ASSOC = np.dtype([("host", "<u4"), ("protocol", "<u4"), ("peer_ip_be", "<u4"), ("local_port_be", "<u2"),
                  ("peer_port_be", "<u2"), ("socket", "<u4")])
LATE = np.dtype([("seq", "<u8"), ("forward_ns", "<u8"), ("status", "<u4"), ("dst_host", "<u4")])
OUT_FIELDS = (("socket", np.uint32), ("forward", np.uint64), ("tag", np.uint64), ("user", np.uint32),
              ("status", np.uint32))


def key_of(a):
    return (int(a["host"]), int(a["protocol"]), int(a["local_port_be"]), int(a["peer_ip_be"]), int(a["peer_port_be"]))


def table_hash(host, peer_ip, ports, udp):
    """the device table's hash of a key (srt_deliver_step.h), for tests that build probe chains"""
    m = 0xFFFFFFFF
    h = ((host * 0x9E3779B1) ^ (peer_ip * 0x85EBCA77) ^ (ports * 0xC2B2AE3D) ^ udp) & m
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & m
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & m
    return h ^ (h >> 16)


def home_slot(a, slots):
    return table_hash(int(a["host"]), int(a["peer_ip_be"]), int(a["local_port_be"]) | int(a["peer_port_be"]) << 16,
                      int(int(a["protocol"]) == UDP)) & (slots - 1)


class DeliverModel:
    def __init__(self, n_hosts, note_cap, log_cap):
        self.n_hosts, self.note_cap, self.log_cap = n_hosts, note_cap, log_cap
        self.assoc = {}
        self.ring, self.note_end = {}, 0
        self.log = {}

    # ---- associations
    def associate(self, recs):
        """-> False, and nothing added, when a key exists (the reference asserts) or a field is out of range"""
        recs = np.asarray(recs, ASSOC)
        keys = [key_of(a) for a in recs]
        bad = any(int(a["host"]) >= self.n_hosts or int(a["socket"]) >= 1 << 31 or int(a["protocol"]) not in (TCP, UDP)
                  for a in recs)
        if bad or len(set(keys)) != len(keys) or any(k in self.assoc for k in keys):
            return False
        for k, a in zip(keys, recs):
            self.assoc[k] = int(a["socket"])
        return True

    def disassociate(self, recs):
        for a in np.asarray(recs, ASSOC):
            self.assoc.pop(key_of(a), None)

    def lookup_one(self, host, m):
        """network_interface.c:157-173"""
        proto, port = int(m["protocol"]), int(m["local_port_be"])
        s = self.assoc.get((host, proto, port, int(m["peer_ip_be"]), int(m["peer_port_be"])))
        if s is None:
            s = self.assoc.get((host, proto, port, 0, 0))
        return NONE32 if s is None else s

    def lookup(self, hosts, meta):
        return np.array([self.lookup_one(int(h), m) for h, m in zip(hosts, np.asarray(meta, RX_META))], np.uint32)

    # ---- the note ring
    def note(self, meta, tag_base):
        meta = np.asarray(meta, RX_META)
        assert tag_base >= self.note_end
        n = len(meta)
        self.note_end = tag_base + n
        for i in range(max(0, n - self.note_cap), n):
            self.ring[(tag_base + i) % self.note_cap] = meta[i].copy()

    def _meta(self, tag):
        if tag >= self.note_end or self.note_end - tag > self.note_cap:
            return None
        return self.ring[tag % self.note_cap]

    # ---- one delivery
    def run(self, dst_ptr, n_pkts, tag, status, forward, seq_base, late, out_cap, monotone=True):
        """the arrays of one inbound call (late: the LATE records that exist) -> dict(host_ptr, socket,
        forward, tag, user, status: the delivery list; flags, n_delivered, n_no_socket)"""
        n_hosts = self.n_hosts
        flags = 0
        lim = min(int(dst_ptr[n_hosts]), n_pkts)
        seg = lambda h: (min(int(dst_ptr[h]), lim), max(min(int(dst_ptr[h]), lim), min(int(dst_ptr[h + 1]), lim)))  # noqa: E731
        # packets that stay in the stage go to the log
        for i in range(lim):
            st = int(status[i])
            if (st & ENQUEUED) and not st & (FORWARDED | ROUTER_DROPPED) and lim - i <= self.log_cap:
                m = self._meta(int(tag[i]))
                if m is None:
                    flags |= NOTE_OVERRUN
                self.log[(seq_base + i) % self.log_cap] = (int(tag[i]), m)
        lates = [[] for _ in range(n_hosts)]
        for r in np.asarray(late, LATE):
            if not int(r["status"]) & FORWARDED:
                continue
            if int(r["dst_host"]) >= n_hosts:
                flags |= BAD_HOST
                continue
            lates[int(r["dst_host"])].append(r)
        recs, host_ptr = [], [0]
        for h in range(n_hosts):
            for r in sorted(lates[h], key=lambda r: int(r["seq"])):
                a = seq_base + n_pkts - int(r["seq"])
                if int(r["seq"]) >= seq_base + n_pkts or a > self.log_cap:
                    flags |= LOG_OVERRUN
                    recs.append(self._record(h, NONE64, r["forward_ns"], r["status"], None))
                    continue
                t, m = self.log.get(int(r["seq"]) % self.log_cap, (0, None))
                if m is None:
                    flags |= NOTE_OVERRUN
                recs.append(self._record(h, t, r["forward_ns"], r["status"], m))
            b, e = seg(h)
            for i in range(b, e):
                if int(status[i]) & FORWARDED:
                    m = self._meta(int(tag[i]))
                    if m is None:
                        flags |= NOTE_OVERRUN
                    recs.append(self._record(h, tag[i], forward[i], status[i], m))
            host_ptr.append(len(recs))
        total = len(recs)
        if total > out_cap:
            flags |= OUT_OVERFLOW
        host_ptr = np.minimum(np.array(host_ptr, np.uint64), out_cap).astype(np.uint32)
        out = dict(host_ptr=host_ptr, flags=flags, n_delivered=total)
        for k, (f, t) in enumerate(OUT_FIELDS):
            out[f] = np.array([r[k] for r in recs[:out_cap]], t)
        out["n_no_socket"] = int(((out["status"] & IF_DROPPED) != 0).sum())
        if monotone and not flags & OUT_OVERFLOW:
            # the relay forwards a host's packets in time order: an invariant of correct inputs
            for h in range(n_hosts):
                f = out["forward"][host_ptr[h]:host_ptr[h + 1]].astype(np.uint64)
                assert (f[1:] >= f[:-1]).all(), h
        return out

    def _record(self, h, tag, forward, status, m):
        if m is None:  # a placeholder: not looked up, the status as the router left it
            return (NONE32, int(forward), int(tag), NONE32, int(status))
        s = self.lookup_one(h, m)
        st = int(status) | RECEIVED | (IF_DROPPED if s == NONE32 else 0)
        return (s, int(forward), int(tag), int(m["user"]), st)
