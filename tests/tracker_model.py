"""Python model of the tracker's heartbeat byte counters for the internet
interface: the checker for srt_tracker (host-only and device forms).

Written from the semantics of the reference (not a transcription of the
library's step):
  host/tracker.c:24-48      Counters: 4 packet counts, 6 byte counts
  tracker.c:188-212         _tracker_updateCounters: payload > 0 is data, else
                            control; PDS_SND_TCP_RETRANSMITTED picks the
                            retransmit class
  tracker.c:214-284         addInputBytes / addOutputBytes: per host and per
                            socket, in and out (only the remote half exists on
                            the internet interface)
  tracker.c:415-433         the counter string
  tracker.c:582-627         the heartbeat logs, then clears
plus the pop-time rule of the output side: a packet is counted in the call in
which the interface popped it (it got SND_INTERFACE_SENT), fed from the
outbound model's outputs, and the input side fed from the deliver model's.
Python ints throughout; records wrap at 2^64 only when they are read out.
"""
import numpy as np

U64 = (1 << 64) - 1
NONE32 = 0xFFFFFFFF
INTERFACE_SENT = 1 << 7
RECEIVED, IF_DROPPED = 1 << 13, 1 << 14
RETRANS = 1
LOG_OVERRUN, NOTE_OVERRUN, BAD_SOCKET, BAD_HOST = 1, 2, 4, 8
TRK_META = np.dtype([("header_size", "<u4"), ("payload_size", "<u4"), ("flags", "<u4"), ("socket_slot", "<u4")])
FIELDS = ("packets_control", "bytes_control_header", "packets_control_retrans", "bytes_control_header_retrans",
          "packets_data", "bytes_data_header", "bytes_data_payload", "packets_data_retrans",
          "bytes_data_header_retrans", "bytes_data_payload_retrans")
COUNTERS = np.dtype([(k, "<u8") for k in FIELDS])


def update(rec, header, payload, retrans):
    """_tracker_updateCounters on a dict record"""
    if payload > 0:
        if retrans:
            rec["packets_data_retrans"] += 1
            rec["bytes_data_header_retrans"] += header
            rec["bytes_data_payload_retrans"] += payload
        else:
            rec["packets_data"] += 1
            rec["bytes_data_header"] += header
            rec["bytes_data_payload"] += payload
    elif retrans:
        rec["packets_control_retrans"] += 1
        rec["bytes_control_header_retrans"] += header
    else:
        rec["packets_control"] += 1
        rec["bytes_control_header"] += header


def counter_string(rec):
    """_tracker_getCounterString: totals first (gsize arithmetic wraps)"""
    g = lambda k: int(rec[k])  # noqa: E731
    packets = (g("packets_control") + g("packets_control_retrans") + g("packets_data") + g("packets_data_retrans")) & U64
    total = sum(g(k) for k in FIELDS if k.startswith("bytes")) & U64
    return ",".join(str(x) for x in [packets, total] + [g(k) for k in FIELDS])


def _new():
    return dict.fromkeys(FIELDS, 0)


def _records(recs):
    out = np.zeros(len(recs), COUNTERS)
    for k, r in enumerate(recs):
        for f in FIELDS:
            out[f][k] = r[f] & U64
    return out


class TrackerModel:
    def __init__(self, n_hosts, n_sockets, note_cap, log_cap):
        self.n_hosts, self.n_sockets, self.note_cap, self.log_cap = n_hosts, n_sockets, note_cap, log_cap
        self.node_in, self.node_out = [_new() for _ in range(n_hosts)], [_new() for _ in range(n_hosts)]
        self.sock_in, self.sock_out = [_new() for _ in range(n_sockets)], [_new() for _ in range(n_sockets)]
        self.remembered = [None] * n_hosts
        self.log, self.notes, self.note_end = {}, {}, 0
        self.flags, self.n_tx, self.n_rx = 0, 0, 0
        self.rules = dict(batch=0, late=0, late_known=0, cached=0)  # which pop-time rule counted (or skipped) a packet

    def _count(self, node, socks, h, slot, m):
        hd, pl, rt = int(m["header_size"]), int(m["payload_size"]), bool(int(m["flags"]) & RETRANS)
        update(node[h], hd, pl, rt)
        if self.n_sockets:
            if slot < self.n_sockets:
                update(socks[slot], hd, pl, rt)
            else:
                self.flags |= BAD_SOCKET

    def _logged(self, seq, seq_base, n_pkts):
        """the meta the log holds for a packet of an earlier call, or None (flagged)"""
        if seq >= seq_base or seq_base + n_pkts - seq > self.log_cap or seq not in self.log:
            self.flags |= LOG_OVERRUN
            return None
        return self.log[seq]

    def tx(self, cached_seq, host_ptr, meta, status, seq_base, late=()):
        """late: (seq, src_host) pairs in any order"""
        n_pkts = len(status)
        lim = min(int(host_ptr[self.n_hosts]), n_pkts)
        for seq, h in late:
            seq, h = int(seq), int(h)
            if h >= self.n_hosts:
                self.flags |= BAD_HOST
                continue
            if seq == self.remembered[h]:
                self.rules["late_known"] += 1  # counted when it was popped, in an earlier call
                continue
            m = self._logged(seq, seq_base, n_pkts)
            if m is not None:
                self._count(self.node_out, self.sock_out, h, int(m["socket_slot"]), m)
                self.n_tx += 1
                self.rules["late"] += 1
        for h in range(self.n_hosts):
            b, e = min(int(host_ptr[h]), lim), min(int(host_ptr[h + 1]), lim)
            for i in range(b, e):
                if int(status[i]) & INTERFACE_SENT:
                    self._count(self.node_out, self.sock_out, h, int(meta[i]["socket_slot"]), meta[i])
                    self.n_tx += 1
                    self.rules["batch"] += 1
                elif n_pkts - i <= self.log_cap:
                    self.log[seq_base + i] = meta[i].copy()
            cs = int(cached_seq[h])
            cs = None if cs == U64 else cs
            if cs is not None and cs < seq_base and cs != self.remembered[h]:
                m = self._logged(cs, seq_base, n_pkts)
                if m is not None:
                    self._count(self.node_out, self.sock_out, h, int(m["socket_slot"]), m)
                    self.n_tx += 1
                    self.rules["cached"] += 1
            self.remembered[h] = cs

    def note(self, meta, tag_base):
        assert tag_base >= self.note_end
        for i in range(len(meta)):
            self.notes[tag_base + i] = meta[i].copy()
        self.note_end = tag_base + len(meta)

    def _noted(self, tag):
        if tag >= self.note_end or self.note_end - tag > self.note_cap:
            return None
        return self.notes[tag]

    def rx(self, host_ptr, socket, tag, status, out_cap=None):
        out_cap = len(socket) if out_cap is None else out_cap
        lim = min(int(host_ptr[self.n_hosts]), out_cap)
        for h in range(self.n_hosts):
            for p in range(min(int(host_ptr[h]), lim), min(int(host_ptr[h + 1]), lim)):
                if not int(status[p]) & RECEIVED:  # a placeholder: never looked up
                    self.flags |= NOTE_OVERRUN
                    continue
                if int(socket[p]) == NONE32:
                    continue
                m = self._noted(int(tag[p]))
                if m is None:
                    self.flags |= NOTE_OVERRUN
                    continue
                self._count(self.node_in, self.sock_in, h, int(socket[p]), m)
                self.n_rx += 1

    def rx_flat(self, host, socket, meta):
        for h, s, m in zip(host, socket, meta):
            h, s = int(h), int(s)
            if h >= self.n_hosts:
                self.flags |= BAD_HOST
            elif s != NONE32:
                self._count(self.node_in, self.sock_in, h, s, m)
                self.n_rx += 1

    def heartbeat(self, hosts=None, sockets=None):
        hs = range(self.n_hosts) if hosts is None else [int(h) for h in hosts]
        ss = range(self.n_sockets) if sockets is None else [int(s) for s in sockets]
        out = (_records([self.node_in[h] for h in hs]), _records([self.node_out[h] for h in hs]),
               _records([self.sock_in[s] for s in ss]), _records([self.sock_out[s] for s in ss]))
        for h in hs:
            self.node_in[h], self.node_out[h] = _new(), _new()
        for s in ss:
            self.sock_in[s], self.sock_out[s] = _new(), _new()
        return out

    def status(self):
        f, self.flags = self.flags, 0
        return f, self.n_tx, self.n_rx
