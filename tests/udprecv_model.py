"""Plain-Python model of the UDP receive stage (srt_udprecv), restated from the
reference's socket code, one socket and one event at a time:

  UdpSocket::new            src/main/host/descriptor/socket/inet/udp.rs:60-68
                            the receive buffer's soft limit is recv_buf_size as given
  push_in_packet            udp.rs:108-168   RcvSocketProcessed; a connected socket drops a
                            packet from another source (:116-135); a buffer without space
                            drops (:140-143); else the message joins the buffer (:160-165)
  recvmsg                   udp.rs:477-572   pop or peek the front message (:502-516),
                            copy min(len, size) (:519), MSG_TRUNC returns the full size
                            (:527-532), msg_flags (:534-535), the last receive time, for
                            peeks too (:537-538); EWOULDBLOCK without MSG_DONTWAIT blocks
                            on READABLE (:550-568)
  SO_RCVBUF                 udp.rs:900-925   doubled, at least 2048, at most 2^28
  MessageBuffer             udp.rs:1056-1134 len_bytes counts payload bytes, has_space is
                            len_bytes < soft_limit, so the limit is soft and a zero-length
                            message never fills the buffer

plus the library's own rules around them (include/srt.h, "UDP socket receive
stage"): the window [previous until, until), pushes before reads at equal times,
the blocked read completing after the pushes of the instant that made the socket
readable, the note ring, the ring of messages kept across calls, and the flags.
Nothing here is shared with the C++ step."""
from collections import Counter, deque

import numpy as np

U64 = (1 << 64) - 1
NO_SOCKET = 0xFFFFFFFF
RECEIVED = 1 << 13
PROCESSED, DROPPED, BUFFERED = 1 << 15, 1 << 16, 1 << 18
PEEK, TRUNC, WAIT = 0x2, 0x20, 0x10000
MSG_TRUNC = 0x20
NOT_TAKEN, DONE, ARMED = 0, 1, 2
EWOULDBLOCK, EBADF = 11, 9
OPEN, CLOSE, SET_PEER, SET_RCVBUF = 1, 2, 3, 4
F_RING_OVERFLOW, F_LATE_OVERFLOW, F_NOTE_OVERRUN, F_BAD_SOCKET, F_READ_ORDER, F_ARMED_TWICE = 1, 2, 4, 8, 16, 32
MARK_RING, MARK_NOTE = 1, 2

META = np.dtype([("src_ip_be", "<u4"), ("src_port_be", "<u2"), ("reserved", "<u2"), ("payload_size", "<u4"),
                 ("user", "<u4")])
READ = np.dtype([("time_ns", "<u8"), ("slot", "<u4"), ("len", "<u4"), ("flags", "<u4"), ("user", "<u4")])
RESULT = np.dtype([("tag", "<u8"), ("recv_ns", "<u8"), ("complete_ns", "<u8"), ("return_val", "<i8"),
                   ("status", "<u4"), ("msg_flags", "<u4"), ("src_ip_be", "<u4"), ("src_port_be", "<u2"),
                   ("reserved", "<u2"), ("user", "<u4"), ("read_user", "<u4")])
LATE = np.dtype([("seq", "<u8"), ("result", RESULT)])
OP = np.dtype([("op", "<u4"), ("slot", "<u4"), ("value", "<u8")])
STATE = np.dtype([("len_bytes", "<u8"), ("soft_limit", "<u8"), ("last_read_recv_ns", "<u8"), ("armed_seq", "<u8"),
                  ("n_msgs", "<u4"), ("peer_ip_be", "<u4"), ("peer_port_be", "<u2"), ("open", "u1"),
                  ("overflow", "u1"), ("reserved", "<u4")])


def rcvbuf_limit(optval):
    """udp.rs:910-924"""
    return min(max(int(optval) * 2, 2048), 1 << 28)


class Socket:
    def __init__(self, host):
        self.host = host
        self.open = False
        self.reset(0)

    def reset(self, limit):
        self.msgs = deque()  # (tag, recv_ns, size, src_ip, src_port, user)
        self.len_bytes = 0
        self.soft_limit = int(limit)
        self.peer = None
        self.last_read_recv_ns = U64
        self.armed = None  # (seq, len, flags, user)
        self.overflow = 0

    def has_space(self):
        return self.len_bytes < self.soft_limit


class Model:
    def __init__(self, socket_ptr, ring_cap, note_cap):
        sp = [int(x) for x in socket_ptr]
        self.n_hosts, self.n_sockets = len(sp) - 1, sp[-1]
        self.socket_ptr = sp
        self.socks = [Socket(h) for h in range(self.n_hosts) for _ in range(sp[h], sp[h + 1])]
        self.ring_cap, self.note_cap = int(ring_cap), int(note_cap)
        self.notes = {}
        self.note_end = 0
        self.flags = 0
        self.n_proc = self.n_buf = self.n_drop = 0
        self.read_base = 0
        self.prev_until = 0
        self.stats = Counter()  # what happened, for the scenarios' own checks

    # ---- between runs
    def config(self, ops):
        ops = np.asarray(ops, OP).reshape(-1)
        if any(int(o["slot"]) >= self.n_sockets or not OPEN <= int(o["op"]) <= SET_RCVBUF for o in ops):
            raise ValueError("bad slot or op: nothing changed")
        for o in ops:
            s, v = self.socks[int(o["slot"])], int(o["value"])
            if o["op"] == OPEN:
                s.reset(v)
                s.open = True
            elif not s.open:
                continue
            elif o["op"] == CLOSE:
                s.reset(0)
                s.open = False
            elif o["op"] == SET_PEER:
                s.peer = (v & 0xFFFFFFFF, (v >> 32) & 0xFFFF) if v & 0xFFFFFFFFFFFF else None
            else:
                s.soft_limit = rcvbuf_limit(v)

    def note(self, meta, tag_base):
        meta = np.asarray(meta, META).reshape(-1)
        assert tag_base >= self.note_end
        for i, m in enumerate(meta):
            self.notes[tag_base + i] = m.copy()
        self.note_end = tag_base + len(meta)
        for t in [t for t in self.notes if self.note_end - t > self.note_cap]:
            del self.notes[t]

    def _note(self, tag):
        if tag < self.note_end and self.note_end - tag <= self.note_cap:
            return self.notes[tag]
        return None

    # ---- one socket's calls
    def _recv(self, s, length, flags, at, read_user):
        """recvmsg on a non-empty buffer (udp.rs:502-545)"""
        tag, recv_ns, size, ip, port, user = s.msgs[0]
        self.stats["read_same_call" if recv_ns >= self.prev_until else "read_carried"] += 1
        self.stats["peek"] += bool(flags & PEEK)
        self.stats["truncated"] += length < size
        if not flags & PEEK:
            s.msgs.popleft()
            s.len_bytes -= size
        copied = min(length, size)
        res = np.zeros((), RESULT)
        res["tag"], res["recv_ns"], res["complete_ns"] = tag, recv_ns, at
        res["return_val"] = size if flags & TRUNC else copied
        res["status"] = DONE
        res["msg_flags"] = MSG_TRUNC if copied < size else 0
        res["src_ip_be"], res["src_port_be"], res["user"], res["read_user"] = ip, port, user, read_user
        s.last_read_recv_ns = recv_ns
        return res

    def _push(self, s, k, tag, forward_ns, status, rx):
        """push_in_packet (udp.rs:108-168); True when the buffer turned non-empty"""
        m = self._note(tag)
        if m is None:
            self.flags |= F_NOTE_OVERRUN
            s.overflow |= MARK_NOTE
            return False
        bits = PROCESSED
        self.n_proc += 1
        turned = False
        src = (int(m["src_ip_be"]), int(m["src_port_be"]))
        self.stats["zero_length"] += int(m["payload_size"]) == 0
        if s.peer is not None and s.peer != src:
            bits |= DROPPED
            self.n_drop += 1
            self.stats["drop_peer"] += 1
        elif not s.has_space():
            bits |= DROPPED
            self.n_drop += 1
            self.stats["drop_full"] += 1
        else:
            bits |= BUFFERED
            self.n_buf += 1
            turned = not s.msgs
            s.msgs.append((int(tag), int(forward_ns), int(m["payload_size"]), src[0], src[1], int(m["user"])))
            s.len_bytes += int(m["payload_size"])
        rx[k] = status | bits
        return turned

    def run(self, out_host_ptr, out_socket, out_forward_ns, out_tag, out_status, read_host_ptr, reads, until_ns,
            late_cap=1 << 30):
        """-> dict(rx_status [walked], results [n_reads], late (sorted by seq), first_readable [n_sockets], seq_base)"""
        assert until_ns >= self.prev_until
        nh = self.n_hosts
        out_cap = len(out_socket)
        lim = min(int(out_host_ptr[nh]), out_cap)
        reads = np.zeros(0, READ) if reads is None else np.asarray(reads, READ).reshape(-1)
        n_reads = len(reads)
        rlim = min(int(read_host_ptr[nh]), n_reads) if n_reads else 0
        rx = np.array(out_status[:lim], np.uint32)
        results = np.zeros(n_reads, RESULT)
        late = []
        first = np.full(self.n_sockets, U64, np.uint64)

        def seg(ptr, top, h):
            b, e = min(int(ptr[h]), top), min(int(ptr[h + 1]), top)
            return b, max(b, e)

        for h in range(nh):
            events = {}  # slot -> ([pushes k], [reads j])
            b, e = seg(out_host_ptr, lim, h)
            for k in range(b, e):
                sock = int(out_socket[k])
                if not int(out_status[k]) & RECEIVED or sock >= self.n_sockets:
                    continue  # no socket, a placeholder
                s = self.socks[sock]
                if not s.open or s.host != h:
                    self.stats["foreign"] += 1
                    continue  # foreign to the stage
                events.setdefault(sock, ([], []))[0].append(k)
            rb, re = seg(read_host_ptr, rlim, h) if n_reads else (0, 0)
            rmax = 0
            for j in range(rb, re):
                t, slot = int(reads[j]["time_ns"]), int(reads[j]["slot"])
                in_win = self.prev_until <= t < until_ns
                if slot >= self.n_sockets or not self.socks[slot].open or self.socks[slot].host != h:
                    self.flags |= F_BAD_SOCKET
                    results[j]["status"], results[j]["return_val"] = DONE, -EBADF
                    results[j]["complete_ns"], results[j]["read_user"] = t, reads[j]["user"]
                elif not (in_win and t >= rmax):
                    self.flags |= F_READ_ORDER
                else:
                    events.setdefault(slot, ([], []))[1].append(j)
                if in_win:
                    rmax = max(rmax, t)
            for slot, (pushes, rds) in events.items():
                self._socket(self.socks[slot], slot, pushes, rds, out_forward_ns, out_tag, out_status, reads, rx,
                             results, late, first)
        for s in self.socks:  # what stays buffered beyond the ring is lost
            if s.open and len(s.msgs) > self.ring_cap:
                self.flags |= F_RING_OVERFLOW
                s.overflow |= MARK_RING
                while len(s.msgs) > self.ring_cap:
                    s.msgs.pop()
        if len(late) > late_cap:
            self.flags |= F_LATE_OVERFLOW
        late.sort(key=lambda r: r[0])
        late_a = np.zeros(len(late), LATE)
        for i, (seq, res) in enumerate(late):
            late_a[i]["seq"], late_a[i]["result"] = seq, res
        base = self.read_base
        self.read_base += n_reads
        self.prev_until = until_ns
        return dict(rx_status=rx, results=results, late=late_a, first_readable=first, seq_base=base)

    def _socket(self, s, slot, pushes, rds, fwd, tags, status, reads, rx, results, late, first):
        armed_here = None
        t_ready = self.prev_until
        i = j = 0

        def complete():
            nonlocal armed_here
            seq, length, flags, user = s.armed
            res = self._recv(s, length, flags, t_ready, user)
            if armed_here is not None:
                results[armed_here] = res
                self.stats["armed_same_call"] += 1
            else:
                late.append((seq, res))
                self.stats["armed_later_call"] += 1
            s.armed = None
            armed_here = None

        while i < len(pushes) or j < len(rds):
            is_push = i < len(pushes) and (j >= len(rds) or int(fwd[pushes[i]]) <= int(reads[rds[j]]["time_ns"]))
            if is_push:
                k = pushes[i]
                t = int(fwd[k])
                if s.armed is not None and s.msgs and t > t_ready:
                    complete()
                if self._push(s, k, int(tags[k]), t, int(status[k]), rx):
                    t_ready = t
                    if first[slot] == U64:
                        first[slot] = t
                i += 1
                continue
            if s.armed is not None and s.msgs:
                complete()
            r = reads[rds[j]]
            t, flags = int(r["time_ns"]), int(r["flags"])
            if s.msgs:
                results[rds[j]] = self._recv(s, int(r["len"]), flags, t, int(r["user"]))
            elif flags & WAIT and s.armed is None:
                s.armed = (self.read_base + rds[j], int(r["len"]), flags, int(r["user"]))
                armed_here = rds[j]
                results[rds[j]]["status"], results[rds[j]]["read_user"] = ARMED, r["user"]
            else:
                if flags & WAIT:
                    self.flags |= F_ARMED_TWICE
                self.stats["ewouldblock"] += 1
                results[rds[j]]["status"], results[rds[j]]["return_val"] = DONE, -EWOULDBLOCK
                results[rds[j]]["complete_ns"], results[rds[j]]["read_user"] = t, r["user"]
            j += 1
        if s.armed is not None and s.msgs:
            complete()

    # ---- what the library reports
    def status(self):
        f = self.flags
        self.flags = 0
        return f, self.n_proc, self.n_buf, self.n_drop

    def state(self):
        out = np.zeros(self.n_sockets, STATE)
        for x, s in enumerate(self.socks):
            out[x]["len_bytes"], out[x]["soft_limit"] = s.len_bytes, s.soft_limit
            out[x]["last_read_recv_ns"] = s.last_read_recv_ns
            out[x]["armed_seq"] = s.armed[0] if s.armed is not None else U64
            out[x]["n_msgs"] = len(s.msgs)
            if s.peer is not None:
                out[x]["peer_ip_be"], out[x]["peer_port_be"] = s.peer
            out[x]["open"], out[x]["overflow"] = int(s.open), s.overflow
        return out
