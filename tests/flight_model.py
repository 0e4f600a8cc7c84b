"""Numpy model of the in-flight store (srt_flight): a list of records, the
window of a pop by np.lexsort within each destination, the flags and the
void-pop rule of include/srt.h.  It shares no code with the library."""
import numpy as np

POOL_OVERFLOW, OUT_OVERFLOW, BAD_HOST, LATE_PUSH, TIME_REGRESSION = 1, 2, 4, 8, 16
SENT = 1 << 8
FIELDS = ("deliver", "src", "event_id", "dst", "size", "tag")
REC = np.dtype([("deliver", "<u8"), ("src", "<u4"), ("event_id", "<u8"), ("dst", "<u4"), ("size", "<u4"),
                ("tag", "<u8")])


class FlightModel:
    def __init__(self, n_dst_hosts, pool_cap):
        self.n_dst, self.cap = n_dst_hosts, pool_cap
        self.recs = np.zeros(0, REC)
        self.flags = 0
        self.n_lost = 0
        self.n_popped = 0
        self.last_until = 0
        self.tag_next = 0

    def push(self, host_ptr, flags, deliver, dst_host, event_id, total_size, tag=None):
        """-> the push's tag base"""
        host_ptr = np.asarray(host_ptr, np.int64)
        n = len(flags)
        base = self.tag_next
        self.tag_next += n
        lim = min(int(host_ptr[-1]), n)
        hp = np.minimum(host_ptr, lim)
        src = np.full(n, -1, np.int64)
        for h in range(len(hp) - 1):
            src[hp[h]:max(hp[h], hp[h + 1])] = h
        sent = (np.asarray(flags, np.uint32) == SENT) & (src >= 0)
        bad = sent & (np.asarray(dst_host, np.uint32) >= self.n_dst)
        if bad.any():
            self.flags |= BAD_HOST
        take = np.flatnonzero(sent & ~bad)
        if (np.asarray(deliver, np.uint64)[take] < np.uint64(self.last_until)).any():
            self.flags |= LATE_PUSH
        room = self.cap - len(self.recs)
        if len(take) > room:
            self.flags |= POOL_OVERFLOW
            self.n_lost += len(take) - room
            take = take[:room]  # which ones are lost is unspecified on the device; the host form keeps the first
        r = np.zeros(len(take), REC)
        r["deliver"] = np.asarray(deliver, np.uint64)[take]
        r["src"] = src[take]
        r["event_id"] = np.asarray(event_id, np.uint64)[take]
        r["dst"] = np.asarray(dst_host, np.uint32)[take]
        r["size"] = np.asarray(total_size, np.uint32)[take]
        r["tag"] = np.asarray(tag, np.uint64)[take] if tag is not None else np.uint64(base) + take.astype(np.uint64)
        self.recs = np.concatenate([self.recs, r])
        return base

    def pop(self, until_ns, out_cap):
        """-> dict(dst_ptr, order, deliver, size, src, event_id, tag), the arrays n_popped long"""
        if until_ns < self.last_until:
            self.flags |= TIME_REGRESSION
        self.last_until = max(self.last_until, until_ns)
        due = self.recs["deliver"] < np.uint64(until_ns)
        n_due = int(due.sum())
        self.n_popped = n_due
        if n_due > out_cap:
            self.flags |= OUT_OVERFLOW
            w = np.zeros(0, REC)
            dst_ptr = np.zeros(self.n_dst + 1, np.uint32)
        else:
            w = self.recs[due]
            self.recs = self.recs[~due]
            w = w[np.lexsort((w["event_id"], w["src"], w["deliver"], w["dst"]))]
            dst_ptr = np.searchsorted(w["dst"], np.arange(self.n_dst + 1)).astype(np.uint32)
        return dict(dst_ptr=dst_ptr, order=np.arange(len(w), dtype=np.uint32), deliver=w["deliver"].copy(),
                    size=w["size"].copy(), src=w["src"].copy(), event_id=w["event_id"].copy(), tag=w["tag"].copy())

    def status(self):
        """-> (flags, n_popped, n_stored, n_lost); clears the flags"""
        f, self.flags = self.flags, 0
        return f, self.n_popped, len(self.recs), self.n_lost
