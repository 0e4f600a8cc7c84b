"""Model of the send-batch gather (srt_sendbatch_run): a lexsort by (source
host, send rank) over the batch's and the late list's forwarded non-local
packets, the meta of late packets looked up by seq in a dict, and the flag
rules of include/srt.h.  A rank gap is only detected here (the positions the
library leaves unwritten then are not modelled)."""
import numpy as np

U64 = 0xFFFFFFFFFFFFFFFF
OUT_OVERFLOW, RANK_GAP, LOG_OVERRUN, BAD_HOST = 1, 2, 4, 8
META_DTYPE = np.dtype([("src_row", "<u4"), ("dst_row", "<u4"), ("payload_size", "<u4"), ("user", "<u4")])
PKT_DTYPE = np.dtype([("src_host", "<u4"), ("src_row", "<u4"), ("dst_row", "<u4"), ("payload_size", "<u4"),
                      ("t_ns", "<u8")])
LATE_DTYPE = np.dtype([("seq", "<u8"), ("send_ns", "<u8"), ("send_rank", "<u8"), ("status", "<u4"),
                       ("src_host", "<u4")])


class SendBatchModel:
    def __init__(self, n_hosts, log_cap):
        self.n_hosts, self.log_cap, self.log = n_hosts, log_cap, {}

    def run(self, host_ptr, meta, send_ns, send_rank, seq_base, late, out_cap):
        """late: the min(count, cap) records that exist -> dict(pkts, host_ptr, user, seq, flags, n_sent)"""
        n, flags = len(send_rank), 0
        end = seq_base + n
        host = np.repeat(np.arange(self.n_hosts, dtype=np.uint32), np.diff(host_ptr.astype(np.int64)))
        rows = []  # (host, rank, send_ns, meta tuple, seq)
        for i in range(n):
            if int(send_rank[i]) == U64:
                if n - i <= self.log_cap:
                    self.log[seq_base + i] = tuple(meta[i])
            else:
                rows.append((int(host[i]), int(send_rank[i]), int(send_ns[i]), tuple(meta[i]), seq_base + i))
        for r in late:
            if int(r["send_rank"]) == U64:
                continue
            if int(r["src_host"]) >= self.n_hosts:
                flags |= BAD_HOST
                continue
            m = self.log[int(r["seq"])] if (end - int(r["seq"])) % 2**64 <= self.log_cap else None
            if m is None:
                flags |= LOG_OVERRUN
                m = (0, 0, 0, 0xFFFFFFFF)
            rows.append((int(r["src_host"]), int(r["send_rank"]), int(r["send_ns"]), m, int(r["seq"])))
        hh = np.array([x[0] for x in rows], np.int64)
        rr = np.array([x[1] for x in rows], np.uint64)
        o = np.lexsort((rr, hh))
        rows = [rows[k] for k in o]
        ptr = np.searchsorted(hh[o], np.arange(self.n_hosts + 1))
        for h in range(self.n_hosts):
            ranks = [x[1] for x in rows[ptr[h]:ptr[h + 1]]]
            if ranks and ranks != list(range(ranks[0], ranks[0] + len(ranks))):
                flags |= RANK_GAP
        n_sent = len(rows)
        if n_sent > out_cap:
            flags |= OUT_OVERFLOW
        rows = rows[:out_cap]
        pkts = np.array([(h, m[0], m[1], m[2], t) for h, _, t, m, _ in rows], PKT_DTYPE)
        return dict(pkts=pkts, host_ptr=np.minimum(ptr, out_cap).astype(np.uint32), flags=flags, n_sent=n_sent,
                    user=np.array([x[3][3] for x in rows], np.uint32), seq=np.array([x[4] for x in rows], np.uint64))
