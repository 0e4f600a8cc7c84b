"""What the tracker stage's tests share: a generator of seven windows whose
output side comes from the outbound model (throttled hosts, so that late lists
and packets cached across a call boundary occur) and whose input side is the
deliver scenario's delivery lists (the deliver model's); a runner that feeds
srt_tracker (host-only or on the device) from numpy arrays, the output side
through the real srt_outbound -> srt_outbound_cached_seq -> srt_tracker_tx chain;
and the hand-made cases both forms must pass."""
import ctypes as C
import functools

import numpy as np

import deliver_model as DM
import deliver_scenario as D
import tracker_model as TM
from outbound_model import CACHED, FIFO, FORWARDED, INTERFACE_SENT, OutboundModel
from outbound_scenario import LATE_DTYPE, OUT_PKT_DTYPE

U64 = TM.U64
MS = 1_000_000
W_NS = 20 * MS
T0 = 1_000 * MS
N_WIN = D.N_WIN + 1   # seven windows; the last has no arrivals and drains
DENSE, SPARSE = D.DENSE, D.SPARSE
SOCKS = 4             # sockets a host, slot = host * SOCKS + socket
BANDWIDTHS = (20_000, 60_000, 2_000_000, 125_000_000)
HEARTBEATS = (3, 7)   # after these windows: a subset of hosts and slots, then all
SENT = INTERFACE_SENT
POPPED_CACHED, POPPED_FWD = INTERFACE_SENT | CACHED, INTERFACE_SENT | FORWARDED
RX_HIT, RX_MISS = D.FWD | DM.RECEIVED, D.FWD | DM.RECEIVED | DM.IF_DROPPED


def rand_meta(rng, n, slots=None):
    """control and data, first and retransmitted, in about equal parts"""
    m = np.zeros(n, TM.TRK_META)
    m["header_size"] = rng.choice(np.array([20, 32, 40, 60], np.uint32), size=n)
    m["payload_size"] = np.where(rng.random(n) < 0.4, 0, rng.integers(1, 1441, size=n))
    m["flags"] = (rng.random(n) < 0.3).astype(np.uint32)
    if slots is not None:
        m["socket_slot"] = slots
    return m


@functools.lru_cache(maxsize=None)
def scenario(n_hosts, shape, seed=33):
    """-> dict(bw, calls, rx): calls[w] = the outbound call of window w (pkts, host_ptr, until, meta) with
    the outbound model's results (status, late, cached_seq, base); rx = the deliver scenario's steps
    with the deliver model's lists and a tracker meta for every tag"""
    rng = np.random.default_rng(seed + n_hosts + (1000 if shape == SPARSE else 0))
    bw = rng.choice(np.array(BANDWIDTHS, np.uint64), size=n_hosts, p=[0.2, 0.3, 0.2, 0.3])
    bw[0] = 60_000
    om = OutboundModel(bw, FIFO, SOCKS)
    prio = np.zeros(n_hosts, np.int64)
    calls = []
    for w in range(N_WIN):
        if w == N_WIN - 1:
            per = np.zeros(n_hosts, np.int64)
        elif shape == DENSE:
            per = rng.integers(0, 201, size=n_hosts)
            per[rng.random(n_hosts) < 0.15] = 0
            per[0] = 150 + int(rng.integers(0, 50))
        else:
            per = rng.integers(0, 3, size=n_hosts)
        n = int(per.sum())
        lo, until = T0 + w * W_NS, T0 + (w + 1) * W_NS if w < N_WIN - 1 else T0 + 12 * W_NS
        host_ptr = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
        host = np.repeat(np.arange(n_hosts), per)
        pk = np.zeros(n, OUT_PKT_DTYPE)
        sock = rng.integers(0, SOCKS, size=n)
        meta = rand_meta(rng, n, host * SOCKS + sock)
        for h in range(n_hosts):
            b, e = int(host_ptr[h]), int(host_ptr[h + 1])
            pk["ready_ns"][b:e] = np.sort(lo + rng.integers(0, 64, size=e - b) * (W_NS // 64))
            pk["priority"][b:e] = prio[h] + 1 + np.arange(e - b)
            prio[h] += e - b
        pk["total_size"] = meta["header_size"] + meta["payload_size"]
        pk["socket"] = sock
        pk["flags"] = (rng.random(n) < 0.03).astype(np.uint32)
        status, _, _, late, base = om.run(pk, host_ptr, until, 0)
        cached = np.array([U64 if h.cached is None else h.cached.tag for h in om.hosts], np.uint64)
        calls.append(dict(pkts=pk, host_ptr=host_ptr, until=until, meta=meta, status=status, base=base,
                          late=[(x[0], x[4]) for x in late], cached_seq=cached))
    dsc = D.scenario(n_hosts, shape)
    trk_meta = rand_meta(np.random.default_rng(seed + 7), dsc["total"])
    return dict(bw=bw, calls=calls, rx_steps=dsc["steps"], rx_lists=D.model_scenario(n_hosts, shape), rx_meta=trk_meta,
                rx_cap=dsc["cap"] + dsc["late_cap"], n_sockets=max(SOCKS * n_hosts, 12 * n_hosts),
                note_cap=dsc["total"], log_cap=sum(len(c["pkts"]) for c in calls) + 1,
                late_cap=sum(len(c["pkts"]) for c in calls) + 1,
                queue_cap=int(sum(np.diff(c["host_ptr"].astype(np.int64)) for c in calls).max()) + 1)


class Runner:
    """srt_tracker fed from numpy arrays; plan=None: the host-only instance"""

    def __init__(self, plan, n_hosts, n_sockets, note_cap, log_cap):
        from shadow_amd import Tracker

        self.plan, self.n_hosts = plan, n_hosts
        self.trk = Tracker(plan, n_hosts, n_sockets, note_cap, log_cap)

    def close(self):
        self.trk.close()

    def _in(self, a):
        a = np.ascontiguousarray(a)
        if self.plan is None:
            return a.view(np.uint8).reshape(-1) if a.dtype.fields else a
        import torch

        if a.dtype.fields:
            return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
        signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype)
        return torch.from_numpy(a.view(signed).copy()).to("cuda:0")

    def tx(self, cached_seq, host_ptr, meta, status, seq_base, late=(), late_cap=None):
        """late: (seq, src_host) pairs"""
        recs = np.zeros(max(len(late), late_cap or 0), LATE_DTYPE)
        for k, (seq, h) in enumerate(late):
            recs[k]["seq"], recs[k]["src_host"], recs[k]["status"] = seq, h, POPPED_FWD
        late_cap = len(recs) if late_cap is None else late_cap
        self.trk.tx(self._in(np.asarray(cached_seq, np.uint64)), self._in(np.asarray(host_ptr, np.uint32)),
                    self._in(np.asarray(meta, TM.TRK_META)), self._in(np.asarray(status, np.uint32)), seq_base,
                    self._in(recs[:late_cap]) if late_cap else None,
                    self._in(np.array([len(late)], np.uint32)) if late_cap else None)

    def tx_chain(self, relay, call, late_cap):
        """srt_outbound_run -> srt_outbound_cached_seq -> srt_tracker_tx on the relay's own arrays, no
        status call and no read-back between the three"""
        n = len(call["pkts"])
        z = lambda k, dt: self._in(np.zeros(k, dt))  # noqa: E731
        st, sn, rk = z(n, np.uint32), z(n, np.uint64), z(n, np.uint64)
        late, cnt, cs = z(late_cap * 32, np.uint8), z(1, np.uint32), z(self.n_hosts, np.uint64)
        hp = self._in(call["host_ptr"])
        base = relay.run(self._in(call["pkts"]) if n else z(32, np.uint8), hp, call["until"], 0, st, sn, rk, late, cnt)
        relay.cached_seq(cs)
        self.trk.tx(cs, hp, self._in(call["meta"]) if n else z(16, np.uint8)[:0], st, base, late, cnt)
        return base

    def note(self, meta, tag_base):
        self.trk.note(self._in(np.asarray(meta, TM.TRK_META)), tag_base)

    def rx(self, host_ptr, socket, tag, status, out_cap=None):
        """the arrays padded to out_cap with values that would count if the walk ran past the list"""
        n = len(socket)
        out_cap = n if out_cap is None else out_cap
        pad = lambda a, dt, fill: np.concatenate([np.asarray(a, dt)[:out_cap],  # noqa: E731
                                                  np.full(max(out_cap - n, 0), fill, dt)])
        self.trk.rx(self._in(np.asarray(host_ptr, np.uint32)), self._in(pad(socket, np.uint32, 0)),
                    self._in(pad(tag, np.uint64, 0)), self._in(pad(status, np.uint32, RX_HIT)))

    def rx_flat(self, host, socket, meta):
        self.trk.rx_flat(self._in(np.asarray(host, np.uint32)), self._in(np.asarray(socket, np.uint32)),
                         self._in(np.asarray(meta, TM.TRK_META)))

    def heartbeat(self, hosts=None, sockets=None):
        return self.trk.heartbeat(hosts, sockets)

    def status(self):
        """-> (flags, n_tx_counted, n_rx_counted, message)"""
        from shadow_amd import _lib

        f, a, b, err = C.c_uint32(), C.c_uint64(), C.c_uint64(), _lib.SrtErr()
        rc = _lib.lib().srt_tracker_status(self.trk._h, C.byref(f), C.byref(a), C.byref(b), C.byref(err))
        assert rc == (_lib.SRT_ERR_INVALID if f.value else _lib.SRT_OK), (rc, err.msg)
        return f.value, a.value, b.value, err.msg.decode()


def same_records(a, b, what=""):
    assert len(a) == len(b) == 4, what
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype == TM.COUNTERS and x.tobytes() == y.tobytes(), (what, k, x, y)


def _walk(sc, tx, note, rx, heartbeat, status):
    """the seven windows: tx, then the window's notes and its delivery list; -> every heartbeat's records
    and the final status"""
    n_hosts = len(sc["bw"])
    runs = [s for s in sc["rx_steps"] if s[0] in ("note", "run")]
    beats, k = [], 0
    for w, call in enumerate(sc["calls"]):
        tx(call)
        while runs:
            st = runs.pop(0)
            if st[0] == "note":
                note(sc["rx_meta"][st[2]:st[2] + len(st[1])], st[2])
                continue
            mo = sc["rx_lists"][k]
            rx(mo["host_ptr"], mo["socket"], mo["tag"], mo["status"])
            k += 1
            break
        if w + 1 in HEARTBEATS:
            beats.append(heartbeat(np.arange(0, n_hosts, 3), np.arange(1, sc["n_sockets"], 5)))
            beats.append(heartbeat(None, None))
    assert k == len(sc["rx_lists"]) == N_WIN and not runs
    return beats, status()


def run_scenario(plan, n_hosts, shape):
    from shadow_amd.plan import OutboundRelay

    sc = scenario(n_hosts, shape)
    r = Runner(plan, n_hosts, sc["n_sockets"], sc["note_cap"], sc["log_cap"])
    relay = OutboundRelay(plan, sc["bw"], FIFO, SOCKS, sc["queue_cap"])
    try:
        def tx(call):
            assert r.tx_chain(relay, call, sc["late_cap"]) == call["base"]

        beats, st = _walk(sc, tx, r.note, lambda *a: r.rx(*a, out_cap=sc["rx_cap"]), r.heartbeat, r.status)
        assert relay.status()[0] == 0
        return beats, st[:3]
    finally:
        relay.close()
        r.close()


@functools.lru_cache(maxsize=None)
def model_scenario(n_hosts, shape):
    """-> (heartbeats, status, the model): fed the outbound model's and the deliver model's outputs"""
    sc = scenario(n_hosts, shape)
    m = TM.TrackerModel(n_hosts, sc["n_sockets"], sc["note_cap"], sc["log_cap"])
    beats, st = _walk(sc, lambda c: m.tx(c["cached_seq"], c["host_ptr"], c["meta"], c["status"], c["base"], c["late"]),
                      m.note, m.rx, m.heartbeat, m.status)
    return beats, st, m


def assert_scenario_is_not_empty(n_hosts, shape):
    """the model, fed the outbound and deliver models, counts in every class, in and out, per host and per
    slot, and (dense) meets every pop-time rule"""
    beats, st, m = model_scenario(n_hosts, shape)
    assert st[0] == 0 and st[1] > 0 and st[2] > 0, st
    for k in range(4):  # node in, node out, sock in, sock out over the all-hosts heartbeats
        tot = {f: sum(int(b[k][f].sum()) for b in beats[1::2]) for f in TM.FIELDS}
        assert all(v > 0 for v in tot.values()) or (shape == SPARSE and n_hosts < 63), (k, tot)
    if shape == DENSE:
        assert all(m.rules[r] > 0 for r in ("batch", "late", "late_known", "cached")), m.rules
    return m.rules


# ------------------------------------------------------------ hand-made cases
class _Pair:
    """the same calls through a runner and the model; heartbeat() compares and returns the records"""

    def __init__(self, make, n_hosts, n_sockets=4, note_cap=64, log_cap=64):
        self.r, self.m = make(n_hosts, n_sockets, note_cap, log_cap), TM.TrackerModel(n_hosts, n_sockets, note_cap, log_cap)
        self.n_hosts = n_hosts

    def tx(self, cached_seq, host_ptr, meta, status, seq_base, late=(), **kw):
        self.r.tx(cached_seq, host_ptr, meta, status, seq_base, late, **kw)
        self.m.tx(np.asarray(cached_seq, np.uint64), host_ptr, np.asarray(meta, TM.TRK_META), status, seq_base, late)

    def note(self, meta, tag_base):
        self.r.note(meta, tag_base)
        self.m.note(np.asarray(meta, TM.TRK_META), tag_base)

    def rx(self, host_ptr, socket, tag, status, out_cap=None):
        self.r.rx(host_ptr, socket, tag, status, out_cap)
        self.m.rx(host_ptr, socket, tag, status)

    def rx_flat(self, host, socket, meta):
        self.r.rx_flat(host, socket, meta)
        self.m.rx_flat(host, socket, np.asarray(meta, TM.TRK_META))

    def status(self):
        a, b = self.r.status(), self.m.status()
        assert a[:3] == b, (a, b)
        return a

    def heartbeat(self, hosts=None, sockets=None):
        a, b = self.r.heartbeat(hosts, sockets), self.m.heartbeat(hosts, sockets)
        same_records(a, b)
        return a

    def close(self):
        self.r.close()


def meta(*rows):
    """(header, payload, flags, slot) rows -> TRK_META records"""
    return np.array(list(rows), TM.TRK_META)


def total(rec):
    return {f: int(rec[f].sum()) for f in TM.FIELDS if int(rec[f].sum())}


NONE = U64


def case_oversize_cached_three_calls(make):
    """a packet popped in call 1 and held by the relay for three calls (oversize for its bucket): once"""
    p = _Pair(make, 2)
    try:
        p.tx([0, NONE], [0, 1, 1], meta((40, 2000, 0, 1)), [POPPED_CACHED], 0)
        assert p.status()[1] == 1
        for base in (1, 1, 1):
            p.tx([0, NONE], [0, 0, 0], meta(), [], base)
        assert p.status()[:3] == (0, 1, 0)
        _, out, _, sout = p.heartbeat()
        assert total(out[0:1]) == dict(packets_data=1, bytes_data_header=40, bytes_data_payload=2000)
        assert total(sout[1:2]) == total(out[0:1]) and not total(out[1:2])
    finally:
        p.close()


def case_popped_after_queuing(make):
    """queued in call 1 (status 0), popped and cached at the end of call 2 (in neither the batch nor the
    late list), forwarded in call 3 (a late record): counted in call 2"""
    p = _Pair(make, 1)
    try:
        p.tx([NONE], [0, 2], meta((20, 0, 0, 0), (32, 100, 1, 3)), [POPPED_FWD, 0], 10)
        assert p.status()[1] == 1
        p.heartbeat()
        p.tx([11], [0, 1], meta((60, 7, 0, 2)), [0], 12)  # seq 11 is the cached packet now; seq 12 queues
        assert p.status()[1] == 2
        _, out, _, sout = p.heartbeat()
        assert total(out) == dict(packets_data_retrans=1, bytes_data_header_retrans=32, bytes_data_payload_retrans=100)
        assert total(sout[3:4]) == total(out)
        p.tx([NONE], [0, 0], meta(), [], 13, late=[(11, 0), (12, 0)])  # 11: known; 12: popped and forwarded here
        assert p.status()[:3] == (0, 3, 0)
        _, out, _, _ = p.heartbeat()
        assert total(out) == dict(packets_data=1, bytes_data_header=60, bytes_data_payload=7)
    finally:
        p.close()


def case_one_packet_per_class(make):
    p = _Pair(make, 3, n_sockets=2)
    try:
        ms = meta((20, 0, 0, 0), (32, 0, 1, 0), (40, 1, 0, 1), (60, 1440, 1, 1))
        p.tx([NONE] * 3, [0, 0, 4, 4], ms, [SENT, POPPED_FWD, POPPED_CACHED, POPPED_FWD | CACHED], 0)
        p.note(ms, 0)
        p.rx([0, 0, 0, 4], [1, 1, 0, 0], [0, 1, 2, 3], [RX_HIT] * 4)
        assert p.status()[:3] == (0, 4, 4)
        nin, nout, sin, sout = p.heartbeat()
        want = dict(packets_control=1, bytes_control_header=20, packets_control_retrans=1, bytes_control_header_retrans=32,
                    packets_data=1, bytes_data_header=40, bytes_data_payload=1, packets_data_retrans=1,
                    bytes_data_header_retrans=60, bytes_data_payload_retrans=1440)
        assert total(nout[1:2]) == want and total(nin[2:3]) == want and total(nout) == want and total(nin) == want
        assert total(sout[0:1]) == dict(packets_control=1, bytes_control_header=20, packets_control_retrans=1,
                                        bytes_control_header_retrans=32)
        assert total(sin[1:2]) == total(sout[0:1]) and total(sin) == want and total(sout) == want
        assert all(not total(x) for x in p.heartbeat())  # cleared
    finally:
        p.close()


def case_carry_past_32_bits(make):
    p = _Pair(make, 1, n_sockets=1)
    try:
        ms = meta(*[(0xFFFFFFFF, 0xFFFFFFFF, 0, 0)] * 3)
        p.tx([NONE], [0, 3], ms, [SENT] * 3, 0)
        p.note(ms, 0)
        p.rx([0, 3], [0, 0, 0], [0, 1, 2], [RX_HIT] * 3)
        p.rx_flat([0, 0, 0], [0, 0, 0], ms)
        nin, nout, sin, sout = p.heartbeat()
        for rec, k in ((nout, 1), (sout, 1), (nin, 2), (sin, 2)):
            assert int(rec["bytes_data_payload"][0]) == int(rec["bytes_data_header"][0]) == 3 * k * 0xFFFFFFFF > 1 << 32
            assert int(rec["packets_data"][0]) == 3 * k
    finally:
        p.close()


def case_socket_slots(make, n_sockets):
    """the slot == n_sockets is flagged and counted at the host only; n_sockets == 0 switches the slots off"""
    p = _Pair(make, 2, n_sockets=n_sockets)
    try:
        last = max(n_sockets - 1, 0)
        ms = meta((20, 5, 0, last), (20, 6, 0, n_sockets), (20, 0, 0, NONE & 0xFFFFFFFF))
        p.tx([NONE, NONE], [0, 1, 3], ms, [SENT] * 3, 0)
        f, n_tx, _, msg = p.status()
        assert n_tx == 3 and f == (TM.BAD_SOCKET if n_sockets else 0) and ("socket slot" in msg) == bool(n_sockets)
        p.note(ms, 0)
        p.rx([0, 2, 3], [last, n_sockets, n_sockets + 7], [0, 1, 2], [RX_HIT] * 3)
        p.rx_flat([1, 1], [n_sockets, last], ms[:2])
        f, _, n_rx, _ = p.status()
        assert n_rx == 5 and f == (TM.BAD_SOCKET if n_sockets else 0)
        nin, nout, sin, sout = p.heartbeat()
        assert int(nout["packets_data"].sum()) == 2 and int(nout["packets_control"].sum()) == 1
        assert int(nin["packets_data"].sum()) == 4 and int(nin["packets_control"].sum()) == 1
        assert len(sin) == len(sout) == n_sockets
        if n_sockets:
            assert total(sout) == dict(packets_data=1, bytes_data_header=20, bytes_data_payload=5)
            assert total(sout[last:]) == total(sout)
            assert total(sin) == dict(packets_data=2, bytes_data_header=40, bytes_data_payload=11)
    finally:
        p.close()


def case_dropped_not_counted(make):
    p = _Pair(make, 2)
    try:
        ms = meta((20, 9, 0, 0), (20, 9, 0, 0), (20, 9, 0, 0))
        p.note(ms, 0)
        p.rx([0, 1, 3], [TM.NONE32, 2, TM.NONE32], [0, 1, 2], [RX_MISS, RX_HIT, RX_MISS])
        p.rx_flat([0, 1], [TM.NONE32, 3], ms[:2])
        assert p.status()[:3] == (0, 0, 2)
        nin, _, sin, _ = p.heartbeat()
        assert total(nin[1:2]) == total(nin) == dict(packets_data=2, bytes_data_header=40, bytes_data_payload=18)
        assert total(sin[2:3]) == total(sin[3:4]) == dict(packets_data=1, bytes_data_header=20, bytes_data_payload=9)
    finally:
        p.close()


def case_placeholder_and_lost_tag(make):
    """a placeholder deliver record (no RCV bit, socket and user UINT32_MAX), a tag older than the ring
    holds and one not noted yet: skipped and flagged; the record between them is counted"""
    p = _Pair(make, 1, note_cap=2)
    try:
        p.note(meta((20, 1, 0, 0), (20, 2, 0, 0), (20, 3, 0, 0)), 0)
        p.rx([0, 1], [TM.NONE32], [U64], [D.FWD])
        f, _, n_rx, msg = p.status()
        assert (f, n_rx) == (TM.NOTE_OVERRUN, 0) and "note ring" in msg
        assert p.status()[0] == 0  # cleared on read
        p.rx([0, 3], [1, 1, 1], [0, 2, 3], [RX_HIT] * 3)
        assert p.status()[:3] == (TM.NOTE_OVERRUN, 0, 1)
        nin, _, _, _ = p.heartbeat()
        assert total(nin) == dict(packets_data=1, bytes_data_header=20, bytes_data_payload=3)
    finally:
        p.close()


def case_log_one_short(make):
    """log_cap 3: of four queued packets the first is not logged; as a late record it is flagged and not
    counted, the others are; and a log_cap of 4 holds all four"""
    for log_cap, flag, n in ((3, TM.LOG_OVERRUN, 4), (4, 0, 5)):
        p = _Pair(make, 2, log_cap=log_cap)
        try:
            ms = meta(*[(20, 10 + k, 0, k) for k in range(4)])
            p.tx([NONE, NONE], [0, 1, 4], ms, [0] * 4, 0)
            p.tx([NONE, NONE], [0, 0, 0], meta(), [], 4, late=[(0, 0), (3, 1), (1, 1)])
            f, n_tx, _, msg = p.status()
            assert (f, n_tx) == (flag, n - 2) and ("older than the log" in msg) == bool(flag)
            # a packet held cached at the end of a later call is read back from the same log
            p.tx([2, NONE], [0, 0, 1], meta((20, 0, 0, 0)), [SENT], 4)
            assert p.status()[:2] == (0, n)
            _, out, _, sout = p.heartbeat()
            assert int(out["packets_data"].sum()) == n - 1 and int(sout["packets_data"].sum()) == n - 1
        finally:
            p.close()


def case_flat_duplicates(make):
    p = _Pair(make, 3, n_sockets=3)
    try:
        rng = np.random.default_rng(3)
        n = 700
        host, sock = rng.integers(0, 2, size=n) * 2, rng.integers(0, 2, size=n)  # four (host, slot) pairs
        ms = rand_meta(rng, n)
        p.rx_flat(host, sock, ms)
        p.rx_flat([0, 3, 0xFFFFFFFF, 2], [2, 0, 0, 2], ms[:4])  # hosts 3 and 2^32-1 do not exist
        f, _, n_rx, msg = p.status()
        assert (f, n_rx) == (TM.BAD_HOST, n + 2) and "n_hosts" in msg
        nin, _, sin, _ = p.heartbeat()
        assert int(sum(nin[f][1] for f in TM.FIELDS)) == 0 and total(sin[2:3])
        assert sum(int(nin[f].sum()) for f in TM.FIELDS if f.startswith("packets")) == n + 2
    finally:
        p.close()


def case_bad_late_host_and_walk_bounds(make):
    """a late record of a host that does not exist is skipped; host_ptr past n_pkts ends at n_pkts; an rx
    list's out_cap below host_ptr[n_hosts] ends the walk there"""
    p = _Pair(make, 2)
    try:
        ms = meta(*[(20, 1 + k, 0, 0) for k in range(4)])
        p.tx([NONE, NONE], [0, 2, 9], ms[:3], [0, SENT, SENT], 0)
        p.tx([NONE, NONE], [0, 0, 0], meta(), [], 3, late=[(0, 2), (0, 0xFFFFFFFF), (0, 0)], late_cap=5)
        assert p.status()[:2] == (TM.BAD_HOST, 3)
        p.note(ms, 0)
        p.r.rx([0, 2, 4], [0, 0, 0, 0], [0, 1, 2, 3], [RX_HIT] * 4, out_cap=3)
        p.m.rx([0, 2, 4], [0, 0, 0, 0], [0, 1, 2, 3], [RX_HIT] * 4, out_cap=3)
        assert p.status()[:3] == (0, 3, 3)
        p.heartbeat()
    finally:
        p.close()


def _slots(n):
    def case(make):
        case_socket_slots(make, n)
    case.__name__ = "case_socket_slots_%d" % n
    return case


CASES = [case_oversize_cached_three_calls, case_popped_after_queuing, case_one_packet_per_class,
         case_carry_past_32_bits, _slots(0), _slots(1), _slots(257), case_dropped_not_counted,
         case_placeholder_and_lost_tag, case_log_one_short, case_flat_duplicates, case_bad_late_host_and_walk_bounds]


def error_paths(plan_handle=None):
    """null arguments and SRT_ERR_INVALID of the entry points, on raw ctypes"""
    from shadow_amd import _lib

    L, err, h = _lib.lib(), _lib.SrtErr(), C.c_void_p()
    inv, ok = _lib.SRT_ERR_INVALID, _lib.SRT_OK
    assert L.srt_tracker_create(plan_handle, 2, 2, 4, 4, None, C.byref(err)) == inv and b"null" in err.msg
    assert L.srt_tracker_create(plan_handle, 1 << 31, 2, 4, 4, C.byref(h), C.byref(err)) == inv and not h
    assert L.srt_tracker_create(plan_handle, 2, 1 << 31, 4, 4, C.byref(h), C.byref(err)) == inv and not h
    assert L.srt_tracker_create(plan_handle, 2, 2, (1 << 31) + 1, 4, C.byref(h), C.byref(err)) == inv and b"note_cap" in err.msg
    assert L.srt_tracker_create(plan_handle, 2, 2, 4, (1 << 31) + 1, C.byref(h), C.byref(err)) == inv
    assert L.srt_tracker_tx(None, None, None, 0, None, None, 0, None, 0, None, C.byref(err)) == inv and b"null" in err.msg
    assert L.srt_tracker_note(None, None, 0, 0, C.byref(err)) == inv
    assert L.srt_tracker_rx(None, None, None, None, None, 0, C.byref(err)) == inv
    assert L.srt_tracker_rx_flat(None, None, None, None, 0, C.byref(err)) == inv
    assert L.srt_tracker_heartbeat(None, None, 0, None, 0, None, None, None, None, C.byref(err)) == inv
    assert L.srt_tracker_status(None, None, None, None, C.byref(err)) == inv
    assert L.srt_outbound_cached_seq(None, None, C.byref(err)) == inv and b"null" in err.msg
    assert L.srt_tracker_counter_string(None, None, 0) == -1
    L.srt_tracker_destroy(None)
    if plan_handle is not None:
        return
    assert L.srt_tracker_create(None, 2, 2, 4, 4, C.byref(h), C.byref(err)) == ok
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    cs, hp = np.full(2, U64, np.uint64), np.array([0, 1, 2], np.uint32)
    ms, st = meta((20, 1, 0, 0), (20, 0, 0, 1)), np.array([SENT, SENT], np.uint32)
    late, cnt = np.zeros(1, LATE_DTYPE), np.zeros(1, np.uint32)

    def tx(f=h, cs=cs, hp=hp, n=2, ms=ms, st=st, late=late, late_cap=1, cnt=cnt, base=0):
        return L.srt_tracker_tx(f, p(cs), p(hp), n, p(ms), p(st), base, p(late), late_cap, p(cnt), C.byref(err))

    for bad in (dict(f=None), dict(cs=None), dict(hp=None), dict(ms=None), dict(st=None), dict(late=None),
                dict(cnt=None), dict(n=1 << 31), dict(late_cap=1 << 31), dict(base=U64)):
        assert tx(**bad) == inv, bad
        assert err.code == inv and err.msg
    assert tx(late=None, cnt=None, late_cap=0) == ok
    assert L.srt_tracker_note(h, None, 2, 0, C.byref(err)) == inv
    assert L.srt_tracker_note(h, p(ms), 1 << 31, 0, C.byref(err)) == inv
    assert L.srt_tracker_note(h, p(ms), 2, 5, C.byref(err)) == ok
    assert L.srt_tracker_note(h, p(ms), 2, 6, C.byref(err)) == inv and b"tag_base" in err.msg  # backwards
    sock, tag, rst = np.array([0, 1], np.uint32), np.array([5, 6], np.uint64), np.array([RX_HIT] * 2, np.uint32)
    for args in ((None, p(sock), p(tag), p(rst)), (p(hp), None, p(tag), p(rst)), (p(hp), p(sock), None, p(rst)),
                 (p(hp), p(sock), p(tag), None)):
        assert L.srt_tracker_rx(h, *args, 2, C.byref(err)) == inv and b"null" in err.msg
    assert L.srt_tracker_rx(h, p(hp), None, None, None, 0, C.byref(err)) == ok  # nothing to walk
    assert L.srt_tracker_rx(h, p(hp), p(sock), p(tag), p(rst), 2, C.byref(err)) == ok
    hosts = np.array([0, 1], np.uint32)
    assert L.srt_tracker_rx_flat(h, p(hosts), None, p(ms), 2, C.byref(err)) == inv
    assert L.srt_tracker_rx_flat(h, p(hosts), p(sock), p(ms), 1 << 31, C.byref(err)) == inv
    assert L.srt_tracker_rx_flat(h, None, None, None, 0, C.byref(err)) == ok
    flags, a8, b8 = C.c_uint32(), C.c_uint64(), C.c_uint64()
    assert L.srt_tracker_status(h, C.byref(flags), C.byref(a8), C.byref(b8), C.byref(err)) == ok
    assert (flags.value, a8.value, b8.value) == (0, 2, 2)
    assert L.srt_tracker_status(h, None, None, None, None) == ok
    # a selection out of range clears nothing
    out = np.zeros(2, TM.COUNTERS)
    bad_h, bad_s = np.array([0, 2], np.uint32), np.array([2], np.uint32)
    assert L.srt_tracker_heartbeat(h, p(bad_h), 2, None, 0, p(out), None, None, None, C.byref(err)) == inv
    assert b"n_hosts" in err.msg
    assert L.srt_tracker_heartbeat(h, None, 0, p(bad_s), 1, None, None, None, None, C.byref(err)) == inv
    twice = np.array([1, 1], np.uint32)  # named twice: returned twice, cleared once
    assert L.srt_tracker_heartbeat(h, p(twice), 2, p(twice), 0, p(out), None, None, None, C.byref(err)) == ok
    assert out["packets_control"].tolist() == [1, 1] and out["bytes_control_header"].tolist() == [20, 20]
    assert L.srt_tracker_heartbeat(h, None, 0, None, 0, p(out), None, None, None, C.byref(err)) == ok
    assert out["packets_data"].tolist() == [1, 0] and out["packets_control"].tolist() == [0, 0]
    L.srt_tracker_destroy(h)
