"""What the interface receive stage's tests share: a generator of windows whose
inbound results come from the real host-only InboundRouter (low download
bandwidths, so packets stay queued and come back as late records of later
calls, and CoDel drops some), with associations added and removed between
windows; a runner that feeds srt_deliver (host-only or on the device) from
numpy arrays and keeps a guard behind every output; and the hand-made cases
both forms must pass."""
import ctypes as C
import functools

import numpy as np

import deliver_model as DM

GUARD = 4
FILL = 0xA5
MS = 1_000_000
W_NS = 20 * MS
T0 = 1_000 * MS
N_WIN = 6            # windows with arrivals; one more drains
DENSE, SPARSE = "dense", "sparse"  # 0 to 200 packets a host and window / about one
G = DM.SORT_CAP      # SORT_CAP of srt_deliver_step.h: the seqs of a late run ranked at once
FWD = DM.ENQUEUED | (1 << 11) | DM.FORWARDED   # what the router leaves on a forwarded packet
QUEUED = DM.ENQUEUED
BANDWIDTHS = (10_000, 2_000_000, 5_000_000, 1_250_000_000)
PORTS, PEER_IPS, PEER_PORTS = (0x5000, 0xBB01, 0x3500), (0, 0x0100000A, 0x0200000A, 0x0300A8C0), (0, 0x901F, 0x5000)


def rand_meta(rng, n):
    m = np.zeros(n, DM.RX_META)
    m["peer_ip_be"] = rng.choice(np.array(PEER_IPS, np.uint32), size=n)
    m["peer_port_be"] = rng.choice(np.array(PEER_PORTS, np.uint16), size=n)
    wild = rng.random(n) < 0.1
    m["peer_ip_be"][wild], m["peer_port_be"][wild] = 0, 0
    m["local_port_be"] = rng.choice(np.array(PORTS, np.uint16), size=n)
    m["protocol"] = rng.choice(np.array([DM.TCP, DM.UDP, 3], np.uint32), size=n, p=[0.55, 0.4, 0.05])
    m["user"] = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    return m


def rand_assoc(rng, n_hosts, n, taken, next_socket):
    """n associations whose keys are not in `taken` (updated), half of them wildcards"""
    out = np.zeros(n, DM.ASSOC)
    k = 0
    while k < n:
        a = out[k]
        a["host"], a["protocol"] = rng.integers(0, n_hosts), rng.choice([DM.TCP, DM.UDP])
        a["local_port_be"] = rng.choice(PORTS)
        if rng.random() < 0.5:
            a["peer_ip_be"], a["peer_port_be"] = rng.choice(PEER_IPS), rng.choice(PEER_PORTS)
        else:
            a["peer_ip_be"], a["peer_port_be"] = 0, 0
        a["socket"] = next_socket + k
        if DM.key_of(a) in taken:
            if len(taken) >= n_hosts * 60:  # the key space is nearly full
                return out[:k]
            continue
        taken.add(DM.key_of(a))
        k += 1
    return out


@functools.lru_cache(maxsize=None)
def scenario(n_hosts, shape, seed=21):
    """-> dict(bw, cap, steps): steps of ("assoc", recs) / ("disassoc", recs) / ("note", meta, tag_base) /
    ("run", window arrays padded to cap, inbound results, seq_base, late records)"""
    from shadow_amd.plan import INBOUND_LATE_DTYPE, InboundRouter

    rng = np.random.default_rng(seed + n_hosts + (1000 if shape == SPARSE else 0))
    bw = rng.choice(np.array(BANDWIDTHS, np.uint64), size=n_hosts, p=[0.15, 0.35, 0.3, 0.2])
    bw[0] = 2_000_000
    wins = []
    for w in range(N_WIN + 1):
        if w == N_WIN:
            per = np.zeros(n_hosts, np.int64)
        elif shape == DENSE:
            per = rng.integers(0, 201, size=n_hosts)
            per[rng.random(n_hosts) < 0.15] = 0
            per[0] = 150 + int(rng.integers(0, 50))
        else:
            per = rng.integers(0, 3, size=n_hosts)
        wins.append(per)
    cap = int(max(p.sum() for p in wins)) + 7  # n_pkts of every call: past what the window holds
    late_cap = int(sum(p.sum() for p in wins)) + 1
    ib = InboundRouter(None, bw, 200 * (N_WIN + 1))
    taken, live, next_socket, tag_next = set(), np.zeros(0, DM.ASSOC), 0, 0
    steps = []
    try:
        for w, per in enumerate(wins):
            # the associations move between the windows
            if w:
                gone = live[rng.random(len(live)) < 0.25]
                for a in gone:
                    taken.discard(DM.key_of(a))
                live = live[~np.isin(live["socket"], gone["socket"])]
                missing = rand_assoc(rng, n_hosts, 2, set(taken), 1 << 30)  # removing a missing key: a no-op
                steps.append(("disassoc", np.concatenate([gone, missing])))
            new = rand_assoc(rng, n_hosts, 4 * n_hosts if w == 0 else n_hosts, taken, next_socket)
            next_socket += len(new)
            live = np.concatenate([live, new])
            steps.append(("assoc", new))
            n = int(per.sum())
            lo, until = T0 + w * W_NS, T0 + (w + 1) * W_NS if w < N_WIN else T0 + 400 * W_NS
            dst_ptr = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
            deliver = np.zeros(cap, np.uint64)
            for h in range(n_hosts):  # final order: a host's packets by deliver time
                deliver[dst_ptr[h]:dst_ptr[h + 1]] = np.sort(lo + rng.integers(0, 64, size=per[h]) * (W_NS // 64))
            size = np.zeros(cap, np.uint32)
            size[:n] = rng.integers(40, 1501, size=n)
            # the round's push: tags tag_next + batch index, the window takes them in another order
            meta = rand_meta(rng, n)
            perm = rng.permutation(n)
            tag = np.zeros(cap, np.uint64)
            tag[:n] = tag_next + perm
            note_meta = np.zeros(n, DM.RX_META)
            note_meta[perm] = meta
            steps.append(("note", note_meta, tag_next))
            tag_next += n
            order = np.arange(cap, dtype=np.uint32)
            status, forward = np.zeros(cap, np.uint32), np.zeros(cap, np.uint64)
            late, cnt = np.zeros(late_cap * 24, np.uint8), np.zeros(1, np.uint32)
            base = ib.run(order, dst_ptr, deliver, size, until, 0, status, forward, late, cnt)
            flags, _ = ib.status(check=False)
            assert flags == 0, flags
            steps.append(("run", dict(dst_ptr=dst_ptr, tag=tag, status=status, forward=forward, seq_base=base,
                                      late=late.view(INBOUND_LATE_DTYPE)[:int(cnt[0])].copy().astype(DM.LATE))))
    finally:
        ib.close()
    return dict(bw=bw, cap=cap, late_cap=late_cap, steps=steps, total=tag_next)


class Runner:
    """srt_deliver fed from numpy arrays; plan=None: the host-only instance"""

    def __init__(self, plan, n_hosts, table_slots_min, note_cap, log_cap):
        from shadow_amd.plan import DeliverStage

        self.plan, self.n_hosts = plan, n_hosts
        self.ds = DeliverStage(plan, n_hosts, table_slots_min, note_cap, log_cap)

    def close(self):
        self.ds.close()

    def _in(self, a):
        a = np.ascontiguousarray(a)
        if self.plan is None:
            return a.view(np.uint8).reshape(-1) if a.dtype.fields else a
        import torch

        if a.dtype.fields:
            return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
        signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype)
        return torch.from_numpy(a.view(signed).copy()).to("cuda:0")

    def _out(self, n, width):
        if self.plan is None:
            return np.full(n * width, FILL, np.uint8)
        import torch

        return torch.full((n * width,), FILL, dtype=torch.uint8, device="cuda:0")

    def associate(self, recs):
        """-> True; False when the library refused the batch"""
        from shadow_amd import _lib

        try:
            self.ds.associate(recs)
            return True
        except _lib.SrtError as e:
            assert e.code == _lib.SRT_ERR_INVALID
            return False

    def disassociate(self, recs):
        self.ds.disassociate(recs)

    def lookup(self, hosts, meta):
        return self.ds.lookup(hosts, meta)

    def note(self, meta, tag_base):
        self.ds.note(self._in(np.asarray(meta, DM.RX_META)), tag_base)

    def status(self):
        """-> (flags, n_delivered, n_no_socket, message)"""
        from shadow_amd import _lib

        f, a, b, err = C.c_uint32(), C.c_uint64(), C.c_uint64(), _lib.SrtErr()
        rc = _lib.lib().srt_deliver_status(self.ds._h, C.byref(f), C.byref(a), C.byref(b), C.byref(err))
        assert rc == (_lib.SRT_ERR_INVALID if f.value else _lib.SRT_OK), (rc, err.msg)
        return f.value, a.value, b.value, err.msg.decode()

    def run(self, dst_ptr, n_pkts, tag, status, forward, seq_base, late, out_cap, late_cap=None, **_):
        """-> dict like the model's, plus msg and untouched: every output byte behind the delivered
        entries, the guard included, still holds the fill"""
        late = np.asarray(late, DM.LATE)
        late_cap = len(late) if late_cap is None else late_cap
        lbuf = np.zeros(max(late_cap, len(late)), DM.LATE)
        lbuf[:len(late)] = late
        cap = out_cap + GUARD
        bufs = {k: self._out(cap, np.dtype(t).itemsize) for k, t in DM.OUT_FIELDS}
        o_hp = self._out(self.n_hosts + 1 + GUARD, 4)
        cut = lambda k, t: bufs[k][:np.dtype(t).itemsize * out_cap]  # noqa: E731
        u4, u8 = (lambda a: np.asarray(a, np.uint32)[:n_pkts]), (lambda a: np.asarray(a, np.uint64)[:n_pkts])
        self.ds.run(self._in(np.asarray(dst_ptr, np.uint32)), self._in(u8(tag)), self._in(u4(status)),
                    self._in(u8(forward)), seq_base, self._in(lbuf[:late_cap]) if late_cap else None,
                    self._in(np.array([len(late)], np.uint32)) if late_cap else None,
                    o_hp[:4 * (self.n_hosts + 1)], cut("socket", np.uint32), cut("forward", np.uint64),
                    cut("tag", np.uint64), cut("user", np.uint32), cut("status", np.uint32))
        st = self.status()
        host = (lambda a: a) if self.plan is None else (lambda a: a.cpu().numpy())
        o_hp = host(o_hp)
        host_ptr = o_hp[:4 * (self.n_hosts + 1)].view(np.uint32)
        k = int(host_ptr[-1])
        assert k <= out_cap
        out = dict(host_ptr=host_ptr, flags=st[0], n_delivered=st[1], n_no_socket=st[2], msg=st[3])
        ok = bool((o_hp[4 * (self.n_hosts + 1):] == FILL).all())
        for name, t in DM.OUT_FIELDS:
            a, w = host(bufs[name]), np.dtype(t).itemsize
            out[name] = a[:w * k].view(t)
            ok = ok and bool((a[w * (out_cap if st[0] & DM.OUT_OVERFLOW else k):] == FILL).all())
        out["untouched"] = ok
        return out


def assert_same(out, mo, what=""):
    """a runner's delivery list against the model's (or another runner's), byte for byte; the records of
    an overflowing call, and the flags that come from records, are unspecified"""
    keep = DM.OUT_OVERFLOW | DM.BAD_HOST if mo["flags"] & DM.OUT_OVERFLOW else 15
    assert out["flags"] & keep == mo["flags"] & keep, (what, out["flags"], mo["flags"])
    assert out["n_delivered"] == mo["n_delivered"], (what, out["n_delivered"], mo["n_delivered"])
    assert np.array_equal(out["host_ptr"], mo["host_ptr"]), what
    assert out.get("untouched", True), what
    if out["flags"] & DM.OUT_OVERFLOW:
        return
    assert out["n_no_socket"] == mo["n_no_socket"], what
    for f, _ in DM.OUT_FIELDS:
        assert out[f].tobytes() == mo[f].tobytes(), (what, f, np.nonzero(out[f] != mo[f])[0][:8])


def _drive(obj, sc, run):
    outs = []
    for st in sc["steps"]:
        if st[0] == "assoc":
            assert obj.associate(st[1])
        elif st[0] == "disassoc":
            obj.disassociate(st[1])
        elif st[0] == "note":
            obj.note(st[1], st[2])
        else:
            outs.append(run(st[1]))
    return outs


def run_scenario(plan, n_hosts, shape):
    """the scenario through a runner -> the delivery lists of its runs"""
    sc = scenario(n_hosts, shape)
    r = Runner(plan, n_hosts, 8, sc["total"], (N_WIN + 1) * sc["cap"])
    try:
        return _drive(r, sc, lambda a: r.run(n_pkts=sc["cap"], out_cap=sc["cap"] + sc["late_cap"],
                                             late_cap=sc["late_cap"], **a))
    finally:
        r.close()


@functools.lru_cache(maxsize=None)
def model_scenario(n_hosts, shape):
    sc = scenario(n_hosts, shape)
    m = DM.DeliverModel(n_hosts, sc["total"], (N_WIN + 1) * sc["cap"])
    return _drive(m, sc, lambda a: m.run(n_pkts=sc["cap"], out_cap=sc["cap"] + sc["late_cap"], **a))


# ------------------------------------------------------------ hand-made cases
class _Pair:
    """the same calls through a runner and the model"""

    def __init__(self, make, n_hosts, table_slots_min=8, note_cap=64, log_cap=64):
        self.r, self.m = make(n_hosts, table_slots_min, note_cap, log_cap), DM.DeliverModel(n_hosts, note_cap, log_cap)
        self.n_hosts = n_hosts

    def associate(self, recs):
        a, b = self.r.associate(recs), self.m.associate(recs)
        assert a == b, (a, b)
        return a

    def disassociate(self, recs):
        self.r.disassociate(recs)
        self.m.disassociate(recs)

    def note(self, meta, tag_base):
        self.r.note(meta, tag_base)
        self.m.note(meta, tag_base)

    def run(self, dst_ptr, tag, status, forward, seq_base, late=(), out_cap=None, n_pkts=None, monotone=True):
        n_pkts = len(status) if n_pkts is None else n_pkts
        late = np.array(list(late), DM.LATE)
        out_cap = n_pkts + len(late) if out_cap is None else out_cap
        out = self.r.run(dst_ptr, n_pkts, tag, status, forward, seq_base, late, out_cap)
        mo = self.m.run(np.asarray(dst_ptr), n_pkts, tag, status, forward, seq_base, late, out_cap, monotone=monotone)
        assert_same(out, mo)
        return out

    def lookup(self, hosts, meta):
        a, b = self.r.lookup(hosts, meta), self.m.lookup(hosts, meta)
        assert np.array_equal(a, b), (a, b)
        return a

    def close(self):
        self.r.close()


def assoc(*rows):
    """(host, protocol, peer_ip, local_port, peer_port, socket) rows -> ASSOC records"""
    return np.array(list(rows), DM.ASSOC)


def meta(*rows):
    """(peer_ip, peer_port, local_port, protocol, user) rows -> RX_META records"""
    return np.array(list(rows), DM.RX_META)


def _one_host(p, metas, tags=None):
    """every meta as one forwarded window packet of host 0 -> the delivery list"""
    n = len(metas)
    return p.run([0, n] + [n] * (p.n_hosts - 1), np.arange(n) if tags is None else tags, [FWD] * n,
                 100 + np.arange(n), 0)


def case_lookup_rules(make):
    """specific beats wildcard; wildcard fallback; no socket gives DROPPED; keys differing only in
    protocol, only in host, only in port; a peer of 0:0"""
    p = _Pair(make, 2)
    try:
        ip, pp, lp = 0x0100000A, 0x901F, 0x5000
        assert p.associate(assoc((0, DM.TCP, ip, lp, pp, 10), (0, DM.TCP, 0, lp, 0, 11), (0, DM.UDP, ip, lp, pp, 12),
                                 (1, DM.TCP, ip, lp, pp, 13), (0, DM.TCP, ip, lp + 1, pp, 14)))
        ms = meta((ip, pp, lp, DM.TCP, 0), (ip + 1, pp, lp, DM.TCP, 1), (ip, pp, lp, DM.UDP, 2),
                  (ip + 1, pp, lp, DM.UDP, 3), (ip, pp, lp + 1, DM.TCP, 4), (ip, pp + 1, lp + 1, DM.TCP, 5),
                  (0, 0, lp, DM.TCP, 6), (0, 0, lp, DM.UDP, 7), (ip, pp, lp, 3, 8), (ip, 0, lp, DM.TCP, 9))
        p.note(ms, 0)
        out = _one_host(p, ms)
        assert out["socket"].tolist() == [10, 11, 12, DM.NONE32, 14, DM.NONE32, 11, DM.NONE32, DM.NONE32, 11]
        assert out["user"].tolist() == list(range(10)) and out["n_no_socket"] == 4
        hit, miss = FWD | DM.RECEIVED, FWD | DM.RECEIVED | DM.IF_DROPPED
        assert out["status"].tolist() == [hit, hit, hit, miss, hit, miss, hit, miss, miss, hit]
        # the same packets at host 1: only its own association answers
        out = p.run([0, 0, 10], np.arange(10), [FWD] * 10, 200 + np.arange(10), 10)
        assert out["socket"].tolist() == [13] + [DM.NONE32] * 9 and out["host_ptr"].tolist() == [0, 0, 10]
        assert p.lookup([0, 1, 0], ms[[0, 0, 3]]).tolist() == [10, 13, DM.NONE32]
    finally:
        p.close()


def case_empty_table(make):
    p = _Pair(make, 1, table_slots_min=0)
    try:
        ms = meta((1, 2, 3, DM.TCP, 70), (0, 0, 3, DM.UDP, 71))
        p.note(ms, 0)
        out = _one_host(p, ms)
        assert out["socket"].tolist() == [DM.NONE32] * 2 and out["user"].tolist() == [70, 71]
        assert p.r.ds.table_stats() == (0, 2, 0, False)
    finally:
        p.close()


def case_table_maintenance(make):
    """a duplicate add is an error and changes nothing; removing a missing key is a no-op; remove, then
    deliver, falls to the wildcard; growth across a doubling"""
    p = _Pair(make, 1)
    try:
        ip, pp, lp = 7, 8, 9
        assert p.associate(assoc((0, DM.TCP, ip, lp, pp, 1), (0, DM.TCP, 0, lp, 0, 2)))
        assert not p.associate(assoc((0, DM.TCP, 5, lp, pp, 3), (0, DM.TCP, ip, lp, pp, 4)))  # the second exists
        assert not p.associate(assoc((0, DM.TCP, 5, lp, pp, 3), (0, DM.TCP, 5, lp, pp, 4)))   # twice in the batch
        assert not p.associate(assoc((1, DM.TCP, 5, lp, pp, 3))) and not p.associate(assoc((0, 3, 5, lp, pp, 3)))
        assert not p.associate(assoc((0, DM.TCP, 5, lp, pp, 1 << 31)))
        assert p.r.ds.table_stats()[:2] == (2, 8)
        ms = meta((ip, pp, lp, DM.TCP, 0), (5, pp, lp, DM.TCP, 1))
        p.note(ms, 0)
        assert _one_host(p, ms)["socket"].tolist() == [1, 2]  # the refused batches left no key behind
        p.disassociate(assoc((0, DM.UDP, ip, lp, pp, 0)))  # a missing key
        assert p.r.ds.table_stats()[:2] == (2, 8)
        p.disassociate(assoc((0, DM.TCP, ip, lp, pp, 99)))  # the socket field is ignored
        assert p.run([0, 2], [0, 1], [FWD] * 2, [300, 301], 2)["socket"].tolist() == [2, 2]
        # 4 of 8 slots hold a load of 1/2; the fifth association doubles the table
        assert p.associate(assoc(*[(0, DM.UDP, 100 + k, lp, pp, 20 + k) for k in range(3)]))
        assert p.r.ds.table_stats()[:2] == (4, 8)
        assert p.associate(assoc((0, DM.UDP, 200, lp, pp, 30)))
        assert p.r.ds.table_stats()[:2] == (5, 16)
        ms = meta(*[(100 + k, pp, lp, DM.UDP, k) for k in range(3)], (200, pp, lp, DM.UDP, 3), (ip, pp, lp, DM.TCP, 4))
        p.note(ms, 2)
        assert p.run([0, 5], 2 + np.arange(5), [FWD] * 5, 400 + np.arange(5), 4)["socket"].tolist() == [20, 21, 22, 30, 2]
    finally:
        p.close()


def probe_chain_keys(slots=8, want=3):
    """`want` specific keys and their wildcard, all with their home in the table's LAST slot: the chain
    runs slots - 1, 0, 1, ... and the longest probe sequence is want + 1"""
    rows, lp = [], 0x5000
    for ip in range(1, 100000):
        a = assoc((0, DM.TCP, ip, lp, 0x901F, len(rows)))[0]
        if DM.home_slot(a, slots) == slots - 1:
            rows.append(tuple(a.tolist()))
            if len(rows) == want:
                break
    for lp2 in range(1, 65536):
        a = assoc((0, DM.UDP, 0, lp2, 0, want))[0]
        if DM.home_slot(a, slots) == slots - 1:
            rows.append(tuple(a.tolist()))
            break
    return assoc(*rows)


def case_probe_chain_wraps(make):
    p = _Pair(make, 1, table_slots_min=8)
    try:
        keys = probe_chain_keys()
        assert len(keys) == 4 and p.associate(keys)
        n, slots, max_probe, wrapped = p.r.ds.table_stats()
        assert (n, slots) == (4, 8) and max_probe >= 3 and wrapped
        ms = meta(*[(int(a["peer_ip_be"]), int(a["peer_port_be"]), int(a["local_port_be"]), int(a["protocol"]), k)
                    for k, a in enumerate(keys)], (12345, 1, int(keys[3]["local_port_be"]), DM.UDP, 4),
                  (12345, 1, 0x5000, DM.TCP, 5))
        p.note(ms, 0)
        out = _one_host(p, ms)
        assert out["socket"].tolist() == [0, 1, 2, 3, 3, DM.NONE32]
        p.disassociate(keys[1:2])  # the chain closes up behind a removed key: the table is rebuilt
        out = p.run([0, 6], np.arange(6), [FWD] * 6, 200 + np.arange(6), 6)
        assert out["socket"].tolist() == [0, DM.NONE32, 2, 3, 3, DM.NONE32]
    finally:
        p.close()


def case_late_lookup_at_delivery(make):
    """a packet queued in one call and forwarded in the next is looked up with the associations of the
    call that delivers it, and comes before the host's batch packets"""
    p = _Pair(make, 2)
    try:
        a1, a2 = assoc((1, DM.TCP, 7, 9, 8, 1)), assoc((1, DM.TCP, 0, 9, 0, 2))
        assert p.associate(a1)
        ms = meta((7, 8, 9, DM.TCP, 50), (7, 8, 9, DM.TCP, 51), (7, 8, 9, DM.TCP, 52))
        p.note(ms, 0)
        out = p.run([0, 0, 3], [2, 0, 1], [FWD, QUEUED, QUEUED], [10, DM.NONE64, DM.NONE64], 0)
        assert out["socket"].tolist() == [1] and out["user"].tolist() == [52] and out["tag"].tolist() == [2]
        p.disassociate(a1)
        assert p.associate(a2)
        p.note(meta((7, 8, 9, DM.TCP, 53)), 3)
        out = p.run([0, 0, 1], [3], [FWD], [40], 3, late=[(2, 30, FWD, 1), (1, 20, FWD, 1), (7, 0, DM.ENQUEUED | DM.ROUTER_DROPPED, 1)])
        assert out["socket"].tolist() == [2, 2, 2] and out["user"].tolist() == [50, 51, 53]
        assert out["tag"].tolist() == [0, 1, 3] and out["forward"].tolist() == [20, 30, 40]
        assert out["host_ptr"].tolist() == [0, 0, 3]
    finally:
        p.close()


def case_late_runs_around_the_sort_capacity(make):
    """late runs of one host of G - 1, G, G + 1 and 3G + 5 records (and hosts with none and with one),
    the late list in shuffled order, behind them batch packets"""
    sizes = [G - 1, 0, G, 1, G + 1, 3 * G + 5]
    n = sum(sizes)
    rng = np.random.default_rng(5)
    p = _Pair(make, len(sizes), note_cap=2 * n + 16, log_cap=n + 16)
    try:
        host = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))  # seq -> host
        assert p.associate(assoc(*[(h, DM.TCP, 0, 9, 0, 100 + h) for h in range(len(sizes))]))
        ms = rand_meta(rng, n)
        ms["local_port_be"], ms["protocol"] = 9, DM.TCP
        p.note(ms, 0)
        # call 1: everything queued, in final order (grouped by host)
        o = np.argsort(host, kind="stable")
        dst_ptr = np.concatenate([[0], np.cumsum(sizes)])
        out = p.run(dst_ptr, o, [QUEUED] * n, [DM.NONE64] * n, 0)
        assert out["n_delivered"] == 0
        # call 2: all of them leave, with one batch packet a host behind them
        seq_of = np.empty(n, np.int64)
        seq_of[o] = np.arange(n)  # tag -> seq
        late = [(int(seq_of[t]), 1000 + int(seq_of[t]), FWD, int(host[t])) for t in rng.permutation(n)]
        ms2 = rand_meta(rng, len(sizes))
        p.note(ms2, n)
        out = p.run(np.arange(len(sizes) + 1), n + np.arange(len(sizes)), [FWD] * len(sizes), [10 ** 6] * len(sizes), n,
                    late=late)
        assert np.diff(out["host_ptr"].astype(np.int64)).tolist() == [s + 1 for s in sizes] and out["flags"] == 0
    finally:
        p.close()


def case_log_overrun(make):
    """log_cap 4: of six queued packets only the last four are logged; a late record of an unlogged seq
    is a placeholder in its place, the call is flagged, the others are intact"""
    p = _Pair(make, 1, log_cap=4)
    try:
        assert p.associate(assoc((0, DM.UDP, 0, 9, 0, 5)))
        ms = meta(*[(1, 2, 9, DM.UDP, 60 + k) for k in range(6)])
        p.note(ms, 0)
        p.run([0, 6], np.arange(6), [QUEUED] * 6, [DM.NONE64] * 6, 0)
        out = p.run([0, 0], [], [], [], 6, late=[(5, 25, FWD, 0), (1, 21, FWD, 0), (2, 22, FWD, 0)], out_cap=3)
        assert out["flags"] == DM.LOG_OVERRUN and "older than the log" in out["msg"] and out["untouched"]
        assert out["socket"].tolist() == [DM.NONE32, 5, 5] and out["user"].tolist() == [DM.NONE32, 62, 65]
        assert out["tag"].tolist() == [DM.NONE64, 2, 5] and out["status"].tolist() == [FWD, FWD | DM.RECEIVED, FWD | DM.RECEIVED]
        assert p.r.status()[0] == 0  # cleared on read
    finally:
        p.close()


def case_note_overrun(make):
    """note_cap 3: a tag older than the ring holds, and one not noted yet, are placeholders that keep
    their tag; a queued packet logged without its meta is one when it leaves, in a later call"""
    p = _Pair(make, 1, note_cap=3)
    try:
        assert p.associate(assoc((0, DM.UDP, 0, 9, 0, 5)))
        p.note(meta(*[(1, 2, 9, DM.UDP, 60 + k) for k in range(5)]), 0)
        out = p.run([0, 4], [1, 2, 9, 0], [FWD, FWD, FWD, QUEUED], [10, 11, 12, DM.NONE64], 0)
        assert out["flags"] == DM.NOTE_OVERRUN and "note ring" in out["msg"] and out["untouched"]
        assert out["socket"].tolist() == [DM.NONE32, 5, DM.NONE32] and out["user"].tolist() == [DM.NONE32, 62, DM.NONE32]
        assert out["tag"].tolist() == [1, 2, 9] and out["status"].tolist() == [FWD, FWD | DM.RECEIVED, FWD]
        out = p.run([0, 1], [4], [FWD], [31], 4, late=[(3, 30, FWD, 0)])
        assert out["flags"] == DM.NOTE_OVERRUN and out["tag"].tolist() == [0, 4] and out["socket"].tolist() == [DM.NONE32, 5]
    finally:
        p.close()


def case_out_overflow_and_bad_host(make):
    p = _Pair(make, 3)
    try:
        assert p.associate(assoc(*[(h, DM.TCP, 0, 9, 0, h) for h in range(3)]))
        ms = meta(*[(1, 2, 9, DM.TCP, k) for k in range(6)])
        p.note(ms, 0)
        args = ([0, 2, 4, 6], np.arange(6), [FWD] * 6, np.arange(6), 0)
        out = p.run(*args, out_cap=6)  # exactly full
        assert out["flags"] == 0 and out["socket"].tolist() == [0, 0, 1, 1, 2, 2]
        out = p.run(*args[:4], 6, out_cap=3)  # one host's run straddles the end
        assert out["flags"] == DM.OUT_OVERFLOW and "out_cap" in out["msg"] and out["n_delivered"] == 6
        assert out["host_ptr"].tolist() == [0, 2, 3, 3] and out["untouched"]
        out = p.run(*args[:4], 12, out_cap=0)
        assert out["flags"] == DM.OUT_OVERFLOW and out["host_ptr"].tolist() == [0, 0, 0, 0] and out["untouched"]
        # a late record for a host that does not exist is skipped; the rest of the call is intact
        p.run([0, 1, 1, 1], [0], [QUEUED], [DM.NONE64], 18)
        out = p.run([0, 0, 0, 0], [], [], [], 19, late=[(18, 50, FWD, 0), (18, 50, FWD, 3), (18, 50, FWD, DM.NONE32)])
        assert out["flags"] == DM.BAD_HOST and "dst_host" in out["msg"] and out["untouched"]
        assert out["host_ptr"].tolist() == [0, 1, 1, 1] and out["user"].tolist() == [0]
        # two flags in one call, every one with its own words
        out = p.run([0, 0, 0, 0], [], [], [], 19, late=[(18, 50, FWD, 0), (18, 50, FWD, 1), (18, 50, FWD, 7)], out_cap=1)
        assert out["flags"] == DM.BAD_HOST | DM.OUT_OVERFLOW and "dst_host" in out["msg"] and "out_cap" in out["msg"]
    finally:
        p.close()


def case_walk_bounded_on_the_device(make):
    """n_pkts past what the window holds (the flight pop's out_cap): the walk ends at dst_ptr[n_hosts];
    and dst_ptr past n_pkts: the walk ends at n_pkts"""
    p = _Pair(make, 2)
    try:
        assert p.associate(assoc((0, DM.TCP, 0, 9, 0, 1), (1, DM.TCP, 0, 9, 0, 2)))
        p.note(meta(*[(1, 2, 9, DM.TCP, k) for k in range(8)]), 0)
        tag, st, fw = np.arange(8), [FWD, QUEUED, FWD, FWD] + [FWD] * 4, [1, 2, 3, 4, 0, 0, 0, 0]
        out = p.run([0, 2, 4], tag, st, fw, 0, n_pkts=8)
        assert out["user"].tolist() == [0, 2, 3] and out["host_ptr"].tolist() == [0, 1, 3]
        out = p.run([0, 2, 9], tag, st, fw, 8, n_pkts=3, late=[(1, 0, FWD, 0)])
        assert out["user"].tolist() == [1, 0, 2] and out["host_ptr"].tolist() == [0, 2, 3]
    finally:
        p.close()


CASES = [case_lookup_rules, case_empty_table, case_table_maintenance, case_probe_chain_wraps,
         case_late_lookup_at_delivery, case_late_runs_around_the_sort_capacity, case_log_overrun, case_note_overrun,
         case_out_overflow_and_bad_host, case_walk_bounded_on_the_device]


def error_paths(plan_handle=None):
    """null arguments and SRT_ERR_INVALID of the entry points, on raw ctypes"""
    from shadow_amd import _lib

    L, err, h = _lib.lib(), _lib.SrtErr(), C.c_void_p()
    inv, ok = _lib.SRT_ERR_INVALID, _lib.SRT_OK
    assert L.srt_deliver_create(plan_handle, 2, 8, 4, 4, None, C.byref(err)) == inv and b"null" in err.msg
    assert L.srt_deliver_create(plan_handle, 0xffffffff, 8, 4, 4, C.byref(h), C.byref(err)) == inv and not h
    assert L.srt_deliver_create(plan_handle, 2, 8, (1 << 31) + 1, 4, C.byref(h), C.byref(err)) == inv and b"note_cap" in err.msg
    assert L.srt_deliver_create(plan_handle, 2, 8, 4, (1 << 31) + 1, C.byref(h), C.byref(err)) == inv
    assert L.srt_deliver_status(None, None, None, None, C.byref(err)) == inv and b"null" in err.msg
    assert L.srt_deliver_associate(None, None, 0, C.byref(err)) == inv
    assert L.srt_deliver_disassociate(None, None, 0, C.byref(err)) == inv
    assert L.srt_deliver_lookup(None, None, None, 0, None, C.byref(err)) == inv
    assert L.srt_deliver_table_stats(None, None, None, None, None, C.byref(err)) == inv
    assert L.srt_deliver_note(None, None, 0, 0, C.byref(err)) == inv
    assert L.srt_deliver_run(None, None, 0, None, None, None, 0, None, 0, None, None, None, None, None, None, None, 0,
                             C.byref(err)) == inv
    L.srt_deliver_destroy(None)
    if plan_handle is not None:
        return
    assert L.srt_deliver_create(None, 2, 8, 4, 4, C.byref(h), C.byref(err)) == ok
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    a = assoc((0, DM.TCP, 0, 9, 0, 1))
    assert L.srt_deliver_associate(h, None, 1, C.byref(err)) == inv and b"null" in err.msg
    assert L.srt_deliver_disassociate(h, None, 1, C.byref(err)) == inv
    assert L.srt_deliver_associate(h, None, 0, C.byref(err)) == ok
    assert L.srt_deliver_associate(h, p(a), 1, C.byref(err)) == ok
    assert L.srt_deliver_associate(h, p(a), 1, C.byref(err)) == inv and b"exists" in err.msg
    ms = meta((1, 2, 9, DM.TCP, 40), (1, 2, 9, DM.TCP, 41))
    hosts, socks = np.array([0, 1], np.uint32), np.zeros(2, np.uint32)
    assert L.srt_deliver_lookup(h, p(hosts), None, 2, p(socks), C.byref(err)) == inv
    assert L.srt_deliver_lookup(h, p(hosts), p(ms), 2, p(socks), C.byref(err)) == ok and socks.tolist() == [1, DM.NONE32]
    assert L.srt_deliver_table_stats(h, None, None, None, None, None) == ok
    assert L.srt_deliver_note(h, None, 2, 0, C.byref(err)) == inv
    assert L.srt_deliver_note(h, p(ms), 1 << 31, 0, C.byref(err)) == inv
    assert L.srt_deliver_note(h, p(ms), 2, 5, C.byref(err)) == ok
    assert L.srt_deliver_note(h, p(ms), 2, 6, C.byref(err)) == inv and b"tag_base" in err.msg
    dp, tag = np.array([0, 1, 2], np.uint32), np.array([5, 6], np.uint64)
    st, fw = np.array([FWD, FWD], np.uint32), np.array([7, 8], np.uint64)
    late, cnt = np.zeros(1, DM.LATE), np.zeros(1, np.uint32)
    o4 = [np.zeros(2, np.uint32) for _ in range(3)]
    o8 = [np.zeros(2, np.uint64) for _ in range(2)]
    ohp = np.full(3, 9, np.uint32)

    def run(f=h, dp=dp, n=2, tag=tag, st=st, fw=fw, late=late, late_cap=1, cnt=cnt, ohp=ohp, sock=o4[0], ofw=o8[0],
            otag=o8[1], user=o4[1], ost=o4[2], out_cap=2):
        return L.srt_deliver_run(f, p(dp), n, p(tag), p(st), p(fw), 0, p(late), late_cap, p(cnt), p(ohp), p(sock),
                                 p(ofw), p(otag), p(user), p(ost), out_cap, C.byref(err))

    for bad in (dict(f=None), dict(dp=None), dict(tag=None), dict(st=None), dict(fw=None), dict(late=None),
                dict(cnt=None), dict(ohp=None), dict(sock=None), dict(ofw=None), dict(otag=None), dict(user=None),
                dict(ost=None), dict(n=1 << 31), dict(late_cap=1 << 31)):
        assert run(**bad) == inv, bad
        assert err.code == inv and err.msg
    # nothing to write: no arrays needed; two are delivered, so the call overflows and says how many
    assert run(sock=None, ofw=None, otag=None, user=None, ost=None, out_cap=0, late=None, cnt=None, late_cap=0) == ok
    flags, a8, b8 = C.c_uint32(), C.c_uint64(), C.c_uint64()
    assert L.srt_deliver_status(h, C.byref(flags), C.byref(a8), C.byref(b8), C.byref(err)) == inv
    assert (flags.value, a8.value) == (_lib.DELIVER_OUT_OVERFLOW, 2) and b"out_cap" in err.msg and ohp.tolist() == [0, 0, 0]
    assert L.srt_deliver_status(h, C.byref(flags), None, None, C.byref(err)) == ok and flags.value == 0
    assert run() == ok and ohp.tolist() == [0, 1, 2] and o4[0].tolist() == [1, DM.NONE32] and o4[1].tolist() == [40, 41]
    assert L.srt_deliver_status(h, None, C.byref(a8), C.byref(b8), None) == ok and (a8.value, b8.value) == (2, 1)
    L.srt_deliver_destroy(h)
