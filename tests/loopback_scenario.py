"""Scenarios for srt_loopback: generators, the runner over the library (host-only
with plan=None, or on a plan's device) and over the model (loopback_model.py),
and the comparison.  A scenario is a list of steps:
  ("assoc", recs) / ("disassoc", recs)   the loopback interface's associations
  ("run", call)                          call: pkts, host_ptr, rx_meta, trk_meta
  ("beat", hosts, slots)                 a heartbeat on a selection (None: all)
Every run is followed by status and tasks in both runners."""
import numpy as np

import loopback_model as LM

OUT_PKT = np.dtype([("ready_ns", "<u8"), ("priority", "<u8"), ("total_size", "<u4"), ("socket", "<u4"),
                    ("flags", "<u4"), ("reserved", "<u4")])
RX_META = np.dtype([("peer_ip_be", "<u4"), ("peer_port_be", "<u2"), ("local_port_be", "<u2"), ("protocol", "<u4"),
                    ("user", "<u4")])
ASSOC = np.dtype([("host", "<u4"), ("protocol", "<u4"), ("peer_ip_be", "<u4"), ("local_port_be", "<u2"),
                  ("peer_port_be", "<u2"), ("socket", "<u4")])
TRK_META = LM.TM.TRK_META
LOCALHOST_BE = 0x0100007F
OUT_FIELDS = ("index", "socket", "recv_ns", "user", "status")


def associations(n_hosts, max_sockets):
    """socket d of a host listens on port 1000 + d: d % 3 == 0 a specific TCP key (peer 127.0.0.1:2000 + d),
    d % 3 == 1 a UDP wildcard, d % 3 == 2 nothing.  The socket's name is its global slot."""
    recs = []
    for h in range(n_hosts):
        for d in range(max_sockets):
            if d % 3 == 0:
                recs.append((h, LM.TCP, LOCALHOST_BE, 1000 + d, 2000 + d, h * max_sockets + d))
            elif d % 3 == 1:
                recs.append((h, LM.UDP, 0, 1000 + d, 0, h * max_sockets + d))
    return np.array(recs, ASSOC)


class Gen:
    """per-host clocks and priorities that go on from call to call"""

    def __init__(self, seed, n_hosts, max_sockets):
        self.rng = np.random.default_rng(seed)
        self.n_hosts, self.max_sockets = n_hosts, max_sockets
        self.now = self.rng.integers(1, 1000, size=n_hosts).astype(np.int64) * 1000
        self.serial = 0

    def call(self, counts, group_max=9, single=False, continue_hosts=()):
        """counts[h] packets of host h, cut into instants of 1..group_max packets (single: one instant);
        a host in continue_hosts begins with the instant its previous call ended with"""
        rng, ms = self.rng, self.max_sockets
        n = int(np.sum(counts))
        pkts, rx, trk = np.zeros(n, OUT_PKT), np.zeros(n, RX_META), np.zeros(n, TRK_META)
        host_ptr = np.zeros(self.n_hosts + 1, np.uint32)
        i = 0
        for h in range(self.n_hosts):
            left, first = int(counts[h]), True
            while left:
                g = left if single else min(left, int(rng.integers(1, group_max + 1)))
                if not (first and h in continue_hosts):
                    self.now[h] += int(rng.integers(1, 5000))
                first = False
                socks = rng.choice(ms, size=min(ms, int(rng.integers(1, 6))), replace=False)
                for _ in range(g):
                    s, d = int(rng.choice(socks)), int(rng.integers(0, ms))
                    self.serial += 1
                    # distinct within a host, not monotone in arrival order
                    pkts[i] = (self.now[h], int(rng.integers(0, 1 << 40)) << 22 | self.serial, 0, s, 0, 0)
                    proto = 7 if rng.random() < 0.05 else (LM.UDP if d % 3 == 1 else LM.TCP)
                    peer = (LOCALHOST_BE, 2000 + d) if d % 3 == 0 else (int(rng.integers(1, 1 << 32)), 3000 + s)
                    if d % 3 == 0 and rng.random() < 0.1:
                        peer = (LOCALHOST_BE, 2999)  # the specific key misses and there is no wildcard
                    rx[i] = (peer[0], peer[1], 1000 + d, proto, self.serial)
                    payload = 0 if rng.random() < 0.3 else int(rng.integers(1, 1400))
                    trk[i] = (int(rng.integers(20, 61)), payload, int(rng.random() < 0.2), h * ms + s)
                    i += 1
                left -= g
            host_ptr[h + 1] = i
        return dict(pkts=pkts, host_ptr=host_ptr, rx_meta=rx, trk_meta=trk)


MAIN_HOSTS, MAIN_SOCKETS = 37, 7


def main_scenario():
    """three calls over 37 hosts, a few hundred packets; a selective heartbeat and a table change between
    calls; hosts 0..9 continue call 1's last instant in call 2"""
    n_hosts, ms = MAIN_HOSTS, MAIN_SOCKETS
    g = Gen(5, n_hosts, ms)
    counts = [g.rng.integers(0, 14, size=n_hosts) for _ in range(3)]
    for c in counts:
        c[3] = 0  # a host with no packets at all
    counts[0][:10] = np.maximum(counts[0][:10], 2)
    counts[1][:10] = np.maximum(counts[1][:10], 2)
    counts[1][20] = 40
    assoc = associations(n_hosts, ms)
    steps = [("assoc", assoc), ("run", g.call(counts[0])),
             ("beat", np.array([1, 5, 5, 30], np.uint32), np.array([1 * ms, 5 * ms + 1, 30 * ms + 2], np.uint32)),
             ("disassoc", assoc[::5]), ("run", g.call(counts[1], group_max=14, continue_hosts=set(range(10)))),
             ("run", g.call(counts[2])), ("beat", None, None)]
    return dict(n_hosts=n_hosts, max_sockets=ms, n_slots=n_hosts * ms, steps=steps)


def split_call(call, n_hosts):
    """one call as two, cut at an instant boundary inside every host (the instants of a call are its own)"""
    pk, hp = call["pkts"], call["host_ptr"].astype(np.int64)
    first, second = [], []
    for h in range(n_hosts):
        b, e = hp[h], hp[h + 1]
        t = pk["ready_ns"][b:e]
        cuts = [k for k in range(1, e - b) if t[k] != t[k - 1]]
        c = b + (cuts[len(cuts) // 2] if cuts else e - b)
        first.append(np.arange(b, c))
        second.append(np.arange(c, e))

    def part(sel):
        ids = np.concatenate(sel) if sel else np.zeros(0, np.int64)
        ptr = np.zeros(n_hosts + 1, np.uint32)
        ptr[1:] = np.cumsum([len(s) for s in sel])
        return dict(pkts=pk[ids], host_ptr=ptr, rx_meta=call["rx_meta"][ids], trk_meta=call["trk_meta"][ids], ids=ids)

    return part(first), part(second)


def split_scenario(sc):
    steps = []
    for st in sc["steps"]:
        if st[0] == "run":
            a, b = split_call(st[1], sc["n_hosts"])
            steps += [("run", a), ("run", b)]
        else:
            steps.append(st)
    return dict(sc, steps=steps)


def run_model(sc, qdisc, n_slots=None):
    m = LM.LoopbackModel(sc["n_hosts"], qdisc, sc["max_sockets"], sc["n_slots"] if n_slots is None else n_slots)
    outs, beats, stats = [], [], []
    for st in sc["steps"]:
        if st[0] == "assoc":
            m.associate(st[1])
        elif st[0] == "disassoc":
            m.disassociate(st[1])
        elif st[0] == "beat":
            beats.append(m.heartbeat(st[1], st[2]))
        else:
            c = st[1]
            outs.append(dict(zip(OUT_FIELDS, m.run(c["pkts"], c["host_ptr"], c["rx_meta"], c.get("trk_meta")))))
            stats.append((m.status(), list(m.tasks)))
    return outs, beats, stats, m


def run_lib(sc, qdisc, plan=None, n_slots=None, table_slots_min=8):
    """the same steps through LoopbackRelay and DeliverStage; status never raises here (flags are compared)"""
    from shadow_amd import LoopbackRelay
    from shadow_amd.plan import DeliverStage

    if plan is not None:
        import torch

        dev = torch.device("cuda:0")
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
        new = lambda n, dt: torch.full((n,), 0x5A, dtype=dt, device=dev)  # noqa: E731
        down = lambda t, dt: t.cpu().numpy().view(dt)  # noqa: E731
        i32, i64 = torch.int32, torch.int64
    else:
        up = lambda a, dt: np.ascontiguousarray(a).view(dt).copy()  # noqa: E731
        new = lambda n, dt: np.full(n, 0x5A, dt)  # noqa: E731
        down = lambda t, dt: t.view(dt)  # noqa: E731
        i32, i64 = np.int32, np.int64
    n_slots = sc["n_slots"] if n_slots is None else n_slots
    dl = DeliverStage(plan, sc["n_hosts"], table_slots_min, 0, 0)
    lb = LoopbackRelay(plan, sc["n_hosts"], qdisc, sc["max_sockets"], n_slots)
    outs, beats, stats = [], [], []
    try:
        for st in sc["steps"]:
            if st[0] == "assoc":
                dl.associate(st[1])
            elif st[0] == "disassoc":
                dl.disassociate(st[1])
            elif st[0] == "beat":
                beats.append(lb.heartbeat(st[1], st[2]))
            else:
                c = st[1]
                n = len(c["pkts"])
                o = [new(n, i32), new(n, i32), new(n, i64), new(n, i32), new(n, i32)]
                trk = c.get("trk_meta")
                lb.run(dl, up(c["pkts"].view(np.uint8), np.uint8), up(c["host_ptr"], np.int32),
                       up(c["rx_meta"].view(np.uint8), np.uint8),
                       None if trk is None else up(trk.view(np.uint8), np.uint8), *o)
                outs.append(dict(zip(OUT_FIELDS, (down(o[0], np.uint32), down(o[1], np.uint32), down(o[2], np.uint64),
                                                  down(o[3], np.uint32), down(o[4], np.uint32)))))
                stats.append((lb.status(check=False), lb.tasks().tolist()))
    finally:
        lb.close()
        dl.close()
    return outs, beats, stats


def same_records(got, want, where=""):
    for name, a, b in zip(("node_in", "node_out", "slot_in", "slot_out"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (where, name)
        if a.tobytes() != b.tobytes():
            k = int(np.nonzero(a != b)[0][0])
            raise AssertionError(f"{where} {name}[{k}]: {a[k]} != {b[k]}")


def assert_same(got, want, where=""):
    """(outs, beats, stats) of two runners, byte for byte"""
    outs, beats, stats = got
    w_outs, w_beats, w_stats = want
    assert len(outs) == len(w_outs) and len(beats) == len(w_beats) and stats == w_stats, (where, stats, w_stats)
    for k, (a, b) in enumerate(zip(outs, w_outs)):
        for f in OUT_FIELDS:
            if a[f].tobytes() != b[f].tobytes():
                i = int(np.nonzero(a[f] != b[f])[0][0])
                raise AssertionError(f"{where} call {k} {f}[{i}]: {a[f][i]} != {b[f][i]}")
    for k, (a, b) in enumerate(zip(beats, w_beats)):
        same_records(a, b, f"{where} beat {k}")


def check(sc, qdisc, plan=None, n_slots=None):
    """the library (plan or host-only) against the model; returns both results"""
    m_outs, m_beats, m_stats, m = run_model(sc, qdisc, n_slots)
    got = run_lib(sc, qdisc, plan, n_slots)
    assert_same(got, (m_outs, m_beats, m_stats), "lib vs model")
    return got, (m_outs, m_beats, m_stats), m


def shape_scenario(seed, n_hosts, max_sockets, counts, single=False, group_max=9):
    """one call of counts[h] packets a host and a heartbeat on everything"""
    g = Gen(seed, n_hosts, max_sockets)
    steps = [("assoc", associations(n_hosts, max_sockets)), ("run", g.call(np.asarray(counts), group_max, single)),
             ("beat", None, None)]
    return dict(n_hosts=n_hosts, max_sockets=max_sockets, n_slots=n_hosts * max_sockets, steps=steps)


def flag_scenario(kind):
    """five hosts, two calls; host 2 is flagged in the second call: "time" (its first arrival lies below
    its last instant of call 1), "time_inside" (a regression inside the call) or "socket"."""
    g = Gen(9, 5, 4)
    c1, c2 = g.call(np.array([6, 5, 7, 0, 8])), g.call(np.array([5, 9, 6, 3, 4]))
    b, e = int(c2["host_ptr"][2]), int(c2["host_ptr"][3])
    if kind == "time":
        c2["pkts"]["ready_ns"][b] = c1["pkts"]["ready_ns"][int(c1["host_ptr"][3]) - 1] - 1
    elif kind == "time_inside":
        c2["pkts"]["ready_ns"][e - 1] = c2["pkts"]["ready_ns"][e - 2] - 1
    else:
        c2["pkts"]["socket"][b + 2] = 4  # == max_sockets
    steps = [("assoc", associations(5, 4)), ("run", c1), ("run", c2), ("run", g.call(np.array([2, 2, 2, 2, 2]))),
             ("beat", None, None)]
    return dict(n_hosts=5, max_sockets=4, n_slots=20, steps=steps)
