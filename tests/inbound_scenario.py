"""The random scenario of the inbound router tests and the plumbing to feed
it to the model (tests/inbound_model.py) and to srt_inbound (host-only or on
the device), in one call or split into windows.  The model's outputs are
computed once per process and shared by the tests that compare against them.
"""
import functools

import numpy as np

from inbound_model import MS, U64, InboundModel

N_HOSTS = 130          # two waves of 64 hosts and a remainder
N_PKTS = 3000
SPAN_NS = 3000 * MS
BOOTSTRAP_END_NS = 400 * MS
UNTIL_NS = SPAN_NS + 50 * MS
BANDWIDTHS = (1_000, 125_000, 125_000_000)
EMPTY_HOST = 77        # receives nothing
HOT_HOSTS = (5, 63, 64, 129)
SEED = 3
SPLITS = 7
LATE_CAP = 4096
STATE_FIELDS = ("balance", "last_refill_ns", "interval_end_ns", "drop_next_ns", "current_drop_count",
                "previous_drop_count", "queue_len", "bytes_stored", "task_ns", "tasks_scheduled", "mode", "cached")


def event_order(dst, deliver, sent, n_hosts):
    """srt_packet_events' outputs for packets that all come from distinct
    (source host, event id) pairs in batch order: per destination, by
    (deliver time, batch index)."""
    idx = np.nonzero(sent)[0]
    o = idx[np.lexsort((idx, deliver[idx], dst[idx]))]
    dst_ptr = np.searchsorted(dst[o], np.arange(n_hosts + 1)).astype(np.uint32)
    return o.astype(np.uint32), dst_ptr


@functools.lru_cache(maxsize=None)
def scenario(seed=SEED):
    rng = np.random.default_rng(seed)
    bw = rng.choice(np.array(BANDWIDTHS, np.uint64), size=N_HOSTS, p=[0.25, 0.45, 0.30])
    # destinations: the slow and the middling hosts get bursts, one host nothing
    w = np.where(bw == 1_000, 1.5, np.where(bw == 125_000, 1.2, 0.5))
    w[EMPTY_HOST] = 0.0
    dst = rng.choice(N_HOSTS, size=N_PKTS, p=w / w.sum()).astype(np.uint32)
    # times from a small pool: many exact ties; half the pool on the 1 ms grid
    # the blocked relay's tasks fall on; bursts in the pool's dense regions
    grid = rng.integers(0, SPAN_NS // MS, size=160) * MS
    burst = (rng.integers(0, 12, size=120) * 250 * MS + rng.integers(0, 30 * MS, size=120))
    free = rng.integers(0, SPAN_NS, size=120)
    pool = np.concatenate([grid, burst, free]).astype(np.uint64)
    deliver = pool[rng.integers(0, len(pool), size=N_PKTS)]
    deliver = np.minimum(deliver, np.uint64(SPAN_NS - 1))
    size = rng.integers(40, 1501, size=N_PKTS).astype(np.uint32)
    size[rng.random(N_PKTS) < 0.4] = 1500
    # a few hot hosts at 125,000 B/s take three bursts each, far enough apart
    # for the queue to drain: Drop mode entered, left and entered again
    for k, h in enumerate(HOT_HOSTS):
        bw[h] = 125_000
        sel = slice(k * 150, (k + 1) * 150)
        dst[sel] = h
        t0 = (600 + 40 * k + 800 * (np.arange(150) // 50)) * MS
        jitter = np.where(rng.random(150) < 0.5, rng.integers(0, 20, size=150) * MS, rng.integers(0, 20 * MS, size=150))
        deliver[sel] = (t0 + jitter).astype(np.uint64)
    sent = rng.random(N_PKTS) < 0.95
    return dict(bw=bw, dst=dst, deliver=deliver, size=size, sent=sent)


def calls_of(sc, untils, n_hosts=N_HOSTS):
    """the stream cut into one call per window: packets with deliver time in
    [previous until, until), in batch order; ids = their global indices"""
    calls, lo = [], 0
    for u in untils:
        ids = np.nonzero((sc["deliver"] >= lo) & (sc["deliver"] < u))[0]
        order, dst_ptr = event_order(sc["dst"][ids], sc["deliver"][ids], sc["sent"][ids], n_hosts)
        calls.append(dict(ids=ids, order=order, dst_ptr=dst_ptr, deliver=sc["deliver"][ids].copy(),
                          size=sc["size"][ids].copy(), until=int(u)))
        lo = u
    return calls


def one_call(sc):
    return calls_of(sc, [UNTIL_NS])


def split_calls(sc):
    cuts = [UNTIL_NS * (k + 1) // SPLITS for k in range(SPLITS)]
    cuts[2] = 1200 * MS  # a cut on the 1 ms grid: arrivals and tasks exactly at a window's end
    return calls_of(sc, cuts)


def run_model(sc, calls, bootstrap_end=BOOTSTRAP_END_NS):
    m = InboundModel(sc["bw"])
    outs = []
    for c in calls:
        st, fw, late, base = m.run(c["order"], c["dst_ptr"], c["deliver"], c["size"], c["until"], bootstrap_end)
        outs.append(dict(status=st, forward=fw, late=late, base=base))
    return outs, m


@functools.lru_cache(maxsize=None)
def model_results(seed=SEED, split=False):
    sc = scenario(seed)
    calls = split_calls(sc) if split else one_call(sc)
    outs, m = run_model(sc, calls)
    return calls, outs, m


def run_lib(sc, calls, plan=None, queue_cap=N_PKTS, late_cap=LATE_CAP, bootstrap_end=BOOTSTRAP_END_NS, bw=None,
            check=True):
    """the same calls through srt_inbound -> (outs, state record array, [(flags, pending)] per call)"""
    from shadow_amd.plan import INBOUND_LATE_DTYPE, InboundRouter

    r = InboundRouter(plan, sc["bw"] if bw is None else bw, queue_cap)
    outs, stats = [], []
    try:
        for c in calls:
            n = len(c["deliver"])
            if plan is None:
                st = np.full(n, 0xdeadbeef, np.uint32)
                fw = np.zeros(n, np.uint64)
                late = np.zeros(late_cap * 24, np.uint8)
                cnt = np.zeros(1, np.uint32)
                base = r.run(c["order"], c["dst_ptr"], c["deliver"], c["size"], c["until"], bootstrap_end, st, fw,
                             late, cnt)
                stats.append(r.status(check=check))
            else:
                import torch

                dev = torch.device("cuda:0")
                t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
                t_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
                t_fw = torch.zeros(n, dtype=torch.int64, device=dev)
                t_late = torch.zeros(max(late_cap, 1) * 24, dtype=torch.uint8, device=dev)
                t_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
                base = r.run(t(c["order"], np.int32) if n else t_st, t(c["dst_ptr"], np.int32),
                             t(c["deliver"], np.int64), t(c["size"], np.int32), c["until"], bootstrap_end, t_st, t_fw,
                             t_late if late_cap else None, t_cnt)
                stats.append(r.status(check=check))
                st = t_st.cpu().numpy().view(np.uint32)
                fw = t_fw.cpu().numpy().view(np.uint64)
                late = t_late.cpu().numpy()
                cnt = t_cnt.cpu().numpy().view(np.uint32)
            k = min(int(cnt[0]), late_cap)
            recs = late[:k * 24].view(INBOUND_LATE_DTYPE)
            outs.append(dict(status=st, forward=fw, base=base, late_count=int(cnt[0]), late=sorted(
                (int(x["seq"]), int(x["forward_ns"]), int(x["status"]), int(x["dst_host"])) for x in recs)))
        return outs, r.state(), stats
    finally:
        r.close()


def assert_same(outs, mouts, state, model, hosts=None):
    """every status word, forward time, late record (sorted by seq) and state field"""
    for k, (o, m) in enumerate(zip(outs, mouts)):
        assert o["base"] == m["base"], k
        if hosts is None:
            assert np.array_equal(o["status"], m["status"]), (k, np.nonzero(o["status"] != m["status"])[0][:10])
            assert np.array_equal(o["forward"], m["forward"]), (k, np.nonzero(o["forward"] != m["forward"])[0][:10])
            assert o["late"] == m["late"], k
    for h, ms in enumerate(model.state()):
        if hosts is not None and h not in hosts:
            continue
        for f in STATE_FIELDS:
            assert int(state[f][h]) == ms[f], (h, f, int(state[f][h]), ms[f])


def resolved(calls, outs):
    """global packet id -> (status, forward) of every packet that left the stage"""
    from inbound_model import DROPPED, FORWARDED

    res = {}
    bases = [(o["base"], c["ids"]) for c, o in zip(calls, outs)]
    for c, o in zip(calls, outs):
        for i, g in enumerate(c["ids"]):
            if o["status"][i] & (DROPPED | FORWARDED):
                res[int(g)] = (int(o["status"][i]), int(o["forward"][i]))
        for seq, fwd, st, _ in o["late"]:
            b, ids = [x for x in bases if x[0] <= seq < x[0] + len(x[1])][0]
            res[int(ids[seq - b])] = (st, fwd)
    return res


assert U64  # re-exported for the tests
