#!/usr/bin/env python3
"""Times srt_loopback_run at the C5 size -- 1M packets over 10k hosts, four
sockets a host (40k socket slots) -- with HIP events on the plan's stream around
one call on a warmed instance, once with one instant a host and once with eight,
in both qdiscs.  Beside it, in the same process:

  (a) the path it replaces, with torch on the device for the round-robin order:
      a stable sort by (host, instant, socket), the rank of a packet within its
      socket and the arrival index of the socket's first packet from scans, a
      stable sort by (host, instant, rank, first); index_add_ of the out and in
      counters into the per-host and per-slot records (device ms by HIP events
      on torch's stream); and the copies a host-side lookup needs -- the metas
      to the host, the sockets back -- as wall ms with the device synchronised
      around them.  Its order and counts are compared with the stage's, outside
      the timed regions;
  (b) the project's own stages doing the same kinds of work unfused for remote
      traffic at that shape: srt_outbound_run (125 MB/s a host: uncongested),
      srt_deliver_run on an uncongested srt_inbound_run window, srt_tracker_tx
      and srt_tracker_rx, HIP events around each call, summed.

Writes the raw samples to profiles/loopback_c5.json and prints a summary line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--packets", type=int, default=1_000_000)
    ap.add_argument("--hosts", type=int, default=10_000)
    ap.add_argument("--sockets", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loopback_c5.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20 (the median of fewer samples is not reported)")

    import torch

    from shadow_amd import LoopbackRelay, NetworkGraph, Tracker, _lib, synth
    from shadow_amd.plan import (ASSOC_DTYPE, OUT_PKT_DTYPE, RX_META_DTYPE, TRK_COUNTER_FIELDS, TRK_META_DTYPE,
                                 DeliverStage, InboundRouter, OutboundRelay, RoutingPlan)

    _lib.require_device()
    hosts, n, S, seed, W = args.hosts, args.packets, args.sockets, 5, 5 * synth.MS
    src, dst, lat, loss = synth.complete_graph(16, seed)
    plan = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32),
                       device=0).run()
    rng = np.random.default_rng(seed)
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
    z = lambda k, dt: torch.zeros(k, dtype=dt, device=dev)  # noqa: E731
    stream = torch.cuda.ExternalStream(plan.stream_ptr(), device=dev)
    cur = torch.cuda.current_stream(dev)
    r0, n_slots = 1_000_000_000, hosts * S

    def timed(fn, s=stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        plan.sync()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    def trk_meta(k, slots):
        m = np.zeros(k, TRK_META_DTYPE)
        m["header_size"] = rng.choice(np.array([20, 32, 40, 60], np.uint32), size=k)
        m["payload_size"] = np.where(rng.random(k) < 0.4, 0, rng.integers(1, 1441, size=k))
        m["flags"] = rng.random(k) < 0.1
        m["socket_slot"] = slots
        return m

    # the associations of both interfaces: per host two wildcards and two specific keys, named by slot
    ports, peers = np.array([0x5000, 0xBB01], np.uint16), np.array([0x0100000A, 0x0200000A, 0x0300000A], np.uint32)
    assoc = np.zeros(hosts * S, ASSOC_DTYPE)
    assoc["host"] = np.repeat(np.arange(hosts), S)
    k = np.tile(np.arange(S), hosts)
    assoc["protocol"] = np.where(k % 2 == 0, _lib.PROTO_TCP, _lib.PROTO_UDP)
    assoc["local_port_be"] = ports[(k // 2) % 2]
    spec = k >= S // 2
    assoc["peer_ip_be"] = np.where(spec, peers[k % 3] + (k // 4 << 24), 0)
    assoc["peer_port_be"] = np.where(spec, 0x901F, 0)
    assoc["socket"] = assoc["host"] * S + k

    def rx_metas():
        m = np.zeros(n, RX_META_DTYPE)
        m["peer_ip_be"] = peers[rng.integers(0, 3, size=n)]
        m["peer_port_be"] = np.where(rng.random(n) < 0.8, 0x901F, 0x3500)
        m["local_port_be"] = np.where(rng.random(n) < 0.9, ports[rng.integers(0, 2, size=n)], 0x1111)
        m["protocol"] = np.where(rng.random(n) < 0.5, _lib.PROTO_TCP, _lib.PROTO_UDP)
        m["user"] = np.arange(n)
        return m

    # ---- the loopback batch: the hosts' packets, `instants` instants a host
    h = np.sort(rng.integers(0, hosts, size=n))
    host_ptr = np.searchsorted(h, np.arange(hosts + 1)).astype(np.int32)
    sock = rng.integers(0, S, size=n)
    lo_trk = trk_meta(n, h * S + sock)
    lo_rx = rx_metas()
    lo_dl = DeliverStage(plan, hosts, 8, 0, 0)
    lo_dl.associate(assoc)
    d_hp, d_rx, d_trk = t(host_ptr, np.int32), t(lo_rx.view(np.uint8), np.uint8), t(lo_trk.view(np.uint8), np.uint8)
    d_host = t(h, np.int64)
    outs = [z(n, torch.int32), z(n, torch.int32), z(n, torch.int64), z(n, torch.int32), z(n, torch.int32)]

    def batch(instants):
        pk = np.zeros(n, OUT_PKT_DTYPE)
        inst = rng.integers(0, instants, size=n)
        pk["ready_ns"] = r0 + np.sort(h * instants + inst) - h * instants  # nondecreasing within a host
        pk["priority"] = rng.permutation(n)
        pk["socket"] = sock
        return pk

    def torch_rr(d_ready, d_sock):
        """the replaced order, round robin -> the batch index at every output position"""
        idx = torch.arange(n, device=dev)
        grp = (d_host << 20) + (d_ready - d_ready.min())  # (host, instant); fewer than 2^20 instants
        o1 = torch.sort((grp << 8) + d_sock, stable=True).indices  # by socket within the instant, arrival order kept
        g1 = ((grp << 8) + d_sock)[o1]
        start = torch.ones(n, dtype=torch.bool, device=dev)
        start[1:] = g1[1:] != g1[:-1]
        seg0 = torch.cummax(torch.where(start, idx, torch.zeros_like(idx)), 0).values  # where the socket's run begins
        rank = idx - seg0
        first = o1[seg0] - d_hp.to(torch.int64)[d_host[o1]]  # arrival index of its first packet, within the host
        key = (((grp[o1] << 10) + rank) << 12) + first  # below 2^63 at this shape (asserted below)
        return o1[torch.sort(key, stable=True).indices]

    def torch_counts(keep_in, slot_in):
        """index_add_ of the out and the in counters -> four [., 10] int64 arrays"""
        m = d_trk.view(torch.int32).view(-1, 4).to(torch.int64) & 0xFFFFFFFF
        data, rt = m[:, 1] > 0, (m[:, 2] & 1) != 0
        col = torch.where(data, torch.where(rt, 7, 4), torch.where(rt, 2, 0))
        one = torch.ones_like(col)
        res = []
        for keep, slot in ((None, m[:, 3]), (keep_in, slot_in.to(torch.int64))):
            node, slots = z(hosts * 10, torch.int64), z(n_slots * 10, torch.int64)
            for rec, key in ((node, d_host), (slots, slot)):
                kk = torch.ones_like(data) if keep is None else keep
                base = key[kk] * 10 + col[kk]
                rec.index_add_(0, base, one[kk])
                rec.index_add_(0, base + 1, m[:, 0][kk])
                both = kk & data
                rec.index_add_(0, key[both] * 10 + col[both] + 2, m[:, 1][both])
            res += [node.view(hosts, 10), slots.view(n_slots, 10)]
        return res  # node_out, slot_out, node_in, slot_in

    def as_matrix(rec):
        return np.stack([rec[f] for f in TRK_COUNTER_FIELDS], axis=1).astype(np.int64)

    shapes, same = {}, True
    for instants in (1, 8):
        pk = batch(instants)
        assert hosts < 1 << 20 and instants < 1 << 10 and int(np.diff(host_ptr).max()) < 1 << 10
        d_pk = t(pk.view(np.uint8), np.uint8)
        d_ready, d_sock = t(pk["ready_ns"], np.int64), t(pk["socket"].astype(np.int64), np.int64)
        smp = {"fifo_ms": [], "rr_ms": [], "torch_order_ms": [], "torch_counts_ms": [], "copies_ms": []}
        lbs = {q: LoopbackRelay(plan, hosts, q, S, n_slots) for q in (_lib.QDISC_FIFO, _lib.QDISC_RR)}
        longest = int(np.unique(h.astype(np.int64) * 1024 + (pk["ready_ns"].astype(np.int64) - r0),
                                return_counts=True)[1].max())
        outcome = {}
        for rep in range(args.warmup + args.reps):
            ms = {}
            if rep:  # the same batch, 16 ns later: a host's arrivals never go back in time
                d_pk.view(torch.int64).view(-1, 4)[:, 0] += 16
                d_ready += 16
            for name, q in (("fifo_ms", _lib.QDISC_FIFO), ("rr_ms", _lib.QDISC_RR)):
                ms[name] = timed(lambda: lbs[q].run(lo_dl, d_pk, d_hp, d_rx, d_trk, *outs))
                flags, n_recv, n_miss = lbs[q].status()
                got = lbs[q].heartbeat()
                same = same and flags == 0 and n_recv == n
            res = {}
            ms["torch_order_ms"] = timed(lambda: res.__setitem__("order", torch_rr(d_ready, d_sock)), cur)
            sock_by_pkt = torch.empty_like(outs[1])
            sock_by_pkt[outs[0].to(torch.int64)] = outs[1]  # the sockets a host-side lookup would return
            ms["torch_counts_ms"] = timed(
                lambda: res.__setitem__("counts", torch_counts(sock_by_pkt != -1, sock_by_pkt)), cur)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            d_rx.cpu()
            t(np.zeros(n, np.int32), np.int32)
            torch.cuda.synchronize(dev)
            ms["copies_ms"] = (time.perf_counter() - t0) * 1e3
            same = same and bool(torch.equal(res["order"], outs[0].to(torch.int64)))  # the last run was RR
            for a, b in zip((got[1], got[3], got[0], got[2]), res["counts"]):
                same = same and np.array_equal(as_matrix(a), b.cpu().numpy())
            outcome = {"received": n_recv, "no_socket": n_miss, "tasks": int(lbs[_lib.QDISC_RR].tasks().sum()),
                       "longest_instant": longest}
            if rep >= args.warmup:
                for name in smp:
                    smp[name].append(ms[name])
        for lb in lbs.values():
            lb.close()
        med = {f: statistics.median(v) for f, v in smp.items()}
        shapes[f"instants_{instants}"] = {"outcome": outcome, "median_ms": med, "samples": smp,
                                          "replaced_over_loopback_rr": (med["torch_order_ms"] + med["torch_counts_ms"] +
                                                                        med["copies_ms"]) / med["rr_ms"]}

    # ---- (b) the unfused stages at that shape, uncongested
    tx_meta = lo_trk
    pk = np.zeros(n, OUT_PKT_DTYPE)
    ready = r0 + rng.integers(0, W, size=n)
    pk["ready_ns"] = ready[np.lexsort((ready, h))]
    pk["priority"] = np.arange(n)
    pk["total_size"] = tx_meta["header_size"] + tx_meta["payload_size"]
    pk["socket"] = sock
    ob_args = dict(st=z(n, torch.int32), sn=z(n, torch.int64), rk=z(n, torch.int64), late=z(32 * 1024, torch.uint8),
                   cnt=z(1, torch.int32), cs=z(hosts, torch.int64), pk=t(pk.view(np.uint8), np.uint8))
    d = np.sort(rng.integers(0, hosts, size=n))
    dst_ptr = np.searchsorted(d, np.arange(hosts + 1)).astype(np.int32)
    deliver = r0 + rng.integers(0, W, size=n)
    deliver = deliver[np.lexsort((deliver, d))].astype(np.int64)
    tag = rng.permutation(n).astype(np.int64)
    note = np.zeros(n, RX_META_DTYPE)
    note[tag] = rx_metas()
    out_cap = 2 * n
    ds = DeliverStage(plan, hosts, 8, n, 2 * n)
    ds.associate(assoc)
    ds.note(t(note.view(np.uint8), np.uint8), 0)
    ib = InboundRouter(plan, np.full(hosts, 125_000_000, np.uint64), 512)
    rx = dict(dst_ptr=t(dst_ptr, np.int32), tag=t(tag, np.int64), st=z(n, torch.int32), fw=z(n, torch.int64),
              late=z(24 * 1024, torch.uint8), cnt=z(1, torch.int32), hp=z(hosts + 1, torch.int32),
              sock=z(out_cap, torch.int32), ofw=z(out_cap, torch.int64), otag=z(out_cap, torch.int64),
              user=z(out_cap, torch.int32), ost=z(out_cap, torch.int32),
              meta=t(trk_meta(n, 0).view(np.uint8), np.uint8))
    rx_base = ib.run(torch.arange(n, dtype=torch.int32, device=dev), rx["dst_ptr"], t(deliver, np.int64),
                     t(rng.integers(40, 1501, size=n).astype(np.int32), np.int32), r0 + W, 0, rx["st"], rx["fw"],
                     rx["late"], rx["cnt"])
    i_flags, i_pending = ib.status()
    trk = Tracker(plan, hosts, n_slots, n, 2 * n)
    trk.note(rx["meta"], 0)
    unf = {"outbound_ms": [], "deliver_ms": [], "tracker_tx_ms": [], "tracker_rx_ms": []}
    o_state = {}
    ob = OutboundRelay(plan, np.full(hosts, 125_000_000, np.uint64), _lib.QDISC_FIFO, S, 512)
    for rep in range(args.warmup + args.reps):
        if rep:  # the same window, W later
            ob_args["pk"].view(torch.int64).view(-1, 4)[:, 0] += W
        base = {}
        a = timed(lambda: base.__setitem__("b", ob.run(ob_args["pk"], d_hp, r0 + (rep + 1) * W, 0, ob_args["st"],
                                                        ob_args["sn"], ob_args["rk"], ob_args["late"],
                                                        ob_args["cnt"])))
        ob.cached_seq(ob_args["cs"])
        o_state = dict(zip(("flags", "pending"), ob.status()))
        b = timed(lambda: ds.run(rx["dst_ptr"], rx["tag"], rx["st"], rx["fw"], rx_base, rx["late"], rx["cnt"], rx["hp"],
                                 rx["sock"], rx["ofw"], rx["otag"], rx["user"], rx["ost"]))
        same = same and ds.status()[0] == 0
        c = timed(lambda: trk.tx(ob_args["cs"], d_hp, d_trk, ob_args["st"], base["b"], ob_args["late"], ob_args["cnt"]))
        e = timed(lambda: trk.rx(rx["hp"], rx["sock"], rx["otag"], rx["ost"]))
        same = same and trk.status()[0] == 0
        trk.heartbeat()
        if rep >= args.warmup:
            for name, v in zip(unf, (a, b, c, e)):
                unf[name].append(v)
    for obj in (trk, ds, ib, ob, lo_dl):
        obj.close()
    plan.close()
    unf_med = {f: statistics.median(v) for f, v in unf.items()}
    unf_sum = sum(unf_med.values())
    out = {"what": "srt_loopback_run at the C5 size, device ms per call (HIP events on the plan's stream around one call "
                   "on a warmed instance), one and eight instants a host, both qdiscs; beside it (a) the torch "
                   "formulation of the round-robin order and the counters (HIP events on torch's stream) plus the "
                   "copies a host-side lookup needs (wall ms), and (b) srt_outbound_run, srt_deliver_run, "
                   "srt_tracker_tx and srt_tracker_rx at the same shape, uncongested, summed",
           "measured_on": "MI355X", "packets": n, "hosts": hosts, "sockets_per_host": S, "socket_slots": n_slots,
           "warmup": args.warmup, "reps": args.reps, "outputs_equal_every_sample": bool(same),
           "loopback": {k: {kk: vv for kk, vv in v.items() if kk != "samples"} for k, v in shapes.items()},
           "unfused": {"outbound": o_state, "inbound": {"flags": i_flags, "pending": i_pending}, "median_ms": unf_med,
                       "sum_ms": unf_sum},
           "loopback_over_unfused": {k: {q: v["median_ms"][q] / unf_sum for q in ("fifo_ms", "rr_ms")}
                                     for k, v in shapes.items()},
           "samples": {"loopback": {k: v["samples"] for k, v in shapes.items()}, "unfused": unf}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "samples"}))
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
