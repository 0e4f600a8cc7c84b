#!/usr/bin/env python3
"""Times srt_tracker_tx and srt_tracker_rx at the C5 size -- 1M packets a window
over 10k hosts, four sockets a host (40k socket slots) -- with HIP events on the
plan's stream around one call on a warmed instance.  tx counts the batch of a
real srt_outbound_run call (125 MB/s a host: every packet is popped in its own
window), rx the delivery list of a real srt_inbound_run -> srt_deliver_run
window.  Beside them, in the same process and on the same inputs:

  * the path they replace: the same counts with torch on the device (the host of
    every packet from the grouping, the class from the meta, index_add_ into the
    per-host and per-slot records), device ms by HIP events on torch's stream;
    and the copies to the host that a per-round host classification needs (tx:
    status and metas; rx: socket, tag and status of the list), wall ms with the
    device synchronised around them.  The torch counts are compared with the
    stage's heartbeat records, outside the timed regions;
  * srt_deliver_run, the call rx follows, as the yardstick: HIP events around
    the call on the same window.

Writes the raw samples to profiles/tracker_c5.json and prints a summary line.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracker_c5.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20 (the median of fewer samples is not reported)")

    import torch

    from shadow_amd import NetworkGraph, Tracker, _lib, synth
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
    r0, n_slots = 1_000_000_000, hosts * S

    def trk_meta(k, slots):
        m = np.zeros(k, TRK_META_DTYPE)
        m["header_size"] = rng.choice(np.array([20, 32, 40, 60], np.uint32), size=k)
        m["payload_size"] = np.where(rng.random(k) < 0.4, 0, rng.integers(1, 1441, size=k))
        m["flags"] = rng.random(k) < 0.1
        m["socket_slot"] = slots
        return m

    # ---- the output side: one srt_outbound_run call, uncongested
    h = np.sort(rng.integers(0, hosts, size=n))
    host_ptr = np.searchsorted(h, np.arange(hosts + 1)).astype(np.int32)
    sock = rng.integers(0, S, size=n)
    tx_meta = trk_meta(n, h * S + sock)
    ready = r0 + rng.integers(0, W, size=n)
    pk = np.zeros(n, OUT_PKT_DTYPE)
    pk["ready_ns"] = ready[np.lexsort((ready, h))]
    pk["priority"] = np.arange(n)
    pk["total_size"] = tx_meta["header_size"] + tx_meta["payload_size"]
    pk["socket"] = sock
    ob = OutboundRelay(plan, np.full(hosts, 125_000_000, np.uint64), _lib.QDISC_FIFO, S, 512)
    tx = dict(hp=t(host_ptr, np.int32), meta=t(tx_meta.view(np.uint8), np.uint8), st=z(n, torch.int32),
              sn=z(n, torch.int64), rk=z(n, torch.int64), late=z(32 * 1024, torch.uint8), cnt=z(1, torch.int32),
              cs=z(hosts, torch.int64))
    tx_base = ob.run(t(pk.view(np.uint8), np.uint8), tx["hp"], r0 + W, 0, tx["st"], tx["sn"], tx["rk"], tx["late"],
                     tx["cnt"])
    ob.cached_seq(tx["cs"])
    o_flags, o_pending = ob.status()

    # ---- the input side: one window through srt_inbound_run and srt_deliver_run, uncongested
    ports, peers = np.array([0x5000, 0xBB01], np.uint16), np.array([0x0100000A, 0x0200000A, 0x0300000A], np.uint32)
    assoc = np.zeros(hosts * S, ASSOC_DTYPE)
    assoc["host"] = np.repeat(np.arange(hosts), S)
    k = np.tile(np.arange(S), hosts)
    assoc["protocol"] = np.where(k % 2 == 0, _lib.PROTO_TCP, _lib.PROTO_UDP)
    assoc["local_port_be"] = ports[(k // 2) % 2]
    spec = k >= S // 2
    assoc["peer_ip_be"] = np.where(spec, peers[k % 3] + (k // 4 << 24), 0)
    assoc["peer_port_be"] = np.where(spec, 0x901F, 0)
    assoc["socket"] = assoc["host"] * S + k  # the association's name is its global slot
    d = np.sort(rng.integers(0, hosts, size=n))
    dst_ptr = np.searchsorted(d, np.arange(hosts + 1)).astype(np.int32)
    deliver = r0 + rng.integers(0, W, size=n)
    deliver = deliver[np.lexsort((deliver, d))].astype(np.int64)
    rxm = np.zeros(n, RX_META_DTYPE)
    rxm["peer_ip_be"] = peers[rng.integers(0, 3, size=n)]
    rxm["peer_port_be"] = np.where(rng.random(n) < 0.8, 0x901F, 0x3500)
    rxm["local_port_be"] = np.where(rng.random(n) < 0.9, ports[rng.integers(0, 2, size=n)], 0x1111)
    rxm["protocol"] = np.where(rng.random(n) < 0.5, _lib.PROTO_TCP, _lib.PROTO_UDP)
    tag = rng.permutation(n).astype(np.int64)
    note = np.zeros(n, RX_META_DTYPE)
    note[tag] = rxm
    rx_meta = trk_meta(n, 0)  # by tag
    out_cap = 2 * n
    ds = DeliverStage(plan, hosts, 8, n, 2 * n)
    ds.associate(assoc)
    ds.note(t(note.view(np.uint8), np.uint8), 0)
    ib = InboundRouter(plan, np.full(hosts, 125_000_000, np.uint64), 512)
    rx = dict(dst_ptr=t(dst_ptr, np.int32), tag=t(tag, np.int64), st=z(n, torch.int32), fw=z(n, torch.int64),
              late=z(24 * 1024, torch.uint8), cnt=z(1, torch.int32), hp=z(hosts + 1, torch.int32),
              sock=z(out_cap, torch.int32), ofw=z(out_cap, torch.int64), otag=z(out_cap, torch.int64),
              user=z(out_cap, torch.int32), ost=z(out_cap, torch.int32), meta=t(rx_meta.view(np.uint8), np.uint8))
    rx_base = ib.run(torch.arange(n, dtype=torch.int32, device=dev), rx["dst_ptr"], t(deliver, np.int64),
                     t(rng.integers(40, 1501, size=n).astype(np.int32), np.int32), r0 + W, 0, rx["st"], rx["fw"],
                     rx["late"], rx["cnt"])
    i_flags, i_pending = ib.status()

    trk = Tracker(plan, hosts, n_slots, n, 2 * n)
    trk.note(rx["meta"], 0)

    def deliver_run():
        ds.run(rx["dst_ptr"], rx["tag"], rx["st"], rx["fw"], rx_base, rx["late"], rx["cnt"], rx["hp"], rx["sock"],
               rx["ofw"], rx["otag"], rx["user"], rx["ost"])

    def timed(fn, s=stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        plan.sync()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    def torch_counts(ptr, meta_u8, keep, slot, n_rec):
        """the replaced device path -> (node [hosts, 10], sock [n_slots, 10]) int64"""
        m = meta_u8.view(torch.int32).view(-1, 4)[:n_rec].to(torch.int64) & 0xFFFFFFFF
        cnt = (ptr[1:] - ptr[:-1]).to(torch.int64)
        host = torch.repeat_interleave(torch.arange(hosts, device=dev), cnt, output_size=n_rec)
        data, rt = m[:, 1] > 0, (m[:, 2] & 1) != 0
        col = torch.where(data, torch.where(rt, 7, 4), torch.where(rt, 2, 0))
        node, socks = z(hosts * 10, torch.int64), z(n_slots * 10, torch.int64)
        one = torch.ones_like(col)
        for rec, key in ((node, host), (socks, slot.to(torch.int64))):
            base = key[keep] * 10 + col[keep]
            rec.index_add_(0, base, one[keep])
            rec.index_add_(0, base + 1, m[:, 0][keep])
            both = keep & data
            rec.index_add_(0, key[both] * 10 + col[both] + 2, m[:, 1][both])
        return node.view(hosts, 10), socks.view(n_slots, 10)

    def torch_tx():
        keep = (tx["st"] & _lib.PDS_SND_INTERFACE_SENT) != 0
        slot = tx["meta"].view(torch.int32).view(-1, 4)[:, 3]
        return torch_counts(tx["hp"], tx["meta"], keep, slot, n)

    def torch_rx(n_del):
        meta = rx["meta"].view(n, 16)[rx["otag"][:n_del]].reshape(-1)
        return torch_counts(rx["hp"], meta, rx["sock"][:n_del] != -1, rx["sock"][:n_del], n_del)

    def copies(tensors):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for a in tensors:
            a.cpu()
        return (time.perf_counter() - t0) * 1e3

    def as_matrix(rec):
        return np.stack([rec[f] for f in TRK_COUNTER_FIELDS], axis=1).astype(np.int64)

    samples = {k: [] for k in ("tracker_tx_ms", "tracker_rx_ms", "deliver_ms", "torch_tx_ms", "torch_rx_ms",
                               "copies_tx_ms", "copies_rx_ms")}
    same, outcome = True, {}
    cur = torch.cuda.current_stream(dev)
    for k in range(args.warmup + args.reps):
        trk.heartbeat()
        dl = timed(deliver_run)
        d_flags, n_del, n_miss = ds.status()
        a = timed(lambda: trk.tx(tx["cs"], tx["hp"], tx["meta"], tx["st"], tx_base, tx["late"], tx["cnt"]))
        b = timed(lambda: trk.rx(rx["hp"], rx["sock"], rx["otag"], rx["ost"]))
        t_flags, n_tx, n_rx = trk.status()
        got = trk.heartbeat()
        res = {}
        ta = timed(lambda: res.__setitem__("tx", torch_tx()), cur)
        tb = timed(lambda: res.__setitem__("rx", torch_rx(n_del)), cur)
        ca = copies([tx["st"], tx["meta"]])
        cb = copies([rx["sock"][:n_del], rx["otag"][:n_del], rx["ost"][:n_del]])
        same = same and d_flags == 0 and t_flags == 0 and \
            np.array_equal(as_matrix(got[1]), res["tx"][0].cpu().numpy()) and \
            np.array_equal(as_matrix(got[3]), res["tx"][1].cpu().numpy()) and \
            np.array_equal(as_matrix(got[0]), res["rx"][0].cpu().numpy()) and \
            np.array_equal(as_matrix(got[2]), res["rx"][1].cpu().numpy())
        outcome = {"delivered": n_del, "no_socket": n_miss, "tx_counted_total": n_tx, "rx_counted_total": n_rx,
                   "rx_counted_per_call": int(as_matrix(got[0])[:, [0, 2, 4, 7]].sum()),
                   "tx_counted_per_call": int(as_matrix(got[1])[:, [0, 2, 4, 7]].sum())}
        if k >= args.warmup:
            for name, v in zip(samples, (a, b, dl, ta, tb, ca, cb)):
                samples[name].append(v)
    med = {f: statistics.median(v) for f, v in samples.items()}
    for obj in (trk, ds, ib, ob):
        obj.close()
    plan.close()
    out = {"what": "srt_tracker_tx and srt_tracker_rx at the C5 size, device ms per call (HIP events on the plan's stream "
                   "around one call on a warmed instance); beside them srt_deliver_run on the same window (HIP events), "
                   "the same counts by torch index_add_ on the device (HIP events on torch's stream) and the copies to the "
                   "host a per-round host classification needs (wall ms, device synchronised around them)",
           "measured_on": "MI355X", "packets_per_window": n, "hosts": hosts, "sockets_per_host": S,
           "socket_slots": n_slots, "note_cap": n, "log_cap": 2 * n, "out_cap": out_cap, "warmup": args.warmup,
           "reps": args.reps, "outbound": {"flags": o_flags, "pending": o_pending},
           "inbound": {"flags": i_flags, "pending": i_pending}, "outcome": outcome,
           "outputs_equal_every_sample": bool(same), "median_ms": med,
           "rx_over_deliver": med["tracker_rx_ms"] / med["deliver_ms"],
           "replaced_tx_over_tracker_tx": (med["torch_tx_ms"] + med["copies_tx_ms"]) / med["tracker_tx_ms"],
           "replaced_rx_over_tracker_rx": (med["torch_rx_ms"] + med["copies_rx_ms"]) / med["tracker_rx_ms"],
           "samples": samples}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "samples"}))
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
