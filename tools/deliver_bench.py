#!/usr/bin/env python3
"""Times srt_deliver_run at the C5 size -- 1M packets a window over 10k
destination hosts, four sockets a host -- with HIP events on the plan's stream
around one call on a warmed instance, in two cases with tools/inbound_bench.py's
bandwidths: uncongested (125 MB/s a host: every packet is forwarded in its own
window, no late list) and congested (125 kB/s a host: the timed call is the
second window's, whose late list holds the first window's packets that left the
router in it).  Beside it, in the same process and on the same inputs:

  * the path it replaces, in torch and numpy: the mask of the forwarded packets,
    the merge with the late list, the stable grouping by host (two stable
    sorts), the gather of tags and metas from the caller's own tensors, and a
    host-side lookup (srt_deliver_lookup, the library's own, over a copy of the
    hosts and metas to the host and of the sockets back).  Wall time with the
    device synchronised before and after, since the host works in it.  Both
    paths' outputs are compared byte for byte every sample, outside the timed
    regions;
  * srt_inbound_run, the call the stage follows, as the yardstick: HIP events
    around the call whose results are delivered, on a fresh srt_inbound a
    sample (its state is consumed by a call), primed as inbound_bench.py does.

Writes the raw samples to profiles/deliver_c5.json and prints a summary line.
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
    ap.add_argument("--sockets", type=int, default=4, help="associations a host: half wildcards, half specific")
    ap.add_argument("--queue-cap", type=int, default=512)
    ap.add_argument("--only", choices=("uncongested", "congested"), help="one case (for a kernel trace of its own)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deliver_c5.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20 (the median of fewer samples is not reported)")

    import torch

    from shadow_amd import NetworkGraph, _lib, synth
    from shadow_amd.plan import ASSOC_DTYPE, RX_META_DTYPE, DeliverStage, InboundRouter, RoutingPlan

    _lib.require_device()
    hosts, n, seed, W = args.hosts, args.packets, 5, 5 * synth.MS
    src, dst, lat, loss = synth.complete_graph(16, seed)
    plan = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32),
                       device=0).run()
    rng = np.random.default_rng(seed)
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
    z = lambda k, dt: torch.zeros(k, dtype=dt, device=dev)  # noqa: E731
    stream = torch.cuda.ExternalStream(plan.stream_ptr(), device=dev)
    r0 = 1_000_000_000

    # ---- the associations: per host `sockets` keys on two ports, wildcards and specific peers
    ports, peers = np.array([0x5000, 0xBB01], np.uint16), np.array([0x0100000A, 0x0200000A, 0x0300000A], np.uint32)
    assoc = np.zeros(hosts * args.sockets, ASSOC_DTYPE)
    assoc["host"] = np.repeat(np.arange(hosts), args.sockets)
    k = np.tile(np.arange(args.sockets), hosts)
    assoc["protocol"] = np.where(k % 2 == 0, _lib.PROTO_TCP, _lib.PROTO_UDP)
    assoc["local_port_be"] = ports[(k // 2) % 2]
    spec = k >= args.sockets // 2
    assoc["peer_ip_be"] = np.where(spec, peers[k % 3] + (k // 4 << 24), 0)
    assoc["peer_port_be"] = np.where(spec, 0x901F, 0)
    assoc["socket"] = k
    assert len(set(zip(*(assoc[f].tolist() for f in ("host", "protocol", "peer_ip_be", "local_port_be",
                                                       "peer_port_be"))))) == len(assoc)

    def window(w):
        """one window in final order: grouped by host, each host's by deliver time; tags of one push"""
        d = np.sort(rng.integers(0, hosts, size=n))
        dst_ptr = np.searchsorted(d, np.arange(hosts + 1)).astype(np.int32)
        deliver = r0 + w * W + rng.integers(0, W, size=n)
        deliver = deliver[np.lexsort((deliver, d))].astype(np.int64)
        size = rng.integers(40, 1501, size=n).astype(np.int32)
        meta = np.zeros(n, RX_META_DTYPE)
        meta["peer_ip_be"] = peers[rng.integers(0, 3, size=n)]
        meta["peer_port_be"] = np.where(rng.random(n) < 0.8, 0x901F, 0x3500)
        meta["local_port_be"] = np.where(rng.random(n) < 0.9, ports[rng.integers(0, 2, size=n)], 0x1111)
        meta["protocol"] = np.where(rng.random(n) < 0.5, _lib.PROTO_TCP, _lib.PROTO_UDP)
        meta["user"] = rng.integers(0, hosts, size=n)
        tag = (w * n + rng.permutation(n)).astype(np.int64)
        note = np.zeros(n, RX_META_DTYPE)
        note[tag - w * n] = meta
        return dict(dst_ptr=t(dst_ptr, np.int32), deliver=t(deliver, np.int64), size=t(size, np.int32),
                    tag=t(tag, np.int64), note=t(note.view(np.uint8), np.uint8))

    wins = [window(0), window(1)]
    t_order = torch.arange(n, dtype=torch.int32, device=dev)
    t_zero = z(hosts + 1, torch.int32)
    late_cap = 2 * n
    out_cap = 2 * n
    ds = DeliverStage(plan, hosts, 8, 2 * n, 4 * n)
    ds.associate(assoc)
    for w, win in enumerate(wins):
        ds.note(win["note"], w * n)
    M = torch.cat([wins[0]["note"], wins[1]["note"]]).view(2 * n, 16)  # the caller's metas by tag
    M_user = M.view(torch.int32).view(2 * n, 4)[:, 3].contiguous()
    T_seq = torch.cat([wins[0]["tag"], wins[1]["tag"]])                # the caller's tags by seq - first base
    st, fw = [z(n, torch.int32) for _ in wins], [z(n, torch.int64) for _ in wins]
    late, cnt = z(24 * late_cap, torch.uint8), z(1, torch.int32)
    o = dict(hp=z(hosts + 1, torch.int32), sock=z(out_cap, torch.int32), fw=z(out_cap, torch.int64),
             tag=z(out_cap, torch.int64), user=z(out_cap, torch.int32), st=z(out_cap, torch.int32))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        r = fn()
        e1.record(stream)
        plan.sync()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1), r

    def deliver(w, base, with_late):
        ds.run(wins[w]["dst_ptr"], wins[w]["tag"], st[w], fw[w], base, late if with_late else None,
               cnt if with_late else None, o["hp"], o["sock"], o["fw"], o["tag"], o["user"], o["st"])

    def torch_path(w, base, base0, with_late):
        """the replaced path -> (host_ptr, socket, forward, tag, user, status)"""
        win = wins[w]
        mask = (st[w] & _lib.PDS_RELAY_FORWARDED) != 0
        idx = torch.nonzero(mask).squeeze(1)
        b_host = torch.searchsorted(win["dst_ptr"][1:].contiguous(), idx.to(torch.int32), right=True)
        host, key = b_host, idx + (1 << 40)
        tag, fwd, status = win["tag"][idx], fw[w][idx], st[w][idx]
        if with_late:
            c = min(int(cnt.item()), late_cap)
            rec = late[:24 * c].view(c, 24)
            l_seq, l_fw = rec[:, 0:8].contiguous().view(torch.int64).squeeze(1), rec[:, 8:16].contiguous().view(
                torch.int64).squeeze(1)
            l_st, l_host = rec[:, 16:20].contiguous().view(torch.int32).squeeze(1), rec[:, 20:24].contiguous().view(
                torch.int32).squeeze(1)
            lm = (l_st & _lib.PDS_RELAY_FORWARDED) != 0
            host = torch.cat([l_host[lm].long(), host])
            key = torch.cat([l_seq[lm], key])
            tag = torch.cat([T_seq[l_seq[lm] - base0], tag])
            fwd, status = torch.cat([l_fw[lm], fwd]), torch.cat([l_st[lm], status])
            p = torch.sort(key, stable=True).indices
            p = p[torch.sort(host[p], stable=True).indices]
            host, tag, fwd, status = host[p], tag[p], fwd[p], status[p]
        host_ptr = torch.searchsorted(host, torch.arange(hosts + 1, device=dev)).to(torch.int32)
        meta = M[tag]
        sock = ds.lookup(host.to(torch.int32).cpu().numpy().view(np.uint32), meta.cpu().numpy().view(RX_META_DTYPE)
                         .reshape(-1))
        sock = torch.from_numpy(sock.view(np.int32)).to(dev)
        status = status | torch.where(sock == -1, _lib.PDS_RCV_INTERFACE_RECEIVED | _lib.PDS_RCV_INTERFACE_DROPPED,
                                      _lib.PDS_RCV_INTERFACE_RECEIVED).to(torch.int32)
        return host_ptr, sock, fwd, tag, M_user[tag], status

    def case(bw_bytes, congested):
        bw = np.full(hosts, bw_bytes, np.uint64)
        w = 1 if congested else 0
        samples = {"inbound_ms": [], "deliver_ms": [], "torch_path_ms": []}
        same, last = True, None
        for k in range(args.warmup + args.reps):
            ib = InboundRouter(plan, bw, args.queue_cap)
            # an empty batch of the same size (no group holds a packet): sizes the record buffer
            base0 = ib.run(t_order, t_zero, wins[0]["deliver"], wins[0]["size"], 0, 0, st[0], fw[0], late, cnt) + n
            ib.status()
            if congested:  # the first window leaves most of its packets queued, and the stage logs them
                b = ib.run(t_order, wins[0]["dst_ptr"], wins[0]["deliver"], wins[0]["size"], r0 + W, 0, st[0], fw[0],
                           late, cnt)
                assert b == base0
                if k == 0:  # the instance keeps the log: the later samples' first windows write the same records
                    deliver(0, b, True)
                ib.status()
            until = r0 + (w + 1) * W + (300 * synth.MS if congested else 0)
            in_ms, base = timed(lambda: ib.run(t_order, wins[w]["dst_ptr"], wins[w]["deliver"], wins[w]["size"], until,
                                               0, st[w], fw[w], late, cnt))
            i_flags, pending = ib.status()
            dl_ms, _ = timed(lambda: deliver(w, base, congested))
            d_flags, n_del, n_miss = ds.status()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            g = torch_path(w, base, base0, congested)
            torch.cuda.synchronize(dev)
            tp_ms = (time.perf_counter() - t0) * 1e3
            same = same and i_flags == 0 and d_flags == 0 and g[1].numel() == n_del and torch.equal(g[0], o["hp"]) \
                and all(torch.equal(a, o[f][:n_del]) for a, f in zip(g[1:], ("sock", "fw", "tag", "user", "st")))
            if k >= args.warmup:
                samples["inbound_ms"].append(in_ms)
                samples["deliver_ms"].append(dl_ms)
                samples["torch_path_ms"].append(tp_ms)
            last = {"delivered": n_del, "no_socket": n_miss, "late_records": int(cnt.item()), "pending": pending,
                    "late_forwarded": n_del - int(((st[w] & _lib.PDS_RELAY_FORWARDED) != 0).sum().item())}
            ib.close()
        med = {f: statistics.median(v) for f, v in samples.items()}
        ratio = [a / b for a, b in zip(samples["torch_path_ms"], samples["deliver_ms"])]
        frac = [a / b for a, b in zip(samples["deliver_ms"], samples["inbound_ms"])]
        return {"bandwidth_down_bytes_per_s": bw_bytes, "outcome": last, "outputs_equal_every_sample": bool(same),
                "median_ms": med, "samples": samples,
                "torch_path_over_deliver": {"median": statistics.median(ratio), "min": min(ratio), "max": max(ratio)},
                "deliver_over_inbound": {"median": statistics.median(frac), "min": min(frac), "max": max(frac)}}

    skipped = {"outputs_equal_every_sample": True, "skipped": True}
    fast = case(125_000_000, False) if args.only != "congested" else skipped
    slow = case(125_000, True) if args.only != "uncongested" else skipped
    stats = ds.table_stats()
    ds.close()
    plan.close()
    out = {"what": "srt_deliver_run at the C5 size, device ms per call (HIP events on the plan's stream around one call "
                   "on a warmed instance); beside it srt_inbound_run (HIP events, the call whose results are delivered) "
                   "and the replaced path in torch and numpy (mask, merge with the late list, two stable sorts, gathers, "
                   "copies to the host, srt_deliver_lookup there, copy back; wall ms, device synchronised around it)",
           "measured_on": "MI355X", "packets_per_window": n, "hosts": hosts, "sockets_per_host": args.sockets,
           "table": {"associations": stats[0], "slots": stats[1], "bytes": 16 * stats[1], "max_probe": stats[2]},
           "note_cap": 2 * n, "log_cap": 4 * n, "out_cap": out_cap, "late_cap": late_cap, "queue_cap": args.queue_cap,
           "warmup": args.warmup, "reps": args.reps, "uncongested": fast, "congested": slow}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) or "samples" not in v else
                          {kk: vv for kk, vv in v.items() if kk != "samples"}) for k, v in out.items()}))
    sys.exit(0 if fast["outputs_equal_every_sample"] and slow["outputs_equal_every_sample"] else 1)


if __name__ == "__main__":
    main()
