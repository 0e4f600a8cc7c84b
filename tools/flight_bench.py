#!/usr/bin/env python3
"""Times the in-flight store (srt_flight_push + srt_flight_pop) in steady state
at the C5 size -- 1M packets a round over 10k hosts, 85% of them sent, every
round's deliver times spread evenly over the four windows that follow it, so
that a window takes about a quarter of each of the last four rounds -- with
HIP events on the plan's stream, and beside it, in the same process and on the
same rounds, the joining INTEGRATION.md prescribed before the store existed:
the caller keeps the sent packets in torch tensors (a mask and a gather of the
round), takes the window's set out with a mask and a gather, brings it into
source-host order (two stable sorts: the set mixes rounds) and orders it with
a second srt_packet_events call over a scratch event_base, then gathers the
window's arrays by that order.  Every round both paths' windows are compared
(dst_ptr, deliver, source host, event id, tag) outside the timed regions.
Writes the raw samples to profiles/flight_c5.json and prints a summary line.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes / s, the figure DESIGN.md's roofline table uses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=6, help="rounds before the timed ones (at least 4: the store fills)")
    ap.add_argument("--packets", type=int, default=1_000_000)
    ap.add_argument("--hosts", type=int, default=10_000)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flight_c5.json"))
    args = ap.parse_args()
    if args.reps < 20 or args.warmup < args.windows:
        ap.error("--reps must be at least 20 and --warmup at least --windows")

    import torch

    from shadow_amd import NetworkGraph, _lib, synth
    from shadow_amd.plan import FlightStore, RoutingPlan

    _lib.require_device()
    hosts, n_pkts, seed, W = args.hosts, args.packets, 5, 5 * synth.MS
    src, dst, lat, loss = synth.complete_graph(16, seed)
    plan = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32),
                       device=0).run()
    rng = np.random.default_rng(seed)
    src_host = np.sort(rng.integers(0, hosts, size=n_pkts))
    host_ptr = np.searchsorted(src_host, np.arange(hosts + 1)).astype(np.int32)
    sent = rng.random(n_pkts) < 0.85
    flags = np.where(sent, _lib.PDS_INET_SENT, _lib.PDS_INET_DROPPED).astype(np.int32)
    rel = rng.integers(0, args.windows * W, size=n_pkts).astype(np.int64)  # deliver time past the round's end
    rank = np.cumsum(sent) - 1
    first = np.concatenate([[0], np.cumsum(sent)])[host_ptr[:-1]]
    eid0 = np.where(sent, rank - np.repeat(first, np.diff(host_ptr)), -1).astype(np.int64)  # per host, send order
    per_round_ids = 1 << 20
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    t_hp, t_f, t_rel, t_eid0, t_sent = t(host_ptr), t(flags), t(rel), t(eid0), t(sent)
    t_src = t(src_host.astype(np.int32))
    t_dst = t(rng.integers(0, hosts, size=n_pkts).astype(np.int32))
    t_size = t(rng.integers(40, 1501, size=n_pkts).astype(np.int32))
    pool_cap = out_cap = args.windows * n_pkts
    w = dict(order=z(out_cap, torch.int32), dst_ptr=z(hosts + 1, torch.int32), deliver=z(out_cap, torch.int64),
             size=z(out_cap, torch.int32), src=z(out_cap, torch.int32), eid=z(out_cap, torch.int64),
             tag=z(out_cap, torch.int64))
    stream = torch.cuda.ExternalStream(plan.stream_ptr(), device=dev)
    fs = FlightStore(plan, hosts, pool_cap)

    def timed(fn, on):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(on)
        r = fn()
        e1.record(on)
        plan.sync()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1), r

    # ---- the prescribed glue: the caller's own store, as torch tensors
    store = {k: z(0, dt) for k, dt in (("deliver", torch.int64), ("src", torch.int32), ("eid", torch.int64),
                                       ("dst", torch.int32), ("size", torch.int32), ("tag", torch.int64))}
    e_base, e_id = z(hosts, torch.int64), z(out_cap, torch.int64)
    e_order, e_ptr = z(out_cap, torch.int32), z(hosts + 1, torch.int32)

    def glue_keep(t_d, t_e, tag0):
        """the round's sent packets join the caller's store"""
        m = t_f == _lib.PDS_INET_SENT
        new = dict(deliver=t_d[m], src=t_src[m], eid=t_e[m], dst=t_dst[m], size=t_size[m],
                   tag=torch.arange(tag0, tag0 + n_pkts, device=dev)[m])
        for k in store:
            store[k] = torch.cat([store[k], new[k]])

    def glue_window(until):
        """the window's set out of the store, in source-host send order, through srt_packet_events"""
        due = store["deliver"] < until
        g = {k: v[due] for k, v in store.items()}
        for k in store:
            store[k] = store[k][~due]
        o = torch.sort(g["eid"], stable=True).indices
        o = o[torch.sort(g["src"][o], stable=True).indices]
        g = {k: v[o] for k, v in g.items()}
        n = g["src"].numel()
        hp = torch.searchsorted(g["src"], torch.arange(hosts + 1, device=dev, dtype=torch.int32)).to(torch.int32)
        f = torch.full((n,), _lib.PDS_INET_SENT, dtype=torch.int32, device=dev)
        e_base.zero_()
        plan.packet_events(hp, f, g["deliver"], g["dst"], hosts, e_base, e_id[:n], e_order[:n], e_ptr, check=False)
        idx = e_order[:n].long()
        return {k: v[idx] for k, v in g.items()}, e_ptr

    samples = {"push_ms": [], "pop_ms": [], "glue_keep_ms": [], "glue_window_ms": []}
    counts, same = [], True
    cur = torch.cuda.current_stream(dev)
    for k in range(args.warmup + args.reps):
        end = 1_000_000_000 + (k + 1) * W
        t_d = t_rel + end
        t_e = torch.where(t_sent, t_eid0 + k * per_round_ids, torch.full_like(t_eid0, -1))
        torch.cuda.synchronize(dev)
        until = end + W
        push_ms, tag0 = timed(lambda: fs.push(t_hp, t_f, t_d, t_dst, t_e, t_size), stream)
        _, _, stored_before, _ = fs.status()
        pop_ms, _ = timed(lambda: fs.pop(until, w["order"], w["dst_ptr"], w["deliver"], w["size"], w["src"], w["eid"],
                                         w["tag"]), stream)
        fl, n_popped, stored_after, lost = fs.status()
        keep_ms, _ = timed(lambda: glue_keep(t_d, t_e, tag0), cur)
        win_ms, (g, g_ptr) = timed(lambda: glue_window(until), cur)
        plan.packet_events_status()
        same = same and fl == 0 and lost == 0 and g["src"].numel() == n_popped and torch.equal(g_ptr, w["dst_ptr"]) \
            and all(torch.equal(g[a], w[a][:n_popped]) for a in ("deliver", "src", "eid", "tag", "size"))
        if k >= args.warmup:
            for name, v in (("push_ms", push_ms), ("pop_ms", pop_ms), ("glue_keep_ms", keep_ms),
                            ("glue_window_ms", win_ms)):
                samples[name].append(v)
            counts.append((stored_before, n_popped, stored_after))
    fs.close()
    plan.close()

    med = {k: statistics.median(v) for k, v in samples.items()}
    stored_before, due, surv = (statistics.median(c[i] for c in counts) for i in range(3))
    n_sent = int(sent.sum())
    # what the stage has to move (bytes): the push reads every flag and a sent packet's 24 bytes of
    # fields and writes its 36-byte record; the pop reads the stored deliver times in the count and
    # again in the move (8 + 8); a due packet's destination is read in both (4 + 4), its slot written
    # and read (4 + 4), the rest of its record read (24), the record staged and read back (32 + 32) and
    # the window's arrays written (36): moved twice; a survivor's other fields are read and its record
    # written (28 + 36): moved once
    push_bytes = 4 * n_pkts + (24 + 36) * n_sent
    pop_bytes = 16 * stored_before + 140 * due + 64 * surv
    out = {
        "what": "srt_flight_push + srt_flight_pop in steady state, device ms per call (HIP events on the plan's "
                "stream); beside them the torch joining the documentation prescribed before (keep: mask and gather "
                "of the round into the caller's tensors; window: mask and gather of the due set, two stable sorts "
                "into source-host order, srt_packet_events over it, gather by its order; events on torch's stream, "
                "the srt_packet_events call inside them)",
        "measured_on": "MI355X",
        "packets_per_round": n_pkts, "sent_per_round": n_sent, "hosts": hosts, "windows": args.windows,
        "pool_cap": pool_cap, "out_cap": out_cap, "warmup_rounds": args.warmup, "reps": args.reps,
        "stored_before_pop": stored_before, "due_per_window": due, "survivors": surv,
        "windows_equal_every_round": bool(same),
        "samples": samples, "median_ms": med,
        "flight_ms": med["push_ms"] + med["pop_ms"], "glue_ms": med["glue_keep_ms"] + med["glue_window_ms"],
        "algorithmic_bytes": {"push": push_bytes, "pop": pop_bytes},
        "fraction_of_hbm_8TBps": {"push": push_bytes / (med["push_ms"] * 1e-3) / HBM_PEAK,
                                  "pop": pop_bytes / (med["pop_ms"] * 1e-3) / HBM_PEAK},
    }
    out["glue_over_flight"] = out["glue_ms"] / out["flight_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "samples"}))
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
