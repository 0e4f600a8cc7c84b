#!/usr/bin/env python3
"""Times srt_udprecv_run at the C5 size -- 1M delivered packets a window over 10k
hosts and 40k socket slots -- next to the srt_inbound_run and srt_deliver_run
calls that produce its input, with HIP events on the plan's stream around each
call of a warmed chain (every repetition is the next 20 ms window: the arrival
times and the flight tags move on, on the device).  Two cases:

  drained   large buffers; every socket has one blocking read at the window's
            start (it returns with the first datagram) and plain reads at the
            window's end that take the rest, so nothing is buffered across calls;
  carried   no reads and 3000-byte buffers (a ring of 32 holds what such a buffer
            can: payloads are at least 100 bytes): the first window fills the
            buffers, every later one -- all the timed ones -- finds them full,
            drops its packets and leaves the rings as they are.

Beside each, the host-only instance on the same inputs (one window's delivery
list copied back once, outside the timed regions; wall clock around its run).
The device's statuses are compared with the host-only form's on that window.

Writes the raw samples to profiles/udprecv_c5.json and prints a summary line.
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

W = 20_000_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--packets", type=int, default=1_000_000)
    ap.add_argument("--hosts", type=int, default=10_000)
    ap.add_argument("--slots-per-host", type=int, default=4)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--no-refs", action="store_true", help="the device chain alone (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "udprecv_c5.json"))
    args = ap.parse_args()
    if args.reps < 20 and not args.no_refs:
        ap.error("--reps must be at least 20 (the median of fewer samples is not reported)")

    import torch

    from shadow_amd import NetworkGraph, UdpReceive, _lib, synth
    from shadow_amd.plan import (ASSOC_DTYPE, RX_META_DTYPE, UDP_META_DTYPE, UDP_OP_DTYPE, UDP_READ_DTYPE, DeliverStage,
                                 InboundRouter, RoutingPlan)

    _lib.require_device()
    hosts, n, sph, seed = args.hosts, args.packets, args.slots_per_host, 5
    n_sock = hosts * sph
    src, dst, lat, loss = synth.complete_graph(16, seed)
    plan = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32),
                       device=0).run()
    rng = np.random.default_rng(seed)
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
    stream = torch.cuda.ExternalStream(plan.stream_ptr(), device=dev)

    # ---- one window's arrivals, grouped by destination host in time order, on a 1 us grid
    h = np.sort(rng.integers(0, hosts, size=n))
    dst_ptr = np.searchsorted(h, np.arange(hosts + 1)).astype(np.uint32)
    when = 1000 * rng.integers(0, W // 1000, size=n)
    deliver = when[np.lexsort((when, h))].astype(np.uint64)
    size = rng.integers(128, 1429, size=n).astype(np.uint32)  # payloads of 100 to 1400 bytes
    slot = (h * sph + rng.integers(0, sph, size=n)).astype(np.uint32)
    rxm = np.zeros(n, RX_META_DTYPE)
    rxm["protocol"], rxm["local_port_be"] = _lib.PROTO_UDP, 0x1000 + slot % sph
    rxm["peer_ip_be"], rxm["peer_port_be"] = rng.integers(1, 1 << 32, size=n), rng.integers(1, 1 << 16, size=n)
    um = np.zeros(n, UDP_META_DTYPE)
    um["src_ip_be"], um["src_port_be"], um["payload_size"] = rxm["peer_ip_be"], rxm["peer_port_be"], size - 28
    assoc = np.zeros(n_sock, ASSOC_DTYPE)
    assoc["host"], assoc["socket"] = np.arange(n_sock) // sph, np.arange(n_sock)
    assoc["protocol"], assoc["local_port_be"] = _lib.PROTO_UDP, 0x1000 + np.arange(n_sock) % sph
    socket_ptr = (np.arange(hosts + 1) * sph).astype(np.uint32)
    late_cap, u_late_cap = n // 4, n_sock
    out_cap = n + late_cap

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        plan.sync()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    def reads_for(case):
        if case == "carried":
            return None, None, 0
        # per slot: a blocking read at the window's start, then plain reads at its end for everything else
        most = int(np.bincount(slot, minlength=n_sock).max())
        r = np.zeros((n_sock, most + 1), UDP_READ_DTYPE)
        r["slot"] = np.arange(n_sock)[:, None]
        r["len"] = 2048
        r["time_ns"][:, 1:] = W - 1
        r["flags"][:, 0] = _lib.UDP_WAIT
        r = r.reshape(hosts, sph, most + 1).transpose(0, 2, 1).reshape(-1)  # a host's reads in time order
        return r, (np.arange(hosts + 1) * sph * (most + 1)).astype(np.uint32), len(r)

    runs, same = {}, True
    for case, limit, ring_cap in (("drained", 1 << 20, 8), ("carried", 3000, 32)):
        ib = InboundRouter(plan, np.full(hosts, 1_250_000_000, np.uint64), 512)
        ds = DeliverStage(plan, hosts, 2 * n_sock, 2 * n, late_cap + n)
        ur = UdpReceive(plan, socket_ptr, ring_cap, 2 * n, u_late_cap)
        ds.associate(assoc)
        ops = np.zeros(n_sock, UDP_OP_DTYPE)
        ops["op"], ops["slot"], ops["value"] = _lib.UDPRECV_OPEN, np.arange(n_sock), limit
        ur.config(ops)
        reads, rp, n_reads = reads_for(case)
        d = dict(order=t(np.arange(n, dtype=np.uint32), np.int32), dst=t(dst_ptr, np.int32), deliver=t(deliver, np.int64),
                 size=t(size, np.int32), tag=torch.arange(n, dtype=torch.int64, device=dev),
                 rxm=t(rxm.view(np.uint8), np.uint8), um=t(um.view(np.uint8), np.uint8),
                 status=torch.zeros(n, dtype=torch.int32, device=dev), fwd=torch.zeros(n, dtype=torch.int64, device=dev),
                 late=torch.zeros(late_cap * 24, dtype=torch.uint8, device=dev),
                 cnt=torch.zeros(1, dtype=torch.int32, device=dev),
                 o_hp=torch.zeros(hosts + 1, dtype=torch.int32, device=dev),
                 o_sock=torch.zeros(out_cap, dtype=torch.int32, device=dev),
                 o_fw=torch.zeros(out_cap, dtype=torch.int64, device=dev),
                 o_tag=torch.zeros(out_cap, dtype=torch.int64, device=dev),
                 o_user=torch.zeros(out_cap, dtype=torch.int32, device=dev),
                 o_st=torch.zeros(out_cap, dtype=torch.int32, device=dev),
                 rx=torch.zeros(out_cap, dtype=torch.int32, device=dev),
                 res=torch.zeros(56 * max(n_reads, 1), dtype=torch.uint8, device=dev)[:56 * n_reads],
                 u_late=torch.zeros(64 * u_late_cap, dtype=torch.uint8, device=dev),
                 u_cnt=torch.zeros(1, dtype=torch.int32, device=dev),
                 first=torch.zeros(n_sock, dtype=torch.int64, device=dev),
                 rp=t(rp, np.int32) if n_reads else None,
                 reads=t(reads.view(np.uint8), np.uint8) if n_reads else None)
        samples = {"inbound_ms": [], "deliver_ms": [], "udprecv_ms": [], "host_only_ms": []}
        kept = None
        for k in range(args.warmup + args.reps):
            until, box = (k + 1) * W, {}
            ds.note(d["rxm"], k * n)
            ur.note(d["um"], k * n)
            plan.sync()
            ms_i = timed(lambda: box.__setitem__("base", ib.run(d["order"], d["dst"], d["deliver"], d["size"], until, 0,
                                                                d["status"], d["fwd"], d["late"], d["cnt"])))
            ms_d = timed(lambda: ds.run(d["dst"], d["tag"], d["status"], d["fwd"], box["base"], d["late"], d["cnt"],
                                        d["o_hp"], d["o_sock"], d["o_fw"], d["o_tag"], d["o_user"], d["o_st"]))
            ms_u = timed(lambda: ur.run(d["o_hp"], d["o_sock"], d["o_fw"], d["o_tag"], d["o_st"], d["rp"], d["reads"],
                                        until, d["rx"], d["res"], d["u_late"], d["u_cnt"], d["first"]))
            if k >= args.warmup:
                samples["inbound_ms"].append(ms_i)
                samples["deliver_ms"].append(ms_d)
                samples["udprecv_ms"].append(ms_u)
            if k == 0 and not args.no_refs:  # the first window, for the host-only form below
                kept = {f: d[f].cpu().numpy() for f in ("o_hp", "o_sock", "o_fw", "o_tag", "o_st", "rx")}
                kept["res"] = d["res"].cpu().numpy().copy()
            # the next window: the same arrivals 20 ms later under the next tags
            d["deliver"] += W
            d["tag"] += n
            if n_reads:
                d["reads"].view(torch.int64).view(-1, 3)[:, 0] += W
        flags = (ib.status(check=False)[0], ds.status(check=False)[0])
        u_flags, n_proc, n_buf, n_drop = ur.status(check=False)
        delivered = int(d["o_hp"][-1])
        for x in (ur, ds, ib):
            x.close()
        host = {}
        if not args.no_refs:
            for _ in range(args.host_reps):
                hu = UdpReceive(None, socket_ptr, ring_cap, 2 * n, u_late_cap)
                hu.config(ops)
                hu.note(um.view(np.uint8), 0)
                h_rx, h_res = np.zeros(out_cap, np.int32), np.zeros(56 * max(n_reads, 1), np.uint8)[:56 * n_reads]
                h_late, h_cnt = np.zeros(64 * u_late_cap, np.uint8), np.zeros(1, np.int32)
                t0 = time.perf_counter()
                hu.run(kept["o_hp"], kept["o_sock"], kept["o_fw"], kept["o_tag"], kept["o_st"], rp if n_reads else None,
                       reads.view(np.uint8) if n_reads else None, W, h_rx, h_res, h_late, h_cnt,
                       np.zeros(n_sock, np.int64))
                samples["host_only_ms"].append(1e3 * (time.perf_counter() - t0))
                host = dict(zip(("flags", "processed", "buffered", "dropped"), hu.status(check=False)))
                hu.close()
            lim = int(kept["o_hp"][-1])
            same = same and np.array_equal(h_rx[:lim], kept["rx"][:lim]) and h_res.tobytes() == kept["res"].tobytes()
        med = {f: statistics.median(v) for f, v in samples.items() if v}
        runs[case] = {"recv_buf_size": limit, "ring_cap": ring_cap, "reads_per_call": n_reads,
                      "delivered_last_call": delivered, "inbound_deliver_flags": flags, "udprecv_flags": u_flags,
                      "processed": n_proc, "buffered": n_buf, "dropped": n_drop, "host_only_first_window": host,
                      "median_ms": med, "udprecv_over_inbound": med["udprecv_ms"] / med["inbound_ms"],
                      "samples": samples}
        if not args.no_refs:
            runs[case]["host_only_over_device"] = med["host_only_ms"] / med["udprecv_ms"]
    plan.close()
    out = {"what": "srt_udprecv_run at the C5 size, device ms per call (HIP events on the plan's stream around one call "
                   "of a warmed inbound -> deliver -> udprecv chain, every repetition the next window), beside the "
                   "srt_inbound_run and srt_deliver_run calls of the same window and the host-only instance on the "
                   "first window's list (wall clock)",
           "measured_on": "MI355X", "packets": n, "hosts": hosts, "slots": n_sock,
           "window_bytes": UdpReceive.window_bytes(), "warmup": args.warmup, "reps": args.reps,
           "host_reps": args.host_reps, "outputs_equal": bool(same) and not args.no_refs, "runs": runs}
    if not args.no_refs:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    for r in runs.values():
        r.pop("samples")
    print(json.dumps(out))
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
