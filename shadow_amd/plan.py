"""Device-resident routing plan (srt_plan_* in include/srt.h) and the batched
packet stage (srt_packet_batch).

Used by bench.py (inputs resident in HBM before the timed region), the
multi-GPU driver and the per-round packet decision.  Device buffers for the
packet stage are torch tensors on the plan's device: torch is only the HBM
allocator here, every kernel is in libsrt.so.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import _lib
from .graph import NetworkGraph, PathTable


class RoutingPlan:
    def __init__(self, graph: NetworkGraph, nodes, algo: int = _lib.SRT_ALGO_AUTO, device: int = -1):
        L = _lib.lib()
        _lib.require_device()
        self.graph = graph
        self.nodes = np.ascontiguousarray(nodes, np.uint32)
        self.n = len(self.nodes)
        self._h = C.c_void_p()
        err = _lib.SrtErr()
        opts = _lib.SrtOpts(algo, device, 0, 0)
        csr = graph.csr()
        _lib.check(L.srt_plan_create(C.byref(csr), self.nodes.ctypes.data_as(C.POINTER(C.c_uint32)), self.n,
                                     C.byref(opts), C.byref(self._h), C.byref(err)), err)

    # ---------------------------------------------------------------- build
    def run(self):
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_plan_run(self._h, C.byref(err)), err)
        return self

    def run_async(self):
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_plan_run_async(self._h, C.byref(err)), err)
        return self

    def sync(self):
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_plan_sync(self._h, C.byref(err)), err)

    def fetch(self, table: bool = True) -> Optional[PathTable]:
        n = self.n
        err = _lib.SrtErr()
        mn = C.c_uint64()
        out = (_lib.SrtPath * max(n * n, 1))() if table else None
        _lib.check(_lib.lib().srt_plan_fetch(self._h, out, C.byref(mn), C.byref(err)), err)
        self.min_latency_ns = mn.value
        if not table:
            return None
        raw = np.frombuffer(out, dtype=np.dtype([("lat", "<u8"), ("loss", "<f4"), ("pad", "<u4")]), count=n * n)
        return PathTable(self.nodes, raw["lat"].reshape(n, n).copy(), raw["loss"].reshape(n, n).copy(), mn.value)

    def describe(self) -> str:
        return _lib.lib().srt_plan_describe(self._h).decode()

    def kernel_stats(self):
        """(dominant-kernel ms summed over its launches, launches, relaxations they
        performed, whole-build device ms) of the last run."""
        a, b, w, c = C.c_double(), C.c_uint64(), C.c_double(), C.c_double()
        _lib.lib().srt_plan_kernel_stats(self._h, C.byref(a), C.byref(b), C.byref(w), C.byref(c))
        return a.value, b.value, w.value, c.value

    def timing(self) -> dict:
        """Phase breakdown of the last run (srt_plan_timing)."""
        t = _lib.SrtTiming()
        _lib.check(_lib.lib().srt_plan_timing(self._h, C.byref(t)), _lib.SrtErr())
        return {k: getattr(t, k) for k, _ in _lib.SrtTiming._fields_}

    def kernel_tiles(self) -> int:
        """C tiles the last run's dominant (FW rest) launches loaded and stored."""
        t = C.c_uint64()
        _lib.lib().srt_plan_kernel_tiles(self._h, C.byref(t))
        return t.value

    def stream_ptr(self) -> int:
        """hipStream_t the plan launches on (for HIP events on that stream)."""
        return _lib.lib().srt_plan_stream(self._h)

    def table_ptrs(self):
        lat, loss, n = C.c_void_p(), C.c_void_p(), C.c_uint32()
        _lib.lib().srt_plan_table(self._h, C.byref(lat), C.byref(loss), C.byref(n))
        return lat.value, loss.value, n.value

    def shard_rows(self, nranks: int, rank: int):
        """srt_plan_shard_rows: this plan builds only table rows
        [rank*n/nranks, (rank+1)*n/nranks), no exchange (LEVEL / SSSP plans)."""
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_plan_shard_rows(self._h, int(nranks), int(rank), C.byref(err)), err)
        return self

    def bind_comm(self, comm):
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_plan_bind_comm(self._h, comm, C.byref(err)), err)

    @property
    def handle(self):
        return self._h

    def close(self):
        for r in list(getattr(self, "_routers", ())):  # InboundRouter / OutboundRelay objects bound to this plan
            r.close()
        if self._h:
            _lib.lib().srt_plan_destroy(self._h)
            self._h = C.c_void_p()
        comm = getattr(self, "_comm", None)
        if comm is not None:  # the plan referenced it: destroy after the plan
            comm.close()
            self._comm = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- packets
    def packet_events(self, host_ptr, flags, deliver, dst_host, n_dst_hosts: int, event_base, event_id, order,
                      dst_ptr, check: bool = True):
        """srt_packet_events (worker.rs:629-639 + event.rs:85-150) on torch CUDA
        tensors of this plan's device: host_ptr int32 [n_hosts+1], flags int32,
        deliver int64, dst_host int32 [n_pkts], event_base int64 [n_hosts]
        (advanced in place); outputs event_id int64 [n_pkts], order int32
        [n_pkts] (first dst_ptr[-1] meaningful), dst_ptr int32 [n_dst_hosts+1]."""
        import torch

        ps = torch.cuda.ExternalStream(self.stream_ptr(), device=flags.device)
        cur = torch.cuda.current_stream(flags.device)
        ps.wait_stream(cur)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_packet_events(
            self._h, host_ptr.data_ptr(), host_ptr.numel() - 1, flags.numel(), flags.data_ptr(), deliver.data_ptr(),
            dst_host.data_ptr(), n_dst_hosts, event_base.data_ptr(), event_id.data_ptr(), order.data_ptr(),
            dst_ptr.data_ptr(), C.byref(err)), err)
        cur.wait_stream(ps)  # torch-side consumers see the outputs (device-side ordering)
        if check:  # the asynchronous call's destination check (synchronises the plan's stream)
            self.packet_events_status()

    def packet_events_status(self):
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_packet_events_status(self._h, C.byref(err)), err)

    def packet_batch(self, pkts, host_ptr, rng, round_end_ns: int, bootstrap_end_ns: int, sim_end_ns: int,
                     flags, deliver, counters=None, stats=None, sync: bool = True):
        """All array arguments are torch CUDA tensors on this plan's device:
        pkts (uint8 view of srt_pkt records), host_ptr int32/uint32 [n_hosts+1],
        rng int64 [n_hosts, 4] (xoshiro256++ state, advanced in place),
        flags int32 [n_pkts], deliver int64 [n_pkts], counters int64 [n*n] or
        None, stats int64 [2] (min-combined; initialise to -1 == UINT64_MAX)."""
        import torch

        n_hosts = host_ptr.numel() - 1
        n_pkts = flags.numel()
        # the plan's stream waits for the producer of the inputs (torch's
        # current stream) on the device: no host round trip per batch
        torch.cuda.ExternalStream(self.stream_ptr(), device=flags.device).wait_stream(
            torch.cuda.current_stream(flags.device))
        r = _lib.SrtRound(round_end_ns, bootstrap_end_ns, sim_end_ns)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_packet_batch(
            self._h, pkts.data_ptr(), host_ptr.data_ptr(), n_hosts, n_pkts, rng.data_ptr(), C.byref(r),
            flags.data_ptr(), deliver.data_ptr(), counters.data_ptr() if counters is not None else None,
            stats.data_ptr() if stats is not None else None, C.byref(err)), err)
        if sync:
            self.sync()

    def packet_batch_ip(self, resolver, pkts, host_ptr, rng, round_end_ns: int, bootstrap_end_ns: int,
                        sim_end_ns: int, flags, deliver, counters=None, stats=None, sync: bool = True):
        """srt_packet_batch_ip: as packet_batch, with pkts a uint8 view of
        srt_pkt_ip records (source / destination IPv4 in network byte order,
        resolved on the device through `resolver`, an IpResolver over this
        plan's table rows).  sync=True also checks srt_packet_status (an
        address without a row raises, as the reference's unwrap panics)."""
        import torch

        n_hosts = host_ptr.numel() - 1
        n_pkts = flags.numel()
        torch.cuda.ExternalStream(self.stream_ptr(), device=flags.device).wait_stream(
            torch.cuda.current_stream(flags.device))
        r = _lib.SrtRound(round_end_ns, bootstrap_end_ns, sim_end_ns)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_packet_batch_ip(
            self._h, resolver.handle, pkts.data_ptr(), host_ptr.data_ptr(), n_hosts, n_pkts, rng.data_ptr(),
            C.byref(r), flags.data_ptr(), deliver.data_ptr(),
            counters.data_ptr() if counters is not None else None,
            stats.data_ptr() if stats is not None else None, C.byref(err)), err)
        if sync:
            self.packet_status()

    def packet_status(self):
        """srt_packet_status: synchronises; raises if a batch met an address without a row."""
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_packet_status(self._h, C.byref(err)), err)


INBOUND_STATE_DTYPE = np.dtype([(k, "<u8") for k in (
    "balance", "last_refill_ns", "interval_end_ns", "drop_next_ns", "current_drop_count", "previous_drop_count",
    "queue_len", "bytes_stored", "task_ns", "tasks_scheduled")] + [(k, "<u4") for k in (
        "mode", "cached", "overflow", "reserved0")])
INBOUND_LATE_DTYPE = np.dtype([("seq", "<u8"), ("forward_ns", "<u8"), ("status", "<u4"), ("dst_host", "<u4")])


_live_routers = None  # device-bound InboundRouter objects, closed before the interpreter finalises


def _close_live_routers():
    for r in list(_live_routers or ()):
        try:
            r.close()
        except Exception:
            pass


def _bind_to_plan(obj, plan):
    """the plan closes `obj` before itself (it runs on the plan's stream); an
    object left open (a caller that raised) is closed while the HIP runtime is
    still up, not by a finaliser during interpreter shutdown"""
    import weakref

    if not hasattr(plan, "_routers"):
        plan._routers = weakref.WeakSet()
    plan._routers.add(obj)
    global _live_routers
    if _live_routers is None:
        import atexit

        _live_routers = weakref.WeakSet()
        atexit.register(_close_live_routers)
    _live_routers.add(obj)


class InboundRouter:
    """srt_inbound: every destination host's CoDel queue and download token
    bucket (router/codel_queue.rs, relay/mod.rs, relay/token_bucket.rs) behind
    the packet events, one call per scheduling window.

    Bound to a RoutingPlan (arrays are torch CUDA tensors of its device, the
    call is asynchronous on its stream; closing the plan closes its routers), or
    host-only with plan=None (arrays are numpy arrays, the same per-host step
    on the CPU)."""

    def __init__(self, plan: Optional[RoutingPlan], bw_down_bytes_per_s, queue_cap: int):
        self.plan = plan
        bw = np.ascontiguousarray(bw_down_bytes_per_s, np.uint64)
        self.n_hosts = len(bw)
        self._h = C.c_void_p()
        if plan is not None:  # the plan closes its routers before itself (they run on its stream)
            import weakref

            if not hasattr(plan, "_routers"):
                plan._routers = weakref.WeakSet()
            plan._routers.add(self)
            # a router left open (a caller that raised) is closed while the HIP
            # runtime is still up, not by a finaliser during interpreter shutdown
            global _live_routers
            if _live_routers is None:
                import atexit

                _live_routers = weakref.WeakSet()
                atexit.register(_close_live_routers)
            _live_routers.add(self)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_inbound_create(plan.handle if plan is not None else None, self.n_hosts,
                                                 bw.ctypes.data_as(C.POINTER(C.c_uint64)), int(queue_cap),
                                                 C.byref(self._h), C.byref(err)), err)

    @staticmethod
    def _ptr(a):
        if a is None:
            return None
        return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data

    def run(self, order, dst_ptr, deliver, total_size, until_ns: int, bootstrap_end_ns: int, status, forward_ns,
            late=None, late_count=None) -> int:
        """srt_inbound_run.  order int32/uint32 (srt_packet_events' output), dst_ptr
        [n_hosts+1], deliver int64/uint64, total_size int32/uint32, outputs
        status int32/uint32 and forward_ns int64/uint64, all [n_pkts]; late: a
        uint8 buffer of 24-byte srt_inbound_late records (INBOUND_LATE_DTYPE)
        with late_count a 1-element int32/uint32.  Returns the batch's sequence
        base.  Device form: enqueue only (status() synchronises)."""
        n_pkts = int(status.numel() if hasattr(status, "numel") else status.size)
        late_cap = 0
        if late is not None:
            late_cap = int(late.numel() * late.element_size() if hasattr(late, "numel") else late.nbytes) // 24
        cur = ps = None
        if self.plan is not None:
            import torch

            ps = torch.cuda.ExternalStream(self.plan.stream_ptr(), device=status.device)
            cur = torch.cuda.current_stream(status.device)
            ps.wait_stream(cur)
        base = C.c_uint64()
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_inbound_run(
            self._h, self._ptr(order), self._ptr(dst_ptr), self._ptr(deliver), self._ptr(total_size), n_pkts,
            int(until_ns), int(bootstrap_end_ns), self._ptr(status), self._ptr(forward_ns), self._ptr(late), late_cap,
            self._ptr(late_count), C.byref(base), C.byref(err)), err)
        if cur is not None:
            cur.wait_stream(ps)  # torch-side consumers see the outputs (device-side ordering)
        return base.value

    def status(self, check: bool = True):
        """srt_inbound_status: synchronises; (flags, packets still pending).
        check=True raises SrtError when a flag is set."""
        flags, pending = C.c_uint32(), C.c_uint64()
        err = _lib.SrtErr()
        rc = _lib.lib().srt_inbound_status(self._h, C.byref(flags), C.byref(pending), C.byref(err))
        if check or (rc != _lib.SRT_OK and not flags.value):
            _lib.check(rc, err)
        return flags.value, pending.value

    def state(self) -> np.ndarray:
        """Every host's state (INBOUND_STATE_DTYPE record array)."""
        out = np.zeros(self.n_hosts, INBOUND_STATE_DTYPE)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_inbound_state(
            self._h, out.ctypes.data_as(C.POINTER(_lib.SrtInboundHostState)), C.byref(err)), err)
        return out

    def control_law(self, counts, use_table: bool = True) -> np.ndarray:
        """apply_control_law's increments for `counts`, evaluated where the stage runs."""
        c = np.ascontiguousarray(counts, np.uint64)
        out = np.zeros(len(c), np.uint64)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_inbound_control_law(
            self._h, c.ctypes.data_as(C.POINTER(C.c_uint64)), len(c), int(use_table),
            out.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(err)), err)
        return out

    def close(self):
        if self._h:
            _lib.lib().srt_inbound_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


OUT_PKT_DTYPE = np.dtype([("ready_ns", "<u8"), ("priority", "<u8"), ("total_size", "<u4"), ("socket", "<u4"),
                          ("flags", "<u4"), ("reserved", "<u4")])
OUTBOUND_STATE_DTYPE = np.dtype([(k, "<u8") for k in (
    "balance", "last_refill_ns", "task_ns", "tasks_scheduled", "sent_total", "queue_len")] + [
        (k, "<u4") for k in ("cached", "overflow")])
OUTBOUND_LATE_DTYPE = np.dtype([("seq", "<u8"), ("send_ns", "<u8"), ("send_rank", "<u8"), ("status", "<u4"),
                                ("src_host", "<u4")])


class OutboundRelay:
    """srt_outbound: every source host's interface qdisc over its sockets and
    its upload token bucket (network_interface.c, network_queuing_disciplines.c,
    relay/mod.rs, relay/token_bucket.rs) in front of the send decision, one
    call per scheduling window.

    Bound to a RoutingPlan (arrays are torch CUDA tensors of its device, the
    call is asynchronous on its stream; closing the plan closes its relays), or
    host-only with plan=None (arrays are numpy arrays, the same per-host step
    on the CPU)."""

    def __init__(self, plan: Optional[RoutingPlan], bw_up_bytes_per_s, qdisc: int, max_sockets: int, queue_cap: int):
        self.plan = plan
        bw = np.ascontiguousarray(bw_up_bytes_per_s, np.uint64)
        self.n_hosts = len(bw)
        self._h = C.c_void_p()
        if plan is not None:
            _bind_to_plan(self, plan)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_outbound_create(plan.handle if plan is not None else None, self.n_hosts,
                                                  bw.ctypes.data_as(C.POINTER(C.c_uint64)), int(qdisc),
                                                  int(max_sockets), int(queue_cap), C.byref(self._h),
                                                  C.byref(err)), err)

    _ptr = staticmethod(InboundRouter._ptr)

    def run(self, pkts, host_ptr, until_ns: int, bootstrap_end_ns: int, status, send_ns, send_rank, late=None,
            late_count=None) -> int:
        """srt_outbound_run.  pkts: a uint8 view of 32-byte srt_out_pkt records
        (OUT_PKT_DTYPE) grouped by source host, host_ptr int32/uint32
        [n_hosts+1]; outputs status int32/uint32, send_ns and send_rank
        int64/uint64, all [n_pkts]; late: a uint8 buffer of 32-byte
        srt_outbound_late records (OUTBOUND_LATE_DTYPE) with late_count a
        1-element int32/uint32.  Returns the batch's sequence base.  Device
        form: enqueue only (status() synchronises)."""
        n_pkts = int(status.numel() if hasattr(status, "numel") else status.size)
        late_cap = 0
        if late is not None:
            late_cap = int(late.numel() * late.element_size() if hasattr(late, "numel") else late.nbytes) // 32
        cur = ps = None
        if self.plan is not None:
            import torch

            ps = torch.cuda.ExternalStream(self.plan.stream_ptr(), device=status.device)
            cur = torch.cuda.current_stream(status.device)
            ps.wait_stream(cur)
        base = C.c_uint64()
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_outbound_run(
            self._h, self._ptr(pkts), self._ptr(host_ptr), n_pkts, int(until_ns), int(bootstrap_end_ns),
            self._ptr(status), self._ptr(send_ns), self._ptr(send_rank), self._ptr(late), late_cap,
            self._ptr(late_count), C.byref(base), C.byref(err)), err)
        if cur is not None:
            cur.wait_stream(ps)  # torch-side consumers see the outputs (device-side ordering)
        return base.value

    def status(self, check: bool = True):
        """srt_outbound_status: synchronises; (flags, packets still pending).
        check=True raises SrtError when a flag is set."""
        flags, pending = C.c_uint32(), C.c_uint64()
        err = _lib.SrtErr()
        rc = _lib.lib().srt_outbound_status(self._h, C.byref(flags), C.byref(pending), C.byref(err))
        if check or (rc != _lib.SRT_OK and not flags.value):
            _lib.check(rc, err)
        return flags.value, pending.value

    def state(self) -> np.ndarray:
        """Every host's state (OUTBOUND_STATE_DTYPE record array)."""
        out = np.zeros(self.n_hosts, OUTBOUND_STATE_DTYPE)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_outbound_state(
            self._h, out.ctypes.data_as(C.POINTER(_lib.SrtOutboundHostState)), C.byref(err)), err)
        return out

    def cached_seq(self, out):
        """srt_outbound_cached_seq: out int64/uint64 [n_hosts] receives the seq of the
        packet every host's relay holds cached after the last run, or UINT64_MAX.
        Device form: enqueue only."""
        if SendBatch._nbytes(out) < 8 * self.n_hosts:
            raise ValueError("OutboundRelay.cached_seq: out is smaller than n_hosts")
        cur, ps = FlightStore._streams(self, out) if self.n_hosts else (None, None)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_outbound_cached_seq(self._h, self._ptr(out), C.byref(err)), err)
        if cur is not None:
            cur.wait_stream(ps)
        return out

    def close(self):
        if self._h:
            _lib.lib().srt_outbound_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SEND_META_DTYPE = np.dtype([("src_row", "<u4"), ("dst_row", "<u4"), ("payload_size", "<u4"), ("user", "<u4")])
SRT_PKT_DTYPE = np.dtype([("src_host", "<u4"), ("src_row", "<u4"), ("dst_row", "<u4"), ("payload_size", "<u4"),
                          ("t_ns", "<u8")])


class SendBatch:
    """srt_sendbatch: one OutboundRelay.run call's results gathered into the
    grouped srt_pkt batch the send decision takes -- per host a count and the
    smallest rank, a scan over the hosts, a scatter; no sort.  The instance
    keeps the log of log_cap srt_send_meta records (SEND_META_DTYPE) through
    which packets that leave the relay in a later call get their rows back.

    Bound to a RoutingPlan (arrays are torch CUDA tensors of its device, the
    call is asynchronous on its stream; closing the plan closes it), or
    host-only with plan=None (arrays are numpy arrays, the same step on the
    CPU)."""

    def __init__(self, plan: Optional[RoutingPlan], n_hosts: int, log_cap: int):
        self.plan = plan
        self.n_hosts = int(n_hosts)
        self._h = C.c_void_p()
        if plan is not None:
            _bind_to_plan(self, plan)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_sendbatch_create(plan.handle if plan is not None else None, self.n_hosts,
                                                   int(log_cap), C.byref(self._h), C.byref(err)), err)

    _ptr = staticmethod(InboundRouter._ptr)

    @staticmethod
    def _nbytes(a):
        if a is None:
            return 0
        return int(a.numel() * a.element_size() if hasattr(a, "numel") else a.nbytes)

    def run(self, host_ptr, meta, send_ns, send_rank, seq_base: int, late, late_count, out_pkts, out_host_ptr,
            out_user, out_seq):
        """srt_sendbatch_run on the arrays of the OutboundRelay.run call just
        made (host_ptr, send_ns, send_rank, its return value as seq_base, late,
        late_count) and meta, a uint8 view of 16-byte srt_send_meta records,
        one a batch packet.  Outputs: out_pkts, a uint8 buffer of out_cap
        24-byte srt_pkt records, out_host_ptr int32/uint32 [n_hosts+1], out_user
        int32/uint32 [out_cap] (its size is out_cap), out_seq int64/uint64
        [out_cap].  Device form: enqueue only (status() synchronises)."""
        n_pkts = int(send_rank.numel() if hasattr(send_rank, "numel") else send_rank.size)
        late_cap = self._nbytes(late) // 32
        out_cap = self._nbytes(out_user) // 4
        if self._nbytes(out_pkts) < 24 * out_cap or self._nbytes(out_seq) < 8 * out_cap or \
                self._nbytes(out_host_ptr) < 4 * (self.n_hosts + 1) or self._nbytes(meta) < 16 * n_pkts:
            raise ValueError("SendBatch.run: an array is smaller than its record count")
        cur = ps = None
        if self.plan is not None:
            import torch

            ps = torch.cuda.ExternalStream(self.plan.stream_ptr(), device=out_host_ptr.device)
            cur = torch.cuda.current_stream(out_host_ptr.device)
            ps.wait_stream(cur)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_sendbatch_run(
            self._h, self._ptr(host_ptr), n_pkts, self._ptr(meta), self._ptr(send_ns), self._ptr(send_rank),
            int(seq_base), self._ptr(late), late_cap, self._ptr(late_count), self._ptr(out_pkts),
            self._ptr(out_host_ptr), self._ptr(out_user), self._ptr(out_seq), out_cap, C.byref(err)), err)
        if cur is not None:
            cur.wait_stream(ps)  # torch-side consumers see the outputs (device-side ordering)

    def status(self, check: bool = True):
        """srt_sendbatch_status: synchronises; (flags, sent packets of the last
        call).  check=True raises SrtError when a flag is set."""
        flags, n_sent = C.c_uint32(), C.c_uint64()
        err = _lib.SrtErr()
        rc = _lib.lib().srt_sendbatch_status(self._h, C.byref(flags), C.byref(n_sent), C.byref(err))
        if check or (rc != _lib.SRT_OK and not flags.value):
            _lib.check(rc, err)
        return flags.value, n_sent.value

    def close(self):
        if self._h:
            _lib.lib().srt_sendbatch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FlightStore:
    """srt_flight: the packets a round's send decision marked SENT, kept until
    the window their deliver time falls in.  push() takes a round's
    srt_packet_events arrays as they are; pop() hands out every stored packet
    with deliver < until_ns grouped by destination host, each group in its
    event queue's pop order (deliver, source host, event id), as the arrays
    InboundRouter.run takes.

    Bound to a RoutingPlan (arrays are torch CUDA tensors of its device, the
    calls are asynchronous on its stream; closing the plan closes it), or
    host-only with plan=None (arrays are numpy arrays, the same step on the
    CPU)."""

    def __init__(self, plan: Optional[RoutingPlan], n_dst_hosts: int, pool_cap: int):
        self.plan = plan
        self.n_dst_hosts = int(n_dst_hosts)
        self._h = C.c_void_p()
        if plan is not None:
            _bind_to_plan(self, plan)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_flight_create(plan.handle if plan is not None else None, self.n_dst_hosts,
                                                int(pool_cap), C.byref(self._h), C.byref(err)), err)

    _ptr = staticmethod(InboundRouter._ptr)
    _nbytes = staticmethod(SendBatch._nbytes)

    def _streams(self, a):
        if self.plan is None:
            return None, None
        import torch

        ps = torch.cuda.ExternalStream(self.plan.stream_ptr(), device=a.device)
        cur = torch.cuda.current_stream(a.device)
        ps.wait_stream(cur)
        return cur, ps

    def push(self, host_ptr, flags, deliver, dst_host, event_id, total_size, tag=None) -> int:
        """srt_flight_push after packet_events of a round: host_ptr int32/uint32
        [n_src_hosts+1], flags int32/uint32, deliver int64/uint64, dst_host
        int32/uint32, event_id int64/uint64, total_size int32/uint32, tag
        int64/uint64 or None, all [n_pkts].  Returns the push's tag base.
        Device form: enqueue only (status() synchronises)."""
        n_pkts = self._nbytes(flags) // 4
        if self._nbytes(deliver) < 8 * n_pkts or self._nbytes(dst_host) < 4 * n_pkts or \
                self._nbytes(event_id) < 8 * n_pkts or self._nbytes(total_size) < 4 * n_pkts or \
                (tag is not None and self._nbytes(tag) < 8 * n_pkts) or self._nbytes(host_ptr) < 4:
            raise ValueError("FlightStore.push: an array is smaller than its record count")
        cur, ps = self._streams(host_ptr)
        base = C.c_uint64()
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_flight_push(
            self._h, self._ptr(host_ptr), self._nbytes(host_ptr) // 4 - 1, n_pkts, self._ptr(flags),
            self._ptr(deliver), self._ptr(dst_host), self._ptr(event_id), self._ptr(total_size), self._ptr(tag),
            C.byref(base), C.byref(err)), err)
        if cur is not None:
            cur.wait_stream(ps)
        return base.value

    def pop(self, until_ns: int, w_order, w_dst_ptr, w_deliver, w_total_size, w_src_host, w_event_id, w_tag):
        """srt_flight_pop: one window.  Outputs w_order int32/uint32 (its size is
        out_cap), w_dst_ptr int32/uint32 [n_dst_hosts+1], w_deliver
        int64/uint64, w_total_size and w_src_host int32/uint32, w_event_id and
        w_tag int64/uint64, [out_cap] each.  Device form: enqueue only
        (status() synchronises and tells how many were popped)."""
        out_cap = self._nbytes(w_order) // 4
        if self._nbytes(w_dst_ptr) < 4 * (self.n_dst_hosts + 1) or self._nbytes(w_deliver) < 8 * out_cap or \
                self._nbytes(w_total_size) < 4 * out_cap or self._nbytes(w_src_host) < 4 * out_cap or \
                self._nbytes(w_event_id) < 8 * out_cap or self._nbytes(w_tag) < 8 * out_cap:
            raise ValueError("FlightStore.pop: an array is smaller than its record count")
        cur, ps = self._streams(w_dst_ptr)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_flight_pop(
            self._h, int(until_ns), self._ptr(w_order), self._ptr(w_dst_ptr), self._ptr(w_deliver),
            self._ptr(w_total_size), self._ptr(w_src_host), self._ptr(w_event_id), self._ptr(w_tag), out_cap,
            C.byref(err)), err)
        if cur is not None:
            cur.wait_stream(ps)  # torch-side consumers see the outputs (device-side ordering)

    def status(self, check: bool = True):
        """srt_flight_status: synchronises; (flags, due count of the last pop,
        packets stored, packets lost since create).  check=True raises SrtError
        when a flag is set."""
        flags, popped, stored, lost = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        err = _lib.SrtErr()
        rc = _lib.lib().srt_flight_status(self._h, C.byref(flags), C.byref(popped), C.byref(stored), C.byref(lost),
                                          C.byref(err))
        if check or (rc != _lib.SRT_OK and not flags.value):
            _lib.check(rc, err)
        return flags.value, popped.value, stored.value, lost.value

    def close(self):
        if self._h:
            _lib.lib().srt_flight_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


RX_META_DTYPE = np.dtype([("peer_ip_be", "<u4"), ("peer_port_be", "<u2"), ("local_port_be", "<u2"),
                          ("protocol", "<u4"), ("user", "<u4")])
ASSOC_DTYPE = np.dtype([("host", "<u4"), ("protocol", "<u4"), ("peer_ip_be", "<u4"), ("local_port_be", "<u2"),
                        ("peer_port_be", "<u2"), ("socket", "<u4")])


class DeliverStage:
    """srt_deliver: the interface's receive stage behind InboundRouter.run
    (networkinterface_push): the forwarded packets of one inbound call, late
    ones included, grouped by destination host in the order the interface
    receives them, each with the socket its host's associations give it at the
    call.  associate() / disassociate() keep the associations (ASSOC_DTYPE
    records, on the host); note() stores a round's RX_META_DTYPE records under
    the flight tags of the round's push; run() delivers.

    Bound to a RoutingPlan (arrays are torch CUDA tensors of its device, the
    calls are asynchronous on its stream; closing the plan closes it), or
    host-only with plan=None (arrays are numpy arrays, the same step on the
    CPU)."""

    def __init__(self, plan: Optional[RoutingPlan], n_hosts: int, table_slots_min: int, note_cap: int, log_cap: int):
        self.plan = plan
        self.n_hosts = int(n_hosts)
        self._h = C.c_void_p()
        if plan is not None:
            _bind_to_plan(self, plan)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_deliver_create(plan.handle if plan is not None else None, self.n_hosts,
                                                 int(table_slots_min), int(note_cap), int(log_cap),
                                                 C.byref(self._h), C.byref(err)), err)

    _ptr = staticmethod(InboundRouter._ptr)
    _nbytes = staticmethod(SendBatch._nbytes)
    _streams = FlightStore._streams

    def associate(self, assoc):
        """srt_deliver_associate: ASSOC_DTYPE records (a host numpy array).
        Raises SrtError, and adds nothing, when a key exists already."""
        a = np.ascontiguousarray(assoc, ASSOC_DTYPE)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_deliver_associate(self._h, a.ctypes.data, len(a), C.byref(err)), err)

    def disassociate(self, assoc):
        """srt_deliver_disassociate: ASSOC_DTYPE records; `socket` is ignored, a missing key is a no-op."""
        a = np.ascontiguousarray(assoc, ASSOC_DTYPE)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_deliver_disassociate(self._h, a.ctypes.data, len(a), C.byref(err)), err)

    def lookup(self, hosts, meta) -> np.ndarray:
        """srt_deliver_lookup on the host: the socket of every (host, RX_META_DTYPE record), 0xffffffff: none."""
        h = np.ascontiguousarray(hosts, np.uint32)
        m = np.ascontiguousarray(meta, RX_META_DTYPE)
        if len(h) != len(m):
            raise ValueError("DeliverStage.lookup: hosts and meta differ in length")
        out = np.zeros(len(h), np.uint32)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_deliver_lookup(self._h, h.ctypes.data, m.ctypes.data, len(h), out.ctypes.data,
                                                 C.byref(err)), err)
        return out

    def lookup_flat(self, hosts, meta, sockets):
        """srt_deliver_lookup_flat: hosts int32/uint32 [n], meta a uint8 view of
        n 16-byte srt_rx_meta records, the output sockets int32/uint32 [n]
        (0xffffffff: none, a host >= n_hosts included).  Device form: enqueue
        only; the table is uploaded first when it has changed."""
        n = self._nbytes(hosts) // 4
        if self._nbytes(meta) < 16 * n or self._nbytes(sockets) < 4 * n:
            raise ValueError("DeliverStage.lookup_flat: an array is smaller than its record count")
        cur, ps = self._streams(hosts) if n else (None, None)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_deliver_lookup_flat(self._h, self._ptr(hosts), self._ptr(meta), n,
                                                      self._ptr(sockets), C.byref(err)), err)
        if cur is not None:
            cur.wait_stream(ps)

    def table_stats(self):
        """srt_deliver_table_stats ->(associations, slots, longest probe sequence, a chain wraps the end)"""
        n, s, p, w, err = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint32(), _lib.SrtErr()
        _lib.check(_lib.lib().srt_deliver_table_stats(self._h, C.byref(n), C.byref(s), C.byref(p), C.byref(w),
                                                      C.byref(err)), err)
        return n.value, s.value, p.value, bool(w.value)

    def note(self, meta, tag_base: int):
        """srt_deliver_note after FlightStore.push (tag=None) of a round: meta, a
        uint8 view of the round's 16-byte srt_rx_meta records, one a batch
        packet; tag_base as the push returned it."""
        n_pkts = self._nbytes(meta) // 16
        cur, ps = self._streams(meta) if n_pkts else (None, None)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_deliver_note(self._h, self._ptr(meta), n_pkts, int(tag_base), C.byref(err)), err)
        if cur is not None:
            cur.wait_stream(ps)

    def run(self, dst_ptr, tag, status, forward_ns, seq_base: int, late, late_count, out_host_ptr, out_socket,
            out_forward_ns, out_tag, out_user, out_status):
        """srt_deliver_run on the arrays of the InboundRouter.run call just made:
        dst_ptr int32/uint32 [n_hosts+1] and tag int64/uint64 (FlightStore.pop's
        w_dst_ptr and w_tag), status int32/uint32 (its size is n_pkts) and
        forward_ns int64/uint64, its return value as seq_base, late (a uint8
        buffer of 24-byte records) and late_count.  Outputs: out_host_ptr
        int32/uint32 [n_hosts+1]; out_socket int32/uint32 (its size is out_cap),
        out_forward_ns and out_tag int64/uint64, out_user and out_status
        int32/uint32, [out_cap] each.  Device form: enqueue only (status()
        synchronises)."""
        n_pkts = self._nbytes(status) // 4
        late_cap = self._nbytes(late) // 24
        out_cap = self._nbytes(out_socket) // 4
        if self._nbytes(dst_ptr) < 4 * (self.n_hosts + 1) or self._nbytes(out_host_ptr) < 4 * (self.n_hosts + 1) or \
                self._nbytes(tag) < 8 * n_pkts or self._nbytes(forward_ns) < 8 * n_pkts or \
                self._nbytes(out_forward_ns) < 8 * out_cap or self._nbytes(out_tag) < 8 * out_cap or \
                self._nbytes(out_user) < 4 * out_cap or self._nbytes(out_status) < 4 * out_cap:
            raise ValueError("DeliverStage.run: an array is smaller than its record count")
        cur, ps = self._streams(out_host_ptr)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_deliver_run(
            self._h, self._ptr(dst_ptr), n_pkts, self._ptr(tag), self._ptr(status), self._ptr(forward_ns),
            int(seq_base), self._ptr(late), late_cap, self._ptr(late_count), self._ptr(out_host_ptr),
            self._ptr(out_socket), self._ptr(out_forward_ns), self._ptr(out_tag), self._ptr(out_user),
            self._ptr(out_status), out_cap, C.byref(err)), err)
        if cur is not None:
            cur.wait_stream(ps)  # torch-side consumers see the outputs (device-side ordering)

    def status(self, check: bool = True):
        """srt_deliver_status: synchronises; (flags, delivered packets of the
        last run, those no socket took).  check=True raises SrtError when a
        flag is set."""
        flags, n, miss = C.c_uint32(), C.c_uint64(), C.c_uint64()
        err = _lib.SrtErr()
        rc = _lib.lib().srt_deliver_status(self._h, C.byref(flags), C.byref(n), C.byref(miss), C.byref(err))
        if check or (rc != _lib.SRT_OK and not flags.value):
            _lib.check(rc, err)
        return flags.value, n.value, miss.value

    def close(self):
        if self._h:
            _lib.lib().srt_deliver_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


TRK_META_DTYPE = np.dtype([("header_size", "<u4"), ("payload_size", "<u4"), ("flags", "<u4"), ("socket_slot", "<u4")])
TRK_COUNTER_FIELDS = ("packets_control", "bytes_control_header", "packets_control_retrans",
                      "bytes_control_header_retrans", "packets_data", "bytes_data_header", "bytes_data_payload",
                      "packets_data_retrans", "bytes_data_header_retrans", "bytes_data_payload_retrans")
TRK_COUNTERS_DTYPE = np.dtype([(k, "<u8") for k in TRK_COUNTER_FIELDS])


class Tracker:
    """srt_tracker: the tracker's heartbeat byte counters of the internet
    interface (host/tracker.c), per host and per socket slot, in and out,
    kept where the pipeline runs: tx() counts what the interface popped in
    the OutboundRelay.run call just made, note() stores a round's
    TRK_META_DTYPE records under the flight tags of the round's push, rx()
    counts DeliverStage.run's list, rx_flat() ungrouped records, heartbeat()
    returns and clears the selected records (TRK_COUNTERS_DTYPE).

    Bound to a RoutingPlan (arrays are torch CUDA tensors of its device, the
    calls are asynchronous on its stream; closing the plan closes it), or
    host-only with plan=None (arrays are numpy arrays, the same step on the
    CPU)."""

    def __init__(self, plan: Optional[RoutingPlan], n_hosts: int, n_sockets: int, note_cap: int, log_cap: int):
        self.plan = plan
        self.n_hosts, self.n_sockets = int(n_hosts), int(n_sockets)
        self._h = C.c_void_p()
        if plan is not None:
            _bind_to_plan(self, plan)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_tracker_create(plan.handle if plan is not None else None, self.n_hosts,
                                                 self.n_sockets, int(note_cap), int(log_cap), C.byref(self._h),
                                                 C.byref(err)), err)

    _ptr = staticmethod(InboundRouter._ptr)
    _nbytes = staticmethod(SendBatch._nbytes)
    _streams = FlightStore._streams

    def tx(self, cached_seq, host_ptr, meta, status, seq_base: int, late=None, late_count=None):
        """srt_tracker_tx on the arrays of the OutboundRelay.run call just made:
        cached_seq int64/uint64 [n_hosts] as OutboundRelay.cached_seq wrote it
        after that call, host_ptr int32/uint32 [n_hosts+1], meta a uint8 view of
        16-byte srt_trk_meta records, one a batch packet, status int32/uint32
        (its size is n_pkts), the run's return value as seq_base, late (a uint8
        buffer of 32-byte records) and late_count.  Device form: enqueue only."""
        n_pkts = self._nbytes(status) // 4
        late_cap = self._nbytes(late) // 32
        if self._nbytes(cached_seq) < 8 * self.n_hosts or self._nbytes(host_ptr) < 4 * (self.n_hosts + 1) or \
                self._nbytes(meta) < 16 * n_pkts or (late_cap and late_count is None):
            raise ValueError("Tracker.tx: an array is smaller than its record count")
        cur, ps = self._streams(host_ptr)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_tracker_tx(
            self._h, self._ptr(cached_seq), self._ptr(host_ptr), n_pkts, self._ptr(meta), self._ptr(status),
            int(seq_base), self._ptr(late), late_cap, self._ptr(late_count), C.byref(err)), err)
        if cur is not None:
            cur.wait_stream(ps)

    def note(self, meta, tag_base: int):
        """srt_tracker_note after FlightStore.push (tag=None) of a round: meta, a
        uint8 view of the round's 16-byte srt_trk_meta records, one a batch
        packet; tag_base as the push returned it."""
        n_pkts = self._nbytes(meta) // 16
        cur, ps = self._streams(meta) if n_pkts else (None, None)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_tracker_note(self._h, self._ptr(meta), n_pkts, int(tag_base), C.byref(err)), err)
        if cur is not None:
            cur.wait_stream(ps)

    def rx(self, out_host_ptr, out_socket, out_tag, out_status):
        """srt_tracker_rx on DeliverStage.run's outputs as they are: out_host_ptr
        int32/uint32 [n_hosts+1], out_socket int32/uint32 (its size is
        out_cap), out_tag int64/uint64 and out_status int32/uint32 [out_cap].
        Device form: enqueue only; nothing is read back."""
        out_cap = self._nbytes(out_socket) // 4
        if self._nbytes(out_host_ptr) < 4 * (self.n_hosts + 1) or self._nbytes(out_tag) < 8 * out_cap or \
                self._nbytes(out_status) < 4 * out_cap:
            raise ValueError("Tracker.rx: an array is smaller than its record count")
        cur, ps = self._streams(out_host_ptr)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_tracker_rx(self._h, self._ptr(out_host_ptr), self._ptr(out_socket),
                                             self._ptr(out_tag), self._ptr(out_status), out_cap, C.byref(err)), err)
        if cur is not None:
            cur.wait_stream(ps)

    def rx_flat(self, host, socket, meta):
        """srt_tracker_rx_flat: host and socket int32/uint32 [n], meta a uint8
        view of n 16-byte srt_trk_meta records."""
        n = self._nbytes(host) // 4
        if self._nbytes(socket) < 4 * n or self._nbytes(meta) < 16 * n:
            raise ValueError("Tracker.rx_flat: an array is smaller than its record count")
        cur, ps = self._streams(host) if n else (None, None)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_tracker_rx_flat(self._h, self._ptr(host), self._ptr(socket), self._ptr(meta), n,
                                                  C.byref(err)), err)
        if cur is not None:
            cur.wait_stream(ps)

    def heartbeat(self, hosts=None, sockets=None):
        """srt_tracker_heartbeat: synchronises; returns (node_in, node_out,
        sock_in, sock_out), TRK_COUNTERS_DTYPE record arrays for the selected
        hosts and socket slots (None: all; an empty list: none), and clears
        exactly those records."""
        def sel(x, n_all):
            if x is None:
                return None, n_all
            a = np.ascontiguousarray(x, np.uint32).reshape(-1)
            if not len(a):
                a = np.zeros(1, np.uint32)  # a selection of none: a non-NULL pointer, count 0
                return a, 0
            return a, len(a)

        hs, nh = sel(hosts, self.n_hosts)
        ss, ns = sel(sockets, self.n_sockets)
        outs = [np.zeros(nh, TRK_COUNTERS_DTYPE), np.zeros(nh, TRK_COUNTERS_DTYPE),
                np.zeros(ns, TRK_COUNTERS_DTYPE), np.zeros(ns, TRK_COUNTERS_DTYPE)]
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_tracker_heartbeat(
            self._h, None if hs is None else hs.ctypes.data, nh, None if ss is None else ss.ctypes.data, ns,
            *[o.ctypes.data if len(o) else None for o in outs], C.byref(err)), err)
        return tuple(outs)

    def status(self, check: bool = True):
        """srt_tracker_status: synchronises; (flags, packets counted on the
        output side since create, on the input side).  check=True raises
        SrtError when a flag is set."""
        flags, a, b = C.c_uint32(), C.c_uint64(), C.c_uint64()
        err = _lib.SrtErr()
        rc = _lib.lib().srt_tracker_status(self._h, C.byref(flags), C.byref(a), C.byref(b), C.byref(err))
        if check or (rc != _lib.SRT_OK and not flags.value):
            _lib.check(rc, err)
        return flags.value, a.value, b.value

    @staticmethod
    def counter_string(rec) -> str:
        """srt_tracker_counter_string: the twelve comma-separated numbers of a
        heartbeat line for one TRK_COUNTERS_DTYPE record."""
        r = np.ascontiguousarray(rec, TRK_COUNTERS_DTYPE).reshape(-1)[:1].copy()
        buf = C.create_string_buffer(256)
        if _lib.lib().srt_tracker_counter_string(r.ctypes.data, buf, 256) < 0:
            raise ValueError("Tracker.counter_string: bad record")
        return buf.value.decode()

    def close(self):
        if self._h:
            _lib.lib().srt_tracker_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


PCAP_REC_DTYPE = np.dtype([("time_ns", "<u8"), ("payload_off", "<u8"), ("src_ip_be", "<u4"), ("dst_ip_be", "<u4"),
                           ("src_port_be", "<u2"), ("dst_port_be", "<u2"), ("seq", "<u4"), ("ack", "<u4"),
                           ("window", "<u2"), ("payload_len", "<u2"), ("protocol", "u1"), ("tcp_flags", "u1"),
                           ("wscale", "u1"), ("wscale_set", "u1"), ("reserved", "<u4")])


class PcapCapture:
    """srt_pcap: the pcap capture of one interface class, a byte stream a
    host, formatted where the pipeline runs: run() merges a span's sent and
    received PCAP_REC_DTYPE records per host by time and writes every record
    as 16 + incl_len bytes into `out`, host h's at out[host_off[h]:
    host_off[h + 1]].  open_files() / append_files() are the file side, on
    the host.

    Bound to a RoutingPlan (arrays are torch CUDA tensors of its device, the
    calls are asynchronous on its stream; closing the plan closes it), or
    host-only with plan=None (arrays are numpy arrays, the same step on the
    CPU)."""

    def __init__(self, plan: Optional[RoutingPlan], n_hosts: int, capture_len: int, rec_cap: int, enabled=None,
                 flags: int = _lib.PCAP_RX_FIRST):
        self.plan = plan
        self.n_hosts, self.capture_len, self.rec_cap = int(n_hosts), int(capture_len), int(rec_cap)
        self._h = C.c_void_p()
        en = None
        if enabled is not None:
            en = np.ascontiguousarray(np.asarray(enabled) != 0, np.uint8).reshape(-1)
            if len(en) != self.n_hosts:
                raise ValueError("PcapCapture: enabled has not n_hosts entries")
        if plan is not None:
            _bind_to_plan(self, plan)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_pcap_create(plan.handle if plan is not None else None, self.n_hosts,
                                              self.capture_len, en.ctypes.data if en is not None and len(en) else None,
                                              self.rec_cap, int(flags), C.byref(self._h), C.byref(err)), err)

    _ptr = staticmethod(InboundRouter._ptr)
    _nbytes = staticmethod(SendBatch._nbytes)
    _streams = FlightStore._streams

    def run(self, tx, tx_host_ptr, rx, rx_host_ptr, payload, out, host_off, tx_idx=None, rx_idx=None):
        """srt_pcap_run.  tx / rx: uint8 views of 48-byte srt_pcap_rec records
        (or None), tx_host_ptr / rx_host_ptr int32/uint32 [n_hosts+1], tx_idx /
        rx_idx optional int32/uint32 indirections (the list's length is then
        the index array's), payload uint8 or None, out uint8 (its size is
        out_cap), host_off int64/uint64 [n_hosts+1].  Device form: enqueue
        only; nothing is read back."""
        n_tx = self._nbytes(tx_idx) // 4 if tx_idx is not None else self._nbytes(tx) // 48
        n_rx = self._nbytes(rx_idx) // 4 if rx_idx is not None else self._nbytes(rx) // 48
        if self._nbytes(tx_host_ptr) < 4 * (self.n_hosts + 1) or self._nbytes(rx_host_ptr) < 4 * (self.n_hosts + 1) or \
                self._nbytes(host_off) < 8 * (self.n_hosts + 1):
            raise ValueError("PcapCapture.run: an array is smaller than its record count")
        cur, ps = self._streams(host_off)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_pcap_run(
            self._h, self._ptr(tx) if n_tx else None, self._ptr(tx_idx), self._ptr(tx_host_ptr), n_tx,
            self._ptr(rx) if n_rx else None, self._ptr(rx_idx), self._ptr(rx_host_ptr), n_rx,
            self._ptr(payload) if self._nbytes(payload) else None, self._nbytes(payload),
            self._ptr(out) if self._nbytes(out) else None, self._nbytes(out), self._ptr(host_off), C.byref(err)), err)
        if cur is not None:
            cur.wait_stream(ps)

    def status(self, check: bool = True):
        """srt_pcap_status: synchronises; (flags, records written since create,
        bytes written since create).  check=True raises SrtError when a flag
        is set."""
        flags, a, b = C.c_uint32(), C.c_uint64(), C.c_uint64()
        err = _lib.SrtErr()
        rc = _lib.lib().srt_pcap_status(self._h, C.byref(flags), C.byref(a), C.byref(b), C.byref(err))
        if check or (rc != _lib.SRT_OK and not flags.value):
            _lib.check(rc, err)
        return flags.value, a.value, b.value

    @staticmethod
    def file_header(capture_len: int) -> bytes:
        """srt_pcap_file_header: the 24 bytes a capture file starts with."""
        buf = C.create_string_buffer(24)
        _lib.lib().srt_pcap_file_header(int(capture_len), C.cast(buf, C.c_void_p))
        return buf.raw

    @staticmethod
    def tile_bytes() -> int:
        """srt_pcap_tile_bytes: the write pass's tile."""
        return int(_lib.lib().srt_pcap_tile_bytes())

    def open_files(self, paths):
        """srt_pcap_open_files: paths, n_hosts file names (None: no file);
        each is created or truncated and gets the file header.  The
        reference's name is <dir>/<hostname>-<interface name>.pcap."""
        if len(paths) != self.n_hosts:
            raise ValueError("PcapCapture.open_files: paths has not n_hosts entries")
        arr = (C.c_char_p * max(1, self.n_hosts))(*[None if p is None else os.fsencode(p) for p in paths])
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_pcap_open_files(self._h, arr, C.byref(err)), err)

    def append_files(self, host_off, data):
        """srt_pcap_append_files: a call's host_off and out bytes, on the host
        (numpy arrays), appended to the hosts' files."""
        ho = np.ascontiguousarray(host_off).view(np.uint64).reshape(-1)
        if len(ho) != self.n_hosts + 1:
            raise ValueError("PcapCapture.append_files: host_off has not n_hosts + 1 entries")
        d = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        if len(d) < int(ho[-1]):
            raise ValueError("PcapCapture.append_files: data is shorter than host_off[n_hosts]")
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_pcap_append_files(self._h, ho.ctypes.data, d.ctypes.data if len(d) else None,
                                                    C.byref(err)), err)

    def close(self):
        if self._h:
            _lib.lib().srt_pcap_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LoopbackRelay:
    """srt_loopback: the loopback interface of every host -- the qdisc's order
    at each instant, relay_loopback's forward task, the receive with the
    loopback interface's own associations (a DeliverStage of the same plan and
    n_hosts) and the tracker's local counters, one fused call.  run() orders,
    looks up and counts; heartbeat() returns and clears the selected local
    records (TRK_COUNTERS_DTYPE, Tracker.counter_string formats them); tasks()
    gives the forward tasks scheduled a host.

    Bound to a RoutingPlan (arrays are torch CUDA tensors of its device, the
    calls are asynchronous on its stream; closing the plan closes it), or
    host-only with plan=None (arrays are numpy arrays, the same step on the
    CPU)."""

    def __init__(self, plan: Optional[RoutingPlan], n_hosts: int, qdisc: int, max_sockets: int, n_slots: int):
        self.plan = plan
        self.n_hosts, self.n_slots = int(n_hosts), int(n_slots)
        self._h = C.c_void_p()
        if plan is not None:
            _bind_to_plan(self, plan)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_loopback_create(plan.handle if plan is not None else None, self.n_hosts, int(qdisc),
                                                  int(max_sockets), self.n_slots, C.byref(self._h), C.byref(err)), err)

    _ptr = staticmethod(InboundRouter._ptr)
    _nbytes = staticmethod(SendBatch._nbytes)
    _streams = FlightStore._streams

    def run(self, deliver: DeliverStage, pkts, host_ptr, rx_meta, trk_meta, out_index, out_socket, out_recv_ns,
            out_user, out_status):
        """srt_loopback_run.  deliver: the DeliverStage that holds the loopback
        interface's associations; pkts a uint8 view of 32-byte srt_out_pkt
        records (OUT_PKT_DTYPE) grouped by host, host_ptr int32/uint32
        [n_hosts+1], rx_meta and trk_meta uint8 views of 16-byte records, one
        a packet (trk_meta None: nothing is counted).  Outputs [n_pkts]:
        out_index, out_socket, out_user, out_status int32/uint32, out_recv_ns
        int64/uint64.  Device form: enqueue only."""
        n_pkts = self._nbytes(pkts) // 32
        if self._nbytes(host_ptr) < 4 * (self.n_hosts + 1) or self._nbytes(rx_meta) < 16 * n_pkts or \
                (trk_meta is not None and self._nbytes(trk_meta) < 16 * n_pkts) or \
                self._nbytes(out_index) < 4 * n_pkts or self._nbytes(out_socket) < 4 * n_pkts or \
                self._nbytes(out_recv_ns) < 8 * n_pkts or self._nbytes(out_user) < 4 * n_pkts or \
                self._nbytes(out_status) < 4 * n_pkts:
            raise ValueError("LoopbackRelay.run: an array is smaller than its record count")
        cur, ps = self._streams(host_ptr)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_loopback_run(
            self._h, deliver._h, self._ptr(pkts), self._ptr(host_ptr), n_pkts, self._ptr(rx_meta),
            self._ptr(trk_meta), self._ptr(out_index), self._ptr(out_socket), self._ptr(out_recv_ns),
            self._ptr(out_user), self._ptr(out_status), C.byref(err)), err)
        if cur is not None:
            cur.wait_stream(ps)

    def heartbeat(self, hosts=None, slots=None):
        """srt_loopback_heartbeat: synchronises; returns (node_in, node_out,
        slot_in, slot_out), TRK_COUNTERS_DTYPE record arrays of the local
        counters for the selected hosts and socket slots (None: all; an empty
        list: none), and clears exactly those records."""
        def sel(x, n_all):
            if x is None:
                return None, n_all
            a = np.ascontiguousarray(x, np.uint32).reshape(-1)
            if not len(a):
                return np.zeros(1, np.uint32), 0  # a selection of none: a non-NULL pointer, count 0
            return a, len(a)

        hs, nh = sel(hosts, self.n_hosts)
        ss, ns = sel(slots, self.n_slots)
        outs = [np.zeros(nh, TRK_COUNTERS_DTYPE), np.zeros(nh, TRK_COUNTERS_DTYPE),
                np.zeros(ns, TRK_COUNTERS_DTYPE), np.zeros(ns, TRK_COUNTERS_DTYPE)]
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_loopback_heartbeat(
            self._h, None if hs is None else hs.ctypes.data, nh, None if ss is None else ss.ctypes.data, ns,
            *[o.ctypes.data if len(o) else None for o in outs], C.byref(err)), err)
        return tuple(outs)

    def tasks(self) -> np.ndarray:
        """srt_loopback_tasks: synchronises; the forward tasks every host's
        loopback relay has scheduled since create (uint64 [n_hosts])."""
        out = np.zeros(self.n_hosts, np.uint64)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_loopback_tasks(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(err)),
                   err)
        return out

    def status(self, check: bool = True):
        """srt_loopback_status: synchronises; (flags, the last run's received
        packets, those no socket took).  check=True raises SrtError when a
        flag is set."""
        flags, a, b = C.c_uint32(), C.c_uint64(), C.c_uint64()
        err = _lib.SrtErr()
        rc = _lib.lib().srt_loopback_status(self._h, C.byref(flags), C.byref(a), C.byref(b), C.byref(err))
        if check or (rc != _lib.SRT_OK and not flags.value):
            _lib.check(rc, err)
        return flags.value, a.value, b.value

    def close(self):
        if self._h:
            _lib.lib().srt_loopback_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


UDP_META_DTYPE = np.dtype([("src_ip_be", "<u4"), ("src_port_be", "<u2"), ("reserved", "<u2"), ("payload_size", "<u4"),
                           ("user", "<u4")])
UDP_READ_DTYPE = np.dtype([("time_ns", "<u8"), ("slot", "<u4"), ("len", "<u4"), ("flags", "<u4"), ("user", "<u4")])
UDP_RESULT_DTYPE = np.dtype([("tag", "<u8"), ("recv_ns", "<u8"), ("complete_ns", "<u8"), ("return_val", "<i8"),
                             ("status", "<u4"), ("msg_flags", "<u4"), ("src_ip_be", "<u4"), ("src_port_be", "<u2"),
                             ("reserved", "<u2"), ("user", "<u4"), ("read_user", "<u4")])
UDP_LATE_DTYPE = np.dtype([("seq", "<u8"), ("result", UDP_RESULT_DTYPE)])
UDP_OP_DTYPE = np.dtype([("op", "<u4"), ("slot", "<u4"), ("value", "<u8")])
UDP_STATE_DTYPE = np.dtype([("len_bytes", "<u8"), ("soft_limit", "<u8"), ("last_read_recv_ns", "<u8"),
                            ("armed_seq", "<u8"), ("n_msgs", "<u4"), ("peer_ip_be", "<u4"), ("peer_port_be", "<u2"),
                            ("open", "u1"), ("overflow", "u1"), ("reserved", "<u4")])


class UdpReceive:
    """srt_udprecv: the UDP sockets' receive buffers and reads behind
    DeliverStage.run (UdpSocket::push_in_packet, recvmsg, MessageBuffer, the
    SO_RCVBUF rule), a socket slot a lane.  socket_ptr [n_hosts+1] gives every
    host its global slots, the ones Tracker uses.  config() opens, closes,
    connects and resizes sockets (UDP_OP_DTYPE, on the host); note() stores a
    round's UDP_META_DTYPE records under the flight tags of the round's push;
    run() pushes one DeliverStage.run list into the sockets and answers the
    window's reads (UDP_READ_DTYPE -> UDP_RESULT_DTYPE, UDP_LATE_DTYPE).

    Bound to a RoutingPlan (arrays are torch CUDA tensors of its device, the
    calls are asynchronous on its stream; closing the plan closes it), or
    host-only with plan=None (arrays are numpy arrays, the same step on the
    CPU)."""

    def __init__(self, plan: Optional[RoutingPlan], socket_ptr, ring_cap: int, note_cap: int, late_cap_hint: int = 0):
        self.plan = plan
        sp = np.ascontiguousarray(socket_ptr, np.uint32).reshape(-1)
        if len(sp) < 1:
            raise ValueError("UdpReceive: socket_ptr needs n_hosts + 1 entries")
        self.n_hosts, self.n_sockets = len(sp) - 1, int(sp[-1])
        self._h = C.c_void_p()
        if plan is not None:
            _bind_to_plan(self, plan)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_udprecv_create(plan.handle if plan is not None else None, self.n_hosts,
                                                 sp.ctypes.data, int(ring_cap), int(note_cap), int(late_cap_hint),
                                                 C.byref(self._h), C.byref(err)), err)

    _ptr = staticmethod(InboundRouter._ptr)
    _nbytes = staticmethod(SendBatch._nbytes)
    _streams = FlightStore._streams

    @staticmethod
    def window_bytes() -> int:
        """srt_udprecv_window_bytes: the bytes of staged delivery records (32
        each) and reads (24 each) a wave holds in LDS"""
        return int(_lib.lib().srt_udprecv_window_bytes())

    def config(self, ops):
        """srt_udprecv_config: UDP_OP_DTYPE records (a host numpy array), applied in
        list order.  Raises SrtError, and changes nothing, for a bad slot or op."""
        a = np.ascontiguousarray(ops, UDP_OP_DTYPE).reshape(-1)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_udprecv_config(self._h, a.ctypes.data if len(a) else None, len(a), C.byref(err)), err)

    def note(self, meta, tag_base: int):
        """srt_udprecv_note after FlightStore.push (tag=None) of a round: meta, a
        uint8 view of the round's 16-byte srt_udp_meta records, one a batch
        packet; tag_base as the push returned it."""
        n_pkts = self._nbytes(meta) // 16
        cur, ps = self._streams(meta) if n_pkts else (None, None)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_udprecv_note(self._h, self._ptr(meta), n_pkts, int(tag_base), C.byref(err)), err)
        if cur is not None:
            cur.wait_stream(ps)

    def run(self, out_host_ptr, out_socket, out_forward_ns, out_tag, out_status, read_host_ptr, reads, until_ns: int,
            rx_status, results, late, late_count, first_readable_ns) -> int:
        """srt_udprecv_run on DeliverStage.run's outputs as they are: out_host_ptr
        int32/uint32 [n_hosts+1], out_socket int32/uint32 (its size is
        out_cap), out_forward_ns and out_tag int64/uint64, out_status
        int32/uint32, [out_cap] each.  read_host_ptr int32/uint32 [n_hosts+1]
        and reads, a uint8 view of 24-byte srt_udp_read records (both None: no
        reads).  Outputs: rx_status int32/uint32 [out_cap]; results, a uint8
        buffer of 56-byte srt_udp_result records, one a read; late, a uint8
        buffer of 64-byte srt_udp_late records with late_count a 1-element
        int32/uint32; first_readable_ns int64/uint64 [n_sockets].  Returns the
        reads' sequence base.  Device form: enqueue only (status() synchronises)."""
        out_cap = self._nbytes(out_socket) // 4
        n_reads = self._nbytes(reads) // 24
        late_cap = self._nbytes(late) // 64
        if self._nbytes(out_host_ptr) < 4 * (self.n_hosts + 1) or self._nbytes(out_forward_ns) < 8 * out_cap or \
                self._nbytes(out_tag) < 8 * out_cap or self._nbytes(out_status) < 4 * out_cap or \
                self._nbytes(rx_status) < 4 * out_cap or self._nbytes(results) < 56 * n_reads or \
                (n_reads and self._nbytes(read_host_ptr) < 4 * (self.n_hosts + 1)) or \
                self._nbytes(first_readable_ns) < 8 * self.n_sockets or (late_cap and late_count is None):
            raise ValueError("UdpReceive.run: an array is smaller than its record count")
        cur, ps = self._streams(out_host_ptr)
        base = C.c_uint64()
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_udprecv_run(
            self._h, self._ptr(out_host_ptr), self._ptr(out_socket), self._ptr(out_forward_ns), self._ptr(out_tag),
            self._ptr(out_status), out_cap, self._ptr(read_host_ptr), self._ptr(reads), n_reads, C.byref(base),
            int(until_ns), self._ptr(rx_status), self._ptr(results), self._ptr(late), late_cap,
            self._ptr(late_count), self._ptr(first_readable_ns), C.byref(err)), err)
        if cur is not None:
            cur.wait_stream(ps)  # torch-side consumers see the outputs (device-side ordering)
        return base.value

    def status(self, check: bool = True):
        """srt_udprecv_status: synchronises; (flags, packets the sockets
        processed, buffered, dropped since create).  check=True raises
        SrtError when a flag is set."""
        flags, a, b, d = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        err = _lib.SrtErr()
        rc = _lib.lib().srt_udprecv_status(self._h, C.byref(flags), C.byref(a), C.byref(b), C.byref(d), C.byref(err))
        if check or (rc != _lib.SRT_OK and not flags.value):
            _lib.check(rc, err)
        return flags.value, a.value, b.value, d.value

    def state(self) -> np.ndarray:
        """srt_udprecv_state: synchronises; every slot's state (UDP_STATE_DTYPE record array)."""
        out = np.zeros(self.n_sockets, UDP_STATE_DTYPE)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_udprecv_state(self._h, out.ctypes.data if len(out) else None, C.byref(err)), err)
        return out

    def close(self):
        if self._h:
            _lib.lib().srt_udprecv_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


UDP_SEND_DTYPE = np.dtype([("time_ns", "<u8"), ("priority", "<u8"), ("slot", "<u4"), ("len", "<u4"),
                           ("dst_ip_be", "<u4"), ("dst_port_be", "<u2"), ("reserved", "<u2"), ("flags", "<u4"),
                           ("user", "<u4")])
UDPSEND_RESULT_DTYPE = np.dtype([("complete_ns", "<u8"), ("priority", "<u8"), ("return_val", "<i8"), ("status", "<u4"),
                                 ("src_ip_be", "<u4"), ("src_port_be", "<u2"), ("reserved", "<u2"), ("user", "<u4")])
UDPSEND_LATE_DTYPE = np.dtype([("seq", "<u8"), ("result", UDPSEND_RESULT_DTYPE)])
UDPSEND_OP_DTYPE = np.dtype([("op", "<u4"), ("slot", "<u4"), ("value", "<u8")])
UDPSEND_SOCKET_STATE_DTYPE = np.dtype([("len_bytes", "<u8"), ("soft_limit", "<u8"), ("armed_seq", "<u8"),
                                       ("n_msgs", "<u4"), ("bound_ip_be", "<u4"), ("peer_ip_be", "<u4"),
                                       ("bound_port_be", "<u2"), ("peer_port_be", "<u2"), ("open", "u1"),
                                       ("shut_wr", "u1"), ("bound", "u1"), ("has_peer", "u1"), ("overflow", "u1"),
                                       ("reserved0", "u1"), ("reserved1", "<u2")])
UDPSEND_HOST_STATE_DTYPE = np.dtype([(k, "<u8") for k in (
    "balance", "last_refill_ns", "task_ns", "tasks_scheduled", "sent_total", "queue_len")] + [
        ("cached", "<u4"), ("overflow", "<u4"), ("next_priority", "<u8")])


class UdpSend:
    """srt_udpsend: every host's UDP send buffers and its outbound relay in one
    fused step (UdpSocket::sendmsg, pull_out_packet, MessageBuffer, the
    SO_SNDBUF rule, shutdown, close, Host::get_next_packet_priority, and
    OutboundRelay's qdisc, bucket and relay loop), a host a lane.  socket_ptr
    [n_hosts+1] gives every host its global slots, the ones UdpReceive and
    Tracker use.  config() opens, binds, connects, resizes, shuts and closes
    sockets and sets a host's priority counter (UDPSEND_OP_DTYPE, on the host);
    run() takes a window's sendmsg calls (UDP_SEND_DTYPE) and answers them
    (UDPSEND_RESULT_DTYPE, UDPSEND_LATE_DTYPE) beside OutboundRelay.run's
    outputs, which SendBatch.run takes as they are.

    Bound to a RoutingPlan (arrays are torch CUDA tensors of its device, the
    calls are asynchronous on its stream; closing the plan closes it), or
    host-only with plan=None (arrays are numpy arrays, the same step on the
    CPU)."""

    def __init__(self, plan: Optional[RoutingPlan], socket_ptr, host_ip_be, bw_up_bytes_per_s, qdisc: int,
                 ring_cap: int, late_cap_hint: int = 0):
        self.plan = plan
        sp = np.ascontiguousarray(socket_ptr, np.uint32).reshape(-1)
        if len(sp) < 1:
            raise ValueError("UdpSend: socket_ptr needs n_hosts + 1 entries")
        self.n_hosts, self.n_sockets = len(sp) - 1, int(sp[-1])
        ip = np.ascontiguousarray(host_ip_be, np.uint32).reshape(-1)
        bw = np.ascontiguousarray(bw_up_bytes_per_s, np.uint64).reshape(-1)
        if len(ip) != self.n_hosts or len(bw) != self.n_hosts:
            raise ValueError("UdpSend: host_ip_be and bw_up_bytes_per_s need n_hosts entries")
        self._h = C.c_void_p()
        if plan is not None:
            _bind_to_plan(self, plan)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_udpsend_create(plan.handle if plan is not None else None, self.n_hosts,
                                                 sp.ctypes.data, ip.ctypes.data if len(ip) else None,
                                                 bw.ctypes.data if len(bw) else None, int(qdisc), int(ring_cap),
                                                 int(late_cap_hint), C.byref(self._h), C.byref(err)), err)

    _ptr = staticmethod(InboundRouter._ptr)
    _nbytes = staticmethod(SendBatch._nbytes)
    _streams = FlightStore._streams

    @staticmethod
    def window_bytes() -> int:
        """srt_udpsend_window_bytes: the LDS a wave of the step kernel asks for"""
        return int(_lib.lib().srt_udpsend_window_bytes())

    def config(self, ops):
        """srt_udpsend_config: UDPSEND_OP_DTYPE records (a host numpy array), applied in
        list order.  Raises SrtError, and changes nothing, for a bad slot or op."""
        a = np.ascontiguousarray(ops, UDPSEND_OP_DTYPE).reshape(-1)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_udpsend_config(self._h, a.ctypes.data if len(a) else None, len(a), C.byref(err)), err)

    def run(self, call_host_ptr, calls, until_ns: int, bootstrap_end_ns: int, results, status, send_ns, send_rank,
            late, late_count, late_results, late_results_count, first_writable_ns) -> int:
        """srt_udpsend_run.  call_host_ptr int32/uint32 [n_hosts+1]; calls, a
        uint8 view of 40-byte srt_udp_send records grouped by host.  Outputs:
        results, a uint8 buffer of 40-byte srt_udpsend_result records, one a
        call; status int32/uint32, send_ns and send_rank int64/uint64, [n_calls]
        each, late (32-byte srt_outbound_late records) and late_count exactly
        as OutboundRelay.run writes them; late_results, a uint8 buffer of
        48-byte srt_udpsend_late records with late_results_count a 1-element
        int32/uint32; first_writable_ns int64/uint64 [n_sockets].  Returns the
        calls' sequence base.  Device form: enqueue only (status() synchronises)."""
        n_calls = self._nbytes(calls) // 40
        late_cap = self._nbytes(late) // 32
        late_res_cap = self._nbytes(late_results) // 48
        if self._nbytes(call_host_ptr) < 4 * (self.n_hosts + 1) or self._nbytes(results) < 40 * n_calls or \
                self._nbytes(status) < 4 * n_calls or self._nbytes(send_ns) < 8 * n_calls or \
                self._nbytes(send_rank) < 8 * n_calls or self._nbytes(first_writable_ns) < 8 * self.n_sockets or \
                (late_cap and late_count is None) or (late_res_cap and late_results_count is None):
            raise ValueError("UdpSend.run: an array is smaller than its record count")
        cur, ps = self._streams(call_host_ptr)
        base = C.c_uint64()
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_udpsend_run(
            self._h, self._ptr(call_host_ptr), self._ptr(calls), n_calls, int(until_ns), int(bootstrap_end_ns),
            self._ptr(results), self._ptr(status), self._ptr(send_ns), self._ptr(send_rank), self._ptr(late), late_cap,
            self._ptr(late_count), self._ptr(late_results), late_res_cap, self._ptr(late_results_count),
            self._ptr(first_writable_ns), C.byref(base), C.byref(err)), err)
        if cur is not None:
            cur.wait_stream(ps)  # torch-side consumers see the outputs (device-side ordering)
        return base.value

    def status(self, check: bool = True):
        """srt_udpsend_status: synchronises; (flags, packets pending, calls
        accepted, answered -EWOULDBLOCK, armed since create).  check=True raises
        SrtError when a flag is set."""
        flags = C.c_uint32()
        n = [C.c_uint64() for _ in range(4)]
        err = _lib.SrtErr()
        rc = _lib.lib().srt_udpsend_status(self._h, C.byref(flags), *[C.byref(x) for x in n], C.byref(err))
        if check or (rc != _lib.SRT_OK and not flags.value):
            _lib.check(rc, err)
        return (flags.value,) + tuple(x.value for x in n)

    def state(self):
        """srt_udpsend_state: synchronises; (hosts, UDPSEND_HOST_STATE_DTYPE; slots, UDPSEND_SOCKET_STATE_DTYPE)."""
        hosts = np.zeros(self.n_hosts, UDPSEND_HOST_STATE_DTYPE)
        socks = np.zeros(self.n_sockets, UDPSEND_SOCKET_STATE_DTYPE)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_udpsend_state(self._h, hosts.ctypes.data if len(hosts) else None,
                                                socks.ctypes.data if len(socks) else None, C.byref(err)), err)
        return hosts, socks

    def cached_seq(self, out):
        """srt_udpsend_cached_seq: out int64/uint64 [n_hosts], as OutboundRelay.cached_seq.  Device form: enqueue only."""
        if self._nbytes(out) < 8 * self.n_hosts:
            raise ValueError("UdpSend.cached_seq: out is smaller than n_hosts")
        cur, ps = self._streams(out) if self.n_hosts else (None, None)
        err = _lib.SrtErr()
        _lib.check(_lib.lib().srt_udpsend_cached_seq(self._h, self._ptr(out), C.byref(err)), err)
        if cur is not None:
            cur.wait_stream(ps)
        return out

    def close(self):
        if self._h:
            _lib.lib().srt_udpsend_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def outbound_send_order(host_ptr, send_rank, late_src_host=None, late_send_rank=None):
    """The grouped send order srt_packet_batch needs, from a round's
    OutboundRelay.run outputs, with torch ops on the tensors' device.

    host_ptr [n_hosts+1] (host_ptr[-1] == n_pkts) and send_rank int64 [n_pkts]
    (-1 == UINT64_MAX: local or not forwarded) describe the batch; late_src_host / late_send_rank (the
    first late_count records' fields) the packets of earlier calls forwarded in
    this one.  Returns (order, send_host_ptr): order int64 [n_sent] names the
    forwarded non-local packets grouped by source host, each host's by rank --
    a value i < n_pkts is batch packet i, a value n_pkts + k is late record k
    -- and send_host_ptr int32 [n_hosts+1] is the grouping of order."""
    import torch

    n_hosts = host_ptr.numel() - 1
    n_pkts = send_rank.numel()
    hp = host_ptr.to(torch.int64)
    host = torch.repeat_interleave(torch.arange(n_hosts, device=hp.device), hp[1:] - hp[:-1], output_size=n_pkts)
    rank = send_rank.to(torch.int64)
    if late_src_host is not None and late_src_host.numel():
        host = torch.cat([host, late_src_host.to(torch.int64)])
        rank = torch.cat([rank, late_send_rank.to(torch.int64)])
    sent = torch.nonzero(rank >= 0).flatten()
    # two stable sorts: by rank, then by host (ranks are below 2^63, hosts below 2^32)
    o = sent[torch.sort(rank[sent], stable=True).indices]
    o = o[torch.sort(host[o], stable=True).indices]
    counts = torch.bincount(host[o], minlength=n_hosts)
    ptr = torch.zeros(n_hosts + 1, dtype=torch.int64, device=hp.device)
    ptr[1:] = torch.cumsum(counts, 0)
    return o, ptr.to(torch.int32)
