"""ctypes binding of libsrt.so (the C ABI declared in include/srt.h).

The product path has no CPU fallback: if libsrt.so is missing or no HIP device
is visible, every entry point raises instead of computing anything elsewhere.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SRT_LIB", os.path.join(_HERE, "libsrt.so"))  # SRT_LIB: A/B builds only

SRT_OK = 0
SRT_ERR_NO_EDGE = 1
SRT_ERR_MULTI_EDGE = 2
SRT_ERR_DISCONNECTED = 3
SRT_ERR_INVALID = 4
SRT_ERR_HIP = 5
SRT_ERR_OOM = 6
SRT_ERR_UNSUPPORTED = 7
SRT_ERR_COMM = 8

SRT_ALGO_AUTO, SRT_ALGO_FW, SRT_ALGO_SSSP, SRT_ALGO_LEVEL = 0, 1, 2, 3
SRT_OPT_SAME_DEVICE = 1  # srt_opts.flags: every n_gpus rank on `device` (tests)
PDS_NONE, PDS_INET_SENT, PDS_INET_DROPPED = 0, 1 << 8, 1 << 9
PDS_ROUTER_ENQUEUED, PDS_ROUTER_DEQUEUED, PDS_ROUTER_DROPPED = 1 << 10, 1 << 11, 1 << 12
PDS_RELAY_CACHED, PDS_RELAY_FORWARDED = 1 << 21, 1 << 22
PDS_SND_INTERFACE_SENT = 1 << 7
PDS_RCV_INTERFACE_RECEIVED, PDS_RCV_INTERFACE_DROPPED = 1 << 13, 1 << 14
# srt_inbound_status flags
INBOUND_RING_OVERFLOW, INBOUND_LATE_OVERFLOW, INBOUND_TIME_REGRESSION, INBOUND_OVERSIZE = 1, 2, 4, 8
INBOUND_AFTER_UNTIL = 16
# srt_outbound_create qdiscs, srt_out_pkt flags, srt_outbound_status flags
QDISC_FIFO, QDISC_RR = 0, 1
OUT_LOCAL = 1
OUTBOUND_RING_OVERFLOW, OUTBOUND_LATE_OVERFLOW, OUTBOUND_TIME_REGRESSION, OUTBOUND_OVERSIZE = 1, 2, 4, 8
OUTBOUND_AFTER_UNTIL, OUTBOUND_BAD_SOCKET = 16, 32
# srt_sendbatch_status flags
SENDBATCH_OUT_OVERFLOW, SENDBATCH_RANK_GAP, SENDBATCH_LOG_OVERRUN, SENDBATCH_BAD_HOST = 1, 2, 4, 8
# srt_flight_status flags
FLIGHT_POOL_OVERFLOW, FLIGHT_OUT_OVERFLOW, FLIGHT_BAD_HOST, FLIGHT_LATE_PUSH, FLIGHT_TIME_REGRESSION = 1, 2, 4, 8, 16
# srt_assoc / srt_rx_meta protocols, srt_deliver_status flags
PROTO_TCP, PROTO_UDP = 1, 2
DELIVER_OUT_OVERFLOW, DELIVER_LOG_OVERRUN, DELIVER_NOTE_OVERRUN, DELIVER_BAD_HOST = 1, 2, 4, 8
# srt_trk_meta flags, srt_tracker_status flags
TRK_RETRANS = 1
TRACKER_LOG_OVERRUN, TRACKER_NOTE_OVERRUN, TRACKER_BAD_SOCKET, TRACKER_BAD_HOST = 1, 2, 4, 8
# srt_loopback_status flags
LOOPBACK_TIME_ORDER, LOOPBACK_BAD_SOCKET, LOOPBACK_BAD_SLOT = 1, 2, 4
# srt_pcap_create flags, srt_pcap_status flags
PCAP_RX_FIRST, PCAP_TX_FIRST = 0, 1
PCAP_OVERFLOW, PCAP_BAD_PROTOCOL, PCAP_BAD_LENGTH, PCAP_BAD_PAYLOAD, PCAP_TIME_ORDER = 1, 2, 4, 8, 16
# the UDP socket's packet status bits, srt_udp_read flags, srt_udp_result status and msg_flags,
# srt_udprecv_op ops, srt_udprecv_status flags, srt_udprecv_socket_state.overflow marks
PDS_RCV_SOCKET_PROCESSED, PDS_RCV_SOCKET_DROPPED, PDS_RCV_SOCKET_BUFFERED = 1 << 15, 1 << 16, 1 << 18
UDP_PEEK, UDP_TRUNC, UDP_WAIT = 0x2, 0x20, 0x10000
UDP_NOT_TAKEN, UDP_DONE, UDP_ARMED = 0, 1, 2
UDP_MSG_TRUNC = 0x20
UDPRECV_OPEN, UDPRECV_CLOSE, UDPRECV_SET_PEER, UDPRECV_SET_RCVBUF = 1, 2, 3, 4
UDPRECV_RING_OVERFLOW, UDPRECV_LATE_OVERFLOW, UDPRECV_NOTE_OVERRUN, UDPRECV_BAD_SOCKET = 1, 2, 4, 8
UDPRECV_READ_ORDER, UDPRECV_ARMED_TWICE = 16, 32
UDPRECV_MARK_RING, UDPRECV_MARK_NOTE = 1, 2
# the UDP send stage: its packet status bit, srt_udp_send flags, srt_udpsend_result status, srt_udpsend_op ops,
# srt_udpsend_status flags
PDS_SND_CREATED = 1 << 1
UDPSEND_HAS_ADDR, UDPSEND_WAIT, UDPSEND_RAW, UDPSEND_LOCAL = 0x1, 0x10000, 0x20000, 0x40000
UDPSEND_NOT_TAKEN, UDPSEND_DONE, UDPSEND_ARMED = 0, 1, 2
UDPSEND_OPEN, UDPSEND_CLOSE, UDPSEND_BIND, UDPSEND_SET_PEER, UDPSEND_SET_SNDBUF, UDPSEND_SHUT_WR = 1, 2, 3, 4, 5, 6
UDPSEND_SET_NEXT_PRIORITY = 7
UDPSEND_RING_OVERFLOW, UDPSEND_LATE_OVERFLOW, UDPSEND_TIME_REGRESSION, UDPSEND_OVERSIZE = 1, 2, 4, 8
UDPSEND_AFTER_UNTIL, UDPSEND_BAD_SOCKET, UDPSEND_UNBOUND, UDPSEND_LOOPBACK = 16, 32, 64, 128
UDPSEND_ARMED_TWICE, UDPSEND_REOPEN_BUSY, UDPSEND_LATE_RESULT_OVERFLOW, UDPSEND_CALL_ORDER = 256, 512, 1024, 2048


class SrtErr(C.Structure):
    _fields_ = [("code", C.c_int32), ("a_id", C.c_uint32), ("b_id", C.c_uint32), ("msg", C.c_char * 256)]


class SrtCsr(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_uint32),
        ("directed", C.c_uint32),
        ("n_adj", C.c_uint64),
        ("row_ptr", C.POINTER(C.c_uint64)),
        ("col", C.POINTER(C.c_uint32)),
        ("lat_ns", C.POINTER(C.c_uint64)),
        ("loss", C.POINTER(C.c_float)),
        ("node_ids", C.POINTER(C.c_uint32)),
    ]


class SrtPath(C.Structure):
    _fields_ = [("latency_ns", C.c_uint64), ("packet_loss", C.c_float), ("_pad", C.c_uint32)]


class SrtOpts(C.Structure):
    _fields_ = [("algo", C.c_uint32), ("device", C.c_int32), ("flags", C.c_uint32), ("n_gpus", C.c_uint32)]


class SrtTiming(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("dominant_ms", C.c_double), ("dominant_launches", C.c_uint64),
                ("dominant_work", C.c_double), ("loss_ms", C.c_double), ("tight_edges", C.c_uint64),
                ("sharded_tail", C.c_uint32), ("sparse_split", C.c_uint32),
                ("sparse_sweeps", C.c_uint64), ("loss_fold", C.c_uint32), ("reserved0", C.c_uint32),
                ("edge_visits", C.c_uint64), ("create_device_ms", C.c_double)]


class SrtRound(C.Structure):
    _fields_ = [("round_end_ns", C.c_uint64), ("bootstrap_end_ns", C.c_uint64), ("sim_end_ns", C.c_uint64)]


class SrtInboundLate(C.Structure):
    _fields_ = [("seq", C.c_uint64), ("forward_ns", C.c_uint64), ("status", C.c_uint32), ("dst_host", C.c_uint32)]


class SrtInboundHostState(C.Structure):
    _fields_ = [("balance", C.c_uint64), ("last_refill_ns", C.c_uint64), ("interval_end_ns", C.c_uint64),
                ("drop_next_ns", C.c_uint64), ("current_drop_count", C.c_uint64),
                ("previous_drop_count", C.c_uint64), ("queue_len", C.c_uint64), ("bytes_stored", C.c_uint64),
                ("task_ns", C.c_uint64), ("tasks_scheduled", C.c_uint64), ("mode", C.c_uint32),
                ("cached", C.c_uint32), ("overflow", C.c_uint32), ("reserved0", C.c_uint32)]


class SrtOutPkt(C.Structure):
    _fields_ = [("ready_ns", C.c_uint64), ("priority", C.c_uint64), ("total_size", C.c_uint32),
                ("socket", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class SrtOutboundLate(C.Structure):
    _fields_ = [("seq", C.c_uint64), ("send_ns", C.c_uint64), ("send_rank", C.c_uint64), ("status", C.c_uint32),
                ("src_host", C.c_uint32)]


class SrtOutboundHostState(C.Structure):
    _fields_ = [("balance", C.c_uint64), ("last_refill_ns", C.c_uint64), ("task_ns", C.c_uint64),
                ("tasks_scheduled", C.c_uint64), ("sent_total", C.c_uint64), ("queue_len", C.c_uint64),
                ("cached", C.c_uint32), ("overflow", C.c_uint32)]


class SrtError(RuntimeError):
    """Error raised by the routing build; `code` is an srt_status."""

    def __init__(self, code: int, msg: str, a_id: int = 0, b_id: int = 0):
        super().__init__(msg)
        self.code, self.a_id, self.b_id = code, a_id, b_id


_lib = None

BCAST_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64)

# name -> (restype, argtypes): the full exported surface of include/srt.h
_vp = C.c_void_p
_u64p, _u32p, _f32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_float)
_errp = C.POINTER(SrtErr)
SIGNATURES = {
    "srt_abi_version": (C.c_int, []),
    "srt_device_count": (C.c_int, []),
    "srt_compute_shortest_paths": (C.c_int, [C.POINTER(SrtCsr), _u32p, C.c_uint32, C.POINTER(SrtPath), _u64p,
                                             C.POINTER(SrtOpts), _errp]),
    "srt_get_direct_paths": (C.c_int, [C.POINTER(SrtCsr), _u32p, C.c_uint32, C.POINTER(SrtPath), _u64p,
                                       C.POINTER(SrtOpts), _errp]),
    "srt_plan_create": (C.c_int, [C.POINTER(SrtCsr), _u32p, C.c_uint32, C.POINTER(SrtOpts), C.POINTER(_vp), _errp]),
    "srt_plan_run": (C.c_int, [_vp, _errp]),
    "srt_plan_run_async": (C.c_int, [_vp, _errp]),
    "srt_plan_sync": (C.c_int, [_vp, _errp]),
    "srt_plan_fetch": (C.c_int, [_vp, C.POINTER(SrtPath), _u64p, _errp]),
    "srt_plan_table": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), _u32p]),
    "srt_plan_describe": (C.c_char_p, [_vp]),
    "srt_plan_stream": (_vp, [_vp]),
    "srt_plan_kernel_tiles": (C.c_int, [_vp, _u64p]),
    "srt_plan_kernel_stats": (C.c_int, [_vp, C.POINTER(C.c_double), _u64p, C.POINTER(C.c_double),
                                        C.POINTER(C.c_double)]),
    "srt_plan_timing": (C.c_int, [_vp, C.POINTER(SrtTiming)]),
    "srt_plan_destroy": (None, [_vp]),
    "srt_comm_unique_id": (C.c_int, [C.c_void_p, _errp]),
    "srt_comm_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(_vp), _errp]),
    "srt_comm_destroy": (None, [_vp]),
    "srt_comm_init_callbacks": (C.c_int, [C.c_int, C.c_int, _vp, _vp, _vp, C.POINTER(_vp), _errp]),
    "srt_comm_init_local": (C.c_int, [C.c_int, C.POINTER(C.c_int32), C.POINTER(_vp), _errp]),
    "srt_comm_abort": (None, [_vp]),
    "srt_plan_bind_comm": (C.c_int, [_vp, _vp, _errp]),
    "srt_plan_shard_rows": (C.c_int, [_vp, C.c_int, C.c_int, _errp]),
    "srt_packet_batch": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.c_uint64, _vp, C.POINTER(SrtRound), _vp, _vp, _vp,
                                   _vp, _errp]),
    "srt_packet_events_status": (C.c_int, [_vp, _errp]),
    "srt_packet_events": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint64, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp,
                                    _vp, _errp]),
    "srt_inbound_create": (C.c_int, [_vp, C.c_uint32, _u64p, C.c_uint32, C.POINTER(_vp), _errp]),
    "srt_inbound_run": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint64, C.c_uint64, C.c_uint64, _vp, _vp, _vp,
                                  C.c_uint32, _vp, _u64p, _errp]),
    "srt_inbound_status": (C.c_int, [_vp, _u32p, _u64p, _errp]),
    "srt_inbound_state": (C.c_int, [_vp, C.POINTER(SrtInboundHostState), _errp]),
    "srt_inbound_control_law": (C.c_int, [_vp, _u64p, C.c_uint64, C.c_int, _u64p, _errp]),
    "srt_inbound_destroy": (None, [_vp]),
    "srt_outbound_create": (C.c_int, [_vp, C.c_uint32, _u64p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_vp),
                                      _errp]),
    "srt_outbound_run": (C.c_int, [_vp, _vp, _vp, C.c_uint64, C.c_uint64, C.c_uint64, _vp, _vp, _vp, _vp,
                                   C.c_uint32, _vp, _u64p, _errp]),
    "srt_outbound_status": (C.c_int, [_vp, _u32p, _u64p, _errp]),
    "srt_outbound_state": (C.c_int, [_vp, C.POINTER(SrtOutboundHostState), _errp]),
    "srt_outbound_cached_seq": (C.c_int, [_vp, _vp, _errp]),
    "srt_outbound_destroy": (None, [_vp]),
    "srt_sendbatch_create": (C.c_int, [_vp, C.c_uint32, C.c_uint64, C.POINTER(_vp), _errp]),
    "srt_sendbatch_run": (C.c_int, [_vp, _vp, C.c_uint64, _vp, _vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp, _vp, _vp,
                                    _vp, _vp, C.c_uint64, _errp]),
    "srt_sendbatch_status": (C.c_int, [_vp, _u32p, _u64p, _errp]),
    "srt_sendbatch_destroy": (None, [_vp]),
    "srt_flight_create": (C.c_int, [_vp, C.c_uint32, C.c_uint64, C.POINTER(_vp), _errp]),
    "srt_flight_push": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, _u64p, _errp]),
    "srt_flight_pop": (C.c_int, [_vp, C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_uint64, _errp]),
    "srt_flight_status": (C.c_int, [_vp, _u32p, _u64p, _u64p, _u64p, _errp]),
    "srt_flight_destroy": (None, [_vp]),
    "srt_deliver_create": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(_vp), _errp]),
    "srt_deliver_associate": (C.c_int, [_vp, _vp, C.c_uint64, _errp]),
    "srt_deliver_disassociate": (C.c_int, [_vp, _vp, C.c_uint64, _errp]),
    "srt_deliver_lookup": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, _errp]),
    "srt_deliver_lookup_flat": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, _errp]),
    "srt_deliver_table_stats": (C.c_int, [_vp, _u64p, _u32p, _u32p, _u32p, _errp]),
    "srt_deliver_note": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, _errp]),
    "srt_deliver_run": (C.c_int, [_vp, _vp, C.c_uint64, _vp, _vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp, _vp, _vp,
                                  _vp, _vp, _vp, _vp, C.c_uint64, _errp]),
    "srt_deliver_status": (C.c_int, [_vp, _u32p, _u64p, _u64p, _errp]),
    "srt_deliver_destroy": (None, [_vp]),
    "srt_tracker_create": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(_vp), _errp]),
    "srt_tracker_tx": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp, _errp]),
    "srt_tracker_note": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, _errp]),
    "srt_tracker_rx": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint64, _errp]),
    "srt_tracker_rx_flat": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64, _errp]),
    "srt_tracker_heartbeat": (C.c_int, [_vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _errp]),
    "srt_tracker_status": (C.c_int, [_vp, _u32p, _u64p, _u64p, _errp]),
    "srt_tracker_counter_string": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "srt_tracker_destroy": (None, [_vp]),
    "srt_loopback_create": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_vp), _errp]),
    "srt_loopback_run": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _errp]),
    "srt_loopback_heartbeat": (C.c_int, [_vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _errp]),
    "srt_loopback_tasks": (C.c_int, [_vp, _u64p, _errp]),
    "srt_loopback_status": (C.c_int, [_vp, _u32p, _u64p, _u64p, _errp]),
    "srt_loopback_destroy": (None, [_vp]),
    "srt_pcap_create": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, C.c_uint64, C.c_uint32, C.POINTER(_vp), _errp]),
    "srt_pcap_run": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64, _vp, _vp, _vp, C.c_uint64, _vp, C.c_uint64, _vp,
                               C.c_uint64, _vp, _errp]),
    "srt_pcap_status": (C.c_int, [_vp, _u32p, _u64p, _u64p, _errp]),
    "srt_pcap_file_header": (None, [C.c_uint32, _vp]),
    "srt_pcap_open_files": (C.c_int, [_vp, C.POINTER(C.c_char_p), _errp]),
    "srt_pcap_append_files": (C.c_int, [_vp, _vp, _vp, _errp]),
    "srt_pcap_tile_bytes": (C.c_uint32, []),
    "srt_pcap_destroy": (None, [_vp]),
    "srt_udprecv_create": (C.c_int, [_vp, C.c_uint32, _vp, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(_vp), _errp]),
    "srt_udprecv_config": (C.c_int, [_vp, _vp, C.c_uint64, _errp]),
    "srt_udprecv_note": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, _errp]),
    "srt_udprecv_run": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_uint64, _vp, _vp, C.c_uint64, _u64p, C.c_uint64,
                                  _vp, _vp, _vp, C.c_uint32, _vp, _vp, _errp]),
    "srt_udprecv_status": (C.c_int, [_vp, _u32p, _u64p, _u64p, _u64p, _errp]),
    "srt_udprecv_state": (C.c_int, [_vp, _vp, _errp]),
    "srt_udprecv_window_bytes": (C.c_uint32, []),
    "srt_udprecv_destroy": (None, [_vp]),
    "srt_udpsend_create": (C.c_int, [_vp, C.c_uint32, _vp, _vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_vp),
                                     _errp]),
    "srt_udpsend_config": (C.c_int, [_vp, _vp, C.c_uint64, _errp]),
    "srt_udpsend_run": (C.c_int, [_vp, _vp, _vp, C.c_uint64, C.c_uint64, C.c_uint64, _vp, _vp, _vp, _vp, _vp, C.c_uint32,
                                  _vp, _vp, C.c_uint32, _vp, _vp, _u64p, _errp]),
    "srt_udpsend_status": (C.c_int, [_vp, _u32p, _u64p, _u64p, _u64p, _u64p, _errp]),
    "srt_udpsend_state": (C.c_int, [_vp, _vp, _vp, _errp]),
    "srt_udpsend_cached_seq": (C.c_int, [_vp, _vp, _errp]),
    "srt_udpsend_window_bytes": (C.c_uint32, []),
    "srt_udpsend_destroy": (None, [_vp]),
    "srt_routing_info_build": (C.c_int, [C.POINTER(SrtCsr), _u32p, C.c_uint32, C.c_int, C.POINTER(SrtOpts),
                                         C.POINTER(_vp), _errp]),
    "srt_routing_info_from_plan": (C.c_int, [_vp, C.POINTER(_vp), _errp]),
    "srt_routing_info_path": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.POINTER(SrtPath)]),
    "srt_routing_info_increment_packet_count": (None, [_vp, C.c_uint32, C.c_uint32]),
    "srt_routing_info_add_packet_counts": (None, [_vp, _u64p]),
    "srt_routing_info_packet_count": (C.c_uint64, [_vp, C.c_uint32, C.c_uint32]),
    "srt_routing_info_smallest_latency_ns": (C.c_int, [_vp, _u64p]),
    "srt_routing_info_row": (C.c_int64, [_vp, C.c_uint32]),
    "srt_routing_info_size": (C.c_uint32, [_vp]),
    "srt_routing_info_table": (C.POINTER(SrtPath), [_vp]),
    "srt_routing_info_record_bytes": (C.c_int, [_vp]),
    "srt_routing_info_copy_table": (None, [_vp, C.POINTER(SrtPath)]),
    "srt_init": (C.c_int, [C.c_int, _errp]),
    "srt_init_async": (None, [C.c_int]),
    "srt_init_wait": (None, []),
    "srt_routing_info_destroy": (None, [_vp]),
    "srt_gml_parse": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(_vp), _errp]),
    "srt_gml_csr": (C.c_int, [_vp, C.POINTER(SrtCsr)]),
    "srt_gml_free": (None, [_vp]),
    "srt_gml_parse_file": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(_vp), _errp]),
    "srt_xz_decompress": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t),
                                    _errp]),
    "srt_free": (None, [_vp]),
    "srt_ip_assignment_create": (C.c_int, [C.POINTER(_vp)]),
    "srt_ip_assignment_destroy": (None, [_vp]),
    "srt_ip_assignment_assign_ip": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _errp]),
    "srt_ip_assignment_assign": (C.c_uint32, [_vp, C.c_uint32]),
    "srt_ip_assignment_get_node": (C.c_int, [_vp, C.c_uint32, _u32p]),
    "srt_ip_assignment_get_nodes": (C.c_uint32, [_vp, _u32p, C.c_uint32]),
    "srt_ip_assignment_size": (C.c_uint32, [_vp]),
    "srt_ip_resolver_create": (C.c_int, [_vp, _u32p, C.c_uint32, C.POINTER(_vp), _errp]),
    "srt_ip_resolver_destroy": (None, [_vp]),
    "srt_ip_resolve_rows": (C.c_int, [_vp, _u32p, C.c_uint64, C.POINTER(C.c_int32)]),
    "srt_packet_batch_ip": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, C.c_uint64, _vp, C.POINTER(SrtRound), _vp,
                                      _vp, _vp, _vp, _errp]),
    "srt_packet_status": (C.c_int, [_vp, _errp]),
    "srt_xoshiro_seed_from_u64": (None, [C.c_uint64, _u64p]),
    "srt_xoshiro_next_u64": (None, [_u64p, C.c_uint64, _u64p]),
    "srt_host_node_seed": (C.c_uint64, [C.c_uint32, C.c_char_p, C.c_size_t]),
}


def lib():
    """Load libsrt.so (raises if it was not built: there is no fallback)."""
    global _lib
    if _lib is None:
        # One HIP runtime per process: torch ships its own libamdhip64.so.7.  If
        # libsrt.so were dlopen'd first, the system copy would load and torch
        # would later bring a second runtime that finds no GPU.  Importing torch
        # first makes libsrt bind to the already-loaded runtime (same SONAME).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise SrtError(SRT_ERR_UNSUPPORTED,
                           f"{LIB_PATH} not built: run __graft_entry__.build() (make -C shadow_amd/csrc)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        if L.srt_abi_version() != 4:
            raise SrtError(SRT_ERR_UNSUPPORTED, "libsrt ABI version mismatch")
        _lib = L
    return _lib


def check(rc: int, err: SrtErr):
    if rc != SRT_OK:
        raise SrtError(rc, err.msg.decode(errors="replace"), err.a_id, err.b_id)


def init(device: int = -1) -> None:
    """srt_init: HIP runtime, kernel code objects and pinned staging, ahead of
    the first build (the cold-start work of generate_routing_info)."""
    err = SrtErr()
    check(lib().srt_init(int(device), C.byref(err)), err)


_exit_wait = []


def init_async(device: int = -1) -> None:
    """srt_init_async: the same on a library thread; the next build waits for it.

    Exit mid-init is safe in the library itself (the calling thread's exit
    joins the init thread before any static destructor runs); the package
    also waits (srt_init_wait: no device work) before the interpreter's
    finalisation, so the join never overlaps it."""
    if not _exit_wait:
        import atexit

        def _wait():
            lib().srt_init_wait()

        atexit.register(_wait)
        _exit_wait.append(_wait)
    lib().srt_init_async(int(device))


def require_device():
    n = lib().srt_device_count()
    if n <= 0:
        raise SrtError(SRT_ERR_HIP, "no HIP device visible: the routing build runs only on MI355X (gfx950)")
    return n
