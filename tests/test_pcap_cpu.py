"""pcap capture stage (srt_pcap: a byte stream a host, the body of the
reference's capture file) without a GPU: the plain-Python model against the
reference's unit-test vectors and the hand-worked packets, the host-only
instance -- the same step the device kernels compile, tile assembly included --
against the model on the multi-call scenarios, the capture lengths, both tie
rules, the hand-made flag cases and the tile edges, the error paths on raw
ctypes, the file side, the record layout, the kernels' resource report, and the
step header under AddressSanitizer and UndefinedBehaviorSanitizer
(tests/asan/pcap_check.cpp, a stand-alone program)."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import pcap_model as PM
import pcap_scenario as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEEDS_HIPCC = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC),
                                 reason="hipcc not available")


def test_model_reproduces_the_reference_vectors_and_the_hand_worked_packets():
    g = P.golden()
    ref = g["reference"]
    assert PM.file_header(ref["file_header"]["capture_len"]) == ref["file_header"]["bytes"]
    assert len(ref["file_header"]["bytes"]) == 24
    for k in ("write_packet", "write_packet_fmt"):
        v = ref[k]
        assert PM.write_packet(v["ts_sec"], v["ts_usec"], v["data"], v["capture_len"]) == v["bytes"]
    names = [p["name"] for p in g["packets"]]
    assert len(names) >= 6 and {"udp_with_payload", "tcp_syn_window_scale", "tcp_ack_with_data",
                                "tcp_rst_without_ack_nonzero_ack_field", "tcp_fin_ack_other_flag_bits_masked",
                                "cut_inside_the_ip_header"} <= set(names)
    for p in g["packets"]:
        assert PM.record_bytes(P.fixture_rec(p)[0], p["payload"], p["capture_len"]) == p["bytes"], p["name"]
    syn = next(p for p in g["packets"] if p["name"] == "tcp_syn_window_scale")
    assert syn["bytes"][:16].hex() == "20000000800000002c0000002c000000" and len(syn["bytes"]) == 60
    cut = next(p for p in g["packets"] if p["name"] == "cut_inside_the_ip_header")
    assert len(cut["bytes"]) - 16 < 20
    rst = next(p for p in g["packets"] if p["name"] == "tcp_rst_without_ack_nonzero_ack_field")
    assert rst["ack"] != 0 and rst["bytes"][16 + 28:16 + 32] == bytes(4)


def test_file_header_equals_the_reference_vector():
    from shadow_amd import PcapCapture

    v = P.golden()["reference"]["file_header"]
    assert PcapCapture.file_header(v["capture_len"]) == v["bytes"]
    assert PcapCapture.file_header(64) == PM.file_header(64)
    assert PcapCapture.tile_bytes() >= 64 and PcapCapture.tile_bytes() % 16 == 0


def test_scenario_holds_every_class():
    """asserted on the generator alone: an empty scenario cannot pass"""
    for n_hosts in (63, 64, 65, 130):
        P.assert_scenario_is_not_empty(n_hosts, P.DENSE)
        P.assert_scenario_is_not_empty(n_hosts, P.SPARSE)
    want, st = P.model_scenario(130, P.DENSE, 65535)
    assert st[0] == 0 and st[1] > 3000 and all(len(w) > 100000 for _, w in want)
    sc = P.scenario(130, P.DENSE)
    assert all(off[h] == off[h + 1] for off, _ in want for h in np.nonzero(~sc["enabled"])[0])


@pytest.mark.parametrize("shape", [P.DENSE, P.SPARSE])
@pytest.mark.parametrize("n_hosts", [1, 63, 64, 65, 130])
def test_host_only_equals_model(n_hosts, shape):
    """three calls in a row on one instance, so the hosts' last times carry over; d_out misaligned by 5"""
    want, w_st = P.model_scenario(n_hosts, shape, 65535)
    got, st = P.run_scenario(None, n_hosts, shape, 65535, misalign=5)
    P.same_outputs(got, want)
    assert st == w_st and st[0] == 0


@pytest.mark.parametrize("capture_len", P.CAPTURE_LENS)
def test_capture_lengths(capture_len):
    for n_hosts, shape, tx_first in ((65, P.SPARSE, False), (64, P.DENSE, True)):
        want, w_st = P.model_scenario(n_hosts, shape, capture_len, tx_first)
        got, st = P.run_scenario(None, n_hosts, shape, capture_len, tx_first)
        P.same_outputs(got, want, (n_hosts, shape))
        assert st == w_st and st[0] == 0
        for (off, data), c in zip(got, P.scenario(n_hosts, shape)["calls"]):
            for h in range(n_hosts):
                for rec in P.parse_stream(data[int(off[h]):int(off[h + 1])], capture_len):
                    assert len(rec[3]) == min(capture_len, rec[2])


def test_tie_rules_differ_and_equal_the_model():
    a, _ = P.run_scenario(None, 130, P.DENSE, 100, False)
    b, _ = P.run_scenario(None, 130, P.DENSE, 100, True)
    P.same_outputs(a, P.model_scenario(130, P.DENSE, 100, False)[0])
    P.same_outputs(b, P.model_scenario(130, P.DENSE, 100, True)[0])
    assert all(np.array_equal(x[0], y[0]) and x[1] != y[1] and len(x[1]) == len(y[1]) for x, y in zip(a, b))


@pytest.mark.parametrize("case", P.CASES, ids=[c.__name__[5:] for c in P.CASES])
def test_hand_made(case):
    case(lambda *a: P.Runner(None, *a))


@pytest.mark.parametrize("case", P.EDGES, ids=[c.__name__[5:] for c in P.EDGES])
def test_tile_edges(case):
    case(lambda *a: P.Runner(None, *a))


def test_error_paths():
    P.error_paths()


def test_files_reproduce_header_and_concatenation(tmp_path):
    """open + append over the scenario's three calls: each file is the header and the host's ranges in call
    order, parses back record by record, and a host without a path gets no file"""
    from shadow_amd import PcapCapture

    n_hosts, capture_len = 7, 100
    sc = P.scenario(n_hosts, P.DENSE)
    want, _ = P.model_scenario(n_hosts, P.DENSE, capture_len)
    paths = [None if h == 2 else str(tmp_path / f"host{h}-eth0.pcap") for h in range(n_hosts)]
    stale = tmp_path / "host0-eth0.pcap"
    stale.write_bytes(b"x" * 1000)  # truncated, as File::create does
    r = P.Runner(None, n_hosts, capture_len, sc["rec_cap"], sc["enabled"])
    try:
        r.pc.open_files(paths)
        for c in sc["calls"]:
            off, out = r.run(c["tx"], c["tx_ptr"], c["rx"], c["rx_ptr"], sc["payload"], 1 << 20, tx_idx=c["tx_idx"],
                             rx_idx=c["rx_idx"])
            r.pc.append_files(off, out)
        assert r.status() == P.model_scenario(n_hosts, P.DENSE, capture_len)[1]
    finally:
        r.close()  # closes the files
    assert sorted(os.listdir(tmp_path)) == sorted(os.path.basename(p) for p in paths if p)
    n_recs = 0
    for h, path in enumerate(paths):
        if path is None:
            continue
        data = open(path, "rb").read()
        body = b"".join(w[int(off[h]):int(off[h + 1])] for off, w in want)
        assert data == PcapCapture.file_header(capture_len) + body, h
        magic, major, minor, zone, sig, snap, link = struct.unpack_from("=IHHiIII", data, 0)
        assert (magic, major, minor, zone, sig, snap, link) == (0xA1B2C3D4, 2, 4, 0, 0, capture_len, 101)
        recs = P.parse_stream(data[24:], capture_len)
        times = [s * 10**6 + u for s, u, _, _ in recs]
        assert times == sorted(times) and all(pkt[:1] == b"\x45" for _, _, _, pkt in recs)
        assert bool(recs) == bool(sc["enabled"][h]) or not body
        n_recs += len(recs)
    assert n_recs > 100


def test_records_match_the_header():
    src = open(os.path.join(ROOT, "include", "srt.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} srt_pcap_rec;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(uint\d+_t) (\w+);", body)
    assert tuple(n for _, n in fields) == PM.FIELDS + ("reserved",)
    assert [int(t[4:-2]) // 8 for t, _ in fields] == [PM.REC[n].itemsize for _, n in fields]
    from shadow_amd.plan import PCAP_REC_DTYPE

    assert PCAP_REC_DTYPE == PM.REC and PM.REC.itemsize == 48
    assert [PM.REC.fields[n][1] for n in PM.FIELDS] == [0, 8, 16, 20, 24, 26, 28, 32, 36, 38, 40, 41, 42, 43]
    from shadow_amd import _lib

    flags = dict(re.findall(r"#define SRT_PCAP_(\w+)\s+(\d+)u", src))
    assert {k: int(v) for k, v in flags.items()} == {
        "RX_FIRST": _lib.PCAP_RX_FIRST, "TX_FIRST": _lib.PCAP_TX_FIRST, "OVERFLOW": PM.OVERFLOW,
        "BAD_PROTOCOL": PM.BAD_PROTOCOL, "BAD_LENGTH": PM.BAD_LENGTH, "BAD_PAYLOAD": PM.BAD_PAYLOAD,
        "TIME_ORDER": PM.TIME_ORDER}
    assert (_lib.PCAP_OVERFLOW, _lib.PCAP_BAD_PROTOCOL, _lib.PCAP_BAD_LENGTH, _lib.PCAP_BAD_PAYLOAD,
            _lib.PCAP_TIME_ORDER) == (1, 2, 4, 8, 16)


@NEEDS_HIPCC
def test_pcap_kernels_use_no_scratch():
    csrc = os.path.join(ROOT, "shadow_amd", "csrc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c",
           os.path.join(csrc, "srt_pcap.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=csrc)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"remark:\s+Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"remark:\s+ScratchSize \[bytes/lane\]:\s+(\d+)", out.stderr)]
    for k in ("pcap_hosts_kernel", "pcap_scan_kernel", "pcap_offsets_kernel", "pcap_write_kernel"):
        assert any(k in n for n in names), (k, names)
    assert len(names) == len(scratch) >= 6  # the hosts and offsets kernels in both widths
    assert not any(scratch), dict(zip(names, scratch))


@NEEDS_HIPCC
def test_step_header_under_asan_ubsan(tmp_path):
    """tests/asan/pcap_check.cpp over srt_pcap_step.h, host arrays sized exactly, built for the host with
    -fsanitize=address,undefined and run directly"""
    exe = str(tmp_path / "pcap_check")
    cmd = [HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-Wall", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "asan", "pcap_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "pcap_check: clean" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
