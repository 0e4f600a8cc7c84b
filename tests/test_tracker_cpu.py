"""Tracker stage (srt_tracker: the heartbeat byte counters of the internet
interface, per host and per socket slot) without a GPU: the host-only instance
-- the same step the device kernels compile -- against the plain-Python model
on the seven-window scenarios and the hand-made cases, the error paths on raw
ctypes, the counter string against hand-worked lines, the kernels' resource
report, and the step header with the outbound accessor under AddressSanitizer
and UndefinedBehaviorSanitizer (tests/asan/tracker_check.cpp, a stand-alone
program)."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import tracker_model as TM
import tracker_scenario as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEEDS_HIPCC = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC),
                                 reason="hipcc not available")


def test_scenario_exercises_every_class_and_pop_time_rule():
    """asserted on the generator and the model's output alone: an empty scenario cannot pass"""
    rules = T.assert_scenario_is_not_empty(130, T.DENSE)
    assert rules["late"] > 100 and rules["late_known"] > 10 and rules["cached"] > 10, rules
    sc = T.scenario(130, T.DENSE)
    per_host = np.diff(sc["calls"][0]["host_ptr"].astype(np.int64))
    assert per_host.max() > 64 and (per_host == 0).any() and len(sc["calls"]) == T.N_WIN == 7
    # a packet cached across a call boundary; local packets; all seven delivery lists
    assert sum(int((c["cached_seq"] != T.U64).sum()) for c in sc["calls"]) > 10
    assert sum(int((c["pkts"]["flags"] & 1).sum()) for c in sc["calls"]) > 10
    assert len(sc["rx_lists"]) == 7
    for n_hosts in (63, 64, 65):
        T.assert_scenario_is_not_empty(n_hosts, T.DENSE)
        T.assert_scenario_is_not_empty(n_hosts, T.SPARSE)


@pytest.mark.parametrize("shape", [T.DENSE, T.SPARSE])
@pytest.mark.parametrize("n_hosts", [1, 63, 64, 65, 130])
def test_host_only_equals_model(n_hosts, shape):
    beats, st = T.run_scenario(None, n_hosts, shape)
    m_beats, m_st, _ = T.model_scenario(n_hosts, shape)
    assert st == m_st and len(beats) == len(m_beats) == 4
    for k, (a, b) in enumerate(zip(beats, m_beats)):
        T.same_records(a, b, k)


@pytest.mark.parametrize("case", T.CASES, ids=[c.__name__[5:] for c in T.CASES])
def test_hand_made(case):
    case(lambda *a: T.Runner(None, *a))


def test_error_paths_and_heartbeat_selection():
    T.error_paths()


def test_counter_string_equals_hand_worked_lines():
    from shadow_amd import Tracker

    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "tracker_lines.json")))
    assert len(cases) >= 4 and any(all(v > 1 << 32 for v in c["record"].values()) for c in cases)
    for c in cases:
        assert list(c["record"]) == list(TM.FIELDS)
        rec = np.zeros(1, TM.COUNTERS)
        for f, v in c["record"].items():
            rec[f] = v
        assert Tracker.counter_string(rec) == c["line"] == TM.counter_string(c["record"]), c
    # a buffer too small: truncated, NUL-terminated, the whole length returned
    import ctypes as C

    from shadow_amd import _lib

    buf = C.create_string_buffer(b"x" * 8, 8)
    rec = np.zeros(1, TM.COUNTERS)
    assert _lib.lib().srt_tracker_counter_string(rec.ctypes.data, buf, 5) == 23 and buf.raw == b"0,0,\0xxx"


def test_records_match_the_header():
    src = open(os.path.join(ROOT, "include", "srt.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} srt_trk_counters;", src).group(1)
    assert tuple(re.findall(r"uint64_t (\w+);", body)) == TM.FIELDS
    from shadow_amd.plan import TRK_COUNTERS_DTYPE, TRK_META_DTYPE

    assert TRK_COUNTERS_DTYPE == TM.COUNTERS and TRK_META_DTYPE == TM.TRK_META and TM.COUNTERS.itemsize == 80


@NEEDS_HIPCC
def test_tracker_kernels_use_no_scratch():
    csrc = os.path.join(ROOT, "shadow_amd", "csrc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c",
           os.path.join(csrc, "srt_tracker.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=csrc)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"remark:\s+Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"remark:\s+ScratchSize \[bytes/lane\]:\s+(\d+)", out.stderr)]
    for k in ("tracker_note_kernel", "tracker_late_kernel", "tracker_tx_kernel", "tracker_rx_kernel",
              "tracker_flat_kernel", "tracker_sum_kernel"):
        assert any(k in n for n in names), (k, names)
    assert len(names) == len(scratch) >= 8
    assert not any(scratch), dict(zip(names, scratch))


@NEEDS_HIPCC
def test_step_header_under_asan_ubsan(tmp_path):
    """tests/asan/tracker_check.cpp over srt_tracker_step.h and the outbound step's accessor, host arrays
    sized exactly, built for the host with -fsanitize=address,undefined and run directly"""
    exe = str(tmp_path / "tracker_check")
    cmd = [HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-Wall", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "asan", "tracker_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "tracker_check: clean" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
