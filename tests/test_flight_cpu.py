"""In-flight store (srt_flight: a round's sent packets kept until the window
their deliver time falls in) without a GPU: the host-only instance -- the same
step the device kernels compile -- against the numpy model on the scenarios and
the hand-made cases at the step's edges, the error paths on raw ctypes, the
kernels' resource report, and the step header alone under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/asan/flight_check.cpp, a stand-alone
program)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import flight_scenario as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEEDS_HIPCC = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC),
                                 reason="hipcc not available")


def test_scenario_exercises_the_hard_paths():
    """asserted on the generator and the model's output alone"""
    steps, total = F.scenario(70, F.DENSE)
    mo = F.model_scenario(70, F.DENSE)
    pushes = [a for k, a in steps if k == "push"]
    assert len(pushes) == 3 and len(mo) == 4
    per_host = np.diff(pushes[0]["host_ptr"].astype(np.int64))
    assert per_host.max() > 64 and (per_host == 0).any()
    assert all((p["flags"] != F.SENT).any() for p in pushes)
    # every pop mixes packets of different pushes (tags of a push are one run), the last one drains
    bounds = np.cumsum([0] + [len(p["flags"]) for p in pushes])
    for k, m in enumerate(mo):
        assert m["status"][0] == 0 and m["status"][1] == len(m["tag"]) > 0
        assert len(set(np.searchsorted(bounds, m["tag"], side="right").tolist())) >= 2, k
    assert mo[-1]["status"][2] == 0 and mo[0]["status"][2] > 0
    # equal deliver times inside a destination's group, across source hosts and within one
    m = mo[1]
    same_t = (np.diff(m["deliver"].astype(np.int64)) == 0) & (np.diff(np.searchsorted(m["dst_ptr"], np.arange(
        len(m["deliver"])), side="right")) == 0)
    assert (same_t & (np.diff(m["src"].astype(np.int64)) > 0)).any()
    assert (same_t & (np.diff(m["src"].astype(np.int64)) == 0)).any()
    assert (m["event_id"] > (1 << 32)).any()


@pytest.mark.parametrize("shape", [F.DENSE, F.SPARSE])
@pytest.mark.parametrize("n_hosts", [1, 70, 130])
def test_host_only_equals_model(n_hosts, shape):
    outs = F.run_scenario(None, n_hosts, shape)
    for k, (o, m) in enumerate(zip(outs, F.model_scenario(n_hosts, shape))):
        F.assert_same(o, m, k)


@pytest.mark.parametrize("case", F.CASES, ids=[c.__name__[5:] for c in F.CASES])
def test_hand_made(case):
    case(lambda n_dst, pool_cap: F.Runner(None, n_dst, pool_cap))


def test_error_paths_and_flags_cleared_by_status():
    F.error_paths()


def test_sort_capacity_constant_matches_the_kernel():
    src = open(os.path.join(ROOT, "shadow_amd", "csrc", "srt_flight.hip")).read()
    assert int(re.search(r"constexpr uint32_t FL_CAP = (\d+);", src).group(1)) == F.G


@NEEDS_HIPCC
def test_flight_kernels_use_no_scratch():
    csrc = os.path.join(ROOT, "shadow_amd", "csrc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c",
           os.path.join(csrc, "srt_flight.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=csrc)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"remark:\s+Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"remark:\s+ScratchSize \[bytes/lane\]:\s+(\d+)", out.stderr)]
    for k in ("flight_push_kernel", "flight_count_kernel", "flight_scan_kernel", "flight_move_kernel",
              "flight_sort_kernel"):
        assert any(k in n for n in names), (k, names)
    assert len(names) == len(scratch) >= 6
    assert not any(scratch), dict(zip(names, scratch))


@NEEDS_HIPCC
def test_step_header_under_asan_ubsan(tmp_path):
    """tests/asan/flight_check.cpp over srt_flight_step.h alone, host arrays sized exactly, built
    for the host with -fsanitize=address,undefined and run directly"""
    exe = str(tmp_path / "flight_check")
    cmd = [HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-Wall", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "asan", "flight_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "flight_check: clean" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
