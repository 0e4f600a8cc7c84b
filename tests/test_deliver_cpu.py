"""Interface receive stage (srt_deliver: the forwarded packets of an inbound
call, each host's in the order its interface receives them, with their sockets)
without a GPU: the host-only instance -- the same step the device kernels
compile -- against the numpy and dict model on the scenarios and the hand-made
cases at the step's edges, the error paths on raw ctypes, the host-side lookup,
the kernels' resource report, and the step header alone under AddressSanitizer
and UndefinedBehaviorSanitizer (tests/asan/deliver_check.cpp, a stand-alone
program)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import deliver_model as DM
import deliver_scenario as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEEDS_HIPCC = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC),
                                 reason="hipcc not available")


def test_scenario_exercises_the_hard_paths():
    """asserted on the generator and the model's output alone"""
    sc = D.scenario(130, D.DENSE)
    runs = [s[1] for s in sc["steps"] if s[0] == "run"]
    mo = D.model_scenario(130, D.DENSE)
    assert len(runs) == D.N_WIN + 1 == len(mo)
    per_host = np.diff(runs[0]["dst_ptr"].astype(np.int64))
    assert per_host.max() > 64 and (per_host == 0).any()
    st = np.concatenate([r["status"] for r in runs])
    late = np.concatenate([r["late"] for r in runs])
    assert ((st & DM.ROUTER_DROPPED) != 0).sum() + ((late["status"] & DM.ROUTER_DROPPED) != 0).sum() > 10  # CoDel
    assert ((late["status"] & DM.FORWARDED) != 0).sum() > 1000 and len(runs[-1]["late"]) > 0
    # late runs of one host longer than a wave; every flag clear; hits, wildcard or specific, and misses
    assert max(np.bincount(r["late"]["dst_host"], minlength=130).max() for r in runs[1:]) > 64
    assert all(m["flags"] == 0 for m in mo) and sum(m["n_delivered"] for m in mo) > 20000
    sock = np.concatenate([m["socket"] for m in mo])
    assert (sock == DM.NONE32).mean() > 0.1 and (sock != DM.NONE32).mean() > 0.1
    assert any(s[0] == "disassoc" and len(s[1]) > 2 for s in sc["steps"])


@pytest.mark.parametrize("shape", [D.DENSE, D.SPARSE])
@pytest.mark.parametrize("n_hosts", [1, 63, 64, 65, 130])
def test_host_only_equals_model(n_hosts, shape):
    outs = D.run_scenario(None, n_hosts, shape)
    for k, (o, m) in enumerate(zip(outs, D.model_scenario(n_hosts, shape))):
        D.assert_same(o, m, k)


@pytest.mark.parametrize("case", D.CASES, ids=[c.__name__[5:] for c in D.CASES])
def test_hand_made(case):
    case(lambda *a: D.Runner(None, *a))


def test_error_paths_and_flags_cleared_by_status():
    D.error_paths()


def test_lookup_equals_model():
    """srt_deliver_lookup against the model's two dict lookups, on the scenario's first table and after
    its first round of removals and additions"""
    n_hosts = 65
    sc = D.scenario(n_hosts, D.SPARSE)
    r, m = D.Runner(None, n_hosts, 8, 0, 0), DM.DeliverModel(n_hosts, 0, 0)
    rng = np.random.default_rng(9)
    try:
        for st in [s for s in sc["steps"] if s[0] in ("assoc", "disassoc")][:3]:
            for obj in (r, m):
                obj.associate(st[1]) if st[0] == "assoc" else obj.disassociate(st[1])
            hosts, metas = rng.integers(0, n_hosts, size=4000).astype(np.uint32), D.rand_meta(rng, 4000)
            got, want = r.lookup(hosts, metas), m.lookup(hosts, metas)
            assert np.array_equal(got, want) and (got != DM.NONE32).sum() > 400 and (got == DM.NONE32).sum() > 400
            n, slots, _, _ = r.ds.table_stats()
            assert n == len(m.assoc) and 2 * n <= slots and slots & (slots - 1) == 0
    finally:
        r.close()


def test_sort_capacity_constant_matches_the_step():
    src = open(os.path.join(ROOT, "shadow_amd", "csrc", "srt_deliver_step.h")).read()
    assert int(re.search(r"constexpr uint32_t SORT_CAP = (\d+);", src).group(1)) == D.G
    flight = open(os.path.join(ROOT, "shadow_amd", "csrc", "srt_flight.hip")).read()
    assert int(re.search(r"constexpr uint32_t FL_CAP = (\d+);", flight).group(1)) == D.G  # the same cap


@NEEDS_HIPCC
def test_deliver_kernels_use_no_scratch():
    csrc = os.path.join(ROOT, "shadow_amd", "csrc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c",
           os.path.join(csrc, "srt_deliver.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=csrc)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"remark:\s+Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"remark:\s+ScratchSize \[bytes/lane\]:\s+(\d+)", out.stderr)]
    for k in ("deliver_note_kernel", "deliver_count_kernel", "deliver_late_kernel", "deliver_scan_kernel",
              "deliver_scatter_kernel", "deliver_order_kernel", "deliver_sum_kernel"):
        assert any(k in n for n in names), (k, names)
    assert len(names) == len(scratch) >= 9
    assert not any(scratch), dict(zip(names, scratch))


@NEEDS_HIPCC
def test_step_header_under_asan_ubsan(tmp_path):
    """tests/asan/deliver_check.cpp over srt_deliver_step.h alone, host arrays sized exactly, built
    for the host with -fsanitize=address,undefined and run directly"""
    exe = str(tmp_path / "deliver_check")
    cmd = [HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-Wall", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "asan", "deliver_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "deliver_check: clean" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
