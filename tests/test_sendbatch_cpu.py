"""Send-batch gather (srt_sendbatch: one srt_outbound_run call's results to the
grouped srt_pkt batch of the send decision) without a GPU: the host-only
instance -- the same step the device kernels compile -- against the numpy model
and against outbound_send_order on real outbound windows, the hand-made cases
at the step's edges, and the kernels' resource report."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import outbound_model as M
import sendbatch_model as SM
import sendbatch_scenario as B

N_HOSTS = 70
QDISCS = pytest.mark.parametrize("qdisc", [M.FIFO, M.RR], ids=["fifo", "rr"])


@QDISCS
def test_scenario_exercises_the_hard_paths(qdisc):
    """asserted on the outbound windows and the model's output alone"""
    ws, n_pkts = B.windows(N_HOSTS, B.DENSE, qdisc)
    mo = B.model_windows(N_HOSTS, B.DENSE, qdisc)
    assert len(ws) == 3 and len(ws[2]["send_rank"]) == 0 and n_pkts == 100 * N_HOSTS
    assert len(ws[1]["late"]) > 100 and len(ws[2]["late"]) > 100            # late packets
    assert all(m["flags"] == 0 and m["n_sent"] > 0 for m in mo)
    per_host = np.diff(ws[0]["host_ptr"].astype(np.int64))
    assert per_host.max() > 64 and (per_host == 0).any()
    groups = np.diff(mo[2]["host_ptr"].astype(np.int64))
    assert (groups > 0).any() and (groups == 0).any()                       # late-only groups, empty groups
    for w, m in zip(ws[:2], mo[:2]):
        assert (np.diff(m["host_ptr"].astype(np.int64)) == 0).any()
        assert w["local"].any() and (w["send_rank"][w["local"]] == M.U64).all()  # local packets: no rank
    # the second window mixes, within one host's group, late packets and batch packets
    host = np.repeat(np.arange(N_HOSTS), np.diff(ws[1]["host_ptr"].astype(np.int64)))
    sent_hosts = set(host[ws[1]["send_rank"] != M.U64].tolist())
    assert sent_hosts & set(ws[1]["late"]["src_host"][ws[1]["late"]["send_rank"] != M.U64].tolist())
    assert any((lt["send_rank"] == M.U64).any() for lt in (w["late"] for w in ws))  # and a late local one


@QDISCS
def test_host_only_equals_model(qdisc):
    outs = B.run_windows(None, N_HOSTS, B.DENSE, qdisc)
    for k, (o, m) in enumerate(zip(outs, B.model_windows(N_HOSTS, B.DENSE, qdisc))):
        B.assert_same(o, m, k)


@QDISCS
def test_host_only_order_equals_outbound_send_order(qdisc):
    """the torch path this stage replaces, on CPU tensors, as a second opinion"""
    import torch

    from shadow_amd.plan import outbound_send_order

    ws, _ = B.windows(N_HOSTS, B.DENSE, qdisc)
    for w, o in zip(ws, B.run_windows(None, N_HOSTS, B.DENSE, qdisc)):
        n = len(w["send_rank"])
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int64))  # noqa: E731
        order, ptr = outbound_send_order(t(w["host_ptr"]), torch.from_numpy(w["send_rank"].view(np.int64).copy()),
                                         t(w["late"]["src_host"]), torch.from_numpy(
                                             w["late"]["send_rank"].view(np.int64).copy()))
        order = order.numpy()
        all_seq = np.concatenate([w["seq_base"] + np.arange(n, dtype=np.uint64), w["late"]["seq"]])
        assert np.array_equal(o["seq"], all_seq[order])
        assert np.array_equal(o["host_ptr"], ptr.numpy().view(np.uint32))


def test_host_only_one_packet_a_host():
    outs = B.run_windows(None, 130, B.SPARSE, M.RR)
    mo = B.model_windows(130, B.SPARSE, M.RR)
    assert sum(len(w["late"]) for w in B.windows(130, B.SPARSE, M.RR)[0]) > 5
    for k, (o, m) in enumerate(zip(outs, mo)):
        B.assert_same(o, m, k)


def test_log_too_small_is_reported_not_faulted():
    """log_cap 8 under the same windows: late packets older than the log come out as placeholders"""
    ws, _ = B.windows(N_HOSTS, B.DENSE, M.RR)
    outs = B.run_windows(None, N_HOSTS, B.DENSE, M.RR, log_cap=8)
    ref = B.model_windows(N_HOSTS, B.DENSE, M.RR)
    assert outs[1]["flags"] == SM.LOG_OVERRUN and outs[1]["untouched"]
    assert np.array_equal(outs[1]["seq"], ref[1]["seq"]) and np.array_equal(outs[1]["host_ptr"], ref[1]["host_ptr"])
    assert (outs[1]["user"] == 0xffffffff).sum() > 50


@pytest.mark.parametrize("case", B.CASES, ids=[c.__name__[5:] for c in B.CASES])
def test_hand_made(case):
    case(lambda n_hosts, log_cap: B.Runner(None, n_hosts, log_cap))


def test_error_paths_and_flags_cleared_by_status():
    B.error_paths()


# ------------------------------------------------------------- the kernels
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_sendbatch_kernels_use_no_scratch():
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "shadow_amd", "csrc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c",
           os.path.join(csrc, "srt_sendbatch.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=csrc)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"remark:\s+Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"remark:\s+ScratchSize \[bytes/lane\]:\s+(\d+)", out.stderr)]
    for k in ("sendbatch_count_kernel", "sendbatch_late_kernel", "sendbatch_scan_kernel", "sendbatch_scatter_kernel"):
        assert any(k in n for n in names), (k, names)
    assert len(names) == len(scratch) >= 6
    assert not any(scratch), dict(zip(names, scratch))
