"""The UDP send side's kernels in the compiler's resource report (no GPU, a
cross-compile for gfx950): the step kernel spills no more than
outbound_step_kernel of the same tree, and its LDS is the launch's request,
which is what srt_udpsend_window_bytes() documents."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shadow_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")


def report(unit):
    """-> {kernel name: dict(scratch, lds, vgprs)} from -Rpass-analysis=kernel-resource-usage, the library's flags"""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-ffp-contract=off",
           "--cuda-device-only", "-c", os.path.join(CSRC, unit), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=CSRC)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"remark:\s+Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"remark:\s+ScratchSize \[bytes/lane\]:\s+(\d+)", out.stderr)]
    lds = [int(x) for x in re.findall(r"remark:\s+LDS Size \[bytes/block\]:\s+(\d+)", out.stderr)]
    vgprs = [int(x) for x in re.findall(r"remark:\s+VGPRs:\s+(\d+)", out.stderr)]
    assert len(names) == len(scratch) == len(lds) == len(vgprs) and names
    return {n: dict(scratch=s, lds=l, vgprs=v) for n, s, l, v in zip(names, scratch, lds, vgprs)}


def pick(rep, kernel):
    hits = [v for n, v in rep.items() if kernel in n]
    assert len(hits) == 1, (kernel, list(rep))
    return hits[0]


def test_step_kernel_scratch_and_lds():
    from shadow_amd.plan import UdpSend

    us = report("srt_udpsend.hip")
    for k in ("udpsend_config_kernel", "udpsend_preset_kernel", "udpsend_step_kernel", "udpsend_cached_seq_kernel"):
        pick(us, k)
    assert len(us) == 4
    step = pick(us, "udpsend_step_kernel")
    outbound = pick(report("srt_outbound.hip"), "outbound_step_kernel")
    assert step["scratch"] <= outbound["scratch"], (step, outbound)
    assert pick(us, "udpsend_preset_kernel")["scratch"] == 0
    # the kernel declares no LDS of its own: all of it is the launch's request, LDS_BYTES, which is what
    # srt_udpsend_window_bytes returns and include/srt.h documents: 1536 * 32 + 320 * (88 + 4), two workgroups a CU
    assert step["lds"] == 0
    src = open(os.path.join(CSRC, "srt_udpsend.hip")).read()
    assert re.search(r"hipLaunchKernelGGL\(udpsend_step_kernel,[^;]*dim3\(64\), LDS_BYTES, s, c\);", src)
    assert re.search(r"srt_udpsend_window_bytes\(void\) \{ return LDS_BYTES; \}", src)
    hdr = open(os.path.join(CSRC, "srt_udpsend_step.h")).read()
    win_cap = int(re.search(r"constexpr uint32_t WIN_CAP = (\d+);", hdr).group(1))
    slot_lds = int(re.search(r"constexpr uint32_t SLOT_LDS = (\d+);", hdr).group(1))
    assert UdpSend.window_bytes() == win_cap * 32 + slot_lds * (88 + 4) == 78592
    assert 2 * UdpSend.window_bytes() <= 160 * 1024
    doc = open(os.path.join(ROOT, "include", "srt.h")).read()
    assert "78,592" in doc and "%d staged calls" % win_cap in doc.replace(",", "") and "%d slot state records" % slot_lds in doc
