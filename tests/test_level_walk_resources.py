"""The level solve's register budget (CPU: hipcc cross-compiles srt_level.hip
for gfx950), from the compiler's own resource report as
tests/test_kernel_resources.py reads it: no instantiation of
level_solve_kernel spills to scratch, and the packed-row instantiations keep
the waves a SIMD that two workgroups of PACK_NT threads a CU need."""
import os
import re
import shutil

import pytest

import test_kernel_resources as KR

needs_hipcc = pytest.mark.skipif(shutil.which(KR.HIPCC) is None and not os.path.exists(KR.HIPCC),
                                 reason="hipcc not available")
_REPORT = {}


def _solve_kernels():
    """{mangled name: resources} of every level_solve_kernel instantiation, compiled once."""
    if not _REPORT:
        _REPORT.update({k: v for k, v in KR._resources("srt_level.hip").items() if "level_solve_kernel" in k})
    return _REPORT


def _pack_nt():
    with open(os.path.join(KR.CSRC, "srt_rowfold.h")) as f:
        (nt,) = re.findall(r"constexpr uint32_t PACK_NT = (\d+);", f.read())
    return int(nt)


def _is_packed(name):
    """level_solve_kernel<LPT, UNR, CLSN, VW, NT, SP, PK>: the last three template
    arguments are bools, mangled Lb0E / Lb1E; PK is the last."""
    bools = re.findall(r"Lb([01])E", name)
    assert len(bools) == 3, name
    return bools[2] == "1"


@needs_hipcc
def test_no_instantiation_uses_scratch():
    ks = _solve_kernels()
    # 3 class-table sizes x non-temporal or plain stores x pipelined or per-item walk, and the two packed ones
    assert len(ks) == 14, sorted(ks)
    assert {k: v["ScratchSize [bytes/lane]"] for k, v in ks.items() if v["ScratchSize [bytes/lane]"]} == {}


@needs_hipcc
def test_packed_instantiations_hold_two_workgroups_a_cu():
    packed = {k: v for k, v in _solve_kernels().items() if _is_packed(k)}
    assert len(packed) == 2, sorted(packed)
    # a workgroup's waves spread over the CU's 4 SIMDs; two workgroups a CU
    nt = _pack_nt()
    assert nt % 256 == 0
    need = 2 * (nt // 64) // 4
    for k, v in packed.items():
        assert v["Occupancy [waves/SIMD]"] >= need, (k, v, need)
