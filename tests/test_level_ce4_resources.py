"""The register budget of the 4-byte-entry packed level solve at each of its
workgroup sizes (CPU: hipcc cross-compiles srt_level.hip for gfx950), from the
compiler's own resource report as tests/test_kernel_resources.py reads it:
level_ce4_kernel<NT> runs PACK_NT threads a workgroup and
level_ce4_wide_kernel<NT, NTH, UNR> the counts of CE4_WIDE_NT; none spills to
scratch, and each keeps the waves a SIMD that two workgroups of its own thread
count a CU need -- 2 (threads / 64) / 4: four at 512, five at 640, six at 768,
which is at most 80 VGPRs."""
import os
import re

import test_kernel_resources as KR
import test_level_walk_resources as WR

_REPORT = {}


def _ce4_kernels():
    """{mangled name: resources} of every level_ce4_kernel / level_ce4_wide_kernel instantiation, compiled once."""
    if not _REPORT:
        _REPORT.update({k: v for k, v in KR._resources("srt_level.hip").items()
                        if "level_ce4_kernel" in k or "level_ce4_wide_kernel" in k})
    return _REPORT


def _source_counts():
    """(PACK_NT, the wide instantiations' thread counts), read from the source."""
    with open(os.path.join(KR.CSRC, "srt_level.hip")) as f:
        (wide,) = re.findall(r"constexpr uint32_t CE4_WIDE_NT\[\] = \{([\d, ]+)\};", f.read())
    return WR._pack_nt(), sorted(int(x) for x in wide.split(","))


def _threads(name, pack_nt):
    """The workgroup's threads of an instantiation: level_ce4_wide_kernel<NT, NTH, UNR> mangles NTH as Li<NTH>E."""
    if "level_ce4_wide_kernel" not in name:
        return pack_nt
    ints = re.findall(r"Li(\d+)E", name)
    assert len(ints) == 2, name  # NTH, UNR
    return int(ints[0])


def test_pack_nt_is_still_512():
    assert WR._pack_nt() == 512


@WR.needs_hipcc
def test_every_thread_count_is_instantiated_without_scratch():
    pack_nt, wide = _source_counts()
    assert wide == [640, 768] and all(t > pack_nt and t % 128 == 0 for t in wide)
    ks = _ce4_kernels()
    # non-temporal or plain stores x {PACK_NT, the wide counts}
    assert sorted(_threads(k, pack_nt) for k in ks) == sorted(2 * ([pack_nt] + wide)), sorted(ks)
    assert {k: v["ScratchSize [bytes/lane]"] for k, v in ks.items() if v["ScratchSize [bytes/lane]"]} == {}


@WR.needs_hipcc
def test_each_count_holds_two_workgroups_a_cu():
    pack_nt, _ = _source_counts()
    for k, v in _ce4_kernels().items():
        t = _threads(k, pack_nt)
        need = 2 * (t // 64) // 4  # a workgroup's waves spread over the CU's 4 SIMDs; two workgroups a CU
        assert (2 * (t // 64)) % 4 == 0 and v["Occupancy [waves/SIMD]"] >= need, (k, v, need)
        if t == 768:  # six waves a SIMD: 512 registers / 6, in granules of 8
            assert v["VGPRs"] <= 80, (k, v)
