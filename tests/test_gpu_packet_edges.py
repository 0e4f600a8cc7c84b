"""srt_packet_batch at round_kernel's constants (HB hosts a workgroup, RT*KP
packets a block before the tail loops, DCAP draws in LDS, the exact re-walk),
at losses of exactly 0 and 1 and at the decision's exact equalities.  Every
round is bit-equal to O.packet_batch on the oracle's own table: flags, deliver
times, RNG states after the round, counters and both stats (the checker is
packet_cases.run_round, the pattern of test_gpu_packet._run);
tests/test_packet_cases_cpu.py proves that each case reaches its branch."""
import numpy as np
import pytest

import packet_cases as P
from oracle import oracle as O
from shadow_amd import NetworkGraph, synth
from shadow_amd.plan import RoutingPlan
from test_gpu_packet import _ip_packets

pytestmark = pytest.mark.gpu


def _new_plan():
    src, dst, lat, loss = P.extremes_graph(P.N_ROWS, P.GRAPH_SEED)
    g = NetworkGraph.from_edges(P.N_ROWS, src, dst, lat, loss)
    return RoutingPlan(g, np.arange(P.N_ROWS, dtype=np.uint32)).run()


@pytest.fixture(scope="module")
def table():
    return P.extremes_table()


@pytest.fixture(scope="module")
def plan(table):
    """One plan for the module; its table is bit-equal to the oracle's, the
    exact 0.0 and 1.0 losses included."""
    plan = _new_plan()
    got = plan.fetch()
    assert np.array_equal(got.latency_ns, table[0])
    assert np.array_equal(got.packet_loss.view(np.uint32), table[1].view(np.uint32))
    yield plan
    plan.close()


def _by_address(case):
    ia, pki = _ip_packets(case.pk, case.host_row, case.n_hosts, 1, scattered=False)
    return ia.resolver(np.arange(P.N_ROWS, dtype=np.uint32)), pki


def test_extreme_losses(plan, table):
    case = P.case_extremes()
    out = P.run_round(plan, table, case)
    bits = table[1].view(np.uint32)[case.pk["src_row"], case.pk["dst_row"]]
    pay, late = case.pk["payload_size"] > 0, case.pk["t_ns"] >= case.bootstrap_end
    one, zero = bits == P.LOSS_ONE_BITS, bits == P.LOSS_ZERO_BITS
    assert (one & pay & late).sum() > 1000 and (out.flags[one & pay & late] == O.PDS_INET_DROPPED).all()
    assert (one & ~pay).sum() > 10 and (out.flags[one & ~pay] == O.PDS_INET_SENT).all()
    assert zero.sum() > 100 and (out.flags[zero] == O.PDS_INET_SENT).all()


def test_extreme_losses_all_bootstrap(plan, table):
    """bootstrap_end past the round: nothing is dropped, every packet still draws."""
    case = P.case_extremes(True)
    out = P.run_round(plan, table, case)
    assert (out.flags == O.PDS_INET_SENT).all()
    before = synth.host_rng_states(case.n_hosts, general_seed=1)
    for h in (0, 199):
        s = before[h].copy()
        for _ in range(int(case.host_ptr[h + 1]) - int(case.host_ptr[h])):
            O.xoshiro_next(s)
        assert np.array_equal(out.rng[h], s)


@pytest.mark.parametrize("by", ["row", "address"])
def test_completed_packets_with_draws_in_scratch(plan, table, by):
    case = P.case_scratch_completed()
    out = P.run_round(plan, table, case, by_ip=_by_address(case) if by == "address" else None)
    assert (out.flags == O.PDS_NONE).sum() == 36_126 and (out.flags == O.PDS_INET_SENT).sum() == 12_889


@pytest.mark.parametrize("last_block,empty_block", [(P.DCAP, False), (P.DCAP + 1, False), (P.DCAP + 1, True)])
def test_block_totals_at_the_constants(plan, table, last_block, empty_block):
    case = P.case_block_totals(last_block, empty_block)
    out = P.run_round(plan, table, case)
    assert (out.flags == O.PDS_NONE).sum() == int(case.host_ptr[P.ALL_DONE_HOST + 1] - case.host_ptr[P.ALL_DONE_HOST]) + 2
    for pin in case.tail_pins:
        assert out.flags[P.pin_index(case.host_ptr, pin)] == O.PDS_NONE


def test_exact_equalities(plan, table):
    case = P.case_equalities()
    out = P.run_round(plan, table, case)
    got = {pin["name"]: (int(out.flags[p]), int(out.deliver[p]))
           for pin in case.pins for p in [P.pin_index(case.host_ptr, pin)]}
    assert got["t == sim_end"] == (O.PDS_NONE, 0)
    assert got["t == sim_end - 1"][0] != O.PDS_NONE
    assert got["t == bootstrap_end"] == (O.PDS_INET_DROPPED, 0)
    assert got["t == bootstrap_end - 1"][0] == O.PDS_INET_SENT
    assert got["t + delay == round_end"] == (O.PDS_INET_SENT, case.round_end)
    assert got["t + delay == round_end - 1"] == (O.PDS_INET_SENT, case.round_end)


def test_round_that_sends_nothing(plan, table):
    case = P.case_sends_nothing()
    out = P.run_round(plan, table, case)
    assert (out.flags == O.PDS_INET_DROPPED).all() and (out.deliver == 0).all()
    assert out.oracle_stats == (int(P.U64_MAX), int(P.U64_MAX))
    assert (out.stats == P.U64_MAX).all()  # initialised to -1, left untouched
    assert not out.counters.any()
    kept = P.run_round(plan, table, case, stats_init=(7, 9))
    assert kept.stats.tolist() == [7, 9]


def test_stats_are_min_combined(plan, table):
    """stats pre-set below every value of a round that does send: kept."""
    case = P.case_equalities()
    out = P.run_round(plan, table, case, stats_init=(1, 2))
    assert out.oracle_stats[0] > 1 and out.oracle_stats[1] > 2
    assert out.stats.tolist() == [1, 2]
    # and one field each way: min latency from the round, next event time from the caller
    out = P.run_round(plan, table, case, stats_init=(int(P.U64_MAX), 2))
    assert out.stats.tolist() == [out.oracle_stats[0], 2]


def test_two_rounds_on_one_plan(table):
    """A small round, then one that overflows its LDS, on a fresh plan: the
    draws scratch grows between them; the RNG states carry over."""
    first, second = P.case_two_rounds()
    plan = _new_plan()
    try:
        a = P.run_round(plan, table, first)
        b = P.run_round(plan, table, second, rng=a.rng.copy())
        assert not np.array_equal(a.rng, b.rng)
    finally:
        plan.close()


def test_unresolved_address_past_a_lanes_first_packets(plan, table):
    import torch

    from shadow_amd import _lib
    case = P.case_late_unresolved()
    res, pki = _by_address(case)
    p = P.pin_index(case.host_ptr, case.pin)
    pki = pki.copy()
    pki["dst_ip"][p] = int.from_bytes(((10 << 24) + 1).to_bytes(4, "big"), "little")  # 10.0.0.1: not assigned
    dev = torch.device("cuda:0")
    t_pk = torch.from_numpy(pki.view(np.uint8).copy()).to(dev)
    t_hp = torch.from_numpy(case.host_ptr.view(np.int32).copy()).to(dev)
    t_rng = torch.from_numpy(synth.host_rng_states(case.n_hosts, 1).view(np.int64).copy()).to(dev)
    t_f = torch.zeros(len(pki), dtype=torch.int32, device=dev)
    t_d = torch.zeros(len(pki), dtype=torch.int64, device=dev)
    plan.packet_batch_ip(res, t_pk, t_hp, t_rng, case.round_end, 0, 2**62, t_f, t_d, sync=False)
    with pytest.raises(_lib.SrtError, match="no node in the routing table"):
        plan.packet_status()
    # the same batch with that packet completed (t >= sim_end): not looked up, and every bit as the oracle's
    out = P.run_round(plan, table, case, by_ip=(res, pki), sim_end=case.t_bad)
    assert np.nonzero(out.flags == O.PDS_NONE)[0].tolist() == [p]
