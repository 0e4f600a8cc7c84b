"""srt_packet_events at its kernels' constants: group sizes around the 64-lane
ballot step, EV_SMALL = 256 and EV_CAP = 1024; more big-list groups than the
big sort has workgroups; more than 64 chunks (the column scan's second step);
the largest chunked launch (15,872 destinations) and the first global-atomic
one.  Event ids, order, dst_ptr and advanced bases are bit-equal to the oracle.

A batch without a group over 1024 events is read after a call with
check=False and only then is srt_packet_events_status called (it must find
nothing to do): the bits compared are the LDS sorts', not the radix
fallback's.  tests/test_packet_cases_cpu.py proves the group sizes and chunk
counts of every batch used here."""
import numpy as np
import pytest

import packet_cases as P
from oracle import oracle as O
from test_packet_events import _plan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plan():
    plan = _plan()
    yield plan
    plan.close()


def _oracle(batch):
    host_ptr, flags, deliver, dst, n_dst, base = batch
    ob = base.copy()
    eid, order, ptr = O.packet_events(host_ptr, flags, deliver, dst, n_dst, ob)
    return eid, order, ptr, ob


def _check_unchecked(plan, batch, ref):
    """check=False, compare, then the status call (no fallback may be pending:
    the outputs are read again after it and must not have changed)."""
    assert P.group_sizes(batch[1], batch[3], batch[4]).max(initial=0) <= P.EV_CAP
    run = P.EventsRun(plan, batch)
    got = run.read()
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and np.array_equal(g, r)
    run.status()
    for g, r in zip(run.read(), ref):
        assert np.array_equal(g, r)


def test_size_ladder_chunked(plan):
    batch = P.events_ladder()
    _check_unchecked(plan, batch, _oracle(batch))


@pytest.mark.parametrize("n_dst", [P.EV_LDS_DST, P.EV_LDS_DST + 1])
def test_size_ladder_at_the_lds_destination_limit(plan, n_dst):
    """15,872 destinations: the largest chunked launch; 15,873: global atomics."""
    batch, _ = P.events_ladder_spread(n_dst)
    _check_unchecked(plan, batch, _oracle(batch))


def test_more_big_groups_than_workgroups_and_65_chunks(plan):
    """600 groups on the big-list sort (512 workgroups: 88 take a second group
    and reuse their LDS) in 70 chunks (the column scan's loops run twice).  The
    reference is the lexicographic statement, proved equal to the oracle's heaps
    on the ladder batches (test_packet_cases_cpu.py)."""
    batch = P.events_many_big()
    _check_unchecked(plan, batch, P.events_lexsort(*batch))


def test_group_of_1025_beside_the_ladder():
    """Its own plan: the pending big-group flag of a failed comparison must not
    reach the next test's batch."""
    plan = _plan()
    try:
        _group_of_1025(plan)
    finally:
        plan.close()


def _group_of_1025(plan):
    batch = P.events_ladder((1025,))
    eid_o, ord_o, ptr_o, base_o = _oracle(batch)
    big = len(P.LADDER)
    assert ptr_o[big + 1] - ptr_o[big] == P.EV_CAP + 1
    run = P.EventsRun(plan, batch)
    eid, order, ptr, base = run.read()
    # before the status check: everything but the one group's range is already exact
    assert np.array_equal(eid, eid_o) and np.array_equal(ptr, ptr_o) and np.array_equal(base, base_o)
    outside = np.ones(len(ord_o), bool)
    outside[ptr_o[big]:ptr_o[big + 1]] = False
    assert np.array_equal(order[outside], ord_o[outside])
    assert sorted(order[~outside].tolist()) == sorted(ord_o[~outside].tolist())
    run.status()  # redoes the batch exactly
    for g, r in zip(run.read(), (eid_o, ord_o, ptr_o, base_o)):
        assert np.array_equal(g, r)
    run.status()


def _counts_for(n_pkts, n_hosts, seed):
    return np.random.default_rng(seed).multinomial(n_pkts, np.ones(n_hosts) / n_hosts)


@pytest.mark.parametrize("n_pkts,n_hosts", [(1, 1), (1, 5), (4096, 5), (4097, 7), (4097, 1)])
def test_batch_shapes(plan, n_pkts, n_hosts):
    """One packet; one chunk exactly and one packet more; host counts that are
    no multiple of the 4 waves a workgroup of the id kernel."""
    batch = P.events_random(_counts_for(n_pkts, n_hosts, n_pkts + n_hosts), 9, n_pkts + n_hosts, p_sent=0.9)
    assert (batch[1] == O.PDS_INET_SENT).any()
    _check_unchecked(plan, batch, _oracle(batch))


def test_empty_batch(plan):
    """No packets, 5 destinations and 3 hosts: all-zero dst_ptr, bases unchanged, no error."""
    batch = P.events_random([0, 0, 0], 5, 1)
    run = P.EventsRun(plan, batch)
    eid, order, ptr, base = run.read()
    assert len(eid) == 0 and len(order) == 0 and ptr.tolist() == [0] * 6
    assert np.array_equal(base, batch[5])
    run.status()


def test_host_sizes_around_the_ballot_step(plan):
    """Hosts of exactly 0, 63, 64, 65 and 128 packets, and one whose packets
    60..70 are all SENT (its ids count across the 64-packet step)."""
    counts = [0, 63, 64, 65, 128, 200, 0]
    host_ptr, flags, deliver, dst, n_dst, base = P.events_random(counts, 6, 91, p_sent=0.6)
    b = int(host_ptr[5])
    flags[b + 60:b + 71] = O.PDS_INET_SENT
    batch = (host_ptr, flags, deliver, dst, n_dst, base)
    ref = _oracle(batch)
    assert np.array_equal(np.diff(ref[0][b + 60:b + 71].astype(np.int64)), np.ones(10, np.int64))
    _check_unchecked(plan, batch, ref)
