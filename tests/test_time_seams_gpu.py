"""GPU parity at the u64 seams of the stages' time arithmetic (csrc/tbucket_ops.h, csrc/codel_lane.h
as compiled into tb_run, codel_run, inb_run, outb_run, rate_check / rate_apply): the inputs of
tests/time_seams.py -- the bucket fuzz, the hand cases derived from the reference's lines, CoDel
batches at both ends of the time range, a drop mode 122,626 control-law steps deep -- bit for bit
against the oracles and the models built on them, and SHD_ERR_INVALID wherever the reference panics.
tests/test_time_seams.py holds what was read in the reference and the branches no input reaches.

Safety of the inputs: every loop they drive is bounded by construction, none by a budget error.
tb_run and rate_check / rate_apply have no data-dependent loop.  CodelLane::pop's drop loop pops a
packet per pass, so the packets queued bound it (at most 131,000 here, in a ring of 131,072; a
control law that is past EMUTIME_MAX sets `bad` and the loop still ends with the queue).  In the
stages a host runs one task per event plus one per blocked packet: a blocked packet's task is at
now + d with d >= 1 and forwards it -- or d saturated and the task is at EMUTIME_MAX, which no
window here (window_end <= EMUTIME_MAX) ever runs.  No case expects kInSpin / kOutSpin.

The outbound stage runs under "fifo" and "round-robin" only: outb_run is one template whose bucket
path (tb_conforming_remove, emutime_sat_add at one site) is the same code in all four instances;
the socket disciplines differ in the queue alone.
"""
import numpy as np
import pytest

from oracle import codel as OC
from oracle import token_bucket as O
from tests import time_seams as S
from tests.inbound_model import IDLE, InboundModel
from tests.outbound_model import OutboundModel
from tests.outbound_rr_model import RrOutboundModel
from tests.rate_model import rerate
from tests.test_time_seams import SEAM_STEPS

pytestmark = pytest.mark.gpu

EMAX, SMAX, START0, L = S.EMAX, S.SMAX, S.START0, S.L
MS, SEC = 10**6, 10**9
HEADER = 52


def _invalid(fn, code="INVALID"):
    from shadow_amd._native import ShdError
    with pytest.raises(ShdError, match=code) as e:
        fn()
    return e.value


# ------------------------------------------------------------------ tb_run
def _tb_state(tbs, r):
    s = tbs.state(r)
    return s["balance"], s["last_refill"], s["pending_until"]


def test_tb_run_fuzz_clean_relays(engine):
    """All 2,953 clean relays of the fuzz in one setup and one run: every status, value and state."""
    from shadow_amd.tbucket import TokenBuckets
    F = S.bucket_fuzz()
    cap, inc, itv, last, off, time, size = S.bucket_subset(F, F.clean)
    tbs = TokenBuckets(engine, cap, inc, itv, last)
    st, val = tbs.run(off, time, size)
    assert st.tolist() == [x for r in F.clean for x in F.res[r].status]
    assert val.tolist() == [x for r in F.clean for x in F.res[r].value]
    for i, r in enumerate(F.clean):
        assert _tb_state(tbs, i) == F.res[r].state, (r, i)


@pytest.mark.parametrize("kind", ["span", "product", "sum"])
def test_tb_run_fuzz_panicking_relays(engine, kind):
    """The fuzz's panicking relays by the kind of panic (no relay panics at the second span: it
    is unreachable), each kind with two clean relays in a fresh setup: SHD_ERR_INVALID.  Then every
    one of them alone among clean relays, so that no relay of a kind hides behind another."""
    from shadow_amd.tbucket import TokenBuckets
    F = S.bucket_fuzz()
    rel = [r for r in F.panicking if F.res[r].kind == kind]
    assert rel, kind
    sub = S.bucket_subset(F, F.clean[:1] + rel + F.clean[1:2])
    tbs = TokenBuckets(engine, *sub[:4])
    _invalid(lambda: tbs.run(*sub[4:]))
    for r in rel[:40]:   # (1,024 first-span relays: the first 40; every product and sum relay)
        sub = S.bucket_subset(F, [F.clean[0], r, F.clean[1]])
        tbs = TokenBuckets(engine, *sub[:4])
        _invalid(lambda: tbs.run(*sub[4:]))


def test_tb_run_two_clean_relays_alone_are_fine(engine):
    """The two relays that accompany the panicking ones raise nothing on their own."""
    from shadow_amd.tbucket import TokenBuckets
    F = S.bucket_fuzz()
    sub = S.bucket_subset(F, F.clean[:2])
    st, _ = TokenBuckets(engine, *sub[:4]).run(*sub[4:])
    assert st.tolist() == [x for r in F.clean[:2] for x in F.res[r].status]


@pytest.mark.parametrize("case", S.BUCKET_CASES, ids=lambda c: c["name"])
def test_tb_run_hand_case(engine, case):
    from shadow_amd.tbucket import TokenBuckets
    c, i, v, l = case["bucket"]
    tbs = TokenBuckets(engine, [c], [i], [v], [l])
    times, sizes = S.bucket_case_ops(case)
    clean = [w for w in case["expect"] if w != "panic"]
    n = len(clean)
    if n:
        st, val = tbs.run([0, n], times[:n], sizes[:n])
        assert list(zip(st.tolist(), val.tolist())) == clean
    if n < len(case["expect"]):
        _invalid(lambda: tbs.run([0, 1], times[n:n + 1], sizes[n:n + 1]))
    else:
        assert _tb_state(tbs, 0) == case["state"]


# ------------------------------------------------------------------ codel_run
def _codel_states_equal(q, queues, hosts=None):
    for i, h in enumerate(range(len(queues)) if hosts is None else hosts):
        assert q.state(i) == S.codel_state(queues[h]), (i, h)


@pytest.mark.parametrize("case", S.CODEL_CASES, ids=lambda c: c["name"])
def test_codel_hand_case(engine, case):
    """State read back after each pop; interval_end and drop_next as numbers (EMUTIME_MAX =
    18446744073709551614 where the case says so); a panic is INVALID, then STATE."""
    from shadow_amd.codel import CoDelQueues
    q = CoDelQueues(engine, 1, 64)
    n_ids = 1 + max(o[2] for o in case["ops"] if o[0] == "push")
    for batch, want in zip(S.codel_case_batches(case), case["expect"]):
        arr = ([0, len(batch)], [b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch])
        if want == "panic":
            _invalid(lambda: q.run(*arr, n_ids=n_ids))
            _invalid(lambda: q.run(*arr, n_ids=n_ids), "STATE")
            return
        pop, fate = q.run(*arr, n_ids=n_ids)
        k = len(batch) - 1
        assert int(pop[k]) == (S.POP if want[0] is None else want[0])
        for d in want[1]:
            assert int(fate[d]) == (k << 2) | 2
        st = q.state(0)
        for key, v in want[2].items():
            assert st[key] == v, (key, st)


def _codel_random(engine, H, off, t, sz, pk, n_ids):
    """Oracle first: which hosts panic.  The clean hosts run in two calls (each host's ops cut in
    half, state carried on the device): pops, fates, then every state.  The panicking hosts, with
    two clean ones, in a fresh setup: INVALID."""
    from shadow_amd.codel import CoDelQueues
    bad = []
    OC.run_ops(H, off, t, sz, pk, panicked=bad)
    clean = [h for h in range(H) if h not in set(bad)]
    c_off, c_t, c_sz, c_pk = S.ops_subset(off, t, sz, pk, clean)
    q = CoDelQueues(engine, len(clean), 128)
    queues = None
    for half in (0, 1):
        idx, o = [], [0]
        for h in range(len(clean)):
            a, b = int(c_off[h]), int(c_off[h + 1])
            m = a + (b - a) // 2
            idx += list(range(a, m) if half == 0 else range(m, b))
            o.append(len(idx))
        idx = np.array(idx, np.int64)
        arr = (np.array(o, np.uint32), c_t[idx], c_sz[idx], c_pk[idx])
        queues, pop_ref, fate_ref = OC.run_ops(len(clean), *arr, queues)
        pop, fate = q.run(*arr, n_ids=n_ids)
        assert pop.tolist() == [int(x) for x in pop_ref]
        assert np.array_equal(fate, S.oracle_fate(fate_ref, n_ids))
    _codel_states_equal(q, queues)
    if bad:
        arr = S.ops_subset(off, t, sz, pk, clean[:1] + bad + clean[1:2])
        q = CoDelQueues(engine, len(bad) + 2, 128)
        _invalid(lambda: q.run(*arr, n_ids=n_ids))
    return queues, bad


def test_codel_random_batches_at_the_top_of_the_range(engine):
    """Times from EMUTIME_MAX - 2 s on: interval_end saturates within the batch (asserted on the
    oracle's final states), and drop mode entered within 100 ms of the end is the panicking part."""
    rng = np.random.default_rng(9001)
    off, t, sz, pk, n_ids = S.codel_ops(rng, 250, 60, [EMAX - 2 * SEC, EMAX - SEC, EMAX - 3 * 10**8], SEAM_STEPS)
    queues, bad = _codel_random(engine, 250, off, t, sz, pk, n_ids)
    assert bad and any(q.interval_end == EMAX for q in queues) and any(q.drop_next is not None for q in queues)


def test_codel_random_batches_with_stamps_more_than_simtime_max_old(engine):
    """Each host's first pushes are stamped at or below SIMULATION_START - 2 and everything else
    happens after EMUTIME_MAX - 1 s: those packets' standing delay is 0, not 17.5e18 ns."""
    rng = np.random.default_rng(9002)
    off, t, sz, pk, n_ids = S.codel_ops(rng, 200, 40, [0], SEAM_STEPS, first_push_before=(START0 - 2, EMAX - SEC))
    _codel_random(engine, 200, off, t, sz, pk, n_ids)


def test_codel_deep_drop_mode(engine):
    """Host 0 drops 122,626 packets in one pop, drop_next the sum of as many control-law terms
    (count 106,521, whose quotient is within 1e-6 of a half, among them); 70 more hosts leave the
    loop at counts of their own.  Every fate, pop and state."""
    from shadow_amd.codel import CoDelQueues
    D = S.deep_drop()
    assert D.queues[0].current_drop_count == 122_626 > 106_521 and len(D.queues[0]) == 8_370
    assert len({q.current_drop_count for q in D.queues}) > 20
    q = CoDelQueues(engine, D.n_hosts, S.DEEP_RING)
    pop, fate = q.run(D.off, D.time, D.size, D.pkt, n_ids=D.n_ids)
    assert np.array_equal(pop, D.pop_ref)
    assert np.array_equal(fate, D.fate_ref)
    _codel_states_equal(q, D.queues)


# ------------------------------------------------------------------ the stages
W1, W2 = L + 2 * SEC, EMAX
A60 = EMAX - 60 * MS
# host 0: blocked until EMUTIME_MAX (the conforming sum overflows u64: SIMTIME_MAX, then the
# EmulatedTime add saturates); host 1: a refill whose token product (2^63 * 2) and sum saturate;
# host 2: the 2^40-token product of 2^30 refills; host 3: an ordinary 1000 B/s bucket, blocked
# across the windows; host 4 (inbound only): a 1500-byte-per-10-ms bucket last refilled 60 ms before
# EMUTIME_MAX, so packets stand in the CoDel queue for TARGET and interval_end saturates
STAGE_BUCKETS = [(3000, 1500, 2**63, L), (S.U64, 2**63, 1000, L), (2**32 - 1, 2**40, 1, L),
                 (*O.create_token_bucket(1000), L), (1500, 1500, 10 * MS, A60)]


def test_inbound_stage_at_the_seams(engine):
    from tests.test_inbound_gpu import _arrays, _same_records, _same_state, _stage
    stage, model = _stage(engine, STAGE_BUCKETS, ring=16), InboundModel(STAGE_BUCKETS)
    w1 = [[(L, 1500, 0), (L, 1500, 1), (L, 3000, 2)],
          [(L, 10, 3), (L + 2500, 1, 4)],
          [(L, 2**31, 5), (L + 2**30, 1500, 6)],
          [(L, 1500, 7), (L, 1500, 8)], []]
    w2 = [[], [], [], [], [(A60, 1500, 10 + k) for k in range(5)]]
    for per_host, end in ((w1, W1), (w2, EMAX - 45 * MS), ([[]] * 5, EMAX)):
        arr = _arrays(per_host)
        _same_records(stage.advance(*arr, window_end=end), model.advance(*arr, end))
        for h in range(5):
            _same_state(stage.state(h), model.hosts[h])
        h0 = stage.state(0)
        assert h0["task_time"] == EMAX and h0["cached"] == (2, 3000) and h0["bucket"]["pending_until"] == EMAX
        if end == W1:
            assert stage.state(1)["bucket"]["balance"] == S.U64 - 1       # product and sum saturated
            assert stage.state(2)["bucket"]["balance"] == 2**32 - 1 - 1500
        if end == EMAX - 45 * MS:
            assert stage.state(4)["codel"]["interval_end"] == EMAX       # saturated, as a number
    # the last window ran to EMUTIME_MAX and left host 0 alone: its packet is the one still stored
    r = stage.advance(window_end=EMAX)
    assert (r.n_stored, r.next_task_time, len(r.pkt)) == (1, EMAX, 0)


IN_PANICS = {
    # the bucket's first span: SIMTIME_MAX + 1
    "bucket_span": ([(100, 10, SEC, START0 - 2)], [[(EMAX - 1, 50, 0)]], EMAX),
    # the CoDel control law before SIMULATION_START: 16 packets behind a 1500-byte-per-10-ms bucket;
    # the pop at 1000 + 110 ms finds interval_end passed with packets to spare and enters drop mode
    "codel_control_law": ([(1500, 1500, 10 * MS, 1000)], [[(1000, 1500, k) for k in range(16)]], SEC),
}


@pytest.mark.parametrize("name", list(IN_PANICS))
def test_inbound_stage_panic_is_invalid_then_state(engine, name):
    from tests.test_inbound_gpu import _arrays, _stage
    buckets, per_host, end = IN_PANICS[name]
    buckets = buckets + [(*O.create_token_bucket(1000), end - SEC)]
    arr = _arrays(per_host + [[]])
    with pytest.raises(O.ReferencePanic):
        InboundModel(buckets).advance(*arr, end)
    stage = _stage(engine, buckets, ring=32)
    _invalid(lambda: stage.advance(*arr, window_end=end))
    _invalid(lambda: stage.advance(window_end=end), "STATE")
    _invalid(lambda: stage.state(0), "STATE")
    stage = _stage(engine, buckets, ring=32)
    t = int(arr[1][0])
    r = stage.advance(*_arrays([[], [(t, 100, 7)]]), window_end=end)
    assert r.records_for(1) == [(1, 7, t)] and r.n_stored == 0 and r.next_task_time == IDLE


def _out_stage(engine, qdisc, buckets):
    from shadow_amd.outbound import OutboundStage
    cap, inc, itv, last = (np.array([b[i] for b in buckets], np.uint64) for i in range(4))
    stage = OutboundStage(engine, cap, inc, itv, last, ring_capacity=16, qdisc=qdisc, max_sockets=4)
    return stage, (OutboundModel if qdisc == "fifo" else RrOutboundModel)(buckets)


def _out_arrays(per_host, qdisc):
    """[[(time, size, pkt)] per host] -> the stage's columns: priorities in offer order under
    "fifo", one socket handle per host under "round-robin"; every packet goes to the next host."""
    from tests.test_outbound_gpu import _arrays
    n = len(per_host)
    return _arrays([[(t, (k + 1) if qdisc == "fifo" else 0x7F00_0000_1000 + h, s, max(s, HEADER) - HEADER, (h + 1) % n, p)
                     for k, (t, s, p) in enumerate(e)] for h, e in enumerate(per_host)])


@pytest.mark.parametrize("qdisc", ["fifo", "round-robin"])
def test_outbound_stage_at_the_seams(engine, qdisc):
    from tests.test_outbound_gpu import _same
    buckets = STAGE_BUCKETS[:4]
    stage, model = _out_stage(engine, qdisc, buckets)
    w1 = [[(L, 1500, 0), (L, 1500, 1), (L, 3000, 2)],
          [(L, 100, 3), (L + 2500, 60, 4)],
          [(L, 2**31, 5), (L + 2**30, 1500, 6)],
          [(L, 1500, 7), (L, 1500, 8)]]
    for per_host, end in ((w1, W1), ([[]] * 4, EMAX)):
        arr = _out_arrays(per_host, qdisc)
        _same(stage.advance(*arr, window_end=end), model.advance(*arr, end, 0))
        for h in range(4):
            st, host = stage.state(h), model.hosts[h]
            assert st["task_time"] == host.task and st["queue_len"] == len(host.q)
            assert st["cached"] == (None if host.cached is None else (host.cached[1], host.cached[2]))
            b = st["bucket"]
            assert (b["balance"], b["last_refill"], b["pending_until"]) == \
                   (host.tb.balance, host.tb.last_refill, host.task or 0)
        h0 = stage.state(0)
        assert h0["task_time"] == EMAX and h0["cached"] == (2, 3000) and h0["bucket"]["pending_until"] == EMAX
    assert stage.state(1)["bucket"]["balance"] == S.U64 - 60
    assert stage.state(2)["bucket"]["balance"] == 2**32 - 1 - 1500
    r = stage.advance(window_end=EMAX)
    assert (r.n_stored, r.next_task_time, len(r.sent_pkt)) == (1, EMAX, 0)


@pytest.mark.parametrize("qdisc", ["fifo", "round-robin"])
def test_outbound_stage_panic_is_invalid_then_state(engine, qdisc):
    """The conforming duration's product in (SIMTIME_MAX, 2^64): three refills of an interval of
    SIMTIME_MAX / 2 + 1."""
    from tests.test_outbound_gpu import _same
    buckets = [(4500, 1500, SMAX // 2 + 1, L), (*O.create_token_bucket(1000), L)]
    per_host = [[(L, 1500, 0), (L, 1500, 1), (L, 1500, 2), (L, 4500, 3)], []]
    stage, model = _out_stage(engine, qdisc, buckets)
    arr = _out_arrays(per_host, qdisc)
    with pytest.raises(O.ReferencePanic) as e:
        model.advance(*arr, W1, 0)
    assert e.value.kind == "product"
    _invalid(lambda: stage.advance(*arr, window_end=W1))
    _invalid(lambda: stage.advance(window_end=W1), "STATE")
    _invalid(lambda: stage.state(0), "STATE")
    stage, model = _out_stage(engine, qdisc, buckets)
    arr = _out_arrays([[(L, 1500, 0), (L, 1500, 1), (L, 1500, 2)], []], qdisc)
    _same(stage.advance(*arr, window_end=W1), model.advance(*arr, W1, 0))


# ------------------------------------------------------------------ re-rating at the seam
AT = EMAX - 1
# host 1's last_refill is SIMTIME_MAX + 1 before AT; hosts 0 and 2 are fine at AT
RATE_BUCKETS = [(100, 10, MS, 2**63), (100, 10, MS, START0 - 2), (100, 10, MS, EMAX - 5)]
NEW = (1501, 1, MS)


def _rate_targets(engine):
    """(name, stage, state(h) -> comparable) for the three update entry points (outbound twice)."""
    from shadow_amd.tbucket import TokenBuckets
    from tests.test_inbound_gpu import _stage as in_stage
    cols = [np.array([b[i] for b in RATE_BUCKETS], np.uint64) for i in range(4)]
    yield "tb", TokenBuckets(engine, *cols), lambda st, h: st.state(h)
    yield "inbound", in_stage(engine, RATE_BUCKETS, ring=8), lambda st, h: st.state(h)
    for qdisc in ("fifo", "round-robin"):
        yield qdisc, _out_stage(engine, qdisc, RATE_BUCKETS)[0], lambda st, h: st.state(h)


def test_rerate_more_than_simtime_max_past_a_last_refill_is_refused(engine):
    """shd_tb_update, shd_inbound_update_buckets, shd_outbound_update_buckets at AT: host 1's
    refill span is SIMTIME_MAX + 1.  The call names it and changes no host -- all read back; the
    same call without host 1 goes through and matches the model."""
    for name, stage, state in _rate_targets(engine):
        before = [state(stage, h) for h in range(3)]
        with pytest.raises(O.ReferencePanic):
            rerate(O.TokenBucket(*RATE_BUCKETS[1]), AT, *NEW)
        e = _invalid(lambda: stage.update_buckets([0, 1, 2], *NEW, AT))
        assert e.host == 1, name
        e = _invalid(lambda: stage.update_buckets([2, 1], 0, 0, 0, AT))   # also on the way to no bucket
        assert e.host == 1, name
        assert [state(stage, h) for h in range(3)] == before, name
        stage.update_buckets([0, 2], *NEW, AT)
        for h in (0, 2):
            want = rerate(O.TokenBucket(*RATE_BUCKETS[h]), AT, *NEW)
            st = state(stage, h)
            b = st if name == "tb" else st["bucket"]
            assert (b["capacity"], b["balance"], b["refill_increment"], b["refill_interval"], b["last_refill"]) == \
                   (want.capacity, want.balance, want.refill_increment, want.refill_interval, want.last_refill), name
        assert state(stage, 1) == before[1], name


def test_rerate_whose_refill_saturates_the_token_sum(engine):
    """(2^64 - 11) + 2^63 tokens saturate to 2^64 - 1 and the new capacity 2^63 + 5 clamps that; a
    wrapping sum would leave 2^63 - 12.  And 2^30 refills of 2^40 tokens into an empty bucket: the
    new capacity 2^33, not the wrapped product's 0."""
    from shadow_amd.tbucket import TokenBuckets
    rows = [(S.U64, 2**63, 1000, L), (2**32 - 1, 2**40, 1, L)]
    tbs = TokenBuckets(engine, *(np.array([r[i] for r in rows], np.uint64) for i in range(4)))
    buckets = [O.TokenBucket(*r) for r in rows]
    arr = ([0, 1, 2], [L, L], [10, 2**32 - 1])
    st, val = tbs.run(*arr)
    assert (st.tolist(), val.tolist()) == tuple(O.relay_run(buckets, [0, 0], *arr, [0, 0]))
    tbs.update_buckets([0], 2**63 + 5, 7, MS, L + 1000)
    tbs.update_buckets([1], 2**33, 7, MS, L + 2**30)
    # (relay 1's refill is clamped to the old capacity 2^32 - 1 first, which is below the new one)
    for r, (at, new, balance) in enumerate(((L + 1000, (2**63 + 5, 7, MS), 2**63 + 5),
                                            (L + 2**30, (2**33, 7, MS), 2**32 - 1))):
        want = rerate(buckets[r], at, *new)
        s = tbs.state(r)
        assert (s["capacity"], s["balance"], s["last_refill"]) == (want.capacity, want.balance, at) == (new[0], balance, at)


def test_values_outside_the_time_types_are_refused_everywhere(engine):
    """A refill interval above SIMTIME_MAX and a last_refill above EMUTIME_MAX are no values of the
    reference's types: every setup and every update entry point refuses them before anything runs;
    the largest values of the types are accepted."""
    from shadow_amd.inbound import InboundStage
    from shadow_amd.outbound import OutboundStage
    from shadow_amd.tbucket import TokenBuckets
    u = lambda *a: np.array(a, np.uint64)   # noqa: E731
    setups = [lambda *r: TokenBuckets(engine, *r), lambda *r: InboundStage(engine, *r, ring_capacity=4)]
    setups += [lambda *r, q=q: OutboundStage(engine, *r, ring_capacity=4, qdisc=q, max_sockets=2)
               for q in ("fifo", "round-robin", "fifo-sockets", "round-robin-sockets")]
    for make in setups:
        for itv, last in ((SMAX + 1, L), (S.U64, L), (MS, EMAX + 1)):
            with pytest.raises(ValueError):
                O.TokenBucket(100, 10, itv, last)
            _invalid(lambda: make(u(100, 100), u(10, 10), u(MS, itv), u(L, last)))
        stage = make(u(100, 100, 0), u(10, 10, 0), u(MS, SMAX, 0), u(L, EMAX, S.U64))   # (no bucket: last_refill unread)
        before = [stage.state(h) for h in range(3)]
        assert _invalid(lambda: stage.update_buckets([0, 1], 100, 10, u(MS, SMAX + 1), L + 5)).host is None
        assert _invalid(lambda: stage.update_buckets([0], 100, 10, MS, S.U64)).host is None
        assert [stage.state(h) for h in range(3)] == before
        stage.update_buckets([0], 100, 10, SMAX, L + 5)
        b = stage.state(0)
        assert (b if "refill_interval" in b else b["bucket"])["refill_interval"] == SMAX
