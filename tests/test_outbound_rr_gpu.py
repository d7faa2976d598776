"""GPU parity of the outbound stage under interface_qdisc: round-robin (shd_outbound_setup_qdisc,
csrc/outbound.hip's round-robin instance over csrc/rr_queue.h) against the CPU model
(tests/outbound_rr_model.py): the batch arrays, sent_pkt, the local CSR, the stored total, the
next task time, the per-host state and the rrQueue's listing, exactly."""
import numpy as np
import pytest

from oracle.token_bucket import SIM_START as S
from tests.outbound_rr_model import IDLE, LOCAL, SENT, RrOutboundModel
from tests.test_outbound import MS, arrays, bucket, check_final
from tests.test_outbound_gpu import HEADER, KEYS, ChainOracle, _arrays, _same, chain_case
from tests.test_outbound_rr import (A, B, GEN_CAPACITY, GEN_MAX_SOCKETS, GEN_SEEDS, RR_CASES, np_arrays,
                                    random_setup, random_window, run_seed)

pytestmark = pytest.mark.gpu


def _stage(engine, buckets, first_host=0, ring=64, max_sockets=8, qdisc="round-robin"):
    from shadow_amd.outbound import OutboundStage
    rows = [(0, 0, 0, S) if b is None else b for b in buckets]
    cap, inc, itv, last = (np.array([r[i] for r in rows], np.uint64) for i in range(4))
    return OutboundStage(engine, cap, inc, itv, last, first_host=first_host, ring_capacity=ring, qdisc=qdisc,
                         max_sockets=max_sockets)


def _same_state(stage, h, host):
    st = stage.state(h)
    assert st["task_time"] == host.task
    assert st["cached"] == (None if host.cached is None else (host.cached[1], host.cached[2]))
    assert st["queue_len"] == len(host.q)
    assert st["head_pkt"] == host.q.head_pkt()
    assert stage.sockets(h) == host.q.listing()
    if host.tb is None:
        assert st["bucket"] is None
    else:
        b = st["bucket"]
        assert (b["capacity"], b["balance"], b["refill_increment"], b["refill_interval"], b["last_refill"]) == \
               (host.tb.capacity, host.tb.balance, host.tb.refill_increment, host.tb.refill_interval,
                host.tb.last_refill)
        assert b["pending_until"] == (host.task or 0)


@pytest.mark.parametrize("name", list(RR_CASES))
def test_hand_cases_on_device(engine, name):
    b, first, steps, final = RR_CASES[name]
    stage = _stage(engine, [b], first)
    model = RrOutboundModel([b], first)
    for offers, w_end, boot, recs, n_stored, nxt, socks in steps:
        cols = arrays([[(S + t, hd, s, d, p) for t, hd, s, d, p in offers]])
        arr = [np.array(c, np.uint64 if i in (1, 2) else np.uint32) for i, c in enumerate(cols)]
        r = stage.advance(arr[0], arr[1], None, *arr[3:], sock=arr[2], window_end=S + w_end, bootstrap_end=boot)
        got = [(SENT, p, t - S) for p, t, _, _ in r.sent_for(0)] + [(LOCAL, p, t - S) for p, t in r.local_for(0)]
        assert got == recs
        assert (r.n_stored, r.next_task_time) == (n_stored, IDLE if nxt is None else S + nxt)
        assert stage.sockets(0) == socks
        _same(r, model.advance(*arr, S + w_end, boot))
        _same_state(stage, 0, model.hosts[0])
    st = stage.state(0)
    check_final(final, None if st["task_time"] is None else st["task_time"] - S,
                None if st["cached"] is None else st["cached"][0],
                None if st["bucket"] is None else st["bucket"]["balance"], st["queue_len"])
    # (what a stage that ran FIFO would get wrong; the one case with a single packet per socket aside)
    assert model.counters["not_in_offer_order"] > 0 or name == "task_at_window_end_is_carried"


def test_prio_and_sock_are_one_column(engine):
    stage = _stage(engine, [bucket()])
    with pytest.raises(ValueError):
        stage.advance(*_arrays([[(S, A, 100, 48, 1, 0)]]), sock=np.array([A], np.uint64), window_end=S + 10)
    with pytest.raises(ValueError):
        _stage(engine, [bucket()], qdisc="rr")


@pytest.mark.parametrize("seed", GEN_SEEDS)
def test_random_windows_vs_model(engine, seed):
    """Five consecutive windows over 30-298 hosts with 1-6 sockets each, mixed buckets,
    bootstrap_end inside the second window, 64 slots a host (reused: tests/test_outbound_rr.py
    holds the generator to that): every array of every window, every host's state and rrQueue
    after every window.  A stage that ran FIFO differs: every seed pops out of offer order."""
    _, n_hosts, buckets, _, _ = random_setup(seed)
    stage = _stage(engine, buckets, ring=GEN_CAPACITY, max_sockets=GEN_MAX_SOCKETS)

    def each_window(arr, end, boot, want, model):
        _same(stage.advance(*arr, window_end=end, bootstrap_end=boot), want)
        for h in range(n_hosts):
            _same_state(stage, h, model.hosts[h])
    model = run_seed(seed, each_window)
    assert model.counters["not_in_offer_order"] > 0 and model.counters["blocked_rotated"] > 0
    assert model.max_depth <= GEN_CAPACITY and model.max_sockets <= GEN_MAX_SOCKETS


def test_many_hosts_past_one_scan_tile_and_nonzero_first_host(engine):
    """9001 hosts with first_host = 4500: more than one 8192-entry tile in all three scans; two
    windows, a quarter of the hosts blocked across them, local packets by global id."""
    rng = np.random.default_rng(178)
    n_hosts, first = 9001, 4500
    buckets = [bucket(1000) if h % 4 == 0 else (None if h % 4 == 1 else bucket(125_000)) for h in range(n_hosts)]
    socks = [[(h << 8) | k for k in range(1 + h % 3)] for h in range(n_hosts)]
    stage = _stage(engine, buckets, first_host=first, ring=8, max_sockets=3)
    model = RrOutboundModel(buckets, first)
    start, pid = S, 0
    for win in (20 * MS, 4000 * MS):
        per_host, pid = random_window(rng, model, socks, start, start + 20 * MS, pid, capacity=8, max_offers=3,
                                      n_dst=first + n_hosts)
        arr = np_arrays(per_host)
        want = model.advance(*arr, start + win, 0)
        _same(stage.advance(*arr, window_end=start + win), want)
        assert want["src_off"][-1] > 8192 and want["loc_off"][-1] > 500
        for h in range(0, n_hosts, 7):
            _same_state(stage, h, model.hosts[h])
        start += win
    assert model.counters["blocks"] > 500 and model.counters["carried"] > 500
    assert model.counters["not_in_offer_order"] > 0


def test_one_socket_per_host_is_fifo(engine):
    """Device against device: one socket per host and ascending priorities -- the same offers
    through a FIFO stage and through a round-robin stage whose handle column is a constant give
    identical batches, window after window."""
    from tests.test_outbound_gpu import RATES, _random_window
    from tests.outbound_model import OutboundModel
    from oracle.token_bucket import create_token_bucket
    rng = np.random.default_rng(31)
    n_hosts = 130
    buckets = [None if rng.random() < 0.1 else (*create_token_bucket(int(rng.choice(RATES))), S)
               for _ in range(n_hosts)]
    fifo = _stage(engine, buckets, ring=512, qdisc="fifo")
    model = OutboundModel(buckets)   # (steers the generator's tie offers only)
    start, pid, prio = S, 0, [0] * n_hosts
    outs = []
    for end in (S + 20 * MS, S + 170 * MS, S + 171 * MS):
        per_host, pid = _random_window(rng, model, start, end, pid, prio)
        # (the generator trades some neighbours' priorities: put each host's back in arrival order)
        per_host = [[(x[0], pr, *x[2:]) for x, pr in zip(o, sorted(y[1] for y in o))] for o in per_host]
        arr = _arrays(per_host)
        model.advance(*arr, end, 0)
        outs.append((arr, end, fifo.advance(*arr, window_end=end)))
        start = end
    rr = _stage(engine, buckets, ring=512, max_sockets=1)
    n_sent = 0
    for arr, end, want in outs:
        got = rr.advance(arr[0], arr[1], np.full(len(arr[1]), 77, np.uint64), *arr[3:], window_end=end)
        for k in KEYS:
            assert np.array_equal(getattr(got, k), getattr(want, k)), k
        assert (got.n_stored, got.next_task_time) == (want.n_stored, want.next_task_time)
        n_sent += len(want.sent_pkt)
    assert n_sent > 1000 and outs[-1][2].n_stored > 100   # queues were standing


_P = lambda t, hd, pkt, size=100, dst=1: (t, hd, size, size - HEADER, dst, pkt)  # noqa: E731
# (buckets, capacity, max_sockets, [(per_host offers, window_end)]): the last step violates the contract
BAD = {
    # capacity 4: p1 is cached behind p0 (it is not queued), then five offers before its task runs
    "capacity_plus_one_packets": ([bucket()], 4, 4, [([[_P(S, A, 0, 1500), _P(S, A, 1, 1500)]], S + 10),
                                                     ([[_P(S + 20 + i, A, 2 + i) for i in range(5)]], S + 100)]),
    # max_sockets 3: three sockets queued behind the cached p1, the fourth is one too many
    "max_sockets_plus_one_sockets": ([bucket()], 16, 3, [([[_P(S, A, 0, 1500), _P(S, A, 1, 1500)]], S + 10),
                                                         ([[_P(S + 20 + i, 50 + i, 2 + i) for i in range(4)]], S + 100)]),
    "decreasing_time": ([bucket()], 4, 2, [([[_P(S + 5, A, 0), _P(S + 4, A, 1)]], S + 10)]),
    "offer_at_window_end": ([bucket()], 4, 2, [([[_P(S + 10, A, 0)]], S + 10)]),
    "pkt_id_uint32_max": ([bucket()], 4, 2, [([[_P(S + 5, A, 2**32 - 1)]], S + 10)]),
    "size_above_capacity": ([bucket()], 4, 2, [([[_P(S + 5, A, 0, 1502)]], S + 10)]),
}


@pytest.mark.parametrize("name", list(BAD))
def test_contract_errors(engine, name):
    """Each violation is SHD_ERR_INVALID from a check in the kernel, every later call
    SHD_ERR_STATE, and a fresh setup works again.  One packet and one socket fewer are taken."""
    from shadow_amd._native import ShdError
    buckets, ring, ms, steps = BAD[name]
    if name.endswith("_packets") or name.endswith("_sockets"):   # the same steps, the last offer left out: fine
        stage = _stage(engine, buckets, ring=ring, max_sockets=ms)
        for per_host, w_end in steps[:-1]:
            stage.advance(*np_arrays(per_host), window_end=w_end)
        r = stage.advance(*np_arrays([steps[-1][0][0][:-1]]), window_end=steps[-1][1])
        assert r.n_stored == len(steps[-1][0][0])   # the cached packet + the queue, full to the brim
        assert len(stage.sockets(0)) == (1 if name.endswith("_packets") else ms)
    stage = _stage(engine, buckets, ring=ring, max_sockets=ms)
    for per_host, w_end in steps[:-1]:
        stage.advance(*np_arrays(per_host), window_end=w_end)
    per_host, w_end = steps[-1]
    with pytest.raises(ShdError, match="INVALID"):
        stage.advance(*np_arrays(per_host), window_end=w_end)
    with pytest.raises(ShdError, match="STATE"):
        stage.advance(window_end=w_end + 10)
    with pytest.raises(ShdError, match="STATE"):
        stage.state(0)
    with pytest.raises(ShdError, match="STATE"):
        stage.sockets(0)
    stage = _stage(engine, buckets, ring=ring, max_sockets=ms)
    r = stage.advance(*np_arrays([[_P(S + 61, B, 7)]]), window_end=S + 70)
    assert r.sent_for(0) == [(7, S + 61, 1, 48)] and r.n_stored == 0 and r.next_task_time == IDLE


def test_setup_and_argument_errors_leave_the_stage_as_it_was(engine):
    """qdisc = 2 and max_sockets = 0 are refused at the setup and the stage set up before goes on;
    so do a NULL array with offers and a window_end below the previous one.  A FIFO stage has no
    rrQueue to list: SHD_ERR_STATE; a host past the last: SHD_ERR_INVALID."""
    import ctypes as C
    import torch
    from shadow_amd import _native as N
    from shadow_amd._native import ShdError
    stage = _stage(engine, [bucket()])
    # p0 leaves; B gives p2, which blocks, and stands behind A again: [A(p1), B(p3)]
    stage.advance(*np_arrays([[_P(S, A, 0, 1500), _P(S, A, 1), _P(S, B, 2, 1500), _P(S, B, 3)]]), window_end=S + 10)
    one = np.array([1501, 1, MS, S], np.uint64)
    p = [N.ptr(one[i:i + 1]) for i in range(4)]
    lib, ctx = engine.lib, engine.ctx
    assert N.STATUS_NAMES[lib.shd_outbound_setup_qdisc(ctx, 1, 0, 4, 2, 4, *p)] == "INVALID"
    assert N.STATUS_NAMES[lib.shd_outbound_setup_qdisc(ctx, 1, 0, 4, N.QDISC_ROUND_ROBIN, 0, *p)] == "INVALID"
    assert N.STATUS_NAMES[lib.shd_outbound_setup_qdisc(ctx, 1, 0, 0, N.QDISC_ROUND_ROBIN, 4, *p)] == "INVALID"
    with pytest.raises(ShdError, match="INVALID"):
        stage.advance(window_end=S + 9)
    d = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(ShdError, match="INVALID"):
        stage.advance_device(d, d, None, d, d, d, d, 1, S + 20)
    with pytest.raises(ShdError, match="INVALID"):
        stage.sockets(1)
    assert stage.sockets(0) == [(A, 1), (B, 1)] and stage.state(0)["cached"] == (2, 1500)   # untouched
    n = C.c_uint32(9)
    assert lib.shd_outbound_get_sockets(ctx, 0, None, None, 0, C.byref(n)) == 0 and n.value == 2
    hd, cn = np.zeros(1, np.uint64), np.zeros(1, np.uint32)   # room for one entry: one is written
    assert lib.shd_outbound_get_sockets(ctx, 0, N.ptr(hd), N.ptr(cn), 1, C.byref(n)) == 0
    assert (hd[0], cn[0], n.value) == (A, 1, 2)
    # max_sockets is ignored under FIFO, and shd_outbound_setup still means FIFO
    assert lib.shd_outbound_setup_qdisc(ctx, 1, 0, 4, N.QDISC_FIFO, 0, *p) == 0
    assert N.STATUS_NAMES[lib.shd_outbound_get_sockets(ctx, 0, None, None, 0, C.byref(n))] == "STATE"
    assert lib.shd_outbound_setup(ctx, 1, 0, 4, *p) == 0
    assert N.STATUS_NAMES[lib.shd_outbound_get_sockets(ctx, 0, None, None, 0, C.byref(n))] == "STATE"


@pytest.mark.parametrize("n_hosts", [1, 70])
def test_empty_and_edge_shapes(engine, n_hosts):
    """One host and a host count that is no multiple of 64: a window without offers or tasks (NULL
    inputs and empty arrays alike), then offers on two sockets that leave tasks outstanding, a call
    with every output pointer NULL that runs them, and the state after it."""
    buckets = [bucket()] * n_hosts
    stage = _stage(engine, buckets)
    model = RrOutboundModel(buckets)
    empty = (np.zeros(n_hosts + 1, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint64)) + \
        (np.zeros(0, np.uint32),) * 4
    for arr in (None, empty):
        r = stage.advance(*(arr or ()), window_end=S + 5)
        assert len(r.sent_pkt) == len(r.loc_pkt) == 0
        assert r.src_off.tolist() == r.loc_off.tolist() == [0] * (n_hosts + 1)
        assert (r.n_stored, r.next_task_time) == (0, IDLE)
    assert stage.sockets(0) == []
    per_host = [[(S + 5 + h, A, 1500, 1448, n_hosts, 3 * h), (S + 6 + h, A, 1, 0, n_hosts, 3 * h + 1),
                 (S + 6 + h, B, 1, 0, n_hosts, 3 * h + 2)] for h in range(n_hosts)]
    arr = np_arrays(per_host)
    _same(stage.advance(*arr, window_end=S + MS), model.advance(*arr, S + MS))
    _same_state(stage, n_hosts - 1, model.hosts[n_hosts - 1])
    none = (None,) * 7
    st = engine.lib.shd_outbound_advance(engine.ctx, *none, 0, S + 3000 * MS, 0, *(None,) * 8)
    assert st == 0
    model.advance(*none, S + 3000 * MS)
    assert model.counters["carried"] == n_hosts
    for h in {0, n_hosts - 1}:
        _same_state(stage, h, model.hosts[h])
        assert stage.state(h)["task_time"] is None
    assert engine.lib.shd_outbound_get_sockets(engine.ctx, 0, None, None, 0, None) == 0
    r = stage.advance(window_end=S + 3001 * MS)
    assert len(r.sent_pkt) == 0 and r.n_stored == 0


# ---- the two-call window over a round-robin stage --------------------------------------------

def rr_chain_offers(k, ws, we, H):
    """Window 0: every host offers a burst of 3-7 packets at one instant in the window's last two
    thirds, two packets a socket (a a b b c c c: the rotation sends a b c a b c c), the last one
    later, a tenth local; window 1: the hosts without an outbound bucket offer a few more, early;
    window 2: none."""
    rng = np.random.default_rng(160 + k)
    per_host, pid = [], k * 100_000
    for h in range(H):
        n = int(rng.integers(3, 8)) if k == 0 else (int(rng.integers(0, 4)) if k == 1 and h % 4 == 3 else 0)
        lo, hi = (ws + (we - ws) // 3, we) if k == 0 else (ws, ws + (we - ws) // 2)
        t0 = int(rng.integers(lo, hi))
        offers = []
        for i in range(n):
            t = t0 if i < n - 1 else int(rng.integers(t0, hi))
            dst = h if rng.random() < 0.1 else int(rng.integers(0, H))
            pay = int(rng.choice([0, 1448, 1448, int(rng.integers(1, 1449))]))
            offers.append((t, (h << 4) | min(i // 2, 2), pay + HEADER, pay, dst, pid + i))
        pid += n
        per_host.append(offers)
    return per_host


class RrChainOracle(ChainOracle):
    """tests/test_outbound_gpu.py's composed oracle with the round-robin model at its front."""

    def __init__(self, end_time):
        super().__init__(end_time)
        self.om = RrOutboundModel(chain_case()[5])


def _rr_chain_offers(o):
    return lambda k, ws, we: rr_chain_offers(k, ws, we, o.H)


def _rr_chain_checks(o):
    assert len(o.batches) >= 2 and sum(len(b[1]) for b in o.batches) > 150
    c = o.om.counters
    assert c["not_in_offer_order"] > 20 and c["blocked_rotated"] > 5 and c["blocks"] > 20 and c["carried"] > 5 and \
        c["local_forwards"] > 5, c


def test_window_open_and_close_over_a_round_robin_stage():
    """Three windows through shd_window_open / shd_window_close: round-robin model -> oracle.relay
    -> oracle queues -> inbound model, every record and status as tests/test_window_gpu.py
    compares them for FIFO."""
    from shadow_amd.outbound import OutboundStage
    from shadow_amd.routing import Engine
    from tests.test_inbound_gpu import _same_state as _same_in_state
    from tests.test_window_gpu import Parts, run_windows
    from tests.test_window_sharded_gpu import _rows
    with Engine(0) as eng:
        o = RrChainOracle(S + 10**12)
        _, _, _, _, rng0, out_b, in_b = chain_case()
        p = Parts(eng, o, rng0, out_b, in_b)
        p.ostage = OutboundStage(eng, *_rows(out_b), ring_capacity=64, qdisc="round-robin", max_sockets=3)
        run_windows(p, o, _rr_chain_offers(o), 3, (S + 10**9, S + 10**9 + o.ra.get()))
        for h in range(o.H):
            _same_state(p.ostage, h, o.om.hosts[h])
            _same_in_state(p.istage.state(h), o.im.hosts[h])
    _rr_chain_checks(o)


def test_sharded_window_over_round_robin_stages():
    """The same three windows on two in-process ranks, each with a round-robin stage for its shard."""
    from shadow_amd.outbound import OutboundStage
    from tests.test_window_sharded_gpu import _rows, _world, run_windows

    def setup_outbound(self):
        self.ostage = OutboundStage(self.eng, *_rows(self.out_b[self.lo:self.hi]), first_host=self.lo,
                                    ring_capacity=64, qdisc="round-robin", max_sockets=3)
    o = RrChainOracle(S + 10**12)
    _, _, _, _, rng0, out_b, in_b = chain_case()
    engines, parts = _world(2, o, rng0, out_b, in_b)
    try:
        for p in parts:
            setup_outbound(p)
        run_windows(parts, o, _rr_chain_offers(o), 3, (S + 10**9, S + 10**9 + o.ra.get()))
        for p in parts:
            for h in range(p.lo, p.hi):
                _same_state(p.ostage, h - p.lo, o.om.hosts[h])
    finally:
        for e in engines:
            e.close()
    _rr_chain_checks(o)
