"""GPU parity of the outbound stage's two socket disciplines (SHD_QDISC_FIFO_SOCKETS,
SHD_QDISC_ROUND_ROBIN_SOCKETS: csrc/outbound.hip's OutFifoSock and OutRrSock over
csrc/sock_queue.h) against the CPU model (tests/outbound_sock_model.py): the batch arrays,
sent_pkt, the local CSR, the stored total, the next task time, the per-host state and the listing
of the queued sockets -- under fifo-sockets the heap array itself -- exactly."""
import numpy as np
import pytest

from oracle.token_bucket import SIM_START as S
from tests.outbound_sock_model import IDLE, LOCAL, SENT, SockOutboundModel
from tests.test_outbound import MS, bucket
from tests.test_outbound_gpu import HEADER, ChainOracle, _same, chain_case
from tests.test_outbound_sock import (A, B, FIFO, GEN_CAPACITY, GEN_HOSTS, GEN_MAX_SOCKETS, GEN_SEEDS, NAMES, QDISCS,
                                      SOCK_INPUTS, SOCK_WANT, case_windows, np_arrays, random_setup, random_window,
                                      run_seed)

pytestmark = pytest.mark.gpu


def _stage(engine, buckets, qdisc, first_host=0, ring=GEN_CAPACITY, max_sockets=GEN_MAX_SOCKETS):
    from shadow_amd.outbound import OutboundStage
    rows = [(0, 0, 0, S) if b is None else b for b in buckets]
    cap, inc, itv, last = (np.array([r[i] for r in rows], np.uint64) for i in range(4))
    return OutboundStage(engine, cap, inc, itv, last, first_host=first_host, ring_capacity=ring, qdisc=qdisc,
                         max_sockets=max_sockets)


def _advance(stage, arr, window_end, bootstrap_end=0):
    """arr: off, time, prio, sock, size, payload, dst, pkt (the model's order)."""
    return stage.advance(arr[0], arr[1], arr[2], *arr[4:], sock=arr[3], window_end=window_end,
                         bootstrap_end=bootstrap_end)


def _same_state(stage, h, host):
    st = stage.state(h)
    assert st["task_time"] == host.task
    assert st["cached"] == (None if host.cached is None else (host.cached[1], host.cached[2]))
    assert st["queue_len"] == len(host.q)
    assert st["head_pkt"] == host.q.head_pkt()
    assert stage.sockets(h) == host.q.listing()   # fifo-sockets: the heap array in index order
    if host.tb is None:
        assert st["bucket"] is None
    else:
        b = st["bucket"]
        assert (b["capacity"], b["balance"], b["refill_increment"], b["refill_interval"], b["last_refill"]) == \
               (host.tb.capacity, host.tb.balance, host.tb.refill_increment, host.tb.refill_interval,
                host.tb.last_refill)
        assert b["pending_until"] == (host.task or 0)


@pytest.mark.parametrize("qdisc", QDISCS)
@pytest.mark.parametrize("name", sorted(SOCK_INPUTS))
def test_hand_cases_on_device(engine, name, qdisc):
    """Records, n_stored, the next task, get_state and get_sockets after every window, against the
    pinned values and against the model."""
    b, first, windows = case_windows(name)
    want = SOCK_WANT[(name, qdisc)]
    stage = _stage(engine, [b], qdisc, first)
    model = SockOutboundModel([b], first, qdisc)
    for (arr, w_end, boot), (recs, n_stored, nxt, socks, head) in zip(windows, want):
        arr = [np.array(c, np.uint64 if i in (1, 2, 3) else np.uint32) for i, c in enumerate(arr)]
        r = _advance(stage, arr, w_end, boot)
        got = [(SENT, p, (t - S) / MS) for p, t, _, _ in r.sent_for(0)] + \
              [(LOCAL, p, (t - S) / MS) for p, t in r.local_for(0)]
        assert got == recs
        assert (r.n_stored, r.next_task_time) == (n_stored, IDLE if nxt is None else S + int(round(nxt * MS)))
        assert [(NAMES[h], n) for h, n in stage.sockets(0)] == socks
        assert stage.state(0)["head_pkt"] == head
        _same(r, model.advance(*arr, w_end, boot))
        _same_state(stage, 0, model.hosts[0])
    task, cached, balance, queue_len = want[-1]
    st = stage.state(0)
    assert (None if st["task_time"] is None else (st["task_time"] - S) / MS,
            None if st["cached"] is None else st["cached"][0],
            None if st["bucket"] is None else st["bucket"]["balance"], st["queue_len"]) == (task, cached, balance, queue_len)


@pytest.mark.parametrize("qdisc", QDISCS)
@pytest.mark.parametrize("seed", GEN_SEEDS)
def test_random_windows_vs_model(engine, seed, qdisc):
    """Four consecutive windows over 130 hosts (two full 64-lane workgroups and a partial one)
    with 1-8 sockets each, 16 slots a host, at most 40 offers per host and window, 30 % control
    packets, every other host on a slow bucket, bootstrap_end inside the second window: every
    array of every window, every host's state and socket listing after every window."""
    stage = _stage(engine, random_setup(seed)[1], qdisc)

    def each_window(arr, end, boot, want, model):
        _same(_advance(stage, arr, end, boot), want)
        for h in range(GEN_HOSTS):
            _same_state(stage, h, model.hosts[h])
    model = run_seed(seed, qdisc, each_window)
    c = model.counters
    assert c["blocked_rotated"] > 0 and c["slots_reused"] > 0 and c["not_lowest"] > 0 and c["carried"] > 0
    assert model.max_depth <= GEN_CAPACITY and 7 <= model.max_sockets <= GEN_MAX_SOCKETS


@pytest.mark.parametrize("qdisc", QDISCS)
def test_many_hosts_past_one_scan_tile_and_nonzero_first_host(engine, qdisc):
    """9001 hosts with first_host = 4500: more than one 8192-entry tile in all three scans; two
    windows, a quarter of the hosts blocked across them, local packets by global id."""
    rng = np.random.default_rng(179)
    n_hosts, first = 9001, 4500
    buckets = [bucket(1000) if h % 4 == 0 else (None if h % 4 == 1 else bucket(125_000)) for h in range(n_hosts)]
    socks = [[(h << 8) | k for k in range(1 + h % 3)] for h in range(n_hosts)]
    stage = _stage(engine, buckets, qdisc, first_host=first, ring=8, max_sockets=3)
    model = SockOutboundModel(buckets, first, qdisc)
    start, pid, prio = S, 0, [1] * n_hosts
    for win in (20 * MS, 4000 * MS):
        per_host, pid = random_window(rng, model.hosts, socks, prio, start, start + 20 * MS, pid, capacity=8,
                                      max_offers=3, n_dst=n_hosts, first_host=first)
        arr = np_arrays(per_host)
        want = model.advance(*arr, start + win, 0)
        _same(_advance(stage, arr, start + win), want)
        assert want["src_off"][-1] > 8192 and want["loc_off"][-1] > 500
        for h in range(0, n_hosts, 7):
            _same_state(stage, h, model.hosts[h])
        start += win
    # (the generator's own figures, the same for every stage: hosts in every workgroup range block,
    # and some four hundred hosts carry a task and their queue over the windows' boundary)
    assert model.counters["blocks"] > 500 and model.counters["carried"] > 300


# Two ACKs queued while the bucket blocks: p1 is cached behind p0, then A and B each offer an ACK
TWO_ACKS = [[[(S, 1, A, 1500, 1448, 1, 0), (S, 2, A, 1500, 1448, 1, 1)]],
            [[(S + 20, 0, A, HEADER, 0, 1, 2), (S + 21, 0, B, HEADER, 0, 1, 3), (S + 22, 3, A, 100, 48, 1, 4)]]]


def test_plain_fifo_refuses_two_queued_control_packets_fifo_sockets_sends_them(engine):
    from shadow_amd._native import ShdError
    plain = _stage(engine, [bucket()], "fifo")
    for k, per_host in enumerate(TWO_ACKS):
        arr = np_arrays(per_host)
        plain_arr = (arr[0], arr[1], arr[2], *arr[4:])
        if k == 0:
            plain.advance(*plain_arr, window_end=S + 10)
        else:
            with pytest.raises(ShdError, match="INVALID"):
                plain.advance(*plain_arr, window_end=S + 100)
            with pytest.raises(ShdError, match="STATE"):
                plain.advance(window_end=S + 200)
    for qdisc in QDISCS:
        stage = _stage(engine, [bucket()], qdisc)
        model = SockOutboundModel([bucket()], 0, qdisc)
        for per_host, end in zip(TWO_ACKS + [[[]]], (S + 10, S + 100, S + 5000 * MS)):
            arr = np_arrays(per_host)
            want = model.advance(*arr, end)
            r = _advance(stage, arr, end)
            _same(r, want)
            _same_state(stage, 0, model.hosts[0])
        # p1 first (cached), then both ACKs, A's and B's in the discipline's order, then the data packet
        assert r.sent_pkt.tolist() == ([1, 3, 2, 4] if qdisc == FIFO else [1, 2, 3, 4]) and r.n_stored == 0


_P = lambda t, hd, pkt, prio=0, size=100, dst=1: (t, prio, hd, size, size - HEADER, dst, pkt)  # noqa: E731
# (capacity, max_sockets, [(per_host offers, window_end)]): the last offer of the last step is one too many
OVER = {
    # capacity 4: p1 is cached behind p0 (it is not queued), then five offers before its task runs
    "capacity_plus_one_packets": (4, 4, [([[_P(S, A, 0, 1, 1500), _P(S, A, 1, 2, 1500)]], S + 10),
                                         ([[_P(S + 20 + i, A, 2 + i, i % 2) for i in range(5)]], S + 100)]),
    # max_sockets 3: three sockets queued behind the cached p1, the fourth is one too many
    "max_sockets_plus_one_sockets": (16, 3, [([[_P(S, A, 0, 1, 1500), _P(S, A, 1, 2, 1500)]], S + 10),
                                             ([[_P(S + 20 + i, 50 + i, 2 + i, i % 2) for i in range(4)]], S + 100)]),
}


@pytest.mark.parametrize("qdisc", QDISCS)
@pytest.mark.parametrize("name", list(OVER))
def test_one_packet_or_socket_too_many(engine, name, qdisc):
    """An overflow by one is SHD_ERR_INVALID from a check in the kernel, every later call
    SHD_ERR_STATE, and a fresh setup works again.  One packet and one socket fewer are taken."""
    from shadow_amd._native import ShdError
    ring, ms, steps = OVER[name]
    stage = _stage(engine, [bucket()], qdisc, ring=ring, max_sockets=ms)
    for per_host, w_end in steps[:-1]:
        _advance(stage, np_arrays(per_host), w_end)
    r = _advance(stage, np_arrays([steps[-1][0][0][:-1]]), steps[-1][1])
    assert r.n_stored == len(steps[-1][0][0])   # the cached packet + the queue, full to the brim
    assert len(stage.sockets(0)) == (1 if name.endswith("_packets") else ms)
    stage = _stage(engine, [bucket()], qdisc, ring=ring, max_sockets=ms)
    for per_host, w_end in steps[:-1]:
        _advance(stage, np_arrays(per_host), w_end)
    with pytest.raises(ShdError, match="INVALID"):
        _advance(stage, np_arrays(steps[-1][0]), steps[-1][1])
    with pytest.raises(ShdError, match="STATE"):
        stage.advance(window_end=steps[-1][1] + 10)
    with pytest.raises(ShdError, match="STATE"):
        stage.state(0)
    with pytest.raises(ShdError, match="STATE"):
        stage.sockets(0)
    stage = _stage(engine, [bucket()], qdisc, ring=ring, max_sockets=ms)
    r = _advance(stage, np_arrays([[_P(S + 61, B, 7)]]), S + 70)
    assert r.sent_for(0) == [(7, S + 61, 1, 48)] and r.n_stored == 0 and r.next_task_time == IDLE


@pytest.mark.parametrize("qdisc", QDISCS)
def test_the_other_contract_errors_keep_their_status(engine, qdisc):
    from shadow_amd._native import ShdError
    for per_host in ([[_P(S + 5, A, 0), _P(S + 4, A, 1)]], [[_P(S + 10, A, 0)]], [[_P(S + 5, A, 2**32 - 1)]],
                     [[_P(S + 5, A, 0, 1, 1502)]]):
        stage = _stage(engine, [bucket()], qdisc)
        with pytest.raises(ShdError, match="INVALID"):
            _advance(stage, np_arrays(per_host), S + 10)
        with pytest.raises(ShdError, match="STATE"):
            stage.advance(window_end=S + 20)
    # equal priorities, zero or not, are no error: the disciplines have no priority rule
    stage = _stage(engine, [bucket()], qdisc)
    r = _advance(stage, np_arrays([[_P(S + 1, A, 0, 5), _P(S + 1, B, 1, 5), _P(S + 1, A, 2, 5)]]), S + 10)
    assert sorted(r.sent_pkt.tolist()) == [0, 1, 2]


def test_setup_and_argument_errors_leave_the_stage_as_it_was(engine):
    """An unknown qdisc and max_sockets = 0 are refused at the setup and the stage set up before
    goes on; so does a NULL socket column with offers.  The two plain disciplines ignore d_sock."""
    import ctypes as C
    import torch
    from shadow_amd import _native as N
    from shadow_amd._native import ShdError
    stage = _stage(engine, [bucket()], FIFO)
    # p0 leaves; the root B gives its ACK p3, which blocks: A(p1) and B(p2) stay, B pushed again
    first = np_arrays([[_P(S, A, 0, 1, 1500), _P(S, A, 1, 2), _P(S, B, 2, 3, 1500), _P(S, B, 3, 0)]])
    _advance(stage, first, S + 10)
    before = (stage.sockets(0), stage.state(0))
    assert before[0] == [(A, 1), (B, 1)] and before[1]["cached"] == (3, 100) and before[1]["head_pkt"] == 1
    one = np.array([1501, 1, MS, S], np.uint64)
    p = [N.ptr(one[i:i + 1]) for i in range(4)]
    lib, ctx = engine.lib, engine.ctx
    for qd in (2, 3, 6, 8):
        assert N.STATUS_NAMES[lib.shd_outbound_setup_qdisc(ctx, 1, 0, 4, qd, 4, *p)] == "INVALID"
    assert (N.QDISC_FIFO_SOCKETS, N.QDISC_ROUND_ROBIN_SOCKETS) == (4, 5)
    for qd in (N.QDISC_FIFO_SOCKETS, N.QDISC_ROUND_ROBIN_SOCKETS):
        assert N.STATUS_NAMES[lib.shd_outbound_setup_qdisc(ctx, 1, 0, 4, qd, 0, *p)] == "INVALID"
        assert N.STATUS_NAMES[lib.shd_outbound_setup_qdisc(ctx, 1, 0, 0, qd, 4, *p)] == "INVALID"
    d = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(ShdError, match="INVALID"):
        stage.advance_device(d, d, d, d, d, d, d, 1, S + 20)                  # d_sock = NULL
    with pytest.raises(ShdError, match="INVALID"):
        stage.advance_device(d, d, None, d, d, d, d, 1, S + 20, d_sock=d)     # d_prio = NULL
    with pytest.raises(ValueError):
        stage.advance(first[0], first[1], first[2], *first[4:], window_end=S + 20)   # no sock=
    with pytest.raises(ShdError, match="INVALID"):
        stage.sockets(1)
    assert (stage.sockets(0), stage.state(0)) == before   # untouched
    n = C.c_uint32(9)
    assert lib.shd_outbound_get_sockets(ctx, 0, None, None, 0, C.byref(n)) == 0 and n.value == 2
    # the old disciplines ignore the socket column: the same batches with it and without it
    arr = np_arrays([[_P(S + 1, 7, 0, 1), _P(S + 2, 7, 1, 2, 1500), _P(S + 2, 9, 2, 3, 1500)]])
    for qd in ("fifo", "round-robin"):
        outs = []
        for with_sock in (False, True):
            plain = _stage(engine, [bucket()], qd)
            dev = [torch.from_numpy(np.ascontiguousarray(a).view(a.dtype.str.replace("u", "i"))).cuda() for a in arr]
            torch.cuda.synchronize()
            out = plain.advance_device(dev[0], dev[1], dev[2], *dev[4:], 3, S + 200 * MS,
                                       d_sock=dev[3] if with_sock else None)
            outs.append(plain.sent(out))
        for k in ("src_off", "send_time", "sent_pkt"):
            assert np.array_equal(getattr(outs[0], k), getattr(outs[1], k)), k
        assert len(outs[0].sent_pkt) == 2 and outs[0].n_stored == outs[1].n_stored == 1
    with pytest.raises(ValueError):
        _stage(engine, [bucket()], "fifo-socket")


# ---- the two-call window over a fifo-sockets stage -------------------------------------------

class _Box:
    """The socket column of the window being run, beside the seven columns the window harness
    of tests/test_window_gpu.py passes on."""
    off = sock = None


def sock_chain_offers(box, k, ws, we, H, prio):
    """Window 0: every host offers a burst of 3-7 packets at one instant in the window's last two
    thirds on up to three sockets, a third of them control packets, the last one later, a tenth
    local; window 1: the hosts without an outbound bucket offer a few more, early; window 2: none.
    Returns the seven plain columns' tuples; the socket column goes into the box."""
    rng = np.random.default_rng(260 + k)
    per_host, socks, pid = [], [], k * 100_000
    for h in range(H):
        n = int(rng.integers(3, 8)) if k == 0 else (int(rng.integers(0, 4)) if k == 1 and h % 4 == 3 else 0)
        lo, hi = (ws + (we - ws) // 3, we) if k == 0 else (ws, ws + (we - ws) // 2)
        t0 = int(rng.integers(lo, hi))
        offers = []
        for i in range(n):
            t = t0 if i < n - 1 else int(rng.integers(t0, hi))
            dst = h if rng.random() < 0.1 else int(rng.integers(0, H))
            if rng.random() < 0.33:
                pr, pay = 0, 0
            else:
                pr, pay = prio[h], int(rng.choice([1448, 1448, int(rng.integers(1, 1449))]))
                prio[h] += 1
            offers.append((t, pr, pay + HEADER, pay, dst, pid + i))
            socks.append((h << 4) | int(rng.integers(0, 3)))
        pid += n
        per_host.append(offers)
    box.off = np.concatenate([[0], np.cumsum([len(e) for e in per_host])])
    box.sock = np.array(socks, np.uint64)
    return per_host


class _SockFront:
    """The socket model where the chain oracle keeps its outbound model: the harness's seven
    columns plus the box's socket column."""

    def __init__(self, model, box):
        self.m, self.box = model, box

    def advance(self, off, time, prio, size, payload, dst, pkt, window_end, bootstrap_end=0):
        return self.m.advance(off, time, prio, None if off is None else self.box.sock, size, payload, dst, pkt,
                              window_end, bootstrap_end)

    def __getattr__(self, k):
        return getattr(self.m, k)


class SockChainOracle(ChainOracle):
    def __init__(self, end_time, box):
        super().__init__(end_time)
        self.om = _SockFront(SockOutboundModel(chain_case()[5], 0, FIFO), box)


class _SockWindow:
    """shadow_amd.window.Window with close() adding the rank's slice of the box's socket column.
    null_first: the first close is made without the column (by this rank if `null_first` is
    True, with it otherwise) and its status kept in `refused`; then the close proper."""

    def __init__(self, win, box, lo, hi, null_first=None):
        self.win, self.box, self.lo, self.hi = win, box, lo, hi
        self.null_first, self.refused = null_first, None

    def close(self, *args):
        import torch
        from shadow_amd._native import ShdError
        d_sock = None
        if args[0] is not None:
            a, z = int(self.box.off[self.lo]), int(self.box.off[self.hi])
            d_sock = torch.from_numpy(self.box.sock[a:z].view(np.int64)).cuda()
            torch.cuda.synchronize()
        if self.null_first is not None:
            try:
                self.win.close(*args, d_sock=None if self.null_first else d_sock)
                self.refused = "OK"
            except ShdError as e:
                self.refused = e.code
            self.null_first = None
        return self.win.close(*args, d_sock=d_sock)

    def __getattr__(self, k):
        return getattr(self.win, k)


def _sock_chain_checks(o):
    assert len(o.batches) >= 2 and sum(len(b[1]) for b in o.batches) > 150
    c = o.om.counters
    assert c["stale_key"] > 5 and c["not_lowest"] > 5 and c["blocked_rotated"] > 5 and c["blocks"] > 20 and \
        c["carried"] > 5 and c["local_forwards"] > 5, c


def test_window_open_and_close_over_a_fifo_sockets_stage():
    """Three windows through shd_window_open / shd_window_close_sockets: socket model -> oracle.relay
    -> oracle queues -> inbound model, every record and status as tests/test_window_gpu.py
    compares them.  A close without the socket column is refused with nothing run: the close
    proper follows it."""
    from shadow_amd.outbound import OutboundStage
    from shadow_amd.routing import Engine
    from tests.test_inbound_gpu import _same_state as _same_in_state
    from tests.test_window_gpu import Parts, run_windows
    from tests.test_window_sharded_gpu import _rows
    box = _Box()
    with Engine(0) as eng:
        o = SockChainOracle(S + 10**12, box)
        _, _, _, _, rng0, out_b, in_b = chain_case()
        p = Parts(eng, o, rng0, out_b, in_b)
        p.ostage = OutboundStage(eng, *_rows(out_b), ring_capacity=64, qdisc=FIFO, max_sockets=3)
        p.win = _SockWindow(p.win, box, 0, o.H, null_first=True)
        prio = [1] * o.H
        run_windows(p, o, lambda k, ws, we: sock_chain_offers(box, k, ws, we, o.H, prio), 3,
                    (S + 10**9, S + 10**9 + o.ra.get()))
        assert p.win.refused == "INVALID"
        for h in range(o.H):
            _same_state(p.ostage, h, o.om.hosts[h])
            _same_in_state(p.istage.state(h), o.im.hosts[h])
    _sock_chain_checks(o)


def test_sharded_window_over_fifo_sockets_stages():
    """The same three windows on two in-process ranks, each with a fifo-sockets stage for its
    shard.  In window 0 rank 1 first calls the close without its socket column: every rank's close
    returns SHD_ERR_INVALID and nothing has run -- the close proper then gives the oracle's window."""
    from shadow_amd.outbound import OutboundStage
    from tests.test_window_sharded_gpu import _rows, _world, run_windows
    box = _Box()
    o = SockChainOracle(S + 10**12, box)
    _, _, _, _, rng0, out_b, in_b = chain_case()
    engines, parts = _world(2, o, rng0, out_b, in_b)
    try:
        for i, p in enumerate(parts):
            p.ostage = OutboundStage(p.eng, *_rows(out_b[p.lo:p.hi]), first_host=p.lo, ring_capacity=64, qdisc=FIFO,
                                     max_sockets=3)
            p.win = _SockWindow(p.win, box, p.lo, p.hi, null_first=(i == 1))
        prio = [1] * o.H
        run_windows(parts, o, lambda k, ws, we: sock_chain_offers(box, k, ws, we, o.H, prio), 3,
                    (S + 10**9, S + 10**9 + o.ra.get()))
        assert [p.win.refused for p in parts] == ["INVALID", "INVALID"]
        for p in parts:
            for h in range(p.lo, p.hi):
                _same_state(p.ostage, h - p.lo, o.om.hosts[h])
    finally:
        for e in engines:
            e.close()
    _sock_chain_checks(o)
