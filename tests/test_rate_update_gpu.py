"""GPU parity of the bucket re-rate (csrc/rate_update.hip: shd_tb_update, shd_inbound_update_buckets,
shd_outbound_update_buckets, shd_window_update_bandwidth) against the CPU models of the stages with
tests/rate_model.py's ``rerate`` applied to their buckets: every record of the windows around a
re-rate and every host's state, exactly; and the refusals, each of which leaves every host as it
was."""
import numpy as np
import pytest

from oracle import token_bucket as TB
from oracle.token_bucket import SIM_START as S, create_token_bucket
from tests.inbound_model import IDLE, InboundModel
from tests.outbound_model import OutboundModel
from tests.outbound_rr_model import RrOutboundModel
from tests.outbound_sock_model import SockOutboundModel
from tests.rate_model import rerate

pytestmark = pytest.mark.gpu

MS = TB.MS
HEADER = 52
NONE = (0, 0, 0)
A, B = 0x7F00_0000_1000, 77   # two sockets' canonical handles


def big(last=S):
    """A bucket that holds 5000 tokens and gains one a millisecond: packets above CONFIG_MTU fit."""
    return (5000, 1, MS, last)


def apply_model(hosts, entries, at):
    """``entries``: [(host, capacity, increment, interval)] as the call names them; a host named
    more than once takes its last entry (the earlier ones do not even refill it)."""
    for h, row in {e[0]: e[1:] for e in entries}.items():
        hosts[h].tb = rerate(hosts[h].tb, at, *row)


def call(stage, entries, at):
    cols = list(zip(*entries)) if entries else [(), (), (), ()]
    stage.update_buckets(*cols, at)


def refused(fn, code="INVALID", host=None):
    from shadow_amd._native import ShdError
    with pytest.raises(ShdError, match=code) as e:
        fn()
    assert getattr(e.value, "host", None) == host
    return e.value


# ---- the replay engine ----

def _tb_state_matches(tbs, r, bucket, pending, last_none):
    st = tbs.state(r)
    if bucket is None:
        assert (st["capacity"], st["balance"], st["refill_increment"], st["refill_interval"]) == (0, 0, 0, 0)
        if last_none[r] is not None:
            assert st["last_refill"] == last_none[r]
    else:
        assert (st["capacity"], st["balance"], st["refill_increment"], st["refill_interval"], st["last_refill"]) == \
               (bucket.capacity, bucket.balance, bucket.refill_increment, bucket.refill_interval, bucket.last_refill)
    assert st["pending_until"] == pending


@pytest.mark.parametrize("n_relays", [1, 64, 300])
def test_replay_engine_batches_with_a_rerate_between(engine, n_relays):
    """Three batches of attempts against oracle.token_bucket.relay_run, a random subset of the
    relays re-rated at each batch boundary: a relay named twice, relays that lose and gain their
    bucket, and relays that are Pending across the call (they stay Pending until their deadline)."""
    from shadow_amd.tbucket import TokenBuckets
    rng = np.random.default_rng(300 + n_relays)
    rates = [1000, 20_000, 1_250_000]
    rows = [NONE if rng.random() < 0.2 else create_token_bucket(int(rng.choice(rates))) for _ in range(n_relays)]
    if n_relays == 1:
        rows = [create_token_bucket(1000)]
    tbs = TokenBuckets(engine, *(np.array([r[i] for r in rows], np.uint64) for i in range(3)), S)
    buckets = [None if r == NONE else TB.TokenBucket(*r, S) for r in rows]
    pending = [0] * n_relays
    last_none = [None] * n_relays   # where a relay lost its bucket: last_refill reads back as that time
    start = S
    pending_across, dup_seen, lost, gained = 0, 0, 0, 0
    for batch in range(3):
        end = start + 40 * MS
        off, time, size, flags = [0], [], [], []
        for r in range(n_relays):
            n = int(rng.integers(1, 12))
            time += np.sort(rng.integers(start, end, n)).tolist()
            size += rng.integers(1, 1501, n).tolist()
            flags += (rng.random(n) < 0.1).astype(np.uint8).tolist()
            off.append(len(time))
        arr = (np.array(off, np.uint32), np.array(time, np.uint64), np.array(size, np.uint32), np.array(flags, np.uint8))
        want_s, want_v = TB.relay_run(buckets, pending, *arr)
        got_s, got_v = tbs.run(*arr)
        assert got_s.tolist() == want_s and got_v.tolist() == want_v, batch
        # the re-rate at the boundary: about half the relays, the first of them named twice
        named = [r for r in range(n_relays) if rng.random() < 0.5] or [0]
        entries = []
        for r in named + named[:1]:
            row = NONE if rng.random() < 0.25 else create_token_bucket(int(rng.choice(rates)))
            entries.append((r, *row))
        dup_seen += entries[0][1:] != entries[-1][1:]
        for r, *row in {e[0]: e for e in entries}.values():
            pending_across += pending[r] > end
            lost += buckets[r] is not None and tuple(row) == NONE
            gained += buckets[r] is None and tuple(row) != NONE
            if buckets[r] is not None and tuple(row) == NONE:
                last_none[r] = end
            elif tuple(row) != NONE:
                last_none[r] = None
        call(tbs, entries, end)
        apply_model([_Slot(buckets, r) for r in range(n_relays)], entries, end)
        for r in range(n_relays):
            _tb_state_matches(tbs, r, buckets[r], pending[r], last_none)
        start = end
    assert pending_across > 0   # a 1000 B/s relay blocks for up to 1.5 s: Pending across the calls
    if n_relays > 1:
        assert dup_seen and lost and gained


class _Slot:
    """buckets[i] behind the ``.tb`` attribute apply_model sets."""

    def __init__(self, buckets, i):
        self.buckets, self.i = buckets, i

    @property
    def tb(self):
        return self.buckets[self.i]

    @tb.setter
    def tb(self, v):
        self.buckets[self.i] = v


def test_replay_engine_refusals(engine):
    from shadow_amd.tbucket import TokenBuckets
    tbs = TokenBuckets(engine, [1501, 0, 1501], [1, 0, 1], [MS, 0, MS], S + 100)
    before = [tbs.state(r) for r in range(3)]
    refused(lambda: tbs.update_buckets([0, 2], 1501, 1, MS, S + 99), host=0)      # before last_refill, both: the lowest
    refused(lambda: tbs.update_buckets([1, 2], 1501, 1, MS, S + 99), host=2)      # relay 1 has no bucket: no last refill
    refused(lambda: tbs.update_buckets([3], 1501, 1, MS, S + 200))                # index
    refused(lambda: tbs.update_buckets([0], 1501, 0, MS, S + 200))                # partial zeros
    assert [tbs.state(r) for r in range(3)] == before
    tbs.update_buckets([], [], [], [], S)                                         # n == 0: nothing
    tbs.update_bandwidth([1, 0], [125_000, None], S + 200)
    assert tbs.state(1)["capacity"] == 1625 and tbs.state(1)["balance"] == 1625 and tbs.state(1)["last_refill"] == S + 200
    assert tbs.state(0) == dict(capacity=0, balance=0, refill_increment=0, refill_interval=0, last_refill=S + 200,
                                pending_until=0)


# ---- the inbound stage: hand cases ----

def _in(engine, buckets, ring=512):
    from tests.test_inbound_gpu import _stage
    return _stage(engine, buckets, ring), InboundModel(buckets)


def _in_window(stage, model, per_host, end, boot=0):
    from tests.test_inbound_gpu import _arrays, _same_records
    arr = _arrays(per_host) if per_host is not None else (None,) * 4
    _same_records(stage.advance(*arr, window_end=end, bootstrap_end=boot), model.advance(*arr, end, boot))


def _in_states(stage, model):
    from tests.test_inbound_gpu import _same_state
    for h, host in enumerate(model.hosts):
        _same_state(stage.state(h), host)


def test_inbound_raised_rate_keeps_the_task_and_the_cached_packet(engine):
    """A 1000 B/s host blocked on a cached packet (its task 1499 ms away) is raised to 125 kB/s: the
    task keeps its time, the packet stays cached, the balance is the old rate's refill, and the
    task then forwards the packet against the new bucket."""
    stage, model = _in(engine, [(*create_token_bucket(1000), S)])
    at = S + 10 * MS + 500_000   # half an interval past the old grid: the new grid starts here, not at S + 10 ms
    _in_window(stage, model, [[(S, 1500, 0), (S, 1500, 1)]], at)
    assert model.hosts[0].task == S + 1499 * MS and model.hosts[0].cached == 1
    entries = [(0, *create_token_bucket(125_000))]
    call(stage, entries, at)
    apply_model(model.hosts, entries, at)
    st = stage.state(0)
    assert st["task_time"] == S + 1499 * MS and st["cached"] == (1, 1500)
    assert st["bucket"] == dict(capacity=1625, balance=11, refill_increment=125, refill_interval=MS,
                                last_refill=at, pending_until=S + 1499 * MS)
    _in_states(stage, model)
    _in_window(stage, model, [[(S + 20 * MS, 1500, 2)]], S + 1600 * MS)   # (packet 2 needs 11 more refills)
    assert model.hosts[0].stored() == 0
    _in_states(stage, model)


def test_inbound_lowered_rate_clamps_and_none_goes_both_ways(engine):
    """Host 0: 125 kB/s and full, lowered to 1000 B/s: the balance is clamped to the new capacity.
    Host 1: no bucket -> a bucket (full, last refilled at the call).  Host 2: a bucket -> none.
    Host 3: none -> none.  Host 4 is named twice: its last entry counts."""
    b = (*create_token_bucket(125_000), S)
    stage, model = _in(engine, [b, None, b, None, b])
    at = S + 5 * MS
    _in_window(stage, model, [[(S + 1, 700, 0)], [(S + 2, 700, 1)], [(S + 3, 700, 2)], [], []], at)
    entries = [(0, *create_token_bucket(1000)), (4, 100, 1, 1), (1, *create_token_bucket(20_000)), (2, *NONE), (3, *NONE),
               (4, 2000, 3, MS)]
    call(stage, entries, at)
    apply_model(model.hosts, entries, at)
    st = [stage.state(h)["bucket"] for h in range(5)]
    assert (st[0]["capacity"], st[0]["balance"], st[0]["last_refill"]) == (1501, 1501, at)
    assert (st[1]["capacity"], st[1]["balance"], st[1]["last_refill"]) == (1520, 1520, at)
    assert st[2] is None and st[3] is None
    assert (st[4]["capacity"], st[4]["balance"], st[4]["refill_increment"]) == (2000, 1625, 3)
    _in_states(stage, model)
    per_host = [[(at + 1, 1500, 10), (at + 2, 1500, 11)] for _ in range(5)]
    _in_window(stage, model, [[(t, s, p + 10 * h) for t, s, p in e] for h, e in enumerate(per_host)], at + 20 * MS)
    assert model.counters["blocks"] >= 2   # hosts 0 and 1 are held back by their new buckets
    _in_states(stage, model)


# ---- refusals leave everything as it was ----

def _refusal_setup(engine):
    """Host 0: a cached packet of 2000 and four queued, the 3000-byte one behind the head at ring
    position 0 -- the ring of 4 has wrapped.  Host 1: a cached packet of 2000 and a queued one of
    100.  Host 2: idle, full."""
    stage, model = _in(engine, [big(), big(), big()], ring=4)
    blocked = [(S, 4000, 0), (S, 2000, 1), (S + 1, 100, 2), (S + 2, 100, 3)]
    _in_window(stage, model, [blocked, [(S, 4000, 10), (S, 2000, 11), (S + 1, 100, 12)], []], S + 10 * MS)
    _in_window(stage, model, [[(S + 11 * MS, 3000, 4), (S + 12 * MS, 100, 5)], [], []], S + 20 * MS)
    h0, h1 = model.hosts[0], model.hosts[1]
    assert h0.task == S + 1000 * MS and h0.cached == 1 and len(h0.q) == 4 and h1.cached == 11 and len(h1.q) == 1
    return stage, model, S + 20 * MS


def _all_states(stage, n):
    return [stage.state(h) for h in range(n)]


def test_inbound_refusals_change_nothing(engine):
    stage, model, at = _refusal_setup(engine)
    before = _all_states(stage, 3)
    rows = lambda cap: (cap, 1, MS)  # noqa: E731
    # below the 3000-byte packet behind the head of the wrapped ring (the cached 2000 would fit)
    refused(lambda: call(stage, [(2, *rows(100)), (0, *rows(2500))], at), host=0)
    # below the cached packet only (the queued one is 100 bytes)
    refused(lambda: call(stage, [(1, *rows(1999))], at), host=1)
    # two hosts fail: the lowest is reported, whatever the order of the entries
    refused(lambda: call(stage, [(1, *rows(1999)), (2, *rows(7)), (0, *rows(2500))], at), host=0)
    # after the outstanding task (S + 1000 ms on hosts 0 and 1); host 2 has none and would pass
    refused(lambda: call(stage, [(2, *rows(5000)), (1, *rows(5000))], S + 1000 * MS + 1), host=1)
    # below the previous window_end, a bad index, partial zeros: refused before any launch
    refused(lambda: call(stage, [(2, *rows(5000))], at - 1))
    refused(lambda: call(stage, [(2, *rows(5000)), (3, *rows(5000))], at))
    refused(lambda: call(stage, [(2, *rows(5000)), (1, 5000, 0, MS)], at))
    assert _all_states(stage, 3) == before
    # `at` before last_refill: host 2 is first re-rated in the future (accepted), then earlier
    call(stage, [(2, *rows(4000))], at + 100 * MS)
    apply_model(model.hosts, [(2, *rows(4000))], at + 100 * MS)
    before = _all_states(stage, 3)
    assert before[2]["bucket"]["last_refill"] == at + 100 * MS
    refused(lambda: call(stage, [(2, *rows(4000))], at + 50 * MS), host=2)
    assert _all_states(stage, 3) == before
    # accepted at the same place: exactly the largest stored size, and the task's own time
    call(stage, [(0, *rows(3000))], S + 1000 * MS)
    apply_model(model.hosts, [(0, *rows(3000))], S + 1000 * MS)
    _in_states(stage, model)
    # the next window is the model's, which saw only the accepted calls
    _in_window(stage, model, None, S + 6000 * MS)
    _in_states(stage, model)


def test_not_ready_is_a_state_error(engine):
    from shadow_amd._native import ShdError
    stage, _ = _in(engine, [big()], ring=4)
    with pytest.raises(ShdError, match="INVALID"):   # a contract error: the event lies at window_end
        stage.advance(np.array([0, 1], np.uint32), np.array([S + 10], np.uint64), np.array([100], np.uint32),
                      np.array([0], np.uint32), window_end=S + 10)
    refused(lambda: call(stage, [(0, 5000, 1, MS)], S + 10), code="STATE")
    refused(lambda: call(stage, [], S + 10), code="STATE")


# ---- must be accepted ----

OUT_KINDS = ("fifo", "round-robin", "fifo-sockets", "round-robin-sockets")


class Out:
    """One outbound stage and its model under a discipline; offers are (time, prio, sock, size,
    payload, dst, pkt) per host."""

    def __init__(self, engine, kind, buckets, first_host=0, ring=16, max_sockets=8):
        from shadow_amd.outbound import OutboundStage
        rows = [(0, 0, 0, S) if b is None else b for b in buckets]
        cap, inc, itv, last = (np.array([r[i] for r in rows], np.uint64) for i in range(4))
        self.kind = kind
        self.stage = OutboundStage(engine, cap, inc, itv, last, first_host=first_host, ring_capacity=ring, qdisc=kind,
                                   max_sockets=max_sockets)
        self.model = (OutboundModel(buckets, first_host) if kind == "fifo" else
                      RrOutboundModel(buckets, first_host) if kind == "round-robin" else
                      SockOutboundModel(buckets, first_host, kind))

    def window(self, per_host, end, boot=0):
        from tests.test_outbound_gpu import _same
        from tests.test_outbound_sock import np_arrays
        off, time, prio, sock, size, pay, dst, pkt = np_arrays(per_host)
        if self.kind == "fifo":
            want = self.model.advance(off, time, prio, size, pay, dst, pkt, end, boot)
            got = self.stage.advance(off, time, prio, size, pay, dst, pkt, window_end=end, bootstrap_end=boot)
        elif self.kind == "round-robin":
            want = self.model.advance(off, time, sock, size, pay, dst, pkt, end, boot)
            got = self.stage.advance(off, time, None, size, pay, dst, pkt, sock=sock, window_end=end, bootstrap_end=boot)
        else:
            want = self.model.advance(off, time, prio, sock, size, pay, dst, pkt, end, boot)
            got = self.stage.advance(off, time, prio, size, pay, dst, pkt, sock=sock, window_end=end, bootstrap_end=boot)
        _same(got, want)
        return want

    def states(self):
        from tests.test_outbound_gpu import _same_state as fifo_state
        from tests.test_outbound_rr_gpu import _same_state as rr_state
        from tests.test_outbound_sock_gpu import _same_state as sock_state
        for h, host in enumerate(self.model.hosts):
            if self.kind == "fifo":
                fifo_state(self.stage.state(h), host)
            else:
                (rr_state if self.kind == "round-robin" else sock_state)(self.stage, h, host)

    def rerate(self, entries, at):
        call(self.stage, entries, at)
        apply_model(self.model.hosts, entries, at)


def _offer(t, prio, sock, size, dst, pkt):
    return (t, prio, sock, size, size - HEADER, dst, pkt)


@pytest.mark.parametrize("kind", OUT_KINDS[1:])
def test_a_packet_that_has_left_does_not_count(engine, kind):
    """The 3000-byte packet has been sent; the pool slot it lay in was freed and still holds its
    size.  A capacity of 2000 covers what is stored now (1500 cached, 100 and 200 queued)."""
    o = Out(engine, kind, [big()])
    offers = [_offer(S, 1, A, 1000, 1, 0), _offer(S, 2, A, 3000, 1, 1), _offer(S, 3, A, 1500, 1, 2),
              _offer(S, 4, A, 100, 1, 3), _offer(S, 5, B, 200, 1, 4)]
    want = o.window([offers], S + 10 * MS)
    host = o.model.hosts[0]
    assert 1 in want["sent_pkt"].tolist() and host.cached is not None and host.cached[2] == 1500 and len(host.q) >= 1
    o.rerate([(0, 2000, 1, MS)], S + 10 * MS)
    o.states()
    refused(lambda: call(o.stage, [(0, 1499, 1, MS)], S + 10 * MS), host=0)   # (the cached one still counts)
    o.window([[]], S + 3000 * MS)
    o.states()
    assert host.stored() == 0


@pytest.mark.parametrize("kind", OUT_KINDS)
def test_a_queued_local_packet_is_exempt(engine, kind):
    """first_host 40: a 4000-byte packet to the host itself waits behind a blocked one.  It never
    meets the bucket, so a capacity of 2000 is accepted; the same size to another host is not."""
    first = 40
    o = Out(engine, kind, [big(), big()], first_host=first)
    offers = lambda h, far: [_offer(S, 1, A, 4900, 1, 10 * h), _offer(S, 2, A, 1500, 1, 10 * h + 1),  # noqa: E731
                             _offer(S, 3, A, 4000, far, 10 * h + 2), _offer(S, 4, B, 100, 1, 10 * h + 3)]
    want = o.window([offers(0, first), offers(1, first)], S + 10 * MS)   # host 1's big packet goes to host 0's id: not local
    assert 2 not in want["loc_pkt"].tolist() and 12 not in want["sent_pkt"].tolist()
    for h, host in enumerate(o.model.hosts):   # the big packet is still queued, behind the cached one
        assert host.cached is not None and host.cached[1] == 10 * h + 1 and host.stored() >= 2
    before = [o.stage.state(h) for h in range(2)]
    refused(lambda: call(o.stage, [(0, 2000, 1, MS), (1, 2000, 1, MS)], S + 10 * MS), host=1)
    assert [o.stage.state(h) for h in range(2)] == before
    o.rerate([(0, 2000, 1, MS)], S + 10 * MS)
    o.states()
    want = o.window([[], []], S + 6000 * MS)
    assert 2 in want["loc_pkt"].tolist()
    o.states()


# ---- random windows against the models ----

SLOW, FAST = [1000, 20_000], [125_000, 1_250_000]
N_HOSTS = [1, 63, 64, 65, 257]   # 257: past one 256-lane workgroup of the check and the apply


def _random_rows(rng, h):
    r = rng.random()
    return NONE if r < 0.2 else create_token_bucket(int(rng.choice(SLOW if (h % 2 == 0) == (r < 0.8) else FAST)))


def _random_entries(rng, n_hosts, buckets_now):
    """About a third of the hosts, one of them twice with other parameters, and hosts that switch
    to and from unlimited."""
    named = [h for h in range(n_hosts) if rng.random() < 0.35] or [0]
    entries = [(h, *_random_rows(rng, h)) for h in named]
    h = named[0]
    entries.append((h, *(create_token_bucket(20_000) if entries[0][1:] != create_token_bucket(20_000)
                         else create_token_bucket(1000))))
    switched = sum((buckets_now[e[0]] is None) != (e[1:] == NONE) for e in entries[1:-1])
    return entries, switched


@pytest.mark.parametrize("n_hosts", N_HOSTS)
def test_inbound_random_windows_with_rerates(engine, n_hosts):
    from tests.test_inbound_gpu import _random_window
    rng = np.random.default_rng(7000 + n_hosts)
    buckets = [None if rng.random() < 0.15 else (*create_token_bucket(int(rng.choice(SLOW if h % 2 == 0 else FAST))), S)
               for h in range(n_hosts)]
    stage, model = _in(engine, buckets)
    start, pid, switched = S, 0, 0
    for _ in range(4):
        end = start + int(rng.choice([20, 150])) * MS
        per_host, pid = _random_window(rng, model, start, end, pid)
        _in_window(stage, model, per_host, end, S + 5 * MS)
        entries, sw = _random_entries(rng, n_hosts, [x.tb for x in model.hosts])
        switched += sw
        call(stage, entries, end)
        apply_model(model.hosts, entries, end)
        _in_states(stage, model)
        start = end
    _in_window(stage, model, None, start + 400 * MS)
    _in_states(stage, model)
    assert model.counters["blocks"] > 0 and model.counters["carried"] > 0
    assert switched > 0 or n_hosts == 1


@pytest.mark.parametrize("kind", OUT_KINDS)
@pytest.mark.parametrize("n_hosts", N_HOSTS)
def test_outbound_random_windows_with_rerates(engine, n_hosts, kind):
    from tests.test_outbound_sock import random_window
    rng = np.random.default_rng(8000 + n_hosts)
    buckets = [None if rng.random() < 0.15 else (*create_token_bucket(int(rng.choice(SLOW if h % 2 == 0 else FAST))), S)
               for h in range(n_hosts)]
    if n_hosts == 1:
        buckets = [(*create_token_bucket(1000), S)]
    socks = [rng.integers(0, 2**64, int(rng.integers(1, 5)), dtype=np.uint64).tolist() for _ in range(n_hosts)]
    o = Out(engine, kind, buckets)
    prio = [1] * n_hosts
    start, pid, switched = S, 0, 0
    for _ in range(4):
        end = start + int(rng.choice([20, 150])) * MS
        # (plain FIFO: priorities are unique per host, so no control packets; at most 12 offers a host and window)
        per_host, pid = random_window(rng, o.model.hosts, socks, prio, start, end, pid, max_offers=12,
                                      control=0.0 if kind == "fifo" else 0.3, n_dst=max(n_hosts, 8))
        o.window(per_host, end, S + 5 * MS)
        entries, sw = _random_entries(rng, n_hosts, [x.tb for x in o.model.hosts])
        if n_hosts == 1:
            entries = [(0, *create_token_bucket(1000)), (0, *create_token_bucket(20_000))]
        switched += sw
        o.rerate(entries, end)
        o.states()
        start = end
    o.window([[] for _ in range(n_hosts)], start + 400 * MS)
    o.states()
    assert o.model.counters["blocks"] > 0 and o.model.counters["carried"] > 0
    assert switched > 0 or n_hosts == 1


# ---- the two-call window ----

def _window_offers(k, ws, we, H, prio):
    """Every window: each host offers a burst somewhere in the window (a tenth local)."""
    rng = np.random.default_rng(90 + k)
    per_host, pid = [], k * 100_000
    for h in range(H):
        n = int(rng.integers(1, 6)) if k < 3 else 0
        times = np.sort(rng.integers(ws, we, n)).tolist()
        offers = []
        for i, t in enumerate(times):
            dst = h if rng.random() < 0.1 else int(rng.integers(0, H))
            pay = int(rng.choice([0, 1448, 1448, int(rng.integers(1, 1449))]))
            offers.append((t, prio[h] + i, pay + HEADER, pay, dst, pid + i))
        prio[h] += n
        pid += n
        per_host.append(offers)
    return per_host


def _bandwidth_plan(k, H):
    """Window k's re-rate: hosts, down and up rates in bytes per second (None: as it is)."""
    rng = np.random.default_rng(190 + k)
    hosts = [h for h in range(H) if rng.random() < 0.4] or [0]
    hosts.append(hosts[0])   # named twice: the last entry counts
    pick = lambda: None if rng.random() < 0.3 else int(rng.choice([2000, 20_000, 125_000, 1_250_000]))  # noqa: E731
    return hosts, [pick() for _ in hosts], [pick() for _ in hosts]


def _apply_bandwidth(o, lo, hosts, down, up, at):
    """The plan on the oracle's models; ``hosts`` are indices from ``lo`` on."""
    for model, rates in ((o.im, down), (o.om, up)):
        last = {h: r for h, r in zip(hosts, rates) if r is not None}   # a skipped entry names no host in that direction
        apply_model(model.hosts, [(lo + h, *create_token_bucket(r)) for h, r in last.items()], at)


def test_window_update_bandwidth_between_close_and_open():
    """Four windows through open and close against the composed oracle, both stages re-rated after
    every close; then the refusals: an outbound refusal leaves the inbound buckets untouched, and a
    call while a window is open is a state error."""
    from shadow_amd.routing import Engine
    from tests.test_inbound_gpu import _same_state as in_state
    from tests.test_outbound_gpu import ChainOracle, _same_state as out_state, chain_case
    from tests.test_window_gpu import Parts, run_windows
    with Engine(0) as eng:
        o = ChainOracle(S + 10**12)
        _, _, _, _, rng0, out_b, in_b = chain_case()
        p = Parts(eng, o, rng0, out_b, in_b)
        prio = [0] * o.H
        ra = o.ra.get()
        we = S + 10**9
        skipped = 0
        for k in range(4):
            ws, we = we, we + ra
            run_windows(p, o, lambda _k, a, b, k=k: _window_offers(k, a, b, o.H, prio), 1, (ws, we), windows=[None])
            hosts, down, up = _bandwidth_plan(k, o.H)
            skipped += sum(d is None for d in down) + sum(u is None for u in up)
            p.win.update_bandwidth(hosts, down, up, we)
            _apply_bandwidth(o, 0, hosts, down, up, we)
            for h in range(o.H):
                out_state(p.ostage.state(h), o.om.hosts[h])
                in_state(p.istage.state(h), o.im.hosts[h])
        assert skipped > 0 and o.om.counters["blocks"] > 0 and o.om.counters["carried"] > 0
        assert o.im.counters["blocks"] > 0 and o.im.counters["carried"] > 0
        # The outbound stage's refusal alone: host h's bw_up bucket is first re-rated 50 ms ahead
        # (its inbound relay is idle and stays as it is), then both directions 10 ms ahead -- before
        # the outbound bucket's last refill, but not the inbound one's.
        h = next(h for h in range(o.H) if o.im.hosts[h].task is None and (o.om.hosts[h].task or IDLE) >= we + 50 * MS)
        p.win.update_bandwidth([h], [None], [20_000], we + 50 * MS)
        before = [(p.istage.state(x), p.ostage.state(x)) for x in range(o.H)]
        assert before[h][1]["bucket"]["last_refill"] == we + 50 * MS
        refused(lambda: p.win.update_bandwidth([h], [20_000], [20_000], we + 10 * MS), host=h)
        refused(lambda: p.win.update_bandwidth([o.H], [20_000], [None], we))        # index, in the direction that is skipped too
        refused(lambda: p.win.update_bandwidth([o.H], [None], [None], we))
        refused(lambda: p.win.update_bandwidth([0], [20_000], [20_000], we - 1))    # below the previous window_end
        assert [(p.istage.state(x), p.ostage.state(x)) for x in range(o.H)] == before
        p.win.open(we + ra)
        refused(lambda: p.win.update_bandwidth([0], [20_000], [20_000], we + ra), code="STATE")
        p.win.close(*(None,) * 7, 0, we + ra, o.end_time)
        p.win.update_bandwidth([0], [20_000], [None], we + ra)


def test_window_update_bandwidth_on_two_ranks():
    """Two in-process ranks, each re-rating hosts of its own shard by local index after every
    close: every rank's results are the one-context oracle's for its hosts."""
    from tests.test_outbound_gpu import ChainOracle, chain_case
    from tests.test_window_sharded_gpu import _run_ranks, _world, run_windows
    from tests.test_inbound_gpu import _same_state as in_state
    from tests.test_outbound_gpu import _same_state as out_state
    o = ChainOracle(S + 10**12)
    _, _, _, _, rng0, out_b, in_b = chain_case()
    engines, parts = _world(2, o, rng0, out_b, in_b)
    try:
        prio = [0] * o.H
        ra = o.ra.get()
        we = S + 10**9
        for k in range(3):
            ws, we = we, we + ra
            run_windows(parts, o, lambda _k, a, b, k=k: _window_offers(k, a, b, o.H, prio), 1, (ws, we))
            plans = [_bandwidth_plan(10 * k + i, p.hi - p.lo) for i, p in enumerate(parts)]
            _run_ranks([lambda p=p, pl=pl, we=we: p.win.update_bandwidth(*pl, we) for p, pl in zip(parts, plans)])
            for p, pl in zip(parts, plans):
                _apply_bandwidth(o, p.lo, *pl, we)
        assert o.om.counters["blocks"] > 0 and o.im.counters["blocks"] > 0
        for p in parts:
            for h in range(p.hi - p.lo):
                out_state(p.ostage.state(h), o.om.hosts[p.lo + h])
                in_state(p.istage.state(h), o.im.hosts[p.lo + h])
    finally:
        for e in engines:
            e.close()
