"""GPU parity of the packet ledger (shadow_amd/ledger.py, csrc/ledger.hip) against the dict model
(tests/ledger_model.py), through the C ABI: the gathered sizes and ids and the stats after every
call, the refusals in the kernel and before it, and shd_outbound_sent_sizes."""
import ctypes as C

import numpy as np
import pytest

from tests.ledger_model import REFUSED, LedgerModel

pytestmark = pytest.mark.gpu

INVALID, STATE = 5, 9


class Pair:
    """The engine's ledger and the model, fed the same calls."""

    def __init__(self, engine, max_live=0, seed=5):
        from shadow_amd.ledger import PacketLedger
        self.eng, self.max_live = engine, max_live
        self.led = PacketLedger(engine, max_live)
        self.m = LedgerModel(max_live)
        self.rng = np.random.default_rng(seed)

    def record(self, batch, n, n_live=None):
        import torch
        size = self.rng.integers(52, 1501, n).astype(np.uint32)
        pkt = self.rng.integers(0, 2**32 - 1, n).astype(np.uint32)
        d = [torch.from_numpy(a.view(np.int32)).cuda() for a in (size, pkt)]
        torch.cuda.synchronize()
        n_live = n if n_live is None else n_live
        self.led.record(batch, d[0] if n else None, d[1] if n else None, n, n_live)
        torch.cuda.synchronize()   # the record reads the two arrays on the engine's stream and does not wait
        self.m.record(batch, size, pkt, n_live)
        self.same_stats()

    def gather(self, tag):
        size, pkt = self.led.gather(tag)
        ok, ws, wp = self.m.gather(tag)
        assert ok
        assert np.array_equal(size, ws) and np.array_equal(pkt, wp)
        self.same_stats()

    def same_stats(self):
        s = self.led.stats()
        assert (s.live_batches, s.live_events, s.entries_held, s.oldest_batch) == self.m.stats()

    def all_tags(self, batches=None):
        """Every live packet of the batches (default: all held), once."""
        t = [np.arange(len(self.m.held[b][0]), dtype=np.uint64) | (np.uint64(b) << np.uint64(32))
             for b in (batches if batches is not None else sorted(self.m.held))]
        return np.concatenate(t) if t else np.zeros(0, np.uint64)


def tags(*pairs):
    return np.array([(b << 32) | i for b, i in pairs], np.uint64)


def test_three_batches_mixed_order(engine):
    p = Pair(engine)
    p.record(0, 5)
    p.record(1, 1)
    p.record(2, 70)
    assert p.m.stats() == (3, 76, 76, 0)
    p.gather(tags((2, 69), (0, 0), (2, 0), (1, 0), (0, 4)))
    p.gather(tags())
    rest = p.rng.permutation(np.setdiff1d(p.all_tags(), tags((2, 69), (0, 0), (2, 0), (1, 0), (0, 4))))
    p.gather(rest[:40])
    p.gather(rest[40:])
    assert p.m.stats() == (0, 0, 0, None)


def test_out_of_order_drain_holds_the_entries(engine):
    p = Pair(engine)
    p.record(0, 6, 2)
    p.record(1, 9)
    p.record(2, 4)
    p.gather(p.all_tags([1]))      # batch 1 drains before batch 0: its 9 entries stay held
    assert p.m.stats() == (2, 6, 19, 0)
    p.gather(tags((0, 5), (0, 1)))   # batch 0 goes, and batch 1 with it
    assert p.m.stats() == (1, 4, 4, 2)


def test_arena_grows_with_its_contents_kept(engine):
    p = Pair(engine)
    p.record(0, 100)
    p.record(1, 200_000)           # past the arena's first 65,536 entries
    p.gather(p.rng.permutation(p.all_tags([0])))
    p.gather(p.rng.permutation(p.all_tags([1]))[:5000])
    p.record(2, 70_000)
    p.gather(p.all_tags([2])[::7])


def test_one_counter(engine):
    """100,000 tags of one batch in one gather: every pop lands on one counter."""
    p = Pair(engine)
    p.record(7, 100_000)
    p.gather(p.rng.permutation(p.all_tags()))
    assert p.m.stats() == (0, 0, 0, None)


def test_more_distinct_batches_than_lanes(engine):
    """65 x 3 tags, neighbouring lanes naming 65 different batches."""
    p = Pair(engine)
    for b in range(65):
        p.record(b, 3)
    p.gather(tags(*((b, i) for i in range(3) for b in range(65))))
    assert p.m.stats() == (0, 0, 0, None)


def test_1025_live_batches(engine):
    """More batches held than the gather keeps rows in LDS, numbers with gaps, one gather in
    random order; then the ledger goes on."""
    p = Pair(engine, 2048)
    numbers = [b + b // 300 for b in range(1025)]   # three numbers never recorded in between
    for b in numbers:
        p.record(b, 2)
    assert p.m.stats() == (1025, 2050, 2050, 0)
    t = p.rng.permutation(p.all_tags())
    p.gather(t[:2049])
    assert p.m.stats()[0] == 1
    p.gather(t[2049:])
    p.record(5000, 3)
    p.gather(p.all_tags())


def test_random_gather_past_one_scan_tile(engine):
    p = Pair(engine)
    for b, n in enumerate((100_000, 50_000, 1, 70_000, 30_000, 49_000, 999)):
        p.record(10 + 2 * b, n)
    t = p.rng.permutation(p.all_tags())
    assert len(t) == 300_000
    p.gather(t)
    assert p.m.stats() == (0, 0, 0, None)


def test_no_live_event_stores_nothing(engine):
    p = Pair(engine)
    p.record(0, 4, 0)
    assert p.m.stats() == (0, 0, 0, None)
    p.record(1, 0, 0)
    p.record(2, 3, 1)
    p.gather(tags((2, 1)))
    assert p.m.stats() == (0, 0, 0, None)


def _three(p):
    """Batches 0 (drained, gone), 1 (4 packets, 2 live), 2 (3 packets, drained but held behind
    1), 4 (2 packets): the oldest held is 1, number 3 was never recorded."""
    p.record(0, 2)
    p.record(1, 4, 2)
    p.record(2, 3, 1)
    p.record(4, 2)
    p.gather(tags((0, 0), (0, 1), (2, 2)))
    assert p.m.stats() == (2, 4, 9, 1)


@pytest.mark.parametrize("bad", [(0, 0), (3, 0), (9, 0), (2, 0), (1, 4), (4, 2**32 - 1), (2**32 - 1, 0)],
                         ids=["older-than-oldest", "never-recorded", "above-newest", "retired", "index-past-batch",
                              "index-max", "batch-max"])
def test_refused_in_the_kernel(engine, bad):
    p = Pair(engine)
    _three(p)
    t = tags((1, 3), bad, (4, 0), (4, 1))
    st, size, pkt = p.led.gather(t, check=False)
    ok, ws, wp = p.m.gather(t)
    assert st == INVALID and not ok
    assert ws[1] == REFUSED and (ws[[0, 2, 3]] != REFUSED).all()
    assert np.array_equal(size, ws) and np.array_equal(pkt, wp)
    _dead_until_setup(p)


def test_overdrawn_batch_is_refused(engine):
    """Batch 1 has 2 live events and is named 3 times in one gather: at least the surplus event is
    refused, every other event of the batch is right or refused, the other batches are right."""
    p = Pair(engine)
    _three(p)
    t = tags((1, 0), (4, 1), (1, 3), (1, 0))
    st, size, pkt = p.led.gather(t, check=False)
    ok, ws, wp = p.m.gather(t)
    assert st == INVALID and not ok and p.m.overdrawn == {1: [0, 2, 3]}
    assert (size[1], pkt[1]) == (p.m.held[4][0][1], p.m.held[4][1][1])
    refused = 0
    for k, i in ((0, 0), (2, 3), (3, 0)):
        got = (size[k], pkt[k])
        assert got in ((REFUSED, REFUSED), (p.m.held[1][0][i], p.m.held[1][1][i]))
        refused += got == (REFUSED, REFUSED)
    assert refused >= 1
    _dead_until_setup(p)


def _dead_until_setup(p):
    import torch
    lib, ctx = p.eng.lib, p.eng.ctx
    d = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    out = (C.c_void_p(), C.c_void_p())
    assert lib.shd_ledger_gather(ctx, C.c_void_p(d.data_ptr()), 1, C.byref(out[0]), C.byref(out[1])) == STATE
    assert lib.shd_ledger_gather(ctx, None, 0, None, None) == STATE
    assert lib.shd_ledger_record(ctx, 100, C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()), 1, 1) == STATE
    assert lib.shd_ledger_stats(ctx, None, None, None, None) == STATE
    q = Pair(p.eng)
    q.record(0, 3)
    q.gather(tags((0, 2), (0, 0)))


def test_refused_before_anything_runs(engine):
    import torch
    lib, ctx = engine.lib, engine.ctx
    p = Pair(engine, 2)
    p.record(5, 3)
    p.record(6, 2)
    d = torch.arange(8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dp = C.c_void_p(d.data_ptr())
    out = (C.c_void_p(), C.c_void_p())
    assert lib.shd_ledger_gather(ctx, None, 1, C.byref(out[0]), C.byref(out[1])) == INVALID
    assert lib.shd_ledger_record(ctx, 7, None, dp, 2, 1) == INVALID     # a NULL array
    assert lib.shd_ledger_record(ctx, 7, dp, None, 2, 1) == INVALID
    assert lib.shd_ledger_record(ctx, 6, dp, dp, 2, 1) == INVALID       # not above the last number
    assert lib.shd_ledger_record(ctx, 2, dp, dp, 2, 1) == INVALID
    assert lib.shd_ledger_record(ctx, 7, dp, dp, 2, 1) == INVALID       # a third batch: max_live_batches is 2
    assert lib.shd_ledger_record(ctx, 2**32 - 1, dp, dp, 2, 1) == INVALID
    assert lib.shd_ledger_setup(ctx, 4097) == INVALID
    p.same_stats()                                   # ... and the ledger is as it was
    p.gather(tags((6, 1), (5, 0), (5, 2), (5, 1)))   # batch 5 gone: batch 7 has a row now
    p.record(7, 4)
    p.gather(tags((7, 3), (6, 0), (7, 0)))
    assert p.m.stats() == (1, 2, 4, 7)


def test_next_batch_counts_the_non_null_batches(engine):
    from shadow_amd.equeue import EventQueues
    from shadow_amd.ledger import PacketLedger
    q = EventQueues(engine, 3)
    led = PacketLedger(engine)
    assert led.next_batch() == 0
    q.advance(window_end=10)
    assert led.next_batch() == 0
    p = q.advance(np.array([0, 1, 1, 2], np.uint32), np.array([15, 50], np.uint64), np.array([1, 2], np.uint32),
                  np.array([0, 0], np.uint64), np.array([1, 0], np.uint32), window_end=20)
    assert led.next_batch() == 1 and p.tag.tolist() == [1]
    q.advance(window_end=30)
    assert led.next_batch() == 1


def test_sent_sizes_of_a_random_outbound_window(engine):
    """shd_outbound_sent_sizes after a random window (blocked hosts, local packets, priorities
    out of order) and after the window that drains what it left: entry i is the size of the offer
    that sent_pkt[i] names."""
    from oracle.token_bucket import SIM_START as S, create_token_bucket
    from tests.outbound_model import OutboundModel
    from tests.test_outbound_gpu import MS, RATES, _arrays, _random_window, _stage
    lib, ctx = engine.lib, engine.ctx
    rng = np.random.default_rng(411)
    n_hosts = 70
    buckets = [None if rng.random() < 0.1 else (*create_token_bucket(int(rng.choice(RATES))), S) for _ in range(n_hosts)]
    d = C.c_void_p(1)
    stage = _stage(engine, buckets)
    assert lib.shd_outbound_sent_sizes(ctx, C.byref(d)) == 0 and d.value is None   # before the first advance
    model = OutboundModel(buckets)
    per_host, _ = _random_window(rng, model, S, S + 20 * MS, 0, [0] * n_hosts)
    size_of = {x[5]: x[2] for offers in per_host for x in offers}
    total = 0
    for arr, end in ((_arrays(per_host), S + 20 * MS), ((None,) * 7, S + 10**6 * MS)):
        r = stage.advance(*arr, window_end=end)
        assert lib.shd_outbound_sent_sizes(ctx, C.byref(d)) == 0
        got = np.zeros(len(r.sent_pkt), np.uint32)
        if len(got):
            assert lib.shd_copy_to_host(ctx, got.ctypes.data_as(C.c_void_p), d, got.nbytes) == 0
        assert got.tolist() == [size_of[p] for p in r.sent_pkt.tolist()]
        total += len(got)
    assert total > 500 and r.n_stored == 0
    # a contract error (an offer before the last window's end) kills the stage: STATE, as get_state
    bad = _arrays([[(S, 10**6, 100, 48, 1, 10**6)]] + [[] for _ in range(n_hosts - 1)])
    with pytest.raises(Exception, match="INVALID"):
        stage.advance(*bad, window_end=S + 2 * 10**6 * MS)
    assert lib.shd_outbound_sent_sizes(ctx, C.byref(d)) == STATE
    assert lib.shd_outbound_get_state(ctx, 0, *(None,) * 7) == STATE
