"""GPU parity of shd_offers_group (shadow_amd/csrc/offers.hip): the worker threads' staged offers
grouped by host on the device, all eight outputs copied back, against the numpy group-by -- the
grouped columns the stages were dealt from (tests/test_offers.py holds the staging against the
stable group-by).  Every comparison is exact and covers every element."""
import numpy as np
import pytest

from tests.test_offers import BASE, random_offers, same_grouped, stage

pytestmark = pytest.mark.gpu

EDGES = [0, 1, 0, 63, 64, 0, 65, 200]          # run lengths on neighbouring hosts: the wave-stride loop's edges
HAS_RUN = [True, True, False, True, True, False, True, True]   # ... hosts 2 and 5 without a run, host 0 a run of 0


def _outbound(engine, n_hosts, first_host, qdisc):
    from shadow_amd.outbound import OutboundStage
    z = np.zeros(n_hosts, np.uint64)
    return OutboundStage(engine, z, z, z, first_host=first_host, ring_capacity=8, qdisc=qdisc, max_sockets=4)


def _case(n_hosts, n_threads, idle, words, first_host, every_host=False, seed=1):
    from shadow_amd.outbound import OfferStages
    rng = np.random.default_rng(seed + n_hosts)
    lengths = EDGES[:n_hosts] if n_hosts >= 5 else [3][:n_hosts]
    cols = random_offers(rng, n_hosts, lengths=lengths, max_per_host=3 if n_hosts > 1000 else 6)
    keep = rng.random(n_hosts) < 0.5
    keep[:len(lengths)] = HAS_RUN[:len(lengths)]
    if every_host:
        keep[:] = True
    st = OfferStages.from_grouped(*cols[:7], time_base=BASE, n_threads=n_threads, first_host=first_host,
                                  sock=cols[7] if words == 10 else None, words=words, idle=idle, seed=seed,
                                  keep_empty=keep)
    return cols, st


# (hosts, threads, idle threads, buffers, width, first_host, qdisc, every host a run)
CASES = [
    (1, 1, (), "pinned", 8, 0, "fifo", False),
    (5, 3, (0,), "pageable", 10, 700, "fifo-sockets", False),
    (5, 16, (15,), "pinned", 8, 700, "round-robin", False),
    (300, 3, (1,), "mixed", 8, 0, "fifo", False),
    (300, 16, (0, 7, 15), "pinned", 10, 700, "round-robin-sockets", False),
    (300, 3, (2,), "pinned-copy", 10, 0, "fifo-sockets", False),
    (300, 1, (), "pinned", 10, 0, "round-robin", False),         # width 10 under a plain discipline
    (8193, 16, (0,), "pinned", 8, 0, "fifo", False),             # d_off's 8194 entries pass one 8192-entry scan tile
    (8193, 3, (), "pageable", 10, 700, "fifo-sockets", False),
    (9001, 3, (1,), "pinned", 10, 700, "fifo-sockets", True),    # 9001 runs: the run scan passes one tile too
    (9001, 16, (), "pinned-copy", 8, 0, "fifo", True),
]


@pytest.mark.parametrize("n_hosts,n_threads,idle,buffers,words,first_host,qdisc,every_host", CASES)
def test_group_vs_numpy(engine, knob, n_hosts, n_threads, idle, buffers, words, first_host, qdisc, every_host):
    cols, st = _case(n_hosts, n_threads, idle, words, first_host, every_host)
    n_runs = sum(len(h) for h in st.run_host)
    assert (n_runs > 8192) == every_host and (n_runs < n_hosts or every_host or n_hosts == 1)
    assert int(cols[1].min()) > 2**32 and int((cols[1] - np.uint64(BASE)).max()) == 2**32 - 1
    ostage = _outbound(engine, n_hosts, first_host, qdisc)
    knob("FLUSH_COPY", 1 if buffers == "pinned-copy" else 0)
    busy = [k for k in range(n_threads) if k not in idle]
    held = st if buffers == "pageable" else st.pinned(engine.lib, None if buffers != "mixed" else set(busy[1:]))
    try:
        g = ostage.group_stages(held, BASE)
        assert g.n_offers == st.n_offers and (g.d_sock is None) == (words == 8)
        same_grouped(ostage.grouped_host(g), cols, words)
    finally:
        held.free()


def _state(ostage, hosts):
    return [ostage.state(h) for h in hosts]


def _code(fn):
    from shadow_amd._native import ShdError
    try:
        fn()
        return "OK"
    except ShdError as e:
        return e.code


def _bent(st, **kw):
    """A copy of the stages with one stage's run_host / run_count replaced (name=(stage, array))."""
    from shadow_amd.outbound import OfferStages
    lists = {"run_host": list(st.run_host), "run_count": list(st.run_count)}
    for k, v in kw.items():
        lists[k][v[0]] = v[1]
    return OfferStages(lists["run_host"], lists["run_count"], st.offers, st.words)


@pytest.mark.parametrize("pinned", [False, True])
def test_refusals_change_nothing(engine, pinned):
    """Every refusal of the header, on a stage that holds queued packets: the outbound state of a few
    hosts is what it was, and a correct group goes through afterwards."""
    from oracle.token_bucket import SIM_START as S
    from shadow_amd.outbound import OfferStages, OutboundStage
    from shadow_amd.routing import Engine
    from tests.test_outbound import bucket
    H, first = 40, 700
    rows = [bucket(1000)] * H   # 1 kB/s: the packets stay queued
    cap, inc, itv, last = (np.array([r[i] for r in rows], np.uint64) for i in range(4))
    rng = np.random.default_rng(3)
    cols = random_offers(rng, H, lengths=[2, 3, 1])
    st = stage(cols, 3, 10, first_host=first)
    assert all(len(h) >= 2 for h in st.run_host)

    def fresh(qdisc):
        o = OutboundStage(engine, cap, inc, itv, last, first_host=first, ring_capacity=64, qdisc=qdisc, max_sockets=8)
        n = 3 * H   # three full packets per host at once: the bucket lets the first through at most
        off = 3 * np.arange(H + 1, dtype=np.uint32)
        t = S + 5 + np.tile(np.arange(3, dtype=np.uint64), H)
        o.advance(off, t, np.arange(1, n + 1, dtype=np.uint64), np.full(n, 1500, np.uint32), np.full(n, 1448, np.uint32),
                  np.zeros(n, np.uint32), np.arange(n, dtype=np.uint32), window_end=S + 10,
                  sock=np.arange(n, dtype=np.uint64) % 2 if "sockets" in qdisc else None)
        return o

    with Engine(0) as bare:   # no outbound stage on this context
        from shadow_amd.outbound import group_stages
        assert _code(lambda: group_stages(bare, st, BASE)) == "STATE"

    ostage = fresh("fifo-sockets")
    hosts = (0, 1, 17, H - 1)
    before = _state(ostage, hosts)
    assert any(s["queue_len"] or s["cached"] for s in before)
    two30 = np.array([2**30, 2**30], np.uint32)
    some = int(st.run_host[0][0])
    bad = {
        "a host below first_host": (_bent(st, run_host=(1, np.r_[first - 1, st.run_host[1][1:]].astype(np.uint32))), "NO_HOST"),
        "a host past the range": (_bent(st, run_host=(2, np.r_[first + H, st.run_host[2][1:]].astype(np.uint32))), "NO_HOST"),
        "a host with two runs, two stages": (_bent(st, run_host=(1, np.r_[some, st.run_host[1][1:]].astype(np.uint32))), "INVALID"),
        "a host with two runs, one stage": (_bent(st, run_host=(0, np.r_[some, some, st.run_host[0][2:]].astype(np.uint32))), "INVALID"),
        "counts that do not add up": (_bent(st, run_count=(1, st.run_count[1] + np.uint32(1))), "INVALID"),
        "offer_words 7": (_bent(st), "INVALID"),
        "offer_words 8 under a socket discipline": (stage(cols, 3, 8, first_host=first), "INVALID"),
        "2^32 offers": (OfferStages([st.run_host[0][:2], st.run_host[1][:2]], [two30, two30],
                                    [np.zeros((0, 10), np.uint32)] * 2, 10), "INVALID"),
    }
    for name, (b, want) in bad.items():
        held = b.pinned(engine.lib) if pinned else b
        if name == "offer_words 7":
            held.words = 7
        if name == "2^32 offers":
            held.stage_offers[0] = held.stage_offers[1] = 2**31   # 2^32 in all; refused before any array is read
        try:
            assert _code(lambda: ostage.group_stages(held, BASE)) == want, name
        finally:
            held.free()
        assert _state(ostage, hosts) == before, name
    # C arguments alone: a NULL array with a count, 2^32 runs (the totals are refused before any array is read)
    for name, field in (("run_host", "p_host"), ("run_count", "p_count"), ("offers", "p_offers")):
        b = _bent(st)
        getattr(b, field)[1] = None
        assert _code(lambda: ostage.group_stages(b, BASE)) == "INVALID", name
    b = _bent(st)
    b.stage_runs[0] = b.stage_runs[1] = 2**31
    assert _code(lambda: ostage.group_stages(b, BASE)) == "INVALID"
    assert _state(ostage, hosts) == before
    # ... and the correct group goes through, and the stage takes it
    held = st.pinned(engine.lib) if pinned else st
    try:
        g = ostage.group_stages(held, BASE)
        same_grouped(ostage.grouped_host(g), cols, 10)
    finally:
        held.free()
    assert _state(ostage, hosts) == before
    # width 10 under a plain discipline is accepted, width 8 too
    plain = fresh("fifo")
    for words in (8, 10):
        g = plain.group_stages(stage(cols, 3, words, first_host=first), BASE)
        same_grouped(plain.grouped_host(g), cols, words)


@pytest.mark.parametrize("words", [8, 10])
def test_pinned_records_not_8_aligned(engine, knob, words):
    """Stages carved out of a pinned arena at a 4-byte boundary: the gather reads those records
    word by word (its other form takes 8 bytes at a time)."""
    import ctypes as C
    cols, st = _case(300, 3, (), words, 0)
    ostage = _outbound(engine, 300, 0, "fifo-sockets" if words == 10 else "fifo")
    knob("FLUSH_COPY", 0)
    held = st.pinned(engine.lib)
    arenas = []
    try:
        for k, rec in enumerate(st.offers):
            arenas.append(engine.lib.shd_host_alloc(rec.nbytes + 4))
            assert arenas[-1] and arenas[-1] % 8 == 0
            C.memmove(arenas[-1] + 4, rec.ctypes.data, rec.nbytes)
            held.p_offers[k] = arenas[-1] + 4
        g = ostage.group_stages(held, BASE)
        same_grouped(ostage.grouped_host(g), cols, words)
    finally:
        held.free()
        for p in arenas:
            engine.lib.shd_host_free(p)
