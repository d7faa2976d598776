"""CPU tier of the inbound stage: the model (tests/inbound_model.py, the oracle's CoDelQueue and
TokenBucket composed as Host::execute -> Router -> Relay -> forward task composes them) pinned on
hand vectors computed from the oracle.  tests/test_inbound_gpu.py runs the same cases on the
device."""
from oracle.token_bucket import SIM_START as S, create_token_bucket
from tests.inbound_model import DROPPED as DROP, FORWARDED as FWD, IDLE, InboundModel

MS = 10**6


def bucket(bps=1000, last=S):
    return (*create_token_bucket(bps), last)


def one_host(b):
    """A one-host model and step(events, window_end, bootstrap_end) -> (records, n_stored, next
    task) with every time an offset from S (events: [(time, size, pkt)])."""
    m = InboundModel([b])

    def step(events, window_end, bootstrap_end=0):
        off = [0, len(events)]
        _, pkt, time, kind, n_stored, nxt = m.advance(
            off, [S + t for t, _, _ in events], [s for _, s, _ in events], [p for _, _, p in events],
            S + window_end, bootstrap_end)
        recs = [(int(k), int(p), int(t) - S) for k, p, t in zip(kind, pkt, time)]
        return recs, n_stored, (None if nxt == IDLE else nxt - S)
    return m, step


# the hand cases, shared with the device tests: (bucket, [(events, window_end, bootstrap_end,
# records, n_stored, next task)], checks on the host's final state)
A1 = ([(0, 1500, 0), (0, 1500, 1)], 10 * MS, 0, [(FWD, 0, 0)], 1, 1499 * MS)
CASES = {
    "A": (bucket(), [A1, ([], 2000 * MS, 0, [(FWD, 1, 1499 * MS)], 0, None)],
          dict(task=None, cached=None, balance=0)),
    "A1": (bucket(), [A1], dict(task=1499 * MS, cached=1, balance=1)),
    "B": (bucket(), [(A1[0], 10 * MS, S + MS, [(FWD, 0, 0), (FWD, 1, 0)], 0, None)],
          dict(task=None, cached=None, balance=1501)),
    "C": (bucket(), [A1, ([(1499 * MS, 60, 2), (1499 * MS + 1, 60, 3)], 1600 * MS, 0,
                          [(FWD, 1, 1499 * MS), (FWD, 2, 1559 * MS)], 1, 1619 * MS)],
          dict(task=1619 * MS, cached=3, balance=0)),
    "D": (bucket(), [([(0, 1500, p) for p in range(20)], 10 * MS, 0, [(FWD, 0, 0)], 19, 1499 * MS),
                     ([], 12000 * MS, 0,
                      [(FWD, 1, 1499 * MS), (FWD, 2, 2999 * MS), (DROP, 3, 2999 * MS), (FWD, 4, 4499 * MS)] +
                      [(DROP, p, 4499 * MS) for p in range(5, 18)] +
                      [(FWD, 18, 5999 * MS), (FWD, 19, 7499 * MS)], 0, None)],
          dict(task=None, cached=None, balance=0, mode=0, current_drop_count=14, drop_next=3_587_853_447)),
    "E": (None, [([(5, 1500, 0), (5, 1500, 1), (9, 10, 2)], 10, 0, [(FWD, 0, 5), (FWD, 1, 5), (FWD, 2, 9)], 0, None)],
          dict(task=None, cached=None)),
}


def check_final(want, task, cached, balance, codel):
    """The case's checks against a host's final state (times as offsets from S)."""
    assert task == want["task"]
    assert cached == want["cached"]
    if "balance" in want:
        assert balance == want["balance"]
    for k in ("mode", "current_drop_count"):
        if k in want:
            assert codel[k] == want[k], k
    if "drop_next" in want:
        assert codel["drop_next"] - S == want["drop_next"]


def run_case(name):
    b, steps, final = CASES[name]
    m, step = one_host(b)
    for events, w_end, boot, recs, n_stored, nxt in steps:
        assert step(events, w_end, boot) == (recs, n_stored, nxt), name
    h = m.hosts[0]
    check_final(final, None if h.task is None else h.task - S, h.cached,
                h.tb.balance if h.tb is not None else None,
                dict(mode=h.q.mode, current_drop_count=h.q.current_drop_count, drop_next=h.q.drop_next))
    return m


def test_a_blocked_packet_is_cached_and_forwarded_by_the_next_task():
    run_case("A1")
    run_case("A")


def test_b_bootstrapping_bypasses_the_bucket():
    run_case("B")


def test_c_packet_at_the_tasks_own_time_is_pushed_before_the_task_runs():
    m = run_case("C")
    assert m.counters["ties"] == 2   # p1 at p0's task (both at 0), p2 at the carried task's time


def test_d_codel_drops_while_the_bucket_holds_the_queue_back():
    m = run_case("D")
    assert m.counters["drops"] == 14 and len(m.hosts[0].q) == 0


def test_e_no_bucket_forwards_at_each_notify():
    run_case("E")


def test_task_at_window_end_stays_outstanding():
    """A task exactly at window_end is not run (T < window_end); the next window runs it."""
    _, step = one_host(bucket())
    assert step(A1[0], 10 * MS) == ([(FWD, 0, 0)], 1, 1499 * MS)
    assert step([], 1499 * MS) == ([], 1, 1499 * MS)
    assert step([], 1499 * MS + 1) == ([(FWD, 1, 1499 * MS)], 0, None)
