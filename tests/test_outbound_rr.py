"""CPU tier of the outbound stage's round-robin discipline: the model (tests/outbound_rr_model.py,
the reference's rrQueue restated under the FIFO model's relay loop) pinned on hand vectors worked
out from network_interface.c:235-273 / :366-392 and token_bucket.rs; the random-window generator
the device tests use, held to the conditions it is there to produce; and rr_queue.h -- the queue
the kernel compiles -- as a program of its own under the sanitizers, against the model's
interface.  tests/test_outbound_rr_gpu.py runs the hand vectors and the generator on the device."""
import os
import subprocess

import numpy as np
import pytest

from oracle.token_bucket import SIM_START as S, create_token_bucket
from tests.outbound_rr_model import IDLE, LOCAL, SENT, RR_COUNTERS, RrInterface, RrOutboundModel
from tests.test_outbound import MS, arrays, bucket, check_final, payload_of, records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B, C = 0x7F00_0000_1000, 0, 2**64 - 1   # canonical handles: compared for equality only, any value

# The hand cases, shared with the device tests: (bucket, first_host, [(offers [(time, handle, size,
# dst, pkt)], window_end, bootstrap_end, records (SENT first, then LOCAL), n_stored, next task,
# the rrQueue after the window [(handle, packets)])], checks on the final state).  The bucket is
# 1000 B/s = (1501, 1, 1 ms): a full packet at S leaves 1 token, and from a refill boundary a
# packet of n bytes that finds the bucket empty waits n ms.
FULL, SMALL = 1500, 100
RR_CASES = {
    # rrQueue [A(p0 p1 p2), B(p3 p4)].  0: A gives p0 (sent, 1 token left) and goes behind B; B gives
    # p3, which misses 99 tokens -- cached, and B has already gone behind A: [A(p1 p2), B(p4)].
    # 99 ms: p3 leaves, A gives p1 (100 ms) -> [B(p4), A(p2)]; 199: p1, B gives p4 -> [A(p2)];
    # 299: p4, A gives p2 and leaves; 399: p2.  FIFO would send 0 1 2 3 4.
    "two_sockets_alternate": (bucket(), 0, [
        ([(0, A, FULL, 1, 0), (0, A, SMALL, 1, 1), (0, A, SMALL, 1, 2), (0, B, SMALL, 1, 3), (0, B, SMALL, 1, 4)],
         1000 * MS, 0,
         [(SENT, 0, 0), (SENT, 3, 99 * MS), (SENT, 1, 199 * MS), (SENT, 4, 299 * MS), (SENT, 2, 399 * MS)], 0, None,
         [])], dict(task=None, cached=None, balance=0, queue_len=0)),
    # The same offers, the windows cut while a packet is cached: after the first p3 is cached and
    # its socket B stands behind A already, with p4 alone; the block over, the cached p3 goes
    # first and the rotation continues from A, now at the head.
    "cached_packet_whose_socket_has_rotated": (bucket(), 0, [
        ([(0, A, FULL, 1, 0), (0, A, SMALL, 1, 1), (0, A, SMALL, 1, 2), (0, B, SMALL, 1, 3), (0, B, SMALL, 1, 4)],
         50 * MS, 0, [(SENT, 0, 0)], 4, 99 * MS, [(A, 2), (B, 1)]),
        ([], 250 * MS, 0, [(SENT, 3, 99 * MS), (SENT, 1, 199 * MS)], 2, 299 * MS, [(A, 1)]),
        ([], 1000 * MS, 0, [(SENT, 4, 299 * MS), (SENT, 2, 399 * MS)], 0, None, [])],
        dict(task=None, cached=None, balance=0, queue_len=0)),
    # [A(p0 p1 p2), B(p3)].  0: p0; B gives p3 (cached) and leaves: [A(p1 p2)].  50 ms: C joins
    # behind A: [A, C(p5)].  99: p3, A gives p1 -> [C, A(p2)]; 199: p1, C gives p5; 299: p5, p2; 399: p2.
    "a_socket_that_joins_waits_for_those_queued": (bucket(), 0, [
        ([(0, A, FULL, 1, 0), (0, A, SMALL, 1, 1), (0, A, SMALL, 1, 2), (0, B, SMALL, 1, 3), (50 * MS, C, SMALL, 1, 5)],
         150 * MS, 0, [(SENT, 0, 0), (SENT, 3, 99 * MS)], 3, 199 * MS, [(C, 1), (A, 1)]),
        ([], 1000 * MS, 0, [(SENT, 1, 199 * MS), (SENT, 5, 299 * MS), (SENT, 2, 399 * MS)], 0, None, [])],
        dict(task=None, cached=None, balance=0, queue_len=0)),
    # [A(p0 p1), B(p2 p3)].  0: p0; B gives p2 (cached) -> [A(p1), B(p3)].  99: p2, A gives p1 and
    # leaves: [B(p3)].  150 ms: A is offered p4 and re-enters behind B.  199: p1, B gives p3;
    # 299: p3, A gives p4; 399: p4.
    "a_drained_socket_re_enters_at_the_tail": (bucket(), 0, [
        ([(0, A, FULL, 1, 0), (0, A, SMALL, 1, 1), (0, B, SMALL, 1, 2), (0, B, SMALL, 1, 3), (150 * MS, A, SMALL, 1, 4)],
         160 * MS, 0, [(SENT, 0, 0), (SENT, 2, 99 * MS)], 3, 199 * MS, [(B, 1), (A, 1)]),
        ([], 1000 * MS, 0, [(SENT, 1, 199 * MS), (SENT, 3, 299 * MS), (SENT, 4, 399 * MS)], 0, None, [])],
        dict(task=None, cached=None, balance=0, queue_len=0)),
    # host 7.  [A(p0 p1), B(p2)]: p0 leaves 1 token; B's p2 is local and leaves all the same; A's
    # p1 misses 99 tokens.
    "local_packet_leaves_without_the_bucket": (bucket(), 7, [
        ([(0, A, FULL, 1, 0), (0, A, SMALL, 1, 1), (0, B, FULL, 7, 2)], 10 * MS, 0,
         [(SENT, 0, 0), (LOCAL, 2, 0)], 1, 99 * MS, [])],
        dict(task=99 * MS, cached=1, balance=1, queue_len=0)),
    # p1 is cached until 1499 ms.  B's p2 and p3 and A's p4 are offered at exactly that time: all
    # three are queued before the task runs -- [B(p2 p3), A(p4)] -- so it forwards p1 and takes
    # p2 (60 ms); 1559: p2, A gives p4 (60 ms, past the window): [B(p3)].
    "offer_at_the_tasks_time": (bucket(), 0, [
        ([(0, A, FULL, 1, 0), (0, A, FULL, 1, 1)], 10 * MS, 0, [(SENT, 0, 0)], 1, 1499 * MS, []),
        ([(1499 * MS, B, 60, 1, 2), (1499 * MS, B, 60, 1, 3), (1499 * MS, A, 60, 1, 4)], 1600 * MS, 0,
         [(SENT, 1, 1499 * MS), (SENT, 2, 1559 * MS)], 2, 1619 * MS, [(B, 1)])],
        dict(task=1619 * MS, cached=4, balance=0, queue_len=1)),
    # a task exactly at window_end is not run; the next window runs it
    "task_at_window_end_is_carried": (bucket(), 0, [
        ([(0, A, FULL, 1, 0), (0, B, FULL, 1, 1)], 10 * MS, 0, [(SENT, 0, 0)], 1, 1499 * MS, []),
        ([], 1499 * MS, 0, [], 1, 1499 * MS, []),
        ([], 1499 * MS + 1, 0, [(SENT, 1, 1499 * MS)], 0, None, [])],
        dict(task=None, cached=None, balance=0, queue_len=0)),
    # the task runs before bootstrap_end: three full packets in rotation order, the bucket untouched
    "bootstrap": (bucket(), 0, [
        ([(0, A, FULL, 1, 0), (0, A, FULL, 1, 1), (0, B, FULL, 1, 2)], 10 * MS, S + MS,
         [(SENT, 0, 0), (SENT, 2, 0), (SENT, 1, 0)], 0, None, [])],
        dict(task=None, cached=None, balance=1501, queue_len=0)),
}


def run_rr_case(name):
    b, first, steps, final = RR_CASES[name]
    m = RrOutboundModel([b], first)
    for offers, w_end, boot, recs, n_stored, nxt, socks in steps:
        r = m.advance(*arrays([[(S + t, hd, s, d, p) for t, hd, s, d, p in offers]]), S + w_end, boot)
        a, z = int(r["src_off"][0]), int(r["src_off"][1])
        assert r["payload"][a:z].tolist() == [payload_of(int(p)) for p in r["sent_pkt"][a:z]]
        got = [(k, p, t - S) for k, p, t in records(r)]
        nx = r["next_task_time"]
        assert (got, r["n_stored"], None if nx == IDLE else nx - S) == (recs, n_stored, nxt), name
        assert m.hosts[0].q.listing() == socks, name
    h = m.hosts[0]
    check_final(final, None if h.task is None else h.task - S, None if h.cached is None else h.cached[1],
                h.tb.balance if h.tb is not None else None, len(h.q))
    return m


def test_two_sockets_alternate_while_the_bucket_holds_the_host_back():
    m = run_rr_case("two_sockets_alternate")
    assert m.counters["not_in_offer_order"] == 2 and m.counters["blocks"] == 4   # p3 before p1, p4 before p2


def test_cached_packet_stays_while_its_socket_has_rotated():
    m = run_rr_case("cached_packet_whose_socket_has_rotated")
    # p3 is cached with B queued behind A, p1 with A queued behind B; p4 and p2 were their sockets' last
    assert m.counters["blocked_rotated"] == 2 and m.counters["carried"] == 2


def test_a_socket_that_joins_is_served_after_every_socket_queued():
    m = run_rr_case("a_socket_that_joins_waits_for_those_queued")
    assert m.counters["joins"] == 2   # B behind A at the start, C behind A at 50 ms


def test_a_drained_socket_re_enters_at_the_tail():
    m = run_rr_case("a_drained_socket_re_enters_at_the_tail")
    assert m.counters["reentries"] == 1


def test_local_packet_leaves_without_the_bucket():
    m = run_rr_case("local_packet_leaves_without_the_bucket")
    assert m.counters["local_forwards"] == 1 and m.hosts[0].tb.balance == 1


def test_offer_at_the_tasks_own_time_is_inserted_before_the_task_runs():
    m = run_rr_case("offer_at_the_tasks_time")
    assert m.counters["ties"] == 4   # p1 at p0's task, p2 p3 p4 at the carried task's time


def test_task_at_window_end_is_carried():
    m = run_rr_case("task_at_window_end_is_carried")
    assert m.counters["carried"] == 2


def test_bootstrapping_bypasses_the_bucket():
    m = run_rr_case("bootstrap")
    assert m.counters["boot_forwards"] == 3 and m.counters["blocks"] == 0


# ---- the random windows of the device tests -------------------------------------------------

HEADER = 52
RATES = [0, 1000, 20_000, 125_000, 1_250_000, 125_000_000]
GEN_SEEDS = tuple(range(6))
GEN_CAPACITY, GEN_MAX_SOCKETS = 64, 6


def random_setup(seed):
    """The host count, buckets and each host's sockets (1-6 handles) of one seed."""
    rng = np.random.default_rng(2611 + seed)
    n_hosts = int(rng.integers(30, 299))
    buckets = [None if rng.random() < 0.1 else (*create_token_bucket(int(rng.choice(RATES))), S)
               for _ in range(n_hosts)]
    socks = [rng.integers(0, 2**64, int(rng.integers(1, GEN_MAX_SOCKETS + 1)), dtype=np.uint64).tolist()
             for _ in range(n_hosts)]
    ends = (np.cumsum([int(rng.choice([1, 20, 150, 400])) * MS for _ in range(5)]) + S).tolist()
    return rng, n_hosts, buckets, socks, ends


def random_window(rng, model, socks, start, end, pid, capacity=GEN_CAPACITY, max_offers=40, n_dst=None):
    """Offers for every host of the model in [start, end), each on one of the host's sockets
    (bursts of one socket and single packets mixed): 10 % local, half the hosts with a same-instant
    pair, half of the pending ones with an offer at the outstanding task's time.  A host is never
    offered more than its queue can still take, so `capacity` holds whatever the bucket does."""
    per_host = []
    n_dst = n_dst or len(model.hosts)
    for h, host in enumerate(model.hosts):
        n = min(int(rng.integers(0, max_offers + 1)), capacity - len(host.q))
        times = np.sort(rng.integers(start, end, n)).tolist()
        if n >= 2 and rng.random() < 0.5:
            times[1] = times[0]
        if n and host.task is not None and start <= host.task < end and rng.random() < 0.5:
            times[int(rng.integers(0, n))] = host.task
            times.sort()
        offers, hd = [], None
        for i, t in enumerate(times):
            if hd is None or rng.random() < 0.6:
                hd = socks[h][int(rng.integers(0, len(socks[h])))]
            dst = host.id if rng.random() < 0.1 else int(rng.integers(0, n_dst))
            pay = int(rng.integers(0, 1449))
            offers.append((t, hd, pay + HEADER, pay, dst, pid + i))
        per_host.append(offers)
        pid += n
    return per_host, pid


def np_arrays(per_host):
    """[[(time, handle, size, payload, dst, pkt)] per host] -> off, time, handle, size, payload, dst, pkt."""
    off = np.zeros(len(per_host) + 1, np.uint32)
    off[1:] = np.cumsum([len(e) for e in per_host])
    flat = [x for e in per_host for x in e]
    col = lambda i, dt: np.array([x[i] for x in flat], dt)  # noqa: E731
    return (off, col(0, np.uint64), col(1, np.uint64), col(2, np.uint32), col(3, np.uint32), col(4, np.uint32),
            col(5, np.uint32))


def run_seed(seed, each_window=None):
    """The five windows of one seed through the model; each_window(arr, end, boot, want, model)."""
    rng, n_hosts, buckets, socks, ends = random_setup(seed)
    model = RrOutboundModel(buckets)
    boot = int(ends[0] + (ends[1] - ends[0]) // 2)
    start, pid = S, 0
    for end in ends:
        per_host, pid = random_window(rng, model, socks, start, end, pid)
        arr = np_arrays(per_host)
        want = model.advance(*arr, end, boot)
        if each_window:
            each_window(arr, end, boot, want, model)
        start = end
    return model


def test_the_generator_reaches_what_the_device_tests_need():
    """Over the seeds: every branch of the relay loop and every round-robin condition is met, some
    host has exactly max_sockets sockets queued at once, some host sends more packets than its
    pool has slots (slots are reused), and no host is ever past its capacity.  Each seed alone
    pops out of offer order: a stage that ran FIFO would differ from the model on every one."""
    total = {}
    models = [run_seed(seed) for seed in GEN_SEEDS]
    for m in models:
        assert m.counters["not_in_offer_order"] > 0 and m.counters["blocked_rotated"] > 0, m.counters
        for k, v in m.counters.items():
            total[k] = total.get(k, 0) + v
    assert set(RR_COUNTERS) <= set(total)
    for k, v in total.items():
        assert v > 0, (k, total)
    assert max(m.max_sockets for m in models) == GEN_MAX_SOCKETS
    assert max(m.max_passed for m in models) > GEN_CAPACITY
    assert max(m.max_depth for m in models) == GEN_CAPACITY   # a queue filled to the last slot
    assert all(30 <= len(m.hosts) <= 298 for m in models)


# ---- rr_queue.h under the sanitizers ---------------------------------------------------------

@pytest.fixture(scope="module")
def rr_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rr_queue") / "rr_queue")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "shadow_amd", "csrc"),
                           os.path.join(ROOT, "tests", "rr_queue_main.cpp"), "-o", exe])
    return exe


class Script:
    """The same operations into the model's interface and into the program's script; the answers
    are compared after the one run.  The model has no limits: the script keeps the two counts and
    expects a refusal, which changes nothing, where an offer passes one."""

    def __init__(self, cap, max_sockets):
        self.cap, self.ms = cap, max_sockets
        self.q = RrInterface({k: 0 for k in RR_COUNTERS})
        self.lines, self.want = [f"setup {cap} {max_sockets}"], []
        self.refused = {"full": 0, "sockets": 0}
        self.at_max_sockets = self.at_cap = 0
        self.pid = 0

    def offer(self, handle):
        p = (handle, self.pid, 60 + self.pid % 1441, self.pid % 1449, self.pid % 7)
        self.pid += 1
        self.lines.append("offer %d %d %d %d %d" % p)
        if len(self.q) >= self.cap:
            ans = "full"
        elif len(self.q.rr) >= self.ms and all(s.handle != handle for s in self.q.rr):
            ans = "sockets"
        else:
            ans = "ok"
            self.q.offer(p)
            self.at_max_sockets += len(self.q.rr) == self.ms
            self.at_cap += len(self.q) == self.cap
        if ans != "ok":
            self.refused[ans] += 1
        self.want.append(ans)

    def pop(self):
        p = self.q.select_round_robin()
        self.lines.append("pop")
        self.want.append("empty" if p is None else "%d %d %d %d" % p[1:])

    def state(self):
        self.lines.append("state")
        head = self.q.head_pkt()
        self.want.append(("%d %d %d" % (len(self.q), len(self.q.rr), -1 if head is None else head),
                          " ".join("%d:%d" % x for x in self.q.listing())))

    def run(self, exe):
        out = subprocess.run([exe], input="\n".join(self.lines) + "\n", text=True, capture_output=True)
        assert out.returncode == 0, out.stderr[-2000:]
        answers = out.stdout.splitlines()
        assert len(answers) == len(self.want)
        bumps = []
        for line, ans, want in zip(self.lines[1:], answers, self.want):
            if isinstance(want, tuple):   # state: "<packets> <sockets> <head> <bump> : <handle>:<count> ..."
                left, right = ans.split(":", 1)
                assert left.split()[:3] == want[0].split() and right.strip() == want[1], (line, ans, want)
                bumps.append(int(left.split()[3]))
            else:
                assert ans == want, (line, ans, want)
        return bumps


def test_rr_queue_hand_script_under_sanitizers(rr_exe):
    """Capacity 4, two sockets: the pool filled exactly, one packet too many, one socket too many,
    both refusals leaving the queue as it was; then the rotation of the first hand case."""
    s = Script(4, 2)
    for hd in (A, A, A, C):
        s.offer(hd)
    s.state()
    s.offer(A)            # the fifth packet
    s.pop()               # p0; [C(p3), A(p1 p2)]
    s.offer(B)            # a third socket
    s.state()
    for _ in range(4):
        s.pop()
    s.state()
    s.pop()               # empty
    s.offer(B)            # B is welcome now
    s.pop()
    s.state()
    assert s.want[4] == ("4 2 0", f"{A}:3 {C}:1") and s.want[5] == "full" and s.want[7] == "sockets"
    assert [w.split()[0] for w in s.want[9:13]] == ["3", "1", "2", "empty"]
    assert s.run(rr_exe)[-1] <= 3   # four slots were never needed: the head packet takes none


@pytest.mark.parametrize("seed,cap,ms,handles", [(0, 8, 3, 4), (1, 64, 6, 6), (2, 5, 1, 2), (3, 33, 16, 40)])
def test_rr_queue_against_the_model_under_sanitizers(rr_exe, seed, cap, ms, handles):
    """Random streams in phases -- fill (offers outweigh pops), drain, mixed -- over more handles
    than max_sockets where the case has them: pool exhaustion, exactly max_sockets sockets, one
    socket too many, and far more packets than slots, so every slot is reused after the bump
    count has reached its end."""
    rng = np.random.default_rng(500 + seed)
    s = Script(cap, ms)
    hs = rng.integers(0, 2**64, handles, dtype=np.uint64).tolist()
    for phase in range(12):
        p_offer = (0.8, 0.3, 0.55)[phase % 3]
        for _ in range(6 * cap):
            if rng.random() < p_offer:
                s.offer(hs[int(rng.integers(0, handles))])
            else:
                s.pop()
            if rng.random() < 0.1:
                s.state()
        s.state()
    while len(s.q):
        s.pop()
    s.pop()
    s.state()
    assert s.refused["full"] > 0 and s.at_cap > 0 and s.at_max_sockets > 0 and s.pid > 10 * cap
    assert (s.refused["sockets"] > 0) == (handles > ms)
    bumps = s.run(rr_exe)
    assert max(bumps) == cap - 1 and bumps[-1] == cap - 1   # every slot has been handed out; reuse since
