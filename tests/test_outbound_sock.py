"""CPU tier of the outbound stage's two socket disciplines ("fifo-sockets", "round-robin-sockets"):
the model (tests/outbound_sock_model.py: socket.c's two buffers, priority_queue.c's array heap
and the rrQueue restated under the FIFO model's relay loop) pinned on hand vectors worked out from
network_interface.c:235-316 / :366-392, priority_queue.c:87-140 / :189-208,
network_queuing_disciplines.c:90-102 and token_bucket.rs; two properties that tie it to the plain
models; the random-window generator the device tests use, held to the conditions it is there to
produce; and sock_queue.h -- the queue the kernel compiles -- as a program of its own under the
sanitizers, against the model's interface.  tests/test_outbound_sock_gpu.py runs the hand vectors
and the generator on the device."""
import os
import subprocess

import numpy as np
import pytest

from oracle.token_bucket import SIM_START as S, create_token_bucket
from tests.outbound_model import OutboundModel
from tests.outbound_rr_model import RrOutboundModel
from tests.outbound_sock_model import (IDLE, LOCAL, SENT, SOCK_COUNTERS, FifoSockInterface, RrSockInterface,
                                       SockOutboundModel)
from tests.test_outbound import MS, bucket, payload_of, records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIFO, RR = "fifo-sockets", "round-robin-sockets"
QDISCS = (FIFO, RR)
# canonical handles: compared for equality only, any value
A, B, C, D, E, F, G, Z = 0x7F00_0000_1000, 0, 2**64 - 1, 5, 2**63, 77, 1, 2**32
NAMES = {A: "A", B: "B", C: "C", D: "D", E: "E", F: "F", G: "G", Z: "Z"}
FULL, SMALL, ACK = 1500, 100, 52

# ---- the reference's heap on the issue's three scripts, at the interface ---------------------


def _interface(itf=FifoSockInterface):
    return itf({k: 0 for k in SOCK_COUNTERS})


def _offer(q, handle, prio, pkt):
    q.offer(((prio, handle), pkt, 60, 8, 1))


def _pops(q, n):
    return [q.select()[1] for _ in range(n)]


def test_a_control_packet_does_not_overtake_a_socket_above_its_own():
    """Offer (A, 1, a1), (B, 2, b2), (B, 0, bc): B stands at index 1 and stays there when its key
    becomes 0 (no re-heapify on an offer to a queued socket).  The pop takes the root A: a1; then
    B alone: bc (control first), b2."""
    q = _interface()
    _offer(q, A, 1, 1), _offer(q, B, 2, 2), _offer(q, B, 0, 3)
    assert q.listing() == [(A, 1), (B, 2)] and q.ctr["stale_key"] == 1
    assert _pops(q, 3) == [1, 3, 2] and q.ctr["not_lowest"] == 1


def test_equal_keys_are_smaller_both_ways():
    """(A, 0), (B, 0), (C, 0): each push sifts up past its parent, a tie being "smaller":
    [A] -> [B, A] -> [C, A, B].  Pop: C leaves, B takes the root, its child A is "smaller": [A, B];
    then A, then B."""
    q = _interface()
    _offer(q, A, 0, 1), _offer(q, B, 0, 2), _offer(q, C, 0, 3)
    assert q.listing() == [(C, 1), (A, 1), (B, 1)]
    assert _pops(q, 3) == [3, 1, 2]


def test_seven_sockets_with_stale_keys():
    """Data A1 ... G7 (the heap in offer order: no push moves), control on G, E, B (three stale
    keys, none moves), two pops (a1, bc), then (A, 8) and (A, 0): the heap array is
    [E, G, B, D, F, C, A] and drains ec gc ac b2 c3 d4 e5 f6 g7 a8."""
    q = _interface()
    socks = [A, B, C, D, E, F, G]
    for i, s in enumerate(socks):
        _offer(q, s, i + 1, i + 1)                 # packet i + 1 = the socket's data packet
    assert [h for h, _ in q.listing()] == socks
    for j, s in enumerate((G, E, B)):
        _offer(q, s, 0, 10 + j)                    # 10: gc, 11: ec, 12: bc
    assert [h for h, _ in q.listing()] == socks and q.ctr["stale_key"] == 3
    assert _pops(q, 2) == [1, 12]
    _offer(q, A, 8, 8), _offer(q, A, 0, 20)        # 20: ac
    assert q.listing() == [(E, 2), (G, 2), (B, 1), (D, 1), (F, 1), (C, 1), (A, 2)]
    assert _pops(q, 10) == [11, 10, 20, 2, 3, 4, 5, 6, 7, 8]
    assert q.select() is None and len(q) == 0


# ---- the hand cases, shared with the device tests -------------------------------------------
# SOCK_INPUTS: name -> (bucket, first_host, [(offers [(time, socket, priority, size, dst, pkt)],
# window_end, bootstrap_end)]); SOCK_WANT: (name, qdisc) -> per window (records (SENT first, then
# LOCAL), n_stored, next task, the queued sockets after the window [(name, packets)] -- the heap
# array under fifo-sockets, the rrQueue otherwise --, the packet the next pop takes) and the final
# (task, cached pkt, balance, queue_len).  Times are offsets from S in ms.  The bucket is 1000 B/s
# = (1501, 1, 1 ms): a full packet at S leaves 1 token, and from a refill boundary a packet of n
# bytes that finds the bucket empty waits n ms.
SEVEN = [A, B, C, D, E, F, G]
SOCK_INPUTS = {
    # no bucket: all three leave at 0.  FIFO: the root A first although B's key is 0 by then.
    "stale_key": (None, 0, [
        ([(0, A, 1, SMALL, 1, 0), (0, B, 2, SMALL, 1, 1), (0, B, 0, ACK, 1, 2)], 10, 0)]),
    # z1 is cached until 1499 ms, so the three ACKs offered at 50 ms stay queued over the window's
    # end: the heap is [C, A, B].  From 1499 ms: z1, then cc ac bc, 52 ms apart.
    "ties": (bucket(), 0, [
        ([(0, Z, 1, FULL, 1, 90), (0, Z, 2, FULL, 1, 91)], 10, 0),
        ([(50, A, 0, ACK, 1, 0), (50, B, 0, ACK, 1, 1), (50, C, 0, ACK, 1, 2)], 100, 0),
        ([], 10000, 0)]),
    # The third script under the relay: a1 (full) leaves 1 token, the second pop takes bc, which
    # blocks for 99 ms and is cached -- popped, so the heap has moved on.  At 50 ms (A, 8), (A, 0);
    # the heap array after that window is [E, G, B, D, F, C, A].  Then one packet per 100 ms
    # (the ACKs 52 ms).
    "seven_sockets": (bucket(), 0, [
        ([(0, s, i + 1, FULL if i == 0 else SMALL, 1, i) for i, s in enumerate(SEVEN)] +
         [(0, G, 0, ACK, 1, 10), (0, E, 0, ACK, 1, 11), (0, B, 0, SMALL, 1, 12)], 10, 0),
        ([(50, A, 8, SMALL, 1, 13), (50, A, 0, ACK, 1, 14)], 60, 0),
        ([], 5000, 0)]),
    # A(p0 p1 | ack p4), B(p2 | ack p3).  The windows are cut while a packet is cached whose socket
    # has been pushed again at the pop.
    "cached_packet_whose_socket_was_pushed_again": (bucket(), 0, [
        ([(0, A, 1, FULL, 1, 0), (0, A, 2, SMALL, 1, 1), (0, B, 3, SMALL, 1, 2), (0, B, 0, SMALL, 1, 3),
          (0, A, 0, SMALL, 1, 4)], 50, 0),
        ([], 250, 0),
        ([], 1000, 0)]),
    # p1 is cached until 1499 ms.  B's p2 and its ACK p3 and A's ACK p4 are offered at exactly that
    # time: all three are queued before the task runs.
    "offer_at_the_tasks_time": (bucket(), 0, [
        ([(0, A, 1, FULL, 1, 0), (0, A, 2, FULL, 1, 1)], 10, 0),
        ([(1499, B, 3, 60, 1, 2), (1499, B, 0, 60, 1, 3), (1499, A, 0, 60, 1, 4)], 1600, 0)]),
    # a task exactly at window_end is not run; the next window runs it
    "task_at_window_end_is_carried": (bucket(), 0, [
        ([(0, A, 1, FULL, 1, 0), (0, B, 0, FULL, 1, 1)], 10, 0),
        ([], 1499, 0),
        ([], 1499 + 1e-6, 0)]),
    # the task runs before bootstrap_end: three full packets, the bucket untouched; A's control
    # packet p1 goes before its data packet p0
    "bootstrap": (bucket(), 0, [
        ([(0, A, 1, FULL, 1, 0), (0, A, 0, FULL, 1, 1), (0, B, 2, FULL, 1, 2)], 10, 1)]),
    # host 7: B's control packet p2 is local and leaves without the bucket
    "local_packet_leaves_without_the_bucket": (bucket(), 7, [
        ([(0, A, 1, FULL, 1, 0), (0, A, 2, SMALL, 1, 1), (0, B, 0, FULL, 7, 2)], 10, 0)]),
}

SOCK_WANT = {
    ("stale_key", FIFO): [
        ([(SENT, 0, 0.0), (SENT, 2, 0.0), (SENT, 1, 0.0)], 0, None, [], None),
        (None, None, None, 0),
    ],
    ("stale_key", RR): [
        ([(SENT, 0, 0.0), (SENT, 2, 0.0), (SENT, 1, 0.0)], 0, None, [], None),
        (None, None, None, 0),
    ],
    ("ties", FIFO): [
        ([(SENT, 90, 0.0)], 1, 1499.0, [], None),
        ([], 4, 1499.0, [('C', 1), ('A', 1), ('B', 1)], 2),
        ([(SENT, 91, 1499.0), (SENT, 2, 1551.0), (SENT, 0, 1603.0), (SENT, 1, 1655.0)], 0, None, [], None),
        (None, None, 0, 0),
    ],
    ("ties", RR): [
        ([(SENT, 90, 0.0)], 1, 1499.0, [], None),
        ([], 4, 1499.0, [('A', 1), ('B', 1), ('C', 1)], 0),
        ([(SENT, 91, 1499.0), (SENT, 0, 1551.0), (SENT, 1, 1603.0), (SENT, 2, 1655.0)], 0, None, [], None),
        (None, None, 0, 0),
    ],
    ("seven_sockets", FIFO): [
        ([(SENT, 0, 0.0)], 9, 99.0, [('E', 2), ('G', 2), ('B', 1), ('D', 1), ('F', 1), ('C', 1)], 11),
        ([], 11, 99.0, [('E', 2), ('G', 2), ('B', 1), ('D', 1), ('F', 1), ('C', 1), ('A', 2)], 11),
        ([(SENT, 12, 99.0), (SENT, 11, 151.0), (SENT, 10, 203.0), (SENT, 14, 255.0), (SENT, 1, 355.0), (SENT, 2, 455.0), (SENT, 3, 555.0), (SENT, 4, 655.0), (SENT, 5, 755.0), (SENT, 6, 855.0), (SENT, 13, 955.0)], 0, None, [], None),
        (None, None, 0, 0),
    ],
    ("seven_sockets", RR): [
        ([(SENT, 0, 0.0)], 9, 99.0, [('C', 1), ('D', 1), ('E', 2), ('F', 1), ('G', 2), ('B', 1)], 2),
        ([], 11, 99.0, [('C', 1), ('D', 1), ('E', 2), ('F', 1), ('G', 2), ('B', 1), ('A', 2)], 2),
        ([(SENT, 12, 99.0), (SENT, 2, 199.0), (SENT, 3, 299.0), (SENT, 11, 351.0), (SENT, 5, 451.0), (SENT, 10, 503.0), (SENT, 1, 603.0), (SENT, 14, 655.0), (SENT, 4, 755.0), (SENT, 6, 855.0), (SENT, 13, 955.0)], 0, None, [], None),
        (None, None, 0, 0),
    ],
    ("cached_packet_whose_socket_was_pushed_again", FIFO): [
        ([(SENT, 4, 0.0), (SENT, 3, 0.0)], 3, 199.0, [('A', 1), ('B', 1)], 1),
        ([(SENT, 0, 199.0)], 2, 299.0, [('B', 1)], 2),
        ([(SENT, 1, 299.0), (SENT, 2, 399.0)], 0, None, [], None),
        (None, None, 0, 0),
    ],
    ("cached_packet_whose_socket_was_pushed_again", RR): [
        ([(SENT, 4, 0.0), (SENT, 3, 0.0)], 3, 199.0, [('B', 1), ('A', 1)], 2),
        ([(SENT, 0, 199.0)], 2, 299.0, [('A', 1)], 1),
        ([(SENT, 2, 299.0), (SENT, 1, 399.0)], 0, None, [], None),
        (None, None, 0, 0),
    ],
    ("offer_at_the_tasks_time", FIFO): [
        ([(SENT, 0, 0.0)], 1, 1499.0, [], None),
        ([(SENT, 1, 1499.0), (SENT, 4, 1559.0)], 2, 1619.0, [('B', 1)], 2),
        (1619.0, 3, 0, 1),
    ],
    ("offer_at_the_tasks_time", RR): [
        ([(SENT, 0, 0.0)], 1, 1499.0, [], None),
        ([(SENT, 1, 1499.0), (SENT, 3, 1559.0)], 2, 1619.0, [('B', 1)], 2),
        (1619.0, 4, 0, 1),
    ],
    ("task_at_window_end_is_carried", FIFO): [
        ([(SENT, 1, 0.0)], 1, 1499.0, [], None),
        ([], 1, 1499.0, [], None),
        ([(SENT, 0, 1499.0)], 0, None, [], None),
        (None, None, 0, 0),
    ],
    ("task_at_window_end_is_carried", RR): [
        ([(SENT, 0, 0.0)], 1, 1499.0, [], None),
        ([], 1, 1499.0, [], None),
        ([(SENT, 1, 1499.0)], 0, None, [], None),
        (None, None, 0, 0),
    ],
    ("bootstrap", FIFO): [
        ([(SENT, 1, 0.0), (SENT, 0, 0.0), (SENT, 2, 0.0)], 0, None, [], None),
        (None, None, 1501, 0),
    ],
    ("bootstrap", RR): [
        ([(SENT, 1, 0.0), (SENT, 2, 0.0), (SENT, 0, 0.0)], 0, None, [], None),
        (None, None, 1501, 0),
    ],
    ("local_packet_leaves_without_the_bucket", FIFO): [
        ([(SENT, 0, 0.0), (LOCAL, 2, 0.0)], 1, 99.0, [], None),
        (99.0, 1, 1, 0),
    ],
    ("local_packet_leaves_without_the_bucket", RR): [
        ([(SENT, 0, 0.0), (LOCAL, 2, 0.0)], 1, 99.0, [], None),
        (99.0, 1, 1, 0),
    ],
}


def ms(x):
    return int(round(x * MS))


def sock_arrays(per_host):
    """[[(time, socket, priority, size, dst, pkt)] per host] -> off, time, prio, sock, size, payload,
    dst, pkt lists."""
    off = [0]
    for e in per_host:
        off.append(off[-1] + len(e))
    flat = [x for e in per_host for x in e]
    return (off, [x[0] for x in flat], [x[2] for x in flat], [x[1] for x in flat], [x[3] for x in flat],
            [payload_of(x[5]) for x in flat], [x[4] for x in flat], [x[5] for x in flat])


def case_windows(name):
    """The case's windows with absolute times: [(arrays, window_end, bootstrap_end)]."""
    b, first, steps = SOCK_INPUTS[name]
    return b, first, [(sock_arrays([[(S + ms(t), s, pr, sz, d, p) for t, s, pr, sz, d, p in offers]]), S + ms(w_end),
                       S + ms(boot) if boot else 0) for offers, w_end, boot in steps]


def run_inputs(name, qdisc):
    """The case through the model -> (what SOCK_WANT pins, the model)."""
    b, first, windows = case_windows(name)
    m = SockOutboundModel([b], first, qdisc)
    got = []
    for arr, w_end, boot in windows:
        r = m.advance(*arr, w_end, boot)
        a, z = int(r["src_off"][0]), int(r["src_off"][1])
        assert r["payload"][a:z].tolist() == [payload_of(int(p)) for p in r["sent_pkt"][a:z]]
        nx = r["next_task_time"]
        q = m.hosts[0].q
        got.append(([(k, p, (t - S) / MS) for k, p, t in records(r)], r["n_stored"],
                    None if nx == IDLE else (nx - S) / MS, [(NAMES[h], n) for h, n in q.listing()], q.head_pkt()))
    h = m.hosts[0]
    final = (None if h.task is None else (h.task - S) / MS, None if h.cached is None else h.cached[1],
             h.tb.balance if h.tb is not None else None, len(h.q))
    return got + [final], m


@pytest.mark.parametrize("qdisc", QDISCS)
@pytest.mark.parametrize("name", sorted(SOCK_INPUTS))
def test_hand_case(name, qdisc):
    got, _ = run_inputs(name, qdisc)
    assert got == SOCK_WANT[(name, qdisc)]


def test_the_hand_cases_meet_what_they_are_named_for():
    _, m = run_inputs("seven_sockets", FIFO)
    # (G, E and B below the root A; later A itself, pushed again behind the others)
    assert m.counters["stale_key"] == 4 and m.counters["control_heads3"] > 0 and m.max_sockets == 7
    for qd in QDISCS:
        _, m = run_inputs("cached_packet_whose_socket_was_pushed_again", qd)
        assert m.counters["blocked_rotated"] >= 1 and m.counters["carried"] == 2
        _, m = run_inputs("offer_at_the_tasks_time", qd)
        assert m.counters["ties"] == 4
        _, m = run_inputs("task_at_window_end_is_carried", qd)
        assert m.counters["carried"] == 2
        _, m = run_inputs("bootstrap", qd)
        assert m.counters["boot_forwards"] == 3 and m.counters["blocks"] == 0
        _, m = run_inputs("local_packet_leaves_without_the_bucket", qd)
        assert m.counters["local_forwards"] == 1 and m.hosts[0].tb.balance == 1


# ---- the random windows of the device tests -------------------------------------------------

HEADER = 52
SLOW, FAST = [1000, 20_000, 125_000], [1_250_000, 125_000_000]
GEN_SEEDS = tuple(range(3))
GEN_HOSTS, GEN_CAPACITY, GEN_MAX_SOCKETS, GEN_WINDOWS, GEN_MAX_OFFERS, GEN_CONTROL = 130, 16, 8, 4, 40, 0.3


def random_setup(seed, n_hosts=GEN_HOSTS, max_sockets=GEN_MAX_SOCKETS):
    """Buckets (every other host a slow one, so that queues carry over; a tenth of the others
    none), each host's sockets (1 to max_sockets handles) and the windows' ends of one seed."""
    rng = np.random.default_rng(4100 + seed)
    buckets = [(*create_token_bucket(int(rng.choice(SLOW))), S) if h % 2 == 0 else
               None if rng.random() < 0.1 else (*create_token_bucket(int(rng.choice(FAST))), S) for h in range(n_hosts)]
    socks = [rng.integers(0, 2**64, int(rng.integers(1, max_sockets + 1)), dtype=np.uint64).tolist()
             for _ in range(n_hosts)]
    ends = (np.cumsum([int(rng.choice([1, 20, 150, 400])) * MS for _ in range(GEN_WINDOWS)]) + S).tolist()
    return rng, buckets, socks, ends


def random_window(rng, hosts, socks, prio, start, end, pid, capacity=GEN_CAPACITY, max_offers=GEN_MAX_OFFERS,
                  control=GEN_CONTROL, n_dst=None, first_host=0):
    """Offers for every host in [start, end): bursts at one instant (one event's sends
    accumulate) on the host's sockets, `control` of them control packets (priority 0, a bare
    header), the others with the host's next priority (prio[h], counted up from 1); 10 % local;
    half of the pending hosts with an offer at the outstanding task's time.  A host is never
    offered more than its queue can still take, so `capacity` holds whatever the bucket does."""
    per_host = []
    n_dst = n_dst or len(hosts)
    for h, host in enumerate(hosts):
        n = min(int(rng.integers(0, max_offers + 1)), capacity - len(host.q))
        times = np.sort(rng.integers(start, end, n)).tolist()
        for i in range(1, n):
            if rng.random() < 0.7:
                times[i] = times[i - 1]
        times.sort()
        if n and host.task is not None and start <= host.task < end and rng.random() < 0.5:
            times[int(rng.integers(0, n))] = host.task
            times.sort()
        offers, hd = [], None
        for i, t in enumerate(times):
            if hd is None or rng.random() < 0.6:
                hd = socks[h][int(rng.integers(0, len(socks[h])))]
            dst = host.id if rng.random() < 0.1 else first_host + int(rng.integers(0, n_dst))
            if rng.random() < control:
                pr, pay = 0, 0
            else:
                pr, pay = prio[h], int(rng.integers(1, 1449))
                prio[h] += 1
            offers.append((t, pr, hd, pay + HEADER, pay, dst, pid + i))
        per_host.append(offers)
        pid += n
    return per_host, pid


def np_arrays(per_host):
    """[[(time, prio, sock, size, payload, dst, pkt)] per host] -> off, time, prio, sock, size,
    payload, dst, pkt."""
    off = np.zeros(len(per_host) + 1, np.uint32)
    off[1:] = np.cumsum([len(e) for e in per_host])
    flat = [x for e in per_host for x in e]
    col = lambda i, dt: np.array([x[i] for x in flat], dt)  # noqa: E731
    return (off, col(0, np.uint64), col(1, np.uint64), col(2, np.uint64), col(3, np.uint32), col(4, np.uint32),
            col(5, np.uint32), col(6, np.uint32))


def run_seed(seed, qdisc, each_window=None, control=GEN_CONTROL, others=(), n_hosts=GEN_HOSTS, first_host=0):
    """The windows of one seed through the model; each_window(arr, end, boot, want, model).
    `others`: further models that are given the same windows, as (model, columns -> its
    arguments); their results go to each_window as a list behind the model."""
    rng, buckets, socks, ends = random_setup(seed, n_hosts)
    model = SockOutboundModel(buckets, first_host, qdisc)
    prio = [1] * n_hosts
    boot = int(ends[0] + (ends[1] - ends[0]) // 2)
    start, pid = S, 0
    for end in ends:
        per_host, pid = random_window(rng, model.hosts, socks, prio, start, end, pid, control=control,
                                      first_host=first_host)
        arr = np_arrays(per_host)
        want = model.advance(*arr, end, boot)
        more = [m.advance(*pick(arr), end, boot) for m, pick in others]
        if each_window:
            each_window(arr, end, boot, want, model, *([more] if others else []))
        start = end
    return model


RESULT_KEYS = ("src_off", "send_time", "dst_host", "payload", "sent_pkt", "loc_off", "loc_pkt", "loc_time")


def same_result(a, b):
    return all(np.array_equal(a[k], b[k]) for k in RESULT_KEYS) and \
        (a["n_stored"], a["next_task_time"]) == (b["n_stored"], b["next_task_time"])


@pytest.mark.parametrize("seed", GEN_SEEDS)
def test_without_control_packets_fifo_sockets_is_the_plain_fifo(seed):
    """No priority 0 and ascending priorities per socket: the heap's keys are never stale and
    never tie, so the root is the lowest priority queued -- the plain FIFO model's records."""
    rng, buckets, _, _ = random_setup(seed)
    plain = OutboundModel(buckets)
    seen = []

    def check(arr, end, boot, want, model, more):
        assert same_result(want, more[0])
        seen.append(len(arr[1]))

    m = run_seed(seed, FIFO, check, control=0.0, others=[(plain, lambda a: (a[0], a[1], a[2], *a[4:]))])
    assert sum(seen) > 1000 and m.counters["not_lowest"] == 0 and m.counters["blocks"] > 0


@pytest.mark.parametrize("seed", GEN_SEEDS)
def test_without_control_packets_round_robin_sockets_is_the_plain_round_robin(seed):
    rng, buckets, _, _ = random_setup(seed)
    plain = RrOutboundModel(buckets)
    seen = []

    def check(arr, end, boot, want, model, more):
        assert same_result(want, more[0])
        seen.append(len(arr[1]))

    m = run_seed(seed, RR, check, control=0.0, others=[(plain, lambda a: (a[0], a[1], a[3], *a[4:]))])
    assert sum(seen) > 1000 and plain.counters["not_in_offer_order"] > 0 and m.counters["blocks"] > 0


class _LowestFirst:
    """What one priority queue per host would do with the same sockets: the socket whose head
    priority is lowest goes first, equal priorities in offer order (packet ids count up with the
    offers)."""

    def __init__(self):
        self.socks = []

    def push(self, sock):
        self.socks.append(sock)

    def pop(self):
        if not self.socks:
            return None
        s = min(self.socks, key=lambda x: (x.peek_next_packet_priority(), (x.control or x.out)[0][1]))
        self.socks.remove(s)
        return s

    def order(self):
        return list(self.socks)


class LowestFirstInterface(FifoSockInterface):
    queue_type = _LowestFirst


def test_the_generator_reaches_what_the_device_tests_need():
    """Over the seeds, under fifo-sockets: control offered to a socket below the heap's root,
    three sockets with control heads at once, heaps of seven and more sockets (and one filled to
    max_sockets), a socket pushed again while its packet is cached, pool slots reused, windows
    that end with packets queued, a queue filled to the last slot, every branch of the relay loop
    -- and on at least half the hosts a send order that "lowest head priority first" does not
    give: a stage that kept one priority queue per host would differ from the model there."""
    total = {}
    for seed in GEN_SEEDS:
        stored, order, other = [], {}, {}

        def each(arr, end, boot, want, model, more):
            stored.append(want["n_stored"])
            for seen, r in ((order, want), (other, more[0])):
                for h in range(len(model.hosts)):
                    seen.setdefault(h, []).extend(p for _, p, _ in records(r, h))

        _, buckets, _, _ = random_setup(seed)
        m = run_seed(seed, FIFO, each, others=[(SockOutboundModel(buckets, 0, LowestFirstInterface), lambda a: a)])
        assert sum(n > 0 for n in stored) >= 2, stored   # (a window inside the bootstrap may drain)
        for k in ("stale_key", "control_heads3", "blocked_rotated", "slots_reused", "not_lowest"):
            assert m.counters[k] > 0, (k, m.counters)
        assert m.max_sockets >= 7
        differ = sum(order[h] != other[h] for h in order)
        assert 2 * differ >= len(m.hosts), (differ, len(m.hosts))
        for k, v in m.counters.items():
            total[k] = total.get(k, 0) + v
        total["max_sockets"] = max(total.get("max_sockets", 0), m.max_sockets)
        total["max_depth"] = max(total.get("max_depth", 0), m.max_depth)
        total["max_passed"] = max(total.get("max_passed", 0), m.max_passed)
    assert set(SOCK_COUNTERS) <= set(total)
    for k, v in total.items():
        assert v > 0, (k, total)
    assert total["max_sockets"] == GEN_MAX_SOCKETS and total["max_depth"] == GEN_CAPACITY
    assert total["max_passed"] > GEN_CAPACITY
    # round-robin: the control list overtakes the data list inside a socket
    m = run_seed(0, RR)
    assert m.counters["blocked_rotated"] > 0 and m.counters["not_lowest"] > 0 and m.counters["slots_reused"] > 0


# ---- sock_queue.h under the sanitizers -------------------------------------------------------

@pytest.fixture(scope="module")
def sq_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sock_queue") / "sock_queue")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "shadow_amd", "csrc"),
                           os.path.join(ROOT, "tests", "sock_queue_main.cpp"), "-o", exe])
    return exe


class Script:
    """The same operations into the model's interface and into the program's script; the answers
    are compared after the one run.  The model has no limits: the script keeps the two counts and
    expects a refusal where an offer passes one.  A refusal changes nothing: the state is asked
    for after each and compared like any other."""

    def __init__(self, cap, max_sockets, qdisc):
        self.cap, self.ms = cap, max_sockets
        self.q = _interface(FifoSockInterface if qdisc == FIFO else RrSockInterface)
        self.lines, self.want = [f"setup {cap} {max_sockets} {int(qdisc == FIFO)}"], []
        self.refused = {"full": 0, "sockets": 0}
        self.at_max_sockets = self.at_cap = 0
        self.pid = 0
        self.prio = 1

    def offer(self, handle, control):
        pr = 0 if control else self.prio
        self.prio += not control
        p = ((pr, handle), self.pid, 60 + self.pid % 1441, self.pid % 1449, self.pid % 7)
        self.pid += 1
        self.lines.append("offer %d %d %d %d %d %d" % (handle, pr, *p[1:]))
        n_socks = len(self.q.listing())
        if len(self.q) >= self.cap:
            ans = "full"
        elif n_socks >= self.ms and all(h != handle for h, _ in self.q.listing()):
            ans = "sockets"
        else:
            ans = "ok"
            self.q.offer(p)
            self.at_max_sockets += len(self.q.listing()) == self.ms
            self.at_cap += len(self.q) == self.cap
        self.want.append(ans)
        if ans != "ok":
            self.refused[ans] += 1
            self.state()

    def pop(self):
        p = self.q.select()
        self.lines.append("pop")
        self.want.append("empty" if p is None else "%d %d %d %d" % p[1:])

    def state(self):
        self.lines.append("state")
        head = self.q.head_pkt()
        self.want.append(("%d %d %d" % (len(self.q), len(self.q.listing()), -1 if head is None else head),
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


def test_sock_queue_hand_scripts_under_sanitizers(sq_exe):
    """The three heap scripts, with the state after every step; then capacity 4, two sockets: the
    pool filled exactly, one packet too many, one socket too many, both refusals leaving the queue
    as it was."""
    s = Script(16, 8, FIFO)
    for hd, ctl in ((A, 0), (B, 0), (B, 1)):
        s.offer(hd, ctl), s.state()
    for _ in range(4):
        s.pop(), s.state()
    for hd in (A, B, C):
        s.offer(hd, 1), s.state()
    assert s.want[-1][1] == f"{C}:1 {A}:1 {B}:1"
    for _ in range(3):
        s.pop(), s.state()
    for hd in SEVEN:
        s.offer(hd, 0)
    for hd in (G, E, B):
        s.offer(hd, 1), s.state()
    s.pop(), s.pop(), s.offer(A, 0), s.offer(A, 1), s.state()
    assert s.want[-1][1] == " ".join(f"{h}:{n}" for h, n in ((E, 2), (G, 2), (B, 1), (D, 1), (F, 1), (C, 1), (A, 2)))
    for _ in range(11):
        s.pop(), s.state()
    assert s.want[-2] == "empty"
    s.run(sq_exe)
    for qd in QDISCS:
        s = Script(4, 2, qd)
        for hd, ctl in ((A, 0), (A, 1), (A, 0), (C, 0)):
            s.offer(hd, ctl)
        s.state()
        s.offer(A, 1)         # the fifth packet
        s.pop()
        s.offer(B, 1)         # a third socket
        for _ in range(3):
            s.pop()
        s.state()
        s.pop()               # empty
        s.offer(B, 1)         # B is welcome now
        s.offer(C, 0)
        s.offer(A, 0)         # and A is the third socket
        s.pop(), s.pop(), s.pop()
        s.state()
        assert s.refused == {"full": 1, "sockets": 2}
        s.run(sq_exe)
    s = Script(1, 1, FIFO)    # a queue of one packet never leaves the words
    s.offer(A, 0), s.offer(A, 0), s.offer(B, 1), s.pop(), s.offer(B, 1), s.state(), s.pop(), s.pop()
    assert s.refused == {"full": 2, "sockets": 0} and s.run(sq_exe) == [0, 0, 0]


@pytest.mark.parametrize("qdisc", QDISCS)
@pytest.mark.parametrize("seed,cap,ms_,handles", [(0, 8, 3, 4), (1, 16, 8, 8), (2, 5, 2, 3), (3, 4, 8, 12),
                                                  (4, 13, 7, 40)])
def test_sock_queue_against_the_model_under_sanitizers(sq_exe, qdisc, seed, cap, ms_, handles):
    """Random streams in phases -- fill (offers outweigh pops), drain, mixed -- with 30 % control
    packets, over more handles than max_sockets where the case has them: pool exhaustion, exactly
    max_sockets sockets, one socket too many, and far more packets than slots."""
    rng = np.random.default_rng(900 + seed)
    s = Script(cap, ms_, qdisc)
    hs = rng.integers(0, 2**64, handles, dtype=np.uint64).tolist()
    for phase in range(12):
        p_offer = (0.8, 0.3, 0.55)[phase % 3]
        for _ in range(6 * cap):
            if rng.random() < p_offer:
                s.offer(hs[int(rng.integers(0, handles))], rng.random() < 0.3)
            else:
                s.pop()
            if rng.random() < 0.1:
                s.state()
        s.state()
    while len(s.q):
        s.pop()
    s.pop()
    s.state()
    assert s.refused["full"] > 0 and s.at_cap > 0 and s.pid > 10 * cap
    assert (s.at_max_sockets > 0) == (ms_ <= cap)
    assert (s.refused["sockets"] > 0) == (handles > ms_ and ms_ <= cap)
    assert s.q.ctr["slots_reused"] > 0
    bumps = s.run(sq_exe)
    assert max(bumps) == cap and bumps[-1] == 0   # every slot has been handed out; an empty queue starts over
