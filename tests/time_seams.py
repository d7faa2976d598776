"""Inputs at the u64 seams of the stages' time arithmetic, shared by the CPU module
(test_time_seams.py) and the GPU module (test_time_seams_gpu.py): the seam values, the token
bucket fuzz with each relay replayed on the Python oracle, the hand cases of both state machines
and the CoDel op batches near both ends of the time range.

Nothing here is derived from the device; the fuzz's expectations come from oracle/token_bucket.py
and oracle/codel.py, the hand cases' from the reference's lines (their comments say which).
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from oracle import codel as OC
from oracle import token_bucket as O

U64 = O.U64_MAX
SMAX, EMAX, START0 = O.SIMTIME_MAX, O.EMUTIME_MAX, O.SIM_START
FORWARDED, BLOCKED, SKIPPED = O.FORWARDED, O.BLOCKED, O.SKIPPED
POP = 0xFFFFFFFF
TARGET, INTERVAL = OC.TARGET, OC.INTERVAL

SEAM = [1, 2, 3, 1500, 2**32 - 1, 2**32, 2**32 + 1, 2**40, 2**62, 2**63 - 1, 2**63, 2**63 + 1,
        SMAX - 1, SMAX, SMAX + 1, EMAX - 1, EMAX, U64]
LAST_REFILL = [0, 1, START0 - 1, START0, START0 + 1, 2**62, 2**63, EMAX - 1, EMAX]
SIZES = [0, 1, 1500, 2**31, 2**32 - 1]
# the panic kinds as the oracle's ReferencePanic names them -> the names used in reports
KINDS = {"span": "first span", "product": "product", "sum": "sum", "span2": "second span"}


# ------------------------------------------------------------------ token bucket: one relay on the oracle
def replay_relay(cap, inc, itv, last, times, sizes):
    """One relay's attempts on a fresh bucket -> SimpleNamespace(status, value, kind, state).
    kind: None, or the oracle's name of the panic (the attempts from it on have no result);
    state: (balance, last_refill, pending_until) after the last attempt (clean relays only)."""
    tb = [O.TokenBucket(cap, inc, itv, last)]
    pending = [0]
    off = [0, len(times)]
    try:
        st, val = O.relay_run(tb, pending, off, times, sizes, [0] * len(times))
    except O.ReferencePanic as e:
        return SimpleNamespace(status=None, value=None, kind=e.kind, state=None)
    return SimpleNamespace(status=st, value=val, kind=None, state=(tb[0].balance, tb[0].last_refill, pending[0]))


@functools.lru_cache(maxsize=None)
def bucket_fuzz(seed: int = 20261021, n_relays: int = 4000):
    """The seam fuzz of the bucket: ``n_relays`` relays, 1-4 attempts each.

    Capacity and increment are any seam value; the interval is a seam value that is a
    SimulationTime (at most SIMTIME_MAX: a larger one is refused at setup, tested apart);
    last_refill is one of LAST_REFILL.  An attempt's time is the previous one (at first:
    last_refill) plus a seam span, or plus a seam multiple of the interval -1 / +0 / +1, cut off at
    EMUTIME_MAX (2^64 - 1 is EMUTIME_INVALID, no time the reference's clock can give); one relay in
    twenty starts 1 ns before its last_refill instead.  Sizes are SIZES.
    Returns SimpleNamespace(cap, inc, itv, last: u64[n]; off: u32[n + 1]; time: u64[m];
    size: u32[m]; res: per relay, replay_relay's result; clean, panicking: relay index lists)."""
    rng = np.random.default_rng(seed)
    itvs = [v for v in SEAM if v <= SMAX]
    cap, inc, itv, last, off, time, size, res = [], [], [], [], [0], [], [], []
    for _ in range(n_relays):
        c, i, v = (int(rng.choice(len(SEAM))), int(rng.choice(len(SEAM))), int(rng.choice(len(itvs))))
        c, i, v = SEAM[c], SEAM[i], itvs[v]
        l = LAST_REFILL[int(rng.integers(len(LAST_REFILL)))]
        t = l
        ts, ss = [], []
        for a in range(int(rng.integers(1, 5))):
            if a == 0 and l > 0 and rng.random() < 0.05:
                t = l - 1
            elif rng.random() < 0.5:
                t = t + SEAM[int(rng.integers(len(SEAM)))]
            else:
                t = t + v * SEAM[int(rng.integers(len(SEAM)))] + int(rng.integers(-1, 2))
            t = min(max(t, 0), EMAX)
            ts.append(t)
            ss.append(SIZES[int(rng.integers(len(SIZES)))])
        cap.append(c); inc.append(i); itv.append(v); last.append(l)
        time += ts; size += ss; off.append(len(time))
        res.append(replay_relay(c, i, v, l, ts, ss))
    u = lambda a: np.array(a, np.uint64)   # noqa: E731
    return SimpleNamespace(cap=u(cap), inc=u(inc), itv=u(itv), last=u(last), off=np.array(off, np.uint32),
                           time=u(time), size=np.array(size, np.uint32), res=res,
                           clean=[r for r in range(n_relays) if res[r].kind is None],
                           panicking=[r for r in range(n_relays) if res[r].kind is not None])


def bucket_subset(F, relays):
    """The fuzz restricted to ``relays`` (in that order) -> (cap, inc, itv, last, off, time, size)."""
    off = [0]
    tm, sz = [], []
    for r in relays:
        a, b = int(F.off[r]), int(F.off[r + 1])
        tm.append(F.time[a:b]); sz.append(F.size[a:b])
        off.append(off[-1] + b - a)
    idx = np.array(relays, np.int64)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)   # noqa: E731
    return (F.cap[idx], F.inc[idx], F.itv[idx], F.last[idx], np.array(off, np.uint32),
            cat(tm, np.uint64), cat(sz, np.uint32))


# ------------------------------------------------------------------ token bucket: hand cases
# Each case: the bucket (capacity, increment, interval, last_refill), its attempts (time, size) and
# what the reference gives for each: (FORWARDED, balance) / (BLOCKED, duration) / (SKIPPED, deadline),
# or "panic" as the last entry with the kind; then the state (balance, last_refill, pending_until).
# Buckets start full (token_bucket.rs:52), so a case first removes what it must at `last` (span 0:
# no refill, :130).  L is an ordinary last_refill.
L = START0 + 1
_HALF = SMAX // 2 + 1   # 2 * _HALF = SMAX + 2: a product in (SIMTIME_MAX, 2^64)

BUCKET_CASES = [
    # increment.saturating_mul(n) (:136-138), n = 2^30 refills of 2^40: 2^70 saturates to 2^64 - 1,
    # the balance 0 + that clamps to the capacity (:141-144).  A wrapping product is 0: balance 0.
    dict(name="token_product_pow2", bucket=(2**32 - 1, 2**40, 1, L),
         attempts=[(L, 2**32 - 1), (L + 2**30, 0)],
         expect=[(FORWARDED, 0), (FORWARDED, 2**32 - 1)], state=(2**32 - 1, L + 2**30, 0)),
    # the same with 2^40 + 1: a wrapping product is 2^30, a balance of 2^30 instead of 2^32 - 1
    dict(name="token_product_pow2_plus1", bucket=(2**32 - 1, 2**40 + 1, 1, L),
         attempts=[(L, 2**32 - 1), (L + 2**30, 0)],
         expect=[(FORWARDED, 0), (FORWARDED, 2**32 - 1)], state=(2**32 - 1, L + 2**30, 0)),
    # balance.saturating_add(num_tokens) (:141-143): (2^64 - 11) + 2^63 saturates to 2^64 - 1 = the
    # capacity.  A wrapping sum is 2^63 - 12.
    dict(name="token_sum", bucket=(U64, 2**63, 1000, L),
         attempts=[(L, 10), (L + 1000, 0)],
         expect=[(FORWARDED, U64 - 10), (FORWARDED, U64)], state=(U64, L + 1000, 0)),
    # compute_conforming_duration (:99-118): empty bucket, 2^32 - 1 tokens missing, increment 1:
    # 2^32 - 1 refills; interval.saturating_mul(2^32 - 2) = 2^33 * (2^32 - 2) overflows u64 ->
    # SIMTIME_MAX (simulation_time.rs:146); next_refill_span = 2^33 (span 0), and
    # SIMTIME_MAX.saturating_add(2^33) = 17500059282299486206 < 2^64 is no SimulationTime: the
    # unwrap (simulation_time.rs:137) panics.
    dict(name="conforming_product_overflows", bucket=(2**32, 1, 2**33, L),
         attempts=[(L, 2**32 - 1), (L, 1), (L, 2**32 - 1)],
         expect=[(FORWARDED, 1), (FORWARDED, 0), "panic"], kind="sum"),
    # two refills needed, interval 2^63: next_refill_span = 2^63 (span 0), interval * 1 = 2^63 (a
    # SimulationTime: 2^63 < SIMTIME_MAX), the sum 2^64 overflows u64 -> SIMTIME_MAX, no panic
    # (simulation_time.rs:136).  forward_later: L + SIMTIME_MAX = EMUTIME_MAX + 2 -> EMUTIME_MAX
    # (emulated_time.rs:103-108): Pending until then.
    dict(name="conforming_sum_overflows", bucket=(3000, 1500, 2**63, L),
         attempts=[(L, 1500), (L, 1500), (L, 3000), (EMAX - 1, 1)],
         expect=[(FORWARDED, 1500), (FORWARDED, 0), (BLOCKED, SMAX), (SKIPPED, EMAX)], state=(0, L, EMAX)),
    # three refills needed: interval.saturating_mul(2) = SIMTIME_MAX + 2 does not overflow u64:
    # from_c_simtime(..).unwrap() panics (simulation_time.rs:146-147)
    dict(name="conforming_product_unrepresentable", bucket=(4500, 1500, _HALF, L),
         attempts=[(L, 1500), (L, 1500), (L, 1500), (L, 4500)],
         expect=[(FORWARDED, 3000), (FORWARDED, 1500), (FORWARDED, 0), "panic"], kind="product"),
    # now.duration_since(last_refill) (:128) = SIMTIME_MAX exactly is a SimulationTime: n =
    # SIMTIME_MAX / 1e9 = 17500059273 refills, the balance stays at the capacity, last_refill
    # advances by n * 1e9, and the removal of 1 leaves 99
    dict(name="span_at_simtime_max", bucket=(100, 10, 10**9, START0),
         attempts=[(EMAX, 1)], expect=[(FORWARDED, 99)],
         state=(99, START0 + (SMAX // 10**9) * 10**9, 0)),
    # one ns more: checked_duration_since is None (emulated_time.rs:84-87), the unwrap (:80) panics;
    # SIMTIME_MAX + 1 = 17500059273709551615 = 5 * 3500011854741910323: the interval divides it
    dict(name="span_above_interval_divides", bucket=(100, 10, 5, START0 - 1),
         attempts=[(EMAX, 1)], expect=["panic"], kind="span"),
    dict(name="span_above_interval_does_not_divide", bucket=(100, 10, 10**9, START0 - 1),
         attempts=[(EMAX, 1)], expect=["panic"], kind="span"),
    # the same at the other end of the range, the interval SIMTIME_MAX itself (one whole refill)
    dict(name="span_above_interval_simtime_max", bucket=(100, 10, SMAX, 0),
         attempts=[(SMAX + 1, 1)], expect=["panic"], kind="span"),
    # and the span exactly SIMTIME_MAX from 0: one refill, last_refill = SIMTIME_MAX
    dict(name="span_at_simtime_max_from_zero", bucket=(100, 10, SMAX, 0),
         attempts=[(SMAX, 1)], expect=[(FORWARDED, 99)], state=(99, SMAX, 0)),
    # now before last_refill: checked_sub is None (emulated_time.rs:85)
    dict(name="now_before_last_refill", bucket=(100, 10, 1000, L),
         attempts=[(L - 1, 1)], expect=["panic"], kind="span"),
]


def bucket_case_ops(case):
    """-> (times, sizes) of a hand case's attempts."""
    return [t for t, _ in case["attempts"]], [s for _, s in case["attempts"]]


# ------------------------------------------------------------------ CoDel: hand cases
# A case is one host's ops in order -- ("push", time, pkt, size) / ("pop", time) -- and after each
# pop what the reference's queue gives: (returned pkt or None, dropped pkts, dict of state fields),
# or "panic".  All packets are 1500 bytes, so "total_bytes_stored <= MTU" (codel_queue.rs:238) is
# "at most one packet left".  MS50 = 50 ms.
MS50 = 50_000_000


def _pushes(t, n, first=0):
    return [("push", t, first + k, 1500) for k in range(n)]


CODEL_CASES = [
    # process_standing_delay (:233-263) at now = EMUTIME_MAX - 50 ms with a standing delay of
    # exactly TARGET and 3 packets left: interval_end = now.saturating_add(INTERVAL) (:259);
    # checked_add (emulated_time.rs:95-97) overflows past EMUTIME_MAX -> EmulatedTime::MAX (:106).
    # One ns before EMUTIME_MAX `now >= end` (:252) is false: the packet is returned, nothing drops.
    dict(name="interval_end_saturates",
         ops=_pushes(EMAX - MS50 - TARGET, 4) + [("pop", EMAX - MS50), ("pop", EMAX - 1)],
         expect=[(0, [], dict(len=3, mode=0, interval_end=EMAX, drop_next=None)),
                 (1, [], dict(len=2, mode=0, interval_end=EMAX, drop_next=None))]),
    # at now = EMUTIME_MAX the comparison holds (EMUTIME_MAX >= EMUTIME_MAX; a sum saturated at
    # 2^64 - 1 would not): ok_to_drop, store mode -> drop_from_store_mode (:151-171), whose
    # apply_control_law(now, 1) (:287-300) takes to_abs_simtime = SIMTIME_MAX and adds 1e8 as
    # SimulationTime::saturating_add: the u64 sum does not overflow, from_c_simtime is None, the
    # unwrap (simulation_time.rs:137) panics.
    dict(name="pop_at_emutime_max_against_saturated_interval_end",
         ops=_pushes(EMAX - MS50 - TARGET, 4) + [("pop", EMAX - MS50), ("pop", EMAX)],
         expect=[(0, [], dict(len=3, mode=0, interval_end=EMAX, drop_next=None)), "panic"]),
    # drop mode entered at exactly EMUTIME_MAX - 100 ms with count 1: the increment is
    # round(1e8 / 1) = 1e8, adjusted = SIMTIME_MAX exactly, drop_next = EMUTIME_MAX, no panic.
    # Pops: TARGET after the pushes sets interval_end = now + INTERVAL (an ordinary sum); at that
    # time packet 1 is dropped, packet 2 returned (3 left: still above MTU, interval_end stays).
    dict(name="drop_next_exactly_emutime_max",
         ops=_pushes(EMAX - 2 * INTERVAL - TARGET, 6) + [("pop", EMAX - 2 * INTERVAL), ("pop", EMAX - INTERVAL)],
         expect=[(0, [], dict(len=5, mode=0, interval_end=EMAX - INTERVAL, drop_next=None)),
                 (2, [1], dict(len=3, mode=1, interval_end=EMAX - INTERVAL, drop_next=EMAX,
                               current_drop_count=1, previous_drop_count=1))]),
    # one ns later the same entry is past EMUTIME_MAX: the panic of the case above, not a
    # saturation -- neither at 2^64 - 2 nor at 2^64 - 1
    dict(name="drop_next_one_past_emutime_max",
         ops=_pushes(EMAX - 2 * INTERVAL - TARGET + 1, 6) + [("pop", EMAX - 2 * INTERVAL + 1),
                                                             ("pop", EMAX - INTERVAL + 1)],
         expect=[(0, [], dict(len=5, mode=0, interval_end=EMAX - INTERVAL + 1, drop_next=None)), "panic"]),
    # in drop mode, drop_next = EMUTIME_MAX from the case before; a pop at EMUTIME_MAX: ok_to_drop
    # (now >= interval_end), drop mode -> drop_from_drop_mode (:173-202): should_drop (EMUTIME_MAX
    # >= EMUTIME_MAX) drops packet 3, count 2; packet 4 comes with 1 packet left: not ok_to_drop
    # (:238), so no control law runs: store mode, packet 4 returned, drop_next stays.
    dict(name="should_drop_at_emutime_max",
         ops=_pushes(EMAX - 2 * INTERVAL - TARGET, 6) + [("pop", EMAX - 2 * INTERVAL), ("pop", EMAX - INTERVAL),
                                                         ("pop", EMAX)],
         expect=[(0, [], dict(len=5, mode=0)),
                 (2, [1], dict(len=3, mode=1, drop_next=EMAX)),
                 (4, [3], dict(len=1, mode=0, interval_end=None, drop_next=EMAX, current_drop_count=2))]),
    # the same with one packet more: packet 4 comes with 2 left and is ok_to_drop, so the control
    # law runs on drop_next = EMUTIME_MAX (:192-195): past the end, a panic
    dict(name="control_law_on_drop_next_at_emutime_max",
         ops=_pushes(EMAX - 2 * INTERVAL - TARGET, 7) + [("pop", EMAX - 2 * INTERVAL), ("pop", EMAX - INTERVAL),
                                                         ("pop", EMAX)],
         expect=[(0, [], dict(len=6, mode=0)), (2, [1], dict(len=4, mode=1, drop_next=EMAX)), "panic"]),
    # a packet stamped SIMULATION_START - 2 and popped at EMUTIME_MAX: the difference is
    # SIMTIME_MAX + 2, checked_duration_since is None, saturating_duration_since is ZERO
    # (emulated_time.rs:84-93): standing delay 0 < TARGET, no interval, no drop, however often
    dict(name="stamp_more_than_simtime_max_ago",
         ops=_pushes(START0 - 2, 5) + [("pop", EMAX), ("pop", EMAX), ("pop", EMAX)],
         expect=[(0, [], dict(len=4, mode=0, interval_end=None, drop_next=None)),
                 (1, [], dict(len=3, mode=0, interval_end=None, drop_next=None)),
                 (2, [], dict(len=2, mode=0, interval_end=None, drop_next=None))]),
    # the same stamp popped SIMTIME_MAX later exactly (at EMUTIME_MAX - 2): the delay is
    # SIMTIME_MAX >= TARGET and interval_end saturates
    dict(name="stamp_exactly_simtime_max_ago",
         ops=_pushes(START0 - 2, 5) + [("pop", EMAX - 2)],
         expect=[(0, [], dict(len=4, mode=0, interval_end=EMAX, drop_next=None))]),
    # drop mode entered before SIMULATION_START: to_abs_simtime (emulated_time.rs:73-75) is
    # duration_since(SIMULATION_START), a panic
    dict(name="control_law_before_simulation_start",
         ops=_pushes(1000, 6) + [("pop", 1000 + TARGET), ("pop", 1000 + TARGET + INTERVAL)],
         expect=[(0, [], dict(len=5, mode=0, interval_end=1000 + TARGET + INTERVAL)), "panic"]),
]


def codel_case_batches(case):
    """A hand case as op batches that each end with a pop (so the state can be read after it):
    list of (time, size, pkt) lists."""
    out, cur = [], []
    for op in case["ops"]:
        if op[0] == "push":
            cur.append((op[1], op[3], op[2]))
        else:
            cur.append((op[1], POP, 0))
            out.append(cur)
            cur = []
    assert not cur
    return out


# ------------------------------------------------------------------ CoDel: op batches near the ends
def codel_ops(rng, n_hosts, per_host, base_choices, steps, pid0=0, first_push_before=None):
    """Per host a run of pushes and pops with non-decreasing times: starts at one of
    ``base_choices``, advances by one of ``steps`` per op, cut off at EMUTIME_MAX.  With
    ``first_push_before`` = (stamp_max, jump_to) the host's first ops are pushes stamped at or
    below stamp_max and the rest run from jump_to.  -> (off, time, size, pkt, next pid)."""
    off, times, sizes, pkts = [0], [], [], []
    pid = pid0
    for _ in range(n_hosts):
        n = int(rng.integers(0, per_host + 1))
        t = int(base_choices[int(rng.integers(len(base_choices)))])
        if first_push_before is not None:
            stamp_max, jump_to = first_push_before
            stamps = np.sort(rng.integers(max(stamp_max - 10**9, 0), stamp_max + 1, int(rng.integers(2, 8))))
            stamps[-1] = stamp_max
            for s in stamps:
                times.append(int(s)); sizes.append(1500); pkts.append(pid); pid += 1
            t = jump_to
        for _ in range(n):
            t = min(t + int(steps[int(rng.integers(len(steps)))]), EMAX)
            if rng.random() < float(rng.choice([0.35, 0.5, 0.65])):
                times.append(t); sizes.append(int(rng.choice([1500, 60, 1200, int(rng.integers(1, 3000))])))
                pkts.append(pid); pid += 1
            else:
                times.append(t); sizes.append(POP); pkts.append(0)
        off.append(len(times))
    return (np.array(off, np.uint32), np.array(times, np.uint64), np.array(sizes, np.uint32),
            np.array(pkts, np.uint32), pid)


def ops_subset(off, time, size, pkt, hosts):
    """The hosts ``hosts`` of an op batch, in that order -> (off, time, size, pkt)."""
    o = [0]
    parts = []
    for h in hosts:
        a, b = int(off[h]), int(off[h + 1])
        parts.append(np.arange(a, b))
        o.append(o[-1] + b - a)
    idx = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    return np.array(o, np.uint32), time[idx], size[idx], pkt[idx]


def oracle_fate(fate_dict, n_ids):
    out = np.zeros(n_ids, np.uint64)
    for p, (k, kind) in fate_dict.items():
        out[p] = (k << 2) | kind
    return out


def exact_control_law_increment(count: int) -> int:
    """round(1e8 / sqrt(count)), half away from zero, in integers: the r with
    r - 1/2 <= 1e8 / sqrt(count) < r + 1/2, i.e. count * (2r - 1)^2 <= 4e16 < count * (2r + 1)^2."""
    from math import isqrt
    r = isqrt(10**16 // count)
    while count * (2 * r + 1) ** 2 <= 4 * 10**16:
        r += 1
    while count * (2 * r - 1) ** 2 > 4 * 10**16:
        r -= 1
    return r


# ------------------------------------------------------------------ CoDel: deep drop mode
DEEP_START = START0 + 10**9
DEEP_RING = 131072


@functools.lru_cache(maxsize=None)
def deep_drop(seed: int = 11):
    """Host 0: 131,000 packets of 1500 bytes pushed at DEEP_START, pops at +TARGET, +TARGET+INTERVAL,
    +5 s and +70 s -- the last one drops for 65 s worth of control-law steps, every drop count up
    to about 122,000.  Hosts 1..70: 0 to 600 packets each, the same first two pops, then two pops
    at times of their own, so the lanes of a wave leave the drop loop at different counts.
    The pop's loop is bounded by the packets queued (each pass pops one).
    -> SimpleNamespace(n_hosts, off, time, size, pkt, n_ids, queues, pop_ref, fate_ref)."""
    rng = np.random.default_rng(seed)
    S, SEC = DEEP_START, 10**9
    off, times, sizes, pkts = [0], [], [], []
    pid = 0
    for h in range(71):
        n = 131000 if h == 0 else int(rng.integers(0, 601))
        times += [S] * n; sizes += [1500] * n; pkts += list(range(pid, pid + n)); pid += n
        pops = ([S + TARGET, S + TARGET + INTERVAL, S + 5 * SEC, S + 70 * SEC] if h == 0 else
                [S + TARGET, S + TARGET + INTERVAL] +
                sorted(int(S + rng.integers(SEC, 60 * SEC)) for _ in range(2)))
        times += pops; sizes += [POP] * 4; pkts += [0] * 4
        off.append(len(times))
    off, time, size, pkt = (np.array(off, np.uint32), np.array(times, np.uint64), np.array(sizes, np.uint32),
                            np.array(pkts, np.uint32))
    queues, pop_ref, fate_ref = OC.run_ops(71, off, time, size, pkt)
    return SimpleNamespace(n_hosts=71, off=off, time=time, size=size, pkt=pkt, n_ids=pid, queues=queues,
                           pop_ref=np.array([int(x) for x in pop_ref], np.uint32),
                           fate_ref=oracle_fate(fate_ref, pid))


def codel_state(q) -> dict:
    """An oracle queue as shadow_amd.codel.CoDelQueues.state() reports one."""
    return {"len": len(q), "mode": q.mode, "interval_end": q.interval_end, "drop_next": q.drop_next,
            "current_drop_count": q.current_drop_count, "previous_drop_count": q.previous_drop_count,
            "total_bytes_stored": q.total_bytes_stored}
