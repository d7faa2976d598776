"""The token bucket's and the CoDel queue's time arithmetic at the u64 seams, CPU tier: the Python
oracles (oracle/token_bucket.py, oracle/codel.py) and the C restatement (oracle/c/queues.c) on hand
cases whose expectations are derived from the reference's lines (tests/time_seams.py), then the two
against each other on seam fuzzes.  tests/test_time_seams_gpu.py runs the same inputs on the device.

What was read in the reference for this (FlyearthR/shadow), end to end, and what each operation
does at the seam:

token_bucket.rs
  :43      new_inner: None unless capacity, increment > 0 and the interval non-zero.  Its interval
           is a SimulationTime and its last_refill an EmulatedTime, so a value above SIMTIME_MAX /
           EMUTIME_MAX cannot be passed at all: refused at setup (ValueError / SHD_ERR_INVALID).
  :128,152 now.duration_since(last_refill): panics for now < last_refill and for a difference above
           SIMTIME_MAX (emulated_time.rs:79-87).  [was: only the first]
  :132-135 as_nanos (u128) checked_div: the interval is non-zero; :138,149 try_into u64 of a
           quotient of u64s: cannot fail.
  :136-138 u64::saturating_mul; :141-144 u64::saturating_add, clamp to the capacity.
  :147-150 SimulationTime::saturating_mul, EmulatedTime::saturating_add.
  :156     interval - span: SimulationTime::sub unwraps checked_sub; span < interval here.
  :99      u64::saturating_sub; :103-104 / and % by the increment (non-zero); :117 checked_sub(1)
           of a count >= 2; :115-117 SimulationTime::saturating_add / saturating_mul.
  relay/mod.rs forward_later: now + duration as EmulatedTime::saturating_add.
simulation_time.rs
  :36-46   from_c_simtime: None for SIMTIME_INVALID (2^64 - 1) and above SIMTIME_MAX.
  :135-148 saturating_add / saturating_mul: checked u64 op, *overflow* -> SIMTIME_MAX, then
           from_c_simtime(..).unwrap(): a result in (SIMTIME_MAX, 2^64) panics.
emulated_time.rs
  :51-57   from_c_emutime: None for 2^64 - 1.   :73-75 to_abs_simtime = duration_since(SIMULATION_START).
  :84-93   checked_duration_since (None: earlier is later, or above SIMTIME_MAX);
           saturating_duration_since: ZERO in both cases.  [was: a plain saturating subtraction]
  :95-108  checked_add / saturating_add: EMUTIME_MAX on u64 overflow and on 2^64 - 1.
           [was, in the CoDel restatements: 2^64 - 1]
codel_queue.rs
  :210-212 usize::saturating_sub of the byte total; :160-162 of the drop counts; :184 count += 1
           (bounded by the packets queued); :308 total += size (usize; 2^32 packets of < 2^32 bytes).
  :215     saturating_duration_since (above).   :259 EmulatedTime::saturating_add (above).
  :252,269 plain comparisons of EmulatedTimes.   :279 saturating_duration_since; INTERVAL.saturating_mul(16)
           = 1.6e9, no seam.
  :287-300 apply_control_law: NOT an EmulatedTime::saturating_add.  original = time.to_abs_simtime()
           panics for a time before SIMULATION_START; original.saturating_add(increment) is
           SimulationTime's: original <= SIMTIME_MAX and increment <= 1e8, so the u64 sum never
           overflows and a sum above SIMTIME_MAX meets the unwrap -- a drop time past EMUTIME_MAX
           panics, it does not saturate; from_abs_simtime(adjusted) = SIMULATION_START + adjusted
           <= EMUTIME_MAX cannot fail.  [was: saturating at 2^64 - 1, no panic]  from_nanos(div.round()
           as u64): 0 < div <= 1e8, the cast is exact.

Branches that no input can reach, and why (restated all the same, not tested):
  * lazy_refill's second duration_since (:152) and the product (:147-149) panicking or saturating:
    once the first span is a SimulationTime, interval * n <= span <= SIMTIME_MAX, so the product is
    exact, last_refill + it <= now does not saturate, and the new span is span mod interval.  The
    fuzz confirms it: no relay panics there.
  * was_dropping_recently's ZERO for a difference above SIMTIME_MAX: drop_next is only ever a
    control law's result, >= SIMULATION_START, and now <= EMUTIME_MAX = SIMULATION_START + SIMTIME_MAX.
  * SimulationTime::saturating_add saturating in the control law (above), and any of these with a
    time of 2^64 - 1: EMUTIME_INVALID is no EmulatedTime, the reference's clock cannot give it.
"""
import numpy as np
import pytest

from oracle import codel as OC
from oracle import corc
from oracle import token_bucket as O
from tests import time_seams as S

EMAX, SMAX, START0 = S.EMAX, S.SMAX, S.START0


# ------------------------------------------------------------------ token bucket
@pytest.mark.parametrize("case", S.BUCKET_CASES, ids=lambda c: c["name"])
def test_bucket_hand_case_python(case):
    tb = O.TokenBucket(*case["bucket"])
    pending = 0
    for (now, size), want in zip(case["attempts"], case["expect"]):
        if want == "panic":
            with pytest.raises(O.ReferencePanic) as e:
                tb.conforming_remove(size, now)
            assert e.value.kind == case["kind"]
            return
        if now < pending:
            got = (S.SKIPPED, pending)
        else:
            ok, v = tb.conforming_remove(size, now)
            got = (S.FORWARDED, v) if ok else (S.BLOCKED, v)
            if not ok:
                pending = O.emutime_sat_add(now, v)   # Relay::forward_later
        assert got == want, (now, size)
    assert (tb.balance, tb.last_refill, pending) == case["state"]


@pytest.mark.parametrize("case", S.BUCKET_CASES, ids=lambda c: c["name"])
def test_bucket_hand_case_c(case):
    times, sizes = S.bucket_case_ops(case)
    c, i, v, l = case["bucket"]
    st, val, panics = corc.tb_run([c], [i], [v], [l], [0, len(times)], times, sizes, [0] * len(times))
    clean = [w for w in case["expect"] if w != "panic"]
    assert panics == (len(clean) != len(case["expect"]))
    assert list(zip(st.tolist(), val.tolist()))[:len(clean)] == clean


def test_bucket_setup_values_outside_the_types():
    O.TokenBucket(1, 1, SMAX, EMAX)
    for itv, last in ((SMAX + 1, 0), (2**64 - 1, 0), (1, EMAX + 1)):
        with pytest.raises(ValueError):
            O.TokenBucket(1, 1, itv, last)


def test_bucket_fuzz_python_vs_c():
    """4,000 seam relays: Python and C agree on which relays panic and, on the clean ones, on every
    status and value.  1,047 relays panic (1,024 first span, 18 sum, 5 product, no second span:
    unreachable, see the module docstring), 2,953 are clean."""
    F = S.bucket_fuzz()
    n = len(F.res)
    print("bucket fuzz:", len(F.clean), "clean,", len(F.panicking), "panicking",
          {k: sum(r.kind == k for r in F.res) for k in S.KINDS})
    assert 0.05 * n <= len(F.panicking) <= 0.50 * n
    assert {r.kind for r in F.res} <= set(S.KINDS) | {None}
    # the clean relays alone: no panic in C, everything equal
    cap, inc, itv, last, off, time, size = S.bucket_subset(F, F.clean)
    st, val, panics = corc.tb_run(cap, inc, itv, last, off, time, size, np.zeros(len(time), np.uint8))
    assert panics == 0
    assert st.tolist() == [x for r in F.clean for x in F.res[r].status]
    assert val.tolist() == [x for r in F.clean for x in F.res[r].value]
    # the panicking ones alone: a relay panics at most once in C (it is skipped from then on), so
    # a total equal to their number is every one of them
    cap, inc, itv, last, off, time, size = S.bucket_subset(F, F.panicking)
    _, _, panics = corc.tb_run(cap, inc, itv, last, off, time, size, np.zeros(len(time), np.uint8))
    assert panics == len(F.panicking)


# ------------------------------------------------------------------ CoDel
def _run_case_python(case):
    """-> per pop (returned, dropped, queue) or "panic" (the last)."""
    q = OC.CoDelQueue()
    out = []
    for op in case["ops"]:
        if op[0] == "push":
            q.push(op[2], op[3], op[1])
            continue
        before = len(q.dropped)
        try:
            got = q.pop(op[1])
        except O.ReferencePanic:
            out.append("panic")
            break
        out.append((got, q.dropped[before:], S.codel_state(q)))
    return out


@pytest.mark.parametrize("case", S.CODEL_CASES, ids=lambda c: c["name"])
def test_codel_hand_case_python(case):
    got = _run_case_python(case)
    assert len(got) == len(case["expect"])
    for g, w in zip(got, case["expect"]):
        if w == "panic":
            assert g == "panic"
            continue
        assert g != "panic" and g[0] == w[0] and g[1] == w[1]
        for k, v in w[2].items():
            assert g[2][k] == v, (k, g[2])


@pytest.mark.parametrize("case", S.CODEL_CASES, ids=lambda c: c["name"])
def test_codel_hand_case_c(case):
    ops = [(o[1], o[3], o[2]) if o[0] == "push" else (o[1], S.POP, 0) for o in case["ops"]]
    n_ids = 1 + max(o[2] for o in case["ops"] if o[0] == "push")
    pop, fate, panicked = corc.codel_run_checked(1, [0, len(ops)], [o[0] for o in ops], [o[1] for o in ops],
                                                 [o[2] for o in ops], n_ids)
    assert bool(panicked[0]) == (case["expect"][-1] == "panic")
    pops = [k for k, o in enumerate(ops) if o[1] == S.POP]
    for k, w in zip(pops, case["expect"]):
        if w == "panic":
            break
        assert int(pop[k]) == (S.POP if w[0] is None else w[0])
        for d in w[1]:
            assert int(fate[d]) == (k << 2) | 2
        if w[0] is not None:
            assert int(fate[w[0]]) == (k << 2) | 1


def test_control_law_every_count_exact():
    """round(1e8 / sqrt(count)) for every count the deep-drop test reaches, against exact integer
    arithmetic; 106,521 is the one whose quotient is within 1e-6 of a half."""
    for c in range(1, 130_001):
        assert OC.control_law_increment(c) == S.exact_control_law_increment(c), c
    assert OC.control_law_increment(0) == OC.INTERVAL
    r = S.exact_control_law_increment(106_521)
    assert r == 306_395 and 106_521 * (2 * r + 1) ** 2 - 4 * 10**16 < 4 * 10**16 * 1e-11
    t = START0 + 12345
    assert OC.apply_control_law(t, 106_521) == t + 306_395
    # the law's own seam: exactly EMUTIME_MAX is a value, one past it panics; before the start too
    assert OC.apply_control_law(EMAX - OC.INTERVAL, 1) == EMAX
    for time, count in ((EMAX - OC.INTERVAL + 1, 1), (EMAX, 130_000), (START0 - 1, 1), (0, 4)):
        with pytest.raises(O.ReferencePanic):
            OC.apply_control_law(time, count)


SEAM_STEPS = [0, 1, 2 * 10**6, 9 * 10**6, 10**7, 6 * 10**7, 10**8, 10**8 + 1, 4 * 10**8, 17 * 10**8]


def codel_seam_batches():
    """Three kinds of hosts in one batch: near the top of the range (adds saturate, drop mode
    panics), at the bottom (the control law before SIMULATION_START panics), and stamped before
    SIMULATION_START - 1 but popped near the top (durations above SIMTIME_MAX)."""
    rng = np.random.default_rng(4242)
    top = [EMAX - 2 * 10**9, EMAX - 10**9, EMAX - 3 * 10**8, EMAX - 10**8 - 10**7]
    a = S.codel_ops(rng, 150, 60, top, SEAM_STEPS)
    b = S.codel_ops(rng, 100, 60, [0, 1, START0 - 10**9, START0 - 2 * 10**8, START0 - 1, START0], SEAM_STEPS, a[4])
    c = S.codel_ops(rng, 100, 40, top, SEAM_STEPS, b[4], first_push_before=(START0 - 2, EMAX - 10**9))
    off = np.concatenate([a[0], b[0][1:] + a[0][-1], c[0][1:] + a[0][-1] + b[0][-1]]).astype(np.uint32)
    cat = lambda k: np.concatenate([a[k], b[k], c[k]])   # noqa: E731
    return 350, off, cat(1), cat(2), cat(3), c[4]


def test_codel_seam_fuzz_python_vs_c():
    """Op batches at both ends of the time range: the same hosts panic in Python and in C, and the
    clean hosts agree on every pop result and packet fate."""
    H, off, t, sz, pk, n_ids = codel_seam_batches()
    bad = []
    _, pop_ref, fate_ref = OC.run_ops(H, off, t, sz, pk, panicked=bad)
    pop, fate, panicked = corc.codel_run_checked(H, off, t, sz, pk, n_ids)
    print("codel seam fuzz:", H - len(bad), "clean hosts,", len(bad), "panicking")
    assert sorted(bad) == np.flatnonzero(panicked).tolist()
    assert 0.05 * H <= len(bad) <= 0.5 * H
    ref_fate = S.oracle_fate(fate_ref, n_ids)
    for h in range(H):
        if panicked[h]:
            continue
        a, b = int(off[h]), int(off[h + 1])
        assert pop[a:b].tolist() == [int(x) for x in pop_ref[a:b]], h
        ids = pk[a:b][sz[a:b] != S.POP]
        assert np.array_equal(fate[ids], ref_fate[ids]), h


def test_deep_drop_python_vs_c():
    """The deep-drop run (131,000 packets, 122,626 drops in one pop): the counts the scenario was
    designed for, and the C restatement's pops and fates -- 122,626 control-law sums deep."""
    D = S.deep_drop()
    q = D.queues[0]
    assert (q.current_drop_count, len(q)) == (122_626, 8_370) and q.current_drop_count > 106_521
    pop, fate = corc.codel_run(D.n_hosts, D.off, D.time, D.size, D.pkt, D.n_ids)
    assert np.array_equal(pop, D.pop_ref)
    assert np.array_equal(fate, D.fate_ref)
