"""CPU tier of the bucket re-rate (shd_tb_update, shd_*_update_buckets, shd_window_update_bandwidth):
the model the GPU tests compare with (tests/rate_model.py), on hand cases with the numbers of the
reference's own bucket tests (token_bucket.rs:187-246: a bucket of 100 tokens, 10 per 10 ms), and
the call's host logic (shadow_amd/csrc/rate_update.h: validation, last entry wins, the records)
compiled alone into a program of its own (tests/rate_update_main.cpp) with the address and
undefined-behaviour sanitizers.  The program stands alone: nothing loaded into Python runs under a
sanitizer."""
import os
import subprocess

import numpy as np
import pytest

from oracle.token_bucket import MS, ReferencePanic, TokenBucket, create_token_bucket
from tests.rate_model import rerate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = 10**9


def drained(now=T0):
    tb = TokenBucket(100, 10, 10 * MS, now)
    assert tb.conforming_remove(100, now) == (True, 0)
    return tb


def test_model_refills_under_the_old_rate_then_clamps():
    # 5 whole intervals and a half at the old rate: 50 tokens (test_refill_after_multiple_intervals)
    at = T0 + 55 * MS
    new = rerate(drained(), at, 1000, 7, 3 * MS)
    assert (new.capacity, new.balance, new.refill_increment, new.refill_interval) == (1000, 50, 7, 3 * MS)
    # the same refill, a capacity below it: clamped
    assert rerate(drained(), at, 30, 7, 3 * MS).balance == 30
    # the refill itself is clamped to the old capacity first (test_capacity_limit: 100 after 15 intervals)
    assert rerate(drained(), T0 + 150 * MS, 5000, 1, MS).balance == 100
    # a full bucket stays full only up to the new capacity
    assert rerate(TokenBucket(100, 10, 10 * MS, T0), T0, 40, 10, 10 * MS).balance == 40


def test_model_new_grid_starts_at_the_call():
    at = T0 + 55 * MS
    new = rerate(drained(), at, 1000, 7, 3 * MS)
    assert new.last_refill == at   # not the old grid's T0 + 50 ms
    # the next refill is one new interval after `at`: 2 ms later nothing, 3 ms later one increment
    assert new.conforming_remove(50, at + 2 * MS) == (True, 0)
    assert new.conforming_remove(8, at + 2 * MS + 999_999)[0] is False
    assert new.conforming_remove(7, at + 3 * MS) == (True, 0)


def test_model_none_to_bucket_and_back():
    new = rerate(None, T0 + 5, *create_token_bucket(10**6))
    assert (new.capacity, new.balance, new.refill_increment, new.refill_interval, new.last_refill) == \
        (2500, 2500, 1000, MS, T0 + 5)   # full, as every new bucket
    assert rerate(drained(), T0 + 55 * MS, 0, 0, 0) is None
    assert rerate(None, T0, 0, 0, 0) is None


def test_model_refusals():
    with pytest.raises(ReferencePanic):
        rerate(drained(), T0 - 1, 100, 10, 10 * MS)     # `at` before last_refill
    with pytest.raises(ReferencePanic):
        rerate(drained(), T0 - 1, 0, 0, 0)              # also on the way to no bucket
    for partial in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1)):
        with pytest.raises(ValueError):
            rerate(None, T0, *partial)
    rerate(drained(), T0, 100, 10, 10 * MS)             # at == last_refill is fine


# ---- the host logic, as a program of its own under the sanitizers ----

@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("rate_update") / "rate_update")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "shadow_amd", "csrc"),
                           os.path.join(ROOT, "tests", "rate_update_main.cpp"), "-o", path])
    return path


def run(exe, text):
    out = subprocess.run([exe], input=text, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.splitlines()


def row(a):
    return " ".join(str(int(x)) for x in a)


def update(hosts, cap, inc, itv, at=0, mask=0):
    return f"update {len(hosts)} {mask} {at}\n{row(hosts)}\n{row(cap)}\n{row(inc)}\n{row(itv)}\n"


def parse(lines):
    """The answers of consecutive update commands: None (refused) or the records as tuples."""
    out, i = [], 0
    while i < len(lines):
        if lines[i] == "refused":
            out.append(None)
            i += 1
            continue
        k = int(lines[i].split()[1])
        out.append([tuple(int(x) for x in ln.split()) for ln in lines[i + 1:i + 1 + k]])
        i += 1 + k
    return out


def test_last_entry_wins(exe):
    head = "stage 10 0\n"
    # host 3 named three times, host 7 twice: the last entries, in record order (last to first)
    hosts, cap = [3, 7, 3, 9, 7, 3, 0], [11, 12, 13, 14, 15, 16, 17]
    got, again, empty = parse(run(exe, head + update(hosts, cap, [1] * 7, [2] * 7) +
                                  update([3, 3], [5, 0], [5, 0], [5, 0]) + update([], [], [], [])))
    assert got == [(0, 17, 1, 2), (3, 16, 1, 2), (7, 15, 1, 2), (9, 14, 1, 2)]
    assert again == [(3, 0, 0, 0)] and empty == []   # stamps are per call; all-zero is "no bucket"; n == 0 is fine
    # against numpy, which keeps the last of repeated indices too
    rng = np.random.default_rng(5)
    H, n = 40, 500
    hosts = rng.integers(0, H, n)
    cap = rng.integers(1, 10**6, n)
    (rec,) = parse(run(exe, f"stage {H} 0\n" + update(hosts, cap, cap + 1, cap + 2)))
    want = np.zeros(H, np.int64)
    want[hosts] = cap
    assert len(rec) == len(np.unique(hosts)) == len({r[0] for r in rec})
    assert all(r[1:] == (want[r[0]], want[r[0]] + 1, want[r[0]] + 2) for r in rec)


def test_refusals(exe):
    head = "stage 10 1000\n"
    one = lambda text: parse(run(exe, head + text))[0]  # noqa: E731
    ok = ([1], [5], [5], [5])
    assert one(update(*ok, at=1000)) == [(1, 5, 5, 5)]            # at == prev_end is allowed
    assert one(update(*ok, at=999)) is None                       # at below prev_end
    assert one(update([], [], [], [], at=999)) == []              # (an empty call does nothing: fine at any time)
    for mask in (1, 2, 4, 8):                                     # each NULL array with n > 0
        assert one(update(*ok, at=1000, mask=mask)) is None
    assert one(update([], [], [], [], at=1000, mask=15)) == []    # NULL arrays with n == 0 are fine
    assert one(update([9], [5], [5], [5], at=1000)) == [(9, 5, 5, 5)]
    assert one(update([10], [5], [5], [5], at=1000)) is None      # index == the host count
    assert one(update([0, 2**32 - 1], [5, 5], [5, 5], [5, 5], at=1000)) is None
    for c, i, n in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (0, 0, 5), (5, 0, 0), (0, 5, 0)):   # some but not all zero
        assert one(update([1, 2], [5, c], [5, i], [5, n], at=1000)) is None
    # ... also in an entry that a later one of the same host would replace
    assert one(update([1, 1], [0, 5], [5, 5], [5, 5], at=1000)) is None
    # a refused call stamps nothing: the next call keeps what it names
    a, b = parse(run(exe, head + update([2, 10], [5, 5], [5, 5], [5, 5], at=1000) + update([2], [6], [6], [6], at=1000)))
    assert a is None and b == [(2, 6, 6, 6)]
    # a stage set up again with another host count starts its stamps over
    a, b = parse(run(exe, "stage 4 0\n" + update([3], [1], [1], [1]) + "stage 2 0\n" + update([1, 3], [1, 1], [1, 1], [1, 1])))
    assert a == [(3, 1, 1, 1)] and b is None


def test_refusals_of_values_outside_the_time_types(exe):
    """An interval above SIMTIME_MAX is no SimulationTime, an `at` above EMUTIME_MAX no EmulatedTime
    (the refill's `now`, the new bucket's last_refill): refused; the types' largest values pass."""
    smax, emax = 17500059273709551614, 2**64 - 2
    one = lambda text: parse(run(exe, "stage 10 0\n" + text))[0]  # noqa: E731
    assert one(update([1], [5], [5], [smax], at=emax)) == [(1, 5, 5, smax)]
    assert one(update([1], [5], [5], [smax + 1], at=1000)) is None
    assert one(update([1, 2], [5, 5], [5, 5], [5, 2**64 - 1], at=1000)) is None
    assert one(update([2, 2], [5, 5], [5, 5], [smax + 1, 5], at=1000)) is None   # also in a replaced entry
    assert one(update([1], [5], [5], [5], at=emax + 1)) is None
    assert one(update([1], [0], [0], [0], at=emax + 1)) is None
    assert one(update([], [], [], [], at=emax + 1)) == []                        # (an empty call does nothing)
    # the model refuses the same values
    for itv, at in ((smax + 1, 1000), (5, emax + 1)):
        with pytest.raises(ValueError):
            rerate(None, at, 5, 5, itv)


def test_bandwidth_rows_are_create_token_bucket(exe):
    rates = [0, 1, 999, 1000, 1001, 125_000, 10**9, 2**40 + 12345]
    lines = run(exe, "".join(f"bandwidth {b}\n" for b in rates))
    assert [tuple(int(x) for x in ln.split()) for ln in lines] == [create_token_bucket(b) for b in rates]


def test_exported_names():
    from shadow_amd._native import EXPORTED
    for name in ("shd_tb_update", "shd_inbound_update_buckets", "shd_outbound_update_buckets",
                 "shd_window_update_bandwidth"):
        assert name in EXPORTED
