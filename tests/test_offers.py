"""CPU tier of the staged offers (shd_offers_group): the Python staging (shadow_amd.outbound.OfferStages)
against a stable numpy group-by, and the engine's host-side part (shadow_amd/csrc/offer_stage.h: the
record's word layout and the stages' shape check) compiled into a program of its own
(tests/offer_stage_main.cpp) with the address and undefined-behaviour sanitizers and run against the
same model.  The program stands alone: nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

from shadow_amd.outbound import OfferStages, group_offers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 2**40 + 12345   # a time_base above 2^32


def random_offers(rng, n_hosts, first_host=0, max_per_host=6, n_dst=1000, lengths=None):
    """Grouped offers of n_hosts hosts: (off, time, prio, size, payload, dst, pkt, sock).  A third
    of the hosts have none; time offsets reach 2^32 - 1, keys use all 64 bits."""
    cnt = rng.integers(0, max_per_host + 1, n_hosts) * (rng.random(n_hosts) < 0.67)
    if lengths is not None:
        cnt[:len(lengths)] = lengths
    off = np.zeros(n_hosts + 1, np.uint32)
    off[1:] = np.cumsum(cnt)
    n = int(off[-1])
    t = rng.integers(0, 2**32, n, dtype=np.uint64)
    if n:
        t[rng.integers(0, n)] = 2**32 - 1
    host = np.repeat(np.arange(n_hosts), cnt)
    t = t[np.lexsort((t, host))]   # time order within a host
    return (off, np.uint64(BASE) + t, rng.integers(0, 2**64, n, dtype=np.uint64),
            rng.integers(52, 1501, n).astype(np.uint32), rng.integers(0, 1449, n).astype(np.uint32),
            rng.integers(0, n_dst, n).astype(np.uint32), rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32),
            rng.integers(0, 2**64, n, dtype=np.uint64))


def stage(cols, n_threads, words, first_host=0, idle=(), seed=7):
    return OfferStages.from_grouped(*cols[:7], time_base=BASE, n_threads=n_threads, first_host=first_host,
                                    sock=cols[7] if words == 10 else None, words=words, idle=idle, seed=seed)


def same_grouped(got, cols, words):
    """got: (off, time, prio, sock, size, payload, dst, pkt) against the grouped columns the
    stages were dealt from."""
    off, time, prio, size, payload, dst, pkt, sock = cols
    want = (off, time, prio, sock if words == 10 else None, size, payload, dst, pkt)
    for name, g, w in zip(("off", "time", "prio", "sock", "size", "payload", "dst", "pkt"), got, want):
        if w is None:
            assert g is None, name
        else:
            assert g.dtype == w.dtype and np.array_equal(g, w), name


@pytest.mark.parametrize("words", [8, 10])
@pytest.mark.parametrize("n_threads,idle", [(1, ()), (3, ()), (3, (0,)), (3, (1,)), (3, (2,)), (16, ()), (16, (0, 7, 15))])
def test_stages_decode_to_the_grouped_columns(n_threads, idle, words):
    """Hosts dealt to threads in shuffled order, an idle thread first, in the middle and last, runs
    of count 0 and hosts without a run: the stable group-by of the stages gives the columns back."""
    rng = np.random.default_rng(100 * n_threads + words + len(idle))
    cols = random_offers(rng, 97)
    st = stage(cols, n_threads, words, idle=idle)
    assert st.n_stages == n_threads and all(len(st.run_host[k]) == 0 for k in idle)
    counts = np.concatenate(st.run_count)
    assert (counts == 0).any() and len(counts) < 97   # runs of count 0, and hosts without a run
    assert all(o.shape[1] == words for o in st.offers) and st.n_offers == int(cols[0][-1])
    same_grouped(st.grouped(BASE, 97), cols, words)


def test_first_host_and_refusals_of_the_model():
    rng = np.random.default_rng(5)
    cols = random_offers(rng, 40)
    st = stage(cols, 3, 8, first_host=700)
    assert min(int(h.min()) for h in st.run_host if len(h)) >= 700
    same_grouped(st.grouped(BASE, 40, 700), cols, 8)
    with pytest.raises(ValueError, match="outside"):
        st.grouped(BASE, 40, 0)
    with pytest.raises(ValueError, match="outside"):
        st.grouped(BASE, int(max(h.max() for h in st.run_host if len(h))) - 700, 700)   # one host short
    dup = OfferStages(st.run_host + [st.run_host[0][:1]], st.run_count + [np.zeros(1, np.uint32)],
                      st.offers + [np.zeros((0, 8), np.uint32)], 8)
    with pytest.raises(ValueError, match="two runs"):
        dup.grouped(BASE, 40, 700)
    with pytest.raises(ValueError, match="add up"):
        group_offers(st.run_host, st.run_count, [o[:-1] if len(o) else o for o in st.offers], 8, BASE, 40, 700)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("offer_stage") / "offer_stage")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "shadow_amd", "csrc"),
                           os.path.join(ROOT, "tests", "offer_stage_main.cpp"), "-o", path])
    return path


def script(st, need_sock, n_hosts, first_host=0, words=None, masks=None, stage_offers=None, no_tables=False):
    """One `group` command: the stages as they are, or bent -- another width on the command line,
    NULL arrays (masks), stage_offers that differ from the records given."""
    words = st.words if words is None else words
    lines = [f"group {words} {int(need_sock)} {BASE} {first_host} {n_hosts} {st.n_stages} {int(no_tables)}"]
    for k in range(st.n_stages):
        n_off = len(st.offers[k]) if stage_offers is None else stage_offers[k]
        rec = st.offers[k].reshape(-1)[:n_off * words]
        assert len(rec) == n_off * words
        lines.append(f"{len(st.run_host[k])} {n_off} {0 if masks is None else masks[k]}")
        lines.append(" ".join(f"{h} {c}" for h, c in zip(st.run_host[k].tolist(), st.run_count[k].tolist())))
        lines.append(" ".join(map(str, rec.tolist())))
    return "\n".join(lines) + "\n"


def run(exe, text):
    out = subprocess.run([exe], input=text, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.splitlines()


def parse(lines, words):
    head = lines[0].split()
    assert head[0] == "ok", lines[0]
    rows = [np.array(x.split(), np.uint64) for x in lines[1:9]]
    kinds = (np.uint32, np.uint64, np.uint64, np.uint64, np.uint32, np.uint32, np.uint32, np.uint32)
    got = [r.astype(k) for r, k in zip(rows, kinds)]
    if words == 8:
        assert not got[3].any()
        got[3] = None
    return int(head[1]), int(head[2]), got


@pytest.mark.parametrize("words", [8, 10])
@pytest.mark.parametrize("n_threads,idle,first_host", [(1, (), 0), (3, (0,), 0), (3, (1,), 700), (16, (15,), 0)])
def test_program_groups_like_the_model(exe, n_threads, idle, first_host, words):
    rng = np.random.default_rng(n_threads + words)
    cols = random_offers(rng, 70)
    st = stage(cols, n_threads, words, first_host=first_host, idle=idle)
    n_runs, n, got = parse(run(exe, script(st, words == 10, 70, first_host)), words)
    assert (n_runs, n) == (sum(len(h) for h in st.run_host), st.n_offers)
    same_grouped(got, cols, words)


def test_program_refusals(exe):
    rng = np.random.default_rng(9)
    cols = random_offers(rng, 30, lengths=[3, 0, 2])
    st = stage(cols, 3, 10)
    assert all(len(h) for h in st.run_host) and all(len(o) > 1 for o in st.offers)
    ok = lambda text: run(exe, text)[0].split()[0]  # noqa: E731
    assert ok(script(st, True, 30)) == "ok"
    # zero stages: nothing to group, every offset 0
    empty = OfferStages([], [], [], 8)
    lines = run(exe, script(empty, False, 5))
    assert lines[0] == "ok 0 0" and lines[1].split() == ["0"] * 6
    assert ok(script(empty, False, 5, no_tables=True)) == "ok"   # (no stage: the tables are not read)
    assert ok(script(st, True, 30, no_tables=True)) == "refused"
    # counts that do not add up: a stage one offer short, and one with an offer too many
    short = [len(o) for o in st.offers]
    short[1] -= 1
    assert ok(script(st, True, 30, stage_offers=short)) == "refused"
    st8 = stage(cols, 3, 8)
    more = OfferStages(st8.run_host, st8.run_count, [np.concatenate([o, o[:1]]) for o in st8.offers], 8)
    assert ok(script(more, False, 30)) == "refused"
    # a NULL array with a count that is not zero: each of the three
    for bit in (1, 2, 4):
        assert ok(script(st, True, 30, masks=[0, bit, 0])) == "refused"
    # ... and NULL arrays of a stage without runs or offers are fine
    idle = stage(cols, 3, 10, idle=(1,))
    assert ok(script(idle, True, 30, masks=[0, 7, 0])) == "ok"
    # widths: 8 under a socket discipline, and neither 8 nor 10
    assert ok(script(st8, True, 30)) == "refused"
    assert ok(script(st8, False, 30)) == "ok"
    assert ok(script(st, False, 30)) == "ok"     # 10 under a plain discipline: the column is ignored later
    seven = OfferStages(st8.run_host, st8.run_count, [o[:, :7] for o in st8.offers], 7)
    assert ok(script(seven, False, 30)) == "refused"
    # the two checks the device makes, walked on the host
    assert ok(script(st, True, 2)) == "nohost"                  # host 2 has a run
    assert ok(script(st, True, 30, first_host=1)) == "nohost"   # and so has host 0
    dup = OfferStages(st.run_host + [st.run_host[0][:1]], st.run_count + [np.zeros(1, np.uint32)],
                      st.offers + [np.zeros((0, 10), np.uint32)], 10)
    assert ok(script(dup, True, 30)) == "dup"


def test_exported_names():
    from shadow_amd._native import EXPORTED
    for name in ("shd_offers_group", "shd_window_close_staged", "shd_window_records_host", "shd_window_sent_host"):
        assert name in EXPORTED
