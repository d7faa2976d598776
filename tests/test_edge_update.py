"""CPU tier of shd_routing_update_edges: its host logic (shadow_amd/csrc/edge_update.h: the edge ->
arc-slot map in build_csr's order, the call's validation and the last-entry-wins pass) compiled
alone into a program of its own (tests/edge_update_main.cpp) with the address and undefined-
behaviour sanitizers, and run against a numpy model.  The program stands alone: nothing loaded
into Python runs under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_SLOT = 0xFFFFFFFF


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("edge_update") / "edge_update")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "shadow_amd", "csrc"),
                           os.path.join(ROOT, "tests", "edge_update_main.cpp"), "-o", path])
    return path


def run(exe, text):
    out = subprocess.run([exe], input=text, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.splitlines()


def row(a):
    return " ".join(str(int(x)) for x in a)


def model_csr(V, es, ed, lat, loss, directed):
    """The out-CSR without self-loops as the prepare step lays it out: each node's arcs by
    destination, parallel arcs in GML order.  Returns (off, dst, lat, loss, edge, back) per slot."""
    keep = es != ed
    e = np.flatnonzero(keep)
    frm, to, edge, back = es[e], ed[e], e, np.zeros(len(e), bool)
    if not directed:
        frm, to = np.concatenate([frm, ed[e]]), np.concatenate([to, es[e]])
        edge, back = np.concatenate([edge, e]), np.concatenate([back, np.ones(len(e), bool)])
    order = np.lexsort((edge, to, frm))   # by node, then destination, then GML position
    off = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(frm, minlength=V), out=off[1:])
    return off, to[order], lat[edge[order]], loss[edge[order]], edge[order], back[order]


def graph(rng, V, E, directed, loops=3, parallel=4, isolated=True):
    """Shuffled edge order, parallel edges (both orientations), self-loops, a node without arcs."""
    hi = V - 1 if isolated else V   # node V - 1 has no arc
    es = rng.integers(0, hi, E).astype(np.uint32)
    ed = rng.integers(0, hi, E).astype(np.uint32)
    for k in range(parallel):   # copies of earlier edges, every other one turned round
        j = int(rng.integers(0, E // 2))
        es[E - 1 - k], ed[E - 1 - k] = (es[j], ed[j]) if k % 2 == 0 else (ed[j], es[j])
    for k in range(loops):
        es[2 * k] = ed[2 * k] = k
    p = rng.permutation(E)
    es, ed = es[p], ed[p]
    lat = rng.integers(1, 10**8, E).astype(np.uint64)
    loss = rng.random(E).astype(np.float32)
    return es, ed, lat, loss


def build(exe, V, es, ed, directed, extra=""):
    lines = run(exe, f"map {V} {len(es)} {int(directed)}\n{row(es)}\n{row(ed)}\n" + extra)
    head = lines[0].split()
    assert head[0] == "ok"
    arr = lambda s: np.array(s.split(), np.int64)  # noqa: E731
    return int(head[1]), arr(lines[1]), arr(lines[2]), arr(lines[3]), lines[4:]


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("V,E", [(9, 40), (70, 500), (300, 900)])
def test_map_sends_each_edge_to_its_own_arcs(exe, V, E, directed):
    rng = np.random.default_rng(V + E + directed)
    es, ed, lat, loss = graph(rng, V, E, directed)
    A, off, fwd, rev, _ = build(exe, V, es, ed, directed)
    m_off, m_dst, m_lat, m_loss, m_edge, m_back = model_csr(V, es, ed, lat, loss, directed)
    assert A == len(m_dst) and np.array_equal(off, m_off)
    assert off[V] == off[V - 1]   # the node without arcs
    loop = es == ed
    assert loop.sum() >= 3 and (fwd[loop] == NO_SLOT).all() and (rev[loop] == NO_SLOT).all()
    e = np.flatnonzero(~loop)
    # the slot's destination and weights are the edge's, and it lies in its source node's range
    assert np.array_equal(m_dst[fwd[e]], ed[e]) and np.array_equal(m_lat[fwd[e]], lat[e])
    assert np.array_equal(m_loss[fwd[e]], loss[e]) and np.array_equal(m_edge[fwd[e]], e)
    assert (off[es[e]] <= fwd[e]).all() and (fwd[e] < off[es[e] + 1]).all() and not m_back[fwd[e]].any()
    if directed:
        assert (rev == NO_SLOT).all()
        used = fwd[e]
    else:
        assert np.array_equal(m_dst[rev[e]], es[e]) and np.array_equal(m_edge[rev[e]], e) and m_back[rev[e]].all()
        assert (off[ed[e]] <= rev[e]).all() and (rev[e] < off[ed[e] + 1]).all()
        used = np.concatenate([fwd[e], rev[e]])
    assert np.array_equal(np.sort(used), np.arange(A))   # every slot has exactly one (edge, direction)
    # parallel arcs: distinct slots, in GML order within the destination
    pairs = {}
    for i in e:
        for a, b, s in ((es[i], ed[i], fwd[i]),) + (() if directed else ((ed[i], es[i], rev[i]),)):
            pairs.setdefault((int(a), int(b)), []).append(int(s))
    multi = [s for s in pairs.values() if len(s) > 1]
    assert multi and all(s == sorted(s) and s[-1] - s[0] == len(s) - 1 for s in multi)


def test_relabelled_copy_starts(exe):
    rng = np.random.default_rng(3)
    V = 50
    es, ed, _, _ = graph(rng, V, 200, False)
    pi = rng.permutation(V)
    A, off, fwd, rev, rest = build(exe, V, es, ed, False, f"copy {V}\n{row(pi)}\n")
    start = np.array(rest[0].split(), np.int64)
    deg = np.diff(off)
    ord_ = np.argsort(pi)   # new id -> node
    want = np.zeros(V, np.int64)
    want[ord_] = np.concatenate([[0], np.cumsum(deg[ord_])[:-1]])
    assert np.array_equal(start, want)
    # the copy's slots of all arcs are a permutation of 0 .. A-1
    e = np.flatnonzero(es != ed)
    slots = np.concatenate([start[es[e]] + fwd[e] - off[es[e]], start[ed[e]] + rev[e] - off[ed[e]]])
    assert np.array_equal(np.sort(slots), np.arange(A))


def bits(loss):
    return np.asarray(loss, np.float32).view(np.uint32)


def update(idx, lat, loss_bits, mask=0):
    return f"update {len(idx)} {mask}\n{row(idx)}\n{row(lat)}\n{row(loss_bits)}\n"


def test_last_entry_wins_and_refusals(exe):
    E = 20
    head = f"map 5 {E} 0\n{row(np.arange(E) % 4)}\n{row((np.arange(E) + 1) % 4)}\n"
    ok = lambda text: run(exe, head + text)[4:]  # noqa: E731
    # an edge named three times and one named twice: the last entries, last to first
    idx = [3, 7, 3, 19, 7, 3, 0]
    out = ok(update(idx, [5] * 7, bits([0.5] * 7)))
    assert out[0] == "ok 4" and out[1].split() == ["6", "5", "4", "3"]
    # a second call starts over (the stamps are per call), then an empty one
    out = ok(update(idx, [5] * 7, bits([0.5] * 7)) + update([3, 3], [1, 2], bits([0.0, 1.0])) + update([], [], []))
    assert out[2] == "ok 1" and out[3].split() == ["1"] and out[4] == "ok 0"
    # model: numpy keeps the last of repeated indices too
    rng = np.random.default_rng(8)
    idx = rng.integers(0, E, 200)
    lat = rng.integers(1, 100, 200)
    out = ok(update(idx, lat, bits(rng.random(200))))
    keep = np.array(out[1].split(), np.int64)
    want = np.zeros(E, np.int64)
    want[idx] = lat
    got = np.zeros(E, np.int64)
    got[idx[keep]] = lat[keep]
    assert out[0] == f"ok {len(np.unique(idx))}" and np.array_equal(got, want) and (np.diff(keep) < 0).all()
    # the loss bounds that pass: -0.0, 0.0, 1.0
    assert ok(update([0, 1, 2], [1, 1, 2**63], [0x80000000, 0, 0x3F800000]))[0] == "ok 3"
    # refusals: each NULL array, an index past the edges, latency 0, loss below 0, above 1, NaN, infinity
    for mask in (1, 2, 4):
        assert ok(update([1], [1], [0], mask))[0] == "refused"
    assert ok(update([], [], [], 7))[0] == "ok 0"   # NULL arrays with n == 0 are fine
    assert ok(update([E], [1], [0]))[0] == "refused"
    assert ok(update([0, E - 1], [1, 0], [0, 0]))[0] == "refused"
    for bad in (np.float32(-1e-9), np.nextafter(np.float32(1), np.float32(2)), np.float32("nan"),
                np.float32("inf")):
        assert ok(update([0, 1], [1, 1], bits([0.25, bad])))[0] == "refused"
    # a refused call stamps nothing: the next call keeps what it names
    out = ok(update([2, E], [1, 1], [0, 0]) + update([2], [1], [0]))
    assert out[0] == "refused" and out[1] == "ok 1"


def test_exported_names():
    from shadow_amd._native import EXPORTED
    for name in ("shd_routing_update_edges", "shd_relay_retable"):
        assert name in EXPORTED
