"""GPU tests of the dense routing build's 16-byte accesses: prune_fused's row load (aligned 4-word
chunks of the row's memory span mapped back to columns, head and tail chunks word by word), the
survivors' loss gather, the NN lists at two entries per lane, and sssp_lds_shadow's vector head
(arc ranges) and tail (four columns per thread) with their scalar fallbacks.  Every case
builds the full table with ALGO_AUTO and compares it bit for bit with the C restatement
(corc.routing), and `arcs_kept` with the numpy model's count (tests/prune_fused_model.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import corc
from tests import prune_fused_model as model
from tests.graphs import engine_graph_from_edges
from tests.prune_fused_cases import case as fused_case

pytestmark = pytest.mark.gpu

AUTO, PRUNED = 0, 2


def _latencies(rng, mode, m):
    from shadow_amd import synth
    if mode == "const":   # every arc ties: S1 = V - 1, nothing prunes
        return np.full(m, 5 * synth.MS, np.uint64)
    if mode == "few":     # three values: ties under the strict compare
        return rng.integers(1, 4, size=m).astype(np.uint64) * np.uint64(synth.MS)
    if mode == "ns":      # ns-granular
        return rng.integers(1_000, 10_000_000, size=m).astype(np.uint64)
    assert mode == "rand"
    return rng.integers(1, 301, size=m).astype(np.uint64) * np.uint64(synth.MS)


def _graph(n, mode, directed, seed, parallel=False):
    """A complete graph with self-loops: undirected (synth.complete_graph, latencies rewritten unless
    `rand`) or directed with every ordered pair its own arc; `parallel`: one more arc 0 -> 1, which
    takes the graph off the dense-CSR input."""
    from shadow_amd import synth
    rng = np.random.default_rng(seed)
    if not directed:
        el = synth.complete_graph(n, seed)
        arcs = el.src != el.dst
        if mode != "rand":
            el.latency_ns[arcs] = _latencies(rng, mode, int(arcs.sum()))
    else:
        s, d = np.nonzero(~np.eye(n, dtype=bool))
        loops = np.arange(n)
        lat = np.concatenate([rng.integers(1, 51, size=n).astype(np.uint64) * np.uint64(synth.MS),
                              _latencies(rng, mode, len(s))])
        s, d = np.concatenate([loops, s]).astype(np.uint32), np.concatenate([loops, d]).astype(np.uint32)
        loss = rng.uniform(0.0, 0.01, size=len(s)).astype(np.float32)
        el = synth.EdgeList(np.arange(n, dtype=np.uint32), s, d, lat, loss, True)
    if parallel:
        el = synth.EdgeList(el.node_ids, np.append(el.src, np.uint32(0)), np.append(el.dst, np.uint32(1)),
                            np.append(el.latency_ns, np.uint64(2 * synth.MS)),
                            np.append(el.packet_loss, np.float32(0.001)), el.directed)
    return el


@functools.lru_cache(maxsize=None)
def _case(n, mode="rand", directed=False, parallel=False):
    """(edge list, used, oracle latency, oracle loss, the model's kept count), once per process."""
    el = _graph(n, mode, directed, 1000 + n, parallel)
    used = np.arange(n, dtype=np.uint32)
    code, lat, loss, _ = corc.routing(n, el.src, el.dst, el.latency_ns, el.packet_loss, el.directed, used)
    assert code == "OK"
    kept = int(model.fused_prune(model.dense_matrix(el)).sum())
    lat.setflags(write=False)
    loss.setflags(write=False)
    return el, used, lat, loss, kept


def _check(engine, el, used, lat, loss, kept):
    t = engine_graph_from_edges(el).compute_shortest_paths(used, engine, algo=AUTO)
    assert np.array_equal(t.lat, lat)
    assert np.array_equal(t.loss.view(np.uint32), loss.view(np.uint32))
    info = engine.last_info()
    assert info["algo_used"] == PRUNED
    assert int(info["arcs_kept"]) == kept


@pytest.mark.parametrize("n", [2, 3, 5, 63, 64, 65, 257, 777, 1001])
def test_vec_node_counts_dense_csr(engine, knob, n):
    """Row u of the dense CSR starts at word u (V - 1): V % 4 == 0 and != 0, row starts at every
    alignment mod 4, and in every row u the diagonal falls inside a 4-word chunk.  V < 5: rows
    shorter than a chunk; 777 and 1001: the SSSP's scalar head and tail (V % 4 == 1), 64: their
    vector forms."""
    knob("PRUNE_DENSE_BUILD", 0)
    _check(engine, *_case(n))


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("mode", ["rand", "const", "few", "ns"])
@pytest.mark.parametrize("n", [65, 257])
@pytest.mark.parametrize("dense_build", [0, 1])
def test_vec_latency_kinds(engine, knob, dense_build, n, mode, directed):
    """Both prune inputs, the dense CSR (stride V - 1) and dense_build's matrix (stride V, forced by
    the knob).  const: all arcs survive the first batch (S1 = V - 1; at 257 two rounds of NN
    lists); few: ties; directed: the gather form of the test (SYM = false)."""
    knob("PRUNE_DENSE_BUILD", dense_build)
    _check(engine, *_case(n, mode, directed))


@pytest.mark.parametrize("n", [65, 257])
def test_vec_parallel_arc_takes_dense_build(engine, n):
    """A complete graph with one parallel arc is no dense CSR: dense_build without the knob."""
    _check(engine, *_case(n, "rand", False, True))


def test_vec_const_many_survivors(engine, knob):
    """Constant latencies at V = 601: S1 = 600 > 512, so the survivors' losses past the first
    512 take the gather's second trip, and the NN lists take four rounds."""
    knob("PRUNE_DENSE_BUILD", 0)
    _check(engine, *_case(601, "const"))


def test_vec_used_subset_permuted(engine):
    """998 of C2's 1000 nodes in a permuted order: the emit goes through the used list, its scalar
    path (and 998 % 4 != 0)."""
    el, _, _, _, _, kept = fused_case("c2")
    used = np.random.default_rng(7).permutation(1000)[:998].astype(np.uint32)
    code, lat, loss, _ = corc.routing(1000, el.src, el.dst, el.latency_ns, el.packet_loss, False, used)
    assert code == "OK"
    _check(engine, el, used, lat, loss, int(kept.sum()))


def test_vec_row_range_offset_outputs(engine):
    """Rows [1, n - 1) of n = 66 through shd_routing_run into the table's rows from the second on:
    a row is 264 bytes, so out_loss is 8 mod 16 at the first row and the emit takes its fallback."""
    import torch

    from shadow_amd import _native as N
    n = 66
    el, used, lat, loss, kept = _case(n)
    g = engine_graph_from_edges(el)._cgraph()
    err = N.Error()
    N.check(engine.lib.shd_routing_prepare(engine.ctx, C.byref(g), N.ptr(used), n, N.ROUTE_SHORTEST, C.byref(err)),
            "prepare", err)
    dl = torch.zeros((n, n), dtype=torch.int64, device="cuda")
    dp = torch.zeros((n, n), dtype=torch.float32, device="cuda")
    assert dp[1:].data_ptr() % 16 == 8
    torch.cuda.synchronize()
    for _ in range(2):
        N.check(engine.lib.shd_routing_run(engine.ctx, AUTO, 1, n - 1, N.ptr(dl[1:]), N.ptr(dp[1:]), C.byref(err)),
                "shd_routing_run", err)
        info = engine.last_info()
        assert info["algo_used"] == PRUNED and int(info["arcs_kept"]) == kept
        hl, hp = dl.cpu().numpy().view(np.uint64), dp.cpu().numpy().view(np.uint32)
        assert np.array_equal(hl[1:n - 1], lat[1:n - 1])
        assert np.array_equal(hp[1:n - 1], loss.view(np.uint32)[1:n - 1])
        assert not hl[0].any() and not hl[n - 1].any() and not hp[0].any() and not hp[n - 1].any()


def test_vec_next_hops(engine):
    """Next hops on 64 nodes (identity used set, V % 4 == 0, aligned rows: the vector emit's case
    but for the next hops): the emit's fallback writes table and hops."""
    el, used, lat, loss, kept = _case(64)
    nh = corc.next_hops(64, el.src, el.dst, el.latency_ns, el.packet_loss, el.directed, used, lat, loss)
    t, gnh = engine_graph_from_edges(el).compute_next_hops(used, engine, algo=AUTO)
    assert np.array_equal(t.lat, lat)
    assert np.array_equal(t.loss.view(np.uint32), loss.view(np.uint32))
    assert np.array_equal(gnh, nh)
    info = engine.last_info()
    assert info["algo_used"] == PRUNED and int(info["arcs_kept"]) == kept
