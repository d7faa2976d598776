"""GPU tests of the second prune stage (prune_rows2: 3-hop detours over the lists prune_rows kept)
and of the 32-slot padded lists it hands the dense SSSP.  Every case compares the whole table,
latency and loss bits, with the C restatement (corc.routing)."""
import functools

import numpy as np
import pytest

from oracle import corc
from tests.graphs import engine_graph_from_edges

pytestmark = pytest.mark.gpu


def _complete(n, mode, seed):
    """synth.complete_graph with the latency rewrites of test_routing_gpu._complete."""
    from shadow_amd import synth
    el = synth.complete_graph(n, seed)
    rng = np.random.default_rng(seed)
    arcs = el.src != el.dst
    if mode == "const":      # every arc ties: stage 1 prunes nothing, stage 2 copies the rows through
        el.latency_ns[arcs] = np.uint64(5 * synth.MS)
    elif mode == "few":      # three latencies: heavy ties, long stage-1 lists
        el.latency_ns[arcs] = rng.integers(1, 4, size=int(arcs.sum())).astype(np.uint64) * np.uint64(synth.MS)
    elif mode == "wide":     # ns-granular latencies over four decades
        el.latency_ns[arcs] = rng.integers(1_000, 10_000_000, size=int(arcs.sum())).astype(np.uint64)
    return el


def _oracle(el):
    used = np.arange(el.n_nodes, dtype=np.uint32)
    code, lat, loss, _ = corc.routing(el.n_nodes, el.src, el.dst, el.latency_ns, el.packet_loss, el.directed, used)
    assert code == "OK"
    return used, lat, loss


@functools.lru_cache(maxsize=None)
def _complete_case(n, mode):
    el = _complete(n, mode, 11 + n)
    return (el, *_oracle(el))


def _assert_table(t, lat, loss):
    assert np.array_equal(t.lat, lat)
    assert np.array_equal(t.loss.view(np.uint32), loss.view(np.uint32))


@pytest.mark.parametrize("n,mode", [(2, "rand"), (5, "rand"), (33, "rand"), (65, "rand"), (63, "const"),
                                    (64, "few"), (130, "few"), (257, "wide")])
@pytest.mark.parametrize("dense_build", [0, 1])
@pytest.mark.parametrize("stage2", [None, 0])
@pytest.mark.parametrize("algo", [2, 0])
def test_stage2_complete_graphs(engine, knob, n, mode, dense_build, stage2, algo):
    """Complete graphs through both prune inputs (the dense CSR and dense_build), with stage 2 on
    (default) and off (SHD_PRUNE_STAGE2=0).  `const` and `few` tie heavily: stage 1 keeps whole
    rows, so stage 2's copy-through cap and its strict comparison decide the lists.  algo 2 runs
    the lists through the plain sweeps (exact list ends), AUTO (0) through the padded-list
    delta-stepping kernel (32-slot lists with stage 2, 64-slot without)."""
    knob("PRUNE_STAGE2", stage2)
    knob("PRUNE_DENSE_BUILD", dense_build)
    el, used, lat, loss = _complete_case(n, mode)
    t = engine_graph_from_edges(el).compute_shortest_paths(used, engine, algo=algo)
    _assert_table(t, lat, loss)
    assert engine.last_info()["algo_used"] == 2


@pytest.mark.parametrize("group", [4, 8, 16])
@pytest.mark.parametrize("stage2", [None, 0])
def test_stage2_forced_group_width(engine, knob, group, stage2):
    """Every forced lane-group width on both pad widths: G = 4 and 8 take the padded-list kernel
    (G x arcs-per-lane = 32 or 64 slots per step), wider groups the unpadded one."""
    knob("PRUNE_STAGE2", stage2)
    knob("SSSP_G", group)
    el, used, lat, loss = _complete_case(257, "wide")
    t = engine_graph_from_edges(el).compute_shortest_paths(used, engine, algo=0)
    _assert_table(t, lat, loss)
    assert engine.last_info()["algo_used"] == 2


def _dense_directed(n, seed, parallel):
    """Every ordered pair an arc with its own latency (lat(y, v) != lat(v, y)), plus self-loops;
    `parallel`: a second arc on a third of the pairs, some shorter than the first."""
    from shadow_amd import synth
    rng = np.random.default_rng(seed)
    s, d = np.nonzero(~np.eye(n, dtype=bool))
    lat = rng.integers(1, 301, size=len(s)).astype(np.uint64) * np.uint64(synth.MS)
    loss = rng.uniform(0.0, 0.01, size=len(s)).astype(np.float32)
    if parallel:
        pick = rng.random(len(s)) < 1 / 3
        s, d = np.concatenate([s, s[pick]]), np.concatenate([d, d[pick]])
        lat = np.concatenate([lat, rng.integers(1, 301, size=int(pick.sum())).astype(np.uint64) * np.uint64(synth.MS)])
        loss = np.concatenate([loss, rng.uniform(0.0, 0.01, size=int(pick.sum())).astype(np.float32)])
    loops = np.arange(n)
    s, d = np.concatenate([loops, s]).astype(np.uint32), np.concatenate([loops, d]).astype(np.uint32)
    lat = np.concatenate([rng.integers(1, 51, size=n).astype(np.uint64) * np.uint64(synth.MS), lat])
    loss = np.concatenate([rng.uniform(0.0, 0.01, size=n).astype(np.float32), loss])
    return synth.EdgeList(np.arange(n, dtype=np.uint32), s, d, lat, loss, True)


@functools.lru_cache(maxsize=None)
def _directed_case(n, parallel):
    el = _dense_directed(n, 100 + n, parallel)
    return (el, *_oracle(el))


@pytest.mark.parametrize("n", [40, 97])
@pytest.mark.parametrize("parallel,dense_build", [(False, 0), (False, 1), (True, 1)])
@pytest.mark.parametrize("algo", [2, 0])
def test_stage2_dense_directed_asymmetric(engine, knob, n, parallel, dense_build, algo):
    """Dense directed graphs with asymmetric latencies: the last arc of a stage-2 detour is
    y -> v, never v -> y (kept(v) only names the candidates y).  With parallel arcs the graph goes
    through dense_build, which folds them."""
    knob("PRUNE_DENSE_BUILD", dense_build)
    el, used, lat, loss = _directed_case(n, parallel)
    t = engine_graph_from_edges(el).compute_shortest_paths(used, engine, algo=algo)
    _assert_table(t, lat, loss)
    assert engine.last_info()["algo_used"] == 2


@pytest.mark.parametrize("lo,hi", [(1_400_000_000, 1_430_000_000), (1_440_000_000, 1_500_000_000)])
@pytest.mark.parametrize("algo", [2, 0])
def test_stage2_three_term_sum_near_u32(engine, lo, hi, algo):
    """n = 33, complete, arc latencies in [lo, hi] ns: every two-arc sum fits u32 and every direct
    arc is tight.  In the first range a three-arc sum lands just below 2^32 - 1 (the +inf mark);
    in the second it passes 2^32 and, taken in 32 bits, would wrap to a few hundred ms -- a
    "shorter" detour that drops a tight arc."""
    from shadow_amd import synth
    el = synth.complete_graph(33, 3)
    rng = np.random.default_rng(3)
    arcs = el.src != el.dst
    el.latency_ns[arcs] = rng.integers(lo, hi + 1, size=int(arcs.sum())).astype(np.uint64)
    assert 2 * hi < 2**32 - 1
    used, lat, loss = _oracle(el)
    t = engine_graph_from_edges(el).compute_shortest_paths(used, engine, algo=algo)
    _assert_table(t, lat, loss)


def test_stage2_kept_counts(engine, knob):
    """n = 257 `rand` (seed 1): stage 2 keeps fewer arcs than stage 1 alone (a CPU model of both
    stages: ~21.3 and ~11.4 arcs per node), never fewer than the tight arcs (lat(u, v) equal to
    the arc's latency, from the oracle table), and the same number on every build."""
    from shadow_amd import synth
    n = 257
    el = synth.complete_graph(n, 1)
    used, lat, loss = _oracle(el)
    W = np.full((n, n), np.iinfo(np.uint64).max, np.uint64)
    arcs = el.src != el.dst
    W[el.src[arcs], el.dst[arcs]] = el.latency_ns[arcs]
    W[el.dst[arcs], el.src[arcs]] = el.latency_ns[arcs]
    tight = int(((lat == W) & ~np.eye(n, dtype=bool)).sum())
    g = engine_graph_from_edges(el)

    def kept():
        t = g.compute_shortest_paths(used, engine, algo=2)
        _assert_table(t, lat, loss)
        return int(engine.last_info()["arcs_kept"])

    with2 = [kept() for _ in range(3)]
    knob("PRUNE_STAGE2", 0)
    stage1 = kept()
    print(f"arcs kept: stage 1 {stage1} ({stage1 / n:.1f} per node), stage 2 {with2[0]} "
          f"({with2[0] / n:.1f} per node), tight {tight} ({tight / n:.1f} per node)")
    assert with2[0] == with2[1] == with2[2]
    assert with2[0] < stage1
    assert with2[0] >= tight


def test_stage2_kept_set_is_run_independent_on_c2(engine):
    """C2 (1000 nodes): stage 1 fills a list in the order its atomics arrive, and some lists hold
    more than 64 arcs, the block stage 2 reads.  The final count and tables are the same on every
    build all the same: stage 2's cut-offs depend on list lengths only."""
    from shadow_amd import synth
    el = synth.complete_graph(1000, 1)
    used = np.arange(1000, dtype=np.uint32)
    g = engine_graph_from_edges(el)
    runs = []
    for _ in range(4):
        t = g.compute_shortest_paths(used, engine, algo=0)
        runs.append((int(engine.last_info()["arcs_kept"]), t.lat.copy(), t.loss.view(np.uint32).copy()))
    print("C2 arcs kept:", [r[0] for r in runs])
    assert len({r[0] for r in runs}) == 1
    for r in runs[1:]:
        assert np.array_equal(r[1], runs[0][1]) and np.array_equal(r[2], runs[0][2])
