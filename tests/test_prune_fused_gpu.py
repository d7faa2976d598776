"""GPU tests of the fused dense prune (nearest_rows + prune_fused, the default when
the default shape and stage 2 are on).  Every case compares the whole table, latency and loss bits,
with the C restatement (corc.routing), and `arcs_kept` with the numpy model's count
(tests/prune_fused_model.py): the kept set is a function of the graph alone."""
import numpy as np
import pytest

from tests import prune_fused_model as model
from tests.graphs import engine_graph_from_edges
from tests.prune_fused_cases import case

pytestmark = pytest.mark.gpu


def _assert_table(t, lat, loss):
    assert np.array_equal(t.lat, lat)
    assert np.array_equal(t.loss.view(np.uint32), loss.view(np.uint32))


def _build(engine, g, name, algo):
    el, used, lat, loss, W, kept = case(name)
    t = g.compute_shortest_paths(used, engine, algo=algo)
    _assert_table(t, lat, loss)
    info = engine.last_info()
    assert info["algo_used"] == 2
    return int(info["arcs_kept"])


@pytest.mark.parametrize("name", ["complete2", "complete5", "complete33", "complete65", "const63", "few130",
                                  "const200", "big33"])
@pytest.mark.parametrize("dense_build", [0, 1])
@pytest.mark.parametrize("algo", [2, 0])
def test_fused_complete_graphs(engine, knob, name, dense_build, algo):
    """Complete graphs through both prune inputs (the dense CSR and dense_build) and both SSSP
    kernels (algo 2: plain sweeps over exact list ends; AUTO: the padded-list kernel).  n = 2, 5:
    nearest lists shorter than a table.  const63, few130: nothing or little prunes, ties under the
    strict compare, final lists far longer than 32 slots.  const200: |S1| = 199, two rounds of the
    undirected form's 192 lists.  big33: latencies in [1.44e9, 1.5e9] ns, a three-term sum passes 2^32."""
    knob("PRUNE_DENSE_BUILD", dense_build)
    kept = case(name)[5]
    n = _build(engine, engine_graph_from_edges(case(name)[0]), name, algo)
    assert n == int(kept.sum())


@pytest.mark.parametrize("name,dense_build", [("directed40", 0), ("directed40", 1), ("directed40p", 1),
                                              ("directed97", 0), ("directed97", 1), ("directed97p", 1),
                                              ("directed_const140", 0), ("directed_const140", 1)])
@pytest.mark.parametrize("algo", [2, 0])
def test_fused_dense_directed_asymmetric(engine, knob, name, dense_build, algo):
    """Dense directed graphs with asymmetric latencies: the last arc of a detour is y -> v from the
    matrix, never v -> y from NN[v].  With parallel arcs (`p`) the graph goes through dense_build,
    which folds them.  directed_const140: |S1| = 139, two rounds of the directed form's 128 lists."""
    knob("PRUNE_DENSE_BUILD", dense_build)
    kept = case(name)[5]
    n = _build(engine, engine_graph_from_edges(case(name)[0]), name, algo)
    assert n == int(kept.sum())


@pytest.mark.parametrize("dense_build", [0, 1])
def test_fused_kept_counts_n257(engine, knob, dense_build):
    """complete_graph(257, 1): the count is the model's (2,909), the same on three builds, below
    stage 1 alone (SHD_PRUNE_STAGE2=0) and at least the tight arcs."""
    knob("PRUNE_DENSE_BUILD", dense_build)
    el, used, lat, loss, W, kept = case("rand257")
    tight = int(model.tight_arcs(W, lat).sum())
    g = engine_graph_from_edges(el)
    fused = [_build(engine, g, "rand257", algo) for algo in (2, 0, 2)]
    knob("PRUNE_STAGE2", 0)
    stage1 = _build(engine, g, "rand257", 2)
    print(f"n = 257 arcs kept: fused {fused}, stage 1 alone {stage1}, tight {tight}")
    assert fused == [2909] * 3 == [int(kept.sum())] * 3
    assert tight <= fused[0] < stage1


def test_fused_c2_four_builds(engine):
    """C2 (complete_graph(1000, 1)): S1 fills in the order its atomics arrive (up to 151 arcs a
    row); the count is the model's on every build and the tables are the oracle's."""
    el, used, lat, loss, W, kept = case("c2")
    g = engine_graph_from_edges(el)
    counts = [_build(engine, g, "c2", 0) for _ in range(4)]
    print("C2 arcs kept:", counts)
    assert counts == [20857] * 4 == [int(kept.sum())] * 4


def test_fused_off_is_the_two_stage_prune_on_c2(engine, knob):
    """SHD_PRUNE_FUSED=0 on C2: prune_rows + prune_rows2 and their 21,273 arcs; the count follows
    the prune path when it changes between two builds of one prepared graph, both ways."""
    el = case("c2")[0]
    g = engine_graph_from_edges(el)
    knob("PRUNE_FUSED", 0)
    assert _build(engine, g, "c2", 0) == 21273
    knob("PRUNE_FUSED", 1)
    assert _build(engine, g, "c2", 0) == 20857
    knob("PRUNE_FUSED", 0)
    assert _build(engine, g, "c2", 0) == 21273
