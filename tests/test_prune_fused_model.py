"""CPU tests of the fused prune's numpy model (tests/prune_fused_model.py): it never drops a tight
arc -- an arc whose latency is the oracle table's entry for its ends -- and its kept counts are the
recorded ones, which the GPU tests compare the kernels' `arcs_kept` with."""
import numpy as np
import pytest

from tests import prune_fused_model as model
from tests.prune_fused_cases import CASES, SMALL, case


@pytest.mark.parametrize("name", SMALL + ["c2"])
def test_model_keeps_every_tight_arc(name):
    el, used, lat, loss, W, kept = case(name)
    tight = model.tight_arcs(W, lat)
    n_kept, n_tight = int(kept.sum()), int(tight.sum())
    print(f"{name}: {int((W != model.INF).sum())} arcs, {n_tight} tight, {n_kept} kept, "
          f"longest list {int(kept.sum(1).max())}")
    assert not (kept & (W == model.INF)).any()
    assert kept[tight].all()
    assert n_kept == CASES[name][1]


def test_model_c2_counts():
    """C2 (complete_graph(1000, 1)): 16,518 tight arcs; the first batch leaves 118,824 arcs (151 in
    the longest S1), the 3-hop test 20,857, one list longer than 32 slots."""
    el, used, lat, loss, W, kept = case("c2")
    nodes, lats = model.nearest_table(W)
    s1 = model.first_batch(W, nodes, lats)
    assert int(model.tight_arcs(W, lat).sum()) == 16518
    assert (int(s1.sum()), int(s1.sum(1).max())) == (118824, 151)
    assert int(kept.sum()) == 20857
    assert int((kept.sum(1) > 32).sum()) == 1


def test_model_nearest_table_order():
    """NN[x]: ascending (latency, index), unused entries at the end, never x itself."""
    el, used, lat, loss, W, kept = case("few130")
    nodes, lats = model.nearest_table(W)
    for x in range(W.shape[0]):
        keys = [(int(l), int(v)) for v, l in zip(nodes[x], lats[x]) if v >= 0]
        assert keys == sorted(keys) and len(keys) == 32 and x not in nodes[x]
        assert keys[-1] <= min((int(W[x, v]), v) for v in range(W.shape[0]) if v not in nodes[x] and v != x)
    el, used, lat, loss, W, kept = case("complete5")
    nodes, lats = model.nearest_table(W)
    assert ((nodes >= 0).sum(1) == 4).all() and (lats[nodes < 0] == model.INF).all()
