"""The routing build at the u32 latency seam and past the delta-stepping bucket range, bit for bit
against the C restatement (tests/seam_graphs.py has the graphs, tests/test_seam_graphs.py proves
their properties on the CPU).

The narrow engines hand a build to the u64 engine when a path latency reaches 2^32 - 1, by five
rules of their own: the per-arc test of relax_node / expand_flat (cl >= lu && cl != 2^32 - 1), the
per-node guard of the padded-list kernels (lat_guard = 2^32 - 2 - max arc), launch_group's switch
to the unpadded kernel on padded lists when the largest arc is 2^32 - 2, the prune's u32 detour
sums, and the blocked engine's saturating adds.  Each is run here with table entries, arc sums and
labels of unused nodes at 2^32 - 2, 2^32 - 1, 2^32 and 2^32 + 1."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import corc
from tests import seam_graphs as SG

pytestmark = pytest.mark.gpu
ALGOS = [0, 1, 2, 3, 4]


def _graph(gr):
    from shadow_amd.routing import NetworkGraph
    return NetworkGraph(*gr)


def _want(gr, used):
    code, lat, loss, _ = corc.routing(len(gr[0]), gr[1], gr[2], gr[3], gr[4], gr[5], used)
    assert code == "OK"
    return lat, loss.view(np.uint32)


def _diff(t, lat, bits):
    """'' when the table is the oracle's, else where it first differs."""
    for name, got, want in (("lat", t.lat, lat), ("loss bits", t.loss.view(np.uint32), bits)):
        if not np.array_equal(got, want):
            i, j = np.argwhere(got != want)[0]
            return f"{name}[{i},{j}] = {int(got[i, j])}, want {int(want[i, j])} ({int((got != want).sum())} differ)"
    return ""


# ---------------------------------------------------------------------------------------------
# a. the ladder on every engine

@functools.lru_cache(maxsize=None)
def _ladder_case(top, directed, embed):
    gr = SG.ladder(top, directed, 5 if embed else None)
    n = len(gr[0])
    used = np.random.default_rng(top % 97 + 2 * directed + embed).permutation(n).astype(np.uint32)
    lat, bits = _want(gr, used)
    return gr, used, lat, bits


LADDERS = [pytest.param(top, directed, embed, id=f"top{top - 2**32:+d}-{'dir' if directed else 'und'}-"
                        f"{'embedded' if embed else 'bare'}")
           for top in SG.TOPS for directed in (False, True) for embed in (False, True)]


def _check_ladder(engine, top, directed, embed, algo, why):
    gr, used, lat, bits = _ladder_case(top, directed, embed)
    t = _graph(gr).compute_shortest_paths(used, engine, algo=algo)
    bad = _diff(t, lat, bits)
    assert not bad, f"{why}: {bad}"
    offd = lat[used[:, None] != used[None, :]]
    assert int(offd.max()) == top
    if top >= SG.SEAM:   # an entry the narrow labels cannot hold: the u64 engine must have run
        assert engine.last_info()["wide_latency"] == 1, why
    return engine.last_info()


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("top,directed,embed", LADDERS)
def test_ladder_lds_and_blocked_engines(engine, top, directed, embed, algo):
    """relax_node's per-arc rule (algos 0, 1, 3 on the sparse ladder; the hub path and the lane
    groups together on the embedded one), the prune's sums and the padded lists (algo 2), the
    blocked engine's saturating adds and check_unreach (algo 4).
    What these cases can show: the top node has arcs out, so a sum above 2^32 - 2 is formed at
    every ``top`` and every narrow engine flags the build (on the embedded ladder, which counts as
    dense, AUTO's padded kernels do at node 2's label of 2^32 - 4 already): the tables are the
    u64 engine's, and the cases prove the hand-over, at each ``top`` and from each engine, not
    the narrow kernels' own seam entries.  Those are test_sink_ladder_row0,
    test_guard_ladder_padded_kernels and test_trap_complete_prune_paths."""
    info = _check_ladder(engine, top, directed, embed, algo, f"algo {algo}")
    if algo == 4:
        assert info["algo_used"] == 4


@pytest.mark.parametrize("reorder", [0, 1])
@pytest.mark.parametrize("algo", [1, 3])
@pytest.mark.parametrize("top,directed,embed", LADDERS)
def test_ladder_global_label_kernel(engine, knob, top, directed, embed, algo, reorder):
    """expand_flat / expand_flat8's per-arc rule (SSSP_GLOBAL=1), on the plain and the
    locality-ordered arcs."""
    knob("SSSP_GLOBAL", 1)
    knob("SSSP_REORDER", reorder)
    info = _check_ladder(engine, top, directed, embed, algo, f"global algo {algo} reorder {reorder}")
    assert info["algo_used"] == algo


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("top,directed,embed", LADDERS)
def test_ladder_blocked_tiles(engine, knob, top, directed, embed, tile):
    knob("FW_TILE", tile)
    info = _check_ladder(engine, top, directed, embed, 4, f"blocked tile {tile}")
    assert info["algo_used"] == 4


@pytest.mark.parametrize("glob", [0, 1])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("top", SG.TOPS)
def test_sink_ladder_row0(engine, knob, top, algo, glob):
    """The ladder whose top node has no arc out, row 0: no sum but the one that makes the top
    node's label reaches 2^32 - 1, so at top = 2^32 - 2 the narrow kernel writes the seam entry
    itself, at 2^32 - 1 only `cl != kLat32Inf` (check_unreach for the blocked engine) and from
    2^32 on only `cl >= lu` (the saturating add) hands the build to the u64 engine."""
    gr = SG.sink_ladder(top)
    used = np.arange(8, dtype=np.uint32)
    code, lat, loss, _ = corc.routing(8, gr[1], gr[2], gr[3], gr[4], True, used, rows=(0, 1))
    assert code == "OK" and int(lat[0, 1:].max()) == top
    knob("SSSP_GLOBAL", glob)
    t = _graph(gr).compute_shortest_paths(used, engine, algo=algo, rows=(0, 1))
    assert not _diff(t, lat, loss.view(np.uint32))
    wide = engine.last_info()["wide_latency"]
    if top >= SG.SEAM:
        assert wide == 1
    elif algo in (1, 2):
        # SSSP runs the unpadded kernel on the plain arcs, PRUNED the same kernel on its pruned lists
        # (it runs without delta, so launch_group sets no guard): both decide per arc and stay narrow.
        # AUTO and DELTA also prune these 8 nodes (they count as dense) but run with delta, so the
        # padded kernels' guard, 2^31 - 2 here, trips at node 1's label of 2^31: wide, as allowed.
        # The blocked engine may hand the other rows' unreachable pairs to the u64 engine.
        assert wide == 0


@pytest.mark.parametrize("top", SG.TOPS)
def test_ladder_next_hops(engine, top):
    gr = SG.ladder(top, False, 5)
    used = np.arange(len(gr[0]), dtype=np.uint32)     # (next hops need every node used)
    lat, bits = _want(gr, used)
    t, nh = _graph(gr).compute_next_hops(used, engine)
    assert not _diff(t, lat, bits)
    ref = corc.next_hops(len(gr[0]), gr[1], gr[2], gr[3], gr[4], gr[5], used, lat, bits.view(np.float32))
    assert np.array_equal(nh, ref)
    if top >= SG.SEAM:
        assert engine.last_info()["wide_latency"] == 1


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("embed", [False, True])
@pytest.mark.parametrize("top", SG.TOPS)
def test_ladder_used_subset_without_the_interior(engine, top, embed, algo):
    """Nodes 0 and 1 of the ladder (and a third of the embedding graph) used: every entry is far
    below the seam while the labels of the unused ladder nodes run up to ``top``, through and past
    2^32 - 1.  The build may go to the u64 engine for them; its table is the oracle's either way."""
    gr = SG.ladder(top, False, 5 if embed else None)
    used = [1, 0] if not embed else [120, 0] + list(np.random.default_rng(8).permutation(np.arange(1, 120))[:40])
    used = np.asarray(used, np.uint32)
    lat, bits = _want(gr, used)
    assert int(lat.max()) <= 2**31
    t = _graph(gr).compute_shortest_paths(used, engine, algo=algo)
    assert not _diff(t, lat, bits)


# ---------------------------------------------------------------------------------------------
# b. complete graphs whose arc sums wrap u32, through every prune path

# each prune / SSSP shape once (shd knobs; None: the default)
PRUNE_SHAPES = [
    {},
    {"PRUNE_SHAPE": 0, "PRUNE_DENSE_BUILD": 0},
    {"PRUNE_SHAPE": 0, "PRUNE_DENSE_BUILD": 1},
    {"PRUNE_DENSE_BUILD": 1},
    {"PRUNE_STAGE2": 0},
    {"PRUNE_STAGE2": 0, "PRUNE_DENSE_BUILD": 1},
    {"PRUNE_SHAPE": 0, "PRUNE_STAGE2": 0},
    {"PRUNE_FUSED": 0},
    {"PRUNE_FUSED": 0, "PRUNE_DENSE_BUILD": 1},
    {"SSSP_SHADOW": 0},
    {"SSSP_G": 4},
    {"SSSP_G": 8},
    {"SSSP_G": 4, "SSSP_SHADOW": 0},
    {"SSSP_G": 8, "PRUNE_STAGE2": 0},
    {"SSSP_G": 4, "PRUNE_STAGE2": 0, "SSSP_SHADOW": 0},
]
ALL_KNOBS = sorted({k for s in PRUNE_SHAPES for k in s})


def _three_builds(engine, knob, gr, lat, bits, shapes, algos=(0, 2), rows=None):
    """Prepare once per shape and run three builds per algo (the second and third know the pruned
    arc count: the padded-list kernel AUTO then picks); every table against the oracle's.
    Returns the mismatches and, per (shape number, algo), the wide_latency values of its builds."""
    import torch

    from shadow_amd import _native as N
    n = len(gr[0])
    used = np.arange(n, dtype=np.uint32)
    g = _graph(gr)
    cg = g._cgraph()
    rb, re = rows or (0, n)
    dl = torch.empty((re - rb, n), dtype=torch.int64, device="cuda")
    dp = torch.empty((re - rb, n), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    bad, wide = [], {}
    for k_shape, shape in enumerate(shapes):
        for k in ALL_KNOBS:
            knob(k, shape.get(k))
        err = N.Error()
        N.check(engine.lib.shd_routing_prepare(engine.ctx, C.byref(cg), N.ptr(used), n, N.ROUTE_SHORTEST,
                                               C.byref(err)), "prepare", err)
        for algo in algos:
            for run in range(3):
                N.check(engine.lib.shd_routing_run(engine.ctx, algo, rb, re, N.ptr(dl), N.ptr(dp), C.byref(err)),
                        "shd_routing_run", err)
                info = engine.last_info()
                if info["algo_used"] != 2:
                    bad.append(f"{shape} algo {algo} run {run}: algo_used {info['algo_used']}")
                wide.setdefault((k_shape, algo), set()).add(info["wide_latency"])
                got_l, got_p = dl.cpu().numpy().view(np.uint64), dp.cpu().numpy().view(np.uint32)
                for name, got, want in (("lat", got_l, lat), ("loss bits", got_p, bits)):
                    if not np.array_equal(got, want):
                        i, j = np.argwhere(got != want)[0]
                        bad.append(f"{shape} algo {algo} run {run}: {name}[{i},{j}] = {int(got[i, j])}, want "
                                   f"{int(want[i, j])} ({int((got != want).sum())} differ)")
    return bad, wide


@pytest.mark.parametrize("max_arc", [2**32 - 2, 2**32 - 3], ids=["guard_off", "guard_1"])
@pytest.mark.parametrize("n", [33, 65, 130, 257])
def test_huge_complete_prune_paths(engine, knob, n, max_arc):
    """Arcs in [2^31, max_arc]: every two-arc sum wraps u32 to less than any arc, so a prune site
    that trusts a wrapped sum drops arcs the table needs.  Largest arc 2^32 - 2: launch_group
    switches the guard off and runs the unpadded kernel on the padded lists; 2^32 - 3: the guard
    is 1 and every expansion but the source's hands the build to the u64 engine."""
    gr = SG.huge_complete(n, max_arc, n)
    lat, bits = _want(gr, np.arange(n, dtype=np.uint32))
    bad, _ = _three_builds(engine, knob, gr, lat, bits, PRUNE_SHAPES)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("top", SG.TOPS)
def test_guard_ladder_padded_kernels(engine, knob, top):
    """A dense graph whose largest arc is the last of the path that reaches ``top``, into a sink:
    the label that arc leaves from is lat_guard + (top - (2^32 - 2)), and no other node with arcs
    out has a label above the guard (tests/test_seam_graphs.py), so that one compare is all that
    stands between the unchecked add and the sentinel's value (2^32 - 1) or a label wrapped to 0
    or 1 (2^32, 2^32 + 1).  Rows 0..40 (the sink starts none).
    sssp_lds_shadow on 32-slot lists with 4 arcs per lane (expand_queue_nr, the default and C2's
    kernel) compares only nodes whose list is not empty, so on it the guard is pinned from both
    sides: the build stays narrow at 2^32 - 2 (the kernel writes that entry itself) and is wide
    at 2^32 - 1 -- a guard one too loose or one too tight fails one of the two.  Its 8-arcs-per-
    lane form (relax_node_pad_nr: SSSP_G=4, or 64-slot lists) and the returning kernel
    (SSSP_SHADOW=0) compare every expanded node, the sink too, so they are wide at every ``top``.  PRUNED (algo 2) runs without delta, hence without guard, on the unpadded
    kernel's per-arc rule, in chaotic order: it adds the largest arc to labels of node 40 that
    are not final yet, and such a sum may leave u32 at 2^32 - 2 too (its table is exact either
    way).  AUTO's buckets are as wide as the smallest arc (1 ms; the mean arc / 256 is less), so a
    node's label is final when it is expanded and only final labels meet the guard."""
    gr = SG.guard_ladder(top, 9)
    n = len(gr[0])
    code, lat, loss, _ = corc.routing(n, gr[1], gr[2], gr[3], gr[4], True, np.arange(n, dtype=np.uint32), rows=(0, 41))
    assert code == "OK" and int(lat[:, 41].max()) == top
    shapes = [{}, {"SSSP_G": 4}, {"PRUNE_STAGE2": 0}, {"SSSP_SHADOW": 0}, {"SSSP_G": 4, "SSSP_SHADOW": 0},
              {"PRUNE_STAGE2": 0, "SSSP_SHADOW": 0}]
    bad, wide = _three_builds(engine, knob, gr, lat, loss.view(np.uint32), shapes, rows=(0, 41))
    assert not bad, "\n".join(bad)
    for (k_shape, algo), w in wide.items():
        if top >= SG.SEAM:
            assert w == {1}, (shapes[k_shape], algo)
        elif algo == 0 and not shapes[k_shape]:
            assert w == {0}, (shapes[k_shape], algo)


@pytest.mark.parametrize("n", [40, 65, 130])
def test_trap_complete_prune_paths(engine, knob, n):
    """Detours whose u32 sum wraps to 0 against arcs the table needs, on a graph where no sum over
    a kept arc leaves u32 (tests/test_seam_graphs.py): the build stays narrow, so the table is the
    pruned lists' own -- the complete graphs above are repaired by the wide rerun whatever the
    prune drops."""
    gr = SG.trap_complete(n, n)
    lat, bits = _want(gr, np.arange(n, dtype=np.uint32))
    bad, wide = _three_builds(engine, knob, gr, lat, bits, PRUNE_SHAPES)
    assert not bad, "\n".join(bad)
    assert set().union(*wide.values()) == {0}


@pytest.mark.parametrize("n", [33, 65, 130, 257])
def test_mixed_complete_prune_paths(engine, knob, n):
    """Arcs of 1..8 ns and of 2^32 - 2 - k: detours that sum to 2^32 - 1 exactly, that wrap to a
    single digit, and that fit by a few ns."""
    gr = SG.mixed_complete(n, SG.mixed_small_share(n), n)
    lat, bits = _want(gr, np.arange(n, dtype=np.uint32))
    bad, _ = _three_builds(engine, knob, gr, lat, bits, PRUNE_SHAPES)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("algo", [1, 3, 4])
@pytest.mark.parametrize("n", [33, 65, 130, 257])
def test_mixed_complete_other_engines(engine, knob, n, algo):
    gr = SG.mixed_complete(n, SG.mixed_small_share(n), n)
    used = np.arange(n, dtype=np.uint32)
    lat, bits = _want(gr, used)
    for glob in ((0, 1) if algo != 4 else (0,)):
        knob("SSSP_GLOBAL", glob)
        t = _graph(gr).compute_shortest_paths(used, engine, algo=algo)
        bad = _diff(t, lat, bits)
        assert not bad, f"global {glob}: {bad}"
        assert engine.last_info()["algo_used"] == algo


# ---------------------------------------------------------------------------------------------
# c. past the bucket range

@functools.lru_cache(maxsize=None)
def _long_case(name):
    make, delta = SG.LONG_CASES[name]
    gr = make()
    n = len(gr[0])
    used = np.random.default_rng(n).permutation(n).astype(np.uint32)
    lat, bits = _want(gr, used)
    return gr, used, lat, bits, delta


@pytest.mark.parametrize("slots", [2, 1])
@pytest.mark.parametrize("reorder", [0, 1])
@pytest.mark.parametrize("name", list(SG.LONG_CASES))
def test_long_graphs_global_label_kernel(engine, knob, name, reorder, slots):
    """The global-label kernel's bucket byte min(255, lat / delta): from every source of these
    graphs most labels lie past bucket 255 (tests/test_seam_graphs.py), so the row converges in
    the shared last bucket, over hundreds of sweeps."""
    gr, used, lat, bits, delta = _long_case(name)
    knob("SSSP_GLOBAL", 1)
    knob("SSSP_DELTA", delta)
    knob("SSSP_REORDER", reorder)
    knob("SSSP_SLOTS", slots)
    t = _graph(gr).compute_shortest_paths(used, engine, algo=3)
    assert engine.last_info()["algo_used"] == 3
    assert not _diff(t, lat, bits)


@pytest.mark.parametrize("algo,no_spread", [(0, 0), (0, 1), (1, 0), (1, 1), (3, 0), (3, 1), (4, 0)])
@pytest.mark.parametrize("name", ["long_path", "ring", "grid", "broom"])
def test_long_graphs_lds_and_blocked_engines(engine, knob, name, algo, no_spread):
    """The LDS kernels' three rotating sweep accumulators over hundreds of sweeps (the broom's
    star centre relaxed by whole waves in the same sweeps as the path's lane groups), on the
    wave-spread lists and the plain ones, and the blocked engine, on the same graphs."""
    gr, used, lat, bits, _ = _long_case(name)
    knob("SSSP_NO_SPREAD", no_spread)
    t = _graph(gr).compute_shortest_paths(used, engine, algo=algo)
    assert not _diff(t, lat, bits)
    assert engine.last_info()["wide_latency"] == 0


@pytest.mark.parametrize("reorder", [0, 1])
def test_every_label_in_the_last_bucket(engine, knob, reorder):
    """1 us buckets under 1 to 6 ms edges: every label but the source's shares bucket byte 255, so
    the whole row is the chaotic fallback inside the last bucket."""
    from tests.test_routing_gpu import _tie_heavy_ba
    n = 3000
    ids, s, d, l, p, directed = _tie_heavy_ba(n, 3, 91, False)
    used = np.random.default_rng(12).permutation(n).astype(np.uint32)
    code, lat, loss, _ = corc.routing(n, s, d, l, p, directed, used)
    assert code == "OK"
    assert int(lat[used[:, None] != used[None, :]].min()) // 1000 > 255
    knob("SSSP_GLOBAL", 1)
    knob("SSSP_DELTA", 1000)
    knob("SSSP_REORDER", reorder)
    t = _graph((ids, s, d, l, p, directed)).compute_shortest_paths(used, engine, algo=3)
    assert engine.last_info()["algo_used"] == 3
    assert not _diff(t, lat, loss.view(np.uint32))
