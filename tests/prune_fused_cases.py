"""The graphs of the fused-prune tests (test_prune_fused_model.py on the CPU, test_prune_fused_gpu.py
on the GPU), each with its oracle table and the model's kept set, computed once per process."""
import functools

import numpy as np

from oracle import corc
from tests import prune_fused_model as model


def _complete(n, mode, seed):
    """synth.complete_graph with its latencies rewritten: `const` every arc ties; `few` three
    values; `big` latencies in [1.44e9, 1.5e9] ns (a three-term sum passes 2^32)."""
    from shadow_amd import synth
    el = synth.complete_graph(n, seed)
    rng = np.random.default_rng(seed)
    arcs = el.src != el.dst
    m = int(arcs.sum())
    if mode == "const":
        el.latency_ns[arcs] = np.uint64(5 * synth.MS)
    elif mode == "few":
        el.latency_ns[arcs] = rng.integers(1, 4, size=m).astype(np.uint64) * np.uint64(synth.MS)
    elif mode == "big":
        el.latency_ns[arcs] = rng.integers(1_440_000_000, 1_500_000_001, size=m).astype(np.uint64)
    else:
        assert mode == "rand"
    return el


def _dense_directed(n, seed, parallel, const=False):
    """Every ordered pair an arc with its own latency (lat(y, v) != lat(v, y)), plus self-loops;
    `parallel`: a second arc on a third of the pairs, some shorter than the first; `const`: one
    latency on every arc instead."""
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
    if const:
        lat[:] = np.uint64(5 * synth.MS)
    loops = np.arange(n)
    s, d = np.concatenate([loops, s]).astype(np.uint32), np.concatenate([loops, d]).astype(np.uint32)
    lat = np.concatenate([rng.integers(1, 51, size=n).astype(np.uint64) * np.uint64(synth.MS), lat])
    loss = np.concatenate([rng.uniform(0.0, 0.01, size=n).astype(np.float32), loss])
    return synth.EdgeList(np.arange(n, dtype=np.uint32), s, d, lat, loss, True)


# name -> (builder, the model's kept count with 8 first-batch detours and 32-entry tables)
CASES = {
    "complete2": (lambda: _complete(2, "rand", 13), 2),
    "complete5": (lambda: _complete(5, "rand", 16), 10),
    "complete33": (lambda: _complete(33, "rand", 44), 184),
    "complete65": (lambda: _complete(65, "rand", 76), 417),
    "const63": (lambda: _complete(63, "const", 74), 63 * 62),
    "few130": (lambda: _complete(130, "few", 141), 11212),
    "const200": (lambda: _complete(200, "const", 211), 200 * 199),
    "rand257": (lambda: _complete(257, "rand", 1), 2909),
    "directed40": (lambda: _dense_directed(40, 140, False), 228),
    "directed40p": (lambda: _dense_directed(40, 140, True), 232),
    "directed97": (lambda: _dense_directed(97, 197, False), 973),
    "directed97p": (lambda: _dense_directed(97, 197, True), 972),
    "directed_const140": (lambda: _dense_directed(140, 240, False, const=True), 140 * 139),
    "big33": (lambda: _complete(33, "big", 3), 33 * 32),
    "c2": (lambda: _complete(1000, "rand", 1), 20857),
}
SMALL = [k for k in CASES if k != "c2"]


@functools.lru_cache(maxsize=None)
def case(name):
    """(edge list, used nodes, oracle latency table, oracle loss table, W, the model's kept set)."""
    el = CASES[name][0]()
    used = np.arange(el.n_nodes, dtype=np.uint32)
    code, lat, loss, _ = corc.routing(el.n_nodes, el.src, el.dst, el.latency_ns, el.packet_loss, el.directed, used)
    assert code == "OK"
    W = model.dense_matrix(el)
    kept = model.fused_prune(W)
    for a in (lat, loss, W, kept):
        a.setflags(write=False)
    return el, used, lat, loss, W, kept
