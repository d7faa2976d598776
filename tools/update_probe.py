"""What shd_routing_update_edges and shd_relay_retable buy: host-clock medians (20 repetitions after
3 warm-up ones) on the C2 graph (1k-node complete) and the C3 graph (10k-node BA m=3), for updates
of n = 1, 1,000 and every edge, of
  * the update call alone (the first call after a prepare, which builds the edge -> arc map, apart),
  * update + shd_routing_run,
  * what there was before: shd_routing_prepare of the modified graph + shd_routing_run,
and, on C5's 100k hosts over the C2 table, of shd_relay_retable(NULL, NULL) against
shd_relay_get_host_state + shd_relay_setup.

    python tools/update_probe.py [c2|c3|relay ...]     (default: all three)
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shadow_amd import _native as N  # noqa: E402
from shadow_amd import synth  # noqa: E402
from shadow_amd.relay import Relay  # noqa: E402
from shadow_amd.routing import Engine, NetworkGraph  # noqa: E402

REPS, WARM = 20, 3


def med_ms(fn, reps=REPS, warm=WARM):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def routing(eng, name, el):
    g = NetworkGraph(el.node_ids, el.src, el.dst, el.latency_ns, el.packet_loss, el.directed)
    n, E = g.n_nodes, len(g.edge_src)
    used = np.arange(n, dtype=np.uint32)
    lat = torch.empty((n, n), dtype=torch.int64, device="cuda")
    loss = torch.empty((n, n), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    err = N.Error()
    lib, ctx = eng.lib, eng.ctx
    rng = np.random.default_rng(1)
    lo, hi = int(g.edge_latency_ns.min()), int(g.edge_latency_ns.max())

    def run():
        N.check(lib.shd_routing_run(ctx, N.ALGO_AUTO, 0, n, N.ptr(lat), N.ptr(loss), C.byref(err)), "run", err)

    def prepare(graph):
        cg = graph._cgraph()
        N.check(lib.shd_routing_prepare(ctx, C.byref(cg), N.ptr(used), n, N.ROUTE_SHORTEST, C.byref(err)), "prepare",
                err)

    prepare(g)
    run()
    print(f"== {name}: {n} nodes, {E} edges; shd_routing_run alone {med_ms(run):.3f} ms ==", flush=True)
    for k in (1, 1000, E):
        idx = rng.permutation(E)[:k].astype(np.uint32)
        # two weight sets of the graph's own range, applied in turn: every call changes every named edge
        sets = [(rng.integers(lo, hi + 1, k).astype(np.uint64), rng.uniform(0, 0.01, k).astype(np.float32))
                for _ in range(2)]
        turn = [0]

        def update():
            l, p = sets[turn[0] & 1]
            turn[0] += 1
            N.check(lib.shd_routing_update_edges(ctx, k, N.ptr(idx), N.ptr(l), N.ptr(p), C.byref(err)), "update", err)

        def update_run():
            update()
            run()

        mods = []
        for l, p in sets:
            m = NetworkGraph(g.node_ids, g.edge_src, g.edge_dst, g.edge_latency_ns.copy(),
                             g.edge_packet_loss.copy(), g.directed)
            m.edge_latency_ns[idx], m.edge_packet_loss[idx] = l, p
            mods.append(m)

        def prepare_run():
            prepare(mods[turn[0] & 1])
            turn[0] += 1
            run()

        prepare(g)   # a new prepare: the next update builds the map
        t0 = time.perf_counter()
        update()
        first = (time.perf_counter() - t0) * 1e3
        u, ur = med_ms(update), med_ms(update_run)
        pr = med_ms(prepare_run)
        print(f"{name} n={k:>7}: first update {first:8.3f} ms | update {u:7.3f} | update+run {ur:7.3f} | "
              f"prepare+run {pr:8.3f} | prepare+run / update+run {pr / ur:5.1f}x", flush=True)
        prepare(g)


def relay(eng):
    H, NN = 100_000, 1000
    el = synth.complete_graph(NN, 1)
    g = NetworkGraph(el.node_ids, el.src, el.dst, el.latency_ns, el.packet_loss, el.directed)
    pg = g.prepare(np.arange(NN, dtype=np.uint32), eng)
    pg.run_resident()
    host_node = synth.c5_host_nodes(H, NN)
    rl = Relay(host_node, synth.host_rng_states(H, 1), np.zeros(H, np.uint64), engine=eng)
    rng, nid = np.zeros((H, 4), np.uint64), np.zeros(H, np.uint64)
    lib, ctx = eng.lib, eng.ctx

    def retable():
        rl.retable()

    def setup_again():
        N.check(lib.shd_relay_get_host_state(ctx, N.ptr(rng), N.ptr(nid)), "get_host_state")
        N.check(lib.shd_relay_setup(ctx, H, N.ptr(host_node), NN, None, None, N.ptr(rng), N.ptr(nid)), "setup")

    a, b = med_ms(retable), med_ms(setup_again)
    print(f"== relay, {H} hosts on the {NN}-node table: shd_relay_retable(NULL, NULL) {a:.3f} ms | "
          f"get_host_state + shd_relay_setup {b:.3f} ms | {b / a:.1f}x ==", flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["c2", "c3", "relay"]
    with Engine(0) as eng:
        if "c2" in what:
            routing(eng, "C2", synth.complete_graph(1000, 1))
        if "c3" in what:
            routing(eng, "C3", synth.barabasi_albert(10_000, 3, 2))
        if "relay" in what:
            relay(eng)
