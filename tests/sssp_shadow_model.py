"""CPU model of the dense SSSP's fire-and-forget sweeps (sssp_lds_shadow, shadow_amd/csrc/routing_sssp_lds.hip).

A plain restatement of the sweep rule, with none of the kernel's machinery:

  * labels are (latency, loss f32) pairs, +inf at first, the source (0, 0.0); a relaxation is a
    minimum that returns nothing;
  * every node has a shadow, the label it was last queued with (+inf at first).  A sweep reads the
    labels: a node is active iff label != shadow, selected iff also latency <= lo + delta; a
    selected node's shadow becomes the label read, an unselected active node feeds m_unsel;
  * the selected nodes are expanded from the label they hold *when expanded* (re-read);
  * floor: lo' = min(m_unsel, lo + amin) if anything was selected, else m_unsel; the row ends when
    nothing was selected and nothing active was left;
  * a cap on the sweep count (2 V + 64).

The kernel's waves scan and expand side by side between two barriers.  `waves` splits the nodes
into that many groups, each of which scans and then expands before the next one scans, so a later
group's scan already sees this sweep's relaxations; `order` picks the order of the nodes (and so
of the relaxations) within a sweep: "fwd", "rev", or a numpy Generator for a fresh shuffle per
sweep.
"""
from __future__ import annotations

import numpy as np

from oracle.routing import fold

INF = (float("inf"), np.float32(0.0))


def sweep_cap(n_nodes: int) -> int:
    return 2 * n_nodes + 64


def shadow_sssp(adj, src: int, delta: int, amin: int, order="fwd", waves: int = 1):
    """adj[u] = [(v, latency_ns, loss f32), ...] -> (labels, sweeps, capped).

    labels[v] = (latency, loss) or INF; sweeps counts every sweep, the closing scan included."""
    n = len(adj)
    lab = [INF] * n
    lab[src] = (0, np.float32(0.0))
    shadow = [INF] * n
    cap = sweep_cap(n)
    lo, sweeps = 0, 0
    while True:
        if sweeps >= cap:
            return lab, sweeps, True
        thr = lo + delta
        nodes = list(range(n))
        if order == "rev":
            nodes.reverse()
        elif order != "fwd":
            order.shuffle(nodes)
        any_sel, m_unsel = False, float("inf")
        for w in range(waves):
            sel = []
            for v in nodes[w::waves]:
                l = lab[v]
                if l != shadow[v]:
                    if l[0] <= thr:
                        shadow[v] = l
                        sel.append(v)
                    else:
                        m_unsel = min(m_unsel, l[0])
            for u in sel:
                lu = lab[u]   # re-read: a relaxation of this sweep may have lowered it
                for (v, elat, eloss) in adj[u]:
                    cand = (lu[0] + elat, fold(lu[1], eloss))
                    if cand < lab[v]:
                        lab[v] = cand
            any_sel = any_sel or bool(sel)
        sweeps += 1
        nxt = min(m_unsel, lo + amin) if any_sel else m_unsel
        if nxt == float("inf"):
            return lab, sweeps, False
        lo = nxt
