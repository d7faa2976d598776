// The host side of shd_routing_update_edges (routing_update.hip): the call's validation, the
// last-entry-wins pass over its entries, and the map from an edge of shd_graph (GML order) to the
// slots of its arcs in build_csr's out-CSR.  No HIP type in here: tests/edge_update_main.cpp
// compiles this header alone, with the address and undefined-behaviour sanitizers, and
// tests/test_edge_update.py runs it against a numpy model.
//
// build_csr (routing.hip) fills each node's arcs in GML order -- an undirected edge (a, b) adds
// a -> b, then b -> a -- and then sorts each node's arcs by destination, stably.  A non-loop edge
// gives a node at most one arc, so within a node the arcs stand in (destination, edge index)
// order: parallel arcs keep GML order within a destination.  Self-loops have no arc (the
// diagonal takes their weights).  The relabelled copies (prepare_reordered, prepare_spread) move
// whole nodes and keep a node's arcs in order: slot k of node u is off_copy[pi[u]] + (k - off[u]).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace shd {

constexpr uint32_t kNoSlot = 0xFFFFFFFFu;   // no arc: a self-loop, or a directed edge's reverse

struct EdgeSlots {
    std::vector<uint32_t> off;        // [V + 1] the out-CSR's offsets
    std::vector<uint32_t> fwd, rev;   // per edge: the slot of src -> dst and of dst -> src
    std::vector<uint32_t> stamp;      // per edge: the call that named it last (edge_updates_unique)
    uint32_t call = 0;
    uint64_t sum_lat = 0;             // the edge latencies' sum, each non-loop edge once (mod 2^64)
    bool built = false;
};

// The map of a graph's edges, in build_csr's order.  O(E log) once per prepared graph.
inline void edge_slots_build(uint32_t V, uint64_t E, const uint32_t* es, const uint32_t* ed, bool directed,
                             EdgeSlots& M) {
    M.off.assign((size_t)V + 1, 0);
    for (uint64_t i = 0; i < E; ++i) {
        if (es[i] == ed[i]) continue;
        M.off[es[i] + 1]++;
        if (!directed) M.off[ed[i] + 1]++;
    }
    for (uint32_t v = 0; v < V; ++v) M.off[v + 1] += M.off[v];
    const size_t A = M.off[V];
    // the arcs in fill order: the edge, and bit 0 of `ad` = the reverse arc
    std::vector<uint32_t> ae(A), ad(A), dst(A), fill(M.off.begin(), M.off.end() - 1);
    for (uint64_t i = 0; i < E; ++i) {
        const uint32_t a = es[i], b = ed[i];
        if (a == b) continue;
        uint32_t k = fill[a]++;
        ae[k] = (uint32_t)i;
        ad[k] = 0;
        dst[k] = b;
        if (!directed) {
            k = fill[b]++;
            ae[k] = (uint32_t)i;
            ad[k] = 1;
            dst[k] = a;
        }
    }
    M.fwd.assign(E, kNoSlot);
    M.rev.assign(E, kNoSlot);
    std::vector<uint32_t> idx;
    for (uint32_t u = 0; u < V; ++u) {
        const uint32_t b0 = M.off[u], b1 = M.off[u + 1];
        idx.resize(b1 - b0);
        for (uint32_t k = 0; k < b1 - b0; ++k) idx[k] = b0 + k;
        std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return dst[x] < dst[y]; });
        for (uint32_t k = 0; k < b1 - b0; ++k) (ad[idx[k]] ? M.rev : M.fwd)[ae[idx[k]]] = b0 + k;
    }
    M.stamp.assign(E, 0);
    M.call = 0;
    M.built = true;
}

// The offsets of a relabelled copy: node u's arcs start at copy_off[pi[u]] (pi: node -> new id, a
// permutation of 0 .. V-1).  Returns per node the copy's first slot.
inline std::vector<uint32_t> edge_copy_starts(const std::vector<uint32_t>& off, const std::vector<uint32_t>& pi) {
    const size_t V = pi.size();
    std::vector<uint32_t> ord(V), start(V);
    for (size_t u = 0; u < V; ++u) ord[pi[u]] = (uint32_t)u;
    uint32_t at = 0;
    for (size_t i = 0; i < V; ++i) {
        start[ord[i]] = at;
        at += off[ord[i] + 1] - off[ord[i]];
    }
    return start;
}

// validate()'s rules (routing.hip) for the entries of one call; nothing is changed by it
inline bool edge_updates_valid(uint64_t n, uint64_t n_edges, const uint32_t* edge_index, const uint64_t* latency_ns,
                               const float* packet_loss) {
    if (n && (!edge_index || !latency_ns || !packet_loss)) return false;
    for (uint64_t i = 0; i < n; ++i) {
        if (edge_index[i] >= n_edges) return false;
        if (latency_ns[i] == 0) return false;
        const float p = packet_loss[i];
        if (!(p >= 0.0f && p <= 1.0f)) return false;
    }
    return true;
}

// The entries that count: an edge named more than once takes its last entry.  Returns the
// positions of those entries, last to first; O(n) (the stamps are per edge, one word).
inline std::vector<uint64_t> edge_updates_unique(EdgeSlots& M, uint64_t n, const uint32_t* edge_index) {
    if (++M.call == 0) {   // the stamp wrapped: start over
        std::fill(M.stamp.begin(), M.stamp.end(), 0u);
        M.call = 1;
    }
    std::vector<uint64_t> keep;
    keep.reserve(n);
    for (uint64_t i = n; i-- > 0;) {
        uint32_t& s = M.stamp[edge_index[i]];
        if (s == M.call) continue;
        s = M.call;
        keep.push_back(i);
    }
    return keep;
}

}  // namespace shd
