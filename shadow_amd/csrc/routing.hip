// The routing build's host side (routing_priv.h has the overview and the reference semantics):
// graph validation and the arc CSR, the prepare step with its packed and relabelled copies, the
// blocked engine's driver, and the ladder that picks an engine for a build.
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "routing_priv.h"

namespace shd {

__global__ __launch_bounds__(256) void arcs_pack(const uint32_t* __restrict__ dst,
                                                 const uint32_t* __restrict__ lat,
                                                 const float* __restrict__ loss,
                                                 uint4* __restrict__ out, uint2* __restrict__ out8,
                                                 float* __restrict__ outq, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float q = one_minus(loss[i]);
    out[i] = make_uint4(dst[i], lat[i], __float_as_uint(q), 0u);
    out8[i] = make_uint2(dst[i], lat[i]);   // compact arcs of the global-label kernel
    outq[i] = q;
}

// compact arcs only (the locality-ordered copy of the global-label kernel)
__global__ __launch_bounds__(256) void arcs_pack8(const uint32_t* __restrict__ dst, const uint32_t* __restrict__ lat,
                                                  const float* __restrict__ loss, uint2* __restrict__ out8,
                                                  float* __restrict__ outq, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out8[i] = make_uint2(dst[i], lat[i]);
    outq[i] = one_minus(loss[i]);
}

// per-build flags (one launch instead of three memsets): [0,16) overflow / misc = 0,
// [16,24) first unreachable pair = ~0, [24,64) = 0 (stats counters at 32)
__global__ __launch_bounds__(64) void flags_init(uint32_t* __restrict__ f) {
    const uint32_t t = threadIdx.x;
    if (t < 16) f[t] = (t == 4 || t == 5) ? 0xFFFFFFFFu : 0u;
}

static uint32_t gml_id(const shd_graph* g, uint32_t idx) {
    return g->node_ids ? g->node_ids[idx] : idx;
}

static shd_status validate(const shd_graph* g, const uint32_t* used, uint32_t n_used) {
    if (!g || !used || n_used == 0) return SHD_ERR_INVALID;
    if (g->n_edges && (!g->edge_src || !g->edge_dst || !g->edge_latency_ns || !g->edge_packet_loss))
        return SHD_ERR_INVALID;
    for (uint32_t i = 0; i < g->n_edges; i++) {
        if (g->edge_src[i] >= g->n_nodes || g->edge_dst[i] >= g->n_nodes) return SHD_ERR_INVALID;
        // ShadowEdge::try_from rejects latency 0 (graph/mod.rs:107); the kernels rely on every
        // arc strictly increasing latency (unique fixed point = Dijkstra's pop-order result)
        if (g->edge_latency_ns[i] == 0) return SHD_ERR_INVALID;
        const float p = g->edge_packet_loss[i];
        if (!(p >= 0.0f && p <= 1.0f)) return SHD_ERR_INVALID;  // ShadowEdge::try_from range
    }
    std::vector<uint8_t> seen(g->n_nodes, 0);
    for (uint32_t i = 0; i < n_used; i++) {
        if (used[i] >= g->n_nodes || seen[used[i]]) return SHD_ERR_INVALID;
        seen[used[i]] = 1;
    }
    return SHD_OK;
}

// Self-loop rule (graph/mod.rs:212-219 via get_edge_weight): exactly one per used node, first
// offender in `used` order.  Fills the diagonal values.
static shd_status diag_from_self_loops(const shd_graph* g, const uint32_t* used, uint32_t n_used,
                                       HostGraph& H, shd_error* err) {
    std::vector<uint32_t> cnt(g->n_nodes, 0), first(g->n_nodes, 0);
    for (uint32_t i = 0; i < g->n_edges; i++) {
        if (g->edge_src[i] != g->edge_dst[i]) continue;
        const uint32_t v = g->edge_src[i];
        if (cnt[v]++ == 0) first[v] = i;
    }
    H.diag_lat.resize(n_used);
    H.diag_loss.resize(n_used);
    for (uint32_t j = 0; j < n_used; j++) {
        const uint32_t v = used[j];
        if (cnt[v] == 0) return set_err(err, SHD_ERR_NO_EDGE, gml_id(g, v), gml_id(g, v));
        if (cnt[v] > 1) return set_err(err, SHD_ERR_MULTI_EDGE, gml_id(g, v), gml_id(g, v));
        H.diag_lat[j] = g->edge_latency_ns[first[v]];
        H.diag_loss[j] = g->edge_packet_loss[first[v]];
    }
    return SHD_OK;
}

// the out-CSR without self-loops (reverse: the in-CSR, for the wide path's pull rounds)
void build_csr(const shd_graph* g, bool reverse, HostGraph& H) {
    const uint32_t V = g->n_nodes;
    H.V = V;
    H.off.assign(V + 1, 0);
    for (uint32_t i = 0; i < g->n_edges; i++) {
        const uint32_t a = g->edge_src[i], b = g->edge_dst[i];
        if (a == b) continue;  // a self-loop never improves a label (latency > 0)
        H.off[(reverse && g->directed ? b : a) + 1]++;
        if (!g->directed) H.off[b + 1]++;
    }
    for (uint32_t v = 0; v < V; v++) H.off[v + 1] += H.off[v];
    const size_t A = H.off[V];
    H.dst.resize(A);
    H.lat.resize(A);
    H.loss.resize(A);
    std::vector<uint32_t> fill(H.off.begin(), H.off.end() - 1);
    H.max_arc_lat = 0;
    H.min_arc_lat = ~0ull;
    for (uint32_t i = 0; i < g->n_edges; i++) {
        const uint32_t a = g->edge_src[i], b = g->edge_dst[i];
        if (a == b) continue;
        const uint64_t l = g->edge_latency_ns[i];
        const float p = g->edge_packet_loss[i] + 0.0f;  // -0.0 -> +0.0: same fold, ordered bits
        H.max_arc_lat = std::max(H.max_arc_lat, l);
        H.min_arc_lat = std::min(H.min_arc_lat, l);
        H.sum_arc_lat += l;
        auto put = [&](uint32_t from, uint32_t to) {
            const uint32_t k = fill[from]++;
            H.dst[k] = to;
            H.lat[k] = l;
            H.loss[k] = p;
        };
        if (g->directed) {
            if (reverse) put(b, a); else put(a, b);
        } else {
            put(a, b);
            put(b, a);
        }
    }
    // each node's arcs in destination order (stable: parallel arcs keep GML order).  The kernels
    // do not depend on the order; a complete graph's CSR then IS its dense matrix without the
    // diagonal, which the prune reads directly (dense_rows)
    std::vector<uint32_t> idx;
    for (uint32_t u = 0; u < V; ++u) {
        const uint32_t b0 = H.off[u], b1 = H.off[u + 1];
        bool sorted = true;
        for (uint32_t k = b0 + 1; k < b1 && sorted; ++k) sorted = H.dst[k - 1] <= H.dst[k];
        if (sorted) continue;
        idx.resize(b1 - b0);
        for (uint32_t k = 0; k < b1 - b0; ++k) idx[k] = b0 + k;
        std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return H.dst[x] < H.dst[y]; });
        std::vector<uint32_t> d2(b1 - b0);
        std::vector<uint64_t> l2(b1 - b0);
        std::vector<float> p2(b1 - b0);
        for (uint32_t k = 0; k < b1 - b0; ++k) {
            d2[k] = H.dst[idx[k]];
            l2[k] = H.lat[idx[k]];
            p2[k] = H.loss[idx[k]];
        }
        std::copy(d2.begin(), d2.end(), H.dst.begin() + b0);
        std::copy(l2.begin(), l2.end(), H.lat.begin() + b0);
        std::copy(p2.begin(), p2.end(), H.loss.begin() + b0);
    }
}

// every node's arc list is exactly the other V - 1 nodes in index order (a complete graph with no
// parallel arcs): the CSR is the dense latency / loss matrix without its diagonal
static bool csr_is_dense(const HostGraph& H) {
    const uint32_t V = H.V;
    if (V < 2 || H.dst.size() != (size_t)V * (V - 1)) return false;
    for (uint32_t u = 0; u < V; ++u) {
        if (H.off[u] != (size_t)u * (V - 1)) return false;
        for (uint32_t k = 0; k + 1 < V; ++k)
            if (H.dst[H.off[u] + k] != k + (k >= u ? 1u : 0u)) return false;
    }
    return true;
}

shd_status reset_flags(shd_ctx* ctx) {
    SHD_TRY(ctx->g_flags.ensure(64));
    flags_init<<<1, 64, 0, ctx->stream>>>(ctx->g_flags.as<uint32_t>());
    SHD_HIP(hipGetLastError());
    return SHD_OK;
}

// Locality order for the global-label kernel (graphs whose labels leave the LDS, C4): nodes
// renumbered in breadth-first order from the highest-degree nodes, so a node's neighbours get
// nearby numbers -- the label reads and memory-side label atomics of one wave's relaxations then
// share cache lines instead of hitting one line each.  Only that kernel's copies are renumbered
// (offsets, compact arcs, the used list); results are indexed by used position, so the table is
// unchanged.  Next hops (lowest-index tie-break in GML order) run on the original numbering.
static shd_status prepare_reordered(shd_ctx* ctx, const HostGraph& H, const uint32_t* used, uint32_t n_used) {
    PreparedGraph& P = ctx->prep;
    P.reordered = false;
    const uint32_t V = P.V;
    if (V == 0 || (sssp_lds_bytes(V, 1024, false) <= ctx->max_lds && ctx->knobs.get(K_SSSP_REORDER, 0) != 1))
        return SHD_OK;   // the LDS kernels take this graph
    hipStream_t s = ctx->stream;
    std::vector<uint32_t> deg(V), roots(V), ord, pi(V, 0xFFFFFFFFu);
    for (uint32_t v = 0; v < V; ++v) {
        deg[v] = H.off[v + 1] - H.off[v];
        roots[v] = v;
    }
    std::stable_sort(roots.begin(), roots.end(), [&](uint32_t a, uint32_t b) { return deg[a] > deg[b]; });
    ord.reserve(V);
    // the K highest-degree nodes first: the global kernel keeps their labels in LDS (the LDS a
    // slot has left at 2 slots per CU, as run_sssp_global sizes it)
    {
        const size_t W = (V + 31) / 32;
        const size_t lds = W * 4 + 16 + 8 * (kQStride + kFlatWords) * 4 + ((size_t)V + 3) / 4 * 4;
        const size_t room = ctx->max_lds / 2;
        P.lds_labels = room > lds + 64 ? (uint32_t)std::min<size_t>(V, (room - lds - 16) / 8) & ~63u : 0u;
    }
    const uint32_t K = P.lds_labels;
    for (uint32_t i = 0; i < K && i < V; ++i) {
        pi[roots[i]] = (uint32_t)ord.size();
        ord.push_back(roots[i]);
    }
    {   // breadth-first from the hubs placed so far: their neighbours come next, together
        size_t head = 0;
        while (head < ord.size()) {
            const uint32_t u = ord[head++];
            for (uint32_t k = H.off[u]; k < H.off[u + 1]; ++k) {
                const uint32_t w = H.dst[k];
                if (pi[w] == 0xFFFFFFFFu) {
                    pi[w] = (uint32_t)ord.size();
                    ord.push_back(w);
                }
            }
        }
    }
    for (uint32_t r : roots) {   // breadth-first from each not yet numbered node, hubs first
        if (pi[r] != 0xFFFFFFFFu) continue;
        size_t head = ord.size();
        pi[r] = (uint32_t)ord.size();
        ord.push_back(r);
        while (head < ord.size()) {
            const uint32_t u = ord[head++];
            for (uint32_t k = H.off[u]; k < H.off[u + 1]; ++k) {
                const uint32_t w = H.dst[k];
                if (pi[w] == 0xFFFFFFFFu) {
                    pi[w] = (uint32_t)ord.size();
                    ord.push_back(w);
                }
            }
        }
    }
    const size_t A = H.dst.size();
    std::vector<uint32_t> offr(V + 1, 0), dstr(A), latr(A), usedr(n_used);
    std::vector<float> lossr(A);
    for (uint32_t i = 0; i < V; ++i) {
        const uint32_t u = ord[i];
        uint32_t at = offr[i];
        for (uint32_t k = H.off[u]; k < H.off[u + 1]; ++k, ++at) {
            dstr[at] = pi[H.dst[k]];
            latr[at] = (uint32_t)H.lat[k];
            lossr[at] = H.loss[k];
        }
        offr[i + 1] = at;
    }
    for (uint32_t j = 0; j < n_used; ++j) usedr[j] = pi[used[j]];
    SHD_TRY(upload(ctx->g_offr, offr, s));
    SHD_TRY(upload(ctx->g_usedr, usedr, s));
    DevBuf d_dst, d_lat, d_loss;
    SHD_TRY(upload(d_dst, dstr, s));
    SHD_TRY(upload(d_lat, latr, s));
    SHD_TRY(upload(d_loss, lossr, s));
    SHD_TRY(ctx->g_arc8r.ensure(std::max<size_t>(A, 1) * 8));
    SHD_TRY(ctx->g_aqr.ensure(std::max<size_t>(A, 1) * 4));
    if (A)
        arcs_pack8<<<div_up(A, 256), 256, 0, s>>>(d_dst.as<uint32_t>(), d_lat.as<uint32_t>(), d_loss.as<float>(),
                                                   ctx->g_arc8r.as<uint2>(), ctx->g_aqr.as<float>(), A);
    SHD_HIP(hipGetLastError());
    SHD_HIP(hipStreamSynchronize(s));   // the temporaries are freed on return
    P.pi_r = std::move(pi);   // shd_routing_update_edges finds the copy's slots through it
    P.reordered = true;
    return SHD_OK;
}

// Wave-spread relabelling for the 1024-thread LDS kernel (sparse graphs whose labels fill the
// LDS, C3).  Its bitmap word k belongs to wave k mod 16 for the whole build, so on a
// preferential-attachment graph -- hubs are the first nodes -- the first waves own every hub and
// the other waves wait for them at each sweep's barrier (24 % of the kernel).  The nodes are
// dealt in descending degree order to the 16 waves' words (rank r -> wave r mod 16), and the
// kernel runs on that copy of the CSR; the table is the same (labels are minima over paths, and
// the used columns keep their order: used[j] -> its new id).  C3 DELTA 6.79 -> 6.59 ms, tables
// identical (tools/c2_probe.py, SSSP_NO_SPREAD=1 alternated; a random relabelling: 7.05).  Not with next hops (the
// kernel would write relabelled ids) nor a seed (indexed by the original ids).
static shd_status prepare_spread(shd_ctx* ctx, const HostGraph& H, const uint32_t* used, uint32_t n_used) {
    PreparedGraph& P = ctx->prep;
    P.spread = false;
    const uint32_t V = P.V;
    constexpr uint32_t NW = 1024 / 64;
    const bool dense = V <= kPruneMaxV && P.arcs * 8 >= (uint64_t)V * V;   // the prune path instead
    if (V == 0 || dense || ctx->knobs.get(K_SSSP_NO_SPREAD, 0) == 1 ||
        sssp_lds_bytes(V, 1024, false) > ctx->max_lds ||          // global labels (C4)
        sssp_lds_bytes(V, 256, true) <= ctx->max_lds / 2)         // not the 1024-thread kernel
        return SHD_OK;
    hipStream_t s = ctx->stream;
    std::vector<uint32_t> deg(V), r2n(V);
    for (uint32_t v = 0; v < V; ++v) {
        deg[v] = H.off[v + 1] - H.off[v];
        r2n[v] = v;
    }
    std::stable_sort(r2n.begin(), r2n.end(), [&](uint32_t a, uint32_t b) { return deg[a] > deg[b]; });
    // rank r -> position ((q / 32) * NW + r mod NW) * 32 + q mod 32 (q = r / NW: the rank's place
    // among its wave's nodes), compacted to 0 .. V-1 in position order
    std::vector<uint64_t> pos(V);
    std::vector<uint32_t> byp(V);
    for (uint32_t r = 0; r < V; ++r) {
        const uint64_t q = r / NW;
        pos[r] = ((q / 32) * NW + r % NW) * 32 + q % 32;
        byp[r] = r;
    }
    std::stable_sort(byp.begin(), byp.end(), [&](uint32_t a, uint32_t b) { return pos[a] < pos[b]; });
    std::vector<uint32_t> pi(V), ord(V);   // node -> new id, new id -> node
    for (uint32_t i = 0; i < V; ++i) {
        ord[i] = r2n[byp[i]];
        pi[ord[i]] = i;
    }
    const size_t A = H.dst.size();
    std::vector<uint32_t> offs(V + 1, 0), dsts(A), lats(A), useds(n_used);
    std::vector<float> losss(A);
    for (uint32_t i = 0; i < V; ++i) {
        const uint32_t u = ord[i];
        uint32_t at = offs[i];
        for (uint32_t k = H.off[u]; k < H.off[u + 1]; ++k, ++at) {
            dsts[at] = pi[H.dst[k]];
            lats[at] = (uint32_t)H.lat[k];
            losss[at] = H.loss[k];
        }
        offs[i + 1] = at;
    }
    for (uint32_t j = 0; j < n_used; ++j) useds[j] = pi[used[j]];
    SHD_TRY(upload(ctx->g_offs, offs, s));
    SHD_TRY(upload(ctx->g_useds, useds, s));
    DevBuf d_dst, d_lat, d_loss, d_a8, d_q;
    SHD_TRY(upload(d_dst, dsts, s));
    SHD_TRY(upload(d_lat, lats, s));
    SHD_TRY(upload(d_loss, losss, s));
    SHD_TRY(ctx->g_arc16s.ensure(std::max<size_t>(A, 1) * 16));
    SHD_TRY(d_a8.ensure(std::max<size_t>(A, 1) * 8));
    SHD_TRY(d_q.ensure(std::max<size_t>(A, 1) * 4));
    if (A)
        arcs_pack<<<div_up(A, 256), 256, 0, s>>>(d_dst.as<uint32_t>(), d_lat.as<uint32_t>(), d_loss.as<float>(),
                                                  ctx->g_arc16s.as<uint4>(), d_a8.as<uint2>(), d_q.as<float>(), A);
    SHD_HIP(hipGetLastError());
    SHD_HIP(hipStreamSynchronize(s));   // the temporaries are freed on return
    P.pi_s = std::move(pi);   // (as P.pi_r)
    P.spread = true;
    return SHD_OK;
}

shd_status routing_prepare_impl(shd_ctx* ctx, const shd_graph* g, const uint32_t* used,
                                uint32_t n_used, uint32_t mode, shd_error* err) {
    if (err) *err = shd_error{SHD_OK, 0, 0};
    PreparedGraph& P = ctx->prep;
    P.ready = false;
    P.upd.built = false;   // the edge -> arc-slot map of the graph before (shd_routing_update_edges)
    SHD_TRY(validate(g, used, n_used));
    if (mode != SHD_ROUTE_SHORTEST && mode != SHD_ROUTE_DIRECT) return SHD_ERR_INVALID;
    hipStream_t s = ctx->stream;
    P.mode = mode;
    P.reordered = false;
    P.spread = false;
    P.V = g->n_nodes;
    P.n_used = n_used;
    P.directed = g->directed != 0;
    P.used.assign(used, used + n_used);
    P.used_ident = n_used == g->n_nodes;
    for (uint32_t j = 0; j < n_used && P.used_ident; j++) P.used_ident = used[j] == j;
    P.node_ids.resize(g->n_nodes);
    for (uint32_t v = 0; v < g->n_nodes; v++) P.node_ids[v] = gml_id(g, v);
    P.es.assign(g->edge_src, g->edge_src + g->n_edges);
    P.ed.assign(g->edge_dst, g->edge_dst + g->n_edges);
    P.el.assign(g->edge_latency_ns, g->edge_latency_ns + g->n_edges);
    P.ep.assign(g->edge_packet_loss, g->edge_packet_loss + g->n_edges);
    SHD_TRY(upload(ctx->g_used, P.used, s));
    if (mode == SHD_ROUTE_DIRECT) {
        std::vector<int32_t> col(g->n_nodes, -1);
        for (uint32_t j = 0; j < n_used; j++) col[used[j]] = (int32_t)j;
        SHD_TRY(upload(ctx->d_es, P.es, s));
        SHD_TRY(upload(ctx->d_ed, P.ed, s));
        SHD_TRY(upload(ctx->d_el, P.el, s));
        SHD_TRY(upload(ctx->d_ep, P.ep, s));
        SHD_TRY(upload(ctx->d_col, col, s));
    } else {
        HostGraph H;
        SHD_TRY(diag_from_self_loops(g, used, n_used, H, err));
        SHD_TRY(upload(ctx->g_diag_lat, H.diag_lat, s));
        SHD_TRY(upload(ctx->g_diag_loss, H.diag_loss, s));
        build_csr(g, /*reverse=*/false, H);
        P.arcs = H.dst.size();
        P.dense_rows = csr_is_dense(H);
        P.max_arc_lat = H.max_arc_lat;
        P.narrow_arcs = H.max_arc_lat < kLat32Inf;
        P.mean_arc_lat = H.dst.empty() ? 1u
                         : (uint32_t)std::min<double>(kLat32Inf - 1, H.sum_arc_lat / H.dst.size());
        P.min_arc_lat = H.dst.empty() ? 1u : (uint32_t)std::min<uint64_t>(kLat32Inf - 1, std::max<uint64_t>(H.min_arc_lat, 1));
        if (P.narrow_arcs) {
            std::vector<uint32_t> l32(H.lat.begin(), H.lat.end());
            SHD_TRY(upload(ctx->g_off, H.off, s));
            SHD_TRY(upload(ctx->g_dst, H.dst, s));
            SHD_TRY(upload(ctx->g_lat, l32, s));
            SHD_TRY(upload(ctx->g_aux, H.loss, s));
            SHD_TRY(ctx->g_arc16.ensure(std::max<size_t>(H.loss.size(), 1) * 16));
            SHD_TRY(ctx->g_arc8.ensure(std::max<size_t>(H.loss.size(), 1) * 8));
            SHD_TRY(ctx->g_aq.ensure(std::max<size_t>(H.loss.size(), 1) * 4));
            if (!H.loss.empty())
                arcs_pack<<<div_up(H.loss.size(), 256), 256, 0, s>>>(
                    ctx->g_dst.as<uint32_t>(), ctx->g_lat.as<uint32_t>(), ctx->g_aux.as<float>(),
                    ctx->g_arc16.as<uint4>(), ctx->g_arc8.as<uint2>(), ctx->g_aq.as<float>(), H.loss.size());
            P.pruned_arcs = 0;
            P.tight_arcs = 0;
            SHD_TRY(prepare_reordered(ctx, H, used, n_used));
            SHD_TRY(prepare_spread(ctx, H, used, n_used));
        }
    }
    SHD_HIP(hipStreamSynchronize(s));
    P.ready = true;
    return SHD_OK;
}

// blocked.hip
shd_status fw_latency(shd_ctx* ctx, uint32_t* D, uint32_t Vp, uint32_t T);
shd_status fw_tight(shd_ctx* ctx, const uint32_t* D, uint32_t Vp, uint32_t* pbeg, uint32_t* pend,
                    uint4* parcs, uint32_t* cursor);

// SHD_ALGO_BLOCKED (blocked.hip): latency closure by blocked min-plus, then the loss pass over
// the globally tight arcs with labels seeded from the closure rows.
static shd_status run_blocked(shd_ctx* ctx, uint32_t rb, uint32_t re, uint64_t* d_lat,
                              float* d_loss) {
    PreparedGraph& P = ctx->prep;
    hipStream_t s = ctx->stream;
    const uint32_t V = P.V;
    const uint32_t T = ctx->knobs.get(K_FW_TILE, V > 2048 ? 128 : 64) == 128 ? 128 : 64;
    const uint32_t Vp = (V + T - 1) / T * T;
    SHD_TRY(ctx->g_fw.ensure((size_t)Vp * Vp * 4));
    SHD_TRY(ctx->g_prune_dst.ensure(std::max<uint64_t>(P.arcs, 1) * 16));
    SHD_TRY(ctx->g_prune_cnt.ensure((size_t)V * 8 + 16));
    uint32_t* D = ctx->g_fw.as<uint32_t>();
    uint32_t* pbeg = ctx->g_prune_cnt.as<uint32_t>();
    uint32_t* pend = pbeg + V;
    uint32_t* cursor = pend + V;
    SHD_HIP(hipEventRecord(ctx->ev[4], s));
    SHD_TRY(fw_latency(ctx, D, Vp, T));
    SHD_HIP(hipEventRecord(ctx->ev[5], s));
    SHD_TRY(fw_tight(ctx, D, Vp, pbeg, pend, ctx->g_prune_dst.as<uint4>(), cursor));
    if (P.tight_arcs == 0) {   // the kept-arc count steers the lane-group width (once per graph)
        uint32_t k = 0;
        SHD_HIP(hipMemcpyAsync(&k, cursor, 4, hipMemcpyDeviceToHost, s));
        SHD_HIP(hipStreamSynchronize(s));
        P.tight_arcs = std::max<uint32_t>(k, 1);
    }
    ArcView A{pbeg, pend, ctx->g_prune_dst.as<uint4>(), P.tight_arcs};
    SHD_TRY(run_sssp(ctx, A, rb, re, d_lat, d_loss, kLat32Inf, D, Vp));
    float ms = 0;
    SHD_HIP(hipEventSynchronize(ctx->ev[5]));
    (void)hipEventElapsedTime(&ms, ctx->ev[4], ctx->ev[5]);
    ctx->info.ms_minplus = ms;
    ctx->info.arcs_kept = P.tight_arcs;
    return SHD_OK;
}

constexpr uint32_t kBlockedMaxV = 16384;   // closure matrix <= 1 GiB

// the dominant kernel's device time, when this build was timed (shd_routing_set_timing)
static float main_ms(shd_ctx* ctx) {
    // the read-back kernel (readback) can return before the runtime has seen the stop event
    // complete: wait for it, on timed builds only
    float ms = -1.0f;
    if (ctx->time_now && (hipEventSynchronize(ctx->ev[3]) != hipSuccess ||
                          hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]) != hipSuccess))
        ms = -1.0f;
    return ms;
}

shd_status routing_run_impl(shd_ctx* ctx, uint32_t algo, uint32_t rb, uint32_t re,
                            uint64_t* d_lat, float* d_loss, shd_error* err) {
    if (err) *err = shd_error{SHD_OK, 0, 0};
    PreparedGraph& P = ctx->prep;
    if (!P.ready) return SHD_ERR_STATE;
    if (re == 0) re = P.n_used;
    if (rb >= re || re > P.n_used) return SHD_ERR_INVALID;
    ctx->info = shd_routing_info{};
    ctx->info.arcs = P.arcs;
    ctx->info.arcs_kept = P.arcs;
    ctx->time_now = ctx->time_every != 0 && ctx->time_calls++ % ctx->time_every == 0;
    // labels + bitmap + queues (+ next hops: pred[V]) must fit the LDS for the LDS-label kernels
    const size_t lds = sssp_lds_bytes(P.V, 1024, false) + (ctx->nh_out ? (size_t)P.V * 4 + 8 : 0);
    const bool blocked = algo == SHD_ALGO_BLOCKED && P.narrow_arcs && lds <= ctx->max_lds && P.V <= kBlockedMaxV;
    const bool lds_path = !blocked && P.narrow_arcs && lds <= ctx->max_lds && ctx->knobs.get(K_SSSP_GLOBAL, 0) != 1;
    const bool dense = P.V <= kPruneMaxV && P.arcs * 8 >= (uint64_t)P.V * P.V;
    const bool prune = lds_path && P.mode != SHD_ROUTE_DIRECT &&
                       (algo == SHD_ALGO_PRUNED || ((algo == SHD_ALGO_AUTO || algo == SHD_ALGO_DELTA) && dense)) &&
                       P.V <= kPruneMaxV;
    SHD_TRY(ctx->g_flags.ensure(64));
    if (!prune) SHD_TRY(reset_flags(ctx));   // the prune path's dense_build (or prune_rows) resets them
    // wall time of the call (host clock): timing events between the build's kernels cost a
    // few microseconds of queue bubble each, so only the main kernel is bracketed by events
    const auto t_call = std::chrono::steady_clock::now();
    auto call_ms = [&] {
        return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    };
    if (P.mode == SHD_ROUTE_DIRECT) {
        shd_status st = run_direct(ctx, rb, re, d_lat, d_loss, err);
        float ms = 0;
        ms = call_ms();
        ctx->info.ms_total = ctx->info.ms_main = ms;
        return st;
    }
    if (blocked) {
        SHD_TRY(run_blocked(ctx, rb, re, d_lat, d_loss));
        ctx->info.algo_used = SHD_ALGO_BLOCKED;
        SHD_TRY(read_flags(ctx));
        const bool ovf = flag_ovf(ctx);
        float ms = 0, ms_main = 0;
        ms = call_ms();
        ms_main = main_ms(ctx);
        ctx->info.ms_total = ms;
        ctx->info.ms_main = ms_main;
        if (!ovf) {
            // an INF closure entry is unreachable OR >= 2^32-1 ns: let the u64 path decide
            const shd_status st = check_unreach(ctx, err);
            if (st != SHD_ERR_UNREACHABLE) return st;
            if (err) *err = shd_error{SHD_OK, 0, 0};
        }
        SHD_TRY(reset_flags(ctx));
        return run_wide(ctx, rb, re, d_lat, d_loss, err);
    }
    if (lds_path) {
        ArcView A{ctx->g_off.as<uint32_t>(), ctx->g_off.as<uint32_t>() + 1, ctx->g_arc16.as<uint4>(),
                  P.arcs};
        if (!prune && P.spread && !ctx->nh_out && ctx->knobs.get(K_SSSP_NO_SPREAD, 0) != 1) {   // prepare_spread
            A = ArcView{ctx->g_offs.as<uint32_t>(), ctx->g_offs.as<uint32_t>() + 1, ctx->g_arc16s.as<uint4>(), P.arcs};
            A.used = ctx->g_useds.as<uint32_t>();
        }
        if (prune) {
            SHD_TRY(run_prune(ctx, &A));
            // the kept-arc count steers the lane-group width: counted once per prepared graph,
            // before its first SSSP launch, so every build (the first too) runs the same kernel
            // (again if a knob changed the prune path between two builds of one prepared graph)
            if (P.pruned_arcs == 0 || P.pruned_pad != A.pad || P.pruned_path != A.path) SHD_TRY(count_kept(ctx, A));
            A.n_arcs = P.pruned_arcs;
        }
        // delta-stepping bucket width (env override for tuning).  SHD_ALGO_DELTA: the mean arc
        // latency x 1.5 (below).  AUTO on a pruned dense graph: the smallest arc latency (never pruned: every
        // detour has two arcs), floored at mean/256 so that a stray tiny arc cannot make the
        // sweep count explode -- a bucket no wider than every arc settles in one sweep, so each
        // node is expanded once (Dial order); the sweep jumps to the smallest active label, so
        // empty buckets cost nothing.  C2: 1 ms -> main kernel 172 -> 120 us, tables identical.
        // AUTO on a sparse graph: buckets of the mean arc latency (C3: 9.9 ms against 11.6 for
        // plain sweeps; 5 ms buckets 11.4, 2 ms 15.8)
        uint32_t delta = kLat32Inf;
        // (LDS labels: 1.5 x mean_arc_lat.  C3 with the hub relaxation, round 5, tools/c3_delta_sweep.sh:
        // 8 ms 7.85, 10 ms 7.38, 12.5 ms (1.0 x, the old default) 7.03, 16 ms 6.88, 20 ms 6.83-6.84,
        // 25 ms 7.02, 30 ms 7.17, 40 ms 7.64)
        if (algo == SHD_ALGO_DELTA || (algo == SHD_ALGO_AUTO && !prune))
            delta = ctx->knobs.get(K_SSSP_DELTA, (uint32_t)std::min<uint64_t>(kLat32Inf - 1, (uint64_t)P.mean_arc_lat * 3 / 2));
        else if (algo == SHD_ALGO_AUTO && prune)
            delta = ctx->knobs.get(K_SSSP_DELTA, std::max(P.min_arc_lat, P.mean_arc_lat / 256));
        SHD_TRY(run_sssp(ctx, A, rb, re, d_lat, d_loss, delta));
        ctx->info.algo_used = algo == SHD_ALGO_DELTA ? SHD_ALGO_DELTA
                              : prune ? SHD_ALGO_PRUNED : delta != kLat32Inf ? SHD_ALGO_DELTA : SHD_ALGO_SSSP;
        SHD_TRY(read_flags(ctx));
        const bool ovf = flag_ovf(ctx);
        float ms = 0, ms_main = 0;
        ms = call_ms();
        ms_main = main_ms(ctx);
        ctx->info.ms_total = ms;
        ctx->info.ms_main = ms_main;
        ctx->info.arcs_kept = prune ? P.pruned_arcs : P.arcs;
        if (!ovf) return check_unreach(ctx, err);
        SHD_TRY(reset_flags(ctx));  // some path latency >= 2^32-1 ns: redo with u64 labels
    }
    if (P.narrow_arcs && (lds > ctx->max_lds || ctx->knobs.get(K_SSSP_GLOBAL, 0) == 1)) {
        // labels exceed the LDS: global-label kernel (C4)
        // bucket width: 0.52 x mean_arc_lat, never below the smallest arc.  (mean_arc_lat is the
        // edge latencies' sum over the arc count: half the mean edge latency of an undirected
        // graph -- C4: 12.5 ms of 25 -- so this is 6.5 ms.)  Re-swept at the end of round 2 with
        // the LDS labels and locality order: rows 0-4095 (tools/c4_delta_sweep.sh) 3 ms 20.2 ms,
        // 4 ms 19.4, 5 ms 19.1, 6 ms 19.0, 8 ms 19.3, 10 ms 20.0, 15 ms 22.2; full builds
        // alternated on one box (tools/c4_full_ab.sh) 4 ms 232.3, 5 ms 229.0 / 229.2, 6 ms 228.4 -
        // 228.8, 7 ms 231.0, 10 ms 241.2 / 242.0.  Round 6 (tools/c4_full_ab.sh, alternated): 5 ms
        // 194.2-194.4, 6.5 ms 193.0-193.2, 8 ms 194.8 -> 0.52 x mean_arc_lat
        uint32_t delta = kLat32Inf;
        if (algo == SHD_ALGO_DELTA)
            delta = ctx->knobs.get(K_SSSP_DELTA, std::max(P.min_arc_lat, (uint32_t)(P.mean_arc_lat * 13ull / 25)));
        ArcView A{ctx->g_off.as<uint32_t>(), ctx->g_off.as<uint32_t>() + 1, ctx->g_arc16.as<uint4>(),
                  P.arcs};
        SHD_TRY(run_sssp_global(ctx, A, rb, re, d_lat, d_loss, delta));
        ctx->info.algo_used = algo == SHD_ALGO_DELTA ? SHD_ALGO_DELTA : SHD_ALGO_SSSP;
        SHD_TRY(read_flags(ctx));
        const bool ovf = flag_ovf(ctx);
        float ms = 0, ms_main = 0;
        ms = call_ms();
        ms_main = main_ms(ctx);
        ctx->info.ms_total = ms;
        ctx->info.ms_main = ms_main;
        if (!ovf) return check_unreach(ctx, err);
        SHD_TRY(reset_flags(ctx));
    }
    return run_wide(ctx, rb, re, d_lat, d_loss, err);
}

}  // namespace shd

// Test hook (not part of the ABI header): the vector registers of the shipped SSSP kernels,
// which sit at the budgets their residency needs (tests/test_routing_gpu.py): 0 = C4's global-
// label kernel, sssp_global_group<512, 4, 4, true> (two 512-thread slots per CU: <= 128), 1 = C2's
// padded-list kernel, sssp_lds_shadow<256, 8, 4> (32-slot lists, G = 8 x 4 arcs per lane,
// fire-and-forget sweeps; four 256-thread workgroups per CU: <= 128), 2 = C3's 1024-thread kernel,
// sssp_lds_group<1024, 4, 2, false, 0> (<= 128).  Each SSSP unit answers for its own kernel.
extern "C" int shd_debug_kernel_vgprs(int which) {
    return which == 0 ? shd::sssp_global_vgprs() : shd::sssp_lds_vgprs(which == 1);
}
