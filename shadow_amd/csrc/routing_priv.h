// Routing build on gfx950: lexicographic (latency, loss) shortest paths into the dense
// used-node table, and the direct-path mode.  The overview, and what the routing units share.
//
// Reference semantics (FlyearthR/shadow src/main/network/graph/mod.rs):
//   compute_shortest_paths :185-230 -- one petgraph Dijkstra per used source; the result of
//     each is the lexicographic minimum over walks of the LEFT-FOLDED path cost (latency u64
//     add; loss 1f32-(1f32-p)*(1f32-e), edge on the right).  Every non-loop edge strictly
//     increases latency and the fold is monotone, so the minimum is a unique fixed point: any
//     label-correcting relaxation that always appends one edge on the right converges to the
//     same bits as Dijkstra.  That is what the kernels do (never segment composition, which is
//     not associative in f32 -- SURVEY F2).
//   diagonal := the node's single self-loop edge, raw loss (:212-219); unreachable -> panic
//     (:221); get_direct_paths :232-254 with get_edge_weight :258-295.
//
// Engines (one stream; the ladder routing_run_impl picks among them):
//   LDS labels     one workgroup per source row, labels and bitmap in LDS: node groups on plain or
//                  padded arc lists, fire-and-forget "shadow" sweeps on the padded lists (C2, C3)
//   global labels  a persistent grid of slots, labels in global memory, edge-parallel expansion,
//                  for graphs whose labels leave the LDS (C4)
//   dense prune    2-hop / 3-hop detour tests that leave a dense graph's tight arcs as padded
//                  lists for the LDS kernels (prune_rows, prune_rows2; nearest_rows + prune_fused)
//   blocked        latency closure by blocked min-plus (blocked.hip), then a seeded loss pass of
//                  the LDS kernel over the tight arcs
//   wide, direct   the u64 rerun when a path latency leaves u32, and the direct-path mode
// Units -- every kernel is defined in one unit and launched only there; another unit reaches it
// through a host function declared below:
//   routing.hip             arcs_pack, arcs_pack8, flags_init; graph validation and the CSR, the
//                           prepare step with its relabelled copies, the blocked engine's driver,
//                           the ladder, the C test hook
//   routing_sssp_lds.hip    sssp_lds_group, sssp_lds_shadow
//   routing_sssp_global.hip sssp_global_group
//   sssp_row.h              device templates only: one source row (sssp_row, row_emit and the
//                           relaxations), included by the two SSSP units
//   routing_prune.hip       dense_build, prune_rows, prune_rows2, nearest_rows, prune_fused
//   routing_wide.hip        sssp_wide_round, wide_*, arcs_q, direct_*
//   routing_update.hip      edge_patch, edge_patch_direct, lat_minmax: shd_routing_update_edges
// Edge updates (shd_routing_update_edges): the builds recompute everything but the prepared
// graph's own arrays on every run, so new weights for n edges are one patch of those arrays.  The
// host (edge_update.h, no HIP types) validates the whole call, keeps the last entry of an edge
// named twice, and maps an edge to its arc slots in build_csr's order (the map is built at the
// first update after a prepare and is resident on the device, as are the slots in the two
// relabelled copies, found through the node permutations prepare keeps).  edge_patch writes whole
// records into g_lat / g_aux / g_arc16 / g_arc8 / g_aq, the copies and the diagonal; lat_minmax
// then reduces the arc latencies so that PreparedGraph's max / min are exact (the prune's bin
// shift, the padded kernels' overflow guard, the bucket widths); the mean keeps prepare's
// definition through an integer sum adjusted per edge; the kept-arc counts are counted again by
// the next build.  A graph with an arc beyond u32 before or after the call is prepared again from
// the context's host copies.
#pragma once
#include <algorithm>
#include <vector>

#include <hip/hip_ext.h>

#include "ctx.h"

namespace shd {

struct HostGraph {
    uint32_t V = 0;
    std::vector<uint32_t> off, dst;      // out-CSR without self-loops (petgraph edges(node))
    std::vector<uint64_t> lat;
    std::vector<float> loss;
    std::vector<uint64_t> diag_lat;      // per used index
    std::vector<float> diag_loss;
    uint64_t max_arc_lat = 0, min_arc_lat = 0;
    double sum_arc_lat = 0;
};

struct ArcView {
    const uint32_t *beg, *end;
    const uint4* arcs;
    uint64_t n_arcs;
    uint32_t pad = 0;      // lists padded to this many slots with no-op arcs (prune_rows 64, prune_rows2 32; 0: not)
    const uint32_t* used = nullptr;   // a relabelled copy (prepare_spread): the used nodes' new ids
    uint32_t path = 0;     // run_prune: which prune kernels made the lists (count_kept recounts when it changes)
};

constexpr uint32_t kQCap = 64;   // per-wave expansion queue: flushed at kQCap, one scan step adds <= 64
constexpr uint32_t kQStride = kQCap + 64;
constexpr uint32_t kFlatWords = 257;   // per-wave scratch of expand_flat: pre[65], beg, lat, q [64]
constexpr uint32_t kPad1 = 64, kPad2 = 32;   // list padding in slots: prune_rows, prune_rows2
constexpr uint32_t kPruneMaxV = 4096;        // the dense prune's LDS rows hold at most this many nodes

// LDS of the LDS-label kernels: labels + bitmap + control + per-wave queues (+ arc ranges,
// 8-byte aligned)
inline size_t sssp_lds_bytes(uint32_t V, uint32_t block, bool cache) {
    const size_t head = (size_t)(V + 64) * 8 + (size_t)((V + 31) / 32) * 4 + 16 + (block / 64) * kQStride * 4;
    return cache ? ((head + 7) & ~(size_t)7) + (size_t)V * 8 : head;
}

inline shd_status set_err(shd_error* err, shd_status st, uint32_t a, uint32_t b) {
    if (err) {
        err->code = st;
        err->node_a = a;
        err->node_b = b;
    }
    return st;
}

template <class T>
shd_status upload(DevBuf& b, const std::vector<T>& v, hipStream_t s) {
    SHD_TRY(b.ensure(std::max<size_t>(v.size(), 1) * sizeof(T)));
    if (!v.empty()) SHD_HIP(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return SHD_OK;
}

// one pinned read-back of the build flags (overflow word, first unreachable pair) and one sync
inline shd_status read_flags(shd_ctx* ctx) {
    return readback(ctx, ctx->stream, 0, ctx->g_flags.p, 24);
}
inline bool flag_ovf(const shd_ctx* ctx) { return (uint32_t)ctx->h_pin[0] != 0; }

// the first unreachable pair of the last read_flags (the reference panics there, graph/mod.rs:221)
inline shd_status check_unreach(shd_ctx* ctx, shd_error* err) {
    PreparedGraph& P = ctx->prep;
    const unsigned long long bad = ctx->h_pin[2];
    if (bad != ~0ull) {
        const uint32_t r = (uint32_t)(bad / P.n_used), c = (uint32_t)(bad % P.n_used);
        return set_err(err, SHD_ERR_UNREACHABLE, P.node_ids[P.used[r]], P.node_ids[P.used[c]]);
    }
    return SHD_OK;
}

// routing.hip
void build_csr(const shd_graph* g, bool reverse, HostGraph& H);
shd_status reset_flags(shd_ctx* ctx);   // the per-build flags back to their start values (flags_init)

// routing_sssp_lds.hip: rows [rb, re) on LDS labels; seed (blocked engine): labels start at the
// closure's latencies.  The caller reads the overflow flag with read_flags().
shd_status run_sssp(shd_ctx* ctx, const ArcView& A, uint32_t rb, uint32_t re, uint64_t* d_lat, float* d_loss,
                    uint32_t delta, const uint32_t* seed = nullptr, uint32_t ss = 0);
int sssp_lds_vgprs(int shadow);   // registers of C2's shadow kernel (1) or C3's 1024-thread kernel (0)

// routing_sssp_global.hip: the same on global labels
shd_status run_sssp_global(shd_ctx* ctx, const ArcView& A, uint32_t rb, uint32_t re, uint64_t* d_lat,
                           float* d_loss, uint32_t delta);
int sssp_global_vgprs();          // registers of C4's kernel

// routing_prune.hip: the pruned, padded arc lists of a dense graph, and their arc count into
// PreparedGraph (one read-back, once per prepared graph and prune path)
shd_status run_prune(shd_ctx* ctx, ArcView* out);
shd_status count_kept(shd_ctx* ctx, const ArcView& A);

// routing_wide.hip
shd_status run_wide(shd_ctx* ctx, uint32_t rb, uint32_t re, uint64_t* d_lat, float* d_loss, shd_error* err);
shd_status run_direct(shd_ctx* ctx, uint32_t rb, uint32_t re, uint64_t* d_lat, float* d_loss, shd_error* err);

}  // namespace shd
