// shd_routing_update_edges: new weights for edges of the prepared graph, patched into the resident
// arc arrays (routing_priv.h has the overview; the host logic is edge_update.h's).  After the
// first call, which builds the edge -> arc-slot map, a call of n edges costs O(n) host work, one
// upload of 16 n bytes, and three launches: the patch, the min / max reduction over the arc
// latencies, and the read-back of its two words.
#include "routing_priv.h"
#include "wave.h"

namespace shd {

shd_status routing_prepare_impl(shd_ctx* ctx, const shd_graph* g, const uint32_t* used,
                                uint32_t n_used, uint32_t mode, shd_error* err);

// what the patch writes: the prepared graph's arc arrays and the copies prepare made (or null)
struct PatchArrays {
    const uint2 *map, *map_r, *map_s;   // per edge: the slots of src -> dst and dst -> src
    const uint32_t* dst;
    uint32_t* lat;
    float* aux;
    uint4* arc16;
    uint2* arc8;
    float* aq;
    uint2* arc8r;
    float* aqr;
    uint4* arc16s;
    uint64_t* diag_lat;
    float* diag_loss;
    unsigned long long* red;   // {min, max} of lat_minmax: set to their start values here
};

// One thread per (update, direction), then one per diagonal entry.  A record is {edge, loss bits,
// latency low, high}; an arc record's loss is p + 0.0f as build_csr stores it, and q comes from
// the device function arcs_pack uses, so a patched arc and a freshly packed one agree in every bit.
// A diagonal record holds the used index in place of the edge and the raw loss.  No two threads
// share a slot: the host keeps one entry per edge, and every arc has one edge.
__global__ __launch_bounds__(256) void edge_patch(const uint4* __restrict__ rec, uint64_t n_arc, uint64_t n_diag,
                                                  PatchArrays a) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t == 0) {
        a.red[0] = ~0ull;
        a.red[1] = 0ull;
    }
    if (t < 2 * n_arc) {
        const uint4 r = rec[t >> 1];
        const bool back = (t & 1) != 0;
        const uint2 m = a.map[r.x];
        const uint32_t slot = back ? m.y : m.x;
        if (slot == kNoSlot) return;   // a directed edge has no reverse arc
        const float p = __uint_as_float(r.y);
        const float q = one_minus(p);
        const uint32_t l = r.z;
        const uint32_t d = a.dst[slot];
        a.lat[slot] = l;
        a.aux[slot] = p;
        a.arc16[slot] = make_uint4(d, l, __float_as_uint(q), 0u);
        a.arc8[slot] = make_uint2(d, l);
        a.aq[slot] = q;
        if (a.map_r) {   // the locality-ordered copy keeps its relabelled destination
            const uint2 mr = a.map_r[r.x];
            const uint32_t s = back ? mr.y : mr.x;
            a.arc8r[s] = make_uint2(a.arc8r[s].x, l);
            a.aqr[s] = q;
        }
        if (a.map_s) {   // and so does the wave-spread copy
            const uint2 ms = a.map_s[r.x];
            const uint32_t s = back ? ms.y : ms.x;
            a.arc16s[s] = make_uint4(a.arc16s[s].x, l, __float_as_uint(q), 0u);
        }
    } else if (t < 2 * n_arc + n_diag) {
        const uint4 r = rec[n_arc + (t - 2 * n_arc)];
        a.diag_lat[r.x] = (uint64_t)r.z | ((uint64_t)r.w << 32);
        a.diag_loss[r.x] = __uint_as_float(r.y);
    }
}

// direct mode keeps the edge arrays themselves: one thread per update
__global__ __launch_bounds__(256) void edge_patch_direct(const uint4* __restrict__ rec, uint64_t n,
                                                         uint64_t* __restrict__ el, float* __restrict__ ep) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const uint4 r = rec[t];
    el[r.x] = (uint64_t)r.z | ((uint64_t)r.w << 32);
    ep[r.x] = __uint_as_float(r.y);
}

// The smallest and largest arc latency after the patch: 16-byte loads, grid-stride, a wave
// reduction, and one atomic pair per workgroup (max_u64_kernel in rounds.hip has the reason).
__global__ __launch_bounds__(256) void lat_minmax(const uint32_t* __restrict__ lat, uint64_t n,
                                                  unsigned long long* __restrict__ red) {
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    const uint64_t n4 = n / 4, step = (uint64_t)gridDim.x * 256;
    const uint4* lat4 = reinterpret_cast<const uint4*>(lat);
    uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * step < n4; i += 4 * step) {   // four independent loads in flight per lane
        const uint4 a = lat4[i], b = lat4[i + step], c = lat4[i + 2 * step], d = lat4[i + 3 * step];
        lo = min(min(min(lo, a.x), min(a.y, min(a.z, a.w))), min(min(b.x, b.y), min(b.z, b.w)));
        lo = min(min(min(lo, c.x), min(c.y, min(c.z, c.w))), min(min(d.x, d.y), min(d.z, d.w)));
        hi = max(max(max(hi, a.x), max(a.y, max(a.z, a.w))), max(max(b.x, b.y), max(b.z, b.w)));
        hi = max(max(max(hi, c.x), max(c.y, max(c.z, c.w))), max(max(d.x, d.y), max(d.z, d.w)));
    }
    for (; i < n4; i += step) {
        const uint4 v = lat4[i];
        lo = min(min(lo, v.x), min(v.y, min(v.z, v.w)));
        hi = max(max(hi, v.x), max(v.y, max(v.z, v.w)));
    }
    for (uint64_t i = n4 * 4 + (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
        lo = min(lo, lat[i]);
        hi = max(hi, lat[i]);
    }
    const uint32_t lane = threadIdx.x & 63;
    lo = wave_min_u32(lo, lane);
    hi = wave_max_u32(hi, lane);
    __shared__ uint32_t part[8];
    if (lane == 0) {
        part[threadIdx.x >> 6] = lo;
        part[4 + (threadIdx.x >> 6)] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) {
            lo = min(lo, part[w]);
            hi = max(hi, part[4 + w]);
        }
        atomicMin(red, (unsigned long long)lo);
        atomicMax(red + 1, (unsigned long long)hi);
    }
}

// the map of the prepared graph, on the host and on the device: once per prepare
static shd_status build_map(shd_ctx* ctx) {
    PreparedGraph& P = ctx->prep;
    hipStream_t s = ctx->stream;
    const uint64_t E = P.es.size();
    P.upd.built = false;   // until the device has it
    if (P.mode == SHD_ROUTE_DIRECT) {   // the edge arrays are patched by edge index: the stamps alone
        P.upd.stamp.assign(E, 0);
        P.upd.call = 0;
    } else {
        edge_slots_build(P.V, E, P.es.data(), P.ed.data(), P.directed, P.upd);
        P.upd.built = false;   // (edge_slots_build set it)
        P.upd.sum_lat = 0;
        for (uint64_t i = 0; i < E; ++i)
            if (P.es[i] != P.ed[i]) P.upd.sum_lat += P.el[i];
        P.upd_col.assign(P.V, -1);
        for (uint32_t j = 0; j < P.n_used; ++j) P.upd_col[P.used[j]] = (int32_t)j;
        std::vector<uint32_t> pairs(2 * std::max<uint64_t>(E, 1), kNoSlot);
        auto send = [&](DevBuf& b, const std::vector<uint32_t>* pi) -> shd_status {
            std::vector<uint32_t> start;
            if (pi) start = edge_copy_starts(P.upd.off, *pi);
            for (uint64_t i = 0; i < E; ++i) {
                const uint32_t f = P.upd.fwd[i], r = P.upd.rev[i];
                const uint32_t a = P.es[i], b2 = P.ed[i];
                pairs[2 * i] = f == kNoSlot || !pi ? f : start[a] + (f - P.upd.off[a]);
                pairs[2 * i + 1] = r == kNoSlot || !pi ? r : start[b2] + (r - P.upd.off[b2]);
            }
            return upload(b, pairs, s);
        };
        SHD_TRY(send(ctx->g_umap, nullptr));
        if (P.reordered) SHD_TRY(send(ctx->g_umap_r, &P.pi_r));
        if (P.spread) SHD_TRY(send(ctx->g_umap_s, &P.pi_s));
        SHD_HIP(hipStreamSynchronize(s));   // `pairs` is reused and freed
        SHD_TRY(ctx->g_ured.ensure(16));
    }
    P.upd.built = true;
    return SHD_OK;
}

// prepare again from the context's own host copies (a wide graph has no resident arc arrays to
// patch).  The map goes with the old prepare, as after any prepare: the new one decides afresh
// which relabelled copies exist, and the next update maps their slots too.
static shd_status prepare_again(shd_ctx* ctx, shd_error* err) {
    PreparedGraph& P = ctx->prep;
    const std::vector<uint32_t> es = P.es, ed = P.ed, used = P.used, ids = P.node_ids;
    const std::vector<uint64_t> el = P.el;
    const std::vector<float> ep = P.ep;
    shd_graph g{};
    g.n_nodes = P.V;
    g.n_edges = (uint32_t)es.size();
    g.edge_src = es.data();
    g.edge_dst = ed.data();
    g.edge_latency_ns = el.data();
    g.edge_packet_loss = ep.data();
    g.node_ids = ids.data();
    g.directed = P.directed;
    return routing_prepare_impl(ctx, &g, used.data(), (uint32_t)used.size(), P.mode, err);
}

static shd_status update_edges(shd_ctx* ctx, uint64_t n, const uint32_t* edge_index, const uint64_t* latency_ns,
                               const float* packet_loss, shd_error* err) {
    PreparedGraph& P = ctx->prep;
    hipStream_t s = ctx->stream;
    if (!edge_updates_valid(n, P.es.size(), edge_index, latency_ns, packet_loss)) return SHD_ERR_INVALID;
    const bool direct = P.mode == SHD_ROUTE_DIRECT;
    // The u32 arc arrays of shortest mode hold no latency of 2^32 - 1 ns or more: a graph that is
    // wide, or that one of these entries makes wide, gets its host copies changed (in the call's
    // order, so the last entry wins) and is prepared again.  That is decided before the map is
    // built, since the map goes with the old prepare.  Direct mode keeps u64 edge latencies.
    bool wide = !direct && !P.narrow_arcs;
    if (!direct && !wide)
        for (uint64_t i = 0; i < n && !wide; ++i)
            wide = latency_ns[i] >= kLat32Inf && P.es[edge_index[i]] != P.ed[edge_index[i]];
    if (wide) {
        for (uint64_t i = 0; i < n; ++i) {
            P.el[edge_index[i]] = latency_ns[i];
            P.ep[edge_index[i]] = packet_loss[i];
        }
        ctx->upd_reprepares++;
        return prepare_again(ctx, err);
    }
    if (!P.upd.built) SHD_TRY(build_map(ctx));
    const std::vector<uint64_t> keep = edge_updates_unique(P.upd, n, edge_index);
    // the host copies first (the wide path rebuilds its CSR from them on every run)
    std::vector<uint4> rec(keep.size());
    uint64_t n_arc = 0, n_diag = keep.size();   // arc records from the front, diagonal ones from the back
    for (const uint64_t i : keep) {
        const uint32_t e = edge_index[i];
        const uint64_t l = latency_ns[i];
        const float p = packet_loss[i];
        const bool loop = P.es[e] == P.ed[e];
        if (!loop && !direct) P.upd.sum_lat += l - P.el[e];   // (the mean of the arc arrays: shortest mode's)
        P.el[e] = l;
        P.ep[e] = p;
        if (direct) {
            rec[n_arc++] = make_uint4(e, __builtin_bit_cast(uint32_t, p), (uint32_t)l, (uint32_t)(l >> 32));
        } else if (!loop) {
            rec[n_arc++] = make_uint4(e, __builtin_bit_cast(uint32_t, p + 0.0f), (uint32_t)l, 0u);
        } else if (P.upd_col[P.es[e]] >= 0) {   // the diagonal entry of a used node
            rec[--n_diag] = make_uint4((uint32_t)P.upd_col[P.es[e]], __builtin_bit_cast(uint32_t, p), (uint32_t)l,
                                       (uint32_t)(l >> 32));
        }
    }
    const uint64_t diag0 = n_diag, n_rec = n_arc + (keep.size() - diag0);
    if (diag0 != n_arc) std::copy(rec.begin() + diag0, rec.end(), rec.begin() + n_arc);   // close the gap
    n_diag = keep.size() - diag0;
    if (n_rec == 0) return SHD_OK;   // self-loops of unused nodes only
    SHD_TRY(ctx->g_urec.ensure(n_rec * 16));
    SHD_HIP(hipMemcpyAsync(ctx->g_urec.p, rec.data(), n_rec * 16, hipMemcpyHostToDevice, s));
    if (direct) {
        edge_patch_direct<<<div_up(n_rec, 256), 256, 0, s>>>(ctx->g_urec.as<uint4>(), n_rec, ctx->d_el.as<uint64_t>(),
                                                              ctx->d_ep.as<float>());
        SHD_HIP(hipGetLastError());
        return wait_stream(ctx, s);
    }
    PatchArrays a{};
    a.map = ctx->g_umap.as<uint2>();
    a.map_r = P.reordered ? ctx->g_umap_r.as<uint2>() : nullptr;
    a.map_s = P.spread ? ctx->g_umap_s.as<uint2>() : nullptr;
    a.dst = ctx->g_dst.as<uint32_t>();
    a.lat = ctx->g_lat.as<uint32_t>();
    a.aux = ctx->g_aux.as<float>();
    a.arc16 = ctx->g_arc16.as<uint4>();
    a.arc8 = ctx->g_arc8.as<uint2>();
    a.aq = ctx->g_aq.as<float>();
    a.arc8r = ctx->g_arc8r.as<uint2>();
    a.aqr = ctx->g_aqr.as<float>();
    a.arc16s = ctx->g_arc16s.as<uint4>();
    a.diag_lat = ctx->g_diag_lat.as<uint64_t>();
    a.diag_loss = ctx->g_diag_loss.as<float>();
    a.red = ctx->g_ured.as<unsigned long long>();
    edge_patch<<<div_up(2 * n_arc + n_diag, 256), 256, 0, s>>>(ctx->g_urec.as<uint4>(), n_arc, n_diag, a);
    SHD_HIP(hipGetLastError());
    if (n_arc == 0) return wait_stream(ctx, s);   // the diagonal alone: no arc changed
    // the builds read these from PreparedGraph, exact: the prune's bin shift and the padded
    // kernels' overflow guard from the largest arc, the bucket widths from the smallest and the mean
    // at most 128 workgroups: every one ends in an atomic pair on the same two words
    const uint32_t grid = (uint32_t)std::min<uint64_t>(128, (P.arcs / 4 + 255) / 256);
    lat_minmax<<<grid ? grid : 1, 256, 0, s>>>(a.lat, P.arcs, a.red);
    SHD_HIP(hipGetLastError());
    SHD_TRY(readback(ctx, s, 16, a.red, 16));
    const uint64_t lo = ctx->h_pin[16], hi = ctx->h_pin[17];
    P.max_arc_lat = hi;
    P.min_arc_lat = (uint32_t)std::min<uint64_t>(kLat32Inf - 1, std::max<uint64_t>(lo, 1));
    // prepare's definition: the edge latencies' sum, each non-loop edge once, over the arc count
    P.mean_arc_lat = (uint32_t)std::min<double>(kLat32Inf - 1, (double)P.upd.sum_lat / (double)P.arcs);
    P.pruned_arcs = 0;   // the kept-arc counts pick the lane-group width: counted again by the next build
    P.tight_arcs = 0;
    return SHD_OK;
}

}  // namespace shd

using namespace shd;

extern "C" shd_status shd_routing_update_edges(shd_ctx* ctx, uint64_t n, const uint32_t* edge_index,
                                               const uint64_t* latency_ns, const float* packet_loss,
                                               shd_error* err) {
    if (!ctx) return SHD_ERR_INVALID;
    if (err) *err = shd_error{SHD_OK, 0, 0};
    if (!ctx->prep.ready) return SHD_ERR_STATE;
    if (n == 0) return SHD_OK;
    SHD_HIP(hipSetDevice(ctx->device));
    return update_edges(ctx, n, edge_index, latency_ns, packet_loss, err);
}
