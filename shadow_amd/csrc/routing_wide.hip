// The routing build's two paths without packed u32 labels (routing_priv.h has the overview): the
// u64 "wide" rerun of a build whose path latencies leave 32 bits, and the direct-path mode.
#include "routing_priv.h"

namespace shd {

// ------------------------------------------------------------------------------------------
// Kernel 2 (wide fallback): u64 latencies, labels in global memory, pull-form Jacobi rounds
// over in-arcs.  Used only when some path latency reaches 2^32-1 ns (or V exceeds the LDS).
// One launch = one round for a batch of sources; grid (ceil(V/256), n_src).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sssp_wide_round(
    const uint32_t* __restrict__ in_off, const uint32_t* __restrict__ in_src,
    const uint64_t* __restrict__ in_lat, const float* __restrict__ in_q, uint32_t V,
    const uint64_t* __restrict__ a_lat, const float* __restrict__ a_loss,
    uint64_t* __restrict__ b_lat, float* __restrict__ b_loss, uint32_t* __restrict__ changed,
    uint32_t* __restrict__ flags) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    const size_t s = blockIdx.y;
    if (v >= V) return;
    const uint64_t* al = a_lat + s * V;
    const float* ap = a_loss + s * V;
    uint64_t bl = al[v];
    float bp = ap[v];
    bool ch = false;
    for (uint32_t k = in_off[v]; k < in_off[v + 1]; ++k) {
        const uint32_t u = in_src[k];
        const uint64_t lu = al[u];
        if (lu == ~0ull) continue;
        const uint64_t cl = lu + in_lat[k];
        if (cl < lu || cl == ~0ull) {
            atomicOr(&flags[1], 1u);  // exceeds u64: LATENCY_OVERFLOW
            continue;
        }
        const float cp = fold_q(one_minus(ap[u]), in_q[k]);
        if (cl < bl || (cl == bl && cp < bp)) {
            bl = cl;
            bp = cp;
            ch = true;
        }
    }
    b_lat[s * V + v] = bl;
    b_loss[s * V + v] = bp;
    if (ch) changed[0] = 1;
}

__global__ void wide_init(uint64_t* lat, float* loss, uint32_t V, const uint32_t* used,
                          uint32_t row0) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    const size_t s = blockIdx.y;
    if (v >= V) return;
    const bool is_src = used[row0 + s] == v;
    lat[s * V + v] = is_src ? 0ull : ~0ull;
    loss[s * V + v] = 0.0f;
}

__global__ void wide_emit(const uint64_t* __restrict__ lat, const float* __restrict__ loss,
                          uint32_t V, const uint32_t* __restrict__ used, uint32_t n_used,
                          uint32_t row0, uint32_t out_row0, const uint64_t* __restrict__ diag_lat,
                          const float* __restrict__ diag_loss, uint64_t* __restrict__ out_lat,
                          float* __restrict__ out_loss, unsigned long long* __restrict__ unreach) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    const size_t s = blockIdx.y;
    if (j >= n_used) return;
    const uint32_t row = row0 + (uint32_t)s;
    uint64_t l;
    float p;
    if (j == row) {
        l = diag_lat[j];
        p = diag_loss[j];
    } else {
        l = lat[s * V + used[j]];
        p = loss[s * V + used[j]];
        if (l == ~0ull) atomicMin(unreach, (unsigned long long)((uint64_t)row * n_used + j));
    }
    const size_t o = (size_t)(out_row0 + s) * n_used + j;
    out_lat[o] = l;
    out_loss[o] = p;
}

// next hops on the wide path: pred(v) = lowest in-neighbour u whose final label extended by
// the arc equals v's label bit for bit (see sssp_row), then the walk back to the source
__global__ void wide_pred(const uint32_t* __restrict__ in_off, const uint32_t* __restrict__ in_src,
                          const uint64_t* __restrict__ in_lat, const float* __restrict__ in_q, uint32_t V,
                          const uint64_t* __restrict__ la, const float* __restrict__ pa,
                          const uint32_t* __restrict__ used, uint32_t row0, uint32_t* __restrict__ pred) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    const size_t s = blockIdx.y;
    if (v >= V) return;
    const uint64_t* al = la + s * V;
    const float* ap = pa + s * V;
    uint32_t best = 0xFFFFFFFFu;
    const uint64_t lv = al[v];
    if (v != used[row0 + s] && lv != ~0ull) {
        const uint32_t pv = __float_as_uint(ap[v]);
        for (uint32_t k = in_off[v]; k < in_off[v + 1]; ++k) {
            const uint32_t u = in_src[k];
            const uint64_t lu = al[u];
            if (u == v || u >= best || lu == ~0ull) continue;
            const uint64_t cl = lu + in_lat[k];
            if (cl < lu || cl != lv) continue;
            if (__float_as_uint(fold_q(one_minus(ap[u]), in_q[k])) == pv) best = u;
        }
    }
    pred[s * V + v] = best;
}

__global__ void wide_next_hop(const uint32_t* __restrict__ pred, uint32_t V, const uint32_t* __restrict__ used,
                              uint32_t n_used, uint32_t row0, uint32_t out_row0, uint32_t* __restrict__ out) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    const size_t s = blockIdx.y;
    if (j >= n_used) return;
    const uint32_t src = used[row0 + s], v = used[j];
    const uint32_t* pr = pred + s * V;
    uint32_t nh = 0xFFFFFFFFu;
    if (v == src) {
        nh = src;
    } else {
        uint32_t w = v, pw = pr[w];
        for (uint32_t hop = 0; hop < V && pw != src && pw != 0xFFFFFFFFu; ++hop) {
            w = pw;
            pw = pr[w];
        }
        if (pw == src) nh = w;
    }
    out[(size_t)(out_row0 + s) * n_used + j] = nh;
}

__global__ void direct_next_hop(const uint32_t* __restrict__ used, uint32_t n_used, uint32_t rb, uint32_t rows,
                                uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (uint64_t)rows * n_used) out[i] = used[i % n_used];   // the one edge's far end (graph/mod.rs:232-254)
    (void)rb;
}

__global__ void arcs_q(const float* __restrict__ loss, float* __restrict__ q, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) q[i] = one_minus(loss[i]);
}

// ------------------------------------------------------------------------------------------
// Direct-path mode: count edges per ordered used pair, keep the edge's raw (lat, loss);
// the first pair (src-major in `used` order) without exactly one edge is the error.
// ------------------------------------------------------------------------------------------
__global__ void direct_scatter(const uint32_t* __restrict__ es, const uint32_t* __restrict__ ed,
                               const uint64_t* __restrict__ el, const float* __restrict__ ep,
                               uint32_t E, int directed, const int32_t* __restrict__ col,
                               uint32_t n_used, uint32_t* __restrict__ cnt,
                               uint64_t* __restrict__ tl, float* __restrict__ tp) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= E) return;
    const int32_t a = col[es[i]], b = col[ed[i]];
    if (a < 0 || b < 0) return;
    size_t c = (size_t)a * n_used + b;
    atomicAdd(&cnt[c], 1u);
    tl[c] = el[i];
    tp[c] = ep[i];
    if (!directed && a != b) {
        c = (size_t)b * n_used + a;
        atomicAdd(&cnt[c], 1u);
        tl[c] = el[i];
        tp[c] = ep[i];
    }
}

__global__ void direct_check(const uint32_t* __restrict__ cnt, uint64_t nn,
                             unsigned long long* __restrict__ first_bad) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nn && cnt[i] != 1u) atomicMin(first_bad, (unsigned long long)i);
}

// Wide path: u64 latency, global labels, Jacobi rounds over in-arcs; batches of sources.
shd_status run_wide(shd_ctx* ctx, uint32_t rb, uint32_t re, uint64_t* d_lat, float* d_loss, shd_error* err) {
    PreparedGraph& P = ctx->prep;
    shd_graph g = P.view();
    HostGraph R;
    build_csr(&g, /*reverse=*/true, R);
    hipStream_t s = ctx->stream;
    DevBuf w_off, w_src, w_lat, w_loss, w_q;
    SHD_TRY(upload(w_off, R.off, s));
    SHD_TRY(upload(w_src, R.dst, s));
    SHD_TRY(upload(w_lat, R.lat, s));
    SHD_TRY(upload(w_loss, R.loss, s));
    SHD_TRY(w_q.ensure(std::max<size_t>(R.loss.size(), 1) * 4));
    if (!R.loss.empty())
        arcs_q<<<div_up(R.loss.size(), 256), 256, 0, s>>>(w_loss.as<float>(), w_q.as<float>(), R.loss.size());
    const uint32_t V = R.V, n_used = P.n_used;
    const uint32_t batch = std::max<uint32_t>(
        1, std::min<uint32_t>(re - rb, (uint32_t)((1ull << 30) / (24ull * V))));
    DevBuf la, pa, lb, pb, ch, pr;
    if (ctx->nh_out) SHD_TRY(pr.ensure((size_t)batch * V * 4));
    SHD_TRY(la.ensure((size_t)batch * V * 8));
    SHD_TRY(lb.ensure((size_t)batch * V * 8));
    SHD_TRY(pa.ensure((size_t)batch * V * 4));
    SHD_TRY(pb.ensure((size_t)batch * V * 4));
    SHD_TRY(ch.ensure(4));
    for (uint32_t r0 = rb; r0 < re; r0 += batch) {
        const uint32_t nb = std::min(batch, re - r0);
        dim3 gv(div_up(V, 256), nb);
        wide_init<<<gv, 256, 0, s>>>(la.as<uint64_t>(), pa.as<float>(), V, ctx->g_used.as<uint32_t>(), r0);
        for (;;) {
            SHD_HIP(hipMemsetAsync(ch.p, 0, 4, s));
            sssp_wide_round<<<gv, 256, 0, s>>>(w_off.as<uint32_t>(), w_src.as<uint32_t>(),
                                               w_lat.as<uint64_t>(), w_q.as<float>(), V,
                                               la.as<uint64_t>(), pa.as<float>(), lb.as<uint64_t>(),
                                               pb.as<float>(), ch.as<uint32_t>(), ctx->g_flags.as<uint32_t>());
            uint32_t changed = 0;
            SHD_HIP(hipMemcpyAsync(&changed, ch.p, 4, hipMemcpyDeviceToHost, s));
            SHD_HIP(hipStreamSynchronize(s));
            std::swap(la, lb);
            std::swap(pa, pb);
            if (!changed) break;
        }
        dim3 ge(div_up(n_used, 256), nb);
        if (ctx->nh_out) {
            wide_pred<<<gv, 256, 0, s>>>(w_off.as<uint32_t>(), w_src.as<uint32_t>(), w_lat.as<uint64_t>(),
                                         w_q.as<float>(), V, la.as<uint64_t>(), pa.as<float>(),
                                         ctx->g_used.as<uint32_t>(), r0, pr.as<uint32_t>());
            wide_next_hop<<<ge, 256, 0, s>>>(pr.as<uint32_t>(), V, ctx->g_used.as<uint32_t>(), n_used, r0, r0 - rb,
                                             ctx->nh_out);
        }
        wide_emit<<<ge, 256, 0, s>>>(la.as<uint64_t>(), pa.as<float>(), V, ctx->g_used.as<uint32_t>(),
                                     n_used, r0, r0 - rb, ctx->g_diag_lat.as<uint64_t>(),
                                     ctx->g_diag_loss.as<float>(), d_lat, d_loss,
                                     reinterpret_cast<unsigned long long*>(ctx->g_flags.as<char>() + 16));
    }
    SHD_TRY(read_flags(ctx));
    if ((uint32_t)(ctx->h_pin[0] >> 32)) return set_err(err, SHD_ERR_LATENCY_OVERFLOW, 0, 0);
    ctx->info.wide_latency = 1;
    return check_unreach(ctx, err);
}

shd_status run_direct(shd_ctx* ctx, uint32_t rb, uint32_t re, uint64_t* d_lat, float* d_loss, shd_error* err) {
    PreparedGraph& P = ctx->prep;
    hipStream_t s = ctx->stream;
    const uint32_t n_used = P.n_used;
    const uint64_t nn = (uint64_t)n_used * n_used;
    const uint32_t E = (uint32_t)P.es.size();
    DevBuf cnt, tl, tp;
    SHD_TRY(cnt.ensure(nn * 4));
    SHD_TRY(tl.ensure(nn * 8));
    SHD_TRY(tp.ensure(nn * 4));
    SHD_HIP(hipEventRecord(ctx->ev[2], s));
    SHD_HIP(hipMemsetAsync(cnt.p, 0, nn * 4, s));
    if (E)
        direct_scatter<<<div_up(E, 256), 256, 0, s>>>(
            ctx->d_es.as<uint32_t>(), ctx->d_ed.as<uint32_t>(), ctx->d_el.as<uint64_t>(),
            ctx->d_ep.as<float>(), E, P.directed, ctx->d_col.as<int32_t>(), n_used,
            cnt.as<uint32_t>(), tl.as<uint64_t>(), tp.as<float>());
    auto* bad_d = reinterpret_cast<unsigned long long*>(ctx->g_flags.as<char>() + 16);
    direct_check<<<div_up(nn, 256), 256, 0, s>>>(cnt.as<uint32_t>(), nn, bad_d);
    const size_t rows = re - rb;
    if (ctx->nh_out && rows)
        direct_next_hop<<<div_up((uint64_t)rows * n_used, 256), 256, 0, s>>>(ctx->g_used.as<uint32_t>(), n_used, rb,
                                                                             (uint32_t)rows, ctx->nh_out);
    SHD_HIP(hipMemcpyAsync(d_lat, tl.as<uint64_t>() + (size_t)rb * n_used, rows * n_used * 8,
                           hipMemcpyDeviceToDevice, s));
    SHD_HIP(hipMemcpyAsync(d_loss, tp.as<float>() + (size_t)rb * n_used, rows * n_used * 4,
                           hipMemcpyDeviceToDevice, s));
        unsigned long long bad = 0;
    SHD_HIP(hipMemcpyAsync(&bad, bad_d, 8, hipMemcpyDeviceToHost, s));
    uint32_t c = 0;
    SHD_HIP(hipStreamSynchronize(s));
    if (bad != ~0ull) {
        SHD_HIP(hipMemcpyAsync(&c, cnt.as<uint32_t>() + bad, 4, hipMemcpyDeviceToHost, s));
        SHD_HIP(hipStreamSynchronize(s));
        const uint32_t r = (uint32_t)(bad / n_used), q = (uint32_t)(bad % n_used);
        return set_err(err, c == 0 ? SHD_ERR_NO_EDGE : SHD_ERR_MULTI_EDGE, P.node_ids[P.used[r]],
                       P.node_ids[P.used[q]]);
    }
    return SHD_OK;
}

}  // namespace shd
