// The global-label SSSP engine (routing_priv.h has the overview): sssp_row (sssp_row.h) with the
// labels in global memory, for graphs whose labels leave the LDS (C4).
#include <cstdio>

#include "sssp_row.h"

namespace shd {

// Kernel 1b: labels in global memory, for graphs whose labels do not fit the LDS (C4: 50k
// nodes = 400 KB per source).  A persistent grid of slots: slot b owns the label array
// glab[b*V, (b+1)*V), starts at row row_begin + b and then takes the next unclaimed row from
// row_ctr; the bitmap and the queues stay in LDS (V/8 bytes).
// (Two slots per CU need <= 128 VGPRs at BLOCK = 512; the kernel sits at exactly 128, so any
// added live value halves its residency -- check .vgpr_count after changes to sssp_row.  A
// waves-per-EU launch bound keeps the count but schedules worse: C4 rows 0-4095 17.4 -> 18.5 ms.)
// The expansion is always edge-parallel (expand_flat8 with FASTG, expand_flat without), so G and R
// reach no code here any more and only G = 4, R = 4 is instantiated.  The template list stays
// until sssp_row is split into an LDS and a global function.
template <int BLOCK, int G, int R, bool FASTG>
__global__ __launch_bounds__(BLOCK) void sssp_global_group(
    const uint32_t* __restrict__ abeg, const uint32_t* __restrict__ aend,
    const uint4* __restrict__ arcs, uint32_t V, const uint32_t* __restrict__ used,
    uint32_t n_used, uint32_t row_begin, uint32_t row_end, const uint64_t* __restrict__ diag_lat,
    const float* __restrict__ diag_loss, uint64_t* __restrict__ out_lat,
    float* __restrict__ out_loss, uint32_t* __restrict__ flags,
    unsigned long long* __restrict__ unreach, uint32_t delta,
    unsigned long long* __restrict__ stats, uint64_t* __restrict__ glab, uint32_t use_bkt, uint32_t use_wmin,
    uint32_t* __restrict__ nh_out, uint32_t* __restrict__ gpred, const uint2* __restrict__ arcs8,
    const float* __restrict__ aq, uint32_t kl, uint32_t* __restrict__ row_ctr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t s_next;
    const uint32_t W = (V + 31) >> 5;
    uint32_t* bits = reinterpret_cast<uint32_t*>(smem);
    uint32_t* ctl = bits + W;
    uint32_t* wq = ctl + 4;
    uint32_t* flat = wq + (BLOCK / 64) * kQStride;   // per-wave scratch of expand_flat / expand_flat8
    uint8_t* bkt = use_bkt ? reinterpret_cast<uint8_t*>(wq + (BLOCK / 64) * (kQStride + kFlatWords)) : nullptr;
    uint64_t* lab = glab + (size_t)blockIdx.x * V;
    // FASTG with use_wmin: the per-word minimum keys (W words) after the bucket bytes
    uint32_t* wmin = FASTG && use_bkt && use_wmin ? reinterpret_cast<uint32_t*>(bkt + ((V + 3) / 4) * 4) : nullptr;
    // kl > 0 (FASTG, no next hops): the labels of nodes [0, kl) in LDS after the bucket bytes (and wmin)
    uint64_t* llab = nullptr;
    if (FASTG && kl) {
        const unsigned char* end = wmin ? reinterpret_cast<unsigned char*>(wmin + W) : bkt + ((V + 3) / 4) * 4;
        const size_t at = ((size_t)(end - smem) + 7) & ~(size_t)7;
        llab = reinterpret_cast<uint64_t*>(smem + at);
    }
    // row_ctr (zeroed before the launch): after its first row a slot takes the next unclaimed row,
    // so the grid drains together instead of waiting for the slot whose fixed rows ran longest
    uint32_t row = row_begin + blockIdx.x;
    while (row < row_end) {
        sssp_row<BLOCK, G, R, false, true, 0, FASTG>(lab, bits, ctl, wq, nullptr, abeg, aend, arcs, V, used,
                                           n_used, row, (size_t)(row - row_begin) * n_used,
                                           diag_lat, diag_loss, out_lat, out_loss, flags, unreach,
                                           delta, stats, nullptr, 0, bkt, flat, nh_out,
                                           gpred ? gpred + (size_t)blockIdx.x * V : nullptr, 0u, arcs8, aq, nullptr,
                                           llab, FASTG ? kl : 0u, wmin);
        __syncthreads();   // the next row re-initialises labels and bitmap
        if (threadIdx.x == 0) s_next = row_begin + gridDim.x + atomicAdd(row_ctr, 1u);
        __syncthreads();
        row = s_next;
    }
}

template <int BLOCK, int G>
static void launch_global(shd_ctx* ctx, const ArcView& A, uint32_t rb, uint32_t re, uint32_t grid,
                          size_t lds, uint64_t* d_lat, float* d_loss, uint32_t delta, uint32_t use_bkt,
                          uint32_t use_wmin, uint32_t kl) {
    PreparedGraph& P = ctx->prep;
    constexpr int R = G >= 32 ? 2 : 4;
    // the events ride on the dispatch packet: the kernel's own duration, no marker gaps
    // bucket bytes + delta (C4's configuration): the kernel without the other paths
    const bool fast = use_bkt && delta != kLat32Inf;
    auto kern = fast ? sssp_global_group<BLOCK, G, R, true> : sssp_global_group<BLOCK, G, R, false>;
    // the locality-ordered copy (prepare_reordered) when it exists and no next hops are asked for
    const bool ro = fast && P.reordered && !ctx->nh_out;
    const uint32_t* beg = ro ? ctx->g_offr.as<uint32_t>() : A.beg;
    const uint32_t* end = ro ? ctx->g_offr.as<uint32_t>() + 1 : A.end;
    const uint32_t* usedp = ro ? ctx->g_usedr.as<uint32_t>() : ctx->g_used.as<uint32_t>();
    const uint2* a8 = ro ? ctx->g_arc8r.as<uint2>() : ctx->g_arc8.as<uint2>();
    const float* aqp = ro ? ctx->g_aqr.as<float>() : ctx->g_aq.as<float>();
    // dynamic row claiming: the counter the slots take their next row from
    uint32_t* row_ctr = reinterpret_cast<uint32_t*>(ctx->g_flags.as<char>() + 48);
    (void)hipMemsetAsync(row_ctr, 0, 4, ctx->stream);
    hipExtLaunchKernelGGL(
        kern, dim3(grid), dim3(BLOCK), (uint32_t)lds, ctx->stream,
        ctx->time_now ? ctx->ev[2] : nullptr, ctx->time_now ? ctx->ev[3] : nullptr, 0u,
        beg, end, A.arcs, P.V, usedp, P.n_used, rb, re,
        (const uint64_t*)ctx->g_diag_lat.as<uint64_t>(), (const float*)ctx->g_diag_loss.as<float>(), d_lat, d_loss,
        ctx->g_flags.as<uint32_t>(), reinterpret_cast<unsigned long long*>(ctx->g_flags.as<char>() + 16), delta,
        ctx->stats_on ? reinterpret_cast<unsigned long long*>(ctx->g_flags.as<char>() + 32) : nullptr,
        ctx->g_glab.as<uint64_t>(), use_bkt, use_wmin, ctx->nh_out,
        ctx->nh_out ? ctx->g_pred.as<uint32_t>() : nullptr, a8, aqp, ro ? kl : 0u, row_ctr);
}

// Kernel 1b driver: labels in global memory (graphs whose labels exceed the LDS).
shd_status run_sssp_global(shd_ctx* ctx, const ArcView& A, uint32_t rb, uint32_t re, uint64_t* d_lat,
                           float* d_loss, uint32_t delta) {
    PreparedGraph& P = ctx->prep;
    constexpr uint32_t BLOCK = 512;   // a 1024-thread single slot per CU: rows 0-4095 23.5 vs 19.1 ms
    const uint32_t W = (P.V + 31) / 32;
    // bitmap + control + per-wave queues and edge-parallel scratch (+ delta-stepping: one bucket
    // byte per node, when it fits beside the bitmap; else the sweeps read the active nodes' global
    // labels)
    size_t lds = (size_t)W * 4 + 16 + (BLOCK / 64) * (kQStride + kFlatWords) * 4;
    if (lds > ctx->max_lds) return SHD_ERR_INVALID;   // bitmap of > ~1.2M nodes
    const size_t lds_bkt = lds + ((size_t)P.V + 3) / 4 * 4;
    const uint32_t use_bkt = delta != kLat32Inf && lds_bkt <= ctx->max_lds;
    if (use_bkt) lds = lds_bkt;
    // the bucket-byte kernel (FASTG) keeps a per-word minimum key beside the bitmap
    uint32_t use_wmin = 0;
    if (use_bkt && lds + (size_t)W * 4 <= ctx->max_lds) {
        lds += (size_t)W * 4;
        use_wmin = 1;
    }
    const uint32_t per_cu = std::max<uint32_t>(1, ctx->knobs.get(K_SSSP_SLOTS, 2));
    // labels of the first kl nodes (locality order: highest degree first) in the LDS left over by
    // per_cu slots per CU: their relaxations take LDS atomics instead of memory-side ones
    uint32_t kl = 0;
    if (use_bkt && P.reordered && !ctx->nh_out) {
        const size_t room = ctx->max_lds / per_cu;
        if (room > lds + 64) kl = std::min<uint32_t>(std::min<uint32_t>(P.V, P.lds_labels), (uint32_t)((room - lds - 16) / 8)) & ~63u;
        if (kl) lds = ((lds + 7) & ~(size_t)7) + (size_t)kl * 8;
    }
    const uint32_t slots = (uint32_t)ctx->n_cu * per_cu;
    const uint32_t reserve = std::max(ctx->slot_reserve, ctx->knobs.get(K_SSSP_RESERVE, 0));   // env: tools/overlap_probe.py
    const uint32_t grid = std::min<uint32_t>(re - rb, slots - std::min(reserve, slots / 2));
    SHD_TRY(ctx->g_glab.ensure((size_t)grid * P.V * 8));
    if (ctx->nh_out) SHD_TRY(ctx->g_pred.ensure((size_t)grid * P.V * 4));
    // (no group width here: the expansion is edge-parallel, see sssp_global_group)
    launch_global<BLOCK, 4>(ctx, A, rb, re, grid, lds, d_lat, d_loss, delta, use_bkt, use_wmin, kl);
    SHD_HIP(hipGetLastError());
    if (ctx->stats_on) {
        unsigned long long st[2];
        SHD_HIP(hipMemcpyAsync(st, ctx->g_flags.as<char>() + 32, 16, hipMemcpyDeviceToHost, ctx->stream));
        SHD_HIP(hipStreamSynchronize(ctx->stream));
        std::fprintf(stderr, "shd_sssp_global: rows=%u slots=%u delta=%u expanded=%llu (%.2f per node) "
                     "sweeps=%llu (%.1f per row)\n", re - rb, grid, delta, st[0],
                     (double)st[0] / ((double)(re - rb) * P.V), st[1], (double)st[1] / (re - rb));
    }
    return SHD_OK;
}

int sssp_global_vgprs() {
    hipFuncAttributes at{};
    const void* f = reinterpret_cast<const void*>(&sssp_global_group<512, 4, 4, true>);
    return hipFuncGetAttributes(&at, f) == hipSuccess ? at.numRegs : -1;
}

}  // namespace shd

#ifdef SHD_SSSP_PROF   // tools/c4_prof.py (c4)
extern "C" int shd_debug_sssp_global_prof(unsigned long long* out, int reset) { return shd::sssp_prof_read(out, reset); }
#endif
