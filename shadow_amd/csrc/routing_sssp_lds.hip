// The LDS-label SSSP engine: one workgroup per source row, labels and bitmap in LDS
// (routing_priv.h has the overview).  sssp_lds_group runs sssp_row (sssp_row.h) on plain or padded
// arc lists; sssp_lds_shadow is the fire-and-forget form of the padded-list sweeps, the default
// on pruned dense graphs (C2).  run_sssp picks block size, group width and kernel.
#include <cstdio>

#include "sssp_row.h"

namespace shd {

// Kernel 1: one workgroup per source row, labels (8 B/node) and the arc ranges in LDS.
// PADR = 8, 4: padded arc lists (prune_rows, prune_rows2), relax_node_pad with PADR arcs per lane per step.
// hub_deg: the hub threshold of the unpadded kernels.  The host always passes kHubDeg (the knob
// that swept it is retired) and 0 for `reserved` (once the offset of the retired LDS edge-parallel
// scratch).  Both stay device arguments, hub_deg behind `if (hub_deg)` in sssp_row, because the
// code the compiler makes of sssp_lds_group<1024, 4, 2, false, 0> (C3) depends on them, measured
// against the parent in alternated builds (parent 6.52-6.57 ms): threshold folded in as a constant
// and both arguments gone, 78 instructions fewer, re-laid-out loops, 6.56-6.62 ms; hub_deg back
// without `reserved`, the parent's instruction sequence but for the argument loads, 6.55-6.58;
// the parent's argument list, the parent's code but for two swapped scalar mask pairs, 6.53-6.58
// with nine of ten builds inside the parent's 6.53-6.56.  49 VGPRs in every form.
template <int BLOCK, int G, int R, bool CACHE, int PADR>
__global__ __launch_bounds__(BLOCK) void sssp_lds_group(
    const uint32_t* __restrict__ abeg, const uint32_t* __restrict__ aend,
    const uint4* __restrict__ arcs, uint32_t V, const uint32_t* __restrict__ used,
    uint32_t n_used, uint32_t row_begin, const uint64_t* __restrict__ diag_lat,
    const float* __restrict__ diag_loss, uint64_t* __restrict__ out_lat,
    float* __restrict__ out_loss, uint32_t* __restrict__ flags,
    unsigned long long* __restrict__ unreach, uint32_t delta,
    unsigned long long* __restrict__ stats, const uint32_t* __restrict__ seed_lat,
    uint32_t seed_stride, uint32_t* __restrict__ nh_out, uint32_t lat_guard, uint32_t use_offl,
    uint32_t reserved, uint32_t hub_deg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr uint32_t NW = BLOCK / 64;
    uint64_t* lab = reinterpret_cast<uint64_t*>(smem);   // V labels + 64 per-lane scratch labels
    const uint32_t W = (V + 31) >> 5;
    uint32_t* bits = reinterpret_cast<uint32_t*>(lab + V + 64);
    uint32_t* ctl = bits + W;            // [0] dirty  [1..3] min active latency
    uint32_t* wq = ctl + 4;              // per-wave queue (kQStride node ids)
    // [V] arc range {beg, end}, 8-byte aligned after the queues
    const uint32_t rng_off =
        (((uint32_t)((wq + NW * kQStride) - reinterpret_cast<uint32_t*>(smem)) * 4u) + 7u) & ~7u;
    uint2* rng = reinterpret_cast<uint2*>(smem + rng_off);
    // !CACHE on a plain CSR (aend == abeg + 1): the offsets alone, 4 B/node, in LDS (use_offl);
    // next hops' pred[V] then follows them
    uint32_t* offl = !CACHE && use_offl ? reinterpret_cast<uint32_t*>(smem + rng_off) : nullptr;
    uint32_t* pred = offl ? offl + V + 1 : reinterpret_cast<uint32_t*>(smem + rng_off);
    sssp_row<BLOCK, G, R, CACHE, false, PADR>(lab, bits, ctl, wq, rng, abeg, aend, arcs, V, used, n_used,
                                              row_begin + blockIdx.x, (size_t)blockIdx.x * n_used,
                                              diag_lat, diag_loss, out_lat, out_loss, flags, unreach,
                                              delta, stats, seed_lat, seed_stride, nullptr, nullptr, nh_out,
                                              pred, lat_guard, nullptr, nullptr, offl, nullptr, 0u, nullptr,
                                              hub_deg);
}

// ------------------------------------------------------------------------------------------
// Kernel 1s: the padded-list delta sweeps with fire-and-forget label atomics (SHD_SSSP_SHADOW,
// default on).  relax_node_pad spends about half its instructions on the value ds_min_rtn_u64
// returns -- the wait, the 64-bit compares, the bitmap atomicOr and the floor minimum per improved
// slot -- only to learn which targets became active.  Here the atomics return nothing, and the
// active set is read back from the labels themselves: thread t owns the nodes t + i * BLOCK and
// keeps, in registers, the label each was last queued with (its shadow, +inf at first).  Once per
// sweep it reads its labels (conflict-free ds_read_b64): a node is active iff label != shadow,
// selected iff also latency <= thr; a selected node is queued and its shadow set to the label
// read.  The expansion re-reads the label; if a relaxation lowered it between the scan and the
// expansion the next scan finds label != shadow and expands the node once more (redundant, never
// wrong: the fixed point is order-free).
// Floor of the next sweep, without knowing what improved: every label written in sweep k is at
// least lo_k + amin (amin <= every arc latency; the expanded labels are >= lo_k), and every active
// node the scan left is >= m_unsel_k, so lo_{k+1} = min(m_unsel_k, lo_k + amin if anything was
// selected) bounds every key active after the sweep from below.  Nothing selected and nothing
// left: the row is done.  A floor that is too low only selects less (the selection has no lower
// bound), so the worst a wrong floor does is cost sweeps; the sweep cap turns even that into the
// overflow flag and the u64 rerun instead of a spinning workgroup.
// LDS layout: sssp_lds_group's (the bitmap words stay unused).
// ------------------------------------------------------------------------------------------
constexpr uint32_t kShadowN = 4;   // owned nodes per thread: V <= kShadowN x BLOCK (8 VGPRs of shadows)

template <int G, int R>
__device__ __forceinline__ void relax_node_pad_nr(uint32_t u, uint32_t gl, uint64_t* lab, const uint2* rng,
                                                  const uint4* __restrict__ arcs, uint32_t lat_guard, bool& ovf) {
    static_assert(G * R == 32 || G * R == 64, "a padded list holds whole G x R steps");
    const uint64_t ku = lab[u];
    const uint32_t lu = key_lat(ku);
    if (lu > lat_guard) ovf = true;
    const float qu = one_minus(key_loss(ku));
    const uint2 r = rng[u];
    for (uint32_t k0 = r.x; k0 < r.y; k0 += G * R) {
        const uint4* ap = arcs + k0 + gl;
        uint4 a[R];
#pragma unroll
        for (int i = 0; i < R; ++i) a[i] = ap[i * G];
#pragma unroll
        for (int i = 0; i < R; ++i)   // result unused: ds_min_u64, no return path, no wait
            (void)__hip_atomic_fetch_min(&lab[a[i].x], pack_key(lu + a[i].y, fold_q(qu, __uint_as_float(a[i].z))),
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// The wave's queue, NG nodes per step, one step ahead: the next step's node, label, arc range and
// first G x R slots are fetched before this step's atomics go out, so a step's chain of round
// trips (queue, label + range, arcs) runs under the previous step's work instead of after it.
// Nothing waits for the atomics, so the only waits left in a step are the fetches'.  Lists longer
// than one G x R block (few on C2's 32-slot lists) finish in a plain loop of their own.
template <int G, int R>
__device__ __forceinline__ void expand_queue_nr(const uint32_t* q, uint32_t qn, uint32_t grp, uint32_t gl,
                                                uint64_t* lab, const uint2* rng, const uint4* __restrict__ arcs,
                                                uint32_t lat_guard, bool& ovf) {
    constexpr uint32_t NG = 64 / G;
    uint4 a[R], b[R];
    uint32_t lu = 0, k1 = 0, ke = 0, lub = 0, k1b = 0, keb = 0;
    float qu = 0.0f, qub = 0.0f;
    // fetch a queued node's head; false: no node for this group, or an empty list.  The reads are
    // issued either way, from the queue's last node or the first list when there is nothing to
    // fetch: a fetch that is sometimes skipped leaves the count of loads in flight unknown at
    // the next wait, which then has to drain them all
    auto head = [&](uint32_t qi, uint4 (&h)[R], uint32_t& l, float& qf, uint32_t& kn, uint32_t& kend) -> bool {
        const uint32_t u = q[min(qi, qn - 1)];
        const uint64_t ku = lab[u];
        const uint2 r = rng[u];
        const bool live = qi < qn && r.x < r.y;
        l = key_lat(ku);
        if (live && l > lat_guard) ovf = true;
        qf = one_minus(key_loss(ku));
        kn = r.x + G * R;
        kend = r.y;
        const uint4* ap = arcs + (r.x < r.y ? r.x : 0u) + gl;
#pragma unroll
        for (int i = 0; i < R; ++i) h[i] = ap[i * G];
        return live;
    };
    auto relax = [&](const uint4 (&h)[R], uint32_t l, float qf, uint32_t kn, uint32_t kend) {
#pragma unroll
        for (int i = 0; i < R; ++i)   // result unused: ds_min_u64, no return path, no wait
            (void)__hip_atomic_fetch_min(&lab[h[i].x], pack_key(l + h[i].y, fold_q(qf, __uint_as_float(h[i].z))),
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        for (uint32_t k0 = kn; k0 < kend; k0 += G * R) {
            const uint4* ap = arcs + k0 + gl;
            uint4 c[R];
#pragma unroll
            for (int i = 0; i < R; ++i) c[i] = ap[i * G];
#pragma unroll
            for (int i = 0; i < R; ++i)
                (void)__hip_atomic_fetch_min(&lab[c[i].x], pack_key(l + c[i].y, fold_q(qf, __uint_as_float(c[i].z))),
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    };
    // two steps per turn, the two register sets swapping roles (a copy would wait for the fetch);
    // qn >= 1
    bool on = head(grp, a, lu, qu, k1, ke), onb;
    for (uint32_t t = NG;; t += 2 * NG) {   // t: the first queue slot of the step to fetch
        if (t >= qn) {   // wave-uniform
            if (on) relax(a, lu, qu, k1, ke);
            break;
        }
        onb = head(t + grp, b, lub, qub, k1b, keb);
        if (on) relax(a, lu, qu, k1, ke);
        if (t + NG >= qn) {
            if (onb) relax(b, lub, qub, k1b, keb);
            break;
        }
        on = head(t + NG + grp, a, lu, qu, k1, ke);
        if (onb) relax(b, lub, qub, k1b, keb);
    }
}

// The table's row in 16-byte stores, four columns per thread: two for the latencies, one for the
// losses (row_emit writes an 8-byte and a 4-byte one per column), non-temporal as there.  For the
// identity used set with n_used % 4 == 0 and both output rows 16-byte aligned; the caller sends
// every other case, and the next hops, through row_emit.  The diagonal and an unreachable column
// are handled per element, as row_emit does.
typedef uint64_t u64x2_t __attribute__((ext_vector_type(2)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
template <int BLOCK>
__device__ __forceinline__ void row_emit4(const uint64_t* lab, uint32_t n_used, uint32_t row, size_t orow,
                                          const uint64_t* __restrict__ diag_lat, const float* __restrict__ diag_loss,
                                          uint64_t* __restrict__ out_lat, float* __restrict__ out_loss,
                                          unsigned long long* __restrict__ unreach) {
    for (uint32_t j0 = 4u * threadIdx.x; j0 < n_used; j0 += 4u * BLOCK) {
        uint64_t k[4], l[4];
        float p[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) k[i] = ld_lab<false>(&lab[j0 + i]);
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t j = j0 + i;
            if (j == row) {
                l[i] = diag_lat[j];
                p[i] = diag_loss[j];
            } else if (k[i] == kKeyInf) {
                atomicMin(unreach, (unsigned long long)((uint64_t)row * n_used + j));
                l[i] = ~0ull;
                p[i] = 0.0f;
            } else {
                l[i] = key_lat(k[i]);
                p[i] = key_loss(k[i]);
            }
        }
        u64x2_t* ol = reinterpret_cast<u64x2_t*>(out_lat + orow + j0);
        __builtin_nontemporal_store(u64x2_t{l[0], l[1]}, ol);
        __builtin_nontemporal_store(u64x2_t{l[2], l[3]}, ol + 1);
        __builtin_nontemporal_store(f32x4_t{p[0], p[1], p[2], p[3]}, reinterpret_cast<f32x4_t*>(out_loss + orow + j0));
    }
}

template <int BLOCK, int G, int PADR>
__device__ __forceinline__ void sssp_row_shadow(
    uint64_t* lab, uint32_t* ctl, uint32_t* wq, uint2* rng, const uint32_t* __restrict__ abeg,
    const uint32_t* __restrict__ aend, const uint4* __restrict__ arcs, uint32_t V,
    const uint32_t* __restrict__ used, uint32_t n_used, uint32_t row, size_t orow,
    const uint64_t* __restrict__ diag_lat, const float* __restrict__ diag_loss, uint64_t* __restrict__ out_lat,
    float* __restrict__ out_loss, uint32_t* __restrict__ flags, unsigned long long* __restrict__ unreach,
    uint32_t delta, uint32_t amin, unsigned long long* __restrict__ stats, uint32_t* nh_out, uint32_t* pred,
    uint32_t lat_guard) {
    constexpr uint32_t NG = 64 / G;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t grp = lane / G, gl = lane % G;
    uint32_t* q = wq + wave * kQStride;
    const uint32_t src = used ? used[row] : row;
    // the arc ranges, four nodes per 16-byte load when both range arrays are 16-byte aligned (the
    // prune's are when V % 4 == 0); every row reads the same arrays
    const bool rng16 = ((reinterpret_cast<uintptr_t>(abeg) | reinterpret_cast<uintptr_t>(aend)) & 15u) == 0;
    const uint32_t v16 = rng16 ? V & ~3u : 0u;
    for (uint32_t v = 4u * tid; v < v16; v += 4u * BLOCK) {
        const uint4 b = *reinterpret_cast<const uint4*>(abeg + v), e = *reinterpret_cast<const uint4*>(aend + v);
        rng[v] = make_uint2(b.x, e.x);
        rng[v + 1] = make_uint2(b.y, e.y);
        rng[v + 2] = make_uint2(b.z, e.z);
        rng[v + 3] = make_uint2(b.w, e.w);
    }
    for (uint32_t v = v16 + tid; v < V; v += BLOCK) rng[v] = make_uint2(abeg[v], aend[v]);
    // PathProperties::default() = (0 ns, 0.0)
    for (uint32_t v = tid; v < V; v += BLOCK) lab[v] = v == src ? 0ull : kKeyInf;
    if (tid < 64) lab[V + tid] = 0;   // scratch labels: no candidate improves them
    if (tid == 0) ctl[1] = ctl[2] = ctl[3] = kLat32Inf;
    __syncthreads();
    uint64_t sh[kShadowN];
#pragma unroll
    for (uint32_t i = 0; i < kShadowN; ++i) sh[i] = kKeyInf;
    bool ovf = false;
    uint32_t expanded = 0, sweeps = 0, slot = 0, lo = 0;
    // one real and one empty sweep per node, and slack: a row that gets here (many re-expansions
    // under a delta far above amin, or a mistake in the rule above) leaves through the overflow
    // flag and the u64 path -- slow and correct, never a spinning workgroup
    const uint32_t cap = 2 * V + 64;
    for (;;) {
        // one-barrier sweeps over three rotating accumulators, as in sssp_row
        if (sweeps != 0) {
            lo = ctl[1 + (slot + 2) % 3];
            if (lo == kLat32Inf) break;   // nothing selected, nothing left
            if (sweeps >= cap) {
                ovf = true;
                break;
            }
        }
        if (tid == 0) ctl[1 + (slot + 1) % 3] = kLat32Inf;
        const uint32_t thr = (uint32_t)min((uint64_t)lo + delta, (uint64_t)kLat32Inf - 1);
        uint32_t mnext = kLat32Inf, selm = 0;
        // (no branch around a read -- past V a lane reads its scratch label and drops it -- so the
        // kShadowN reads are in flight together)
        uint64_t l[kShadowN];
#pragma unroll
        for (uint32_t i = 0; i < kShadowN; ++i) {
            const uint32_t v = tid + i * BLOCK;
            l[i] = ld_lab<false>(&lab[v < V ? v : V + lane]);
        }
#pragma unroll
        for (uint32_t i = 0; i < kShadowN; ++i) {
            const bool act = tid + i * BLOCK < V && l[i] != sh[i], sel = act && key_lat(l[i]) <= thr;
            sh[i] = sel ? l[i] : sh[i];
            selm |= (sel ? 1u : 0u) << i;
            mnext = min(mnext, act && !sel ? key_lat(l[i]) : kLat32Inf);
        }
        uint32_t qn = 0;   // wave-uniform queue length
        bool any = false;  // wave-uniform: this wave selected a node
        auto flush = [&]() {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            expanded += qn;
            // fetch ahead with 4 arcs per lane only: two sets of 8 would take 64 registers and a
            // workgroup per CU (169 VGPRs)
            if constexpr (PADR <= 4) {
                expand_queue_nr<G, PADR>(q, qn, grp, gl, lab, rng, arcs, lat_guard, ovf);
            } else {
                for (uint32_t t = 0; t < qn; t += NG) {
                    const uint32_t qi = t + grp;
                    if (qi < qn) relax_node_pad_nr<G, PADR>(q[qi], gl, lab, rng, arcs, lat_guard, ovf);
                }
            }
            qn = 0;
            __builtin_amdgcn_wave_barrier();
        };
#pragma unroll 1
        for (uint32_t i = 0; i < kShadowN; ++i) {
            const bool has = (selm >> i) & 1u;
            const uint64_t bal = __ballot(has);
            if (bal == 0) continue;   // wave-uniform
            any = true;
            if (has) q[qn + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = tid + i * BLOCK;
            qn += (uint32_t)__popcll(bal);
            if (qn >= kQCap) flush();
        }
        if (qn > 0) flush();
        ++sweeps;
        if (any) mnext = min(mnext, (uint32_t)min((uint64_t)lo + amin, (uint64_t)kLat32Inf - 1));
        for (int o = 32; o > 0; o >>= 1) mnext = min(mnext, (uint32_t)__shfl_xor((int)mnext, o));
        if (lane == 0 && mnext != kLat32Inf) atomicMin(&ctl[1 + slot], mnext);
        __syncthreads();   // (drains the wave's label atomics: the only wait for them in a sweep)
        slot = slot == 2 ? 0 : slot + 1;
    }
    if (ovf) atomicOr(&flags[0], 1u);
    if (stats && lane == 0) {
        atomicAdd(&stats[0], (unsigned long long)expanded);
        if (wave == 0) atomicAdd(&stats[1], (unsigned long long)sweeps);
    }
    if (!used && !nh_out && n_used % 4 == 0 &&
        ((reinterpret_cast<uintptr_t>(out_lat + orow) | reinterpret_cast<uintptr_t>(out_loss + orow)) & 15u) == 0)
        row_emit4<BLOCK>(lab, n_used, row, orow, diag_lat, diag_loss, out_lat, out_loss, unreach);
    else
        row_emit<BLOCK, false>(lab, pred, abeg, aend, arcs, V, used, n_used, src, row, orow, diag_lat, diag_loss,
                               out_lat, out_loss, unreach, nh_out, nullptr, 0u);
}

template <int BLOCK, int G, int PADR>
__global__ __launch_bounds__(BLOCK) void sssp_lds_shadow(
    const uint32_t* __restrict__ abeg, const uint32_t* __restrict__ aend, const uint4* __restrict__ arcs,
    uint32_t V, const uint32_t* __restrict__ used, uint32_t n_used, uint32_t row_begin,
    const uint64_t* __restrict__ diag_lat, const float* __restrict__ diag_loss, uint64_t* __restrict__ out_lat,
    float* __restrict__ out_loss, uint32_t* __restrict__ flags, unsigned long long* __restrict__ unreach,
    uint32_t delta, uint32_t amin, unsigned long long* __restrict__ stats, uint32_t* __restrict__ nh_out,
    uint32_t lat_guard) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr uint32_t NW = BLOCK / 64;
    uint64_t* lab = reinterpret_cast<uint64_t*>(smem);   // V labels + 64 per-lane scratch labels
    uint32_t* ctl = reinterpret_cast<uint32_t*>(lab + V + 64) + ((V + 31) >> 5);
    uint32_t* wq = ctl + 4;
    const uint32_t rng_off =
        (((uint32_t)((wq + NW * kQStride) - reinterpret_cast<uint32_t*>(smem)) * 4u) + 7u) & ~7u;
    uint2* rng = reinterpret_cast<uint2*>(smem + rng_off);   // next hops' pred[V] takes its place at the end
    sssp_row_shadow<BLOCK, G, PADR>(lab, ctl, wq, rng, abeg, aend, arcs, V, used, n_used, row_begin + blockIdx.x,
                                    (size_t)blockIdx.x * n_used, diag_lat, diag_loss, out_lat, out_loss, flags,
                                    unreach, delta, amin, stats, nh_out, reinterpret_cast<uint32_t*>(rng), lat_guard);
}

template <int BLOCK, int G, bool CACHE>
static void launch_group(shd_ctx* ctx, const ArcView& A, uint32_t rb, uint32_t re, size_t lds,
                         uint64_t* d_lat, float* d_loss, uint32_t delta, const uint32_t* seed,
                         uint32_t seed_stride, uint32_t use_offl) {
    PreparedGraph& P = ctx->prep;
    constexpr int R = G >= 32 ? 2 : G == 4 ? 2 : 4;   // arcs in flight per lane (R = 6, 8 at G = 8 measured slower on C2)
    // padded lists: labels stay below 2^32 - 1 while lu <= guard (0 = unpadded path)
    const uint64_t guard = (uint64_t)kLat32Inf - 1 - P.max_arc_lat;
    const uint32_t lat_guard =
        A.pad != 0 && delta != kLat32Inf && !seed && P.max_arc_lat < kLat32Inf - 1
            ? (uint32_t)std::max<uint64_t>(guard, 1)
            : 0u;
    uint32_t* flags = ctx->g_flags.as<uint32_t>();
    auto* unreach = reinterpret_cast<unsigned long long*>(ctx->g_flags.as<char>() + 16);
    auto* stats = ctx->stats_on ? reinterpret_cast<unsigned long long*>(ctx->g_flags.as<char>() + 32) : nullptr;
    hipEvent_t e0 = ctx->time_now ? ctx->ev[2] : nullptr, e1 = ctx->time_now ? ctx->ev[3] : nullptr;
    const uint32_t* usedp = A.used ? A.used : P.used_ident ? nullptr : (const uint32_t*)ctx->g_used.as<uint32_t>();
    if constexpr (G == 4 || G == 8) {
        if (lat_guard) {
            // a group step covers G x PADR slots: a whole list of 64 (G = 8) or 32 slots (G = 4 with 8
            // arcs per lane, G = 8 with 4), or half a 64-slot list (G = 4); wider groups take the
            // unpadded path below
            // fire-and-forget sweeps (sssp_lds_shadow; SHD_SSSP_SHADOW=0: the returning atomics, for
            // A/B) while a thread's kShadowN shadows cover the nodes and the arc-range cache fits
            if (CACHE && P.V <= kShadowN * BLOCK && ctx->knobs.get(K_SSSP_SHADOW, 1) != 0) {
                auto kern = sssp_lds_shadow<BLOCK, G, 8>;
                if constexpr (G == 8)
                    if (A.pad == 32) kern = sssp_lds_shadow<BLOCK, G, 4>;
                hipExtLaunchKernelGGL(kern, dim3(re - rb), dim3(BLOCK), (uint32_t)lds, ctx->stream, e0, e1, 0u,
                                      A.beg, A.end, A.arcs, P.V, usedp, P.n_used, rb,
                                      (const uint64_t*)ctx->g_diag_lat.as<uint64_t>(),
                                      (const float*)ctx->g_diag_loss.as<float>(), d_lat, d_loss, flags, unreach,
                                      delta, P.min_arc_lat, stats, ctx->nh_out, lat_guard);
                return;
            }
            auto kern = sssp_lds_group<BLOCK, G, R, CACHE, 8>;
            if constexpr (G == 8)
                if (A.pad == 32) kern = sssp_lds_group<BLOCK, G, R, CACHE, 4>;
            hipExtLaunchKernelGGL(kern, dim3(re - rb), dim3(BLOCK), (uint32_t)lds,
                                  ctx->stream, e0, e1, 0u, A.beg, A.end, A.arcs, P.V, usedp, P.n_used, rb,
                                  (const uint64_t*)ctx->g_diag_lat.as<uint64_t>(),
                                  (const float*)ctx->g_diag_loss.as<float>(), d_lat, d_loss, flags, unreach, delta,
                                  stats, seed, seed_stride, ctx->nh_out, lat_guard, use_offl, 0u, 0u);
            return;
        }
    }
    hipExtLaunchKernelGGL((sssp_lds_group<BLOCK, G, R, CACHE, 0>), dim3(re - rb), dim3(BLOCK), (uint32_t)lds,
                          ctx->stream, e0, e1, 0u, A.beg, A.end, A.arcs, P.V, usedp, P.n_used, rb,
                          (const uint64_t*)ctx->g_diag_lat.as<uint64_t>(), (const float*)ctx->g_diag_loss.as<float>(),
                          d_lat, d_loss, flags, unreach, delta, stats, seed, seed_stride, ctx->nh_out, 0u,
                          use_offl, 0u, kHubDeg);
}

template <int BLOCK, bool CACHE>
static void launch_by_degree(shd_ctx* ctx, const ArcView& A, uint32_t rb, uint32_t re, uint64_t* d_lat,
                             float* d_loss, uint32_t delta, uint32_t G, const uint32_t* seed,
                             uint32_t ss) {
    const uint32_t V = ctx->prep.V;
    size_t lds = sssp_lds_bytes(V, BLOCK, CACHE);
    if (ctx->nh_out && !CACHE) lds = ((lds + 7) & ~(size_t)7) + (size_t)V * 4;   // pred[V]
    // no room for the {beg, end} cache: a plain CSR's offsets alone (4 B/node) when they fit
    // (C3, 10k nodes: every relaxation's arc range from LDS instead of two dependent loads)
    uint32_t use_offl = 0;
    if (!CACHE && A.end == A.beg + 1 && lds + (size_t)(V + 1) * 4 + 8 <= ctx->max_lds) {
        lds = ((lds + 7) & ~(size_t)7) + (size_t)(V + 1) * 4;
        use_offl = 1;
    }
    switch (G) {
        case 64: launch_group<BLOCK, 64, CACHE>(ctx, A, rb, re, lds, d_lat, d_loss, delta, seed, ss, use_offl); break;
        case 32: launch_group<BLOCK, 32, CACHE>(ctx, A, rb, re, lds, d_lat, d_loss, delta, seed, ss, use_offl); break;
        case 16: launch_group<BLOCK, 16, CACHE>(ctx, A, rb, re, lds, d_lat, d_loss, delta, seed, ss, use_offl); break;
        case 8: launch_group<BLOCK, 8, CACHE>(ctx, A, rb, re, lds, d_lat, d_loss, delta, seed, ss, use_offl); break;
        default: launch_group<BLOCK, 4, CACHE>(ctx, A, rb, re, lds, d_lat, d_loss, delta, seed, ss, use_offl); break;
    }
}

shd_status run_sssp(shd_ctx* ctx, const ArcView& A, uint32_t rb, uint32_t re, uint64_t* d_lat, float* d_loss,
                    uint32_t delta, const uint32_t* seed, uint32_t ss) {
    PreparedGraph& P = ctx->prep;
    hipStream_t s = ctx->stream;
    const double deg = (double)A.n_arcs / std::max<uint32_t>(P.V, 1);
    // G lanes x R arcs (R = 4 below G = 32) per node; measured best on C2 (pruned, ~48 arcs
    // per node) at G = 8 and on C3 (BA, ~6 arcs per node) at G = 4
    uint32_t G = deg >= 64 ? 16 : deg >= 24 ? 8 : 4;
    // 32-slot padded lists (prune_rows2, ~21 arcs per node on C2): G = 8 with 4 arcs per lane, equal
    // or ~1 us ahead of G = 4 with 8 (54 against 72 VGPRs; DESIGN 4, routing item 2)
    if (A.pad == kPad2) G = 8;
    G = ctx->knobs.get(K_SSSP_G, G);          // tuning overrides (results are identical)
    // Workgroup shape: once a source's labels need most of the LDS, one 1024-thread workgroup
    // per CU (the LDS arc-range cache is dropped when it no longer fits).  Otherwise rows per CU
    // decide: with one row or fewer per CU the row's sweeps are the critical path and 16 waves
    // shorten them (C2, 125 rows: 71 us at 1024 threads vs 151 at 256); with ~4 rows per CU
    // the CU is full either way and 256 is best (196 vs 252 us).
    const size_t half = ctx->max_lds / 2;
    const uint32_t rows_per_cu = div_up(re - rb, (uint32_t)ctx->n_cu);
    uint32_t block = sssp_lds_bytes(P.V, 256, true) > half ? 1024
                     : rows_per_cu <= 1 ? 1024 : rows_per_cu <= 2 ? 512 : 256;
    block = ctx->knobs.get(K_SSSP_BLOCK, block);
    if (block != 256 && block != 512 && block != 1024) block = 256;
    // (edge-parallel expand_flat, as in the global-label kernel, measured slower here: the
    // kernel is issue-bound and the owner search costs more than the dead group slots; C2
    // 132 -> 197 us, so the LDS kernels keep node groups)
    const bool cache = sssp_lds_bytes(P.V, block, true) <= ctx->max_lds;
    // launch_group records ev[2] / ev[3] on the kernel's dispatch packet (hipExtLaunchKernel):
    // separate event markers around it cost ~6 us of queue gap each on C2
    if (block == 1024) {
        if (cache) launch_by_degree<1024, true>(ctx, A, rb, re, d_lat, d_loss, delta, G, seed, ss);
        else launch_by_degree<1024, false>(ctx, A, rb, re, d_lat, d_loss, delta, G, seed, ss);
    } else if (block == 512) {
        if (cache) launch_by_degree<512, true>(ctx, A, rb, re, d_lat, d_loss, delta, G, seed, ss);
        else launch_by_degree<512, false>(ctx, A, rb, re, d_lat, d_loss, delta, G, seed, ss);
    } else {
        if (cache) launch_by_degree<256, true>(ctx, A, rb, re, d_lat, d_loss, delta, G, seed, ss);
        else launch_by_degree<256, false>(ctx, A, rb, re, d_lat, d_loss, delta, G, seed, ss);
    }
    SHD_HIP(hipGetLastError());
    if (ctx->stats_on) {
        unsigned long long st[2];
        SHD_HIP(hipMemcpyAsync(st, ctx->g_flags.as<char>() + 32, 16, hipMemcpyDeviceToHost, s));
        SHD_HIP(hipStreamSynchronize(s));
        std::fprintf(stderr, "shd_sssp: rows=%u G=%u block=%u delta=%u expanded=%llu (%.2f per node) "
                     "sweeps=%llu (%.1f per row) arcs=%llu\n", re - rb, G, block, delta, st[0],
                     (double)st[0] / ((double)(re - rb) * P.V), st[1], (double)st[1] / (re - rb),
                     (unsigned long long)A.n_arcs);
    }
    return SHD_OK;
}

int sssp_lds_vgprs(int shadow) {
    hipFuncAttributes at{};
    const void* f = shadow ? reinterpret_cast<const void*>(&sssp_lds_shadow<256, 8, 4>)
                           : reinterpret_cast<const void*>(&sssp_lds_group<1024, 4, 2, false, 0>);
    return hipFuncGetAttributes(&at, f) == hipSuccess ? at.numRegs : -1;
}

}  // namespace shd

#ifdef SHD_SSSP_PROF   // tools/sssp_prof.py, tools/c4_prof.py (c3)
extern "C" int shd_debug_sssp_prof(unsigned long long* out, int reset) { return shd::sssp_prof_read(out, reset); }
#endif
