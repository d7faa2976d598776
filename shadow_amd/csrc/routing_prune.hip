// The dense prune (routing_priv.h has the overview): a dense graph's arcs that can lie on a
// shortest-latency path, left as padded lists for the LDS-label SSSP.
#include "routing_priv.h"

namespace shd {

#ifdef SHD_SSSP_PROF
// tuning builds only (tools/prune_prof.py; tools/build_prof.sh compiles this unit under the macro).
// prune_rows: shader clocks per phase summed over workgroups (thread 0): row load + max, histogram,
// boundary bin, detour selection, 2-hop tests, list write; [6] first start, [7] last end (100 MHz)
__device__ unsigned long long g_prune_prof[4096 * 8];   // per workgroup (row u < 4096)
#define PR_MARK(slot) do { if (threadIdx.x == 0) { const uint64_t t_ = __builtin_amdgcn_s_memtime(); \
    pr_acc[slot] += t_ - pr_t; pr_t = t_; } } while (0)
#else
#define PR_MARK(slot) do { } while (0)
#endif

// ------------------------------------------------------------------------------------------
// Dense-graph arc pruning (SHD_ALGO_PRUNED).  An arc (u,v) lies on no shortest-latency path if
// some 2-hop detour u->x->v is STRICTLY shorter; such arcs cannot change any lexicographic
// label (the latency part is decided first and every tight path avoids them), so the SSSP
// runs on the surviving arcs only and still reproduces the reference's bits.  x ranges
// over the K lowest-latency neighbours of u (any subset is sound; the nearest catch almost
// all: C2 keeps ~49 of 999 arcs per node with K = 32).  Ties (detour == arc) are kept.
// ------------------------------------------------------------------------------------------
// One workgroup per row u: the row's arc keys (parallel arcs folded by a lexicographic LDS
// atomicMin) built in LDS and written once as the latency row Wl and the loss row Wp -- one
// pass instead of init + global-atomic scatter + a latency-extract pass (C2: 16 -> 7 us); the
// prune reads its own row's latencies from Wl and the loss only of the arcs it keeps, so the
// 8-byte key row is not written (round 3).
// (A u16 latency row rounded up -- sound for the prune, half the gathered bytes -- measured
// slower: prune_rows 32 -> 57 us, the decode outweighing the bytes.)
__global__ __launch_bounds__(256) void dense_build(const uint32_t* __restrict__ off,
                                                   const uint32_t* __restrict__ adst,
                                                   const uint32_t* __restrict__ alat,
                                                   const float* __restrict__ aloss, uint32_t V,
                                                   float* __restrict__ Wp, uint32_t* __restrict__ Wl,
                                                   uint32_t* __restrict__ flags) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* rowk = reinterpret_cast<uint64_t*>(smem);
    const uint32_t u = blockIdx.x, tid = threadIdx.x;
    for (uint32_t v = tid; v < V; v += 256) rowk[v] = kKeyInf;
    if (u == 0 && tid < 16) flags[tid] = (tid == 4 || tid == 5) ? 0xFFFFFFFFu : 0u;   // as flags_init
    __syncthreads();
    for (uint32_t k = off[u] + tid; k < off[u + 1]; k += 256)
        atomicMin(reinterpret_cast<unsigned long long*>(&rowk[adst[k]]), (unsigned long long)pack_key(alat[k], aloss[k]));
    __syncthreads();
    const size_t base = (size_t)u * V;
    for (uint32_t v = tid; v < V; v += 256) {
        const uint64_t k = rowk[v];
        Wp[base + v] = key_loss(k);
        Wl[base + v] = key_lat(k);
    }
}

// DCSR (complete graphs without parallel arcs, PreparedGraph::dense_rows): the arc CSR is the
// dense matrix itself -- node x's arcs are every other node in index order, so the latency of
// (x, v) is Wl[x (V - 1) + v - (v > x)] and (x, x) has none -- and the prune reads it directly:
// no dense_build pass, no V x V matrices (the CSR's latency and loss arrays are Wl and Wp).
// Block 0 then also resets the build flags (dense_build's job otherwise).
template <bool DCSR>
__device__ __forceinline__ uint32_t dense_lat(const uint32_t* __restrict__ Wl, uint32_t V, uint32_t x, uint32_t v) {
    if constexpr (DCSR) return v == x ? kLat32Inf : Wl[(size_t)x * (V - 1) + v - (v > x ? 1u : 0u)];
    else return Wl[(size_t)x * V + v];
}

// Row u of the matrix into LDS (row[v]: latency, +inf where there is no arc and at v == u), read
// in 16-byte pieces: the row's memory span [u rs, u rs + rs), rs the row stride, walked in aligned
// 4-word chunks, each element mapped back to its column (DCSR: a column at or past the diagonal
// moves up by one).  The head and tail chunks, which reach outside the span, load word by word.
template <int BLOCK, bool DCSR>
__device__ __forceinline__ void load_row16(const uint32_t* __restrict__ Wl, uint32_t V, uint32_t u, uint32_t* row) {
    const uint32_t rs = DCSR ? V - 1 : V, base = u * rs, a0 = base & ~3u;   // (V <= 4096: indices fit u32)
    const uint32_t nch = (base + rs - a0 + 3u) >> 2;
    for (uint32_t c = threadIdx.x; c < nch; c += BLOCK) {
        const uint32_t p = a0 + 4u * c;
        uint32_t w[4];
        if (p >= base && p + 4u <= base + rs) {
            const uint4 q = *reinterpret_cast<const uint4*>(Wl + p);
            w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) w[i] = p + i >= base && p + i < base + rs ? Wl[p + i] : kLat32Inf;
        }
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t e = p + i - base;   // (before the span: wraps past rs)
            if (e >= rs) continue;
            const uint32_t v = e + (DCSR && e >= u ? 1u : 0u);
            row[v] = v == u ? kLat32Inf : w[i];
        }
    }
    if (DCSR && threadIdx.x == 0) row[u] = kLat32Inf;   // (x, x) has no entry
}

// The detour selection shared by prune_rows and nearest_rows: the K nearest out-arcs of the row
// held in LDS (row[v]: latency or +inf; mx: this thread's largest finite one, read without CMP
// only; shg: the bin shift from the graph's largest arc latency, read with CMP only), left in
// selx / sela (unused slots: node 0, latency +inf).  Detour nodes x: ~K of u's lowest-latency
// neighbours, chosen by a 256-bin latency histogram (every node in the bins below the K-th
// smallest latency's bin, then nodes of that bin in index order up to K).  CMP: exactly the K
// smallest (latency, index) pairs in ascending order, ranked in LDS by all waves.  Ends with a
// barrier; cnt[0] (kept arcs) and cnt[7] (first-batch survivors) are reset for the caller.
struct SelectLds {
    uint32_t *cnt, *hist, *selx, *sela, *row;   // [8], [256], [K], [K], [V]
    uint16_t* binv;                             // [V] bin per node (0xFFFF: no arc)
    uint64_t* cand;                             // CMP: [64] detour candidates
    uint32_t* rk;                               // CMP: [64] their ranks
};
template <int BLOCK, int K, bool CMP, class Mark>
__device__ __forceinline__ void select_nearest(const SelectLds& L, uint32_t V, uint32_t mx, uint32_t shg, Mark&& mark) {
    uint32_t *const cnt = L.cnt, *const hist = L.hist, *const selx = L.selx, *const sela = L.sela, *const row = L.row;
    uint16_t* const binv = L.binv;
    uint64_t* const cand = L.cand;
    uint32_t* const rk = L.rk;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    for (uint32_t i = tid; i < 256; i += BLOCK) hist[i] = 0;
    if (tid < 8) cnt[tid] = 0;
    if (CMP && tid < 64) rk[tid] = 0;
    uint32_t sh;
    if constexpr (CMP) {   // bins from the graph's largest arc latency (host, shg): one barrier
        __syncthreads();
        sh = shg;
    } else {   // bins from the row's own largest latency
        for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
        __syncthreads();
        if (lane == 0) atomicMax(&cnt[2], mx);
        __syncthreads();
        const uint32_t bits = 32u - (uint32_t)__clz((int)max(cnt[2], 1u));
        sh = bits > 8 ? bits - 8 : 0;
    }
    mark(0);
    for (uint32_t v = tid; v < V; v += BLOCK) {
        const uint32_t w = row[v];
        binv[v] = w != kLat32Inf ? (uint16_t)(w >> sh) : (uint16_t)0xFFFF;
        if (w != kLat32Inf) atomicAdd(&hist[w >> sh], 1u);
    }
    __syncthreads();
    mark(1);
    if (tid < 64) {   // wave 0: the bin holding the K-th smallest latency
        uint32_t c[4], sum = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            c[i] = hist[tid * 4 + i];
            sum += c[i];
        }
        uint32_t incl = sum;
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        uint32_t run = incl - sum, bsel = 256, below = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (bsel == 256 && run + c[i] >= (uint32_t)K) {
                bsel = tid * 4 + i;
                below = run;
            }
            run += c[i];
        }
        const uint64_t m = __ballot(bsel != 256);
        if (m) {
            const uint32_t first = (uint32_t)__ffsll((unsigned long long)m) - 1u;
            const uint32_t b = __shfl((int)bsel, first), bl = __shfl((int)below, first);
            if (tid == 0) {
                cnt[4] = b;
                cnt[3] = bl;
            }
        } else if (tid == 0) {
            cnt[4] = 256;      // fewer than K finite entries: take them all
            cnt[3] = 0;
        }
        if (tid == 0) {
            cnt[5] = 0;        // slots below the bin
            cnt[6] = 0;        // slots in the bin
        }
    }
    __syncthreads();
    mark(2);
    // CMP: the detours are the K smallest (latency, index) pairs in ascending order.  Fast path:
    // the bins below and the boundary bin hold at most 64 candidates -- collect them, and wave 0
    // sorts them in registers; otherwise the index-order boundary scan below, then a rank sort.
    bool sel_done = false;
    if constexpr (CMP && K <= 64) {
        const uint32_t bsel = cnt[4];
        const uint32_t ncand = bsel < 256 ? cnt[3] + hist[bsel] : (uint32_t)K;
        if (ncand <= 64) {
            // rank sort: wave p compares every candidate with its share of the others
            for (uint32_t v = tid; v < V; v += BLOCK) {
                if (binv[v] <= bsel) {   // (no arc: 0xFFFF, above every bin)
                    const uint32_t sl = atomicAdd(&cnt[5], 1u);
                    cand[sl] = (uint64_t)row[v] << 32 | v;
                }
            }
            __syncthreads();
            const uint32_t n = cnt[5];
            constexpr uint32_t per = 64 / (BLOCK / 64);
            if (lane < n) {
                const uint64_t ki = cand[lane];
                const uint32_t j0 = (tid >> 6) * per;
                uint32_t r = 0;
#pragma unroll
                for (uint32_t jj = 0; jj < per; ++jj)
                    r += j0 + jj < n && cand[j0 + jj] < ki ? 1u : 0u;
                if (r) atomicAdd(&rk[lane], r);
            }
            __syncthreads();
            if (tid < 64) {
                if (lane < n) {
                    const uint32_t r = rk[lane];
                    if (r < (uint32_t)K) {
                        const uint64_t k = cand[lane];
                        selx[r] = (uint32_t)k;
                        sela[r] = (uint32_t)(k >> 32);
                    }
                } else if (lane < (uint32_t)K) {   // unused slots: no detour
                    selx[lane] = 0u;
                    sela[lane] = kLat32Inf;
                }
                if (tid == 0) {
                    cnt[0] = 0;
                    cnt[7] = 0;
                }
            }
            sel_done = true;
        }
    }
    if (!sel_done) {   // every node of the bins below; then wave 0 takes the boundary bin in index order, so
        // the detour set (and with it the kept-arc count) is the same on every run
        const uint32_t bsel = cnt[4], below = cnt[3];
        for (uint32_t v = tid; v < V; v += BLOCK) {
            if (binv[v] < bsel) {
                const uint32_t sl = atomicAdd(&cnt[5], 1u);
                selx[sl] = v;
                sela[sl] = row[v];
            }
        }
        if (tid < 64 && bsel < 256) {
            uint32_t taken = 0;
            for (uint32_t v0 = 0; v0 < V && below + taken < (uint32_t)K; v0 += 64) {
                const uint32_t v = v0 + lane;
                const bool hit = v < V && binv[v] == bsel;
                const uint64_t m = __ballot(hit);
                const uint32_t sl = below + taken + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                if (hit && sl < (uint32_t)K) {
                    selx[sl] = v;
                    sela[sl] = row[v];
                }
                taken += (uint32_t)__popcll(m);
            }
            if (tid == 0) cnt[6] = taken;
        }
        __syncthreads();
        const uint32_t nsel = min((uint32_t)K, cnt[5] + cnt[6]);
        for (uint32_t j = nsel + tid; j < (uint32_t)K; j += BLOCK) {   // unused slots: no detour
            selx[j] = 0u;
            sela[j] = kLat32Inf;
        }
        if (tid == 0) cnt[0] = 0;
        if constexpr (CMP) {   // detours in ascending latency (ties by index): wave 0 ranks them
            __syncthreads();
            uint32_t* tx = hist;   // the histogram is spent; K <= 128 pairs fit its 256 words
            uint32_t* ta = hist + K;
            if (tid < 64) {
                for (uint32_t i = lane; i < (uint32_t)K; i += 64) {
                    const uint32_t ai = sela[i], xi = selx[i];
                    uint32_t r = 0;
#pragma unroll 4   // (unrolled whole, the K flags are summed at the end: > 64 VGPRs)
                    for (uint32_t j = 0; j < (uint32_t)K; ++j) {
                        const uint32_t aj = sela[j], xj = selx[j];
                        r += aj < ai || (aj == ai && (xj < xi || (xj == xi && j < i))) ? 1u : 0u;
                    }
                    tx[r] = xi;
                    ta[r] = ai;
                }
            }
            __syncthreads();
            for (uint32_t j = tid; j < (uint32_t)K; j += BLOCK) {
                selx[j] = tx[j];
                sela[j] = ta[j];
            }
            if (tid == 0) cnt[7] = 0;   // survivors of the first batch
        }
    }
    __syncthreads();
}

template <int BLOCK, int K, bool DCSR = false, int VB = 4, int KB = 8, bool CMP = false, int PB = 8>
__global__ __launch_bounds__(BLOCK) void prune_rows(
    const uint32_t* __restrict__ Wl, const float* __restrict__ Wp, uint32_t V,
    uint32_t* __restrict__ pbeg, uint32_t* __restrict__ pend, uint4* __restrict__ parcs,
    uint32_t* __restrict__ flags, uint32_t shg = 0) {
    // Detour nodes x: ~K of u's lowest-latency neighbours (select_nearest).  Any set of detour
    // nodes is sound -- it only decides how many arcs are dropped -- so this replaces a full
    // bitonic sort of the row (55 barrier stages) by three passes over it.
    // CMP (round 5, the K = 32 default; C2 prune 24.4 -> 15.6 us): the detours are the K
    // smallest (latency, index) pairs in ascending order, ranked in LDS by all waves; the first
    // batch tests every arc against the KB nearest, skipping detours no shorter than the arc; its
    // survivors (~11 % of a C2 row) are packed and tested one lane each against the rest, PB at a
    // time, stopping at the first detour no shorter than the arc -- instead of every wave
    // carrying a few live lanes through every batch.  The row's losses come in with its
    // latencies, so the kept arcs read them from LDS.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint4* kept = reinterpret_cast<uint4*>(smem);      // V staged arcs
    uint32_t* cnt = reinterpret_cast<uint32_t*>(kept + V);   // [0] kept [1] base [2] max [3] below-bin
    uint32_t* hist = cnt + 8;                          // 256 bins
    uint32_t* selx = hist + 256;                       // K detour nodes
    uint32_t* sela = selx + K;                         // their latencies
    uint32_t* row = sela + K;                          // u's exact arc latencies
    uint16_t* binv = reinterpret_cast<uint16_t*>(row + V);   // bin per node (0xFFFF: no arc)
    uint2* live2 = reinterpret_cast<uint2*>((reinterpret_cast<uintptr_t>(binv + V) + 7) & ~(uintptr_t)7);   // CMP: first-batch survivors
    uint64_t* cand = reinterpret_cast<uint64_t*>(live2 + V);   // CMP: <= 64 detour candidates
    uint32_t* rk = reinterpret_cast<uint32_t*>(cand + 64);        // and their ranks
    float* prow = reinterpret_cast<float*>(rk + 64);              // CMP: u's arc losses
    const uint32_t u = blockIdx.x, tid = threadIdx.x;
#ifdef SHD_SSSP_PROF
    uint64_t pr_acc[6] = {0, 0, 0, 0, 0, 0}, pr_t = __builtin_amdgcn_s_memtime();
    const uint64_t pr_t0 = __builtin_amdgcn_s_memrealtime();
#endif
    if (DCSR && u == 0 && tid < 16) flags[tid] = (tid == 4 || tid == 5) ? 0xFFFFFFFFu : 0u;   // as flags_init
    uint32_t mx = 0;
    for (uint32_t v = tid; v < V; v += BLOCK) {
        const uint32_t w = dense_lat<DCSR>(Wl, V, u, v);
        row[v] = w;
        if (w != kLat32Inf) mx = max(mx, w);
        if constexpr (CMP) {   // the row's losses ride the same memory trip (kept arcs read them)
            if (w != kLat32Inf) prow[v] = Wp[DCSR ? (size_t)u * (V - 1) + v - (v > u ? 1u : 0u) : (size_t)u * V + v];
        }
    }
    select_nearest<BLOCK, K, CMP>(SelectLds{cnt, hist, selx, sela, row, binv, cand, rk}, V, mx, shg,
                                  [&](int slot) { (void)slot; PR_MARK(slot); });
    PR_MARK(3);
    // 2-hop test of every arc of u: each thread tests VB arcs at once against batches of KB
    // detours (VB x KB loads in flight), and a lane stops loading for an arc as soon as a
    // strictly shorter detour is found -- most arcs of a dense row fall to the first batch
    for (uint32_t v0 = tid; v0 < V; v0 += BLOCK * VB) {
        uint32_t w[VB], z[VB];
#pragma unroll
        for (int i = 0; i < VB; ++i) {
            const uint32_t v = v0 + i * BLOCK;
            w[i] = v < V ? row[v] : kLat32Inf;
            z[i] = kLat32Inf;
        }
        for (int j0 = 0; j0 < (CMP ? KB : K); j0 += KB) {
            bool any = false;
#pragma unroll
            for (int i = 0; i < VB; ++i) any |= w[i] != kLat32Inf && w[i] <= z[i];
            if (!any) break;
            uint32_t as[KB], bv[VB][KB], xs[KB];
            size_t xb[KB];
#pragma unroll
            for (int j = 0; j < KB; ++j) {
                as[j] = sela[j0 + j];
                xs[j] = selx[j0 + j];
                xb[j] = (size_t)xs[j] * (DCSR ? V - 1 : V);
            }
#pragma unroll
            for (int i = 0; i < VB; ++i) {
                const uint32_t v = v0 + i * BLOCK;
                const bool live = w[i] != kLat32Inf && w[i] <= z[i];
#pragma unroll
                for (int j = 0; j < KB; ++j) {
                    if constexpr (CMP)   // sorted detours: one no shorter than the arc cannot beat it
                        bv[i][j] = live && as[j] < w[i] && v != xs[j]
                                       ? Wl[xb[j] + v - (DCSR && v > xs[j] ? 1u : 0u)]
                                       : kLat32Inf;
                    else if constexpr (DCSR)   // (x, x) has no arc; past the diagonal the row is shifted by one
                        bv[i][j] = live && as[j] != kLat32Inf && v != xs[j] ? Wl[xb[j] + v - (v > xs[j] ? 1u : 0u)]
                                                                            : kLat32Inf;
                    else
                        bv[i][j] = live && as[j] != kLat32Inf ? Wl[xb[j] + v] : kLat32Inf;
                }
            }
#pragma unroll
            for (int i = 0; i < VB; ++i)
#pragma unroll
                for (int j = 0; j < KB; ++j) {
                    const uint32_t t = as[j] + bv[i][j];
                    if (as[j] != kLat32Inf && bv[i][j] != kLat32Inf && t >= as[j]) z[i] = min(z[i], t);
                }
        }
#pragma unroll
        for (int i = 0; i < VB; ++i) {
            if (w[i] == kLat32Inf || w[i] > z[i]) continue;
            const uint32_t v = v0 + i * BLOCK;
            if constexpr (CMP) {   // survivors of the first batch: the rest of the detours below
                if (K > KB && w[i] > sela[KB]) {
                    const uint32_t li = atomicAdd(&cnt[7], 1u);
                    live2[li] = make_uint2(v, w[i]);
                    continue;
                }
            }
            const uint32_t slot = atomicAdd(&cnt[0], 1u);
            const size_t at = DCSR ? (size_t)u * (V - 1) + v - (v > u ? 1u : 0u) : (size_t)u * V + v;
            kept[slot] = make_uint4(v, w[i], __float_as_uint(one_minus(CMP ? prow[v] : Wp[at])), 0u);
        }
    }
    if constexpr (CMP && K > KB) {
        // the first batch's survivors, packed: one lane per arc over the remaining detours in
        // batches of 8 (a wave's loads are all live instead of a few lanes of every wave)
        __syncthreads();
        const uint32_t nl = cnt[7];
        for (uint32_t i = tid; i < nl; i += BLOCK) {
            const uint2 e = live2[i];
            const uint32_t v = e.x, wv = e.y;
            uint32_t z = kLat32Inf;
            for (int j0 = KB; j0 < K && wv <= z && sela[j0] < wv; j0 += PB) {
                uint32_t as[PB], bq[PB];
#pragma unroll
                for (int j = 0; j < PB; ++j) {
                    as[j] = j0 + j < K ? sela[j0 + j] : kLat32Inf;
                    const uint32_t x = j0 + j < K ? selx[j0 + j] : 0u;
                    bq[j] = as[j] < wv && v != x
                                ? Wl[(size_t)x * (DCSR ? V - 1 : V) + v - (DCSR && v > x ? 1u : 0u)]
                                : kLat32Inf;
                }
#pragma unroll
                for (int j = 0; j < PB; ++j) {
                    const uint32_t t = as[j] + bq[j];
                    if (as[j] != kLat32Inf && bq[j] != kLat32Inf && t >= as[j]) z = min(z, t);
                }
            }
            if (wv > z) continue;
            const uint32_t slot = atomicAdd(&cnt[0], 1u);
            kept[slot] = make_uint4(v, wv, __float_as_uint(one_minus(prow[v])), 0u);
        }
    }
    __syncthreads();
    PR_MARK(4);
    // each list is padded to kPad1 slots with no-op arcs for relax_node_pad (scratch label
    // V + i, lat 0, q 0: candidate (lu, 1.0f) against a scratch label holding 0).  Row u's list
    // starts at u * roundup(V, kPad1): the 1000 workgroups of C2 finish together, and one
    // shared cursor (rows packed in arrival order) serialised their atomics at the end of the
    // kernel; the slots a sweep touches are the same lines either way.
    // (at least one block of slots, also for an empty list: prune_rows2 reads the first kPad1 slots
    // of other rows' lists without their lengths)
    const uint32_t n = cnt[0], np = max((n + kPad1 - 1) / kPad1 * kPad1, kPad1);
    const uint32_t at = u * ((V + kPad1 - 1) / kPad1 * kPad1);
    for (uint32_t i = tid; i < np; i += BLOCK)
        parcs[at + i] = i < n ? kept[i] : make_uint4(V + (i & 63u), 0u, 0u, 0u);
    if (tid == 0) {
        pbeg[u] = at;
        pend[u] = at + n;
    }
#ifdef SHD_SSSP_PROF
    PR_MARK(5);
    if (tid == 0 && u < 4096) {
        for (int k = 0; k < 6; ++k) g_prune_prof[u * 8 + k] = pr_acc[k];
        g_prune_prof[u * 8 + 6] = pr_t0;
        g_prune_prof[u * 8 + 7] = __builtin_amdgcn_s_memrealtime();
    }
#endif
}

// Second prune stage (prune_rows2): a 3-hop test over the lists that prune_rows kept, one
// workgroup per row u.  The 2-hop prune stops at ~48 arcs per node on C2 because its survivors
// need 3-hop detours to fall; over the dense matrix that test costs as much as the prune, over
// the kept lists it is ~2,400 pairs per row:
//   d2[y] = min(lat(u, y) if (u, y) is kept, min over kept x of lat(u, x) + lat(x, y) with
//           (x, y) kept by row x)                                   -- a walk u -> x -> y
//   (u, v) is dropped iff some y in kept(v), y != u, y != v, has d2[y] + lat(y, v) < lat(u, v),
//   lat(y, v) read from the dense matrix (the arc y -> v itself: kept(v) only names candidates,
//   and on a directed graph lat(v, y) is another number).
// Soundness: every compared detour is a walk u -> (x ->) y -> v of real arcs with their original
// latencies (the stage-1 lists hold arcs of the graph unchanged, Wl holds the graph's arcs).  An
// arc with a strictly shorter walk between its ends lies on no shortest-latency path, and the loss
// is chosen only among shortest-latency paths, so the tables do not see it.  A tight arc
// (lat(u, v) = d(u, v)) has no strictly shorter walk, so it is never dropped -- whatever other
// rows drop at the same time: the test reads only stage-1 lists and the matrix, never a
// stage-2 list, and every shortest path is made of tight arcs alone.  Ties (<, strictly) keep
// the arc.  Any candidate set is sound; it only decides how much is dropped.
// The sums: lat(u, x) + lat(x, y) is guarded as in prune_rows (a wrapped or +inf sum is no
// detour); the three-term sum is formed in 64 bits, so it cannot wrap into a "shorter" walk.
// +inf entries (no arc) are never added.
// Memory trips: a stage-1 list starts at its row's fixed offset and its first kPad1 slots are
// always written (pads name a node >= V), so the kernel needs no list length but its own: one
// trip for kept(u), one for the first 64 slots of every kept node's list (wave w takes lists w,
// w + 8, ..., a lane per slot), one for
// the lat(y, v) gathers of the pairs whose d2[y] is below lat(u, v), and the list write.
// Bounded work: 64 lists x 64 slots = 4,096 pairs at most (C2: ~2,400).  A row of more than
// kP2MaxKept = 64 kept arcs (heavily tied graphs, where stage 1 prunes nothing; a handful of C2
// rows) is copied through unchanged, and a kept node's list of 64 arcs or more (its slot 63 is no
// pad) names no candidates: both rules depend on list lengths only, never on the order in which
// stage 1's atomics filled a list, so they are the same on every run.  The surviving set is the
// same on every run (d2 is a minimum, the drop flags are idempotent); survivors keep their
// stage-1 order.
// Lists are padded to kPad2 = 32 slots with the same no-op arcs as stage 1, at the same fixed
// per-row offset in a second buffer (the kernel reads other rows' stage-1 lists while it runs).
constexpr uint32_t kP2MaxKept = 64;   // C2: 48.5 arcs per row, 66 at most
constexpr int kP2Block = 512, kP2Half = 8;   // 8 waves x kP2Half lists = the 64 lists tested
static size_t prune2_lds_bytes(uint32_t V) { return (size_t)kP2MaxKept * 16 + (size_t)kP2MaxKept * 4 + (size_t)V * 4; }
template <bool DCSR>
__global__ __launch_bounds__(kP2Block) void prune_rows2(
    const uint32_t* __restrict__ Wl, uint32_t V, const uint32_t* __restrict__ beg1,
    const uint32_t* __restrict__ end1, const uint4* __restrict__ arcs1, uint32_t* __restrict__ pbeg,
    uint32_t* __restrict__ pend, uint4* __restrict__ parcs) {
    static_assert((kP2Block / 64) * kP2Half == 64 && kP2MaxKept == 64 && kPad1 == 64, "64 lists, a lane per slot");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint4* ku = reinterpret_cast<uint4*>(smem);                      // kept(u), as stage 1 wrote it
    uint32_t* drop = reinterpret_cast<uint32_t*>(ku + kP2MaxKept);   // [kP2MaxKept] arc falls
    uint32_t* d2 = drop + kP2MaxKept;                                // [V] 2-hop row
    const uint32_t u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t stride = (V + kPad1 - 1) / kPad1 * kPad1;
    const uint32_t at = u * stride;   // the row's fixed offset, in both buffers
    const uint4* mine = arcs1 + at;
    uint4 a = make_uint4(0u, 0u, 0u, 0u);
    if (tid < kPad1) a = mine[tid];   // (always written: rides the same trip as the length)
    const uint32_t n = end1[u] - beg1[u];
    if (n > kP2MaxKept) {   // too long a list (too much work): the stage-1 list as it is
        const uint32_t np = (n + kPad2 - 1) / kPad2 * kPad2;
        for (uint32_t i = tid; i < np; i += kP2Block)
            parcs[at + i] = i < n ? mine[i] : make_uint4(V + (i & 63u), 0u, 0u, 0u);
        if (tid == 0) {
            pbeg[u] = at;
            pend[u] = at + n;
        }
        return;
    }
    if (tid < n) ku[tid] = a;
    if (tid < kP2MaxKept) drop[tid] = 0u;
    for (uint32_t v = tid; v < V; v += kP2Block) d2[v] = kLat32Inf;
    __syncthreads();
    // pair (list j = kept(u)[j], slot): {y, lat(x, y)}; a pad slot (y >= V) or a list past n: none
    auto load_half = [&](uint32_t h, uint2* pr) {
#pragma unroll
        for (int k = 0; k < kP2Half; ++k) {
            const uint32_t j = h * 64 + (uint32_t)k * (kP2Block / 64) + wave;   // wave-uniform
            pr[k] = make_uint2(0xFFFFFFFFu, kLat32Inf);
            if (j < n) pr[k] = *reinterpret_cast<const uint2*>(arcs1 + (size_t)ku[j].x * stride + lane);
            // a list of 64 arcs or more (slot 63 holds an arc) is cut off by the block: not used
            if ((uint32_t)__shfl((int)pr[k].x, 63) < V) pr[k] = make_uint2(0xFFFFFFFFu, kLat32Inf);
        }
    };
    auto build_half = [&](uint32_t h, const uint2* pr) {   // d2 over the walks u -> x -> y
#pragma unroll
        for (int k = 0; k < kP2Half; ++k) {
            const uint32_t j = h * 64 + (uint32_t)k * (kP2Block / 64) + wave;
            if (j >= n) continue;
            const uint32_t l1 = ku[j].y, t = l1 + pr[k].y;
            if (pr[k].x < V && pr[k].x != u && pr[k].y != kLat32Inf && t >= l1 && t != kLat32Inf)
                atomicMin(&d2[pr[k].x], t);
        }
    };
    auto test_half = [&](uint32_t h, const uint2* pr) {   // (u, v = list j's node) against u ~> y -> v
        uint32_t lyv[kP2Half], dy[kP2Half];
#pragma unroll
        for (int k = 0; k < kP2Half; ++k) {
            const uint32_t j = h * 64 + (uint32_t)k * (kP2Block / 64) + wave;
            lyv[k] = kLat32Inf;
            dy[k] = kLat32Inf;
            if (j >= n) continue;
            const uint32_t y = pr[k].x, v = ku[j].x;
            if (y >= V || y == u || y == v) continue;
            const uint32_t d = d2[y];
            // (a walk no shorter than the arc before its last step cannot beat it: no load)
            if (d != kLat32Inf && d < ku[j].y) {
                dy[k] = d;
                lyv[k] = dense_lat<DCSR>(Wl, V, y, v);
            }
        }
#pragma unroll
        for (int k = 0; k < kP2Half; ++k) {
            const uint32_t j = h * 64 + (uint32_t)k * (kP2Block / 64) + wave;
            if (j < n && lyv[k] != kLat32Inf && dy[k] != kLat32Inf && (uint64_t)dy[k] + lyv[k] < (uint64_t)ku[j].y)
                drop[j] = 1u;
        }
    };
    // the pairs stay in registers through both passes
    uint2 pr0[kP2Half];
    load_half(0, pr0);
    if (tid < n) atomicMin(&d2[ku[tid].x], ku[tid].y);   // the direct arcs u -> y
    build_half(0, pr0);
    __syncthreads();
    test_half(0, pr0);
    __syncthreads();
    // survivors in stage-1 order (wave 0), then the pad slots
    if (tid < 64) {
        const bool k0 = lane < n && drop[lane] == 0u;
        const uint64_t b0 = __ballot(k0);
        const uint32_t n2 = (uint32_t)__popcll(b0);
        if (k0) parcs[at + (uint32_t)__popcll(b0 & ((1ull << lane) - 1ull))] = ku[lane];
        const uint32_t np = (n2 + kPad2 - 1) / kPad2 * kPad2;
        if (n2 + lane < np) parcs[at + n2 + lane] = make_uint4(V + ((n2 + lane) & 63u), 0u, 0u, 0u);
        if (lane == 0) {
            pbeg[u] = at;
            pend[u] = at + n2;
        }
    }
}

// The fused prune (the K = 32 default; SHD_PRUNE_FUSED=0: prune_rows + prune_rows2 above): two
// launches whose rows each make three to four dependent memory trips, instead of two whose rows
// make nine.  prune_rows' survivor pass over detours 8..31 and the hand-over of its lists to
// prune_rows2 fall away: the 3-hop test is the stronger one and runs on the first batch's
// survivors directly, its candidates coming from a per-node nearest-neighbour table instead of
// other rows' stage-1 lists.
//
// nearest_rows: NN[x][0..kNear) = {node, latency} of x's kNear smallest (latency, index)
// out-arcs in ascending order (select_nearest, CMP: the detours prune_rows picks), unused
// entries {0xFFFFFFFF, +inf}; 256 B per node.
constexpr uint32_t kNear = 32;
static size_t nearest_lds_bytes(uint32_t V) { return 64 * 12 + (8 + 256 + 2 * kNear + (size_t)V) * 4 + (size_t)V * 2; }
template <int BLOCK, bool DCSR>
__global__ __launch_bounds__(BLOCK, BLOCK / 64) void nearest_rows(   // 8 waves per SIMD at BLOCK = 512
    const uint32_t* __restrict__ Wl, uint32_t V, uint2* __restrict__ NN, uint32_t* __restrict__ flags, uint32_t shg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* cand = reinterpret_cast<uint64_t*>(smem);
    uint32_t* rk = reinterpret_cast<uint32_t*>(cand + 64);
    uint32_t* cnt = rk + 64;
    uint32_t* hist = cnt + 8;
    uint32_t* selx = hist + 256;
    uint32_t* sela = selx + kNear;
    uint32_t* row = sela + kNear;
    uint16_t* binv = reinterpret_cast<uint16_t*>(row + V);
    const uint32_t x = blockIdx.x, tid = threadIdx.x;
    if (DCSR && x == 0 && tid < 16) flags[tid] = (tid == 4 || tid == 5) ? 0xFFFFFFFFu : 0u;   // as flags_init
    for (uint32_t v = tid; v < V; v += BLOCK) row[v] = v == x ? kLat32Inf : dense_lat<DCSR>(Wl, V, x, v);
    select_nearest<BLOCK, (int)kNear, true>(SelectLds{cnt, hist, selx, sela, row, binv, cand, rk}, V, 0u, shg, [](int) {});
    if (tid < kNear) {
        const uint32_t a = sela[tid];
        NN[(size_t)x * kNear + tid] = make_uint2(a != kLat32Inf ? selx[tid] : 0xFFFFFFFFu, a);
    }
}

// prune_fused, one workgroup per row u:
//   S1(u)  the arcs (u, v) that survive prune_rows' first batch: no detour u -> x -> v over the
//          kPfFirst nearest x = NN[u][0..kPfFirst) is strictly shorter (a detour node no nearer
//          than the arc is skipped); ~119 arcs of a C2 row, every arc of a constant-latency one.
//   d2[y]  min(lat(u, y), min over x in S1(u) and (y, l) in NN[x], y != u, of lat(u, x) + l)
//          -- a walk u (-> x) -> y.
//   (u, v), v in S1(u), is dropped iff some y in NN[v], y != u, y != v, has
//          d2[y] + lat(y, v) < lat(u, v), lat(y, v) the arc y -> v of the dense matrix (NN[v] only
//          names the candidates: on a directed graph lat(v, y) is another number).  SYM, an
//          undirected graph: the matrix is symmetric, so lat(y, v) is the latency NN[v] holds
//          beside y and the gather falls away (C2: 20.8 -> 14.7 us).
// Soundness is prune_rows2's: every compared detour is a walk of real arcs with their own
// latencies, so a tight arc is never dropped whatever the candidate sets are, and ties keep the
// arc.  The sums are guarded as there (a two-term sum that wraps or reaches +inf is no walk; the
// three-term sum is formed in 64 bits).
// Memory trips: the row's latencies and NN[u]; the first batch's gathers; NN[x] of the S1 nodes,
// 16 lanes per 256-B list, and with them the losses of the S1 arcs (no other arc needs its loss);
// the lat(y, v) gathers of the pairs with d2[y] below lat(u, v) (not SYM); the list write.  The
// row and the lists move 16 bytes per lane (load_row16, two NN entries per lane); the first
// batch stays one dword per lane and detour: four consecutive columns per thread in one 16-byte
// load measured slower, unaligned or as two aligned loads and a shift (routing item 2).
// The lists are taken kPfRound = 16 kPfLists at a time, kPfLists / 2 per 16-lane group with two
// entries per lane (SYM 12: one round covers C2's longest S1, 151; 8 with the gather's
// registers), so registers stay bounded for any |S1|: every round lowers d2 first (last round
// first, so round 0's lists are still in registers), then after one barrier every round is
// tested, rounds past the first reading their lists again (L2 hits).  d2 is complete before the
// first test, d2 is a minimum and a drop flag is only ever set, so the kept set is a function of
// the graph alone, whatever order the first batch's atomics filled S1 in; only the order of a
// final list follows it.  No list is cut off or copied through.
// The final list goes to row u's fixed offset, padded to kPad2 slots with prune_rows2's no-op arcs.
constexpr int kPfBlock = 512, kPfFirst = 8;
static size_t fused_lds_bytes(uint32_t V) { return (size_t)V * 20 + (2 * kNear + 8) * 4; }
template <bool DCSR, bool SYM>
__global__ __launch_bounds__(kPfBlock, 8) void prune_fused(   // 8 waves per SIMD: four workgroups per CU
    const uint32_t* __restrict__ Wl, const float* __restrict__ Wp, uint32_t V, const uint2* __restrict__ NN,
    uint32_t* __restrict__ pbeg, uint32_t* __restrict__ pend, uint4* __restrict__ parcs) {
    static_assert(kNear == 32 && (kPfFirst == 8 || kPfFirst == 16), "16 lanes, two entries each, per list");
    constexpr int kPfLists = SYM ? 12 : 8;   // list entries per lane and round (the gather form holds dy / lyv too)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint2* s1 = reinterpret_cast<uint2*>(smem);         // [V] S1(u): {v, lat(u, v)}, in arrival order
    uint32_t* d2 = reinterpret_cast<uint32_t*>(s1 + V); // [V] u's latency row, then the 2-hop row
    float* prow = reinterpret_cast<float*>(d2 + V);     // [V] the S1 arcs' losses, by S1 slot
    uint32_t* drop = reinterpret_cast<uint32_t*>(prow + V);   // [V] S1 arc j falls
    uint32_t* nnx = drop + V;                           // NN[u]: nodes
    uint32_t* nna = nnx + kNear;                        //        latencies
    uint32_t* cnt = nna + kNear;                        // [0] |S1| [1] kept
    const uint32_t u = blockIdx.x, tid = threadIdx.x;
    const uint32_t rs = DCSR ? V - 1 : V;               // row stride of the matrix (V <= 4096: indices fit u32)
    load_row16<kPfBlock, DCSR>(Wl, V, u, d2);
    for (uint32_t v = tid; v < V; v += kPfBlock) drop[v] = 0u;
    if (tid < kNear) {
        const uint2 e = NN[(size_t)u * kNear + tid];
        nnx[tid] = e.x;
        nna[tid] = e.y;
    }
    if (tid < 8) cnt[tid] = 0u;
    __syncthreads();
    // the first batch: VB arcs per thread against the kPfFirst nearest detours, 16 loads in flight
    constexpr int VB = 16 / kPfFirst;
    for (uint32_t v0 = tid; v0 < V; v0 += kPfBlock * VB) {
        uint32_t w[VB], z[VB], bv[VB][kPfFirst], as[kPfFirst];
#pragma unroll
        for (int i = 0; i < VB; ++i) {
            const uint32_t v = v0 + i * kPfBlock;
            w[i] = v < V ? d2[v] : kLat32Inf;
            z[i] = kLat32Inf;
        }
#pragma unroll
        for (int j = 0; j < kPfFirst; ++j) {
            as[j] = nna[j];
            const uint32_t x = nnx[j];
#pragma unroll
            for (int i = 0; i < VB; ++i) {
                const uint32_t v = v0 + i * kPfBlock;
                // (an unused entry has latency +inf, a missing arc w = +inf: neither loads)
                bv[i][j] = w[i] != kLat32Inf && as[j] < w[i] && v != x ? Wl[x * rs + v - (DCSR && v > x ? 1u : 0u)]
                                                                       : kLat32Inf;
            }
        }
#pragma unroll
        for (int i = 0; i < VB; ++i) {
#pragma unroll
            for (int j = 0; j < kPfFirst; ++j) {
                const uint32_t t = as[j] + bv[i][j];
                if (bv[i][j] != kLat32Inf && t >= as[j]) z[i] = min(z[i], t);
            }
            if (w[i] != kLat32Inf && w[i] <= z[i]) s1[atomicAdd(&cnt[0], 1u)] = make_uint2(v0 + i * kPfBlock, w[i]);
        }
    }
    __syncthreads();
    // NN lists in 16-byte loads: two entries per lane, 16 lanes per 256-B list, four lists per
    // wave instruction; kPfLists / 2 lists per 16-lane group hold the registers kPfLists did
    static_assert(kPfLists % 2 == 0, "two entries per lane");
    constexpr int kPfL4 = kPfLists / 2;
    constexpr uint32_t kPfGroups = kPfBlock / 16, kPfRound = kPfGroups * kPfL4;
    const uint32_t n1 = cnt[0], rounds = (n1 + kPfRound - 1) / kPfRound;
    const uint32_t qw = tid >> 4, sl = tid & 15;
    uint4 pr[kPfL4];   // entries 2 sl, 2 sl + 1 of this group's lists: {y, lat(x, y)} twice
    auto load_round = [&](uint32_t r) {
#pragma unroll
        for (int k = 0; k < kPfL4; ++k) {
            const uint32_t j = r * kPfRound + (uint32_t)k * kPfGroups + qw;
            pr[k] = make_uint4(0xFFFFFFFFu, kLat32Inf, 0xFFFFFFFFu, kLat32Inf);
            if (j < n1) pr[k] = *reinterpret_cast<const uint4*>(NN + (size_t)s1[j].x * kNear + 2u * sl);
        }
    };
    // the S1 arcs' losses (the row's other arcs never need theirs), by S1 slot: the first
    // kPfBlock ride the first round's memory trip in a register, the rest (heavily tied rows) follow
    float pl = 0.0f;
    if (tid < n1) {
        const uint32_t v = s1[tid].x;
        pl = Wp[u * rs + v - (DCSR && v > u ? 1u : 0u)];
    }
    for (uint32_t r = rounds; r-- > 0;) {   // d2 over the walks u -> x -> y
        load_round(r);
#pragma unroll
        for (int k = 0; k < kPfL4; ++k) {
            const uint32_t j = r * kPfRound + (uint32_t)k * kPfGroups + qw;
            if (j >= n1) continue;
            const uint32_t l1 = s1[j].y;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t y = h ? pr[k].z : pr[k].x, l = h ? pr[k].w : pr[k].y, t = l1 + l;
                if (y < V && y != u && l != kLat32Inf && t >= l1 && t != kLat32Inf) atomicMin(&d2[y], t);
            }
        }
    }
    if (tid < n1) prow[tid] = pl;
    for (uint32_t j = kPfBlock + tid; j < n1; j += kPfBlock) {
        const uint32_t v = s1[j].x;
        prow[j] = Wp[u * rs + v - (DCSR && v > u ? 1u : 0u)];
    }
    __syncthreads();
    for (uint32_t r = 0; r < rounds; ++r) {   // (u, v = list j's node) against u ~> y -> v
        if (r) load_round(r);
        uint32_t dy[kPfLists], lyv[kPfLists];
#pragma unroll
        for (int k = 0; k < kPfL4; ++k) {
            const uint32_t j = r * kPfRound + (uint32_t)k * kPfGroups + qw;
            const uint2 e = j < n1 ? s1[j] : make_uint2(0u, 0u);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                dy[2 * k + h] = kLat32Inf;
                lyv[2 * k + h] = kLat32Inf;
                if (j >= n1) continue;
                const uint32_t y = h ? pr[k].z : pr[k].x;
                if (y >= V || y == u || y == e.x) continue;
                const uint32_t d = d2[y];
                // (a walk no shorter than the arc before its last step cannot beat it: no load)
                if (d < e.y) {
                    dy[2 * k + h] = d;
                    // SYM (undirected graphs): lat(y, v) = lat(v, y), which NN[v] holds -- no gather
                    lyv[2 * k + h] = SYM ? (h ? pr[k].w : pr[k].y) : Wl[y * rs + e.x - (DCSR && e.x > y ? 1u : 0u)];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kPfL4; ++k) {
            const uint32_t j = r * kPfRound + (uint32_t)k * kPfGroups + qw;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t d = dy[2 * k + h], l = lyv[2 * k + h];
                if (j < n1 && l != kLat32Inf && d != kLat32Inf && (uint64_t)d + l < (uint64_t)s1[j].y) drop[j] = 1u;
            }
        }
    }
    __syncthreads();
    const uint32_t at = u * ((V + kPad1 - 1) / kPad1 * kPad1);   // the row's fixed offset (prune_rows2's)
    for (uint32_t j = tid; j < n1; j += kPfBlock) {
        if (drop[j]) continue;
        const uint2 e = s1[j];
        parcs[at + atomicAdd(&cnt[1], 1u)] = make_uint4(e.x, e.y, __float_as_uint(one_minus(prow[j])), 0u);
    }
    __syncthreads();
    const uint32_t n2 = cnt[1], np = (n2 + kPad2 - 1) / kPad2 * kPad2;
    for (uint32_t i = n2 + tid; i < np; i += kPfBlock) parcs[at + i] = make_uint4(V + (i & 63u), 0u, 0u, 0u);
    if (tid == 0) {
        pbeg[u] = at;
        pend[u] = at + n2;
    }
}

constexpr uint32_t kPruneK = 32;   // detour nodes per row

// Dense arc matrix + k-nearest 2-hop prune over all V rows -> pruned arc lists (row stride V),
// then the 3-hop stage over those lists (prune_rows2; SHD_PRUNE_STAGE2=0: stage 1 alone, 64-slot lists);
// by default both in one pass over the first batch's survivors (nearest_rows + prune_fused).
shd_status run_prune(shd_ctx* ctx, ArcView* out) {
    PreparedGraph& P = ctx->prep;
    hipStream_t s = ctx->stream;
    const uint32_t V = P.V;
    const uint64_t nn = (uint64_t)V * V;
    const bool stage2 = ctx->knobs.get(K_PRUNE_STAGE2, 1) != 0;
    SHD_TRY(ctx->g_prune_cnt.ensure((size_t)V * 16 + 16));
    uint32_t* pbeg = ctx->g_prune_cnt.as<uint32_t>();
    uint32_t* pend = pbeg + V;
    uint32_t* pbeg2 = pend + V + 4;   // the final lists' ranges (stage 2)
    uint32_t* pend2 = pbeg2 + V;
    uint32_t* flags = ctx->g_flags.as<uint32_t>();
    const size_t plds = (size_t)V * 22 + (8 + 256 + 2 * (size_t)kPruneK) * 4;
    // the sorted-detour kernel (CMP) with the first batch's survivors packed; SHD_PRUNE_SHAPE=0
    // keeps the round-4 kernel for A/B (same tables)
    const size_t plds_c = plds + 8 + (size_t)V * 12 + 64 * 12;   // + survivors (uint2 each), sort scratch, losses
    const bool legacy = ctx->knobs.get(K_PRUNE_SHAPE, 1) == 0;
    // CMP: bins from the graph's largest arc latency instead of each row's
    const uint32_t gbits = 64u - (uint32_t)__builtin_clzll(std::max<uint64_t>(std::min<uint64_t>(P.max_arc_lat, kLat32Inf - 1), 1));
    const uint32_t shg = gbits > 8 ? gbits - 8 : 0;
    const bool dcsr = P.dense_rows && !ctx->knobs.on(K_PRUNE_DENSE_BUILD);
    // the default shape and stage 2 on: nearest_rows + prune_fused (SHD_PRUNE_FUSED=0: the two
    // kernels below).  The path id tells count_kept which kernels made the lists it counted.
    const bool fused = !legacy && stage2 && ctx->knobs.get(K_PRUNE_FUSED, 1) != 0;
    const uint32_t path = (legacy ? 1u << 8 : 0u) | (stage2 ? 1u << 9 : 0u) | (fused ? 1u << 10 : 0u);
    const uint64_t stride = ((uint64_t)V + kPad1 - 1) / kPad1 * kPad1;   // a row's fixed offset: u * stride
    if (fused) {
        SHD_TRY(ctx->g_prune_nn.ensure(std::max<uint64_t>(V, 1) * kNear * 8));
        SHD_TRY(ctx->g_prune_dst2.ensure(std::max<uint64_t>(V * stride, 1) * 16));
        uint2* nnb = ctx->g_prune_nn.as<uint2>();
        uint4* pa2 = ctx->g_prune_dst2.as<uint4>();
        const size_t ldn = nearest_lds_bytes(V), ldf = fused_lds_bytes(V);
        // an undirected graph's matrix is symmetric: lat(y, v) comes with NN[v], no gather (SYM)
        const bool sym = !P.directed;
        if (dcsr) {
            const uint32_t* Wl = ctx->g_lat.as<uint32_t>();
            nearest_rows<512, true><<<V, 512, ldn, s>>>(Wl, V, nnb, flags, shg);
            const float* Wp = ctx->g_aux.as<float>();
            if (sym) prune_fused<true, true><<<V, kPfBlock, ldf, s>>>(Wl, Wp, V, nnb, pbeg2, pend2, pa2);
            else prune_fused<true, false><<<V, kPfBlock, ldf, s>>>(Wl, Wp, V, nnb, pbeg2, pend2, pa2);
        } else {
            SHD_TRY(ctx->g_dense.ensure(nn * 8));
            SHD_TRY(ctx->g_labels.ensure(nn * 4));
            float* Wp = ctx->g_dense.as<float>();
            uint32_t* Wl = ctx->g_labels.as<uint32_t>();
            dense_build<<<V, 256, (size_t)V * 8, s>>>(ctx->g_off.as<uint32_t>(), ctx->g_dst.as<uint32_t>(),
                                                      ctx->g_lat.as<uint32_t>(), ctx->g_aux.as<float>(), V, Wp, Wl, flags);
            nearest_rows<512, false><<<V, 512, ldn, s>>>(Wl, V, nnb, flags, shg);
            if (sym) prune_fused<false, true><<<V, kPfBlock, ldf, s>>>(Wl, Wp, V, nnb, pbeg2, pend2, pa2);
            else prune_fused<false, false><<<V, kPfBlock, ldf, s>>>(Wl, Wp, V, nnb, pbeg2, pend2, pa2);
        }
        SHD_HIP(hipGetLastError());
        *out = ArcView{pbeg2, pend2, pa2, 0, kPad2, nullptr, path};
        return SHD_OK;
    }
    SHD_TRY(ctx->g_prune_dst.ensure((nn + (uint64_t)V * kPad1) * 16));   // + list padding
    uint4* pa = ctx->g_prune_dst.as<uint4>();
    if (dcsr) {
        // the CSR is the dense matrix (complete graph, arcs in index order): prune straight from it
        const uint32_t* Wl = ctx->g_lat.as<uint32_t>();
        const float* Wp = ctx->g_aux.as<float>();
        if (legacy) prune_rows<256, kPruneK, true><<<V, 256, plds, s>>>(Wl, Wp, V, pbeg, pend, pa, flags);
        else prune_rows<512, kPruneK, true, 2, 8, true, 12><<<V, 512, plds_c, s>>>(Wl, Wp, V, pbeg, pend, pa, flags, shg);
    } else {
        SHD_TRY(ctx->g_dense.ensure(nn * 8));
        SHD_TRY(ctx->g_labels.ensure(nn * 4));
        float* Wp = ctx->g_dense.as<float>();   // the lexicographic-min arc's loss per pair (its latency: Wl)
        uint32_t* Wl = ctx->g_labels.as<uint32_t>();
        dense_build<<<V, 256, (size_t)V * 8, s>>>(ctx->g_off.as<uint32_t>(), ctx->g_dst.as<uint32_t>(),
                                                  ctx->g_lat.as<uint32_t>(), ctx->g_aux.as<float>(), V, Wp, Wl, flags);
        if (legacy) prune_rows<256, kPruneK><<<V, 256, plds, s>>>(Wl, Wp, V, pbeg, pend, pa, flags);
        else prune_rows<512, kPruneK, false, 2, 8, true, 12><<<V, 512, plds_c, s>>>(Wl, Wp, V, pbeg, pend, pa, flags, shg);
    }
    SHD_HIP(hipGetLastError());
    *out = ArcView{pbeg, pend, ctx->g_prune_dst.as<uint4>(), 0, kPad1, nullptr, path};
    if (!stage2) return SHD_OK;
    // stage 2 reads other rows' stage-1 lists while it runs: its lists go to a second buffer, each
    // at its row's stage-1 offset (a final list is no longer than the stage-1 one)
    SHD_TRY(ctx->g_prune_dst2.ensure(std::max<uint64_t>(V * stride, 1) * 16));
    uint4* pa2 = ctx->g_prune_dst2.as<uint4>();
    const size_t lds2 = prune2_lds_bytes(V);
    if (dcsr) prune_rows2<true><<<V, kP2Block, lds2, s>>>(ctx->g_lat.as<uint32_t>(), V, pbeg, pend, pa, pbeg2, pend2, pa2);
    else prune_rows2<false><<<V, kP2Block, lds2, s>>>(ctx->g_labels.as<uint32_t>(), V, pbeg, pend, pa, pbeg2, pend2, pa2);
    SHD_HIP(hipGetLastError());
    *out = ArcView{pbeg2, pend2, pa2, 0, kPad2, nullptr, path};
    return SHD_OK;
}

shd_status count_kept(shd_ctx* ctx, const ArcView& A) {
    std::vector<uint32_t> b(ctx->prep.V), e(ctx->prep.V);
    SHD_HIP(hipMemcpyAsync(b.data(), A.beg, b.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    SHD_HIP(hipMemcpyAsync(e.data(), A.end, e.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    SHD_HIP(hipStreamSynchronize(ctx->stream));
    uint64_t k = 0;
    for (size_t i = 0; i < b.size(); i++) k += e[i] - b[i];
    ctx->info.arcs_kept = k;
    ctx->prep.pruned_arcs = k;
    ctx->prep.pruned_pad = A.pad;
    ctx->prep.pruned_path = A.path;
    return SHD_OK;
}

}  // namespace shd

#ifdef SHD_SSSP_PROF
extern "C" int shd_debug_prune_prof(unsigned long long* out, int reset) {   // 4096 x 8 words
    (void)reset;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(shd::g_prune_prof), sizeof(unsigned long long) * 4096 * 8) != hipSuccess;
}
#endif
