// One source row of the label-correcting SSSP, device templates only: the relaxations, the sweep
// loop (sssp_row) and the end of a row (row_emit).  Included by routing_sssp_lds.hip (labels in
// LDS) and routing_sssp_global.hip (labels in global memory); routing_priv.h has the overview.
// (SHD_SSSP_PROF tuning builds add the phase counters, a copy per unit.)
// sssp_row serves both: sssp_global_group<512, 4, 4, true> sits at exactly 128 VGPRs, the budget
// its two slots per CU need, so check that kernel's register count after any change here.
#pragma once
#include "routing_priv.h"

namespace shd {

// ------------------------------------------------------------------------------------------
// Kernel 1: batched per-source SSSP, one workgroup per source row, labels in LDS.
// Label = packed u64 key (lat32 << 32 | f32 loss bits); ds_min_rtn_u64 keeps the lexicographic
// minimum exactly.  Active set = LDS bitmap; sweeps until a sweep improves nothing.
// Arcs are 16-byte AoS records {dst, lat32,
// q = 1f32 - loss bits, 0} so one dwordx4 load fetches an arc; a group of G lanes relaxes one
// active node's arcs together (G ~ average degree), so a node costs one load latency instead
// of `degree` dependent ones.  64/G nodes are in flight per wave, NW waves per source.
// ------------------------------------------------------------------------------------------
// delta = bucket width in ns for delta-stepping (SHD_ALGO_DELTA): a sweep only expands active
// nodes whose latency is <= (min active latency + delta), which keeps the expansion order close
// to Dijkstra's and cuts re-expansions.  delta = 0xFFFFFFFF expands every active node (plain
// chaotic Bellman-Ford).  Both converge to the same unique fixed point.
// Label loads: labels in LDS are read at workgroup scope; labels in global memory (kernel 1b)
// at agent scope, which bypasses the CU's L1 -- the L2 atomics never update it.
template <bool GLAB>
__device__ __forceinline__ uint64_t ld_lab(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED,
                             GLAB ? __HIP_MEMORY_SCOPE_AGENT : __HIP_MEMORY_SCOPE_WORKGROUP);
}

// delta-stepping bucket of a latency for the global-label kernel's LDS bucket bytes: any
// estimate works (it only orders the expansions), so a float multiply, saturating at 255
// The byte holds the latency in steps of delta / kBktSub: the sweeps schedule by byte >>
// kBktShift (delta-wide buckets) while the relax filter compares whole bytes, kBktSub times finer.
constexpr uint32_t kBktShift = 0, kBktSub = 1u << kBktShift;   // shift 2 (4x finer filter) measured no faster on C4
__device__ __forceinline__ uint8_t bucket_of(uint32_t lat, float inv_delta) {
    return (uint8_t)fminf(255.0f, (float)lat * inv_delta);
}

// LDS labels only: the global-label kernel expands edge-parallel (expand_flat, expand_flat8)
template <int G, int R, bool CACHE>
__device__ __forceinline__ void relax_node(uint32_t u, uint32_t gl, uint64_t* lab, uint32_t* bits,
                                           uint32_t scratch, const uint2* rng, const uint32_t* offl,
                                           const uint32_t* __restrict__ abeg,
                                           const uint32_t* __restrict__ aend,
                                           const uint4* __restrict__ arcs, bool& ovf, bool& dirty,
                                           uint32_t& mnext) {
    const uint64_t ku = ld_lab<false>(&lab[u]);
    const uint32_t lu = key_lat(ku);
    const float qu = one_minus(key_loss(ku));
    const uint2 r = CACHE ? rng[u] : offl ? make_uint2(offl[u], offl[u + 1]) : make_uint2(abeg[u], aend[u]);
    for (uint32_t k0 = r.x + gl; k0 < r.y; k0 += G * R) {
        // R arc loads, then R label atomics, all issued back to back: the loads are clamped into
        // the node's range and the atomics are unconditional (a dead slot carries the +inf key,
        // which min leaves unchanged, aimed at the lane's own scratch label so no two lanes
        // collide), so no branch splits them and each group waits for one load and one LDS
        // round trip per R arcs instead of R of each
        uint4 a[R];
        bool live[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const uint32_t k = k0 + i * G;
            live[i] = k < r.y;
            a[i] = arcs[live[i] ? k : r.y - 1];
        }
        uint64_t cand[R], old[R];
        uint32_t tgt[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const uint32_t cl = lu + a[i].y;
            const bool ok = live[i] && a[i].y != kLat32Inf && cl >= lu && cl != kLat32Inf;
            if (live[i] && a[i].y != kLat32Inf && !ok) ovf = true;   // leaves u32: wide rerun
            cand[i] = ok ? pack_key(cl, fold_q(qu, __uint_as_float(a[i].z))) : kKeyInf;
            tgt[i] = ok ? a[i].x : scratch;
        }
        // unconditional atomics, one LDS round trip for the R arcs (a filtering read first
        // measured slower: C2 172 -> 205 us, C3 11.2 -> 13.5 ms)
#pragma unroll
        for (int i = 0; i < R; ++i)
            old[i] = atomicMin(reinterpret_cast<unsigned long long*>(&lab[tgt[i]]), (unsigned long long)cand[i]);
        uint32_t imp = 0;
#pragma unroll
        for (int i = 0; i < R; ++i) imp |= (cand[i] < old[i] ? 1u : 0u) << i;
        if (imp) {
            dirty = true;
#pragma unroll
            for (int i = 0; i < R; ++i)
                if ((imp >> i) & 1u) {
                    atomicOr(&bits[a[i].x >> 5], 1u << (a[i].x & 31));
                    mnext = min(mnext, key_lat(cand[i]));
                }
        }
    }
}

// Padded arc lists (pruned dense graphs, prune_rows / prune_rows2): every node's list is a multiple
// of the pad width ArcView::pad (64 or 32 slots, a multiple of the group step G x R), the tail
// filled with no-op arcs {scratch label V + i, lat 0, q 0} whose
// candidate (lu, 1.0f) meets a scratch label holding 0.  The group then loads its G x R slots
// at immediate offsets from one address, with no clamp, liveness test or per-arc select, and
// the u32 overflow test is one compare per node: a label above lat_guard (2^32 - 2 - the
// largest arc latency) flags the build for the wide rerun before any add can wrap.  The
// kernel is issue-bound (C2 PMC: VALU pipe ~70% busy), so these per-arc instructions are the
// cost that matters.
template <int G, int R, bool CACHE>
__device__ __forceinline__ void relax_node_pad(uint32_t u, uint32_t gl, uint64_t* lab, uint32_t* bits,
                                               const uint2* rng, const uint32_t* __restrict__ abeg,
                                               const uint32_t* __restrict__ aend,
                                               const uint4* __restrict__ arcs, uint32_t lat_guard,
                                               bool& ovf, bool& dirty, uint32_t& mnext) {
    static_assert(G * R == 32 || G * R == 64, "a padded list holds whole G x R steps");
    const uint64_t ku = lab[u];
    const uint32_t lu = key_lat(ku);
    // the build is flagged and this node's arcs are left alone: their unchecked sums could wrap to
    // labels below every real one, each of which wraps on in turn -- the labels then sink a few
    // ns per sweep and these sweeps have no cap (arcs in [2^31, 2^32 - 3] on 33 nodes: more than
    // 200,000 sweeps).  The table is the wide rerun's either way
    if (lu > lat_guard) {
        ovf = true;
        return;
    }
    const float qu = one_minus(key_loss(ku));
    const uint2 r = CACHE ? rng[u] : make_uint2(abeg[u], aend[u]);
    for (uint32_t k0 = r.x; k0 < r.y; k0 += G * R) {
        const uint4* ap = arcs + k0 + gl;
        uint4 a[R];
#pragma unroll
        for (int i = 0; i < R; ++i) a[i] = ap[i * G];
        uint64_t cand[R], old[R];
#pragma unroll
        for (int i = 0; i < R; ++i) cand[i] = pack_key(lu + a[i].y, fold_q(qu, __uint_as_float(a[i].z)));
        // (a plain read first and the atomic only for a better candidate measured slower: C2 SSSP
        // 61 -> 66 us)
#pragma unroll
        for (int i = 0; i < R; ++i)
            old[i] = atomicMin(reinterpret_cast<unsigned long long*>(&lab[a[i].x]), (unsigned long long)cand[i]);
        uint32_t imp = 0;
#pragma unroll
        for (int i = 0; i < R; ++i) imp |= (cand[i] < old[i] ? 1u : 0u) << i;
        if (imp) {
            dirty = true;
#pragma unroll
            for (int i = 0; i < R; ++i)
                if ((imp >> i) & 1u) {
                    atomicOr(&bits[a[i].x >> 5], 1u << (a[i].x & 31));
                    mnext = min(mnext, key_lat(cand[i]));
                }
        }
    }
}

// LDS kernels on unpadded lists: a queued node of more than kHubDeg arcs is relaxed by its whole
// wave (sssp_row).  C3 (BA m = 3, 10k nodes), full build on one box: off 8.80-8.85 ms, 16: 7.27,
// 32: 7.02, 64: 7.18, 128: 7.62 (the sweep that settled the threshold; it was a knob then.  The host passes it as hub_deg)
constexpr uint32_t kHubDeg = 32;
constexpr int kFlatR = 8;              // arcs per lane per round of expand_flat

// Global labels: expand up to 64 queued nodes at once, edge-parallel.  The nodes' arc ranges
// are laid end to end (a wave prefix sum of the degrees) and every lane takes kFlatR arcs of
// the concatenation, so a round of the wave issues 64 x kFlatR independent arc loads, label
// reads and atomics -- one chain of global round trips per ~512 relaxations instead of one per
// node group.  The owner of an arc is the last node whose prefix is <= its position.  BA and
// internet-like graphs mix hubs and low-degree nodes; this keeps every lane busy on both.
__device__ __forceinline__ void expand_flat(const uint32_t* q, uint32_t qn, uint32_t lane, uint64_t* lab,
                                            uint32_t* bits, const uint32_t* __restrict__ abeg,
                                            const uint32_t* __restrict__ aend, const uint4* __restrict__ arcs,
                                            uint32_t* fx, bool& ovf, bool& dirty, uint8_t* bkt, float inv_delta,
                                            uint32_t& mnext) {
    uint32_t* pre = fx;          // [65]
    uint32_t* beg = fx + 65;     // [64]
    uint32_t* nl = fx + 129;     // [64] latency of the node's label
    uint32_t* nq = fx + 193;     // [64] q = 1f32 - loss of the node's label
    for (uint32_t c0 = 0; c0 < qn; c0 += 64) {
        const uint32_t cn = min(64u, qn - c0);
        uint32_t deg = 0, b = 0;
        uint64_t ku = kKeyInf;
        if (lane < cn) {
            const uint32_t u = q[c0 + lane];
            b = abeg[u];
            deg = aend[u] - b;
            ku = ld_lab<true>(&lab[u]);
        }
        uint32_t incl = deg;
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        const uint32_t T = __shfl(incl, 63);
        pre[lane] = incl - deg;
        beg[lane] = b;
        nl[lane] = key_lat(ku);
        nq[lane] = __float_as_uint(one_minus(key_loss(ku)));
        if (lane == 0) pre[64] = T;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (uint32_t t0 = 0; t0 < T; t0 += 64 * kFlatR) {
            uint4 a[kFlatR];
            uint32_t lu[kFlatR];
            float qu[kFlatR];
            bool live[kFlatR];
#pragma unroll
            for (int r = 0; r < kFlatR; ++r) {
                const uint32_t t = t0 + r * 64 + lane;
                live[r] = t < T;
                const uint32_t tc = min(t, T - 1);   // dead slots load the last arc (in bounds)
                uint32_t lo = 0, hi = 64;   // last j with pre[j] <= tc (zero-degree nodes are skipped)
#pragma unroll
                for (int it = 0; it < 6; ++it) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (pre[mid] <= tc) lo = mid; else hi = mid;
                }
                lu[r] = nl[lo];
                qu[r] = __uint_as_float(nq[lo]);
                a[r] = arcs[beg[lo] + (tc - pre[lo])];
            }
            uint64_t cand[kFlatR], cur[kFlatR];
#pragma unroll
            for (int r = 0; r < kFlatR; ++r) {
                const uint32_t cl = lu[r] + a[r].y;
                const bool ok = live[r] && a[r].y != kLat32Inf && cl >= lu[r] && cl != kLat32Inf;
                if (live[r] && a[r].y != kLat32Inf && !ok) ovf = true;   // leaves u32: wide rerun
                cand[r] = ok ? pack_key(cl, fold_q(qu[r], __uint_as_float(a[r].z))) : kKeyInf;
            }
            // bucket-byte filter: bkt[v] >= the bucket of v's label (it is written only by a
            // relaxation that just lowered the label, and the label only falls further), so
            // a candidate in a higher bucket cannot improve it -- skip its global label read
            // (most relaxations of a sparse graph fail; the byte is in LDS)
            if (bkt) {
#pragma unroll
                for (int r = 0; r < kFlatR; ++r)
                    if (cand[r] != kKeyInf && bucket_of(key_lat(cand[r]), inv_delta) > bkt[a[r].x]) cand[r] = kKeyInf;
            }
#pragma unroll
            for (int r = 0; r < kFlatR; ++r) cur[r] = cand[r] != kKeyInf ? ld_lab<true>(&lab[a[r].x]) : 0ull;
#pragma unroll
            for (int r = 0; r < kFlatR; ++r) {
                // labels only decrease: a candidate not below the label read now cannot improve it
                if (cand[r] < cur[r]) {
                    const uint64_t old =
                        atomicMin(reinterpret_cast<unsigned long long*>(&lab[a[r].x]), (unsigned long long)cand[r]);
                    if (cand[r] < old) {
                        dirty = true;
                        if (bkt) {
                            const uint8_t bk = bucket_of(key_lat(cand[r]), inv_delta);
                            bkt[a[r].x] = bk;
                            mnext = min(mnext, (uint32_t)(bk >> kBktShift));
                        }
                        atomicOr(&bits[a[r].x >> 5], 1u << (a[r].x & 31));
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// expand_flat for the global-label kernel on compact arcs: {dst, lat} (8 B) per arc, q = 1f32 -
// loss in a side array read only by the relaxations that survive the bucket-byte filter.  Most
// relaxations of a sparse graph fail, so the arc stream a sweep reads halves and (C4: 400k arcs,
// 3.2 MB) fits one XCD's L2.
__device__ __forceinline__ void expand_flat8(const uint32_t* q, uint32_t qn, uint32_t lane, uint64_t* lab,
                                             uint32_t* bits, const uint32_t* __restrict__ abeg,
                                             const uint32_t* __restrict__ aend, const uint2* __restrict__ arcs8,
                                             const float* __restrict__ aq, uint32_t* fx, bool& ovf, bool& dirty,
                                             uint8_t* bkt, float inv_delta, uint32_t& mnext, uint64_t* llab,
                                             uint32_t kl, uint32_t* wmin) {
    uint32_t* pre = fx;          // [65]
    uint32_t* beg = fx + 65;     // [64]
    uint32_t* nl = fx + 129;     // [64] latency of the node's label
    uint32_t* nq = fx + 193;     // [64] q = 1f32 - loss of the node's label
    for (uint32_t c0 = 0; c0 < qn; c0 += 64) {
        const uint32_t cn = min(64u, qn - c0);
        uint32_t deg = 0, b = 0;
        uint64_t ku = kKeyInf;
        if (lane < cn) {
            const uint32_t u = q[c0 + lane];
            b = abeg[u];
            deg = aend[u] - b;
            ku = u < kl ? llab[u] : ld_lab<true>(&lab[u]);
        }
        uint32_t incl = deg;
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        const uint32_t T = __shfl(incl, 63);
        pre[lane] = incl - deg;
        beg[lane] = b;
        nl[lane] = key_lat(ku);
        nq[lane] = __float_as_uint(one_minus(key_loss(ku)));
        if (lane == 0) pre[64] = T;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (uint32_t t0 = 0; t0 < T; t0 += 64 * kFlatR) {
            uint2 a[kFlatR];
            uint32_t lu[kFlatR], k[kFlatR], cl[kFlatR];
            float qu[kFlatR];
            bool ok[kFlatR], sure[kFlatR];
            // (every round issues all kFlatR slots: skipping a short last round's empty slots
            // behind wave-uniform branches measured slower, C4 rows 0-4095 17.2 -> 18.2 ms)
#pragma unroll
            for (int r = 0; r < kFlatR; ++r) {
                const uint32_t t = t0 + r * 64 + lane;
                ok[r] = t < T;
                const uint32_t tc = min(t, T - 1);   // dead slots load the last arc (in bounds)
                uint32_t lo = 0, hi = 64;   // last j with pre[j] <= tc (zero-degree nodes are skipped)
#pragma unroll
                for (int it = 0; it < 6; ++it) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (pre[mid] <= tc) lo = mid; else hi = mid;
                }
                lu[r] = nl[lo];
                qu[r] = __uint_as_float(nq[lo]);
                k[r] = beg[lo] + (tc - pre[lo]);
                a[r] = arcs8[k[r]];
            }
#pragma unroll
            for (int r = 0; r < kFlatR; ++r) {
                cl[r] = lu[r] + a[r].y;
                const bool fit = cl[r] >= lu[r] && cl[r] != kLat32Inf;
                if (ok[r] && !fit) ovf = true;   // leaves u32: wide rerun
                // bucket-byte filter (see expand_flat): a higher bucket cannot improve the label;
                // a strictly lower one surely does (bkt >= the label's bucket), so its atomic
                // goes out without the filtering read -- one global round trip less on the
                // flush's chain (C4 rows 0-4095: 19.3 -> 17.6 ms)
                const uint32_t bq = bucket_of(cl[r], inv_delta), bv = bkt[a[r].x];
                ok[r] = ok[r] && fit && bq <= bv;
                sure[r] = bq < bv;
            }
            uint64_t cur[kFlatR];
            float qa[kFlatR];
#pragma unroll
            for (int r = 0; r < kFlatR; ++r) {
                cur[r] = !ok[r] ? 0ull : a[r].x < kl ? llab[a[r].x] : sure[r] ? kKeyInf : ld_lab<true>(&lab[a[r].x]);
                qa[r] = ok[r] ? aq[k[r]] : 0.0f;
            }
#pragma unroll
            for (int r = 0; r < kFlatR; ++r) {
                if (!ok[r]) continue;
                const uint64_t cand = pack_key(cl[r], fold_q(qu[r], qa[r]));
                // labels only decrease: a candidate not below the label read now cannot improve it
                if (cand < cur[r]) {
                    // the hottest nodes' labels live in LDS (kl, locality order: highest degree
                        // first), the rest in the slot's global row
                    const uint64_t old =
                        a[r].x < kl ? atomicMin(reinterpret_cast<unsigned long long*>(&llab[a[r].x]), (unsigned long long)cand)
                                    : atomicMin(reinterpret_cast<unsigned long long*>(&lab[a[r].x]), (unsigned long long)cand);
                    if (cand < old) {
                        dirty = true;
                        const uint8_t bk = (uint8_t)bucket_of(cl[r], inv_delta);
                        bkt[a[r].x] = bk;
                        mnext = min(mnext, (uint32_t)(bk >> kBktShift));
                        atomicOr(&bits[a[r].x >> 5], 1u << (a[r].x & 31));
                        // after the bit (sssp_row's word scan relies on this order): a release,
                        // so neither the compiler nor the LDS queue lets the minimum go first
                        if (wmin)
                            __hip_atomic_fetch_min(&wmin[a[r].x >> 5], (uint32_t)(bk >> kBktShift), __ATOMIC_RELEASE,
                                                   __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

#ifdef SHD_SSSP_PROF
// tuning builds only (tools/sssp_prof.py, tools/c4_prof.py): shader clocks per phase of sssp_row,
// summed over waves: init, bitmap scan, relaxation (flush), sweep end (reduce + barrier), output.
// A unit built under the macro counts into its own copy and reads it through its own hook:
// shd_debug_sssp_prof (routing_sssp_lds.hip), shd_debug_sssp_global_prof (routing_sssp_global.hip).
static __device__ unsigned long long g_sssp_prof[8];
static int sssp_prof_read(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sssp_prof), sizeof(unsigned long long) * 8) != hipSuccess) return 1;
    if (reset) {
        unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_sssp_prof), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
#define SS_MARK(slot) do { if (true) { const uint64_t t_ = __builtin_amdgcn_s_memtime(); \
    ss_acc[slot] += t_ - ss_t; ss_t = t_; } } while (0)
#else
#define SS_MARK(slot) do { } while (0)
#endif

// The end of a source row, after its labels are final: the next hops (if asked for) and the used
// columns of the table.  pred: V words, where the arc-range cache was (LDS kernels) or a global row.
template <int BLOCK, bool GLAB>
__device__ __forceinline__ void row_emit(
    uint64_t* lab, uint32_t* pred, const uint32_t* __restrict__ abeg, const uint32_t* __restrict__ aend,
    const uint4* __restrict__ arcs, uint32_t V, const uint32_t* __restrict__ used, uint32_t n_used, uint32_t src,
    uint32_t row, size_t orow, const uint64_t* __restrict__ diag_lat, const float* __restrict__ diag_loss,
    uint64_t* __restrict__ out_lat, float* __restrict__ out_loss, unsigned long long* __restrict__ unreach,
    uint32_t* nh_out, const uint64_t* llab, uint32_t kl) {
    const uint32_t tid = threadIdx.x;
    if (nh_out) {
        // Next hops (north star; the reference keeps none).  pred(v) = the lowest node
        // index u with an arc u -> v that is tight for the final labels (key(u) (+) arc == key(v),
        // bit for bit); every label is reached through such an arc (the fold is monotone), and
        // latency strictly grows along it, so the pred chain of any reached node ends at the
        // source.  next hop(src, d) = the node after src on d's pred chain.  pred lives where
        // the arc-range cache was (LDS kernel) or in a global scratch row (global labels).
        __syncthreads();
        for (uint32_t v = tid; v < V; v += BLOCK) pred[v] = 0xFFFFFFFFu;
        if (GLAB) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (uint32_t u = tid; u < V; u += BLOCK) {
            const uint64_t ku = ld_lab<GLAB>(&lab[u]);
            if (ku == kKeyInf) continue;
            const uint32_t lu = key_lat(ku);
            const float qu = one_minus(key_loss(ku));
            const uint32_t e = aend[u];
            for (uint32_t k = abeg[u]; k < e; ++k) {
                const uint4 a = arcs[k];
                const uint32_t cl = lu + a.y;
                if (a.x == u || a.y == kLat32Inf || cl < lu || cl == kLat32Inf) continue;
                if (pack_key(cl, fold_q(qu, __uint_as_float(a.z))) == ld_lab<GLAB>(&lab[a.x]))
                    atomicMin(&pred[a.x], u);
            }
        }
        if (GLAB) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (uint32_t j = tid; j < n_used; j += BLOCK) {
            const uint32_t v = GLAB || used ? used[j] : j;
            uint32_t nh = 0xFFFFFFFFu;
            if (v == src) {
                nh = src;
            } else {
                uint32_t w = v, pw = GLAB ? __hip_atomic_load(&pred[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : pred[w];
                for (uint32_t hop = 0; hop < V && pw != src && pw != 0xFFFFFFFFu; ++hop) {
                    w = pw;
                    pw = GLAB ? __hip_atomic_load(&pred[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : pred[w];
                }
                if (pw == src) nh = w;
            }
            __builtin_nontemporal_store(nh, &nh_out[orow + j]);
        }
    }
    constexpr uint32_t kOut = 4;   // columns per thread per iteration: their loads in flight together
    for (uint32_t j0 = tid; j0 < n_used; j0 += kOut * BLOCK) {
        uint32_t uj[kOut];
        uint64_t k[kOut];
#pragma unroll
        for (uint32_t i = 0; i < kOut; ++i) {
            const uint32_t j = j0 + i * BLOCK;
            uj[i] = j < n_used ? (GLAB || used ? used[j] : j) : 0u;
        }
#pragma unroll
        for (uint32_t i = 0; i < kOut; ++i) {
            const uint32_t j = j0 + i * BLOCK;
            k[i] = j < n_used && j != row ? (uj[i] < kl ? llab[uj[i]] : ld_lab<GLAB>(&lab[uj[i]])) : 0ull;
        }
#pragma unroll
        for (uint32_t i = 0; i < kOut; ++i) {
            const uint32_t j = j0 + i * BLOCK;
            if (j >= n_used) break;
            uint64_t l;
            float p;
            if (j == row) {
                l = diag_lat[j];
                p = diag_loss[j];
            } else if (k[i] == kKeyInf) {
                atomicMin(unreach, (unsigned long long)((uint64_t)row * n_used + j));
                l = ~0ull;
                p = 0.0f;
            } else {
                l = key_lat(k[i]);
                p = key_loss(k[i]);
            }
            // the table is written once and never read here: non-temporal stores keep it from
            // evicting the label rows (C4: 600 KB of table per source row) from L2 / Infinity Cache
            __builtin_nontemporal_store(l, &out_lat[orow + j]);
            __builtin_nontemporal_store(p, &out_loss[orow + j]);
        }
    }
}

// One source row: init, sweeps until nothing improves, emit the used columns.
// FASTG (global labels): flat expansion + bucket bytes + one-barrier delta sweeps only (C4)
template <int BLOCK, int G, int R, bool CACHE, bool GLAB, int PADR = 0, bool FASTG = false>
__device__ __forceinline__ void sssp_row(
    uint64_t* lab, uint32_t* bits, uint32_t* ctl, uint32_t* wq, uint2* rng,
    const uint32_t* __restrict__ abeg, const uint32_t* __restrict__ aend,
    const uint4* __restrict__ arcs, uint32_t V, const uint32_t* __restrict__ used,
    uint32_t n_used, uint32_t row, size_t orow, const uint64_t* __restrict__ diag_lat,
    const float* __restrict__ diag_loss, uint64_t* __restrict__ out_lat,
    float* __restrict__ out_loss, uint32_t* __restrict__ flags,
    unsigned long long* __restrict__ unreach, uint32_t delta,
    unsigned long long* __restrict__ stats, const uint32_t* __restrict__ seed_lat,
    uint32_t seed_stride, uint8_t* bkt, uint32_t* flat, uint32_t* nh_out, uint32_t* pred,
    uint32_t lat_guard, const uint2* __restrict__ arcs8 = nullptr, const float* __restrict__ aq = nullptr,
    uint32_t* offl = nullptr, uint64_t* llab = nullptr, uint32_t kl = 0, uint32_t* wmin = nullptr,
    uint32_t hub_deg = 0) {
    // bkt (global labels + delta-stepping): per node, the bucket of the latency that last
    // activated it, in LDS, so choosing a sweep's nodes reads no global label
    constexpr uint32_t NW = BLOCK / 64, NG = 64 / G;
    const uint32_t W = (V + 31) >> 5;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t grp = lane / G, gl = lane % G;
    uint32_t* q = wq + wave * kQStride;
    // (LDS kernels: nullptr = every node used, in index order; the global-label kernel always
    // passes the array -- a runtime check there cost the one VGPR above 128 that halves its
    // residency: C4 rows 0-4095 17.3 -> 27.2 ms)
    uint32_t src;
    if constexpr (GLAB) src = used[row];
    else src = used ? used[row] : row;
#ifdef SHD_SSSP_PROF
    uint64_t ss_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ss_t = __builtin_amdgcn_s_memtime();
#endif
    // PADR kernels run only delta-stepping with one-barrier sweeps and no seed (launch_group)
    const bool use_delta = PADR != 0 || FASTG || delta != kLat32Inf;
    // bucket bytes count steps of delta / kBktSub (global labels); the LDS kernels do not use them
    const float inv_delta = use_delta ? (float)kBktSub / (float)delta : 0.0f;
    // the ordering key of an active node: its bucket byte, or its label's latency
    auto act_key = [&](uint32_t v) -> uint32_t {
        // LDS labels: the latency half only, a 4-byte read (C3 DELTA 6.86 -> 6.79 ms; the 64-bit
        // atomics write both halves at once, so the half read is always one label's latency)
        if constexpr (!GLAB && !FASTG)
            if (!bkt)
                return __hip_atomic_load(reinterpret_cast<const uint32_t*>(&lab[v]) + 1, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_WORKGROUP);
        return FASTG || bkt ? (uint32_t)(bkt[v] >> kBktShift) : key_lat(ld_lab<GLAB>(&lab[v]));
    };

    // seed_lat (blocked path): labels start at (final latency, +inf loss) so only the loss
    // part can still improve, and only through tight arcs
    const uint32_t* seed = PADR == 0 && seed_lat ? seed_lat + (size_t)src * seed_stride : nullptr;
    for (uint32_t v = tid; v < V; v += BLOCK) {
        uint64_t l0 = kKeyInf;
        if (seed) {
            const uint32_t d = seed[v];
            if (d != kLat32Inf) l0 = ((uint64_t)d << 32) | 0xFFFFFFFFull;
        }
        if (GLAB) {
            if (v == src) l0 = 0;   // PathProperties::default() = (0 ns, 0.0)
            if (v < kl) llab[v] = l0;
            else __hip_atomic_store(&lab[v], l0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            lab[v] = l0;
        }
        if (CACHE) rng[v] = make_uint2(abeg[v], aend[v]);
        else if (offl) offl[v] = abeg[v];
    }
    for (uint32_t w = tid; w < W; w += BLOCK) bits[w] = 0;
    if (wmin)   // per bitmap word, a lower bound of its active nodes' bucket keys (none: +inf)
        for (uint32_t w = tid; w < W; w += BLOCK) wmin[w] = w == (src >> 5) ? 0u : kLat32Inf;
    if (bkt)   // unreached: the top bucket (the relax filter never skips against it)
        for (uint32_t w = tid; w < (V + 3) / 4; w += BLOCK) reinterpret_cast<uint32_t*>(bkt)[w] = 0xFFFFFFFFu;
    if (offl && tid == 0) offl[V] = aend[V - 1];   // CSR: aend == abeg + 1
    if (!GLAB && tid < 64) lab[V + tid] = 0;   // scratch labels: no candidate improves them
    // global labels: every storing wave drains its stores before the barrier, so the L2 holds
    // them before any wave's atomics
    if (GLAB) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // One-barrier sweeps (LDS labels + delta-stepping): the next sweep's bucket floor is the
    // minimum over the nodes still active after this one -- those the selection skipped, and
    // those a relaxation just improved -- gathered while the sweep runs, so no separate scan
    // and only one barrier per sweep.  Three rotating accumulators ctl[1..3]: sweep k writes
    // slot k%3, all read it after the barrier, and sweep k resets slot (k+1)%3, whose last
    // readers passed the barrier of sweep k-1.  A floor taken from a node that the same sweep
    // then expands is only lower than needed: the next sweep selects less, never wrongly.
    const bool fused = PADR != 0 || FASTG || (use_delta && (!GLAB || bkt));
    if (tid == 0) {
        if (!GLAB) lab[src] = 0;  // PathProperties::default() = (0 ns, 0.0)
        bits[src >> 5] = 1u << (src & 31);
        if (bkt) bkt[src] = 0;
        if (fused) ctl[1] = ctl[2] = ctl[3] = kLat32Inf;
    }
    if (fused) __syncthreads();
    SS_MARK(0);
    bool ovf = false;
    uint32_t expanded = 0, sweeps = 0;
    uint32_t slot = 0;   // fused: this sweep's accumulator, ctl[1 + slot]
    for (;;) {
        uint32_t thr = kLat32Inf;
        uint32_t mnext = kLat32Inf;   // fused: lowest latency active after this sweep (this lane)
        if (fused) {
            const uint32_t lo = sweeps == 0 ? 0u : ctl[1 + (slot + 2) % 3];
            if (lo == kLat32Inf) break;  // no active node anywhere
            if (tid == 0) ctl[1 + (slot + 1) % 3] = kLat32Inf;
            thr = bkt ? lo : lo + delta < lo ? kLat32Inf - 1 : lo + delta;
        } else {
            if (tid == 0) {
                ctl[0] = 0;
                ctl[1] = kLat32Inf;
            }
            __syncthreads();
        }
        if (use_delta && !fused) {
            uint32_t m = kLat32Inf;
            for (uint32_t widx = lane * NW + wave; widx < W; widx += NW * 64) {   // lane per word
                const uint32_t word = __hip_atomic_load(&bits[widx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                for (uint32_t mm = word; mm; mm &= mm - 1) m = min(m, act_key(widx * 32 + __builtin_ctz(mm)));
            }
            for (int o = 32; o > 0; o >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, o));
            if (lane == 0 && m != kLat32Inf) atomicMin(&ctl[1], m);
            __syncthreads();
            const uint32_t lo = ctl[1];
            if (lo == kLat32Inf) break;  // no active node anywhere
            thr = bkt ? lo : lo + delta < lo ? kLat32Inf - 1 : lo + delta;
        }
        bool dirty = false;
        uint32_t qn = 0;  // wave-uniform queue length
        // expand the queued nodes: NG nodes per step, G lanes each (or edge-parallel, global labels)
        auto flush = [&]() {
            SS_MARK(1);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            expanded += qn;
            if constexpr (GLAB) {
                if constexpr (FASTG) {
                    expand_flat8(q, qn, lane, lab, bits, abeg, aend, arcs8, aq, flat + wave * kFlatWords, ovf, dirty,
                                 bkt, inv_delta, mnext, llab, kl, wmin);
                } else {
                    expand_flat(q, qn, lane, lab, bits, abeg, aend, arcs, flat + wave * kFlatWords, ovf, dirty, bkt,
                                inv_delta, mnext);
                }
            } else {
                if constexpr (PADR == 0) {
                    // hubs (sparse power-law graphs, C3): a queued node of more than hub_deg arcs is
                    // relaxed by the whole wave first, 128 arcs per step, instead of by one lane group
                    // that the other groups of the wave -- and the sweep's other waves at its
                    // barrier -- would wait for.  (hub_deg is always kHubDeg; it stays a guarded
                    // device argument because the constant re-schedules the C3 kernel: see
                    // sssp_lds_group)
                    if (hub_deg) {
                        for (uint32_t t0 = 0; t0 < qn; t0 += 64) {
                            const uint32_t qi = t0 + lane;
                            const uint32_t u = qi < qn ? q[qi] : 0xFFFFFFFFu;
                            uint32_t deg = 0;
                            if (u != 0xFFFFFFFFu) {
                                const uint2 r = CACHE ? rng[u] : offl ? make_uint2(offl[u], offl[u + 1])
                                                                      : make_uint2(abeg[u], aend[u]);
                                deg = r.y - r.x;
                            }
                            uint64_t big = __ballot(deg > hub_deg);
                            while (big) {   // wave-uniform
                                const uint32_t b = (uint32_t)__ffsll((unsigned long long)big) - 1u;
                                big &= big - 1ull;
                                relax_node<64, 2, CACHE>((uint32_t)__shfl((int)u, (int)b), lane, lab, bits, V + lane,
                                                         rng, offl, abeg, aend, arcs, ovf, dirty, mnext);
                            }
                            if (deg > hub_deg) q[qi] = 0xFFFFFFFFu;   // done: the group pass skips it
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    }
                }
                for (uint32_t t = 0; t < qn; t += NG) {
                    const uint32_t qi = t + grp;
                    if (qi >= qn) continue;
                    if constexpr (PADR != 0) {   // padded lists: G x PADR slots (a whole 32-slot list) per group step
                        relax_node_pad<G, PADR, CACHE>(q[qi], gl, lab, bits, rng, abeg, aend, arcs, lat_guard,
                                                       ovf, dirty, mnext);
                    } else {
                        const uint32_t u = q[qi];
                        if (u != 0xFFFFFFFFu)
                            relax_node<G, R, CACHE>(u, gl, lab, bits, V + lane, rng, offl, abeg, aend, arcs, ovf,
                                                    dirty, mnext);
                    }
                }
            }
            qn = 0;
            __builtin_amdgcn_wave_barrier();
            SS_MARK(2);
        };
        // scan form: the LDS kernels take nibbles under delta-stepping or a seed and a word per
        // step otherwise, the global-label kernels (large V) only the lane-per-word one, so the
        // 128-VGPR kernel carries one loop
        // (plain chaotic sweeps, no delta, keep the word-per-step form: C3 SSSP 11.2 ms against
        // 17.4 with lane-per-word, whose frontier there is dense)
        constexpr bool lane_scan = GLAB;
        // (plain chaotic sweeps on an unpruned graph keep the word-per-step form: C2 SSSP 2.65 ms
        // against 2.95 with nibbles; the seeded loss pass of the blocked engine takes nibbles)
        if (!lane_scan && (use_delta || seed)) {
            // bits in parallel (LDS labels; C2: 32 words over 4 waves, C3: 313 over 16): a wave
            // takes 8 of its words at once, each lane 4 bits of one, so the key reads of all 8
            // words are in flight together -- one LDS round trip per 256 bits instead of one per
            // word step (the word-per-step form used half the lanes, one word at a time; the
            // lane-per-word form walked a word's bits one dependent read after another)
            for (uint32_t k0 = 0;; k0 += 8) {
                const bool more = k0 * NW + wave < W;   // wave-uniform
                const uint32_t widx = (k0 + (lane >> 3)) * NW + wave, nb = (lane & 7) * 4;
                uint32_t sel4 = 0;
                if (more && widx < W) {
                    const uint32_t word = __hip_atomic_load(&bits[widx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    const uint32_t nib = (word >> nb) & 0xFu;
                    uint32_t key[4];
#pragma unroll
                    for (uint32_t i = 0; i < 4; ++i)
                        key[i] = (nib >> i) & 1u ? (use_delta ? act_key(widx * 32 + nb + i) : 0u) : kLat32Inf;
#pragma unroll
                    for (uint32_t i = 0; i < 4; ++i) {
                        if (!((nib >> i) & 1u)) continue;   // (thr is +inf in plain chaotic sweeps)
                        if (key[i] <= thr) sel4 |= 1u << i;
                        else mnext = min(mnext, key[i]);
                    }
                    // words are owned by one wave; other waves only set bits: clearing is exact
                    if (sel4) atomicAnd(&bits[widx], ~(sel4 << nb));
                }
#pragma unroll
                for (uint32_t i = 0; i < 4; ++i) {
                    const bool has = (sel4 >> i) & 1u;
                    const uint64_t bal = __ballot(has);
                    if (bal == 0) continue;   // wave-uniform
                    if (has) q[qn + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = widx * 32 + nb + i;
                    qn += (uint32_t)__popcll(bal);
                    if (qn >= kQCap) flush();
                }
                if (!more) {
                    if (qn > 0) flush();
                    break;
                }
            }
        } else if (!lane_scan) {
            // small bitmap (C2: 32 words over 4 waves): a word per wave step, lane per bit
            for (uint32_t widx = wave;; widx += NW) {
                const bool more = widx < W;
                if (more) {
                    const uint32_t word = __hip_atomic_load(&bits[widx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (word != 0) {  // wave-uniform
                        bool sel = lane < 32 && ((word >> lane) & 1u);
                        if (use_delta && sel) {
                            const uint32_t key = act_key(widx * 32 + lane);
                            sel = key <= thr;
                            if (!sel) mnext = min(mnext, key);
                        }
                        const uint32_t mask = (uint32_t)__ballot(sel);
                        if (mask) {
                            // words are owned by one wave; other waves only set bits: clearing is exact
                            if (lane == 0) atomicAnd(&bits[widx], ~mask);
                            if (sel) q[qn + __popc(mask & ((1u << lane) - 1u))] = widx * 32 + lane;
                            qn += __popc(mask);
                        }
                    }
                }
                if (qn >= kQCap || (!more && qn > 0)) flush();
                if (!more) break;
            }
        }
        if (lane_scan) {
        // Lane per bitmap word: a wave reads 64 words at once, each lane picks its word's selected
        // nodes (bits clear first; other waves only set bits in a word this lane owns, so the
        // atomicAnd is exact), then the selected nodes enter the queue one per lane per step.  A
        // sweep's frontier is sparse (C4: about one active node per word), so this reads the
        // bitmap 64x faster than a word per wave step with half the lanes idle (C4 DELTA, 4096
        // rows: 50.8 -> 38.7 ms).  Words are dealt round-robin (word k*NW + wave to lane k).
        for (uint32_t k0 = 0;; k0 += 64) {
            const bool more = k0 * NW + wave < W;   // wave-uniform: the wave has words in this batch
            const uint32_t widx = (k0 + lane) * NW + wave;
            uint32_t rem = 0;           // this lane's selected nodes not yet queued
            // Per-word minimum (wmin, global labels): a word whose active nodes all lie above
            // the threshold is skipped on one LDS read instead of one bucket-byte read per active
            // node -- most active nodes of a sparse graph wait many sweeps for their bucket.
            // The scanning lane owns the word: it resets wmin, then reads the bits and puts the
            // keys of those it leaves back; a relaxation sets the bit first and lowers wmin
            // after, so every set bit is either seen by that read or lowers wmin afterwards.
            bool scan_word = more && widx < W;
            if (scan_word && wmin) {
                const uint32_t m = __hip_atomic_load(&wmin[widx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (m > thr) {
                    mnext = min(mnext, m);
                    scan_word = false;
                } else {   // an acquire: the bits below are read after the reset, never before
                    (void)__hip_atomic_exchange(&wmin[widx], kLat32Inf, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
            if (scan_word) {
                const uint32_t word = __hip_atomic_load(&bits[widx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (word) {
                    uint32_t selm = word;
                    if (use_delta) {
                        selm = 0;
                        uint32_t rest = kLat32Inf;
                        for (uint32_t mm = word; mm; mm &= mm - 1) {
                            const uint32_t b = __builtin_ctz(mm);
                            const uint32_t key = act_key(widx * 32 + b);
                            if (key <= thr) selm |= 1u << b;
                            else rest = min(rest, key);
                        }
                        mnext = min(mnext, rest);
                        if (wmin && rest != kLat32Inf) atomicMin(&wmin[widx], rest);
                    }
                    if (selm) atomicAnd(&bits[widx], ~selm);
                    rem = selm;
                }
            }
            for (;;) {
                const uint64_t bal = __ballot(rem != 0);
                if (more && bal == 0) break;   // this batch of words is queued
                if (rem) {
                    q[qn + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = widx * 32 + __builtin_ctz(rem);
                    rem &= rem - 1;
                }
                qn += (uint32_t)__popcll(bal);
                if (qn < kQCap && (more || qn == 0)) {
                    if (more) continue;
                    break;
                }
                flush();
                if (!more && bal == 0) break;
            }
            if (!more) break;
        }
        }
        ++sweeps;
        SS_MARK(1);
        if (fused) {
            for (int o = 32; o > 0; o >>= 1) mnext = min(mnext, (uint32_t)__shfl_xor((int)mnext, o));
            if (lane == 0 && mnext != kLat32Inf) atomicMin(&ctl[1 + slot], mnext);
            __syncthreads();
            SS_MARK(3);
            slot = slot == 2 ? 0 : slot + 1;
        } else if (!use_delta) {
            if (dirty) ctl[0] = 1;
            __syncthreads();
            const bool again = ctl[0] != 0;
            __syncthreads();
            if (!again) break;
        } else {
            __syncthreads();
        }
    }
    if (ovf) atomicOr(&flags[0], 1u);
    if (stats && lane == 0) {
        atomicAdd(&stats[0], (unsigned long long)expanded);
        if (wave == 0) atomicAdd(&stats[1], (unsigned long long)sweeps);
    }
    row_emit<BLOCK, GLAB>(lab, pred, abeg, aend, arcs, V, used, n_used, src, row, orow, diag_lat, diag_loss, out_lat,
                          out_loss, unreach, nh_out, llab, kl);
#ifdef SHD_SSSP_PROF
    SS_MARK(4);
    if (lane == 0) {
        for (int k = 0; k < 5; ++k) atomicAdd(&g_sssp_prof[k], (unsigned long long)ss_acc[k]);
        atomicAdd(&g_sssp_prof[5], (unsigned long long)sweeps);
        atomicAdd(&g_sssp_prof[6], (unsigned long long)expanded);
        atomicAdd(&g_sssp_prof[7], 1ull);
    }
#endif
}

}  // namespace shd
