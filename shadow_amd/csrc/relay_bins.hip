// Relay pipeline 7 after the stamp (overview and the list of units: relay_priv.h): the bin
// histograms and scans before it, K4 bin_sort_v7 after it -- for pipeline 8 over the records
// gathered from every rank -- and the pipeline's host side.
#include <algorithm>

#include "relay_bins.h"

namespace shd {

// ==========================================================================================
// Pipeline v7: destination-bin placement instead of a radix sort.  The stamp writes every
// packet's record straight into its destination bin (kBinDst destinations); the slots of a
// (stamp workgroup, bin) pair are counted beforehand by relay_bin_hist, which walks exactly the
// packets that workgroup will stamp.  bin_sort_v7 then loads one bin into LDS, drops the unsent
// records, splits the rest by destination and sorts each destination's run by
// (deliver, packet index) -- packet-index order is (src host, event id) order, the EventQueue
// tie-break -- so the slot order inside a bin never shows in the output.  Global traffic: the
// stamp's 16-byte record write plus one coalesced read of it, instead of two radix passes.
// ==========================================================================================
#ifndef SHD_B7_THREADS
#define SHD_B7_THREADS 512
#endif
constexpr uint32_t kB7Threads = SHD_B7_THREADS;
constexpr uint32_t kB7Per = (kB7Cap + kB7Threads - 1) / kB7Threads;
constexpr unsigned long long kLbAgg = 1ull << 62, kLbIncl = 2ull << 62, kLbMask = (1ull << 62) - 1;

// Histogram row r = g * kHistSplit + k counts, per destination bin, the packets of the host
// groups g + (k + j * kHistSplit) * G (j = 0, 1, ...) -- together the rows g * kHistSplit + k
// cover exactly the groups the stamp's workgroup g walks, every packet with a valid
// destination.  The rows' exclusive prefix at row g * kHistSplit is that workgroup's segment
// start.  A group's packet positions are flattened over the workgroup (owner by binary search
// in the 64-entry prefix) with kHistUnroll independent loads in flight per thread.
constexpr uint32_t kHistUnroll = 8;

__global__ __launch_bounds__(256) void relay_bin_hist(RelayArgs3 a, uint32_t G, uint32_t* __restrict__ cnt) {
    extern __shared__ uint32_t s_cnt[];
    __shared__ uint32_t s_beg[kS5Hosts], s_pre[kS5Hosts + 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    if (blockIdx.x == 0 && tid < 8) a.red[tid] = (tid <= 1 || tid == 3) ? ~0ull : 0ull;   // as red_init
    const uint32_t g = blockIdx.x / kHistSplit, k = blockIdx.x % kHistSplit;
    for (uint32_t i = tid; i < a.n_bins; i += 256) s_cnt[i] = 0;
    const uint32_t n_groups = (a.n_src + a.gs - 1) / a.gs;
    for (uint32_t grp = g + k * G; grp < n_groups; grp += kHistSplit * G) {
        const uint32_t h0 = grp * a.gs, nh = min(a.gs, a.n_src - h0);
        __syncthreads();
        if (tid < 64) {
            uint32_t len = 0;
            if (tid < nh) {
                const uint32_t h = a.order[h0 + tid];
                s_beg[tid] = a.src_off[h - a.src_lo];
                len = a.src_off[h - a.src_lo + 1] - s_beg[tid];
            }
            uint32_t incl = len;
            for (uint32_t o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(incl, o);
                if (lane >= o) incl += y;
            }
            if (tid < nh) s_pre[tid + 1] = incl;
            if (tid == 0) s_pre[0] = 0;
        }
        __syncthreads();
        const uint32_t T = s_pre[nh];
        for (uint32_t base = 0; base < T; base += 256 * kHistUnroll) {
            uint32_t d[kHistUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kHistUnroll; ++u) {
                const uint32_t p = base + u * 256 + tid;
                d[u] = ~0u;
                if (p < T) {
                    uint32_t lo = 0, hi = nh;   // s_pre[lo] <= p < s_pre[lo + 1]
                    while (hi - lo > 1) {
                        const uint32_t m = (lo + hi) >> 1;
                        if (s_pre[m] <= p) lo = m; else hi = m;
                    }
                    d[u] = a.dst_host[s_beg[lo] + (p - s_pre[lo])];
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < kHistUnroll; ++u)
                if (d[u] < a.n_hosts) {
                    uint32_t dl;
                    atomicAdd(&s_cnt[dst_bin(a, d[u], dl)], 1u);
                }
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < a.n_bins; i += 256) cnt[(size_t)blockIdx.x * a.n_bins + i] = s_cnt[i];
}

// relay_bin_hist, vector form (the batch's dst_host 16-byte aligned): the same rows, but four
// threads per host of a group walk the host's own range in aligned 16-byte chunks (chunk c =
// destinations [4c, 4c + 4), entries outside the host's range skipped), so no position needs a
// search for its owner and each load brings four destinations.  Chunks reaching past the batch
// end are read element by element.
constexpr uint32_t kHist4Threads = 1024;   // four groups at a time: 4 threads x 64 host slots each

__global__ __launch_bounds__(kHist4Threads) void relay_bin_hist4(RelayArgs3 a, uint32_t G, uint32_t n_pkt,
                                                                 uint32_t* __restrict__ cnt) {
    extern __shared__ uint32_t s_cnt[];
    const uint32_t tid = threadIdx.x, hs = (tid >> 2) & 63, qq = tid & 3;
    const uint32_t g = blockIdx.x / kHistSplit, k = blockIdx.x % kHistSplit;
    if (blockIdx.x == 0 && tid < 8) a.red[tid] = (tid <= 1 || tid == 3) ? ~0ull : 0ull;   // as red_init
    for (uint32_t i = tid; i < a.n_bins; i += kHist4Threads) s_cnt[i] = 0;
    __syncthreads();
    const uint32_t n_groups = (a.n_src + a.gs - 1) / a.gs;
    const uint32_t full = n_pkt & ~3u;   // chunks below this lie inside the batch
    for (uint32_t grp = g + (k + (tid >> 8) * kHistSplit) * G; grp < n_groups; grp += 4 * kHistSplit * G) {
        const uint32_t h0 = grp * a.gs, nh = min(a.gs, a.n_src - h0);
        if (hs >= nh) continue;
        const uint32_t h = a.order[h0 + hs];
        const uint32_t b = a.src_off[h - a.src_lo], e = a.src_off[h - a.src_lo + 1];
#ifndef SHD_HIST_UNROLL
#define SHD_HIST_UNROLL 4   // (C5 histogram 49.9 -> 41.1 us; 1 and 2 for A/B builds)
#endif
        // HU chunks per thread per step, their loads in flight together (a C5 host's ~100 sends
        // are ~6 chunks per thread: one dependent load after another at HU = 1)
        constexpr uint32_t HU = SHD_HIST_UNROLL;
        for (uint32_t c0 = (b >> 2) + qq; 4 * c0 < e; c0 += 4 * HU) {
            uint32_t d[HU][4];
#pragma unroll
            for (uint32_t j = 0; j < HU; ++j) {
                const uint32_t c = c0 + 4 * j;
                if (4 * c >= e) {
                    d[j][0] = d[j][1] = d[j][2] = d[j][3] = ~0u;
                } else if (4 * c + 4 <= full) {
                    const uint4 v = reinterpret_cast<const uint4*>(a.dst_host)[c];
                    d[j][0] = v.x; d[j][1] = v.y; d[j][2] = v.z; d[j][3] = v.w;
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u) d[j][u] = 4 * c + u < n_pkt ? a.dst_host[4 * c + u] : ~0u;
                }
            }
#pragma unroll
            for (uint32_t j = 0; j < HU; ++j)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t i = 4 * (c0 + 4 * j) + u;
                    if (i >= b && i < e && d[j][u] < a.n_hosts) {
                        uint32_t dl;
                        atomicAdd(&s_cnt[dst_bin(a, d[j][u], dl)], 1u);
                    }
                }
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < a.n_bins; i += kHist4Threads) cnt[(size_t)blockIdx.x * a.n_bins + i] = s_cnt[i];
}

// seg[g][b] = number of bin-b slots of stamp workgroups before g (the sum of kHistSplit
// histogram rows per workgroup, exclusive prefix over g); tot[b] = all of bin b.  Lane = bin,
// wave = a slice of workgroups; every row load of a slice is independent.  A workgroup count
// (the stamp's slot counters are 32-bit since round 6: no workgroup count overflows them).
constexpr uint32_t kColMaxG = 256;   // stamp workgroups (one per CU)

// (base != nullptr: bin_base_scan folded in -- each block's 64 bin totals, a wave scan, and a
// decoupled look-back over the earlier blocks (blockIdx order: at most 128 blocks, all resident)
// give the bins' record bases; the look-back states carry an epoch (scan.h layout), so they are
// never cleared.  One launch and one queue gap less per round.)
__global__ __launch_bounds__(1024) void bin_col_scan(uint32_t G, uint32_t n_bins, const uint32_t* __restrict__ cnt,
                                                     uint32_t* __restrict__ seg, uint32_t* __restrict__ tot,
                                                     unsigned long long* __restrict__ red,
                                                     uint32_t* __restrict__ base = nullptr,
                                                     unsigned long long* __restrict__ lb = nullptr,
                                                     unsigned long long* __restrict__ state = nullptr,
                                                     uint32_t epoch = 0) {
    __shared__ uint32_t s[16][64];
    constexpr uint32_t kPer = kColMaxG / 16;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.x * 64 + lane;
    const uint32_t g0 = min(G, w * kPer), g1 = min(G, g0 + kPer);
    uint32_t c[kPer];
    uint32_t sum = 0;
    // every row load unconditional (indices clamped, values masked) so all of them are in flight
    // together instead of one guarded load at a time
    const uint32_t bc = min(b, n_bins - 1);
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
        const uint32_t g = min(g0 + i, G - 1);
        c[i] = 0;
#pragma unroll
        for (uint32_t k = 0; k < kHistSplit; ++k) c[i] += cnt[((size_t)g * kHistSplit + k) * n_bins + bc];
    }
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
        if (!(g0 + i < g1 && b < n_bins)) c[i] = 0;
        sum += c[i];
    }
    s[w][lane] = sum;
    __syncthreads();
    uint32_t run = 0;
    for (uint32_t u = 0; u < w; ++u) run += s[u][lane];
    if (b < n_bins) {
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i) {
            const uint32_t g = g0 + i;
            if (g < g1) seg[(size_t)g * n_bins + b] = run;
            run += c[i];
        }
        if (w == 15) tot[b] = run;
    }
    if (base && w == 15) {   // wave 15 holds the 64 bin totals of this block
        const uint32_t t = b < n_bins ? run : 0u;
        if (t > kB7Cap) atomicOr(&red[6], 1ull);
        uint32_t incl = t;
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        const uint32_t agg = __shfl(incl, 63);
        const unsigned long long tag = (unsigned long long)epoch << 34;
        unsigned long long* st = state + 2 + (size_t)blockIdx.x * 2;
        uint32_t excl = 0;
        if (blockIdx.x != 0) {
            if (lane == 0) __hip_atomic_store(st, tag | (1ull << 32) | agg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int64_t hi = (int64_t)blockIdx.x - 1;;) {   // 64 earlier blocks a step
                const int64_t j = hi - (int64_t)lane;
                const unsigned long long v =
                    j >= 0 ? __hip_atomic_load(&state[2 + (size_t)j * 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                           : tag | (2ull << 32);   // before block 0: an inclusive 0
                const uint32_t f = (uint32_t)(v >> 32) & 3u;
                const bool ok = (uint32_t)(v >> 34) == epoch && f != 0;
                const uint64_t incl_m = __ballot(ok && f == 2), bad_m = __ballot(!ok);
                const uint32_t fi = incl_m ? (uint32_t)__builtin_ctzll(incl_m) : 64u;
                const uint64_t upto = fi == 64 ? ~0ull : ((2ull << fi) - 1ull);
                if (bad_m & upto) {
                    __builtin_amdgcn_s_sleep(1);
                    continue;
                }
                uint32_t add = lane <= fi ? (uint32_t)v : 0u;
                for (int o = 32; o > 0; o >>= 1) add += __shfl_xor(add, o);
                excl += add;
                if (fi < 64) break;
                hi -= 64;
            }
        }
        if (lane == 0) __hip_atomic_store(st, tag | (2ull << 32) | (excl + agg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (b < n_bins) {
            base[b] = excl + incl - t;
            lb[b] = 0;   // bin_sort_v7's look-back states
        }
        if (b == n_bins - 1) {
            base[n_bins] = excl + incl;
            lb[n_bins] = 0;   // its ticket
        }
    }
}

// one workgroup: bin_base = exclusive scan of tot (bin_base[n_bins] = total); clears the
// look-back states and the ticket of bin_sort_v7; a bin larger than its LDS stage flags red[6]
__global__ __launch_bounds__(1024) void bin_base_scan(uint32_t n_bins, const uint32_t* __restrict__ tot,
                                                      uint32_t* __restrict__ base,
                                                      unsigned long long* __restrict__ lb,
                                                      unsigned long long* __restrict__ red) {
    __shared__ uint32_t s_w[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t per = (n_bins + 1023) / 1024, b0 = min(n_bins, tid * per), b1 = min(n_bins, b0 + per);
    uint32_t sum = 0;
    bool over = false;
    for (uint32_t b = b0; b < b1; ++b) {
        sum += tot[b];
        over |= tot[b] > kB7Cap;
    }
    if (over) atomicOr(&red[6], 1ull);
    uint32_t incl = sum;
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    if (lane == 63) s_w[w] = incl;
    __syncthreads();
    uint32_t run = incl - sum;
    for (uint32_t u = 0; u < w; ++u) run += s_w[u];
    for (uint32_t b = b0; b < b1; ++b) {
        base[b] = run;
        run += tot[b];
    }
    if (tid == 1023) base[n_bins] = run;
    for (uint32_t b = tid; b <= n_bins; b += 1024) lb[b] = 0;   // lb[n_bins]: the ticket
}

// 64-bit wave bitonic (element e = lane + 64 c), lane exchanges through xor_lane on both halves
template <int NPL>
__device__ __forceinline__ void wave_bitonic64(uint64_t (&k)[NPL], uint32_t lane) {
#pragma unroll
    for (uint32_t kk = 2; kk <= 64u * NPL; kk <<= 1) {
#pragma unroll
        for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
            if (j >= 64) {
                const uint32_t cj = j / 64;
#pragma unroll
                for (int c = 0; c < NPL; ++c) {
                    if ((c & cj) == 0) {
                        const bool asc = ((lane + 64u * c) & kk) == 0;
                        const uint64_t x = k[c], y = k[c | cj];
                        const bool sw = (y < x) == asc;   // unique keys
                        k[c] = sw ? y : x;
                        k[c | cj] = sw ? x : y;
                    }
                }
            } else {
#pragma unroll
                for (int c = 0; c < NPL; ++c) {
                    const uint32_t lo = xor_lane((uint32_t)k[c], j, lane);
                    const uint32_t hi = xor_lane((uint32_t)(k[c] >> 32), j, lane);
                    const uint64_t o = ((uint64_t)hi << 32) | lo;
                    // keys are unique: take the partner's key iff it is smaller where this lane
                    // keeps the minimum (one 64-bit compare, one select)
                    const bool take_min = ((lane & j) == 0) == (((lane + 64u * c) & kk) == 0);
                    k[c] = (o < k[c]) == take_min ? o : k[c];
                }
            }
        }
    }
}

struct V7Out {
    uint64_t* deliver;
    uint32_t* src;
    uint64_t* seq;
    uint32_t* pkt;
    const uint64_t* seq_base;
    uint64_t round_end;
    // a flush round (shd_relay_flush, one context): the compact event records instead of the
    // arrays -- {deliver - round_end, src, id relative to the source's first of the round (the
    // records hold relative ids then), send index in stage order = perm[packet]}, 16 or 12 bytes
    void* fl_out = nullptr;
    const uint32_t* fl_perm = nullptr;
    uint32_t fl_b12 = 0;
};

__device__ __forceinline__ void v7_emit(const V7Out& o, size_t at, const uint4& r) {
    const uint32_t src = r.y & (kV7MaxHosts - 1);
    if (o.fl_out) {
        const uint32_t send = o.fl_perm[r.w];
        if (o.fl_b12) {
            uint32_t* e = static_cast<uint32_t*>(o.fl_out) + 3 * at;
            e[0] = r.x;
            e[1] = r.z;
            e[2] = send;
        } else {
            static_cast<uint4*>(o.fl_out)[at] = make_uint4(r.x, src, r.z, send);
        }
        return;
    }
    o.deliver[at] = o.round_end + r.x;
    o.src[at] = src;
    o.seq[at] = o.seq_base ? o.seq_base[src] + r.z : r.z;
    o.pkt[at] = r.w;
}

// one destination run (bin slots ls[0..n), n <= 256) sorted by (deliver offset, packet index),
// key = (x - lo) << 32 | (pkt - pmin) << 8 | e  (pkt - pmin < 2^24, e < 256: unique); writes
// the run's order as slots: pm[rank] = slot
template <int NPL>
__device__ __forceinline__ void v7_sort_run(uint32_t n, uint32_t lane, const uint4* x, const uint16_t* ls,
                                            uint16_t* pm) {
    uint2 v[NPL];
    uint32_t lo = ~0u, pmin = ~0u;
#pragma unroll
    for (int c = 0; c < NPL; ++c) {
        const uint32_t e = lane + 64u * c;
        if (e < n) {
            const uint4 r = x[ls[e]];
            v[c] = make_uint2(r.x, r.w);
        } else {
            v[c] = make_uint2(~0u, ~0u);
        }
        lo = min(lo, v[c].x);
        pmin = min(pmin, v[c].y);
    }
    lo = wave_min_u32(lo, lane);
    pmin = wave_min_u32(pmin, lane);
    {   // 32-bit keys (deliver - lo) << 8 | e when the run's deliver times span < 2^24 ns: half the
        // lane exchanges and compares of the 64-bit network.  Equal deliver times would need the
        // packet order: a run with any is redone on the 64-bit keys below.
        uint32_t hi = 0;
#pragma unroll
        for (int c = 0; c < NPL; ++c)
            if (lane + 64u * c < n) hi = max(hi, v[c].x);
        hi = wave_max_u32(hi, lane);
        if (hi - lo < (1u << 24)) {
            uint32_t k32[NPL];
#pragma unroll
            for (int c = 0; c < NPL; ++c) {
                const uint32_t e = lane + 64u * c;
                k32[c] = e < n ? ((v[c].x - lo) << 8) | e : ~0u;
            }
            wave_bitonic32<NPL>(k32, lane);
            // sorted: element r = lane + 64 c; a tie is an equal upper 24 bits in neighbours r, r + 1
            bool tie = false;
#pragma unroll
            for (int c = 0; c < NPL; ++c) {
                // (both shuffles with every lane active: a read of an inactive lane returns 0)
                const uint32_t down = (uint32_t)__shfl_down((int)k32[c], 1);
                const uint32_t first = c + 1 < NPL ? (uint32_t)__shfl((int)k32[c + 1 < NPL ? c + 1 : c], 0) : ~0u;
                const uint32_t nx = lane == 63 ? first : down;
                const uint32_t r = lane + 64u * c;
                if (r + 1 < n && (nx >> 8) == (k32[c] >> 8)) tie = true;
            }
            if (__ballot(tie) == 0) {
#pragma unroll
                for (int c = 0; c < NPL; ++c) {
                    const uint32_t rank = lane + 64u * c;
                    if (rank < n) pm[rank] = ls[k32[c] & 0xFFu];
                }
                return;
            }
        }
    }
    uint64_t k[NPL];
#pragma unroll
    for (int c = 0; c < NPL; ++c) {
        const uint32_t e = lane + 64u * c;
        k[c] = e < n ? ((uint64_t)(v[c].x - lo) << 32) | ((uint64_t)(v[c].y - pmin) << 8) | e : ~0ull;
    }
    wave_bitonic64<NPL>(k, lane);
#pragma unroll
    for (int c = 0; c < NPL; ++c) {
        const uint32_t rank = lane + 64u * c;
        if (rank < n) pm[rank] = ls[(uint32_t)k[c] & 0xFFu];
    }
}

// (K4 of a sharded round, bin_sort_v7<true>: its sources XSrc are in relay_priv.h)
// the round's agreed status from the exchange's status part: the lowest failing rank's
__device__ __forceinline__ uint32_t xs_status(const XSrc& xs) {
    for (uint32_t q = 0; q < xs.world; ++q) {
        const uint32_t v = q == xs.me ? xs.own_st : (uint32_t)xs.rst[q];
        if (v) return v;
    }
    return 0u;
}

// a rank without bins: no bin sort writes its event count and the agreed status
__global__ __launch_bounds__(64) void xs_fin_empty(XSrc xs, uint32_t* __restrict__ ev_off) {
    if (threadIdx.x == 0) {
        ev_off[0] = 0;
        ev_off[1] = xs_status(xs);
    }
}

// Phase pricing (tuning builds, tools/b7_phases.sh): -DSHD_B7_STOP=k makes bin_sort_v7 return after
// phase k = 1 load, 2 look-back, 3 grouping, 4 sorts; the output is wrong, only the time is read
#ifndef SHD_B7_STOP
#define SHD_B7_STOP 0
#endif
// K4 (v7): one workgroup per bin, bins taken in ticket order so the event offsets can use a
// decoupled look-back (publish the bin's sent count, add the predecessors' counts).  The bin's
// records are staged in LDS, grouped by destination, each run sorted by one wave into the
// bin's output order, and the bin's events stored in that order (coalesced).
template <bool X>
__global__ __launch_bounds__(kB7Threads) void bin_sort_v7(uint32_t n_hosts, uint32_t n_bins,
                                                          const uint32_t* __restrict__ bin_base,
                                                          const uint4* __restrict__ rec,
                                                          unsigned long long* __restrict__ lb,
                                                          uint32_t* __restrict__ ev_off, V7Out o,
                                                          const unsigned long long* __restrict__ red, XSrc xs) {
    __shared__ uint4 x[kB7Cap];
    __shared__ uint16_t ls[kB7Cap], pm[kB7Cap];
    __shared__ uint32_t s_cnt[kBinDst], s_off[kBinDst + 1], s_cur[kBinDst], s_bin, s_excl;
    __shared__ uint32_t s_pb[X ? 64 : 1];
    // (X: the own sender's records are read from xs.own, every other sender's from rec)
    if (!X && red[6]) return;   // overflow: the host reruns the round on v3
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) s_bin = atomicAdd(reinterpret_cast<unsigned int*>(&lb[n_bins]), 1u);
    if (tid < kBinDst) s_cnt[tid] = s_cur[tid] = 0;
    __syncthreads();
    const uint32_t bin = s_bin;
    uint32_t B = 0, N = 0;
    // X: every wave reads the senders' segments of the bin itself (lane q: sender q) and keeps
    // them in registers, so no wave waits at a barrier for another's loads before its record
    // loads (measured the same as a wave-0 table in LDS behind a barrier: the X form's extra
    // ~25 us over bin_sort_v7<false> at world size 1 is its look-back phase, +13 us, and the
    // loads, +6 us; priced with SHD_B7_STOP builds)
    uint32_t x_at = 0, x_pre = 0, x_pb = 0;
    if constexpr (X) {
        uint32_t c = 0;
        if (lane < xs.world) {
            const uint32_t* sq = xs.sc + (size_t)lane * xs.stride + xs.fb;
            const uint32_t a0 = sq[0], a1 = sq[bin], a2 = sq[bin + 1];
            x_at = lane == xs.me ? a1 : xs.rbase[lane] + (a1 - a0);
            c = a2 - a1;
            x_pb = xs.pbase[lane];
        }
        uint32_t incl = c;
        for (uint32_t q = 1; q < 64; q <<= 1) {
            const uint32_t y = __shfl_up(incl, q);
            if (lane >= q) incl += y;
        }
        x_pre = incl - c;
        if (w == 0) s_pb[lane] = x_pb;   // (read by the emit, behind later barriers)
        N = __shfl(incl, xs.world - 1);   // <= kB7Cap: the host checked every bin's total before the exchange
    } else {
        B = bin_base[bin];
        N = bin_base[bin + 1] - B;
    }
    {   // every load of the bin in flight at once (N <= kB7Cap)
        uint4 r[kB7Per];
        uint32_t qs[kB7Per], pbq[kB7Per];   // X: each record's sender and its packet base
#pragma unroll
        for (uint32_t u = 0; u < kB7Per; ++u) {
            const uint32_t i = tid + u * kB7Threads;
            if constexpr (X) {
                // (the shuffles run on every lane, outside the i < N guard: a bpermute must not
                // read a lane that skipped the computation)
                uint32_t q = 0;   // the sender of staged index i: the last q with pre[q] <= i
                for (uint32_t k = xs.kq; k > 0; k >>= 1) {   // (kq: the largest power of two < world)
                    const uint32_t pk = (uint32_t)__shfl((int)x_pre, (int)min(q + k, xs.world - 1));
                    if (q + k < xs.world && pk <= i) q += k;
                }
                const uint32_t at = (uint32_t)__shfl((int)x_at, (int)q), pre = (uint32_t)__shfl((int)x_pre, (int)q);
                qs[u] = q;
                pbq[u] = (uint32_t)__shfl((int)x_pb, (int)q);
                if (i < N) r[u] = (q == xs.me ? xs.own : rec)[at + (i - pre)];
            } else {
                if (i < N) r[u] = rec[B + i];
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < kB7Per; ++u) {
            const uint32_t i = tid + u * kB7Threads;
            if (i < N) {
                if constexpr (X) {
                    r[u].w += pbq[u];          // global packet order
                    r[u].y |= qs[u] << 26;     // the sender, for the packet index of the output
                }
                x[i] = r[u];
                if (((r[u].y >> 24) & 3u) == kStSent) atomicAdd(&s_cnt[(r[u].y >> 18) & (kBinDst - 1)], 1u);
            }
        }
    }
    __syncthreads();
    if (SHD_B7_STOP == 1) return;
    if (w == 0) {
        const uint32_t c = lane < kBinDst ? s_cnt[lane] : 0u;
        uint32_t incl = c;
        for (uint32_t q = 1; q < 64; q <<= 1) {
            const uint32_t y = __shfl_up(incl, q);
            if (lane >= q) incl += y;
        }
        if (lane <= kBinDst) s_off[lane] = incl - c;
        const uint32_t agg = __shfl(incl, 63);
        unsigned long long excl = 0;
        if (bin == 0) {
            if (lane == 0) __hip_atomic_store(&lb[0], kLbIncl | agg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            if (lane == 0) __hip_atomic_store(&lb[bin], kLbAgg | agg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // look-back 64 predecessors at a time: lane l reads bin hi - l; the nearest inclusive
            // state ends the walk once every state up to it has been published (bin 0 always is)
            for (int32_t hi = (int32_t)bin - 1;;) {
                const int32_t j = hi - (int32_t)lane;
                const unsigned long long v =
                    j >= 0 ? __hip_atomic_load(&lb[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : kLbIncl;
                const uint64_t incl_m = __ballot((v & kLbIncl) != 0), zero_m = __ballot(v == 0);
                const uint32_t fi = incl_m ? (uint32_t)__builtin_ctzll(incl_m) : 64u;
                const uint64_t upto = fi == 64 ? ~0ull : ((2ull << fi) - 1ull);
                if (zero_m & upto) {
                    __builtin_amdgcn_s_sleep(1);
                    continue;
                }
                unsigned long long add = lane <= fi ? (v & kLbMask) : 0ull;
                for (int q = 32; q > 0; q >>= 1) add += __shfl_xor(add, q);
                excl += add;
                if (fi < 64) break;
                hi -= 64;
            }
            if (lane == 0)
                __hip_atomic_store(&lb[bin], kLbIncl | (excl + agg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) s_excl = (uint32_t)excl;
    }
    __syncthreads();
    const uint32_t excl = s_excl, d0 = bin * kBinDst, S = s_off[kBinDst];
    if (tid < kBinDst && d0 + tid < n_hosts) ev_off[d0 + tid] = excl + s_off[tid];
    if (tid == 0 && bin == n_bins - 1) {
        ev_off[n_hosts] = excl + S;
        if constexpr (X) ev_off[n_hosts + 1] = xs_status(xs);   // (read back with the count)
    }
    if (SHD_B7_STOP == 2) return;
    for (uint32_t i = tid; i < N; i += kB7Threads) {
        const uint32_t y = x[i].y;
        if (((y >> 24) & 3u) == kStSent) {
            const uint32_t dl = (y >> 18) & (kBinDst - 1);
            ls[s_off[dl] + atomicAdd(&s_cur[dl], 1u)] = (uint16_t)i;
        }
    }
    __syncthreads();
    if (SHD_B7_STOP == 3) return;
    for (uint32_t dl = w; dl < kBinDst; dl += kB7Threads / 64) {
        const uint32_t b = s_off[dl], n = s_off[dl + 1] - b;
        if (n == 0) continue;
        if (n <= 64) v7_sort_run<1>(n, lane, x, ls + b, pm + b);
        else if (n <= 128) v7_sort_run<2>(n, lane, x, ls + b, pm + b);
        else if (n <= 256) v7_sort_run<4>(n, lane, x, ls + b, pm + b);
        else {   // long run (rare): rank = number of smaller (deliver, packet) keys
            for (uint32_t e = lane; e < n; e += 64) {
                const uint4 q0 = x[ls[b + e]];
                uint32_t rank = 0;
                for (uint32_t f = 0; f < n; ++f) {
                    const uint4 q = x[ls[b + f]];
                    rank += (q.x < q0.x || (q.x == q0.x && q.w < q0.w)) ? 1u : 0u;
                }
                pm[b + rank] = ls[b + e];
            }
        }
    }
    __syncthreads();
    if (SHD_B7_STOP == 4) return;
    for (uint32_t p = tid; p < S; p += kB7Threads) {
        uint4 r = x[pm[p]];
        if constexpr (X) {
            r.w -= s_pb[r.y >> 26];   // back to the index in the sender's batch
            r.y &= kV7MaxHosts - 1;
        }
        v7_emit(o, (size_t)excl + p, r);
    }
}

// v7 eligibility: narrow table, LDS host map, src ids and packet indices within the record /
// key fields, and the stamp's LDS (map + slot counters) within the CU's 160 KB
bool relay_v7_ok(shd_ctx* ctx, uint64_t n, uint32_t n_bins) {
    RelayState& R = ctx->relay;
    if (R.force_v3 || R.n_hosts > kV7MaxHosts || n > kV7MaxPackets) return false;
    if (R.n_src == 0 || std::min<uint32_t>(div_up(R.n_src, kS5Hosts), (uint32_t)ctx->n_cu) > kColMaxG) return false;
    const size_t stat_lds = relay_stamp_bins_static_lds();
    if (!stat_lds) return false;
    return stat_lds + (R.hn_bits ? (size_t)R.hn_words * 4 : 0) + (size_t)n_bins * 4 <= 160 * 1024;
}

// Hosts per stamp group: about S sends per group (SHD_RELAY_GROUP_SENDS, 0 = fixed kS5Hosts),
// so a group is one full chunk of the stamp, and a group count that is a multiple of the stamp's
// G workgroups, so no pass of the persistent grid runs with most workgroups idle.
static uint32_t v7_group_size(const shd_ctx* ctx, uint32_t n_src, uint32_t G, uint64_t n) {
    // default: one chunk's worth (C5: 40 hosts, ~4000 sends; stamp 310 -> 283 us; 36 hosts: 290)
    const uint64_t S = ctx->knobs.get64(K_RELAY_GROUP_SENDS, (uint64_t)relay_stamp_chunk());
    if (!S || !n || !n_src || !G) return kS5Hosts;
    const double per_host = (double)n / n_src;
    const uint32_t want = (uint32_t)std::min<double>(kS5Hosts, std::max<double>(8.0, (double)S / per_host));
    const uint64_t m = div_up((uint64_t)n_src, (uint64_t)G * want);
    return (uint32_t)std::min<uint64_t>(kS5Hosts, std::max<uint64_t>(1, div_up((uint64_t)n_src, (uint64_t)G * m)));
}

XShard xshard(uint32_t H, uint32_t world) {
    XShard x;
    x.per = (uint32_t)div_up((uint64_t)H, (uint64_t)world);
    x.bpr = div_up(x.per, kBinDst);
    x.mul = ((1ull << 40) + x.per - 1) / x.per;
    for (uint32_t r = 0; r < world; ++r) {
        uint32_t lo = 0, hi = 0;
        shard_range(H, (int)world, (int)r, &lo, &hi);
        x.n_bins += div_up(hi - lo, kBinDst);
    }
    return x;
}

// pipeline 7 on one GPU, or (xsh) up to and including the stamp for a sharded round (relay_priv.h)
shd_status relay_device_v7(shd_ctx* ctx, const shd_batch* b, const shd_round* rd, shd_relay_out* o,
                           const XShard* xsh) {
    RelayState& R = ctx->relay;
    hipStream_t s = ctx->stream;
    const uint64_t n = b->n_packets;
    const uint32_t H = R.n_hosts;
    const size_t nn = std::max<uint64_t>(n, 1);
    const uint32_t n_bins = xsh ? xsh->n_bins : div_up(H, kBinDst);
    const uint32_t G = std::min<uint32_t>(div_up(R.n_src, kS5Hosts), (uint32_t)ctx->n_cu);
    SHD_TRY(R.rec.ensure(nn * 16));
    SHD_TRY(R.draws.ensure(nn * 4));
    SHD_TRY(R.bin_cnt.ensure((size_t)G * (kHistSplit + 1) * n_bins * 4));
    SHD_TRY(R.bin_base.ensure((size_t)(2 * n_bins + 1) * 4));
    SHD_TRY(R.bin_lb.ensure((size_t)(n_bins + 1) * 8));
    RelayArgs3 a = relay_args3(ctx, b, rd, o);
    a.gs = v7_group_size(ctx, R.n_src, G, n);
    if (xsh) {
        a.sh_per = xsh->per;
        a.sh_bpr = xsh->bpr;
        a.sh_mul = xsh->mul;
    }
    uint32_t* tot = R.bin_base.as<uint32_t>() + n_bins + 1;
    a.bin_base = R.bin_base.as<uint32_t>();
    a.n_bins = n_bins;
    uint32_t* seg = R.bin_cnt.as<uint32_t>() + (size_t)G * kHistSplit * n_bins;
    a.seg_pre = seg;
    // K0 in line before the histogram (round 5): K0 30 us + histogram 21 us back to back beat K0
    // beside the histogram on a side stream (39 ‖ 41 us, each slowed by the other taking wave
    // slots) plus the fork / join events: C5 round 0.467-0.476 -> 0.457 ms
    relay_launch_draws(ctx, a);
    // the histogram's first block also resets the round's reductions (red_init's job: one
    // launch less; only the scans and the stamp read them, all after the histogram)
    // (SHD_HIST_SCALAR=1, tuning A/B: the flattened-position form)
    if (((uintptr_t)b->dst_host & 15) == 0 && n < (1ull << 31) && !ctx->knobs.on(K_HIST_SCALAR))
        relay_bin_hist4<<<G * kHistSplit, kHist4Threads, (size_t)n_bins * 4, s>>>(a, G, (uint32_t)n,
                                                                             R.bin_cnt.as<uint32_t>());
    else
        relay_bin_hist<<<G * kHistSplit, 256, (size_t)n_bins * 4, s>>>(a, G, R.bin_cnt.as<uint32_t>());
    if (ctx->knobs.get(K_RELAY_SCAN2, 0) != 0 || div_up(n_bins, 64) > 128) {   // (A/B: two launches)
        bin_col_scan<<<div_up(n_bins, 64), 1024, 0, s>>>(G, n_bins, R.bin_cnt.as<uint32_t>(), seg, tot, a.red);
        bin_base_scan<<<1, 1024, 0, s>>>(n_bins, tot, R.bin_base.as<uint32_t>(), R.bin_lb.as<unsigned long long>(), a.red);
    } else {   // the bases from the column scan's own look-back (bin_col_scan)
        ScanScratch& SS = R.col_scan;
        const uint64_t blocks = div_up(n_bins, 64);
        if (blocks * 16 + 16 > SS.state.bytes) {
            SHD_TRY(SS.state.ensure(blocks * 16 + 16));
            SHD_HIP(hipMemsetAsync(SS.state.p, 0, SS.state.bytes, s));
            SS.epoch = 0;
        }
        if (++SS.epoch >= (1u << 30)) {
            SHD_HIP(hipMemsetAsync(SS.state.p, 0, SS.state.bytes, s));
            SS.epoch = 1;
        }
        bin_col_scan<<<(uint32_t)blocks, 1024, 0, s>>>(G, n_bins, R.bin_cnt.as<uint32_t>(), seg, tot, a.red,
                                                       R.bin_base.as<uint32_t>(), R.bin_lb.as<unsigned long long>(),
                                                       SS.state.as<unsigned long long>(), SS.epoch);
    }
    relay_launch_stamp_bins(ctx, a, G, (R.hn_bits ? (size_t)R.hn_words * 4 : 0) + (size_t)n_bins * 4);
    if (xsh) {
        SHD_HIP(hipGetLastError());
        return SHD_OK;
    }
    V7Out vo{o->ev_deliver, o->ev_src, o->ev_seq, o->ev_pkt,
             a.abs_seq ? nullptr : R.next_id.as<uint64_t>(), rd->round_end};
    if (R.fl_ev_out && !a.abs_seq) {   // a flush round: compact records straight from the bin sort
        vo.fl_out = R.fl_ev_out;
        vo.fl_perm = R.fl_perm.as<uint32_t>();
        vo.fl_b12 = R.fl_b12;
        R.fl_direct = true;
    }
    bin_sort_v7<false><<<n_bins, kB7Threads, 0, s>>>(H, n_bins, R.bin_base.as<uint32_t>(), R.rec.as<uint4>(),
                                                    R.bin_lb.as<unsigned long long>(), o->ev_off, vo, a.red,
                                                    XSrc{});
    return relay_read_red(ctx);
}

void relay_launch_bin_sort_x(shd_ctx* ctx, uint32_t n_own, uint32_t nb, uint64_t round_end, const XSrc& xs) {
    RelayState& R = ctx->relay;
    hipStream_t s = ctx->stream;
    if (nb) {
        V7Out vo{R.m_deliver.as<uint64_t>(), R.m_src.as<uint32_t>(), R.m_seq.as<uint64_t>(), R.m_pkt.as<uint32_t>(),
                 nullptr, round_end};
        bin_sort_v7<true><<<nb, kB7Threads, 0, s>>>(n_own, nb, nullptr, R.x_rrec.as<uint4>(),
                                                    R.bin_lb.as<unsigned long long>(), R.m_off.as<uint32_t>(), vo,
                                                    nullptr, xs);
    } else {
        xs_fin_empty<<<1, 64, 0, s>>>(xs, R.m_off.as<uint32_t>());
    }
}

}  // namespace shd
