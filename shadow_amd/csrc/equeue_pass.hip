// One pass over the event queues' sources (overview: equeue_priv.h): the count, merge and totals
// kernels and eq_pass, which launches them and reads the totals back.
#include <algorithm>

#include "equeue_priv.h"
#include "scan.h"
#include "wave.h"

namespace shd {

__device__ __forceinline__ bool eq_less(uint64_t ta, uint32_t sa, uint64_t qa, uint64_t tb, uint32_t sb,
                                        uint64_t qb) {
    if (ta != tb) return ta < tb;
    if (sa != sb) return sa < sb;
    return qa < qb;
}

__device__ __forceinline__ uint32_t lower_bound_time(const uint64_t* t, uint32_t b, uint32_t e, uint64_t x) {
    while (b < e) {
        const uint32_t m = (b + e) >> 1;
        if (t[m] < x) b = m + 1; else e = m;
    }
    return b;
}

// lower_bound from the front: a run's popped prefix is short (C5: ~10 events per host and run),
// so probing b, b+1, b+3, b+7, ... finds the cut within a line or two of the cursor, where a
// plain bisection of the whole run touches a line per step
__device__ __forceinline__ uint32_t lower_bound_gallop(const uint64_t* t, uint32_t b, uint32_t e, uint64_t x) {
    if (b >= e || !(t[b] < x)) return b;
    uint32_t prev = b, step = 1;   // t[prev] < x
    while (step < e - prev && t[prev + step] < x) {
        prev += step;
        step <<= 1;
    }
    return lower_bound_time(t, prev + 1, min(e, prev + step), x);
}

// per host and source: the cut (first event at or past window_end); popped count per host, the
// batch's kept count per host, events left per source and the earliest kept deliver time.
// kEqLanes lanes per host, lane k on source k: the sources' binary searches run side by side.
constexpr uint32_t kEqLanes = 16;
static_assert(kEqSrcMax <= kEqLanes, "a lane per source");

__global__ __launch_bounds__(256) void eqr_count(uint32_t n_hosts, EqSrcs S, uint64_t window_end,
                                                 uint32_t* __restrict__ pop, uint32_t* __restrict__ keep,
                                                 unsigned long long* __restrict__ part, uint2* __restrict__ ranges) {
    __shared__ unsigned long long s_w[4][kEqPart];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t total = ((uint64_t)n_hosts + 1) * kEqLanes;
    uint64_t head = ~0ull, rem_acc = 0;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t - threadIdx.x < total;
         t += (uint64_t)gridDim.x * 256) {   // wave-uniform trip count (total is a multiple of 16)
        const uint32_t h = (uint32_t)(t / kEqLanes), k = (uint32_t)(t % kEqLanes);
        uint32_t np = 0;
        uint64_t rem = 0;
        if (h < n_hosts && k < S.n) {
            const EqSrc& q = S.s[k];
            const uint32_t lo = q.lo ? q.lo[h] : q.off[h], hi = q.off[h + 1];
            // a compaction (window_end = ~0) takes every event: one load confirms the run's last
            // event is below it, instead of a gallop across the whole run
            // (loading the first 8 or 16 times of the run at once and counting, instead of the
            // gallop's dependent loads, measured slower: C5 advance 0.37 / 0.45 ms against 0.35)
            const uint32_t m = window_end == ~0ull && lo < hi && q.deliver[hi - 1] < window_end
                                   ? hi
                                   : lower_bound_gallop(q.deliver, lo, hi, window_end);
            q.cut[h] = m;
            ranges[(size_t)h * kEqSrcMax + k] = make_uint2(lo, m);   // eqr_merge: one line per host
            np = m - lo;
            rem = hi - m;
            if (m < hi) head = q.deliver[m] < head ? q.deliver[m] : head;
        }
        // the new run's events of this host: the batch's remainder and the folded runs'
        uint32_t kp = h < n_hosts && k < S.n && ((int32_t)k == S.b || ((S.fold >> k) & 1u)) ? (uint32_t)rem : 0u;
        for (uint32_t o = kEqLanes / 2; o > 0; o >>= 1) {
            np += __shfl_xor(np, o);
            kp += __shfl_xor(kp, o);
        }
        if (h < n_hosts && k == 0) {
            pop[h] = np;
            keep[h] = kp;
        }
        if (h == n_hosts && k == 0) {
            pop[n_hosts] = 0;
            keep[n_hosts] = 0;
        }
        rem_acc += rem;   // lane k mod kEqLanes keeps source k's sum
    }
    for (uint32_t o = kEqLanes; o < 64; o <<= 1) rem_acc += __shfl_xor(rem_acc, o);
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t x = __shfl_xor(head, o);
        head = x < head ? x : head;
    }
    if (lane < kEqSrcMax) s_w[w][1 + lane] = rem_acc;
    if (lane == 0) s_w[w][0] = head;
    __syncthreads();
    if (threadIdx.x < kEqPart) {
        unsigned long long v = s_w[0][threadIdx.x];
        for (int ww = 1; ww < 4; ++ww) {
            const unsigned long long x = s_w[ww][threadIdx.x];
            v = threadIdx.x == 0 ? (x < v ? x : v) : v + x;
        }
        part[(size_t)blockIdx.x * kEqPart + threadIdx.x] = v;
    }
}

// One wave per host: every source's popped prefix [lo, cut) goes to its merged rank in the
// popped output: its index in its own prefix + the number of smaller events in each other
// prefix.  When the host's popped events fit kEqStage, the prefixes are staged in LDS (whole
// events, a lane per staged event), every lane then takes one staged event and
// binary-searches the other prefixes in LDS; larger hosts search global memory source by
// source.  Then the batch's remainder [cut, end) is copied to the new run (in the same wave: a
// separate streaming kernel, alone or beside the merge on the side stream, measured slower).
// (an LDS table of the sources' arrays read by a per-lane source index, instead of the selects
// over every source's pointers, measured slower: C5 advance 0.395 against 0.377 ms)
constexpr uint32_t kEqStage = 160;   // 17.5 KB per 4-wave workgroup: 8 workgroups (32 waves) per CU

// Rank a host's staged popped events by a wave sort instead of searches: (t - tmin) << 8 | staged
// index is a unique key, 32 bits when the deliver times span less than 2^24 ns (a window of up
// to ~16 ms: every normal pass), 64 bits otherwise (a compaction's whole runs), and a bitonic
// network over the wave (wave.h: one DPP / swizzle / permlane exchange per stage, 28 stages for
// 128 events) orders them -- a bisection per other source per event costs several times the
// VALU issue, which is what bounds the merge (~100 events per host on C5) -- and the events
// leave in rank order (coalesced stores).  Equal times, whose order needs (src, seq), return
// false: the caller's searches take the host.
template <int NPL>
__device__ __forceinline__ bool eq_sort_emit(uint32_t npop, uint32_t lane, const uint64_t* st, const uint32_t* ss,
                                             const uint64_t* sq, const uint64_t* sg, uint32_t po, EqOut popped) {
    static_assert(64 * NPL <= 256, "staged index in 8 key bits");
    uint64_t t[NPL], tmn = ~0ull, tmx = 0;
#pragma unroll
    for (int c = 0; c < NPL; ++c) {
        const uint32_t i = lane + 64u * c;
        t[c] = i < npop ? st[i] : 0ull;
        if (i < npop) {
            tmn = t[c] < tmn ? t[c] : tmn;
            tmx = t[c] > tmx ? t[c] : tmx;
        }
    }
    tmn = wave_min_u64(tmn);
    tmx = wave_max_u64(tmx);
    uint32_t idx[NPL];
    bool tie = false;   // equal times in sorted neighbours r, r + 1
    if (tmx - tmn < (1ull << 24)) {   // wave-uniform
        uint32_t k[NPL];
#pragma unroll
        for (int c = 0; c < NPL; ++c) {
            const uint32_t i = lane + 64u * c;   // npop < 256 here: no valid key reaches ~0u
            k[c] = i < npop ? ((uint32_t)(t[c] - tmn) << 8) | i : ~0u;
        }
        wave_bitonic32<NPL>(k, lane);
#pragma unroll
        for (int c = 0; c < NPL; ++c) {
            // (both shuffles with every lane active: a read of an inactive lane returns 0)
            const uint32_t down = (uint32_t)__shfl_down((int)k[c], 1);
            const uint32_t first = c + 1 < NPL ? (uint32_t)__shfl((int)k[c + 1 < NPL ? c + 1 : c], 0) : ~0u;
            const uint32_t nx = lane == 63 ? first : down;
            if (lane + 64u * c + 1 < npop && (nx >> 8) == (k[c] >> 8)) tie = true;
            idx[c] = k[c] & 0xFFu;
        }
    } else if (tmx - tmn < (1ull << 56)) {
        uint64_t k[NPL];
#pragma unroll
        for (int c = 0; c < NPL; ++c) {
            const uint32_t i = lane + 64u * c;
            k[c] = i < npop ? ((t[c] - tmn) << 8) | i : ~0ull;
        }
        wave_bitonic<NPL>(k, lane);
#pragma unroll
        for (int c = 0; c < NPL; ++c) {
            const uint64_t down = __shfl_down(k[c], 1);
            const uint64_t first = c + 1 < NPL ? __shfl(k[c + 1 < NPL ? c + 1 : c], 0) : ~0ull;
            const uint64_t nx = lane == 63 ? first : down;
            if (lane + 64u * c + 1 < npop && (nx >> 8) == (k[c] >> 8)) tie = true;
            idx[c] = (uint32_t)k[c] & 0xFFu;
        }
    } else {
        return false;
    }
    if (__ballot(tie) != 0) return false;
#pragma unroll
    for (int c = 0; c < NPL; ++c) {
        const uint32_t r = lane + 64u * c;
        if (r < npop) {
            const uint32_t i = idx[c];
            popped.deliver[po + r] = st[i];
            popped.src[po + r] = ss[i];
            popped.seq[po + r] = sq[i];
            popped.tag[po + r] = sg[i];
        }
    }
    return true;
}

// One host's merge (a wave): lane k < S.n holds source k's popped range [my_lo, my_m); po is the
// host's first popped slot, rb_no its first slot in the new run (a batch source only); sort_rank:
// rank staged hosts by eq_sort_emit first (false: the searches alone).
template <uint32_t STAGE>
__device__ __forceinline__ void eq_merge_host(uint32_t h, uint32_t w, uint32_t lane, const EqSrcs& S, uint32_t my_lo,
                                              uint32_t my_m, uint32_t po, EqOut popped, EqOut nrun, uint32_t rb_no,
                                              uint32_t* __restrict__ nrun_cur, uint64_t (*s_t)[STAGE],
                                              uint64_t (*s_q)[STAGE], uint64_t (*s_g)[STAGE],
                                              uint32_t (*s_s)[STAGE], bool sort_rank) {
    const uint32_t cnt = my_m - my_lo;
    uint32_t incl = cnt;
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    const uint32_t my_sb = incl - cnt, npop = __shfl(incl, 63);
    // every source's range as wave-uniform values (read while all lanes are active: a lane read
    // from inside the divergent loops below would see inactive lanes as 0)
    uint32_t u_lo[kEqSrcMax], u_c[kEqSrcMax], u_sb[kEqSrcMax];
#pragma unroll
    for (uint32_t k = 0; k < kEqSrcMax; ++k) {
        u_lo[k] = __builtin_amdgcn_readlane(my_lo, k);
        u_c[k] = __builtin_amdgcn_readlane(cnt, k);
        u_sb[k] = __builtin_amdgcn_readlane(my_sb, k);
    }
    // the batch remainder's first 128 events are loaded up front: their latency overlaps the
    // merge instead of following it (its cut is the batch range's end from eqr_count)
    uint32_t rb_m = 0, rb_e = 0;
    uint64_t pf_t[2] = {0, 0}, pf_q[2] = {0, 0};
    uint32_t pf_s[2] = {0, 0}, pf_p[2] = {0, 0};
    if (S.b >= 0) {
        const EqSrc& q = S.s[S.b];
#pragma unroll
        for (uint32_t k = 0; k < kEqSrcMax; ++k)
            if ((int32_t)k == S.b) rb_m = u_lo[k] + u_c[k];
        rb_e = q.off[h + 1];
#pragma unroll
        for (uint32_t u = 0; u < 2; ++u) {
            const uint32_t j = rb_m + lane + 64 * u;
            if (j < rb_e) {
                pf_t[u] = q.deliver[j];
                pf_s[u] = q.src[j];
                pf_q[u] = q.seq[j];
                pf_p[u] = q.pkt[j];
            }
        }
    }
    if (npop <= STAGE) {
        uint64_t* st = s_t[w];
        uint64_t* sq = s_q[w];
        uint64_t* sg = s_g[w];
        uint32_t* ss = s_s[w];
        // lane i0 loads staged event i0 straight from its source (the source's arrays picked by
        // selects on wave-uniform values): every source's loads are in flight at once, instead
        // of one source's round trip after another
        for (uint32_t i0 = lane; i0 < npop; i0 += 64) {
            uint32_t at = u_lo[0] + i0;
            const uint64_t* dl = S.s[0].deliver;
            const uint64_t* qp = S.s[0].seq;
            const uint32_t* sp = S.s[0].src;
            const uint64_t* tp = S.s[0].tag;
            const uint32_t* pp = S.s[0].pkt;
            uint64_t bt = S.s[0].batch;
#pragma unroll
            for (uint32_t j = 1; j < kEqSrcMax; ++j) {
                if (j < S.n && u_sb[j] <= i0) {
                    at = u_lo[j] + (i0 - u_sb[j]);
                    dl = S.s[j].deliver;
                    qp = S.s[j].seq;
                    sp = S.s[j].src;
                    tp = S.s[j].tag;
                    pp = S.s[j].pkt;
                    bt = S.s[j].batch;
                }
            }
            st[i0] = dl[at];
            sq[i0] = qp[at];
            ss[i0] = sp[at];
            sg[i0] = tp ? tp[at] : ((bt << 32) | pp[at]);
        }
        wave_sync_lds();
        static_assert(STAGE <= 256, "staged index in 8 key bits");
        const bool sorted = sort_rank && npop > 1 &&
                            (npop <= 64    ? eq_sort_emit<1>(npop, lane, st, ss, sq, sg, po, popped)
                             : npop <= 128 ? eq_sort_emit<2>(npop, lane, st, ss, sq, sg, po, popped)
                                           : eq_sort_emit<4>(npop, lane, st, ss, sq, sg, po, popped));
        for (uint32_t i0 = sorted ? npop : lane; i0 < npop; i0 += 64) {
            uint32_t k = 0;   // staged event i0 belongs to source k: u_sb[k] <= i0 < u_sb[k + 1]
            for (uint32_t j = 1; j < S.n; ++j) k = u_sb[j] <= i0 ? j : k;
            const uint64_t t = st[i0], qq = sq[i0];
            const uint32_t sv = ss[i0];
            uint32_t rank = i0 - u_sb[k];
            for (uint32_t k2 = 0; k2 < S.n; ++k2) {
                if (k2 == k) continue;
                const uint32_t sb2 = u_sb[k2];
                uint32_t a = 0, b = u_c[k2];
                while (a < b) {
                    const uint32_t m = (a + b) >> 1, x = sb2 + m;
                    const uint64_t tm = st[x];
                    const bool less = tm != t ? tm < t : eq_less(tm, ss[x], sq[x], t, sv, qq);
                    if (less) a = m + 1; else b = m;
                }
                rank += a;
            }
            popped.deliver[po + rank] = t;
            popped.src[po + rank] = sv;
            popped.seq[po + rank] = qq;
            popped.tag[po + rank] = sg[i0];
        }
    } else {
        for (uint32_t k = 0; k < S.n; ++k) {
            const EqSrc& q = S.s[k];
            const uint32_t lo = u_lo[k], c = u_c[k];
            for (uint32_t i = lane; i < c; i += 64) {
                const uint64_t t = q.deliver[lo + i], qq = q.seq[lo + i];
                const uint32_t sv = q.src[lo + i];
                const uint64_t tg = q.tag ? q.tag[lo + i] : ((q.batch << 32) | q.pkt[lo + i]);
                uint32_t rank = i;
                for (uint32_t k2 = 0; k2 < S.n; ++k2) {
                    if (k2 == k) continue;
                    const EqSrc& r = S.s[k2];
                    const uint32_t lo2 = u_lo[k2];
                    uint32_t a = 0, b = u_c[k2];
                    while (a < b) {
                        const uint32_t m = (a + b) >> 1;
                        const uint64_t tm = r.deliver[lo2 + m];
                        const bool less = tm != t ? tm < t : eq_less(tm, r.src[lo2 + m], r.seq[lo2 + m], t, sv, qq);
                        if (less) a = m + 1; else b = m;
                    }
                    rank += a;
                }
                popped.deliver[po + rank] = t;
                popped.src[po + rank] = sv;
                popped.seq[po + rank] = qq;
                popped.tag[po + rank] = tg;
            }
        }
    }
    if (S.b >= 0) {   // the batch's remainder becomes the new run, whose cursor starts at its offset
        const EqSrc& q = S.s[S.b];
#pragma unroll
        for (uint32_t u = 0; u < 2; ++u) {
            const uint32_t j = rb_m + lane + 64 * u;
            if (j < rb_e) {
                const uint32_t at = rb_no + (j - rb_m);
                nrun.deliver[at] = pf_t[u];
                nrun.src[at] = pf_s[u];
                nrun.seq[at] = pf_q[u];
                nrun.tag[at] = (q.batch << 32) | pf_p[u];
            }
        }
        for (uint32_t j = rb_m + 128 + lane; j < rb_e; j += 64) {
            const uint32_t at = rb_no + (j - rb_m);
            nrun.deliver[at] = q.deliver[j];
            nrun.src[at] = q.src[j];
            nrun.seq[at] = q.seq[j];
            nrun.tag[at] = (q.batch << 32) | q.pkt[j];
        }
        if (lane == 0) nrun_cur[h] = rb_no;
    }
}


// STAGE: staged events per host -- kEqStage on the normal passes (8 workgroups per CU), 256 on a
// compaction's (whole runs: ~100-250 pending per host on C5, sorted rather than searched in
// global memory)
// keep (a folded compaction's second launch): the sources in S.fold merge their remainders
// [cut, end) into `popped` = the new run at pop_off = its offsets, whose cursor starts there.
template <uint32_t STAGE>
__global__ __launch_bounds__(256) void eqr_merge(uint32_t n_hosts, EqSrcs S, const uint32_t* __restrict__ pop_off,
                                                 EqOut popped, EqOut nrun, const uint32_t* __restrict__ nrun_off,
                                                 uint32_t* __restrict__ nrun_cur, const uint2* __restrict__ ranges,
                                                 uint32_t sort_rank, uint32_t keep = 0) {
    __shared__ uint64_t s_t[4][STAGE], s_q[4][STAGE], s_g[4][STAGE];
    __shared__ uint32_t s_s[4][STAGE];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t h = blockIdx.x * 4 + w;
    if (h >= n_hosts) return;   // wave-uniform; the kernel has no workgroup barrier
    // lane k < S.n holds source k's popped range and its place in the LDS stage
    uint32_t my_lo = 0, my_m = 0;
    if (keep) {
        if (lane < S.n && ((S.fold >> lane) & 1u)) {
            my_lo = S.s[lane].cut[h];
            my_m = S.s[lane].off[h + 1];
        }
        eq_merge_host<STAGE>(h, w, lane, S, my_lo, my_m, pop_off[h], popped, EqOut{}, 0u, nullptr, s_t, s_q, s_g,
                             s_s, sort_rank != 0);
        if (lane == 0) nrun_cur[h] = pop_off[h];
        return;
    }
    if (lane < S.n) {   // eqr_count's (cursor, cut) pairs of this host: one line
        const uint2 r = ranges[(size_t)h * kEqSrcMax + lane];
        my_lo = r.x;
        my_m = r.y;
    }
    eq_merge_host<STAGE>(h, w, lane, S, my_lo, my_m, pop_off[h], popped, nrun, S.b >= 0 ? nrun_off[h] : 0u,
                         nrun_cur, s_t, s_q, s_g, s_s, sort_rank != 0);
}

// the call's totals (popped, kept batch events, head time, left per source) from eqr_count's
// per-block partials, into one word array the host reads with one copy
__global__ __launch_bounds__(1024) void eq_totals(uint32_t n_hosts, uint32_t n_part, const uint32_t* __restrict__ pop_off,
                                                  const uint32_t* __restrict__ keep_off,
                                                  const unsigned long long* __restrict__ part,
                                                  unsigned long long* __restrict__ words,
                                                  unsigned long long* host_words, unsigned long long* marker) {
    __shared__ unsigned long long s_v[16][kEqPart];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // a thread takes whole partial records (independent loads), then one reduction per word
    unsigned long long v[kEqPart];
#pragma unroll
    for (uint32_t j = 0; j < kEqPart; ++j) v[j] = j == 0 ? ~0ull : 0ull;
    for (uint32_t b = threadIdx.x; b < n_part; b += 1024) {
#pragma unroll
        for (uint32_t j = 0; j < kEqPart; ++j) {
            const unsigned long long x = part[(size_t)b * kEqPart + j];
            v[j] = j == 0 ? (x < v[j] ? x : v[j]) : v[j] + x;
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < kEqPart; ++j) {
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long x = __shfl_xor(v[j], o);
            v[j] = j == 0 ? (x < v[j] ? x : v[j]) : v[j] + x;
        }
        if (lane == 0) s_v[w][j] = v[j];
    }
    __syncthreads();
    // host_words (the read-back in the same launch): the words go straight to the pinned host
    // words and the marker the host polls follows them (as rounds.hip readback_mark)
    unsigned long long* out = host_words ? host_words : words;
    if (threadIdx.x < kEqPart) {
        const uint32_t j = threadIdx.x;
        unsigned long long t = s_v[0][j];
        for (int ww = 1; ww < 16; ++ww) t = j == 0 ? (s_v[ww][j] < t ? s_v[ww][j] : t) : t + s_v[ww][j];
        if (j == 0) out[3] = t;
        else out[3 + j] = t;   // words[4 + k] = left of source k
    }
    if (threadIdx.x == 0) {
        out[1] = pop_off[n_hosts];
        out[2] = keep_off ? keep_off[n_hosts] : 0u;
    }
    if (host_words) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // every thread's words reach the host first
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(marker, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// (contract: equeue_priv.h)
shd_status eq_pass(shd_ctx* ctx, const EqSrcs& S, uint64_t window_end, uint32_t* out_off, EqOut out, EqRunBuf* nrun,
                   uint32_t* nrun_cur, uint64_t n_in) {
    // S.fold: the batch's remainder (when there is one) and the folded runs' are merged into the
    // new run by a second merge launch; the first one then only pops
    EqState& Q = ctx->eq;
    hipStream_t s = ctx->stream;
    const uint32_t H = Q.n_hosts;
    unsigned long long* words = Q.next.as<unsigned long long>();
    unsigned long long* part = words + kEqWords;
    const EqOut nr = nrun ? eq_run_out(*nrun) : EqOut{};
    const uint32_t nb = std::min<uint32_t>(kEqCountBlocks, div_up(((uint64_t)H + 1) * kEqLanes, 256));
    // EQ_SEARCH_ONLY=1 ranks staged hosts by the LDS searches alone -- the fallback eq_sort_emit
    // leaves to hosts with equal deliver times, which only this knob puts under volume in the suite
    const uint32_t srt = ctx->knobs.get(K_EQ_SEARCH_ONLY, 0) == 1 ? 0u : 1u;
    SHD_TRY(Q.ranges.ensure((size_t)H * kEqSrcMax * 8));
    eqr_count<<<nb, 256, 0, s>>>(H, S, window_end, Q.pop_cnt.as<uint32_t>(), Q.keep_cnt.as<uint32_t>(), part,
                                 Q.ranges.as<uint2>());
    SHD_HIP(hipGetLastError());
    // the popped offsets and the new run's offsets: one hand-written look-back scan launch (scan.h)
    SHD_TRY(scan_excl2(Q.scan, Q.pop_cnt.as<uint32_t>(), out_off, nrun ? Q.keep_cnt.as<uint32_t>() : nullptr,
                       nrun ? nrun->off.as<uint32_t>() : nullptr, H + 1, s));
    if (n_in && S.fold) {
        EqSrcs SP = S, SK = S;
        SP.b = -1;   // no remainder copy: the keep launch merges the batch's with the folded runs'
        SP.fold = 0;
        SK.fold = S.fold | (S.b >= 0 ? 1u << S.b : 0u);
        SK.b = -1;
        (window_end == ~0ull ? eqr_merge<256> : eqr_merge<kEqStage>)<<<div_up(H, 4), 256, 0, s>>>(
            H, SP, out_off, out, EqOut{}, nullptr, nullptr, Q.ranges.as<uint2>(), srt, 0u);
        eqr_merge<256><<<div_up(H, 4), 256, 0, s>>>(H, SK, nrun->off.as<uint32_t>(), nr, EqOut{}, nullptr, nrun_cur,
                                                     Q.ranges.as<uint2>(), srt, 1u);
    } else if (n_in) {
        (window_end == ~0ull ? eqr_merge<256> : eqr_merge<kEqStage>)<<<div_up(H, 4), 256, 0, s>>>(
            H, S, out_off, out, nr, nrun ? nrun->off.as<uint32_t>() : nullptr, nrun_cur, Q.ranges.as<uint2>(), srt,
            0u);
    }
    SHD_HIP(hipGetLastError());
    if (ctx->spin_wait && ctx->knobs.get(K_SYNC_KERNEL, 1) != 0) {   // totals + read-back in one launch
        volatile unsigned long long* mark = ctx->h_pin + kPinMarker;
        *mark = 0;
        eq_totals<<<1, 1024, 0, s>>>(H, nb, out_off, nrun ? nrun->off.as<uint32_t>() : nullptr, part, words,
                                     ctx->h_pin + kEqPinWord, const_cast<unsigned long long*>(mark));
        SHD_HIP(hipGetLastError());
        return wait_marker(ctx, s);
    }
    eq_totals<<<1, 1024, 0, s>>>(H, nb, out_off, nrun ? nrun->off.as<uint32_t>() : nullptr, part, words, nullptr,
                                 nullptr);
    return readback(ctx, s, kEqPinWord, words, kEqWords * 8);
}

}  // namespace shd
