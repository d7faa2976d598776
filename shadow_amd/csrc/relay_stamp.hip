// The relay's K0 and K1 (overview and the list of units: relay_priv.h), for the narrow pipelines
// (every path latency < 2^32 ns and every deliver - round_end < 2^32): 16-byte event records
// {deliver - round_end, src host, seq - seq_base[src], packet index}.
//   K0 relay_draws      lane per source host: its Xoshiro256++ stream (the only sequential work)
//   K1 relay_stamp_v5   workgroup per 64 source hosts (in source-node order), lane per send:
//                       coalesced loads, path lookup (LDS-staged rows), drop rule, deliver
//                       stamp, scan-based event ids, coalesced stores of status / key / record
//      relay_stamp_v6   the same with the host -> node map in LDS; BIN: the records go straight
//                       into their destination bins (relay_bins.hip)
#include <algorithm>
#include <type_traits>

#include "relay_bins.h"

namespace shd {

#ifndef SHD_DRAW_SLICE
#define SHD_DRAW_SLICE 16
#endif
constexpr uint32_t kDrawSlice = SHD_DRAW_SLICE;   // draws per host per LDS transpose (16: 43 us vs 47 at 8 on C5)

// K0 relay_draws: the only sequential part of the relay -- every source host's Xoshiro256++
// stream (host.rs:218, worker.rs:365) -- as its own kernel: one lane per host (64 consecutive
// hosts per one-wave workgroup), staged through LDS so the draws leave as 64-byte runs.  A send
// draws iff now < sim_end (worker.rs:334-341); send times are non-decreasing within a host (a
// host's sends happen in simulated-time order; the stamp checks it), so the drawing sends are a
// prefix of the host's range, found from its last send (binary search when it is skipped).
#ifndef SHD_K0_WAVES
#define SHD_K0_WAVES 1
#endif
#ifdef SHD_STAMP_PROF
// K0 (relay_draws, tuning builds): per wave, shader clocks of setup / draws / stores and its
// 100 MHz start / end (tools/k0_prof.py)
__device__ unsigned long long g_k0_prof[4096][5];
#endif
constexpr uint32_t kK0Waves = SHD_K0_WAVES;   // waves (64 hosts each) per K0 workgroup
__global__ __launch_bounds__(64 * kK0Waves) void relay_draws(RelayArgs3 a, uint32_t* __restrict__ draw) {
    __shared__ uint32_t s_all[kK0Waves][kDrawSlice][65];   // the draws' top 32 bits (draw_drops)
    __shared__ uint32_t s_beg_all[kK0Waves][64], s_nd_all[kK0Waves][64];
    const uint32_t wv = threadIdx.x >> 6;
    auto& s = s_all[wv];
    uint32_t* s_beg = s_beg_all[wv];
    uint32_t* s_nd = s_nd_all[wv];
    const uint32_t lane = threadIdx.x & 63, hl = (blockIdx.x * kK0Waves + wv) * 64 + lane, h = a.src_lo + hl;
#ifdef SHD_STAMP_PROF
    const uint64_t k0_t0 = __builtin_amdgcn_s_memrealtime();
    uint64_t k0_c = __builtin_amdgcn_s_memtime(), k0_acc[3] = {0, 0, 0};
#define K0_MARK(i) do { const uint64_t t_ = __builtin_amdgcn_s_memtime(); k0_acc[i] += t_ - k0_c; k0_c = t_; } while (0)
#else
#define K0_MARK(i) do { } while (0)
#endif
    uint32_t nd = 0;
    Xoshiro r{0, 0, 0, 0};
    if (hl < a.n_src) {
        // the stream's state first: its loads need nothing below, so they share the first trip
        r = Xoshiro{a.rng[4 * (size_t)h], a.rng[4 * (size_t)h + 1], a.rng[4 * (size_t)h + 2],
                    a.rng[4 * (size_t)h + 3]};
        const uint32_t b = a.src_off[hl], e = a.src_off[hl + 1];
        nd = e - b;
        if (nd && !(a.send_time[e - 1] < a.sim_end)) {   // first send with now >= sim_end
            uint32_t lo = b, hi = e;
            while (lo < hi) {
                const uint32_t m = (lo + hi) >> 1;
                if (a.send_time[m] < a.sim_end) lo = m + 1; else hi = m;
            }
            nd = lo - b;
        }
        s_beg[lane] = b;
    } else {
        s_beg[lane] = 0;
    }
    s_nd[lane] = nd;
    uint32_t mx = nd;
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // the store pattern below: kDrawSlice lanes per host write its kDrawSlice consecutive draws
    // (4 B each), 64 / kDrawSlice hosts per step.  The hosts' (count, start) a lane stores for
    // are the same every slice: read once into registers (read per store, each store waited on
    // two dependent LDS round trips: C5 K0 alone 34.6 -> 30.1 us)
    K0_MARK(0);
    constexpr uint32_t kG = kDrawSlice, kHpg = 64 / kDrawSlice;
    const uint32_t kl = lane % kDrawSlice;
    uint32_t g_nd[kG], g_beg[kG];
#pragma unroll
    for (uint32_t g = 0; g < kG; ++g) {
        const uint32_t hl = g * kHpg + lane / kDrawSlice;
        g_nd[g] = s_nd[hl];
        g_beg[g] = s_beg[hl];
    }
    for (uint32_t j0 = 0; j0 < mx; j0 += kDrawSlice) {
        // the slice's draws in registers first, then to LDS together: a draw written to LDS as it
        // came made the next draw wait for that write (its registers were reused), an LDS round
        // trip per draw on the generator's chain
        uint32_t dv[kDrawSlice];
#pragma unroll
        for (uint32_t k = 0; k < kDrawSlice; ++k) {
            dv[k] = 0u;
            if (j0 + k < nd) dv[k] = (uint32_t)(r.next() >> 32);
        }
        K0_MARK(1);
#pragma unroll
        for (uint32_t k = 0; k < kDrawSlice; ++k) s[k][lane] = dv[k];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        uint32_t v[kG];
#pragma unroll
        for (uint32_t g = 0; g < kG; ++g) v[g] = s[kl][g * kHpg + lane / kDrawSlice];
#pragma unroll
        for (uint32_t g = 0; g < kG; ++g)
            if (j0 + kl < g_nd[g]) draw[g_beg[g] + j0 + kl] = v[g];
        __builtin_amdgcn_wave_barrier();
        K0_MARK(2);
    }
    if (hl < a.n_src) {
        a.rng_out[4 * (size_t)h] = r.s0;
        a.rng_out[4 * (size_t)h + 1] = r.s1;
        a.rng_out[4 * (size_t)h + 2] = r.s2;
        a.rng_out[4 * (size_t)h + 3] = r.s3;
    }
#ifdef SHD_STAMP_PROF
    {
        const uint32_t wid = blockIdx.x * kK0Waves + wv;
        if (lane == 0 && wid < 4096) {
            g_k0_prof[wid][0] = k0_acc[0];
            g_k0_prof[wid][1] = k0_acc[1];
            g_k0_prof[wid][2] = k0_acc[2];
            g_k0_prof[wid][3] = k0_t0;
            g_k0_prof[wid][4] = __builtin_amdgcn_s_memrealtime();
        }
    }
#endif
#undef K0_MARK
}

// A path-table entry from global memory through an explicit global (addrspace 1) pointer.  Next
// to an LDS-staged alternative a plain `cond ? s_rows[i] : path[j]` lets the compiler select the
// pointer and issue a flat load, and a flat load makes every later s_waitcnt wait for the
// wave's outstanding stores as well -- which serialised the stamp's record stores.
__device__ __forceinline__ uint2 path_global(const uint2* p, size_t i) {
    const unsigned long long v = ((const __attribute__((address_space(1))) unsigned long long*)p)[i];
    return make_uint2((uint32_t)v, (uint32_t)(v >> 32));
}

// K1 relay_stamp_v5: a workgroup owns kS5Hosts source hosts taken in source-node order
// (R.order), so its path lookups stay in one or two table rows, staged in LDS when they fit.
// The hosts' sends (one contiguous range per host) form one list, processed in chunks of
// kS5Cap positions with consecutive lanes on consecutive positions (coalesced inside every
// host's range).  No sequential work is left: lane per send, the raw loads, the draw (K0), the
// destination node and path, the drop rule and deliver stamp (worker.rs:370-402); a block-wide
// exclusive scan of the sent flags gives every sent packet its event id (host.rs:580-584).
constexpr uint32_t kS5Per = 4;                  // sends per thread per chunk
constexpr uint32_t kS5Cap = 256 * kS5Per;
constexpr uint32_t kS5RowLds = 2048;            // staged path-table entries (16 KB)

// (round 6: the chunk's loads issued together -- the sends' fields, then the destinations' nodes,
// then the path entries, each a batch of independent loads -- instead of one guarded chain per
// send; CH as relay_stamp_v6's)
template <bool CH>
__global__ __launch_bounds__(256) void relay_stamp_v5(RelayArgs3 a, const uint32_t* __restrict__ draw) {
    __shared__ uint2 s_rows[kS5RowLds];
    __shared__ uint16_t s_scan[kS5Cap + 1];
    __shared__ uint32_t s_host[kS5Hosts], s_beg[kS5Hosts], s_pre[kS5Hosts + 1], s_node[kS5Hosts];
    __shared__ uint32_t s_rowof[kS5Hosts], s_rownode[kS5Hosts], s_run[kS5Hosts], s_base[kS5Hosts];
    __shared__ uint32_t s_wsum[4], s_nrows;
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t h0 = blockIdx.x * kS5Hosts;
    const uint32_t nh = min(kS5Hosts, a.n_src - h0);
    if (tid < 64) {   // wave 0: this workgroup's hosts, their ranges (prefix) and staged rows
        uint32_t len = 0, nd = 0;
        if (tid < nh) {
            const uint32_t h = a.order[h0 + tid];
            const uint32_t b = a.src_off[h - a.src_lo];
            len = a.src_off[h - a.src_lo + 1] - b;
            nd = a.host_node[h];
            s_host[tid] = h;
            s_beg[tid] = b;
            s_node[tid] = nd;
            s_run[tid] = 0;
            s_base[tid] = a.abs_seq ? (uint32_t)a.next_id[h] : 0u;
        }
        uint32_t incl = len;
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        if (tid < nh) s_pre[tid + 1] = incl;
        if (tid == 0) s_pre[0] = 0;
        const uint32_t prev = __shfl_up(nd, 1);
        const bool first = tid < nh && (tid == 0 || nd != prev);
        const uint64_t fm = __ballot(first);
        if (tid < nh) {
            const uint32_t ri = (uint32_t)__popcll(fm & ((2ull << tid) - 1ull)) - 1u;
            s_rowof[tid] = ri;
            if (first) s_rownode[ri] = nd;
        }
        if (tid == 0) s_nrows = (uint32_t)__popcll(fm);
    }
    __syncthreads();
    const bool staged = (uint64_t)s_nrows * a.n_nodes <= kS5RowLds;
    if (staged) {
        const uint32_t tot = s_nrows * a.n_nodes;
        for (uint32_t e = tid; e < tot; e += 256) {
            const uint32_t rr = e / a.n_nodes, c = e - rr * a.n_nodes;
            s_rows[e] = a.path[(size_t)s_rownode[rr] * a.n_nodes + c];
        }
    }
    __syncthreads();
    const uint32_t T = s_pre[nh];
    uint64_t min_d = ~0ull, min_l = ~0ull;
    bool wide = false, disorder = false;
    for (uint32_t c0 = 0; c0 < T; c0 += kS5Cap) {
        const uint32_t cn = min(kS5Cap, T - c0);
        uint8_t st[kS5Per];
        uint32_t doff[kS5Per], dst[kS5Per], idx[kS5Per], hl[kS5Per], dn[kS5Per];
        bool k0[kS5Per];
        // (a) owners and packet indices (positions past the chunk clamped onto its last packet,
        // so every load below is in bounds and unconditional)
#pragma unroll
        for (uint32_t i = 0; i < kS5Per; ++i) {
            const uint32_t gp = c0 + min(tid + 256 * i, cn - 1);
            uint32_t lo = 0, hi = nh;       // s_pre[lo] <= gp < s_pre[lo + 1]
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_pre[mid] <= gp) lo = mid; else hi = mid;
            }
            hl[i] = lo;
            const uint32_t k = gp - s_pre[lo];
            k0[i] = k == 0;
            idx[i] = s_beg[lo] + k;
        }
        // (b) the sends' fields, (c) their destinations' nodes, (d) the path entries
        uint64_t now[kS5Per], prv[kS5Per];
        std::conditional_t<CH, double, uint32_t> rv[kS5Per];
        uint32_t pay[kS5Per];
#pragma unroll
        for (uint32_t i = 0; i < kS5Per; ++i) {
            now[i] = a.send_time[idx[i]];
            prv[i] = a.send_time[idx[i] - (k0[i] ? 0u : 1u)];
            dst[i] = a.dst_host[idx[i]];
            pay[i] = a.payload[idx[i]];
            if constexpr (CH) rv[i] = a.chance[idx[i]];
            else rv[i] = draw[idx[i]];
        }
#pragma unroll
        for (uint32_t i = 0; i < kS5Per; ++i) dn[i] = a.host_node[min(dst[i], a.n_hosts - 1)];
        uint2 pp[kS5Per];
#pragma unroll
        for (uint32_t i = 0; i < kS5Per; ++i)
            pp[i] = staged ? s_rows[s_rowof[hl[i]] * a.n_nodes + dn[i]]
                           : path_global(a.path, (size_t)s_node[hl[i]] * a.n_nodes + dn[i]);
#pragma unroll
        for (uint32_t i = 0; i < kS5Per; ++i) {
            const uint32_t pos = tid + 256 * i;
            st[i] = kStSkipped;
            doff[i] = 0;
            if (pos < cn) {
                // a drawing send after a skipped one breaks K0's prefix rule
                disorder |= !k0[i] & (now[i] < a.sim_end) & !(prv[i] < a.sim_end);
                if (dst[i] >= a.n_hosts) {      // "No host ID for dest address" (worker.rs:350-355)
                    atomicMin(&a.red[3], (unsigned long long)idx[i]);
                } else if (now[i] < a.sim_end) {
                    const double reliability = (double)one_minus(__uint_as_float(pp[i].y));
                    bool tie = false;
                    bool ge;
                    if constexpr (CH) ge = rv[i] >= reliability;
                    else ge = draw_drops(rv[i], reliability, tie);
                    wide |= tie;   // a draw whose low bits would decide: redo the round on pipeline 1
                    if (!(now[i] < a.bootstrap_end) && ge && pay[i] > 0) {
                        st[i] = kStDropped;
                    } else {
                        uint64_t tt = now[i] + pp[i].x;
                        if (tt < a.round_end) tt = a.round_end;
                        const uint64_t dd = tt - a.round_end;
                        wide |= (dd >> 32) != 0;
                        min_d = tt < min_d ? tt : min_d;
                        min_l = pp[i].x < min_l ? pp[i].x : min_l;
                        doff[i] = (uint32_t)dd;
                        st[i] = kStSent;
                    }
                }
            }
            s_scan[pos] = st[i] == kStSent ? 1 : 0;
        }
        __syncthreads();
        {   // block-wide exclusive scan of the sent flags (kS5Per consecutive entries per thread)
            uint32_t v[kS5Per], sum = 0;
#pragma unroll
            for (uint32_t i = 0; i < kS5Per; ++i) {
                v[i] = s_scan[tid * kS5Per + i];
                sum += v[i];
            }
            uint32_t incl = sum;
#pragma unroll
            for (uint32_t o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(incl, o);
                if (lane >= o) incl += y;
            }
            if (lane == 63) s_wsum[w] = incl;
            __syncthreads();
            uint32_t run = incl - sum;
            for (uint32_t ww = 0; ww < w; ++ww) run += s_wsum[ww];
#pragma unroll
            for (uint32_t i = 0; i < kS5Per; ++i) {
                s_scan[tid * kS5Per + i] = (uint16_t)run;
                run += v[i];
            }
            if (tid == 255) s_scan[kS5Cap] = (uint16_t)run;
        }
        __syncthreads();
        // stores; event id = host's running count + sent sends before this one in its range
#pragma unroll
        for (uint32_t i = 0; i < kS5Per; ++i) {
            const uint32_t pos = tid + 256 * i;
            if (pos < cn) {
                a.status[idx[i]] = st[i];
                a.key[idx[i]] = st[i] == kStSent ? dst[i] : a.n_hosts;
                if (st[i] == kStSent) {
                    const uint32_t first = max(s_pre[hl[i]], c0) - c0;
                    const uint32_t local = s_base[hl[i]] + s_run[hl[i]] + s_scan[pos] - s_scan[first];
                    a.rec[idx[i]] = make_uint4(doff[i], s_host[hl[i]], local, idx[i]);
                    if (a.counts) atomicAdd(&a.counts[(size_t)s_node[hl[i]] * a.n_nodes + dn[i]], 1ull);
                }
            }
        }
        __syncthreads();
        if (tid < nh) {   // running counts for the next chunk
            const uint32_t pb = max(s_pre[tid], c0), pe = min(s_pre[tid + 1], c0 + cn);
            if (pe > pb) s_run[tid] += s_scan[pe - c0] - s_scan[pb - c0];
        }
        __syncthreads();
    }
    uint64_t ns = 0;
    if (tid < nh) {
        const size_t h = s_host[tid];
        if (a.chance || a.keep_rng)
            for (int k = 0; k < 4; ++k) a.rng_out[4 * h + k] = a.rng[4 * h + k];
        ns = s_run[tid];
        a.next_id_out[h] = a.next_id[h] + ns;
    }
    min_d = wave_min_u64(min_d);
    min_l = wave_min_u64(min_l);
    for (int o = 32; o > 0; o >>= 1) ns += __shfl_xor(ns, o);
    const bool any_wide = __ballot(wide) != 0, any_disorder = __ballot(disorder) != 0;
    if (lane == 0) {
        if (min_d != ~0ull) atomicMin(&a.red[0], (unsigned long long)min_d);
        if (min_l != ~0ull) atomicMin(&a.red[1], (unsigned long long)min_l);
        if (ns) atomicAdd(&a.red[2], (unsigned long long)ns);
        if (any_wide) atomicOr(&a.red[4], 1ull);
        if (any_disorder) atomicOr(&a.red[5], 1ull);
    }
}

// K1 (small node count): relay_stamp_v6 is relay_stamp_v5 with the host -> node map resident in
// LDS, bit-packed at ceil(log2 n_nodes) bits per host (C5: 100k hosts x 10 bits = 125 KB), so
// the destination-node lookup -- otherwise one random 64-byte L2 request per send, the stamp's
// dominant cost -- becomes an LDS read.  One persistent 1024-thread workgroup per CU loads the
// packed map once and walks the host groups (kS5Hosts hosts each, in source-node order).
constexpr uint32_t kS6Threads = 1024;
#ifndef SHD_S6PER
#define SHD_S6PER 4   // sends per thread and chunk (5 and 6 spill registers: slower)
#endif
constexpr uint32_t kS6Per = SHD_S6PER;
constexpr uint32_t kS6Cap = kS6Threads * kS6Per;
constexpr uint32_t kS6FixedLds = kS5RowLds * 8 + (kS6Cap + 2) * 2 + kS6Cap + 4096;   // rows + scan + owners + small

__device__ __forceinline__ uint32_t packed_get(const uint32_t* t, uint32_t j, uint32_t bits) {
    const uint32_t o = j * bits, w = o >> 5, sh = o & 31;
    uint64_t v = t[w];
    if (sh + bits > 32) v |= (uint64_t)t[w + 1] << 32;
    return (uint32_t)(v >> sh) & ((1u << bits) - 1u);
}

#ifdef SHD_STAMP_PROF
// tuning builds only (tools/stamp_prof.sh): shader clocks per phase, summed over workgroups
__device__ unsigned long long g_stamp_prof[12];
#define SP_MARK(slot) do { if (threadIdx.x == 0) { const uint64_t t_ = __builtin_amdgcn_s_memtime(); \
    sp_acc[slot] += t_ - sp_t; sp_t = t_; } } while (0)
#else
#define SP_MARK(slot) do { } while (0)
#endif

// BIN (pipeline v7): every packet with a valid destination is also placed, sent or not, into
// its destination bin (kBinDst consecutive destinations): the workgroup's slots of bin b are
// the segment bin_base[b] + seg_pre[g][b] counted by relay_bin_hist; the slot inside the
// segment comes from an LDS counter (one u32 per bin holding the absolute next slot).  The records carry the
// status and the destination's low bits so bin_sort_v7 can filter and split them.

// CH: the batch carries f64 chances (a.chance) instead of K0's draws.  A template parameter, not
// a run-time select: `a.chance ? chance64[i] : draw[i]` compiled to a branch whose join moved the
// loaded value with an s_waitcnt vmcnt(0), so each of a thread's kS6Per load sets waited for the
// one before it (four memory round trips per chunk instead of one).
// MAP = false (round 6, C5b): the host -> node map does not fit the LDS (50k nodes: 16 bits x
// 100k hosts), so each chunk gathers its destinations' nodes from global memory (a 400 KB array,
// L2-resident) and, the rows being too long to stage, its path entries from the packed table --
// each a batch of unconditional loads -- and the records still go straight to their bins
// (pipeline 7 instead of pipeline 3's radix sort: the bins need only the slot counters in LDS).
template <bool BIN, bool CH, bool MAP = true>
__global__ __launch_bounds__(kS6Threads) void relay_stamp_v6(RelayArgs3 a, const uint32_t* __restrict__ draw,
                                                             const uint32_t* __restrict__ packed,
                                                             uint32_t n_words, uint32_t bits) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_tbl[];   // packed host -> node
    // BIN: per bin, the next record slot of this workgroup's segment (absolute: bin base + segment
    // start + records placed), so placing a record is one LDS atomic -- no per-record loads of
    // the bases (a scattered load costs ~64 TA cycles per wave instruction: ~30 us of the stamp)
    uint32_t* s_slot = s_tbl + n_words;
    if (BIN && a.red[6]) return;   // a bin overflowed bin_sort_v7's LDS stage: the host reruns v3
    constexpr uint32_t kW = kS6Threads / 64;
    static_assert(kS6Per * kW <= 64, "one wave scans the chunk's (i, wave) sent totals");
    __shared__ uint2 s_rows[kS5RowLds];
    __shared__ uint32_t s_host[kS5Hosts], s_beg[kS5Hosts], s_pre[kS5Hosts + 1], s_node[kS5Hosts];
    __shared__ uint32_t s_rowof[kS5Hosts], s_rownode[kS5Hosts], s_run[kS5Hosts], s_base[kS5Hosts];
    __shared__ uint32_t s_off[kS5Hosts];    // a host's event id = s_off + the chunk's sent prefix
    __shared__ uint32_t s_wt[64], s_nrows;  // sent sends per (i, wave) of the chunk
    __shared__ uint8_t s_own[kS6Cap];   // chunk position -> host slot in the group
    // next group's distinct source nodes: up to one per host of the group (a group of kS5Hosts
    // hosts spans at most kS5Hosts nodes; the prefetch stages pn * n_nodes <= kS5RowLds entries)
    __shared__ uint32_t s_pfnode[kS5Hosts], s_pfn;
    static_assert(kS5RowLds % kS6Threads == 0, "row prefetch: whole entries per thread");
    constexpr uint32_t kPf = kS5RowLds / kS6Threads;
    uint2 pf[kPf];             // the next group's staged path rows, prefetched during this group
    bool have_pf = false;
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#ifdef SHD_STAMP_PROF
    uint64_t sp_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, sp_t = __builtin_amdgcn_s_memtime();
#endif
    if constexpr (MAP)
        for (uint32_t i = tid; i < n_words; i += kS6Threads) s_tbl[i] = packed[i];
    if (BIN)
        for (uint32_t b = tid; b < a.n_bins; b += kS6Threads)
            s_slot[b] = a.bin_base[b] + a.seg_pre[(size_t)blockIdx.x * a.n_bins + b];
    const uint32_t n_groups = (a.n_src + a.gs - 1) / a.gs;
    uint64_t min_d = ~0ull, min_l = ~0ull, ns_total = 0;
    bool wide = false, disorder = false;
    // wave 0 keeps the next group's host descriptors in registers: order[] is fetched when a
    // group starts and the dependent src_off / host_node / next_id loads are issued once its
    // path rows are staged, so neither latency sits on the critical path of the next group
    uint32_t p_h = 0, p_b = 0, p_len = 0, p_nd = 0, p_base = 0;
    auto fetch_hosts = [&](uint32_t g) {
        const uint32_t hh0 = g * a.gs;
        if (g < n_groups && tid < min(a.gs, a.n_src - hh0)) {
            p_b = a.src_off[p_h - a.src_lo];
            p_len = a.src_off[p_h - a.src_lo + 1] - p_b;
            p_nd = a.host_node[p_h];
            p_base = a.abs_seq ? (uint32_t)a.next_id[p_h] : 0u;
        }
    };
    if (tid < 64 && blockIdx.x < n_groups && tid < min(a.gs, a.n_src - blockIdx.x * a.gs)) {
        p_h = a.order[blockIdx.x * a.gs + tid];
    }
    if (tid < 64) fetch_hosts(blockIdx.x);
    // 16 threads per host slot fill the owner map of the chunk starting at position cb
    static_assert(kS6Threads == kS5Hosts * 16, "owner fill: 16 threads per host slot");
    auto fill_owner = [&](uint32_t cb, uint32_t nh) {
        const uint32_t hh = tid >> 4, sub = tid & 15;
        if (hh < nh) {
            const uint32_t pb = max(s_pre[hh], cb), pe = min(s_pre[hh + 1], cb + kS6Cap);
            for (uint32_t p = pb + sub; p < pe; p += 16) s_own[p - cb] = (uint8_t)hh;
        }
    };
    const uint64_t* __restrict__ chance64 = reinterpret_cast<const uint64_t*>(a.chance);
    for (uint32_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const uint32_t h0 = grp * a.gs;
        const uint32_t nh = min(a.gs, a.n_src - h0);
        const uint32_t nxt = grp + gridDim.x;
        __syncthreads();   // the previous group's host arrays / rows are no longer read
        SP_MARK(0);
        if (tid < 64) {
            uint32_t len = 0, nd = 0;
            if (tid < nh) {
                len = p_len;
                nd = p_nd;
                s_host[tid] = p_h;
                s_beg[tid] = p_b;
                s_node[tid] = nd;
                s_run[tid] = 0;
                s_base[tid] = p_base;
            }
            if (nxt < n_groups && tid < min(a.gs, a.n_src - nxt * a.gs))
                p_h = a.order[nxt * a.gs + tid];
            uint32_t incl = len;
            for (uint32_t o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(incl, o);
                if (lane >= o) incl += y;
            }
            if (tid < nh) s_pre[tid + 1] = incl;
            if (tid == 0) s_pre[0] = 0;
            const uint32_t prev = __shfl_up(nd, 1);
            const bool first = tid < nh && (tid == 0 || nd != prev);
            const uint64_t fm = __ballot(first);
            if (tid < nh) {
                const uint32_t ri = (uint32_t)__popcll(fm & ((2ull << tid) - 1ull)) - 1u;
                s_rowof[tid] = ri;
                if (first) s_rownode[ri] = nd;
            }
            if (tid == 0) s_nrows = (uint32_t)__popcll(fm);
        }
        __syncthreads();
        SP_MARK(1);
        const bool staged = MAP && (uint64_t)s_nrows * a.n_nodes <= kS5RowLds;
        if (staged) {
            const uint32_t tot = s_nrows * a.n_nodes;
            if (have_pf) {   // rows loaded during the previous group (same node list by construction)
#pragma unroll
                for (uint32_t j = 0; j < kPf; ++j)
                    if (tid + j * kS6Threads < tot) s_rows[tid + j * kS6Threads] = pf[j];
            } else {
                for (uint32_t e = tid; e < tot; e += kS6Threads) {
                    const uint32_t rr = e / a.n_nodes, c = e - rr * a.n_nodes;
                    s_rows[e] = a.path[(size_t)s_rownode[rr] * a.n_nodes + c];
                }
            }
        }
        have_pf = false;
        fill_owner(0, nh);
        if (tid < 64) fetch_hosts(nxt);
        __syncthreads();
        SP_MARK(2);
        const uint32_t T = s_pre[nh];
        for (uint32_t c0 = 0; c0 < T; c0 += kS6Cap) {
            const uint32_t cn = min(kS6Cap, T - c0);
            if (c0 == 0 && tid < 64) {   // the next group's distinct source nodes, as at its start
                const uint32_t nh2 = nxt < n_groups ? min(a.gs, a.n_src - nxt * a.gs) : 0u;
                const uint32_t nd = p_nd, prev = __shfl_up(nd, 1);
                const bool first = tid < nh2 && (tid == 0 || nd != prev);
                const uint64_t fm = __ballot(first);
                if (first) {
                    const uint32_t ri = (uint32_t)__popcll(fm & ((2ull << tid) - 1ull)) - 1u;
                    s_pfnode[ri] = nd;   // ri < nh2 <= kS5Hosts
                }
                if (tid == 0) s_pfn = (uint32_t)__popcll(fm);
            }
            // (a) positions -> packet indices through the owner map (positions past the chunk end
            // are clamped onto its last packet so every load below is in bounds and unconditional)
            // hl: the host slot, plus kFirst / kLast when the position is the host's first / last send
            // (the position inside the host is needed only for those and the load below: one
            // register per position less)
            constexpr uint32_t kFirst = 0x100, kLast = 0x200, kSlot = 0xFF;
            uint32_t idx[kS6Per], hl[kS6Per];
#pragma unroll
            for (uint32_t i = 0; i < kS6Per; ++i) {
                const uint32_t q = min(tid + kS6Threads * i, cn - 1);
                const uint32_t gp = c0 + q;
                const uint32_t lo = s_own[q];       // s_pre[lo] <= gp < s_pre[lo + 1]
                const uint32_t k = gp - s_pre[lo];
                hl[i] = lo | (k == 0 ? kFirst : 0u) | (gp + 1 == s_pre[lo + 1] ? kLast : 0u);
                idx[i] = s_beg[lo] + k;
            }
            SP_MARK(8);
            // (b) all loads of the chunk in flight together
            uint64_t now[kS6Per], prv[kS6Per];
            std::conditional_t<CH, uint64_t, uint32_t> rv[kS6Per];
            uint32_t dst[kS6Per], pay[kS6Per];
#pragma unroll
            for (uint32_t i = 0; i < kS6Per; ++i) {
                now[i] = a.send_time[idx[i]];
                prv[i] = a.send_time[idx[i] - ((hl[i] & kFirst) ? 0u : 1u)];
                dst[i] = a.dst_host[idx[i]];
                pay[i] = a.payload[idx[i]];
                if constexpr (CH) rv[i] = chance64[idx[i]];
                else rv[i] = draw[idx[i]];
            }
            SP_MARK(9);
            uint32_t dn[kS6Per];
            uint2 pg[kS6Per];   // (!MAP: the path entries, gathered together)
            if constexpr (!MAP) {
#pragma unroll
                for (uint32_t i = 0; i < kS6Per; ++i) dn[i] = a.host_node[min(dst[i], a.n_hosts - 1)];
#pragma unroll
                for (uint32_t i = 0; i < kS6Per; ++i)   // (unconditional: a select on `staged` made
                                                         // each a branch, waited at its join)
                    pg[i] = path_global(a.path, (size_t)s_node[hl[i] & kSlot] * a.n_nodes + dn[i]);
            }
            // (c) decisions
            uint8_t st[kS6Per];
            uint32_t doff[kS6Per];
#pragma unroll
            for (uint32_t i = 0; i < kS6Per; ++i) {
                const uint32_t pos = tid + kS6Threads * i;
                st[i] = kStSkipped;
                doff[i] = 0;
                if constexpr (MAP) dn[i] = 0;
                if (pos < cn) {
                    // a drawing send after a skipped one breaks K0's prefix rule
                    // (bitwise, not short-circuit: a `&&` chain let the compiler sink prv's load
                    // under the now[i] test -- a second, dependent memory round trip)
                    disorder |= !(hl[i] & kFirst) & (now[i] < a.sim_end) & !(prv[i] < a.sim_end);
                    if (dst[i] >= a.n_hosts) {      // "No host ID for dest address" (worker.rs:350-355)
                        atomicMin(&a.red[3], (unsigned long long)idx[i]);
                    } else if (now[i] < a.sim_end) {
                        uint2 pp;
                        if constexpr (MAP) {
                            dn[i] = packed_get(s_tbl, dst[i], bits);
                            pp = staged ? s_rows[s_rowof[hl[i] & kSlot] * a.n_nodes + dn[i]]
                                        : path_global(a.path, (size_t)s_node[hl[i] & kSlot] * a.n_nodes + dn[i]);
                        } else {
                            pp = pg[i];   // (no row staging without the LDS map: see `staged`)
                        }
                        const double reliability = (double)one_minus(__uint_as_float(pp.y));
                        bool tie = false;
                        const bool ge = CH ? __longlong_as_double((long long)rv[i]) >= reliability
                                           : draw_drops((uint32_t)rv[i], reliability, tie);
                        wide |= tie;   // a draw whose low bits would decide: redo the round on pipeline 1
                        if (!(now[i] < a.bootstrap_end) && ge && pay[i] > 0) {
                            st[i] = kStDropped;
                        } else {
                            uint64_t tt = now[i] + pp.x;
                            if (tt < a.round_end) tt = a.round_end;
                            const uint64_t dd = tt - a.round_end;
                            wide |= (dd >> 32) != 0;
                            min_d = tt < min_d ? tt : min_d;
                            min_l = pp.x < min_l ? pp.x : min_l;
                            doff[i] = (uint32_t)dd;
                            st[i] = kStSent;
                        }
                    }
                }
            }
            SP_MARK(10);
            // the chunk's event ids without a block scan: sent flags -> one ballot per (i, wave),
            // the 64 wave totals through LDS, and every wave scans those itself (one barrier).
            // Position order is pos = tid + kS6Threads * i: i-major, then wave, then lane.
            uint64_t sm[kS6Per];
#pragma unroll
            for (uint32_t i = 0; i < kS6Per; ++i) sm[i] = __ballot(st[i] == kStSent);
            if (lane == 0) {
#pragma unroll
                for (uint32_t i = 0; i < kS6Per; ++i) s_wt[i * kW + w] = (uint32_t)__popcll(sm[i]);
            }
            __syncthreads();
            SP_MARK(3);
            if (c0 == 0) {   // prefetch the next group's rows; they land while this group runs
                const uint32_t pn = s_pfn;
                if (MAP && pn && (uint64_t)pn * a.n_nodes <= kS5RowLds) {
#pragma unroll
                    for (uint32_t j = 0; j < kPf; ++j) {
                        const uint32_t e = tid + j * kS6Threads;
                        if (e < pn * a.n_nodes) {
                            const uint32_t rr = e / a.n_nodes, c = e - rr * a.n_nodes;
                            pf[j] = path_global(a.path, (size_t)s_pfnode[rr] * a.n_nodes + c);
                        }
                    }
                    have_pf = true;
                }
            }
            uint32_t pre[kS6Per];   // sent sends of the chunk before each own position
            {
                const uint32_t v = lane < kS6Per * kW ? s_wt[lane] : 0u;
                uint32_t incl = v;
#pragma unroll
                for (uint32_t o = 1; o < 64; o <<= 1) {
                    const uint32_t y = __shfl_up(incl, o);
                    if (lane >= o) incl += y;
                }
                const uint32_t ex = incl - v;
#pragma unroll
                for (uint32_t i = 0; i < kS6Per; ++i)
                    pre[i] = (uint32_t)__shfl((int)ex, (int)(i * kW + w)) +
                             __builtin_amdgcn_mbcnt_hi((uint32_t)(sm[i] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)sm[i], 0u));
            }
            // a host's first position in the chunk (its first send, or the chunk's start) fixes the
            // offset of its ids in this chunk: id = s_off + pre
#pragma unroll
            for (uint32_t i = 0; i < kS6Per; ++i) {
                const uint32_t pos = tid + kS6Threads * i;
                const uint32_t h = hl[i] & kSlot;
                if (pos < cn && ((hl[i] & kFirst) || pos == 0)) s_off[h] = s_base[h] + s_run[h] - pre[i];
            }
            __syncthreads();
            SP_MARK(4);
            // stores: the ids, each record's slot in its bin (one LDS atomic), then every store; a
            // host's last position in the chunk carries its sent count into s_run
            uint32_t local[kS6Per], slot[kS6Per];
#pragma unroll
            for (uint32_t i = 0; i < kS6Per; ++i) {
                const uint32_t pos = tid + kS6Threads * i;
                local[i] = 0;
                slot[i] = 0;
                if (pos < cn) {
                    const uint32_t h = hl[i] & kSlot, so = s_off[h];
                    if (st[i] == kStSent) local[i] = so + pre[i];
                    if (BIN && dst[i] < a.n_hosts) {
                        uint32_t dl;
                        slot[i] = atomicAdd(&s_slot[dst_bin(a, dst[i], dl)], 1u);
                    }
                    if (pos == cn - 1 || (hl[i] & kLast))
                        s_run[h] = so + pre[i] + (st[i] == kStSent ? 1u : 0u) - s_base[h];
                }
            }
#pragma unroll
            for (uint32_t i = 0; i < kS6Per; ++i) {
                const uint32_t pos = tid + kS6Threads * i;
                if (pos < cn) {
#ifndef SHD_PRICE_STATUS   // (tuning builds: price the stamp's stores away; wrong output)
                    a.status[idx[i]] = st[i];
#endif
                    if (!BIN) {
                        a.key[idx[i]] = st[i] == kStSent ? dst[i] : a.n_hosts;
                        if (st[i] == kStSent) a.rec[idx[i]] = make_uint4(doff[i], s_host[hl[i] & kSlot], local[i], idx[i]);
                    } else if (dst[i] < a.n_hosts) {
                        uint32_t dl;
                        dst_bin(a, dst[i], dl);
#if defined(SHD_PRICE_REC) && SHD_PRICE_REC == 2
                        if (slot[i] == 0xFFFFFFFFu)   // never: the record store priced away
#elif defined(SHD_PRICE_REC)
                        slot[i] = idx[i];             // coalesced by packet index instead of the bin slot
#endif
                        a.rec[slot[i]] = make_uint4(doff[i],
                                                    s_host[hl[i] & kSlot] | (dl << 18) |
                                                        ((uint32_t)st[i] << 24),
                                                    local[i], idx[i]);
                    }
                    if (st[i] == kStSent && a.counts)
                        atomicAdd(&a.counts[(size_t)s_node[hl[i] & kSlot] * a.n_nodes + dn[i]], 1ull);
                }
            }
            if (c0 + kS6Cap < T) fill_owner(c0 + kS6Cap, nh);   // s_own of this chunk is consumed
            __syncthreads();
            SP_MARK(5);
        }
        if (tid < nh) {
            const size_t h = s_host[tid];
            if (a.chance || a.keep_rng)
                for (int k = 0; k < 4; ++k) a.rng_out[4 * h + k] = a.rng[4 * h + k];
            ns_total += s_run[tid];
            a.next_id_out[h] = a.next_id[h] + s_run[tid];
        }
    }
#ifdef SHD_STAMP_PROF
    SP_MARK(7);
    if (tid == 0)
        for (int q = 0; q < 12; ++q) atomicAdd(&g_stamp_prof[q], (unsigned long long)sp_acc[q]);
#endif
    min_d = wave_min_u64(min_d);
    min_l = wave_min_u64(min_l);
    for (int o = 32; o > 0; o >>= 1) ns_total += __shfl_xor(ns_total, o);
    const bool any_wide = __ballot(wide) != 0, any_disorder = __ballot(disorder) != 0;
#ifndef SHD_RED_PER_WAVE   // (tuning A/B: one set of global atomics per wave)
    // the workgroup's 16 waves combine in LDS first: one atomic per word per workgroup instead of
    // per wave -- the grid's waves all end together, and 4096 atomics on the same few words
    // serialise at the memory side (~12 ns each)
    __shared__ unsigned long long s_red[3][kS6Threads / 64];
    __shared__ uint32_t s_flag[kS6Threads / 64];
    if (lane == 0) {
        s_red[0][w] = min_d;
        s_red[1][w] = min_l;
        s_red[2][w] = ns_total;
        s_flag[w] = (any_wide ? 1u : 0u) | (any_disorder ? 2u : 0u);
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long md = ~0ull, ml = ~0ull, ns = 0;
        uint32_t fl = 0;
        for (uint32_t k = 0; k < kS6Threads / 64; ++k) {
            md = s_red[0][k] < md ? s_red[0][k] : md;
            ml = s_red[1][k] < ml ? s_red[1][k] : ml;
            ns += s_red[2][k];
            fl |= s_flag[k];
        }
        if (md != ~0ull) atomicMin(&a.red[0], md);
        if (ml != ~0ull) atomicMin(&a.red[1], ml);
        if (ns) atomicAdd(&a.red[2], ns);
        if (fl & 1u) atomicOr(&a.red[4], 1ull);
        if (fl & 2u) atomicOr(&a.red[5], 1ull);
    }
#else
    if (lane == 0) {
        if (min_d != ~0ull) atomicMin(&a.red[0], (unsigned long long)min_d);
        if (min_l != ~0ull) atomicMin(&a.red[1], (unsigned long long)min_l);
        if (ns_total) atomicAdd(&a.red[2], (unsigned long long)ns_total);
        if (any_wide) atomicOr(&a.red[4], 1ull);
        if (any_disorder) atomicOr(&a.red[5], 1ull);
    }
#endif
}

void relay_launch_draws(shd_ctx* ctx, const RelayArgs3& a) {
    RelayState& R = ctx->relay;
    if (a.chance || R.cpu_draws || !R.n_src) return;   // (shd_relay_flush filled the draws from the CPU's)
    relay_draws<<<div_up(R.n_src, 64 * kK0Waves), 64 * kK0Waves, 0, ctx->stream>>>(a, R.draws.as<uint32_t>());
}

void relay_launch_stamp(shd_ctx* ctx, const RelayArgs3& a) {
    RelayState& R = ctx->relay;
    hipStream_t s = ctx->stream;
    if (R.n_src == 0) {
    } else if (R.hn_bits) {   // host -> node map fits the LDS: persistent stamp, no node gathers
        const uint32_t groups = div_up(R.n_src, kS5Hosts);
        auto* k = a.chance ? &relay_stamp_v6<false, true> : &relay_stamp_v6<false, false>;
        k<<<std::min<uint32_t>(groups, (uint32_t)ctx->n_cu), kS6Threads, (size_t)R.hn_words * 4, s>>>(
            a, R.draws.as<uint32_t>(), R.hn_packed.as<uint32_t>(), R.hn_words, R.hn_bits);
    } else {
        (a.chance ? relay_stamp_v5<true> : relay_stamp_v5<false>)<<<div_up(R.n_src, kS5Hosts), 256, 0, s>>>(
            a, R.draws.as<uint32_t>());
    }
}

void relay_launch_stamp_bins(shd_ctx* ctx, const RelayArgs3& a, uint32_t G, size_t lds) {
    RelayState& R = ctx->relay;
    // (no LDS host map -- e.g. C5b's 50k nodes -- : the stamp gathers the destinations' nodes)
    auto* stamp = R.hn_bits ? (a.chance ? &relay_stamp_v6<true, true> : &relay_stamp_v6<true, false>)
                            : (a.chance ? &relay_stamp_v6<true, true, false> : &relay_stamp_v6<true, false, false>);
    stamp<<<G, kS6Threads, lds, ctx->stream>>>(
        a, R.draws.as<uint32_t>(), R.hn_packed.as<uint32_t>(), R.hn_bits ? R.hn_words : 0u, R.hn_bits);
}

size_t relay_stamp_bins_static_lds() {
    // the stamp's static LDS, asked once (a function-local static: initialised once even when
    // two in-process ranks call the relay from two threads)
    static const size_t stat_lds = [] {
        hipFuncAttributes at{};
        // (both chance forms' static LDS: the larger)
        const void* ks[] = {reinterpret_cast<const void*>(&relay_stamp_v6<true, false>),
                            reinterpret_cast<const void*>(&relay_stamp_v6<true, true>),
                            reinterpret_cast<const void*>(&relay_stamp_v6<true, false, false>),
                            reinterpret_cast<const void*>(&relay_stamp_v6<true, true, false>)};
        size_t m = 0;
        for (const void* k : ks) {
            if (hipFuncGetAttributes(&at, k) != hipSuccess) return (size_t)0;
            m = std::max(m, (size_t)at.sharedSizeBytes);
        }
        return m;
    }();
    return stat_lds;
}

uint32_t relay_stamp_chunk() { return kS6Cap; }
uint32_t relay_stamp_fixed_lds() { return kS6FixedLds; }

}  // namespace shd

#ifdef SHD_STAMP_PROF
extern "C" int shd_debug_k0_prof(unsigned long long* out) {   // 4096 x 5 words
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(shd::g_k0_prof), sizeof(unsigned long long) * 4096 * 5) != hipSuccess;
}
extern "C" int shd_debug_stamp_prof(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(shd::g_stamp_prof), sizeof(unsigned long long) * 12) != hipSuccess) return 1;
    if (reset) {
        unsigned long long z[12] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(shd::g_stamp_prof), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
#endif
