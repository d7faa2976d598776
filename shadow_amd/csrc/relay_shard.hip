// Relay pipeline 8 (overview and the list of units: relay_priv.h): the rounds under a
// communicator -- the bins exchanged as they lie, and the packing path behind it.
#include <algorithm>
#include <vector>

#include "relay_bins.h"

namespace shd {

// ------------------------------------------------------------------------------------------
// Sharded rounds (hosts split by id over the ranks).  Each rank stamps its own
// source hosts (their RNG streams and event ids live there) into events grouped by destination
// over ALL hosts; the events bound for rank r's hosts are one contiguous slice.  Per round:
//   1. local pipeline (as one GPU) -> events grouped by destination, in EventQueue order;
//   2. pack them as 24-byte records (deliver, seq, src, packet) and write, per peer, the
//      peer's per-destination offsets; one all-gather of every rank's sizing row -- its status,
//      reductions, receive capacity and event count per peer -- so every rank sees the whole
//      count matrix: the round's reductions ride on it, and whether any rank must grow its
//      receive buffers is known to all (then a second, one-word agreement follows the growth);
//   3. one host sync: sizes, and every rank's status (a failed round on any rank fails the
//      round everywhere, no host state is committed);
//   4. one grouped point-to-point exchange (offsets + records to every peer);
//   5. device k-way merge of the per-sender runs into this rank's destinations' events: the
//      senders own disjoint source ranges, so the merge by (deliver, src, seq) is EventQueue
//      order again (event.rs:84-155).
// No rank returns between two collectives on a local failure: allocations that depend on the
// round are folded into the status of the next agreement, the rest is sized at setup.
// ------------------------------------------------------------------------------------------
struct Ev24 {
    uint64_t deliver, seq;
    uint32_t src, pkt;
};
static_assert(sizeof(Ev24) == 24, "24-byte event record");
// sizing row of a rank: [0] status [1] min deliver [2] min latency [3] sent [4] receive
// capacity (events) [5..7] spare, then [kXHead + r] = events for rank r
constexpr uint32_t kXHead = 8;

// rel (a sharded flush, RelayState::rel_ids): ids relative to the source host's first id of the
// round, which only the sender holds
__global__ __launch_bounds__(256) void pack_events24(uint64_t n, const uint64_t* __restrict__ t,
                                                     const uint64_t* __restrict__ q, const uint32_t* __restrict__ sv,
                                                     const uint32_t* __restrict__ p, const uint64_t* __restrict__ rel,
                                                     Ev24* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = Ev24{t[i], rel ? q[i] - rel[sv[i]] : q[i], sv[i], p[i]};
}

__device__ __forceinline__ void shard_of(uint32_t total, uint32_t world, uint32_t r, uint32_t* lo, uint32_t* hi) {
    const uint64_t per = ((uint64_t)total + world - 1) / world;
    const uint64_t a = min((uint64_t)r * per, (uint64_t)total);
    *lo = (uint32_t)a;
    *hi = (uint32_t)min(a + per, (uint64_t)total);
}

__global__ __launch_bounds__(64) void shard_words(uint32_t world, uint32_t H, const uint32_t* __restrict__ ev_off,
                                                  uint64_t st, uint64_t md, uint64_t ml, uint64_t ns, uint64_t cap,
                                                  uint64_t* __restrict__ w) {
    for (uint32_t r = threadIdx.x; r < world; r += 64) {
        uint32_t lo, hi;
        shard_of(H, world, r, &lo, &hi);
        w[kXHead + r] = ev_off ? (uint64_t)(ev_off[hi] - ev_off[lo]) : 0ull;
    }
    if (threadIdx.x < kXHead) {
        const uint64_t v[kXHead] = {st, md, ml, ns, cap, 0, 0, 0};
        w[threadIdx.x] = v[threadIdx.x];
    }
}

// peer r's block: its destinations' offsets relative to the slice start, at stage[lo_r + r ..]
__global__ __launch_bounds__(256) void shard_offsets(uint32_t world, uint32_t H, const uint32_t* __restrict__ ev_off,
                                                     uint32_t* __restrict__ stage) {
    const uint32_t r = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    uint32_t lo, hi;
    shard_of(H, world, r, &lo, &hi);
    if (i <= hi - lo) stage[lo + r + i] = ev_off[lo + i] - ev_off[lo];
}

// ------------------------------------------------------------------------------------------
// Multi-GPU receive side: k-way merge of per-sender runs.  The input is n_runs chunks laid end
// to end; chunk r holds its events grouped by destination (local offsets off[r][0..n_dst]) and
// each destination's run sorted in EventQueue order.  Senders own disjoint source-host ranges,
// so the merged order is again (deliver, src, seq): every event finds its output rank by a
// binary search in each sibling run (keys are unique) -- no atomics, deterministic.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool ev3_less(uint64_t ta, uint32_t sa, uint64_t qa, uint64_t tb,
                                         uint32_t sb, uint64_t qb) {
    if (ta != tb) return ta < tb;
    if (sa != sb) return sa < sb;
    return qa < qb;
}

__global__ __launch_bounds__(256) void merge_offsets(uint32_t n_runs, uint32_t n_dst,
                                                     const uint32_t* __restrict__ off,
                                                     uint32_t* __restrict__ out_off) {
    const uint32_t d = blockIdx.x * 256 + threadIdx.x;
    if (d > n_dst) return;
    uint32_t t = 0;
    for (uint32_t r = 0; r < n_runs; ++r) t += off[(size_t)r * (n_dst + 1) + d] - off[(size_t)r * (n_dst + 1)];
    out_off[d] = t;
}

// merge_dst24: a wave per destination takes the destination's events of every sender run (<= 128:
// C5 has ~100 per destination), sorts the unique keys (deliver - tmin) << 8 | index with the wave
// network (wave.h) and stores them in rank order, coalesced -- a thread per event searching every
// sibling run's segment (the kernel this one replaced) was a chain of dependent 24-byte loads per
// run.  A destination with more events, a deliver-time span of 2^24 ns or more, or two equal
// deliver times (their order needs (src, seq)) is merged by the per-event searches in the same wave.
__global__ __launch_bounds__(256) void merge_dst24(uint32_t n_runs, uint32_t n_dst, const uint32_t* __restrict__ base,
                                                   const uint32_t* __restrict__ off, const Ev24* __restrict__ in,
                                                   const uint32_t* __restrict__ out_off, uint64_t* __restrict__ out_t,
                                                   uint32_t* __restrict__ out_s, uint64_t* __restrict__ out_q,
                                                   uint32_t* __restrict__ out_p) {
    constexpr int NPL = 2;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t d = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (d >= n_dst) return;   // wave-uniform; no barrier in this kernel
    // lane q < n_runs: run q's segment of destination d
    uint32_t seg = 0, cnt = 0;
    if (lane < n_runs) {
        const uint32_t* o = off + (size_t)lane * (n_dst + 1);
        seg = base[lane] + o[d];
        cnt = o[d + 1] - o[d];
    }
    uint32_t incl = cnt;
    for (uint32_t k = 1; k < 64; k <<= 1) {
        const uint32_t y = __shfl_up(incl, k);
        if (lane >= k) incl += y;
    }
    const uint32_t pre = incl - cnt;
    // the destination's event count from the merged offsets (every run, also past lane 63)
    const uint32_t out0 = out_off[d], n = out_off[d + 1] - out0;
    bool done = false;
    if (n <= 64u * NPL && n_runs <= 64) {
        Ev24 x[NPL];
        uint64_t tmn = ~0ull, tmx = 0;
#pragma unroll
        for (int c = 0; c < NPL; ++c) {
            const uint32_t i = lane + 64u * c;
            // the run holding staged index i: the last q whose prefix is <= i (ballot over lanes)
            const uint64_t m = __ballot(lane < n_runs && cnt > 0);
            uint32_t at = 0;
            for (uint64_t mm = m; mm; mm &= mm - 1) {
                const int q = __builtin_ctzll(mm);
                const uint32_t pq = __shfl(pre, q), sq = __shfl(seg, q);
                if (i < n && pq <= i) at = sq + (i - pq);
            }
            x[c] = i < n ? in[at] : Ev24{~0ull, 0, 0, 0};
            if (i < n) {
                tmn = x[c].deliver < tmn ? x[c].deliver : tmn;
                tmx = x[c].deliver > tmx ? x[c].deliver : tmx;
            }
        }
        for (int k = 32; k > 0; k >>= 1) {
            const uint64_t a = __shfl_xor(tmn, k), b = __shfl_xor(tmx, k);
            tmn = a < tmn ? a : tmn;
            tmx = b > tmx ? b : tmx;
        }
        if (n > 0 && tmx - tmn < (1ull << 24)) {
            uint32_t k32[NPL];
#pragma unroll
            for (int c = 0; c < NPL; ++c) {
                const uint32_t i = lane + 64u * c;
                k32[c] = i < n ? ((uint32_t)(x[c].deliver - tmn) << 8) | i : ~0u;
            }
            wave_bitonic32<NPL>(k32, lane);
            bool tie = false;
#pragma unroll
            for (int c = 0; c < NPL; ++c) {
                const uint32_t down = (uint32_t)__shfl_down((int)k32[c], 1);
                const uint32_t first = c + 1 < NPL ? (uint32_t)__shfl((int)k32[c + 1 < NPL ? c + 1 : c], 0) : ~0u;
                const uint32_t nx = lane == 63 ? first : down;
                if (lane + 64u * c + 1 < n && (nx >> 8) == (k32[c] >> 8)) tie = true;
            }
            if (__ballot(tie) == 0) {
#pragma unroll
                for (int c = 0; c < NPL; ++c) {
                    const uint32_t r = lane + 64u * c, i = k32[c] & 0xFFu;
                    const int src_lane = (int)(i & 63u);
                    // element i sits in lane i % 64, register i / 64 (every lane shuffles both)
                    Ev24 y{0, 0, 0, 0};
#pragma unroll
                    for (int c2 = 0; c2 < NPL; ++c2) {
                        const uint64_t t = __shfl(x[c2].deliver, src_lane), q = __shfl(x[c2].seq, src_lane);
                        const uint32_t sv = (uint32_t)__shfl((int)x[c2].src, src_lane);
                        const uint32_t pv = (uint32_t)__shfl((int)x[c2].pkt, src_lane);
                        if ((i >> 6) == (uint32_t)c2) y = Ev24{t, q, sv, pv};
                    }
                    if (r < n) {
                        out_t[out0 + r] = y.deliver;
                        out_s[out0 + r] = y.src;
                        out_q[out0 + r] = y.seq;
                        out_p[out0 + r] = y.pkt;
                    }
                }
                done = true;
            }
        }
    }
    if (done) return;
    // per-event searches (rank = the events before it in every sibling run) over this destination's events
    for (uint32_t i = lane; i < n; i += 64) {
        uint32_t q0 = 0, at = 0, rank = 0;
        uint32_t acc = 0;   // i's run: the segment counts' running sum
        for (uint32_t q = 0; q < n_runs; ++q) {
            const uint32_t* o = off + (size_t)q * (n_dst + 1);
            const uint32_t c = o[d + 1] - o[d];
            if (i >= acc && i < acc + c) {
                q0 = q;
                at = base[q] + o[d] + (i - acc);
                rank = i - acc;
            }
            acc += c;
        }
        const Ev24 x = in[at];
        for (uint32_t r2 = 0; r2 < n_runs; ++r2) {
            if (r2 == q0) continue;
            const uint32_t* o2 = off + (size_t)r2 * (n_dst + 1);
            uint32_t a = base[r2] + o2[d], b = base[r2] + o2[d + 1];
            const uint32_t a0 = a;
            while (a < b) {
                const uint32_t m = (a + b) >> 1;
                const Ev24 y = in[m];
                if (ev3_less(y.deliver, y.src, y.seq, x.deliver, x.src, x.seq)) a = m + 1; else b = m;
            }
            rank += a - a0;
        }
        out_t[out0 + rank] = x.deliver;
        out_s[out0 + rank] = x.src;
        out_q[out0 + rank] = x.seq;
        out_p[out0 + rank] = x.pkt;
    }
}

// ------------------------------------------------------------------------------------------
// Sharded rounds without the merge (relay_round_sharded_v7, the default when every rank runs
// pipeline 7).  The stamp places every record into its destination bin as on one GPU, but the
// bins restart at every rank's first destination (XShard), so the records bound for rank r are
// one contiguous slice of the stamp's output and each of r's bins is a sub-slice of it.  The
// exchange moves those 16-byte records as they lie -- no packing, no per-peer offsets: every
// rank's per-bin counts ride in the one sizing all-gather -- and the receiver runs the bin sort
// over its own bins with each bin's records gathered from every sender's slice (bin_sort_v7<X>):
// that yields its destinations' events in EventQueue order directly, so no merge pass follows.
// One host sync sizes the exchange (statuses, reductions, counts, fallback flags of every
// rank); a second reads the number of events received.
// The sizing row of a rank (u64 words): [0] status [1] min deliver [2] min latency [3] sent
// [4] receive capacity (events) [5] fallback flags [6] packets [7] spare, then the u32 record
// count of every bin (all ranks' bins) from word kXsHead on.
constexpr uint32_t kXsHead = 8;
constexpr uint32_t kXsOverflow = 1, kXsWide = 2, kXsHost = 4;

static size_t xs_row_words(uint32_t n_bins) { return kXsHead + ((size_t)n_bins + 1) / 2; }

__global__ __launch_bounds__(256) void xs_row(const unsigned long long* __restrict__ red, const uint32_t* __restrict__ tot,
                                              uint32_t n_bins, uint32_t ran, int32_t st_local, uint64_t cap,
                                              uint64_t n_pkt, uint32_t host_flags, int32_t st_nohost,
                                              int32_t st_invalid, uint64_t* __restrict__ row) {
    const uint32_t t = threadIdx.x, b = blockIdx.x * 256 + t;
    uint32_t* rt = reinterpret_cast<uint32_t*>(row + kXsHead);
    if (b < n_bins) rt[b] = ran ? tot[b] : 0u;   // a bin per thread (one block: 13 dependent trips, 7 us)
    if (blockIdx.x == 0 && t == 0) {
        uint64_t st = (uint64_t)(int64_t)st_local, md = ~0ull, ml = ~0ull, ns = 0;
        uint32_t fl = host_flags;
        if (ran) {
            if (red[6]) {
                fl |= kXsOverflow;   // the stamp did not run: the fallback reruns the round
            } else {
                if (red[3] != ~0ull) st = (uint64_t)(int64_t)st_nohost;   // as relay_run: NO_HOST first
                else if (red[5]) st = (uint64_t)(int64_t)st_invalid;
                if (red[4]) fl |= kXsWide;
                md = red[0];
                ml = red[1];
                ns = red[2];
            }
        }
        row[0] = st;
        row[1] = md;
        row[2] = ml;
        row[3] = ns;
        row[4] = cap;
        row[5] = fl;
        row[6] = n_pkt;
        row[7] = 0;
    }
}

// bins per thread of xs_sizing's 1024: n_bins <= 2^18 / 32 hosts + 64 ranks (relay_round_sharded_v7)
constexpr uint32_t kXsPer = 9;
static_assert(kXsPer * 1024 >= (kV7MaxHosts >> kBinShift) + 64, "xs_sizing: bins per thread");

// The sizing summary every rank derives alike from the gathered rows, one workgroup: sender by
// sender, the exclusive scan of its bin counts -> sc[q * (n_bins + 1) + b] (a thread's counts in
// registers); then out[0] = the largest bin over all senders (the receiver's LDS stage bound),
// out[1 ..] the world headers, then the record counts M[q][r] (sender q -> rank r); xb[q] =
// sender q's slice in this rank's received records (own records are not received), xb[world +
// q] = the packets of the senders before q.  (A block per sender with the last one to finish
// writing the summary took 15 us at world size 1: its device-scope fences write the XCD's L2
// back after the stamp's stores.  One workgroup needs no fence beyond its own.)
__global__ __launch_bounds__(1024) void xs_sizing(const uint64_t* __restrict__ rows, size_t row_words, uint32_t n_bins,
                                                  uint32_t world, uint32_t me, uint32_t bpr, uint32_t* sc,
                                                  uint64_t* __restrict__ out, uint32_t* __restrict__ xb) {
    __shared__ uint32_t s_w[16];
    __shared__ uint32_t s_max;
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t per = (n_bins + 1023) / 1024, b0 = min(n_bins, tid * per), b1 = min(n_bins, b0 + per);
    if (tid == 0) s_max = 0;
    uint32_t tot[kXsPer];
#pragma unroll
    for (uint32_t j = 0; j < kXsPer; ++j) tot[j] = 0;
    for (uint32_t q = 0; q < world; ++q) {
        const uint32_t* t = reinterpret_cast<const uint32_t*>(rows + (size_t)q * row_words + kXsHead);
        uint32_t* o = sc + (size_t)q * (n_bins + 1);
        uint32_t v[kXsPer];   // (per <= kXsPer: every load of the thread in flight at once)
#pragma unroll
        for (uint32_t j = 0; j < kXsPer; ++j) v[j] = b0 + j < b1 ? t[b0 + j] : 0u;
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t j = 0; j < kXsPer; ++j) {
            sum += v[j];
            tot[j] += v[j];
        }
        uint32_t incl = sum;
        for (uint32_t k = 1; k < 64; k <<= 1) {
            const uint32_t y = __shfl_up(incl, k);
            if (lane >= k) incl += y;
        }
        if (lane == 63) s_w[w] = incl;
        __syncthreads();
        uint32_t run = incl - sum;
        for (uint32_t u = 0; u < w; ++u) run += s_w[u];
#pragma unroll
        for (uint32_t j = 0; j < kXsPer; ++j) {
            if (b0 + j < b1) o[b0 + j] = run;
            run += v[j];
        }
        if (tid == 1023) o[n_bins] = run;
        __syncthreads();   // (s_w is rewritten by the next sender)
    }
    uint32_t mx = 0;
#pragma unroll
    for (uint32_t j = 0; j < kXsPer; ++j) mx = max(mx, tot[j]);
    atomicMax(&s_max, mx);
    for (uint32_t i = tid; i < world * kXsHead; i += 1024) out[1 + i] = rows[(size_t)(i / kXsHead) * row_words + i % kXsHead];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // the scans' stores, before the reads below
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    uint64_t* M = out + 1 + (size_t)world * kXsHead;
    for (uint32_t i = tid; i < world * world; i += 1024) {
        const uint32_t p = i / world, r = i % world;
        const uint32_t* sp = sc + (size_t)p * (n_bins + 1);
        M[i] = sp[min(r * bpr + bpr, n_bins)] - sp[min(r * bpr, n_bins)];
    }
    if (tid == 0) {
        uint32_t rb = 0;
        uint64_t pb = 0;
        for (uint32_t p = 0; p < world; ++p) {
            const uint32_t* sp = sc + (size_t)p * (n_bins + 1);
            xb[p] = rb;
            if (p != me) rb += sp[min(me * bpr + bpr, n_bins)] - sp[min(me * bpr, n_bins)];
            xb[world + p] = (uint32_t)pb;
            pb += rows[(size_t)p * row_words + 6];
        }
        out[0] = s_max;
    }
}

// sharded rounds' buffers that depend only on the host count and the ranks (shd_relay_setup)
shd_status relay_shard_alloc(shd_ctx* ctx) {
    RelayState& R = ctx->relay;
    const uint32_t world = (uint32_t)ctx->comm->size, H = R.n_hosts;
    uint32_t own_lo = 0, own_hi = 0;
    shard_range(H, (int)world, ctx->comm->rank, &own_lo, &own_hi);
    const size_t n_own = own_hi - own_lo;
    const XShard xsh = xshard(H, world);
    const size_t rw = std::max<size_t>(xs_row_words(xsh.n_bins), kXHead + world);
    SHD_TRY(R.x_words.ensure((size_t)world * rw * 8 + (size_t)world * 8 + 64));
    SHD_TRY(R.xs_sc.ensure((size_t)world * (xsh.n_bins + 1) * 4));
    const size_t out_bytes = (1 + (size_t)world * kXsHead + (size_t)world * world) * 8 + 64;
    SHD_TRY(R.xs_out.ensure(out_bytes));
    SHD_TRY(R.xs_pin.ensure(out_bytes));
    SHD_TRY(R.xs_b.ensure((size_t)world * 8 + 64));
    SHD_TRY(R.x_off.ensure(((size_t)H + world) * 4));
    SHD_TRY(R.x_roff.ensure((size_t)world * (n_own + 1) * 4 + (size_t)(world + 1) * 4));
    SHD_TRY(R.m_off.ensure((n_own + 4) * 4));   // + the received statuses' word (bin_sort_v7<true>)
    SHD_TRY(R.xs_st.ensure(((size_t)world + 1) * 8));
    SHD_HIP(hipMemsetAsync(R.xs_st.p, 0, ((size_t)world + 1) * 8, ctx->stream));
    R.xs_st_dirty = false;
    SHD_TRY(R.ev_off.ensure(((size_t)H + 1) * 4));
    R.x_cap = 0;
    return SHD_OK;
}

// receive side of a sharded round for n events (records, merged arrays), with headroom
static shd_status relay_recv_grow(RelayState& R, uint64_t n) {
    const uint64_t m = std::max<uint64_t>(n + n / 2, 1024);
    SHD_TRY(R.x_rrec.ensure(m * 24));
    SHD_TRY(R.m_deliver.ensure(m * 8));
    SHD_TRY(R.m_src.ensure(m * 4));
    SHD_TRY(R.m_seq.ensure(m * 8));
    SHD_TRY(R.m_pkt.ensure(m * 4));
    R.x_cap = m;
    return SHD_OK;
}

// local: the caller's own status on entry (a failure skips the local pipeline and is this rank's
// status in the sizing row, so the round commits on no rank)
static shd_status relay_round_sharded_x24(shd_ctx* ctx, const shd_batch* b, const shd_round* rd,
                                          shd_relay_out* d_out, shd_status local = SHD_OK) {
    RelayState& R = ctx->relay;
    Comm& C = *ctx->comm;
    hipStream_t s = ctx->stream;
    const uint32_t H = R.n_hosts, world = (uint32_t)C.size, WR = kXHead + world;
    const uint64_t n = b->n_packets;
    const size_t nn = std::max<uint64_t>(n, 1);
    // 1. the local pipeline into internal buffers (the caller's status array); a failure here is
    //    this rank's status in the sizing row, not a return
    shd_status st = local;
    shd_relay_out lo{};
    if (st == SHD_OK &&
        (R.ev_deliver.ensure(nn * 8) != SHD_OK || R.ev_src.ensure(nn * 4) != SHD_OK ||
         R.ev_seq.ensure(nn * 8) != SHD_OK || R.ev_pkt.ensure(nn * 4) != SHD_OK || R.x_rec.ensure(nn * 24) != SHD_OK))
        st = SHD_ERR_NOMEM;
    if (st == SHD_OK) {
        lo.status = d_out->status;
        lo.ev_off = R.ev_off.as<uint32_t>();
        lo.ev_deliver = R.ev_deliver.as<uint64_t>();
        lo.ev_src = R.ev_src.as<uint32_t>();
        lo.ev_seq = R.ev_seq.as<uint64_t>();
        lo.ev_pkt = R.ev_pkt.as<uint32_t>();
        st = relay_run(ctx, b, rd, &lo);
    }
    // 2. records, per-peer offset blocks, this rank's sizing row (buffers sized at setup)
    uint64_t* rows = R.x_words.as<uint64_t>();            // [world][WR] after the all-gather
    uint64_t* agree = rows + (size_t)world * WR;           // [world] growth agreement
    const uint64_t ns_local = st == SHD_OK ? R.red_host[2] : 0;
    if (st == SHD_OK && ns_local)
        pack_events24<<<div_up(ns_local, 256), 256, 0, s>>>(ns_local, lo.ev_deliver, lo.ev_seq, lo.ev_src,
                                                            lo.ev_pkt, R.rel_ids ? R.next_id.as<uint64_t>() : nullptr,
                                                            R.x_rec.as<Ev24>());
    shard_words<<<1, 64, 0, s>>>(world, H, st == SHD_OK ? lo.ev_off : nullptr, (uint64_t)st,
                                 st == SHD_OK ? R.red_host[0] : ~0ull, st == SHD_OK ? R.red_host[1] : ~0ull,
                                 ns_local, R.x_cap, rows + (size_t)C.rank * WR);
    if (st == SHD_OK)
        shard_offsets<<<dim3(div_up((uint64_t)(H + world - 1) / world + 1, 256), world), 256, 0, s>>>(
            world, H, lo.ev_off, R.x_off.as<uint32_t>());
    if (hipGetLastError() != hipSuccess && st == SHD_OK) st = SHD_ERR_HIP;
    SHD_TRY(C.all_gather(rows + (size_t)C.rank * WR, rows, (size_t)WR * 8, s));   // agreed (LocalComm) / fatal (RCCL)
    // 3. one host sync: the count matrix, every rank's outcome and capacity
    std::vector<uint64_t> w((size_t)world * WR);
    SHD_HIP(hipMemcpyAsync(w.data(), rows, w.size() * 8, hipMemcpyDeviceToHost, s));
    SHD_HIP(hipStreamSynchronize(s));
    auto row = [&](uint32_t q) { return w.data() + (size_t)q * WR; };
    uint64_t md = ~0ull, ml = ~0ull, ns = 0;
    for (uint32_t q = 0; q < world; ++q)
        if ((shd_status)row(q)[0] != SHD_OK) return (shd_status)row(q)[0];   // the lowest failing rank's
    for (uint32_t q = 0; q < world; ++q) {
        md = std::min<uint64_t>(md, row(q)[1]);
        ml = std::min<uint64_t>(ml, row(q)[2]);
        ns += row(q)[3];
    }
    // receive totals of every rank: whether any rank must grow is known to all of them
    bool grow = false;
    for (uint32_t r = 0; r < world; ++r) {
        uint64_t t = 0;
        for (uint32_t q = 0; q < world; ++q) t += row(q)[kXHead + r];
        grow = grow || t > row(r)[4];
    }
    uint32_t own_lo = 0, own_hi = 0;
    shard_range(H, (int)world, C.rank, &own_lo, &own_hi);
    const uint32_t n_own = own_hi - own_lo;
    std::vector<uint32_t> rbase(world + 1, 0);
    for (uint32_t q = 0; q < world; ++q) rbase[q + 1] = rbase[q] + (uint32_t)row(q)[kXHead + C.rank];
    const uint64_t n_recv = rbase[world];
    if (grow) {   // every rank takes this branch: one more agreement, on the growth's outcome
        shd_status gs = n_recv > R.x_cap ? relay_recv_grow(R, n_recv) : SHD_OK;
        ctx->h_pin[44] = (uint64_t)gs;
        if (hipMemcpyAsync(agree + C.rank, ctx->h_pin + 44, 8, hipMemcpyHostToDevice, s) != hipSuccess && gs == SHD_OK)
            gs = SHD_ERR_HIP;   // (the row still goes out: the peers wait for it)
        SHD_TRY(C.all_gather(agree + C.rank, agree, 8, s));
        std::vector<uint64_t> a(world);
        SHD_HIP(hipMemcpyAsync(a.data(), agree, world * 8, hipMemcpyDeviceToHost, s));
        SHD_HIP(hipStreamSynchronize(s));
        for (uint32_t q = 0; q < world; ++q)
            if ((shd_status)a[q] != SHD_OK) return (shd_status)a[q];
        if (gs != SHD_OK) return gs;
    }
    // 4. the exchange: part 0 = offsets block, part 1 = records
    std::vector<const void*> sp(2 * world);
    std::vector<void*> rp(2 * world);
    std::vector<size_t> sb(2 * world), rb(2 * world);
    uint64_t sent_before = 0;
    const uint64_t* mine = row((uint32_t)C.rank);
    for (uint32_t r = 0; r < world; ++r) {
        uint32_t a = 0, z = 0;
        shard_range(H, (int)world, (int)r, &a, &z);
        sp[2 * r] = R.x_off.as<uint32_t>() + a + r;
        sb[2 * r] = (size_t)(z - a + 1) * 4;
        sp[2 * r + 1] = R.x_rec.as<Ev24>() + sent_before;
        sb[2 * r + 1] = (size_t)mine[kXHead + r] * 24;
        sent_before += mine[kXHead + r];
        rp[2 * r] = R.x_roff.as<uint32_t>() + (size_t)r * (n_own + 1);
        rb[2 * r] = (size_t)(n_own + 1) * 4;
        rp[2 * r + 1] = R.x_rrec.as<Ev24>() + rbase[r];
        rb[2 * r + 1] = (size_t)row(r)[kXHead + C.rank] * 24;
    }
    SHD_TRY(C.exchange(2, sp.data(), sb.data(), rp.data(), rb.data(), s));   // agreed (LocalComm) / fatal (RCCL)
    // 5. merge the per-sender runs (no collective follows: a HIP failure from here on is local)
    uint32_t* d_base = R.x_roff.as<uint32_t>() + (size_t)world * (n_own + 1);
    SHD_HIP(hipMemcpyAsync(d_base, rbase.data(), (world + 1) * 4, hipMemcpyHostToDevice, s));
    merge_offsets<<<div_up((uint64_t)n_own + 1, 256), 256, 0, s>>>(world, n_own, R.x_roff.as<uint32_t>(),
                                                                  R.m_off.as<uint32_t>());
    if (n_recv)
        merge_dst24<<<div_up(n_own, 4), 256, 0, s>>>(world, n_own, d_base, R.x_roff.as<uint32_t>(),
                                                     R.x_rrec.as<Ev24>(), R.m_off.as<uint32_t>(),
                                                     R.m_deliver.as<uint64_t>(), R.m_src.as<uint32_t>(),
                                                     R.m_seq.as<uint64_t>(), R.m_pkt.as<uint32_t>());
    SHD_HIP(hipGetLastError());
    SHD_TRY(relay_commit(ctx, &lo));
    SHD_HIP(hipStreamSynchronize(s));   // rbase (host memory) was read by the copy above
    d_out->ev_off = R.m_off.as<uint32_t>();
    d_out->ev_deliver = R.m_deliver.as<uint64_t>();
    d_out->ev_src = R.m_src.as<uint32_t>();
    d_out->ev_seq = R.m_seq.as<uint64_t>();
    d_out->ev_pkt = R.m_pkt.as<uint32_t>();
    d_out->min_deliver = md;
    d_out->min_latency = ml;
    d_out->n_sent = ns;
    d_out->n_dst = n_own;
    d_out->n_events = (uint32_t)n_recv;
    round_note(ctx, md, ml);
    R.last_recv = n_recv;
    return SHD_OK;
}

// One sharded round without the merge (see xs_row above).  *fallback = true (the same on every
// rank: the decision reads only the gathered rows) when any rank cannot take this path -- not
// pipeline 7, a bin over its LDS stage, a deliver offset or event ids
// past 32 bits, more than 2^24 packets over all ranks -- and the caller then runs the packing
// path (relay_round_sharded_x24), which reruns the round from the uncommitted state.
static shd_status relay_round_sharded_v7(shd_ctx* ctx, const shd_batch* b, const shd_round* rd,
                                         shd_relay_out* d_out, bool* fallback, shd_status local = SHD_OK) {
    RelayState& R = ctx->relay;
    Comm& C = *ctx->comm;
    hipStream_t s = ctx->stream;
    const uint32_t H = R.n_hosts, world = (uint32_t)C.size, me = (uint32_t)C.rank;
    const uint64_t n = b->n_packets;
    const XShard xsh = xshard(H, world);
    const uint32_t n_bins = xsh.n_bins;
    const size_t rw = xs_row_words(n_bins);
    *fallback = false;
    // 1. the local pipeline up to the stamp (records left in their bins); a failure is this
    //    rank's status in its sizing row, not a return
    const bool ok7 = world <= 64 && R.n_src > 0 && R.table_narrow && !R.force_v1 && relay_v7_ok(ctx, n, n_bins);
    // absolute ids must fit the records' 32 bits; relative ids (a sharded flush) always do
    const bool abs_seq = R.rel_ids || R.seq_bound + n < (1ull << 32);
    shd_status st = local;   // (the caller's own failure: as one of the local pipeline)
    shd_relay_out lo{};
    lo.status = d_out->status;
    bool ran = false;
    if (st == SHD_OK && ok7 && abs_seq) {
        const uint64_t nn = (uint64_t)R.n_nodes * R.n_nodes;   // the round's counter increments start at 0
        if (R.red.ensure(64) != SHD_OK || (R.count_on && R.counts_round.ensure(nn * 8) != SHD_OK))
            st = SHD_ERR_NOMEM;
        else if (R.count_on && hipMemsetAsync(R.counts_round.p, 0, nn * 8, s) != hipSuccess)
            st = SHD_ERR_HIP;
        if (st == SHD_OK) st = relay_device_v7(ctx, b, rd, &lo, &xsh);
        ran = st == SHD_OK;
    }
    uint64_t* rows = R.x_words.as<uint64_t>();
    uint64_t* agree = rows + (size_t)world * rw;
    xs_row<<<std::max<uint32_t>(1, div_up(n_bins, 256)), 256, 0, s>>>(ran ? R.red.as<unsigned long long>() : nullptr,
                             ran ? R.bin_base.as<uint32_t>() + n_bins + 1 : nullptr, n_bins, ran ? 1u : 0u,
                             (int32_t)st, R.x_cap, n, (ok7 && abs_seq) ? 0u : kXsHost, (int32_t)SHD_ERR_NO_HOST,
                             (int32_t)SHD_ERR_INVALID, rows + (size_t)me * rw);
    if (hipGetLastError() != hipSuccess) {
        // the row the peers size the exchange from must carry the failure: written from the host
        if (st == SHD_OK) st = SHD_ERR_HIP;
        std::vector<uint64_t> hrow(rw, 0);
        hrow[0] = (uint64_t)(int64_t)st;
        hrow[1] = hrow[2] = ~0ull;
        (void)hipMemcpy(rows + (size_t)me * rw, hrow.data(), rw * 8, hipMemcpyHostToDevice);
    }
    SHD_TRY(C.all_gather(rows + (size_t)me * rw, rows, rw * 8, s));   // agreed (LocalComm) / fatal (RCCL)
    // 2. the sizing summary, one host sync.  From here on a local failure is carried into the
    //    exchange (its status part) instead of returned: the peers are on their way to it.  A
    //    failure of the summary's own read-back leaves this rank without the sizes, which is fatal
    //    to the communicator, as an RCCL failure is.
    shd_status st_post = SHD_OK;
    uint32_t* xb = R.xs_b.as<uint32_t>();
    xs_sizing<<<1, 1024, 0, s>>>(rows, rw, n_bins, world, me, xsh.bpr, R.xs_sc.as<uint32_t>(),
                                 R.xs_out.as<uint64_t>(), xb);
    const size_t out_words = 1 + (size_t)world * kXsHead + (size_t)world * world;
    SHD_TRY(readback_into(ctx, s, R.xs_out.p, out_words * 8, R.xs_pin.as<unsigned long long>()));
    if (hipGetLastError() != hipSuccess) st_post = SHD_ERR_HIP;
    if (ctx->knobs.get(K_TEST_FAIL, 0) == 1) st_post = SHD_ERR_HIP;   // (fault injection, tests)
    const uint64_t* pin = R.xs_pin.as<uint64_t>();
    auto hdr = [&](uint32_t q) { return pin + 1 + (size_t)q * kXsHead; };
    auto M = [&](uint32_t q, uint32_t r) { return pin[1 + (size_t)world * kXsHead + (size_t)q * world + r]; };
    for (uint32_t q = 0; q < world; ++q)
        if ((shd_status)hdr(q)[0] != SHD_OK) return (shd_status)hdr(q)[0];   // the lowest failing rank's
    uint64_t pk = 0;
    bool fb = pin[0] > kB7Cap;
    for (uint32_t q = 0; q < world; ++q) {
        fb = fb || hdr(q)[5] != 0;
        pk += hdr(q)[6];
    }
    if (fb || pk >= kV7MaxPackets) {
        *fallback = true;
        return SHD_OK;
    }
    uint64_t md = ~0ull, ml = ~0ull, ns = 0;
    for (uint32_t q = 0; q < world; ++q) {
        md = std::min<uint64_t>(md, hdr(q)[1]);
        ml = std::min<uint64_t>(ml, hdr(q)[2]);
        ns += hdr(q)[3];
    }
    // receive capacity (records, and the events they hold): whether any rank grows is known to all
    bool grow = false;
    uint64_t n_recv = 0;
    for (uint32_t r = 0; r < world; ++r) {
        uint64_t t = 0;
        for (uint32_t q = 0; q < world; ++q) t += M(q, r);
        grow = grow || t > hdr(r)[4];
        if (r == me) n_recv = t;
    }
    if (grow) {   // every rank takes this branch: one more agreement, on the growth's outcome
        shd_status gs = n_recv > R.x_cap ? relay_recv_grow(R, n_recv) : SHD_OK;
        ctx->h_pin[44] = (uint64_t)gs;
        if (hipMemcpyAsync(agree + me, ctx->h_pin + 44, 8, hipMemcpyHostToDevice, s) != hipSuccess && gs == SHD_OK)
            gs = SHD_ERR_HIP;   // (the row still goes out: the peers wait for it)
        SHD_TRY(C.all_gather(agree + me, agree, 8, s));
        std::vector<uint64_t> a(world);
        SHD_HIP(hipMemcpyAsync(a.data(), agree, world * 8, hipMemcpyDeviceToHost, s));
        SHD_HIP(hipStreamSynchronize(s));   // (a failed read-back of the agreement: fatal, as above)
        for (uint32_t q = 0; q < world; ++q)
            if ((shd_status)a[q] != SHD_OK) return (shd_status)a[q];
    }
    // 3. the exchange: part 0 is the sender's status after the gather (every rank learns every
    //    peer's, under RCCL too), part 1 the records of rank r's bins as the stamp laid them out
    //    (own: none)
    uint64_t* xst = R.xs_st.as<uint64_t>();
    if (st_post != SHD_OK || R.xs_st_dirty) {
        if (hipMemsetD32Async(xst, (uint32_t)st_post, 1, s) != hipSuccess && st_post == SHD_OK) st_post = SHD_ERR_HIP;
        R.xs_st_dirty = st_post != SHD_OK;
    }
    std::vector<const void*> sp(2 * (size_t)world);
    std::vector<void*> rp(2 * (size_t)world);
    std::vector<size_t> sb(2 * (size_t)world), rb(2 * (size_t)world);
    uint64_t sent_before = 0, recv_before = 0;
    for (uint32_t r = 0; r < world; ++r) {
        sp[2 * r] = xst;
        sb[2 * r] = r == me ? 0 : 8;
        rp[2 * r] = xst + 1 + r;
        rb[2 * r] = r == me ? 0 : 8;
        sp[2 * r + 1] = R.rec.as<uint4>() + sent_before;
        sb[2 * r + 1] = r == me ? 0 : (size_t)M(me, r) * 16;
        sent_before += M(me, r);
        rp[2 * r + 1] = R.x_rrec.as<uint4>() + recv_before;
        rb[2 * r + 1] = r == me ? 0 : (size_t)M(r, me) * 16;
        if (r != me) recv_before += M(r, me);
    }
    SHD_TRY(C.exchange(2, sp.data(), sb.data(), rp.data(), rb.data(), s, st_post));   // agreed (LocalComm, HostComm)
    // 4. the bin sort of this rank's bins over every sender's records; it also combines the
    //    statuses of part 0, which come back with the event count (no collective follows)
    uint32_t own_lo = 0, own_hi = 0;
    shard_range(H, (int)world, (int)me, &own_lo, &own_hi);
    const uint32_t n_own = own_hi - own_lo;
    const uint32_t fb_me = xsh.first_bin(me), nb = xsh.first_bin(me + 1) - fb_me;
    uint32_t kq = 0;
    while ((kq ? 2 * kq : 1u) < world) kq = kq ? 2 * kq : 1u;
    XSrc xs{world, me, fb_me, n_bins + 1, kq, R.xs_sc.as<uint32_t>(), xb, xb + world, R.rec.as<uint4>(),
            xst + 1, (uint32_t)st_post};
    relay_launch_bin_sort_x(ctx, n_own, nb, rd->round_end, xs);
    SHD_HIP(hipGetLastError());
    // 5. the number of events this rank received (= its destinations' SENT events: the bins also
    //    hold the dropped packets' records, so the record matrix does not give it) and the agreed
    //    status: 16 aligned bytes holding m_off[n_own] and m_off[n_own + 1]
    SHD_TRY(readback_into(ctx, s, R.m_off.as<uint32_t>() + (n_own & ~1u), 16, R.xs_pin.as<unsigned long long>()));
    const uint32_t n_ev = R.xs_pin.as<uint32_t>()[n_own & 1u];
    const shd_status agreed = (shd_status)R.xs_pin.as<uint32_t>()[(n_own & 1u) + 1];
    if (agreed != SHD_OK) return agreed;   // every rank: nothing of the hosts' state is committed
    R.red_host[0] = hdr(me)[1];
    R.red_host[1] = hdr(me)[2];
    R.red_host[2] = hdr(me)[3];
    R.last_pipe = 8;   // pipeline 7's stamp, its bins exchanged and sorted by their destination ranks
    R.last_v2 = true;
    SHD_TRY(relay_commit(ctx, &lo));
    d_out->ev_off = R.m_off.as<uint32_t>();
    d_out->ev_deliver = R.m_deliver.as<uint64_t>();
    d_out->ev_src = R.m_src.as<uint32_t>();
    d_out->ev_seq = R.m_seq.as<uint64_t>();
    d_out->ev_pkt = R.m_pkt.as<uint32_t>();
    d_out->min_deliver = md;
    d_out->min_latency = ml;
    d_out->n_sent = ns;
    d_out->n_dst = n_own;
    d_out->n_events = n_ev;
    round_note(ctx, md, ml);
    R.last_recv = n_ev;
    return SHD_OK;
}

static shd_status relay_round_sharded(shd_ctx* ctx, const shd_batch* b, const shd_round* rd, shd_relay_out* d_out,
                                      shd_status local = SHD_OK) {
    // (more hosts than the records' source bits: every rank has the same host count, so every
    // rank takes the packing path without asking; xs_sizing's registers also assume it)
    if (ctx->knobs.on(K_RELAY_SHARD_X24) || ctx->relay.n_hosts > kV7MaxHosts)
        return relay_round_sharded_x24(ctx, b, rd, d_out, local);
    bool fallback = false;
    SHD_TRY(relay_round_sharded_v7(ctx, b, rd, d_out, &fallback, local));
    return fallback ? relay_round_sharded_x24(ctx, b, rd, d_out, local) : SHD_OK;
}

shd_status relay_round_sharded_local(shd_ctx* ctx, const shd_batch* b, const shd_round* rd, shd_relay_out* o,
                                     shd_status local) {
    return relay_round_sharded(ctx, b, rd, o, local);
}

// shd_relay_flush under a communicator (flush.hip): this rank's grouped sends, the CPU's draws
shd_status relay_flush_round_sharded(shd_ctx* ctx, const shd_batch* b, const shd_round* rd, shd_relay_out* o) {
    return relay_round_sharded(ctx, b, rd, o);
}

}  // namespace shd
