// Relay pipeline 3 (overview: relay_priv.h), the radix back end: the stamp's records sorted by destination
// (radix_sort_pairs below), then every destination's run sorted by one wave.  The fallback of pipeline 7.
//
// radix_sort_pairs: stable LSD radix sort of (u32 key, 16-byte record) pairs, 6 bits per pass --
// a per-tile digit histogram, one scan of the digit-major counts (scan.h), and a stable scatter
// (each thread ranks its 16 consecutive keys, a block scan orders the tile digit-major).
#include <algorithm>

#include "relay_priv.h"
#include "scan.h"

namespace shd {

constexpr uint32_t kRsT = 256, kRsK = 16, kRsTile = kRsT * kRsK;   // 4096 pairs per tile
constexpr uint32_t kRsBits = 6, kRsDig = 1u << kRsBits;

// counts[d * n_tiles + tile] = keys of the tile with digit d
__global__ __launch_bounds__(kRsT) void rs_hist(const uint32_t* __restrict__ keys, uint64_t n, uint32_t shift,
                                                uint32_t n_tiles, uint32_t* __restrict__ counts) {
    __shared__ uint32_t h[kRsDig];
    const uint32_t tid = threadIdx.x, tile = blockIdx.x;
    if (tid < kRsDig) h[tid] = 0;
    __syncthreads();
    const uint64_t b = (uint64_t)tile * kRsTile;
#pragma unroll 4
    for (uint32_t j = 0; j < kRsK; ++j) {
        const uint64_t i = b + (uint64_t)j * kRsT + tid;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & (kRsDig - 1)], 1u);
    }
    __syncthreads();
    if (tid < kRsDig) counts[(size_t)tid * n_tiles + tile] = h[tid];
}

// stable scatter: thread t owns the tile's keys [t*K, t*K+K); its keys' ranks come from a
// digit-major block scan of the per-thread digit counts (LDS, u16)
__global__ __launch_bounds__(kRsT) void rs_scatter(const uint32_t* __restrict__ kin, const uint4* __restrict__ vin,
                                                   uint32_t* __restrict__ kout, uint4* __restrict__ vout, uint64_t n,
                                                   uint32_t shift, uint32_t n_tiles,
                                                   const uint32_t* __restrict__ offs) {
    constexpr uint32_t S = kRsT + 1;   // padded row (bank spread)
    __shared__ uint16_t cnt[kRsDig * S];
    __shared__ uint32_t s_part[kRsT];
    __shared__ uint32_t s_dstart[kRsDig];
    const uint32_t tid = threadIdx.x, tile = blockIdx.x;
    const uint64_t b = (uint64_t)tile * kRsTile + (uint64_t)tid * kRsK;
    uint32_t key[kRsK], rank[kRsK];
    for (uint32_t d = 0; d < kRsDig; ++d) cnt[d * S + tid] = 0;
#pragma unroll
    for (uint32_t j = 0; j < kRsK; ++j) key[j] = b + j < n ? kin[b + j] : 0xFFFFFFFFu;
#pragma unroll
    for (uint32_t j = 0; j < kRsK; ++j) {
        if (b + j < n) {
            const uint32_t d = (key[j] >> shift) & (kRsDig - 1);
            rank[j] = cnt[d * S + tid]++;
        }
    }
    __syncthreads();
    // digit-major exclusive scan over (d, t): thread x takes row d = x / 4, columns (x % 4) * 64 ..
    const uint32_t d0 = tid >> 2, c0 = (tid & 3) * 64;
    uint32_t sum = 0;
    for (uint32_t c = 0; c < 64; ++c) sum += cnt[d0 * S + c0 + c];
    s_part[tid] = sum;
    __syncthreads();
    if (tid < 64) {   // one wave scans the 256 partial sums (4 per lane)
        uint32_t p[4], t = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            p[i] = s_part[tid * 4 + i];
            t += p[i];
        }
        uint32_t incl = t;
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (tid >= o) incl += y;
        }
        uint32_t run = incl - t;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            s_part[tid * 4 + i] = run;
            run += p[i];
        }
    }
    __syncthreads();
    {
        uint32_t run = s_part[tid];
        if ((tid & 3) == 0) s_dstart[d0] = run;   // the digit's first position in the tile
        for (uint32_t c = 0; c < 64; ++c) {
            const uint32_t v = cnt[d0 * S + c0 + c];
            cnt[d0 * S + c0 + c] = (uint16_t)run;
            run += v;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kRsK; ++j) {
        if (b + j < n) {
            const uint32_t d = (key[j] >> shift) & (kRsDig - 1);
            const uint32_t pos = cnt[d * S + tid] + rank[j];   // position in the digit-major tile
            const uint64_t gp = (uint64_t)offs[(size_t)d * n_tiles + tile] + (pos - s_dstart[d]);
            kout[gp] = key[j];
            vout[gp] = vin[b + j];
        }
    }
}

// Stable sort of n (key, record) pairs by the low `bits` bits of the key, ping-ponging between
// (k0, v0) and (k1, v1); *in_first says where the result is (true: k0 / v0).
static shd_status radix_sort_pairs(DevBuf& counts, ScanScratch& scan, uint32_t* k0, uint4* v0, uint32_t* k1, uint4* v1, uint64_t n,
                                   uint32_t bits, bool* in_first, hipStream_t s) {
    *in_first = true;
    if (n == 0) return SHD_OK;
    const uint32_t n_tiles = (uint32_t)((n + kRsTile - 1) / kRsTile);
    const uint64_t nc = (uint64_t)n_tiles * kRsDig;
    SHD_TRY(counts.ensure(nc * 4 + 16));
    uint32_t* kin = k0;
    uint4* vin = v0;
    uint32_t* kout = k1;
    uint4* vout = v1;
    for (uint32_t shift = 0; shift < bits; shift += kRsBits) {
        rs_hist<<<n_tiles, kRsT, 0, s>>>(kin, n, shift, n_tiles, counts.as<uint32_t>());
        SHD_HIP(hipGetLastError());
        SHD_TRY(scan_excl2(scan, counts.as<uint32_t>(), counts.as<uint32_t>(), nullptr, nullptr, nc, s));
        rs_scatter<<<n_tiles, kRsT, 0, s>>>(kin, vin, kout, vout, n, shift, n_tiles, counts.as<uint32_t>());
        SHD_HIP(hipGetLastError());
        std::swap(kin, kout);
        std::swap(vin, vout);
        *in_first = !*in_first;
    }
    return SHD_OK;
}

// ev_off[d] = first position of destination d in the sorted keys (lower bound), d in [0, H]
__global__ __launch_bounds__(256) void bucket_offsets(const uint32_t* __restrict__ key, uint64_t n,
                                                      uint32_t n_hosts, uint32_t* __restrict__ ev_off) {
    const uint32_t d = blockIdx.x * 256 + threadIdx.x;
    if (d > n_hosts) return;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t m = (lo + hi) >> 1;
        if (key[m] < d) lo = m + 1; else hi = m;
    }
    ev_off[d] = (uint32_t)lo;
}

__device__ __forceinline__ bool rec_less(const uint4& a, const uint4& b) {
    if (a.x != b.x) return a.x < b.x;     // deliver offset
    if (a.y != b.y) return a.y < b.y;     // src host
    return a.z < b.z;                     // event id offset
}

constexpr uint32_t kWaveSeg = 256;

// Sort one destination run held in LDS (xs[0..n), n <= kWaveSeg) by one wave; writes the sorted
// order as LDS positions pm[e] = base + position.  32-bit keys ((offset - min) << PB | position)
// when the run's deliver offsets leave room for PB position bits, else 64-bit keys.
template <int NPL, int PB>
__device__ __forceinline__ void wave_sort_perm(uint32_t n, uint32_t lane, const uint4* xs,
                                               uint32_t lo, uint32_t span, uint16_t* pm,
                                               uint32_t base) {
    if (span < (1u << (32 - PB)) - 1u) {
        uint32_t k[NPL];
#pragma unroll
        for (int c = 0; c < NPL; ++c) {
            const uint32_t e = lane + 64u * c;
            k[c] = e < n ? ((xs[e].x - lo) << PB) | e : ~0u;
        }
        wave_bitonic32<NPL>(k, lane);
#pragma unroll
        for (int c = 0; c < NPL; ++c) {
            const uint32_t e = lane + 64u * c;
            if (e < n) pm[e] = (uint16_t)(base + (k[c] & ((1u << PB) - 1u)));
        }
    } else {
        uint64_t k[NPL];
#pragma unroll
        for (int c = 0; c < NPL; ++c) {
            const uint32_t e = lane + 64u * c;
            k[c] = e < n ? (((uint64_t)xs[e].x << 32) | e) : ~0ull;
        }
        wave_bitonic<NPL>(k, lane);
#pragma unroll
        for (int c = 0; c < NPL; ++c) {
            const uint32_t e = lane + 64u * c;
            if (e < n) pm[e] = (uint16_t)(base + (uint32_t)k[c]);
        }
    }
}

__device__ __forceinline__ void wave_sort_run(uint32_t n, uint32_t lane, const uint4* xs,
                                              uint16_t* pm, uint32_t base) {
    uint32_t lo = ~0u, hi = 0;
    for (uint32_t e = lane; e < n; e += 64) {
        lo = min(lo, xs[e].x);
        hi = max(hi, xs[e].x);
    }
    lo = wave_min_u32(lo, lane);
    const uint32_t span = wave_max_u32(hi, lane) - lo;
    if (n <= 64) wave_sort_perm<1, 6>(n, lane, xs, lo, span, pm, base);
    else if (n <= 128) wave_sort_perm<2, 7>(n, lane, xs, lo, span, pm, base);
    else wave_sort_perm<4, 8>(n, lane, xs, lo, span, pm, base);
}

// K4: a workgroup owns kSegDst consecutive destinations; their runs are one contiguous range of
// the sorted records, so it is loaded and stored in bulk (coalesced) while each wave sorts whole
// runs in LDS.  Runs longer than kWaveSeg go to the merge kernel; a range larger than the LDS
// stage (only with such runs) is handled run by run.
constexpr uint32_t kSegDst = 8;
constexpr uint32_t kRunCap = 1536;

__global__ __launch_bounds__(256) void segment_sort_v5(
    uint32_t n_hosts, const uint32_t* __restrict__ ev_off, const uint4* __restrict__ brec,
    uint64_t round_end, const uint64_t* __restrict__ seq_base, uint64_t* __restrict__ ev_deliver,
    uint32_t* __restrict__ ev_src, uint64_t* __restrict__ ev_seq, uint32_t* __restrict__ ev_pkt,
    uint32_t* __restrict__ big) {
    __shared__ uint4 x[kRunCap];
    __shared__ uint16_t pm[kRunCap];
    __shared__ uint32_t off[kSegDst + 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t d0 = blockIdx.x * kSegDst;
    const uint32_t nd = min(kSegDst, n_hosts - d0);
    if (tid <= nd) off[tid] = ev_off[d0 + tid];
    __syncthreads();
    const uint32_t B = off[0], N = off[nd] - B;
    if (N > kRunCap) {   // run by run through a per-wave stage
        uint4* xw = x + w * kWaveSeg;
        uint16_t* pw = pm + w * kWaveSeg;
        for (uint32_t dl = w; dl < nd; dl += 4) {
            const uint32_t b = off[dl], n = off[dl + 1] - b;
            if (n == 0) continue;
            if (n > kWaveSeg) {
                if (lane == 0) big[atomicAdd(&big[0], 1u) + 1] = d0 + dl;
                continue;
            }
            for (uint32_t e = lane; e < n; e += 64) xw[e] = brec[b + e];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            wave_sort_run(n, lane, xw, pw, 0);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (uint32_t e = lane; e < n; e += 64) {
                const uint4 r = xw[pw[e]];
                ev_deliver[b + e] = round_end + r.x;
                ev_src[b + e] = r.y;
                ev_seq[b + e] = seq_base ? seq_base[r.y] + r.z : r.z;
                ev_pkt[b + e] = r.w;
            }
            __builtin_amdgcn_wave_barrier();
        }
        return;
    }
    for (uint32_t i = tid; i < N; i += 256) x[i] = brec[B + i];
    __syncthreads();
    for (uint32_t dl = w; dl < nd; dl += 4) {
        const uint32_t b = off[dl] - B, n = off[dl + 1] - off[dl];
        if (n == 0) continue;
        if (n > kWaveSeg) {   // the merge kernel writes this run; the bulk store skips it
            if (lane == 0) big[atomicAdd(&big[0], 1u) + 1] = d0 + dl;
            for (uint32_t e = lane; e < n; e += 64) pm[b + e] = 0xFFFFu;
            continue;
        }
        wave_sort_run(n, lane, x + b, pm + b, b);
    }
    __syncthreads();
    for (uint32_t i = tid; i < N; i += 256) {
        const uint32_t p = pm[i];
        if (p == 0xFFFFu) continue;
        const uint4 r = x[p];
        ev_deliver[B + i] = round_end + r.x;
        ev_src[B + i] = r.y;
        ev_seq[B + i] = seq_base ? seq_base[r.y] + r.z : r.z;
        ev_pkt[B + i] = r.w;
    }
}

// Runs longer than kWaveSeg: bottom-up merge passes by one workgroup in a
// global scratch copy of the bucket (rank by binary search in the sibling run; keys unique).
__global__ __launch_bounds__(256) void segment_sort_v2_big(
    const uint32_t* __restrict__ big, const uint32_t* __restrict__ ev_off, uint4* __restrict__ brec,
    uint4* __restrict__ tmp, uint64_t round_end, const uint64_t* __restrict__ seq_base,
    uint64_t* __restrict__ ev_deliver, uint32_t* __restrict__ ev_src, uint64_t* __restrict__ ev_seq,
    uint32_t* __restrict__ ev_pkt) {
    for (uint32_t bi = blockIdx.x; bi < big[0]; bi += gridDim.x) {
        const uint32_t d = big[1 + bi];
        const uint32_t b = ev_off[d], n = ev_off[d + 1] - b;
        uint4* A = brec + b;
        uint4* T = tmp + b;
        for (uint32_t w = 1; w < n; w <<= 1) {
            for (uint32_t o = threadIdx.x; o < n; o += 256) {
                const uint32_t lo = (o / (2 * w)) * 2 * w;
                const uint32_t mid = min(lo + w, n), hi = min(lo + 2 * w, n);
                const uint4 xv = A[o];
                uint32_t rank;
                if (o < mid) {
                    uint32_t l = mid, h = hi;
                    while (l < h) {
                        const uint32_t m = (l + h) >> 1;
                        if (rec_less(A[m], xv)) l = m + 1; else h = m;
                    }
                    rank = (o - lo) + (l - mid);
                } else {
                    uint32_t l = lo, h = mid;
                    while (l < h) {
                        const uint32_t m = (l + h) >> 1;
                        if (rec_less(xv, A[m])) h = m; else l = m + 1;
                    }
                    rank = (o - mid) + (l - lo);
                }
                T[lo + rank] = xv;
            }
            __syncthreads();
            for (uint32_t o = threadIdx.x; o < n; o += 256) A[o] = T[o];
            __syncthreads();
        }
        for (uint32_t i = threadIdx.x; i < n; i += 256) {
            const uint4 e = A[i];
            ev_deliver[b + i] = round_end + e.x;
            ev_src[b + i] = e.y;
            ev_seq[b + i] = seq_base ? seq_base[e.y] + e.z : e.z;
            ev_pkt[b + i] = e.w;
        }
        __syncthreads();
    }
}

// Narrow pipeline: K1 stamp, K2 radix sort by destination, K3 offsets, K4 per-run sort; one
// host sync (for the round reductions).
// the round's reductions: [0] min deliver, [1] min latency, [2] sent, [3] first bad index,
// [4] wide offset, [5] send-order violation; plus the big-run counter of K4
__global__ __launch_bounds__(64) void red_init(unsigned long long* __restrict__ red, uint32_t* __restrict__ n_big) {
    const uint32_t t = threadIdx.x;
    if (t < 8) red[t] = (t <= 1 || t == 3) ? ~0ull : 0ull;
    if (t == 0) *n_big = 0;
}

shd_status relay_device_v3(shd_ctx* ctx, const shd_batch* b, const shd_round* rd, shd_relay_out* o) {
    RelayState& R = ctx->relay;
    hipStream_t s = ctx->stream;
    const uint64_t n = b->n_packets;
    const uint32_t H = R.n_hosts;
    const size_t nn = std::max<uint64_t>(n, 1);
    SHD_TRY(R.rec.ensure(nn * 16));
    SHD_TRY(R.brec.ensure(nn * 16));
    SHD_TRY(R.ev_val.ensure(nn * 4));    // keys
    SHD_TRY(R.ev_key.ensure(nn * 4));    // keys (second buffer)
    SHD_TRY(R.ev_val2.ensure((size_t)(H + 2) * 4));
    SHD_TRY(R.draws.ensure(nn * 4));
    red_init<<<1, 64, 0, s>>>(R.red.as<unsigned long long>(), R.ev_val2.as<uint32_t>());
    RelayArgs3 a = relay_args3(ctx, b, rd, o);
    const uint64_t* seq_base = a.abs_seq ? nullptr : R.next_id.as<uint64_t>();
    relay_launch_draws(ctx, a);   // K0: the per-host generator streams
    relay_launch_stamp(ctx, a);
    SHD_HIP(hipGetLastError());
    // stable LSD radix sort of the records by destination (keys <= H), hand-written
    uint32_t bits = 1;
    while (bits < 32 && (H >> bits) != 0) ++bits;
    bool first = true;
    SHD_TRY(radix_sort_pairs(R.rs_counts, R.rs_scan, R.ev_val.as<uint32_t>(), R.rec.as<uint4>(),
                             R.ev_key.as<uint32_t>(), R.brec.as<uint4>(), n, bits, &first, s));
    uint4* sorted = first ? R.rec.as<uint4>() : R.brec.as<uint4>();
    uint4* spare = first ? R.brec.as<uint4>() : R.rec.as<uint4>();
    const uint32_t* skeys = first ? R.ev_val.as<uint32_t>() : R.ev_key.as<uint32_t>();
    bucket_offsets<<<div_up((uint64_t)H + 1, 256), 256, 0, s>>>(skeys, n, H, o->ev_off);
    segment_sort_v5<<<div_up(H, kSegDst), 256, 0, s>>>(
        H, o->ev_off, sorted, rd->round_end, seq_base, o->ev_deliver, o->ev_src,
        o->ev_seq, o->ev_pkt, R.ev_val2.as<uint32_t>());
    segment_sort_v2_big<<<64, 256, 0, s>>>(R.ev_val2.as<uint32_t>(), o->ev_off, sorted,
                                           spare, rd->round_end, seq_base,
                                           o->ev_deliver, o->ev_src, o->ev_seq, o->ev_pkt);
    return relay_read_red(ctx);
}

}  // namespace shd
