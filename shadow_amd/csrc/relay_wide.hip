// Relay pipeline 1 (overview: relay_priv.h): 64-bit deliver times, for a table with a path latency of
// 2^32 ns or more, or a round whose deliver offsets need more than 32 bits.
#include <algorithm>

#include "relay_priv.h"
#include "scan.h"

namespace shd {

struct RelayArgs {
    uint32_t n_hosts, n_nodes;
    uint32_t src_lo, n_src;    // source hosts of this context: [src_lo, src_lo + n_src)
    const uint32_t* src_off;   // [n_src + 1], host src_lo + k's sends are [src_off[k], src_off[k+1])
    const uint64_t* send_time;
    const uint32_t* dst_host;
    const uint32_t* payload;
    const double* chance;
    const uint32_t* draw_cpu;  // CPU-drawn top 32 bits of next_u64 per packet (shd_relay_flush), or null
    const uint32_t* host_node;
    const uint64_t* lat;
    const float* loss;
    const uint64_t* rng;       // host state at round start (read)
    const uint64_t* next_id;
    uint64_t* rng_out;         // host state after the round (written; committed on success)
    uint64_t* next_id_out;
    unsigned long long* counts;  // nullable
    uint64_t round_end, sim_end, bootstrap_end;
    uint8_t* status;
    uint64_t* deliver;
    uint64_t* seq;
    uint32_t* slot;
    uint32_t* dst_cnt;
    unsigned long long* red;     // [0] min deliver, [1] min latency, [2] n_sent, [3] bad dst
};

__global__ __launch_bounds__(256) void relay_stamp(RelayArgs a) {
    const uint32_t hl = blockIdx.x * 256 + threadIdx.x, h = a.src_lo + hl;
    uint64_t my_min_d = ~0ull, my_min_l = ~0ull, my_sent = 0;
    if (hl < a.n_src) {
        Xoshiro r{a.rng[4 * (size_t)h], a.rng[4 * (size_t)h + 1], a.rng[4 * (size_t)h + 2],
                  a.rng[4 * (size_t)h + 3]};
        uint64_t id = a.next_id[h];
        const uint32_t sn = a.host_node[h];
        const uint32_t i1 = a.src_off[hl + 1];
        for (uint32_t i = a.src_off[hl]; i < i1; ++i) {
            const uint64_t now = a.send_time[i];
            uint8_t st = kStSkipped;
            if (now < a.sim_end) {
                const uint32_t d = a.dst_host[i];
                if (d >= a.n_hosts) {  // "No host ID for dest address" (worker.rs:350-355)
                    atomicMin(&a.red[3], (unsigned long long)i);
                    a.status[i] = kStSkipped;
                    continue;
                }
                const size_t pi = (size_t)sn * a.n_nodes + a.host_node[d];
                const double reliability = (double)one_minus(a.loss[pi]);
                bool ge;
                if (a.draw_cpu) {   // the top 32 bits decide exactly for a table reliability (draw_drops)
                    bool tie = false;
                    ge = draw_drops(a.draw_cpu[i], reliability, tie);
                } else {
                    ge = (a.chance ? a.chance[i] : r.gen_f64()) >= reliability;
                }
                const bool boot = now < a.bootstrap_end;
                if (!boot && ge && a.payload[i] > 0) {
                    st = kStDropped;
                } else {
                    const uint64_t delay = a.lat[pi];
                    uint64_t t = now + delay;
                    if (t < a.round_end) t = a.round_end;
                    st = kStSent;
                    a.deliver[i] = t;
                    a.seq[i] = id++;
                    a.slot[i] = atomicAdd(&a.dst_cnt[d], 1u);
                    if (a.counts) atomicAdd(&a.counts[pi], 1ull);
                    my_min_d = t < my_min_d ? t : my_min_d;
                    my_min_l = delay < my_min_l ? delay : my_min_l;
                    ++my_sent;
                }
            }
            a.status[i] = st;
        }
        a.rng_out[4 * (size_t)h] = r.s0;
        a.rng_out[4 * (size_t)h + 1] = r.s1;
        a.rng_out[4 * (size_t)h + 2] = r.s2;
        a.rng_out[4 * (size_t)h + 3] = r.s3;
        a.next_id_out[h] = id;
    }
    my_min_d = wave_min_u64(my_min_d);
    my_min_l = wave_min_u64(my_min_l);
    for (int o = 32; o > 0; o >>= 1) my_sent += __shfl_xor(my_sent, o);
    if ((threadIdx.x & 63) == 0) {
        if (my_min_d != ~0ull) atomicMin(&a.red[0], (unsigned long long)my_min_d);
        if (my_min_l != ~0ull) atomicMin(&a.red[1], (unsigned long long)my_min_l);
        if (my_sent) atomicAdd(&a.red[2], (unsigned long long)my_sent);
    }
}

// Per-packet source host from the grouped offsets (binary search; hosts are few per packet).
__device__ __forceinline__ uint32_t owner_of(const uint32_t* off, uint32_t n_hosts, uint32_t i) {
    uint32_t lo = 0, hi = n_hosts;  // find h with off[h] <= i < off[h+1]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void relay_scatter(
    uint64_t n, uint32_t n_src, uint32_t src_lo, const uint32_t* __restrict__ src_off,
    const uint8_t* __restrict__ status, const uint32_t* __restrict__ dst_host,
    const uint32_t* __restrict__ slot, const uint64_t* __restrict__ deliver,
    const uint64_t* __restrict__ seq, const uint32_t* __restrict__ ev_off,
    uint64_t* __restrict__ ev_deliver, uint32_t* __restrict__ ev_src, uint64_t* __restrict__ ev_seq,
    uint32_t* __restrict__ ev_pkt) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || status[i] != kStSent) return;
    const uint32_t pos = ev_off[dst_host[i]] + slot[i];
    ev_deliver[pos] = deliver[i];
    ev_src[pos] = src_lo + owner_of(src_off, n_src, (uint32_t)i);
    ev_seq[pos] = seq[i];
    ev_pkt[pos] = (uint32_t)i;
}

// Sort one destination's bucket by (deliver, src, seq) -- bitonic network in LDS.
constexpr uint32_t kV1Cap = 1024;

struct EvKey {
    uint64_t t;
    uint64_t sq;   // seq
    uint32_t src;
    uint32_t pkt;
};
__device__ __forceinline__ bool ev_less(const EvKey& a, const EvKey& b) {
    if (a.t != b.t) return a.t < b.t;
    if (a.src != b.src) return a.src < b.src;
    return a.sq < b.sq;
}

__global__ __launch_bounds__(256) void segment_sort(
    uint32_t n_hosts, const uint32_t* __restrict__ ev_off, uint64_t* __restrict__ ev_deliver,
    uint32_t* __restrict__ ev_src, uint64_t* __restrict__ ev_seq, uint32_t* __restrict__ ev_pkt,
    uint32_t* __restrict__ big) {
    __shared__ EvKey s[kV1Cap];
    const uint32_t d = blockIdx.x;
    const uint32_t b = ev_off[d], n = ev_off[d + 1] - b;
    if (n <= 1) return;
    if (n > kV1Cap) {
        if (threadIdx.x == 0) big[atomicAdd(&big[0], 1u) + 1] = d;
        return;
    }
    uint32_t P = 1;
    while (P < n) P <<= 1;
    for (uint32_t i = threadIdx.x; i < P; i += 256) {
        if (i < n)
            s[i] = EvKey{ev_deliver[b + i], ev_seq[b + i], ev_src[b + i], ev_pkt[b + i]};
        else
            s[i] = EvKey{~0ull, ~0ull, ~0u, ~0u};
    }
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < P; i += 256) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const bool up = (i & k) == 0;
                    EvKey x = s[i], y = s[l];
                    if (ev_less(y, x) == up) {
                        s[i] = y;
                        s[l] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        const EvKey e = s[i];
        ev_deliver[b + i] = e.t;
        ev_src[b + i] = e.src;
        ev_seq[b + i] = e.sq;
        ev_pkt[b + i] = e.pkt;
    }
}

// Oversized buckets (> kV1Cap events for one destination in one round): bottom-up merge
// sort of that bucket by one workgroup through a global scratch area.
__global__ __launch_bounds__(256) void segment_sort_big(
    const uint32_t* __restrict__ big, const uint32_t* __restrict__ ev_off,
    uint64_t* __restrict__ ev_deliver, uint32_t* __restrict__ ev_src, uint64_t* __restrict__ ev_seq,
    uint32_t* __restrict__ ev_pkt, EvKey* __restrict__ tmp) {
    const uint32_t d = big[1 + blockIdx.x];
    const uint32_t b = ev_off[d], n = ev_off[d + 1] - b;
    EvKey* A = tmp + b;  // this bucket's slice of the scratch (one EvKey per event)
    for (uint32_t i = threadIdx.x; i < n; i += 256)
        A[i] = EvKey{ev_deliver[b + i], ev_seq[b + i], ev_src[b + i], ev_pkt[b + i]};
    __syncthreads();
    // merge passes of run width w; each element finds its output rank by binary search in
    // the sibling run (keys are unique, so ranks never collide)
    for (uint32_t w = 1; w < n; w <<= 1) {
        // merge runs [i, i+w) and [i+w, i+2w) into ev_* arrays, then copy back
        for (uint32_t o = threadIdx.x; o < n; o += 256) {
            const uint32_t run = o / (2 * w), lo = run * 2 * w;
            const uint32_t mid = min(lo + w, n), hi = min(lo + 2 * w, n);
            // rank of element o within the merged output: binary search in the other run
            const EvKey x = A[o];
            uint32_t rank;
            if (o < mid) {
                uint32_t l = mid, h = hi;  // count of elements in right run strictly less
                while (l < h) {
                    const uint32_t m = (l + h) >> 1;
                    if (ev_less(A[m], x)) l = m + 1; else h = m;
                }
                rank = (o - lo) + (l - mid);
            } else {
                uint32_t l = lo, h = mid;  // count of elements in left run <= x (keys unique)
                while (l < h) {
                    const uint32_t m = (l + h) >> 1;
                    if (ev_less(x, A[m])) h = m; else l = m + 1;
                }
                rank = (o - mid) + (l - lo);
            }
            const uint32_t dst = b + lo + rank;
            ev_deliver[dst] = x.t;
            ev_src[dst] = x.src;
            ev_seq[dst] = x.sq;
            ev_pkt[dst] = x.pkt;
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n; i += 256)
            A[i] = EvKey{ev_deliver[b + i], ev_seq[b + i], ev_src[b + i], ev_pkt[b + i]};
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------------
// v1 pipeline: u64 deliver times (used when a path latency or deliver offset needs > 32 bits)
shd_status relay_device_v1(shd_ctx* ctx, const shd_batch* b, const shd_round* rd, shd_relay_out* o) {
    RelayState& R = ctx->relay;
    hipStream_t s = ctx->stream;
    const uint64_t n = b->n_packets;
    const uint32_t H = R.n_hosts;
    SHD_TRY(R.ev_key.ensure(std::max<uint64_t>(n, 1) * 8));   // deliver per packet
    SHD_TRY(R.ev_key2.ensure(std::max<uint64_t>(n, 1) * 8));  // seq per packet
    SHD_TRY(R.ev_val.ensure(std::max<uint64_t>(n, 1) * 4));   // slot per packet
    unsigned long long init[8] = {~0ull, ~0ull, 0ull, ~0ull, 0ull, 0ull, 0ull, 0ull};
    SHD_HIP(hipMemcpyAsync(R.red.p, init, sizeof(init), hipMemcpyHostToDevice, s));
    SHD_HIP(hipMemsetAsync(R.dst_cnt.p, 0, (size_t)(H + 1) * 4, s));
    RelayArgs a{};
    a.n_hosts = H;
    a.n_nodes = R.n_nodes;
    a.src_lo = R.src_lo;
    a.n_src = R.n_src;
    a.src_off = b->src_off;
    a.send_time = b->send_time;
    a.dst_host = b->dst_host;
    a.payload = b->payload;
    a.chance = b->chance;
    a.draw_cpu = R.cpu_draws ? R.draws.as<uint32_t>() : nullptr;
    a.host_node = R.host_node.as<uint32_t>();
    a.lat = R.own_table ? R.lat.as<uint64_t>() : ctx->t_lat.as<uint64_t>();
    a.loss = R.own_table ? R.loss.as<float>() : ctx->t_loss.as<float>();
    a.rng = R.rng.as<uint64_t>();
    a.next_id = R.next_id.as<uint64_t>();
    a.rng_out = R.rng2.as<uint64_t>();
    a.next_id_out = R.next_id2.as<uint64_t>();
    a.counts = R.count_on ? R.counts_round.as<unsigned long long>() : nullptr;
    a.round_end = rd->round_end;
    a.sim_end = rd->sim_end;
    a.bootstrap_end = rd->bootstrap_end;
    a.status = o->status;
    a.deliver = R.ev_key.as<uint64_t>();
    a.seq = R.ev_key2.as<uint64_t>();
    a.slot = R.ev_val.as<uint32_t>();
    a.dst_cnt = R.dst_cnt.as<uint32_t>();
    a.red = R.red.as<unsigned long long>();
    relay_stamp<<<div_up(std::max<uint32_t>(R.n_src, 1), 256), 256, 0, s>>>(a);
    SHD_HIP(hipGetLastError());
    // destination offsets: one hand-written look-back scan launch (scan.h); ev_off must be
    // 16-byte aligned (the relay's own buffers are; a caller's device array from hipMalloc too)
    SHD_TRY(scan_excl2(R.scan, R.dst_cnt.as<uint32_t>(), o->ev_off, nullptr, nullptr, (uint64_t)H + 1, s));
    if (n)
        relay_scatter<<<div_up(n, 256), 256, 0, s>>>(n, R.n_src, R.src_lo, b->src_off, o->status, b->dst_host,
                                                     R.ev_val.as<uint32_t>(), R.ev_key.as<uint64_t>(),
                                                     R.ev_key2.as<uint64_t>(), o->ev_off, o->ev_deliver,
                                                     o->ev_src, o->ev_seq, o->ev_pkt);
    SHD_TRY(R.ev_val2.ensure((size_t)(H + 2) * 4));
    SHD_HIP(hipMemsetAsync(R.ev_val2.p, 0, 4, s));
    segment_sort<<<H, 256, 0, s>>>(H, o->ev_off, o->ev_deliver, o->ev_src, o->ev_seq, o->ev_pkt,
                                   R.ev_val2.as<uint32_t>());
    SHD_HIP(hipGetLastError());
    uint32_t n_big = 0;
    SHD_HIP(hipMemcpyAsync(&n_big, R.ev_val2.p, 4, hipMemcpyDeviceToHost, s));
    SHD_HIP(hipMemcpyAsync(R.red_host, R.red.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    SHD_HIP(hipStreamSynchronize(s));
    if (n_big) {
        SHD_TRY(R.tmp.ensure(std::max<uint64_t>(n, 1) * sizeof(EvKey)));
        segment_sort_big<<<n_big, 256, 0, s>>>(R.ev_val2.as<uint32_t>(), o->ev_off, o->ev_deliver,
                                               o->ev_src, o->ev_seq, o->ev_pkt, R.tmp.as<EvKey>());
        SHD_HIP(hipGetLastError());
        SHD_HIP(hipStreamSynchronize(s));
    }
    return SHD_OK;
}

}  // namespace shd
