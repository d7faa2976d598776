// Per-round inter-host packet relay on gfx950: the overview, and what the relay's units share.
//
// Reference semantics, per staged send (FlyearthR/shadow src/main/core/worker.rs:328-413):
//   now >= sim_end -> nothing happens (no RNG draw, no status)                      :334-341
//   reliability = (1.0f32 - loss) as f64                                 WorkerShared :538-543
//   chance = src_host.rng.gen::<f64>() = (xoshiro256++ >> 11) * 2^-53                  :365
//   drop iff !bootstrapping && chance >= reliability && payload_size > 0              :370-378
//   deliver = max(now + latency, round_end); next-event-time min; lowest-used-latency  :380-406
//   event (deliver, Packet, src_host_id, src_host_event_id) into the dst queue  :408-411, 619-629
// Destination order = EventQueue pop order (core/work/event.rs:84-155): time, then src host id,
// then src event id.  Every event of round r has deliver >= round_end, so batching the whole
// round to the barrier (core/manager.rs:455-464) is exact.
//
// Pipelines (one stream, one host sync per round):
//   7  K0 draws, bin histogram + scans; K1 stamp places every record into its destination
//      bin (32 destinations); K4 bin_sort_v7 sorts each bin in LDS (decoupled look-back for
//      the event offsets) and stores the events in order
//   3  K0; K1 stamp writes records by packet; K2 radix sort by destination; K3 offsets; K4
//      per-destination wave sort (fallback when a bin overflows pipeline 7's limits)
//   1  64-bit records (path latencies >= 2^32 ns)
//   8  under a communicator: pipeline 7's K0 + K1 on every rank, the bins restarting at every
//      rank's first destination; the records are exchanged as they lie and each rank runs K4
//      over its own bins with the records gathered from every sender (no merge pass).  A rank
//      that cannot take it sends every rank to the packing path: pipeline 7, 3 or 1 locally,
//      24-byte events exchanged and merged per destination (reported as the local pipeline)
// Units -- every kernel is defined in one unit and launched only there; another unit reaches it
// through a host function declared below:
//   relay_stamp.hip   3 7 8   K0 and the K1 stamps (by packet for 3, into the bins for 7 and 8)
//   relay_bins.hip    7 8     pipeline 7's histograms, scans and K4 (for 8 over gathered records)
//   relay_shard.hip   8       the sharded rounds: the bins exchanged, and the packing path
//   relay_radix.hip   3       K2-K4 of the radix back end
//   relay_wide.hip    1       the 64-bit pipeline
//   relay.hip                 the ladder over the pipelines, the commit, the C entry points
// relay_bins.h holds the limits and the bin arithmetic that several of them compile.
#pragma once
#include <algorithm>

#include "ctx.h"
#include "wave.h"

namespace shd {

constexpr uint32_t kStSkipped = 0, kStDropped = 1, kStSent = 2;

__device__ __forceinline__ uint64_t rotl64(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }

struct Xoshiro {
    uint64_t s0, s1, s2, s3;
    __device__ __forceinline__ uint64_t next() {
        const uint64_t res = rotl64(s0 + s3, 23) + s0;
        const uint64_t t = s1 << 17;
        s2 ^= s0;
        s3 ^= s1;
        s1 ^= s2;
        s0 ^= s3;
        s2 ^= t;
        s3 = rotl64(s3, 45);
        return res;
    }
    // rand 0.8.5 Standard for f64: 53 high bits, multiply-based, [0, 1)
    __device__ __forceinline__ double gen_f64() {
        return (double)(next() >> 11) * (1.0 / 9007199254740992.0);
    }
};

// chance >= reliability (worker.rs:365-370) from the draw's top 32 bits h = draw >> 32, which is
// all K0 keeps (4 bytes per draw instead of 8).  chance = (draw >> 11) * 2^-53 exactly, so the
// test is draw >> 11 >= T = ceil(reliability * 2^53) (exact: a power-of-two scale).  With
// th = T >> 21 it is h >= th when T is a multiple of 2^21.  That always holds for a table loss
// in [0, 1]: reliability = 1f32 - loss is >= 2^-9 (then reliability * 2^53 = m * 2^(e + 30),
// e >= -9, a multiple of 2^21) or is 1 - loss for loss in [0.5, 1], a multiple of 2^-24 (T a
// multiple of 2^29).  For any other value h > th decides unless h == th, where the low bits
// would: `tie` is set and the round is redone on the 64-bit pipeline (its own exact draws).
// reliability <= 0 always drops, NaN never (as the f64 comparison).
__device__ __forceinline__ bool draw_drops(uint32_t h, double reliability, bool& tie) {
    if (!(reliability > 0.0)) return reliability <= 0.0;
    if (reliability >= 1.0) return false;   // chance < 1
    const uint64_t T = (uint64_t)ceil(reliability * 9007199254740992.0);
    const uint64_t th = T >> 21;
    const bool low = (T & 0x1FFFFFull) != 0;
    if (low && (uint64_t)h == th) tie = true;
    return (uint64_t)h >= th + (low ? 1u : 0u);
}

// The narrow pipelines' arguments (relay_stamp.hip, relay_bins.hip, relay_radix.hip)
struct RelayArgs3 {
    uint32_t n_hosts, n_nodes;
    uint32_t src_lo, n_src;    // source hosts of this context: [src_lo, src_lo + n_src)
    const uint32_t* src_off;   // [n_src + 1], indexed by host - src_lo
    const uint64_t* send_time;
    const uint32_t* dst_host;
    const uint32_t* payload;
    const double* chance;
    uint32_t keep_rng;         // 1: the draws came from the CPU (shd_relay_flush): device streams untouched
    const uint32_t* host_node;
    const uint32_t* order;     // the n_src source host ids sorted by host_node (workgroup -> hosts)
    const uint2* path;         // {latency ns (u32), packet loss bits} per node pair
    const uint64_t* rng;
    const uint64_t* next_id;
    uint64_t* rng_out;
    uint64_t* next_id_out;
    unsigned long long* counts;
    uint64_t round_end, sim_end, bootstrap_end;
    uint32_t abs_seq;    // 1: every event id of the round fits 32 bits -> records hold absolute ids
    uint8_t* status;
    uint4* rec;          // per packet (valid when SENT)
    uint32_t* key;       // per packet: destination host if SENT, else n_hosts (sorts last)
    unsigned long long* red;   // [0] min deliver [1] min latency [2] n_sent [3] bad dst [4] wide
                               // [5] send-order violation [6] v7 bin overflow
    // v7 (destination-bin placement): the records of bin b written by stamp workgroup g start at
    // bin_base[b] + seg_pre[g * n_bins + b]
    const uint32_t* bin_base;
    const uint32_t* seg_pre;
    uint32_t n_bins;
    uint32_t gs;         // hosts per group of relay_stamp_v6 / relay_bin_hist (<= kS5Hosts)
    // v7 under a communicator (relay_round_sharded_v7): every rank's destinations [r * sh_per,
    // ...) start a fresh bin, so rank r's bins are [r * sh_bpr, ...) and the records bound for it
    // one contiguous slice; sh_mul = ceil(2^40 / sh_per).  sh_per = 0: bins of consecutive hosts.
    uint32_t sh_per, sh_bpr;
    uint64_t sh_mul;
};

// The bins of a sharded round (relay_round_sharded_v7): rank r's destinations [r * per, ...)
// start bin r * bpr; n_bins over all ranks
struct XShard {
    uint32_t per = 0, bpr = 0, n_bins = 0;
    uint64_t mul = 0;
    uint32_t first_bin(uint32_t r) const { return std::min<uint32_t>(r * bpr, n_bins); }
};

// K4 of a sharded round (relay_round_sharded_v7, bin_sort_v7<true>): bin j of this rank's own bins takes
// its records from every sender's received slice: sender q's records of the bin start at
// rbase[q] + sc[q * stride + fb + j] - sc[q * stride + fb] (sc: the senders' exclusive bin scans
// from the gathered sizing rows).  Packet indices are per sender; the sort key uses the global
// packet order (the senders' batches back to back, pbase[q] = packets of the senders before q),
// which is (src host, event id) order because the senders own increasing source ranges.
struct XSrc {
    uint32_t world, me, fb, stride, kq;
    const uint32_t* sc;
    const uint32_t* rbase;   // sender q's slice in the received records (q != me)
    const uint32_t* pbase;
    const uint4* own;        // this rank's own records stay where its stamp put them (never exchanged)
    const uint64_t* rst;     // [world] the status each sender carried into the exchange (own: own_st)
    uint32_t own_st;
};

// relay.hip
RelayArgs3 relay_args3(shd_ctx* ctx, const shd_batch* b, const shd_round* rd, shd_relay_out* o);
// the pending launch error, then the round's reductions into R.red_host (one host sync)
shd_status relay_read_red(shd_ctx* ctx);
// the ladder over the local pipelines (nothing of the hosts' state committed), and the commit
shd_status relay_run(shd_ctx* ctx, const shd_batch* b, const shd_round* rd, shd_relay_out* o);
shd_status relay_commit(shd_ctx* ctx, shd_relay_out* o);
// shd_relay_flush (flush.hip): one round on the batch it grouped on the device
shd_status relay_flush_round(shd_ctx* ctx, const shd_batch* b, const shd_round* rd, shd_relay_out* o);

// relay_stamp.hip
// K0 (no launch when the batch carries chances or the CPU's draws) and the stamp that writes the
// records by packet (pipeline 3)
void relay_launch_draws(shd_ctx* ctx, const RelayArgs3& a);
void relay_launch_stamp(shd_ctx* ctx, const RelayArgs3& a);
// the stamp that places the records into their bins (pipelines 7, 8): G workgroups, lds dynamic bytes
void relay_launch_stamp_bins(shd_ctx* ctx, const RelayArgs3& a, uint32_t G, size_t lds);
// that stamp's static LDS bytes (0: the query failed), its sends per chunk, and relay_stamp_v6's
// LDS besides the host -> node map (shd_relay_setup: does the map fit)
size_t relay_stamp_bins_static_lds();
uint32_t relay_stamp_chunk();
uint32_t relay_stamp_fixed_lds();

// relay_bins.hip
bool relay_v7_ok(shd_ctx* ctx, uint64_t n, uint32_t n_bins);
XShard xshard(uint32_t H, uint32_t world);
// v7 up to and including the stamp; with xsh (a sharded round) the records stay in their bins
// for the exchange (no bin sort, no read-back), else the bin sort and the reductions' read-back
shd_status relay_device_v7(shd_ctx* ctx, const shd_batch* b, const shd_round* rd, shd_relay_out* o,
                           const XShard* xsh = nullptr);
// K4 of a sharded round over this rank's nb bins and n_own destinations, into R.m_*; without
// bins only the event count and the agreed status are written
void relay_launch_bin_sort_x(shd_ctx* ctx, uint32_t n_own, uint32_t nb, uint64_t round_end, const XSrc& xs);

// relay_shard.hip
shd_status relay_shard_alloc(shd_ctx* ctx);   // buffers sized by the host count and the ranks (shd_relay_setup)
// shd_relay_flush under a communicator (flush.hip): this rank's grouped sends, the CPU's draws
shd_status relay_flush_round_sharded(shd_ctx* ctx, const shd_batch* b, const shd_round* rd, shd_relay_out* o);

// relay_wide.hip, relay_radix.hip: one pipeline attempt each
shd_status relay_device_v1(shd_ctx* ctx, const shd_batch* b, const shd_round* rd, shd_relay_out* o);
shd_status relay_device_v3(shd_ctx* ctx, const shd_batch* b, const shd_round* rd, shd_relay_out* o);

}  // namespace shd
