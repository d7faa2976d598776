// The packet ledger: each relay batch's (total size, packet id) per packet, kept on the device
// from the round that sent the batch until its last event has popped from the destination event
// queues.  A popped event carries only its tag, (batch number << 32) | index in that batch; the
// inbound stage wants the packet's total size and the caller's packet id.  ledger_gather turns a
// window's popped tags into those two arrays without the host seeing a packet.
//
// Storage (the bookkeeping is ledger_book.h's):
//   arena   uint2 {size, pkt} entries; a batch is one contiguous slice, written by ledger_record
//   rows    LedgerRow {batch, base, n_packets, live} per slot = batch & mask; the batches held are
//           the numbers oldest .. oldest + span - 1, row d = batch - oldest.  A gather only reads
//           the rows: `live` is the count at the call's start for every workgroup alike
//   pops    per slot, the running gather's pops; ledger_settle takes them off the rows' live
//           counts, zeroes them and writes every held batch's new count behind the status word,
//           which the call reads back once: that is how the host learns which batches are gone
//
// ledger_gather, a workgroup per 1024 events, four per thread (two 16-byte tag loads):
//   A  the first kLgRows rows of the span -> LDS; per event the row, the checks, the dependent
//      8-byte entry load (issued here, used in C); the pops counted per wave: the lanes that name
//      one batch are found with __ballot and their leader adds the count to the batch's LDS
//      counter -- one LDS add per wave and distinct batch, where a per-event add would put 64
//      lanes on one word (a window's pops come from a handful of batches, often from one)
//   B  one global atomicAdd per workgroup and touched batch onto pops[slot]; a sum past the row's
//      live count marks the batch overdrawn for this workgroup
//   C  two coalesced 8-byte stores per thread and vector (sizes, ids)
// A batch at row kLgRows or beyond (more batches held than the LDS table has rows) takes the same
// path with its row read from global memory and its wave's count added to pops[slot] directly.
//
// Every index is checked before it is used for a load: a tag whose batch is not held or has no
// live event left, an index >= the batch's n_packets (or an entry past the arena, which the
// bookkeeping rules out), a batch popped more often than its live count.  Such an event gets
// UINT32_MAX in both outputs and the call fails; nothing is read for it.  Of an overdrawn batch
// the events of every workgroup (row >= kLgRows: wave) whose count went past the live count are
// refused -- at least the surplus; which ones depends on the order the atomics landed in.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "ctx.h"
#include "scan.h"

namespace shd {

constexpr uint32_t kLgThreads = 256;
constexpr uint32_t kLgVec = 2;                            // 16-byte tag loads per thread
constexpr uint32_t kLgTile = kLgThreads * kLgVec * 2;     // events per workgroup
constexpr uint32_t kLgRows = 1024;                        // rows (and counters) in LDS: 16 + 4 KB
constexpr uint32_t kLgMaxBatches = 4096;
constexpr uint64_t kLgArena0 = 65536;                     // the arena's first size, entries
// status bits (words[0]); any of them is SHD_ERR_INVALID
constexpr uint32_t kLgNotLive = 1u;     // the tag's batch is not held, or has no live event left
constexpr uint32_t kLgBadIndex = 2u;    // index >= the batch's n_packets
constexpr uint32_t kLgOverdrawn = 4u;   // a batch popped more often than its live count
static_assert(sizeof(LedgerRow) == 16, "LedgerRow layout");

__global__ __launch_bounds__(256) void ledger_record(const uint32_t* __restrict__ size, const uint32_t* __restrict__ pkt,
                                                     uint64_t n, uint2* __restrict__ slice, LedgerRow* row_slot,
                                                     LedgerRow row) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) slice[i] = make_uint2(size[i], pkt[i]);
    if (i == 0) *row_slot = row;
}

// The lanes with ok set name row d; per distinct d one lane adds the lanes' count: to the LDS
// counter (d < nl), or to the slot's global counter, whose answer decides `over` for those lanes.
__device__ __forceinline__ bool lg_count(bool ok, uint32_t d, uint32_t nl, uint32_t* s_cnt, uint32_t* pop_slot,
                                         uint32_t live) {
    const uint32_t lane = threadIdx.x & 63;
    bool over = false;
    uint64_t todo = __ballot(ok);
    while (todo) {   // (todo is the same in every lane: the loop does not diverge)
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t kd = (uint32_t)__shfl((int)d, leader);
        const bool same = ok && d == kd;
        const uint64_t m = __ballot(same);
        const uint32_t c = (uint32_t)__popcll(m);
        uint32_t ov = 0;
        if (lane == (uint32_t)leader) {
            if (kd < nl) atomicAdd(&s_cnt[kd], c);
            else ov = atomicAdd(pop_slot, c) + c > live ? 1u : 0u;
        }
        ov = (uint32_t)__shfl((int)ov, leader);
        if (same && ov) over = true;
        todo &= ~m;
    }
    return over;
}

__global__ __launch_bounds__(256) void ledger_gather(
    const uint64_t* __restrict__ tag, uint64_t n, int vec_ok, const LedgerRow* __restrict__ rows, uint32_t mask,
    uint64_t oldest, uint32_t span, const uint2* __restrict__ arena, uint64_t arena_cap, uint32_t* pops,
    uint32_t* __restrict__ out_size, uint32_t* __restrict__ out_pkt, uint32_t* status) {
    __shared__ LedgerRow s_row[kLgRows];
    __shared__ uint32_t s_cnt[kLgRows];
    const uint32_t nl = min(span, kLgRows);
    for (uint32_t i = threadIdx.x; i < nl; i += kLgThreads) {
        s_row[i] = rows[(uint32_t)(oldest + i) & mask];
        s_cnt[i] = 0;
    }
    __syncthreads();
    const uint64_t tile = (uint64_t)blockIdx.x * kLgTile;
    uint32_t d[kLgVec][2];
    bool ok[kLgVec][2], over[kLgVec][2];
    uint2 ent[kLgVec][2];
    uint32_t err = 0;
#pragma unroll
    for (uint32_t v = 0; v < kLgVec; ++v) {
        const uint64_t i0 = tile + (uint64_t)v * (kLgThreads * 2) + threadIdx.x * 2;
        uint64_t t[2] = {0, 0};
        if (vec_ok && i0 + 1 < n) {
            const ulonglong2 q = *reinterpret_cast<const ulonglong2*>(tag + i0);
            t[0] = q.x;
            t[1] = q.y;
        } else {
            if (i0 < n) t[0] = tag[i0];
            if (i0 + 1 < n) t[1] = tag[i0 + 1];
        }
#pragma unroll
        for (uint32_t k = 0; k < 2; ++k) {
            const bool valid = i0 + k < n;
            const uint64_t b = t[k] >> 32;
            const uint32_t ix = (uint32_t)t[k];
            const uint64_t dd = b - oldest;           // (b < oldest: wraps far past span)
            const bool inspan = valid && dd < span;
            d[v][k] = inspan ? (uint32_t)dd : 0u;
            LedgerRow r{kLedgerNoBatch, 0, 0, 0};
            if (inspan) r = d[v][k] < nl ? s_row[d[v][k]] : rows[(uint32_t)b & mask];
            const bool held = inspan && r.batch == (uint32_t)b && r.live > 0;
            const uint64_t at = (uint64_t)r.base + ix;
            const bool good = held && ix < r.n_packets && at < arena_cap;
            if (valid && !held) err |= kLgNotLive;
            else if (valid && !good) err |= kLgBadIndex;
            ok[v][k] = good;
            ent[v][k] = make_uint2(~0u, ~0u);
            if (good) ent[v][k] = arena[at];
            over[v][k] = lg_count(good, d[v][k], nl, s_cnt, pops + ((uint32_t)b & mask), r.live);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nl; i += kLgThreads) {
        const uint32_t c = s_cnt[i];
        if (c) {
            const uint32_t old = atomicAdd(pops + ((uint32_t)(oldest + i) & mask), c);
            s_cnt[i] = old + c > s_row[i].live ? 1u : 0u;   // from here on: the batch is overdrawn
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t v = 0; v < kLgVec; ++v) {
        const uint64_t i0 = tile + (uint64_t)v * (kLgThreads * 2) + threadIdx.x * 2;
        uint2 o[2];
#pragma unroll
        for (uint32_t k = 0; k < 2; ++k) {
            const bool ov = ok[v][k] && (d[v][k] < nl ? s_cnt[d[v][k]] != 0 : over[v][k]);
            if (ov) err |= kLgOverdrawn;
            o[k] = ok[v][k] && !ov ? ent[v][k] : make_uint2(~0u, ~0u);
        }
        if (i0 + 1 < n) {   // (engine-owned outputs: 8-byte aligned at every even index)
            *reinterpret_cast<uint2*>(out_size + i0) = make_uint2(o[0].x, o[1].x);
            *reinterpret_cast<uint2*>(out_pkt + i0) = make_uint2(o[0].y, o[1].y);
        } else if (i0 < n) {
            out_size[i0] = o[0].x;
            out_pkt[i0] = o[0].y;
        }
    }
    if (err) atomicOr(status, err);
}

// Row d of the span: its pops come off its live count (an overdrawn batch keeps its count and
// fails the call), the slot's counter is zero again, the new count goes behind the status word.
__global__ __launch_bounds__(256) void ledger_settle(LedgerRow* rows, uint32_t mask, uint64_t oldest, uint32_t span,
                                                     uint32_t* pops, unsigned long long* words) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= span) return;
    const uint32_t slot = (uint32_t)(oldest + i) & mask;
    const uint32_t p = pops[slot];
    pops[slot] = 0;
    LedgerRow r = rows[slot];
    unsigned long long live = ~0ull;   // no batch of this number is held
    if (r.batch == (uint32_t)(oldest + i)) {
        if (p > r.live) atomicOr(reinterpret_cast<uint32_t*>(words), kLgOverdrawn);
        else r.live -= p;
        rows[slot].live = r.live;
        live = r.live;
    }
    words[1 + i] = live;
}

// ------------------------------------------------------------------------------------------
// The sharded record (shd_ledger_record_sharded).  A sharded relay round hands a rank the events
// of ITS destination hosts, whose ev_pkt is the packet's index in its SENDER rank's batch -- a
// batch the receiver never saw.  So after a committed round every rank sends each SENT entry's
// (index, {size, pkt}) to the rank that owns the entry's destination, records what it received
// as one batch of its own, and rewrites its events' ev_pkt to the index in that slice:
//   ledger_pack_count / _scatter   sender side, a workgroup per 1024 batch entries: a stable
//       compaction per destination rank into rank-major send buffers.  Per wave the lanes bound
//       for one rank are found with __ballot (as ledger_gather counts its pops): their count is
//       the (wave, pass) slot's LDS word for that rank, a lane's place the set bits below it --
//       no atomic anywhere.  The per-(rank, workgroup) counts are scanned rank-major (scan.h), so
//       a rank's entries are one slice with the indices ascending; the scatter repeats the
//       ballots and adds the slots before its own
//   ledger_words     the three words per peer of the sizing all-to-all: entries for it, own status,
//       own batch entries (the receiver sizes its inverse table from them)
//   ledger_remap_table   receiver side, a thread per received event: the sender is the owner of
//       ev_src; the entry's place comes from an inverse table over the senders' batches, which
//       ledger_inv_scatter fills from the received indices (ledger_remap: the same by a binary
//       search of the sender's ascending slice -- 21 dependent loads at 2.5 M entries)
//   ledger_record_ent  the received entries into the batch's arena slice, with its row
constexpr uint32_t kLpThreads = 256, kLpPasses = 4, kLpTile = kLpThreads * kLpPasses;
constexpr uint32_t kLpSlots = (kLpThreads / 64) * kLpPasses;
constexpr uint32_t kLpMaxWorld = 256;   // ranks: kLpSlots words of LDS each (16 KB at the limit)
constexpr uint32_t kLgNoEntry = 1u;     // remap status: an event whose packet its sender never sent

// The lanes with ok set name rank r: per distinct r its leader stores the lanes' count in the
// slot's word of that rank; -> the number of such lanes below this one.
__device__ __forceinline__ uint32_t lp_wave(bool ok, uint32_t r, uint32_t* s_slot) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t below = 0;
    uint64_t todo = __ballot(ok);
    while (todo) {   // (todo is the same in every lane: the loop does not diverge)
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t kr = (uint32_t)__shfl((int)r, leader);
        const bool same = ok && r == kr;
        const uint64_t m = __ballot(same);
        if (lane == (uint32_t)leader) s_slot[kr] = (uint32_t)__popcll(m);
        if (same) below = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        todo &= ~m;
    }
    return below;
}

// the tile's entries: which are SENT and whose; fills the slots' counts (s: [kLpSlots][world])
__device__ __forceinline__ void lp_tile(const uint8_t* __restrict__ status, const uint32_t* __restrict__ dst, uint64_t n,
                                        uint32_t n_hosts, uint32_t world, uint32_t* s, bool* sent, uint32_t* rank,
                                        uint32_t* below) {
    for (uint32_t i = threadIdx.x; i < kLpSlots * world; i += kLpThreads) s[i] = 0;
    __syncthreads();
    const uint64_t tile = (uint64_t)blockIdx.x * kLpTile;
    const uint32_t wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t p = 0; p < kLpPasses; ++p) {
        const uint64_t i = tile + (uint64_t)p * kLpThreads + threadIdx.x;
        sent[p] = i < n && status[i] == SHD_PKT_SENT;
        rank[p] = sent[p] ? shard_owner(n_hosts, world, dst[i]) : 0u;
        below[p] = lp_wave(sent[p], rank[p], s + (size_t)(p * (kLpThreads / 64) + wave) * world);
    }
    __syncthreads();
}

// cnt[r * n_wg + workgroup] = the tile's entries for rank r; cnt[world * n_wg] = 0 (the scan's end)
__global__ __launch_bounds__(256) void ledger_pack_count(const uint8_t* __restrict__ status,
                                                         const uint32_t* __restrict__ dst, uint64_t n, uint32_t n_hosts,
                                                         uint32_t world, uint32_t n_wg, uint32_t* __restrict__ cnt) {
    __shared__ uint32_t s[kLpSlots * kLpMaxWorld];
    bool sent[kLpPasses];
    uint32_t rank[kLpPasses], below[kLpPasses];
    lp_tile(status, dst, n, n_hosts, world, s, sent, rank, below);
    for (uint32_t r = threadIdx.x; r < world; r += kLpThreads) {
        uint32_t c = 0;
#pragma unroll
        for (uint32_t k = 0; k < kLpSlots; ++k) c += s[k * world + r];
        cnt[(size_t)r * n_wg + blockIdx.x] = c;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[(size_t)world * n_wg] = 0;
}

// base: the scanned counts.  Entry i goes to base[rank][workgroup] + the slots before its own +
// the lanes below it; the send buffers hold n entries, every place is checked against that.
__global__ __launch_bounds__(256) void ledger_pack_scatter(const uint8_t* __restrict__ status,
                                                           const uint32_t* __restrict__ dst,
                                                           const uint32_t* __restrict__ size,
                                                           const uint32_t* __restrict__ pkt, uint64_t n, uint32_t n_hosts,
                                                           uint32_t world, uint32_t n_wg, const uint32_t* __restrict__ base,
                                                           uint32_t* __restrict__ s_idx, uint2* __restrict__ s_ent) {
    __shared__ uint32_t s[kLpSlots * kLpMaxWorld];
    bool sent[kLpPasses];
    uint32_t rank[kLpPasses], below[kLpPasses];
    lp_tile(status, dst, n, n_hosts, world, s, sent, rank, below);
    for (uint32_t r = threadIdx.x; r < world; r += kLpThreads) {
        uint32_t run = base[(size_t)r * n_wg + blockIdx.x];
#pragma unroll
        for (uint32_t k = 0; k < kLpSlots; ++k) {
            const uint32_t c = s[k * world + r];
            s[k * world + r] = run;
            run += c;
        }
    }
    __syncthreads();
    const uint64_t tile = (uint64_t)blockIdx.x * kLpTile;
    const uint32_t wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t p = 0; p < kLpPasses; ++p) {
        if (!sent[p]) continue;
        const uint64_t i = tile + (uint64_t)p * kLpThreads + threadIdx.x;
        const uint32_t at = s[(size_t)(p * (kLpThreads / 64) + wave) * world + rank[p]] + below[p];
        if (at < n) {
            s_idx[at] = (uint32_t)i;
            s_ent[at] = make_uint2(size[i], pkt[i]);
        }
    }
}

// The words for rank r: [0] entries for it (base == nullptr: none were packed), [1] this rank's
// status, [2] this rank's batch entries (the bound of the indices it sends).
constexpr uint32_t kLpWords = 3;
__global__ __launch_bounds__(256) void ledger_words(const uint32_t* __restrict__ base, uint32_t n_wg, uint32_t world,
                                                    int32_t status, uint64_t n_packets, uint64_t* __restrict__ words) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= world) return;
    words[kLpWords * r] = base ? base[(size_t)(r + 1) * n_wg] - base[(size_t)r * n_wg] : 0u;
    words[kLpWords * r + 1] = (uint64_t)(int64_t)status;
    words[kLpWords * r + 2] = n_packets;
}

__global__ __launch_bounds__(256) void ledger_fill(uint64_t* words, uint32_t n, uint64_t v) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) words[i] = v;
}

// The received words of sender q: [0] its entries here (their sum is n_ev: checked on the host),
// [2] its batch entries (their sum fits 32 bits where the table is used: checked on the host).
// -> s_base[q] = sender q's first entry in r_idx, s_pb[q] = its first slot in the inverse table.
__device__ __forceinline__ void lg_prefixes(const uint64_t* __restrict__ recv_words, uint32_t world, uint32_t* s_base,
                                            uint32_t* s_pb) {
    for (uint32_t q = threadIdx.x; q < world; q += 256) {
        s_base[q + 1] = (uint32_t)recv_words[kLpWords * q];
        s_pb[q + 1] = (uint32_t)recv_words[kLpWords * q + 2];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0, rp = 0;
        for (uint32_t q = 0; q < world; ++q) {
            const uint32_t c = s_base[q + 1], p = s_pb[q + 1];
            s_base[q] = run;
            s_pb[q] = rp;
            run += c;
            rp += p;
        }
        s_base[world] = run;
        s_pb[world] = rp;
    }
    __syncthreads();
}

// The inverse table, a slot per batch entry of every sender: inv[s_pb[q] + index in q's batch] =
// the entry's place in r_idx.  Only the received entries' slots are written; the table is not
// cleared, so a reader holds what it finds against r_idx (ledger_remap_table).
__global__ __launch_bounds__(256) void ledger_inv_scatter(uint32_t n_ev, uint32_t world,
                                                          const uint64_t* __restrict__ recv_words,
                                                          const uint32_t* __restrict__ r_idx, uint32_t* __restrict__ inv) {
    __shared__ uint32_t s_base[kLpMaxWorld + 1], s_pb[kLpMaxWorld + 1];
    lg_prefixes(recv_words, world, s_base, s_pb);
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= min(n_ev, s_base[world])) return;
    uint32_t lo = 0, hi = world;   // s_base[lo] <= j < s_base[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (s_base[mid] <= j) lo = mid;
        else hi = mid;
    }
    const uint32_t key = r_idx[j];
    if (key < s_pb[lo + 1] - s_pb[lo]) inv[s_pb[lo] + key] = (uint32_t)j;
}

// ev_pkt[e]: index in the sender's batch -> index in r_idx (= in the batch recorded here), through
// the inverse table: two dependent loads per event.  What the table holds is checked against the
// sender's slice and against r_idx before it is believed (a slot never written holds anything).
__global__ __launch_bounds__(256) void ledger_remap_table(const uint32_t* __restrict__ ev_src,
                                                          uint32_t* __restrict__ ev_pkt, uint32_t n_ev, uint32_t n_hosts,
                                                          uint32_t world, const uint64_t* __restrict__ recv_words,
                                                          const uint32_t* __restrict__ r_idx,
                                                          const uint32_t* __restrict__ inv, uint32_t* status) {
    __shared__ uint32_t s_base[kLpMaxWorld + 1], s_pb[kLpMaxWorld + 1];
    lg_prefixes(recv_words, world, s_base, s_pb);
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_ev) return;
    const uint32_t q = shard_owner(n_hosts, world, ev_src[e]);
    const uint32_t key = ev_pkt[e];
    const uint32_t lo = min(s_base[q], n_ev), end = min(s_base[q + 1], n_ev);
    uint32_t p = ~0u;
    if (key < s_pb[q + 1] - s_pb[q]) p = inv[s_pb[q] + key];
    const bool found = p >= lo && p < end && r_idx[p] == key;
    ev_pkt[e] = found ? p : ~0u;
    if (!found) atomicOr(status, kLgNoEntry);
}

// The same by a binary search of the sender's ascending index slice (no table: LEDGER_REMAP_SEARCH=1,
// or the senders' batches together pass 32 bits, or the table cannot be allocated).  The slice
// bounds are clamped to n_ev before any load.
__global__ __launch_bounds__(256) void ledger_remap(const uint32_t* __restrict__ ev_src, uint32_t* __restrict__ ev_pkt,
                                                    uint32_t n_ev, uint32_t n_hosts, uint32_t world,
                                                    const uint64_t* __restrict__ recv_words,
                                                    const uint32_t* __restrict__ r_idx, uint32_t* status) {
    __shared__ uint32_t s_base[kLpMaxWorld + 1], s_pb[kLpMaxWorld + 1];
    lg_prefixes(recv_words, world, s_base, s_pb);
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_ev) return;
    const uint32_t q = shard_owner(n_hosts, world, ev_src[e]);
    const uint32_t key = ev_pkt[e];
    uint32_t lo = min(s_base[q], n_ev);
    const uint32_t end = min(s_base[q + 1], n_ev);
    uint32_t hi = end;
    while (lo < hi) {   // the first index >= key
        const uint32_t mid = lo + (hi - lo) / 2;
        if (r_idx[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    const bool found = lo < end && r_idx[lo] == key;
    ev_pkt[e] = found ? lo : ~0u;
    if (!found) atomicOr(status, kLgNoEntry);
}

__global__ __launch_bounds__(256) void ledger_record_ent(const uint2* __restrict__ ent, uint64_t n,
                                                         uint2* __restrict__ slice, LedgerRow* row_slot, LedgerRow row) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) slice[i] = ent[i];
    if (i == 0) *row_slot = row;
}

shd_status comm_agree(shd_ctx* ctx, shd_status local) {
    if (!ctx->comm || ctx->comm->size == 1) return local;
    Comm& C = *ctx->comm;
    hipStream_t s = ctx->stream;
    uint64_t* w = reinterpret_cast<uint64_t*>(ctx->comm_scratch.as<char>() + comm_ledger_words_at(C.size));
    ledger_fill<<<1, 256, 0, s>>>(w + C.rank, 1, (uint64_t)(int64_t)local);
    if (hipGetLastError() != hipSuccess) {   // the word the peers read must carry a status: from the host
        const uint64_t v = (uint64_t)(int64_t)(local != SHD_OK ? local : SHD_ERR_HIP);
        (void)hipMemcpy(w + C.rank, &v, 8, hipMemcpyHostToDevice);
    }
    SHD_TRY(C.all_gather(w + C.rank, w, 8, s));   // agreed (LocalComm, HostComm) / fatal (RCCL)
    std::vector<uint64_t> all((size_t)C.size);
    SHD_HIP(hipMemcpyAsync(all.data(), w, all.size() * 8, hipMemcpyDeviceToHost, s));
    SHD_HIP(hipStreamSynchronize(s));
    for (int q = 0; q < C.size; ++q)
        if ((shd_status)all[q] != SHD_OK) return (shd_status)all[q];   // the lowest failing rank's
    return SHD_OK;
}

static shd_status ledger_live(shd_ctx* ctx, LedgerState** out) {
    if (!ctx) return SHD_ERR_INVALID;
    if (!ctx->ledger.ready) return SHD_ERR_STATE;   // not set up, or a refused event since
    *out = &ctx->ledger;
    return SHD_OK;
}

// the arena takes n more entries: its contents move to the front of a larger one, the rows follow
static shd_status ledger_grow(shd_ctx* ctx, LedgerState& L, uint64_t n) {
    hipStream_t s = ctx->stream;
    const LedgerMove m = L.book.plan_grow(n);
    if (m.new_cap >= 0xFFFFFFFFull) return SHD_ERR_NOMEM;   // bases are 32-bit
    DevBuf bigger;
    SHD_TRY(bigger.ensure(m.new_cap * sizeof(uint2)));
    for (int k = 0; k < 2; ++k)
        if (m.len[k])
            SHD_HIP(hipMemcpyAsync(bigger.as<uint2>() + m.dst[k], L.arena.as<uint2>() + m.src[k], m.len[k] * sizeof(uint2),
                                   hipMemcpyDeviceToDevice, s));
    L.book.apply_grow(m);
    SHD_HIP(hipMemcpyAsync(L.rows.p, L.book.rows.data(), L.book.rows.size() * sizeof(LedgerRow), hipMemcpyHostToDevice, s));
    SHD_HIP(hipStreamSynchronize(s));   // the copies have read the old arena before it is freed
    L.arena = std::move(bigger);
    return SHD_OK;
}

}  // namespace shd

using namespace shd;

extern "C" {

shd_status shd_ledger_setup(shd_ctx* ctx, uint32_t max_live_batches) {
    if (!ctx || max_live_batches > kLgMaxBatches) return SHD_ERR_INVALID;
    LedgerState& L = ctx->ledger;
    L.ready = false;
    ctx->win.opened = false;   // a window sequence starts over with its ledger
    ctx->win.has_out = false;
    SHD_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    L.book.setup(max_live_batches ? max_live_batches : 1024, kLgArena0);
    const size_t slots = L.book.rows.size();
    SHD_TRY(L.arena.ensure(kLgArena0 * sizeof(uint2)));
    SHD_TRY(L.rows.ensure(slots * sizeof(LedgerRow)));
    SHD_TRY(L.pops.ensure(slots * 4));
    SHD_TRY(L.words.ensure((1 + (size_t)kLgMaxBatches) * 8));
    SHD_TRY(L.pin.ensure((1 + (size_t)kLgMaxBatches) * 8));
    SHD_TRY(L.g_size.ensure(16));
    SHD_TRY(L.g_pkt.ensure(16));
    SHD_HIP(hipMemsetAsync(L.rows.p, 0xFF, slots * sizeof(LedgerRow), s));   // every slot: no batch
    SHD_HIP(hipMemsetAsync(L.pops.p, 0, slots * 4, s));
    SHD_HIP(hipStreamSynchronize(s));
    L.ready = true;
    return SHD_OK;
}

shd_status shd_ledger_record(shd_ctx* ctx, uint64_t batch, const uint32_t* d_size, const uint32_t* d_pkt,
                             uint64_t n_packets, uint64_t n_live) {
    LedgerState* Lp;
    SHD_TRY(ledger_live(ctx, &Lp));
    LedgerState& L = *Lp;
    // refused before anything runs, the ledger stays as it was
    if (n_packets && (!d_size || !d_pkt)) return SHD_ERR_INVALID;
    const int what = L.book.check_record(batch, n_packets, n_live);
    if (what < 0) return SHD_ERR_INVALID;
    L.book.last = batch;
    if (what == 1) return SHD_OK;   // no event of it will pop: nothing to keep
    SHD_HIP(hipSetDevice(ctx->device));
    uint64_t base = 0;
    if (!L.book.place(n_packets, &base)) {
        SHD_TRY(ledger_grow(ctx, L, n_packets));
        if (!L.book.place(n_packets, &base)) return SHD_ERR_NOMEM;
    }
    L.book.commit_record(batch, base, n_packets, n_live);
    const LedgerRow row = L.book.row(batch);
    ledger_record<<<div_up(n_packets, 256), 256, 0, ctx->stream>>>(d_size, d_pkt, n_packets, L.arena.as<uint2>() + base,
                                                                   L.rows.as<LedgerRow>() + (batch & L.book.mask), row);
    SHD_HIP(hipGetLastError());
    return SHD_OK;
}

shd_status shd_ledger_record_sharded(shd_ctx* ctx, uint64_t batch, const uint32_t* d_size, const uint32_t* d_pkt,
                                     const uint32_t* d_dst_host, const uint8_t* d_status, uint64_t n_packets,
                                     shd_relay_out* d_out, shd_status local) {
    if (!ctx || !d_out) return SHD_ERR_INVALID;
    if (!ctx->comm) return SHD_ERR_STATE;
    Comm& C = *ctx->comm;
    LedgerState& L = ctx->ledger;
    if (C.size == 1) {   // one rank: its own batch is what its events name
        if (local != SHD_OK) return local;
        return shd_ledger_record(ctx, batch, d_size, d_pkt, n_packets, d_out->n_sent);
    }
    const uint32_t world = (uint32_t)C.size, me = (uint32_t)C.rank;
    if (world > kLpMaxWorld) return SHD_ERR_INVALID;
    SHD_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // Whatever can differ between the ranks is this rank's status in the sizing words, never a
    // return before the collective: the peers are on their way to it.
    shd_status st = local;
    if (st == SHD_OK && (!L.ready || !ctx->relay.ready || !ctx->relay.sharded)) st = SHD_ERR_STATE;
    if (st == SHD_OK && ((n_packets && (!d_size || !d_pkt || !d_dst_host || !d_status)) || n_packets >= 0xFFFFFFFFull))
        st = SHD_ERR_INVALID;
    const uint64_t n_ev = st == SHD_OK ? d_out->n_events : 0;
    if (n_ev && (!d_out->ev_src || !d_out->ev_pkt)) st = SHD_ERR_INVALID;
    // (a rank that received nothing records nothing: its queues take no batch, the number stays free)
    if (st == SHD_OK && n_ev && L.book.check_record(batch, n_ev, n_ev) < 0) st = SHD_ERR_INVALID;
    const uint32_t n_hosts = ctx->relay.n_hosts;
    const uint32_t n_wg = (uint32_t)div_up(n_packets, kLpTile);
    // 1. both sides' buffers, sized before the collective: a rank receives exactly n_ev entries
    if (st == SHD_OK &&
        (L.x_sidx.ensure(std::max<uint64_t>(n_packets, 1) * 4) != SHD_OK ||
         L.x_sent.ensure(std::max<uint64_t>(n_packets, 1) * 8) != SHD_OK ||
         L.x_cnt.ensure(((size_t)world * n_wg + 1 + kScanV) * 4) != SHD_OK ||
         L.x_ridx.ensure(std::max<uint64_t>(n_ev, 1) * 4) != SHD_OK ||
         L.x_rent.ensure(std::max<uint64_t>(n_ev, 1) * 8) != SHD_OK || L.x_st.ensure(8) != SHD_OK))
        st = SHD_ERR_NOMEM;
    // 2. pack: counts, their rank-major scan, the scatter
    uint32_t* cnt = L.x_cnt.as<uint32_t>();
    bool packed = false;
    if (st == SHD_OK && n_packets) {
        ledger_pack_count<<<n_wg, kLpThreads, 0, s>>>(d_status, d_dst_host, n_packets, n_hosts, world, n_wg, cnt);
        if (hipGetLastError() != hipSuccess) st = SHD_ERR_HIP;
        if (st == SHD_OK) st = scan_excl2(L.x_scan, cnt, cnt, nullptr, nullptr, (uint64_t)world * n_wg + 1, s);
        if (st == SHD_OK) {
            ledger_pack_scatter<<<n_wg, kLpThreads, 0, s>>>(d_status, d_dst_host, d_size, d_pkt, n_packets, n_hosts,
                                                            world, n_wg, cnt, L.x_sidx.as<uint32_t>(),
                                                            L.x_sent.as<uint2>());
            if (hipGetLastError() != hipSuccess) st = SHD_ERR_HIP;
        }
        packed = st == SHD_OK;
    }
    // 3. sizing and status: three words per peer (comm_scratch: sized with the communicator)
    uint64_t* w_send = reinterpret_cast<uint64_t*>(ctx->comm_scratch.as<char>() + comm_ledger_words_at((int)world));
    uint64_t* w_recv = w_send + kLpWords * (size_t)world;
    ledger_words<<<div_up(world, 256), 256, 0, s>>>(packed ? cnt : nullptr, n_wg, world, (int32_t)st, n_packets,
                                                    w_send);
    if (hipGetLastError() != hipSuccess) {   // the words the peers size from must carry the failure: from the host
        if (st == SHD_OK) st = SHD_ERR_HIP;
        std::vector<uint64_t> hw(kLpWords * (size_t)world, 0);
        for (uint32_t r = 0; r < world; ++r) hw[kLpWords * r + 1] = (uint64_t)(int64_t)st;
        (void)hipMemcpy(w_send, hw.data(), hw.size() * 8, hipMemcpyHostToDevice);
    }
    SHD_TRY(C.all_to_all_u64(w_send, w_recv, kLpWords, s));   // agreed (LocalComm, HostComm) / fatal (RCCL)
    // one read-back: what this rank sends to and receives from every rank, and every rank's status.
    // (A failure of the read-back itself leaves this rank without the sizes: fatal, as an RCCL one.)
    std::vector<uint64_t> w(2 * kLpWords * (size_t)world);
    SHD_HIP(hipMemcpyAsync(w.data(), w_send, w.size() * 8, hipMemcpyDeviceToHost, s));
    SHD_HIP(hipStreamSynchronize(s));
    const uint64_t* ws = w.data();
    const uint64_t* wr = w.data() + kLpWords * (size_t)world;
    for (uint32_t q = 0; q < world; ++q) {
        const shd_status sq = q == me ? st : (shd_status)(int64_t)wr[kLpWords * q + 1];
        if (sq != SHD_OK) return sq;   // the lowest failing rank's, on every rank; no ledger has changed
    }
    // 4. the exchange: part 0 the indices, part 1 the entries.  The counts received must be the
    //    events received; a rank where they are not says so in the exchange's own status.
    uint64_t got = 0, slots = 0;   // entries received; the senders' batch entries (the inverse table's slots)
    for (uint32_t q = 0; q < world; ++q) {
        got += wr[kLpWords * q];
        slots += wr[kLpWords * q + 2];
    }
    const shd_status st_x = got == n_ev ? SHD_OK : SHD_ERR_INVALID;
    std::vector<const void*> sp(2 * (size_t)world);
    std::vector<void*> rp(2 * (size_t)world);
    std::vector<size_t> sb(2 * (size_t)world), rb(2 * (size_t)world);
    uint64_t s_at = 0, r_at = 0;
    for (uint32_t r = 0; r < world; ++r) {
        const uint64_t cs = ws[kLpWords * r], cr = st_x == SHD_OK ? wr[kLpWords * r] : 0;
        sp[2 * r] = L.x_sidx.as<uint32_t>() + s_at;
        sb[2 * r] = (size_t)cs * 4;
        sp[2 * r + 1] = L.x_sent.as<uint2>() + s_at;
        sb[2 * r + 1] = (size_t)cs * 8;
        rp[2 * r] = L.x_ridx.as<uint32_t>() + r_at;
        rb[2 * r] = (size_t)cr * 4;
        rp[2 * r + 1] = L.x_rent.as<uint2>() + r_at;
        rb[2 * r + 1] = (size_t)cr * 8;
        s_at += cs;
        r_at += cr;
    }
    SHD_TRY(C.exchange(2, sp.data(), sb.data(), rp.data(), rb.data(), s, st_x));
    // 5. record and remap: no collective follows, a failure from here on is this rank's alone
    if (n_ev == 0) return SHD_OK;
    uint64_t base = 0;
    if (!L.book.place(n_ev, &base)) {
        SHD_TRY(ledger_grow(ctx, L, n_ev));
        if (!L.book.place(n_ev, &base)) return SHD_ERR_NOMEM;
    }
    L.book.last = batch;
    L.book.commit_record(batch, base, n_ev, n_ev);
    const LedgerRow row = L.book.row(batch);
    ledger_record_ent<<<div_up(n_ev, 256), 256, 0, s>>>(L.x_rent.as<uint2>(), n_ev, L.arena.as<uint2>() + base,
                                                        L.rows.as<LedgerRow>() + (batch & L.book.mask), row);
    SHD_HIP(hipGetLastError());
    uint32_t* xst = L.x_st.as<uint32_t>();
    SHD_HIP(hipMemsetAsync(xst, 0, 8, s));
    // the inverse table (two loads per event) where it can be had, else the binary search
    if (!ctx->knobs.on(K_LEDGER_REMAP_SEARCH) && slots < 0xFFFFFFFFull &&
        L.x_inv.ensure(std::max<uint64_t>(slots, 1) * 4) == SHD_OK) {
        ledger_inv_scatter<<<div_up(n_ev, 256), 256, 0, s>>>((uint32_t)n_ev, world, w_recv, L.x_ridx.as<uint32_t>(),
                                                             L.x_inv.as<uint32_t>());
        ledger_remap_table<<<div_up(n_ev, 256), 256, 0, s>>>(d_out->ev_src, d_out->ev_pkt, (uint32_t)n_ev, n_hosts, world,
                                                             w_recv, L.x_ridx.as<uint32_t>(), L.x_inv.as<uint32_t>(),
                                                             xst);
    } else {
        ledger_remap<<<div_up(n_ev, 256), 256, 0, s>>>(d_out->ev_src, d_out->ev_pkt, (uint32_t)n_ev, n_hosts, world,
                                                       w_recv, L.x_ridx.as<uint32_t>(), xst);
    }
    SHD_HIP(hipGetLastError());
    unsigned long long* pin = L.pin.as<unsigned long long>();
    SHD_TRY(readback_into(ctx, s, xst, 8, pin));
    if ((uint32_t)pin[0]) {
        // an event names a packet its sender never sent: the batch's live count no longer says
        // what will pop -- as after a refused gather, shd_ledger_setup must run again
        L.ready = false;
        return SHD_ERR_INVALID;
    }
    return SHD_OK;
}

shd_status shd_ledger_gather(shd_ctx* ctx, const uint64_t* d_tag, uint64_t n, const uint32_t** d_size,
                             const uint32_t** d_pkt) {
    LedgerState* Lp;
    SHD_TRY(ledger_live(ctx, &Lp));
    LedgerState& L = *Lp;
    if ((n && !d_tag) || n >= 0xFFFFFFFFull) return SHD_ERR_INVALID;
    SHD_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    SHD_TRY(L.g_size.ensure((n + 4) * 4));
    SHD_TRY(L.g_pkt.ensure((n + 4) * 4));
    if (d_size) *d_size = L.g_size.as<uint32_t>();
    if (d_pkt) *d_pkt = L.g_pkt.as<uint32_t>();
    if (n == 0) return SHD_OK;
    LedgerBook& B = L.book;
    const uint64_t oldest = B.oldest == kLedgerNone ? 0 : B.oldest;
    const uint32_t span = (uint32_t)B.span();
    unsigned long long* words = L.words.as<unsigned long long>();
    SHD_HIP(hipMemsetAsync(words, 0, 8, s));
    ledger_gather<<<div_up(n, kLgTile), kLgThreads, 0, s>>>(
        d_tag, n, ((uintptr_t)d_tag & 15) == 0 ? 1 : 0, L.rows.as<LedgerRow>(), B.mask, oldest, span, L.arena.as<uint2>(),
        B.cap, L.pops.as<uint32_t>(), L.g_size.as<uint32_t>(), L.g_pkt.as<uint32_t>(), reinterpret_cast<uint32_t*>(words));
    SHD_HIP(hipGetLastError());
    if (span) {
        ledger_settle<<<div_up(span, 256), 256, 0, s>>>(L.rows.as<LedgerRow>(), B.mask, oldest, span, L.pops.as<uint32_t>(),
                                                        words);
        SHD_HIP(hipGetLastError());
    }
    // the status word and every held batch's live count in one read
    unsigned long long* w = L.pin.as<unsigned long long>();
    SHD_TRY(readback_into(ctx, s, words, (1 + (size_t)span) * 8, w));
    if ((uint32_t)w[0]) {
        // the good events' pops are counted, the refused ones' are not: the counts no longer say
        // what is pending -- shd_ledger_setup must run again
        L.ready = false;
        return SHD_ERR_INVALID;
    }
    for (uint32_t i = 0; i < span; ++i)
        if (w[1 + i] != ~0ull && B.holds(oldest + i)) B.set_live(oldest + i, (uint32_t)w[1 + i]);
    B.reclaim();
    return SHD_OK;
}

shd_status shd_ledger_stats(shd_ctx* ctx, uint64_t* live_batches, uint64_t* live_events, uint64_t* entries_held,
                            uint64_t* oldest_batch) {
    LedgerState* Lp;
    SHD_TRY(ledger_live(ctx, &Lp));
    const LedgerBook& B = Lp->book;
    if (live_batches) *live_batches = B.live_batches;
    if (live_events) *live_events = B.live_events;
    if (entries_held) *entries_held = B.entries_held;
    if (oldest_batch) *oldest_batch = B.oldest;
    return SHD_OK;
}

}  // extern "C"
