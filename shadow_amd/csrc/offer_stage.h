// The staged offer record of shd_offers_group (offers.hip) and the host-side check of the stages'
// shape.  No HIP type in here: tests/offer_stage_main.cpp compiles this header alone, with the
// address and undefined-behaviour sanitizers, and tests/test_offers.py runs it against the numpy
// group-by; the kernels read records through the same constants and the same decode.
//
// A stage is one worker thread's buffer at the round barrier: runs (host, count) and, run after
// run, the hosts' offers in the order each host made them -- `offer_words` u32 words per offer:
//   0 time_off (now - time_base)   1 dst (global HostId)   2 size (total)   3 payload   4 pkt
//   5 reserved   6, 7 the d_prio key, low then high   8, 9 d_sock, low then high (width 10 only)
#pragma once
#include <stdint.h>

#if defined(__HIP__)   // a HIP unit: the kernels decode with the same function
#define SHD_OFFER_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define SHD_OFFER_HD inline
#endif

namespace shd {

constexpr uint32_t kOfferTime = 0, kOfferDst = 1, kOfferSize = 2, kOfferPayload = 3, kOfferPkt = 4, kOfferPrio = 6,
                   kOfferSock = 8;
constexpr uint32_t kOfferWords = 8, kOfferWordsSock = 10;   // the two record widths

struct Offer {   // one record, decoded: the outbound stage's columns
    uint64_t time, prio, sock;
    uint32_t size, payload, dst, pkt;
};

// w: the record's words (`words` of them; sock is 0 at width 8)
SHD_OFFER_HD Offer offer_decode(const uint32_t* w, uint32_t words, uint64_t time_base) {
    Offer o;
    o.time = time_base + w[kOfferTime];
    o.prio = (uint64_t)w[kOfferPrio] | ((uint64_t)w[kOfferPrio + 1] << 32);
    o.sock = words == kOfferWordsSock ? (uint64_t)w[kOfferSock] | ((uint64_t)w[kOfferSock + 1] << 32) : 0;
    o.size = w[kOfferSize];
    o.payload = w[kOfferPayload];
    o.dst = w[kOfferDst];
    o.pkt = w[kOfferPkt];
    return o;
}

// The stages' shape, checked on the host before anything is uploaded: a width the discipline takes
// (need_sock: one of the two socket disciplines, which have no 8-word form), no NULL array where a
// count is not zero, every stage's run counts adding up to its stage_offers, fewer than 2^32 runs
// and offers in all.  Reads the run counts only; false: refused, the totals are not written.
inline bool offer_stages_ok(uint32_t n_stages, const uint32_t* stage_runs, const uint32_t* const* run_host,
                            const uint32_t* const* run_count, const uint64_t* stage_offers,
                            const uint32_t* const* offers, uint32_t offer_words, bool need_sock, uint64_t* n_runs,
                            uint64_t* n_offers) {
    if (offer_words != kOfferWords && offer_words != kOfferWordsSock) return false;
    if (need_sock && offer_words != kOfferWordsSock) return false;
    if (n_stages && (!stage_runs || !run_host || !run_count || !stage_offers || !offers)) return false;
    uint64_t nr = 0, no = 0;
    for (uint32_t k = 0; k < n_stages; ++k) {   // the totals first: no array is read for a call too large
        if (stage_offers[k] >= (1ull << 32)) return false;
        nr += stage_runs[k];
        no += stage_offers[k];
        if (nr >= (1ull << 32) || no >= (1ull << 32)) return false;
    }
    for (uint32_t k = 0; k < n_stages; ++k) {
        if (stage_runs[k] && (!run_host[k] || !run_count[k])) return false;
        if (stage_offers[k] && !offers[k]) return false;
        uint64_t c = 0;
        for (uint32_t r = 0; r < stage_runs[k]; ++r) c += run_count[k][r];
        if (c != stage_offers[k]) return false;
    }
    if (n_runs) *n_runs = nr;
    if (n_offers) *n_offers = no;
    return true;
}

}  // namespace shd
