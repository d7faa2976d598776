// The staged offer record of shd_offers_group (offers.hip) and the host-side check of its
// arguments (the stages' shape is stage_shape.h's).  No HIP type in here:
// tests/offer_stage_main.cpp compiles this header alone, with the address and undefined-behaviour
// sanitizers, and tests/test_offers.py runs it against the numpy group-by; the kernels read
// records through the same constants and the same decode.
//
// A stage is one worker thread's buffer at the round barrier: runs (host, count) and, run after
// run, the hosts' offers in the order each host made them -- `offer_words` u32 words per offer:
//   0 time_off (now - time_base)   1 dst (global HostId)   2 size (total)   3 payload   4 pkt
//   5 reserved   6, 7 the d_prio key, low then high   8, 9 d_sock, low then high (width 10 only)
#pragma once
#include <stdint.h>

#include <vector>

#include "stage_shape.h"

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

// The stages as stage_shape.h's neutral views (what the shared check and stage_group take); the
// five tables hold n_stages entries each.
inline std::vector<StageView> offer_stage_views(uint32_t n_stages, const uint32_t* stage_runs,
                                                const uint32_t* const* run_host, const uint32_t* const* run_count,
                                                const uint64_t* stage_offers, const uint32_t* const* offers) {
    std::vector<StageView> v(n_stages);
    for (uint32_t k = 0; k < n_stages; ++k)
        v[k] = StageView{stage_runs[k], run_host[k], run_count[k], stage_offers[k], offers[k]};
    return v;
}

// A width the discipline takes (need_sock: one of the two socket disciplines, which have no 8-word
// form), the five tables present, and the stages' shape (stages_ok).  false: refused, the totals
// are not written.
inline bool offer_stages_ok(uint32_t n_stages, const uint32_t* stage_runs, const uint32_t* const* run_host,
                            const uint32_t* const* run_count, const uint64_t* stage_offers,
                            const uint32_t* const* offers, uint32_t offer_words, bool need_sock, uint64_t* n_runs,
                            uint64_t* n_offers) {
    if (offer_words != kOfferWords && offer_words != kOfferWordsSock) return false;
    if (need_sock && offer_words != kOfferWordsSock) return false;
    if (n_stages && (!stage_runs || !run_host || !run_count || !stage_offers || !offers)) return false;
    return stages_ok(offer_stage_views(n_stages, stage_runs, run_host, run_count, stage_offers, offers).data(), n_stages,
                     n_runs, n_offers);
}

}  // namespace shd
