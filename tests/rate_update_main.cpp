// Stand-alone driver of shadow_amd/csrc/rate_update.h for tests/test_rate_update.py: built with the
// address and undefined-behaviour sanitizers and run as a program of its own.  Commands on stdin:
//   stage H prev_end                      the stage the next calls name: H hosts, its last window_end
//   update n mask at / n hosts / n capacities / n increments / n intervals
//       mask: 1, 2, 4, 8 pass the host, capacity, increment, interval array as NULL
//       -> "refused", or "ok k" and k lines "host capacity increment interval", in record order
//   bandwidth bytes_per_s                 -> "capacity increment interval" (create_token_bucket)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rate_update.h"

using namespace shd;

template <class T>
static bool read_n(std::vector<T>& v, uint64_t n) {
    v.resize(n);
    for (uint64_t i = 0; i < n; ++i) {
        unsigned long long x = 0;
        if (std::scanf("%llu", &x) != 1) return false;
        v[i] = (T)x;
    }
    return true;
}

int main() {
    RateStamps S;
    uint32_t n_hosts = 0;
    uint64_t prev_end = 0;
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "stage")) {
            unsigned long long pe = 0;
            if (std::scanf("%u %llu", &n_hosts, &pe) != 2) return 2;
            prev_end = pe;
        } else if (!std::strcmp(cmd, "update")) {
            unsigned long long n = 0, at = 0;
            unsigned mask = 0;
            if (std::scanf("%llu %u %llu", &n, &mask, &at) != 3) return 2;
            std::vector<uint32_t> host;
            std::vector<uint64_t> cap, inc, itv;
            if (!read_n(host, n) || !read_n(cap, n) || !read_n(inc, n) || !read_n(itv, n)) return 2;
            const uint32_t* ph = (mask & 1) ? nullptr : host.data();
            const uint64_t* pc = (mask & 2) ? nullptr : cap.data();
            const uint64_t* pi = (mask & 4) ? nullptr : inc.data();
            const uint64_t* pn = (mask & 8) ? nullptr : itv.data();
            if (!rate_updates_valid(n, n_hosts, ph, pc, pi, pn, at, prev_end)) {
                std::printf("refused\n");
                continue;
            }
            const std::vector<RateRec> rec = rate_updates_records(S, n_hosts, n, ph, pc, pi, pn);
            std::printf("ok %zu\n", rec.size());
            for (const RateRec& r : rec)
                std::printf("%u %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", r.host, r.capacity, r.increment, r.interval);
        } else if (!std::strcmp(cmd, "bandwidth")) {
            unsigned long long b = 0;
            if (std::scanf("%llu", &b) != 1) return 2;
            uint64_t c, i, n;
            rate_from_bandwidth(b, c, i, n);
            std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", c, i, n);
        } else {
            return 2;
        }
    }
    return 0;
}
