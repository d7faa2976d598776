// Drives shadow_amd/csrc/offer_stage.h from a script on stdin: tests/test_offers.py builds this with
// the address and undefined-behaviour sanitizers and holds its answers against the numpy group-by
// (shadow_amd.outbound.group_offers).  Every array is allocated at exactly its stated length, so a
// read past a stage's runs or records is the sanitizer's to find.
//
//   group <words> <need_sock 0|1> <time_base> <first_host> <n_hosts> <n_stages> <no_tables 0|1>
//     then per stage: <n_runs> <n_offers> <null mask: 1 run_host, 2 run_count, 4 offers>,
//                     n_runs pairs <host> <count>, n_offers * words record words
//   -> "refused" (offer_stages_ok) | "nohost" | "dup" |
//      "ok <n_runs> <n_offers>" and eight lines: off, time, prio, sock, size, payload, dst, pkt
//      (the host's walk of what the kernels do: run -> host, counts -> offsets, offer_decode per record)
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "offer_stage.h"

int main() {
    std::string op;
    while (std::cin >> op) {
        if (op != "group") {
            std::printf("unknown op %s\n", op.c_str());
            return 2;
        }
        uint32_t words, need_sock, first_host, n_hosts, n_stages, no_tables;
        uint64_t time_base;
        std::cin >> words >> need_sock >> time_base >> first_host >> n_hosts >> n_stages >> no_tables;
        std::vector<uint32_t*> rh(n_stages), rc(n_stages), rec(n_stages);
        std::vector<uint32_t> stage_runs(n_stages);
        std::vector<uint64_t> stage_offers(n_stages);
        std::vector<const uint32_t*> p_rh(n_stages), p_rc(n_stages), p_rec(n_stages);
        const uint32_t w_rec = words ? words : 1;
        for (uint32_t k = 0; k < n_stages; ++k) {
            uint32_t mask;
            std::cin >> stage_runs[k] >> stage_offers[k] >> mask;
            rh[k] = new uint32_t[stage_runs[k]];
            rc[k] = new uint32_t[stage_runs[k]];
            rec[k] = new uint32_t[stage_offers[k] * w_rec];
            for (uint32_t r = 0; r < stage_runs[k]; ++r) std::cin >> rh[k][r] >> rc[k][r];
            for (uint64_t i = 0; i < stage_offers[k] * w_rec; ++i) std::cin >> rec[k][i];
            p_rh[k] = mask & 1 ? nullptr : rh[k];
            p_rc[k] = mask & 2 ? nullptr : rc[k];
            p_rec[k] = mask & 4 ? nullptr : rec[k];
        }
        uint64_t n_runs = 0, n = 0;
        const bool ok = shd::offer_stages_ok(n_stages, no_tables ? nullptr : stage_runs.data(), p_rh.data(), p_rc.data(),
                                             stage_offers.data(), p_rec.data(), words, need_sock != 0, &n_runs, &n);
        const char* verdict = ok ? nullptr : "refused";
        // run -> host, as of_runs; then counts -> offsets, and the records through offer_decode
        std::vector<int64_t> run_of(n_hosts, -1), st_of(n_hosts, -1);
        std::vector<uint64_t> first_of(n_hosts, 0);
        std::vector<uint32_t> off(n_hosts + 1, 0);
        if (ok) {
            bool nohost = false, dup = false;
            for (uint32_t k = 0; k < n_stages; ++k) {
                uint64_t at = 0;
                for (uint32_t r = 0; r < stage_runs[k]; ++r) {
                    const uint32_t host = p_rh[k][r];
                    if (host < first_host || host - first_host >= n_hosts) {
                        nohost = true;
                    } else {
                        const uint32_t h = host - first_host;
                        if (run_of[h] >= 0) dup = true;
                        run_of[h] = r;
                        st_of[h] = k;
                        first_of[h] = at;
                        off[h + 1] = p_rc[k][r];
                    }
                    at += p_rc[k][r];
                }
            }
            verdict = nohost ? "nohost" : dup ? "dup" : nullptr;
        }
        if (verdict) {
            std::puts(verdict);
        } else {
            for (uint32_t h = 0; h < n_hosts; ++h) off[h + 1] += off[h];
            std::vector<shd::Offer> g(n);
            for (uint32_t h = 0; h < n_hosts; ++h)
                for (uint32_t i = 0; i < off[h + 1] - off[h]; ++i)
                    g[off[h] + i] = shd::offer_decode(p_rec[st_of[h]] + (first_of[h] + i) * words, words, time_base);
            std::printf("ok %llu %llu\n", (unsigned long long)n_runs, (unsigned long long)n);
            for (uint32_t h = 0; h <= n_hosts; ++h) std::printf("%u ", off[h]);
            std::puts("");
            auto line = [&](auto get) {
                for (const shd::Offer& o : g) std::printf("%llu ", (unsigned long long)get(o));
                std::puts("");
            };
            line([](const shd::Offer& o) { return o.time; });
            line([](const shd::Offer& o) { return o.prio; });
            line([](const shd::Offer& o) { return o.sock; });
            line([](const shd::Offer& o) { return (uint64_t)o.size; });
            line([](const shd::Offer& o) { return (uint64_t)o.payload; });
            line([](const shd::Offer& o) { return (uint64_t)o.dst; });
            line([](const shd::Offer& o) { return (uint64_t)o.pkt; });
        }
        for (uint32_t k = 0; k < n_stages; ++k) {
            delete[] rh[k];
            delete[] rc[k];
            delete[] rec[k];
        }
    }
    return 0;
}
