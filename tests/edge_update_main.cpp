// Stand-alone driver of shadow_amd/csrc/edge_update.h for tests/test_edge_update.py: built with the
// address and undefined-behaviour sanitizers and run as a program of its own.  Commands on stdin:
//   map V E directed / E sources / E destinations
//       -> "ok A" / the V + 1 offsets / the E forward slots / the E reverse slots
//   copy V / V new ids (pi)              -> the V first slots of the relabelled copy (last map)
//   update n mask / n indices / n latencies / n loss bit patterns
//       mask: 1, 2, 4 pass the index, latency, loss array as NULL; against the last map
//       -> "refused", or "ok k" / the k kept positions, last to first
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "edge_update.h"

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

static void print_u32(const std::vector<uint32_t>& v) {
    for (size_t i = 0; i < v.size(); ++i) std::printf(i ? " %u" : "%u", v[i]);
    std::printf("\n");
}

int main() {
    EdgeSlots M;
    uint64_t n_edges = 0;
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "map")) {
            unsigned V = 0, directed = 0;
            unsigned long long E = 0;
            if (std::scanf("%u %llu %u", &V, &E, &directed) != 3) return 2;
            std::vector<uint32_t> es, ed;
            if (!read_n(es, E) || !read_n(ed, E)) return 2;
            edge_slots_build(V, E, es.data(), ed.data(), directed != 0, M);
            n_edges = E;
            std::printf("ok %u\n", M.off[V]);
            print_u32(M.off);
            print_u32(M.fwd);
            print_u32(M.rev);
        } else if (!std::strcmp(cmd, "copy")) {
            unsigned V = 0;
            if (std::scanf("%u", &V) != 1) return 2;
            std::vector<uint32_t> pi;
            if (!read_n(pi, V)) return 2;
            print_u32(edge_copy_starts(M.off, pi));
        } else if (!std::strcmp(cmd, "update")) {
            unsigned long long n = 0;
            unsigned mask = 0;
            if (std::scanf("%llu %u", &n, &mask) != 2) return 2;
            std::vector<uint32_t> idx, bits;
            std::vector<uint64_t> lat;
            if (!read_n(idx, n) || !read_n(lat, n) || !read_n(bits, n)) return 2;
            std::vector<float> loss(n);
            if (n) std::memcpy(loss.data(), bits.data(), n * 4);
            const uint32_t* pi = (mask & 1) ? nullptr : idx.data();
            const uint64_t* pl = (mask & 2) ? nullptr : lat.data();
            const float* pp = (mask & 4) ? nullptr : loss.data();
            if (!edge_updates_valid(n, n_edges, pi, pl, pp)) {
                std::printf("refused\n");
                continue;
            }
            const std::vector<uint64_t> keep = edge_updates_unique(M, n, pi);
            std::printf("ok %zu\n", keep.size());
            for (size_t i = 0; i < keep.size(); ++i) std::printf(i ? " %" PRIu64 : "%" PRIu64, keep[i]);
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
