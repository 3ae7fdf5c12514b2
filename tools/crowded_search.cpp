// tools/crowded_search.cpp -- how many wall candidates can ONE 9x9 position leave to search?
// The wavefront of legal_wave.hpp has 64 task lanes; the interleaved layout runs a second round beyond 64 candidates.  This program
// anneals over wall sets (add / remove a wall) for the largest number of candidates that are placeable and kept by the touch-count
// prefilter, using the rule header itself.  Every run so far ends at 63 -- with walls added under the placement rules and, with the
// argument "free", with any wall set a record can hold -- which is where tests/witness_cases.most_crowded() comes from.
//   g++ -O2 -std=c++17 -Wno-unknown-pragmas -o /tmp/crowded_search tools/crowded_search.cpp && /tmp/crowded_search [seed] [free]
#include "../alphaquoridorgnn_amd/csrc/quoridor_core.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
using namespace aqg;
constexpr int N = 9;

static int candidates(uint64_t hw, uint64_t vw) {
    uint64_t hp, vp, hb, vb;
    placeable_masks<N>(hw, vw, hp, vp);
    possibly_blocking_masks<N>(hw, vw, hb, vb);
    return __builtin_popcountll(hp & hb) + __builtin_popcountll(vp & vb);
}

int main(int argc, char** argv) {
    std::mt19937_64 rng(argc > 1 ? atoi(argv[1]) : 1);
    const bool any_layout = argc > 2 && !strcmp(argv[2], "free");
    const int restarts = 20;
    uint64_t bh = 0, bv = 0;
    int best = 0;
    for (int r = 0; r < restarts; ++r) {
        uint64_t hw = 0, vw = 0;
        int cur = 0;
        double T = 2.0;
        for (long it = 0; it < 3000000; ++it, T = std::max(0.25, T * 0.9999985)) {
            uint64_t h = hw, v = vw;
            const uint64_t b = 1ull << (rng() % 64);
            if ((h | v) & b) { h &= ~b; v &= ~b; }
            else {
                uint64_t hp, vp;
                placeable_masks<N>(h, v, hp, vp);
                if (rng() & 1) { if (!any_layout && !(hp & b)) continue; h |= b; }
                else { if (!any_layout && !(vp & b)) continue; v |= b; }
            }
            const int n = candidates(h, v);
            if (n >= cur || std::exp((n - cur) / T) * 4294967296.0 > (double)(rng() & 0xffffffffu)) {
                hw = h; vw = v; cur = n;
                if (cur > best) { best = cur; bh = hw; bv = vw; }
            }
        }
        fprintf(stderr, "restart %d: best so far %d\n", r, best);
    }
    printf("most candidates %d with hw = 0x%llx, vw = 0x%llx (%d walls)\n", best, (unsigned long long)bh, (unsigned long long)bv,
           __builtin_popcountll(bh | bv));
    return 0;
}
