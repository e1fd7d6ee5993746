// The running-peak fold of a single-pass Normalize tile (termdaw_amd/csrc/sum_runmax.h, shared with k_sum16w) on the CPU, under
// AddressSanitizer / UBSan (tests/test_sum_runmax_host.py).  A timeline of T tiles of NB blocks (NB = 1, 2, 4), seeded block peaks
// (drawn from a few values, so that ties are the rule; zero peaks; a record in the first block, in the last, nowhere) and a carried
// max below, among and above them; every tile folds twice as the kernel does -- from a random subset of the lower tiles' peaks
// ("seen": none, all, any), and from all of them:
//   - the second fold is the plain prefix maximum `max_b = peak_b.max(max_{b-1})` over the whole timeline, block for block;
//   - the value leaving the last tile is the maximum of everything;
//   - redo_mask raises bit b exactly where the first fold's running peak of block b is another float than the prefix maximum;
//   - with every lower tile seen nothing is raised, and a first fold never exceeds the second.
// usage: asan_sum_runmax [timelines per shape]
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "sum_runmax.h"

#define CHECK(c)                                                                                                 \
    do {                                                                                                         \
        if (!(c)) {                                                                                              \
            fprintf(stderr, "sum_runmax: %s fails at NB=%d case=%d tile=%u (line %d)\n", #c, NB, cs, t, __LINE__); \
            return 1;                                                                                            \
        }                                                                                                        \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // xorshift64*: seeded, the same cases on every run
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

template <int NB>
static int run_shape(int cases, unsigned long long* tiles, unsigned long long* redone) {
    for (int cs = 0; cs < cases; ++cs) {
        uint32_t t = 0;
        const uint32_t T = 1u + rnd() % 40u;
        const uint32_t levels = 1u + rnd() % 6u;   // few distinct values: ties
        std::vector<float> peak((size_t)T * NB);
        for (float& p : peak) p = (rnd() % 4u == 0u) ? 0.0f : 0.25f * (float)(rnd() % levels);
        switch (cs % 5) {
            case 1: peak.front() = 1000.0f; break;                                                  // block 0 is the record
            case 2: peak.back() = 1000.0f; break;                                                   // the last block is
            case 3: for (size_t i = 0; i < peak.size(); ++i) peak[i] = 1.0f + (float)i; break;      // every block a new record
            case 4: for (float& p : peak) p = 0.0f; break;                                          // silence
            default: break;
        }
        const float carried_of[5] = {0.0f, 0.5f, 0.25f * (float)levels, 2000.0f, 0.25f * (float)(rnd() % levels)};
        const float carried = carried_of[(cs / 5) % 5];
        // the plain prefix maximum over the whole timeline
        std::vector<float> want(peak.size());
        float mx = carried;
        for (size_t i = 0; i < peak.size(); ++i) {
            if (peak[i] > mx) mx = peak[i];
            want[i] = mx;
        }
        std::vector<float> tile_peak(T);
        for (t = 0; t < T; ++t) {
            float m = 0.0f;
            for (int b = 0; b < NB; ++b) m = tdrm::fmax2(m, peak[(size_t)t * NB + b]);
            tile_peak[t] = m;
        }
        const uint32_t seen_mode = rnd() % 4u;   // 0: nothing, 1: everything, 2 / 3: any subset
        float leaving = carried;
        for (t = 0; t < T; ++t) {
            float pb[NB], run_spec[NB], run_final[NB];
            for (int b = 0; b < NB; ++b) pb[b] = peak[(size_t)t * NB + b];
            float lower_seen = 0.0f, lower_all = 0.0f;
            bool all_seen = true;
            for (uint32_t u = 0; u < t; ++u) {
                const bool seen = seen_mode == 1u || (seen_mode >= 2u && (rnd() & 1u));
                if (seen) lower_seen = tdrm::fmax2(lower_seen, tile_peak[u]);
                else all_seen = false;
                lower_all = tdrm::fmax2(lower_all, tile_peak[u]);
            }
            tdrm::fold<NB>(tdrm::entering(carried, lower_seen), pb, run_spec);
            leaving = tdrm::fold<NB>(tdrm::entering(carried, lower_all), pb, run_final);
            const uint32_t mask = tdrm::redo_mask<NB>(run_spec, run_final);
            CHECK(mask < (1u << NB));
            for (int b = 0; b < NB; ++b) {
                const float w = want[(size_t)t * NB + b];
                CHECK(run_final[b] == w);
                CHECK(run_spec[b] <= run_final[b]);
                CHECK((((mask >> b) & 1u) != 0u) == (run_spec[b] != w));
                CHECK(tdrm::differs(run_spec[b], run_final[b]) == (run_spec[b] != w));
                *redone += (mask >> b) & 1u;
            }
            if (all_seen) CHECK(mask == 0u);
            if (cs % 5 == 3 && carried <= 1.0f) CHECK(mask == 0u);   // (a block's own peak is its running peak)
            ++*tiles;
        }
        t = T - 1u;
        CHECK(leaving == mx);
    }
    return 0;
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 20000;
    unsigned long long tiles = 0, redone = 0;
    if (run_shape<1>(cases, &tiles, &redone) || run_shape<2>(cases, &tiles, &redone) || run_shape<4>(cases, &tiles, &redone)) return 1;
    printf("asan_sum_runmax done: %d timelines per shape, %llu tiles, %llu blocks to redo\n", cases, tiles, redone);
    return 0;
}
