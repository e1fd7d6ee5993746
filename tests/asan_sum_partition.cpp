// The quad-granular partition of the ragged packed sum (termdaw_amd/csrc/sum_partition.h) on the CPU, under AddressSanitizer /
// UBSan (tests/test_sum_partition_host.py): for every timeline of Q quads and every grid of G workgroups that groups_ok() admits
//   - the workgroups' ranges tile [0, Q) exactly, in order;
//   - workgroup sizes differ by at most 1 and lie in 4 .. 16; the waves' ranges tile the workgroup's, their sizes differ by at
//     most 1 and lie in 1 .. 4;
//   - a reference block (4 quads) lies in at most two workgroups, and tail_straddles() says exactly when a workgroup's last
//     block continues in the next one.
// usage: asan_sum_partition [Q_lo Q_hi]
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

#include "sum_partition.h"

#define CHECK(c)                                                                                     \
    do {                                                                                             \
        if (!(c)) {                                                                                  \
            fprintf(stderr, "sum_partition: %s fails at Q=%u G=%u g=%u (line %d)\n", #c, Q, G, g, __LINE__); \
            return 1;                                                                                \
        }                                                                                            \
    } while (0)

int main(int argc, char** argv) {
    using namespace tdsp;
    const uint32_t q_lo = argc > 2 ? (uint32_t)atoi(argv[1]) : 16u, q_hi = argc > 2 ? (uint32_t)atoi(argv[2]) : 20000u;
    unsigned long long grids = 0, groups = 0, straddles = 0;
    std::vector<uint32_t> owners_of_block;
    for (uint32_t Q = q_lo; Q <= q_hi; ++Q) {
        // every admissible G for small timelines; for long ones the two ends of the admissible range, the grids that fill a
        // device of 256 CUs (2 .. 6 workgroups per CU) and a few in between
        const uint32_t g_min = (Q + kMaxQuads - 1u) / kMaxQuads, g_max = Q / kMinQuads;
        const uint32_t stride = Q <= 600u ? 1u : 1u + (g_max - g_min) / 3u;
        std::vector<uint32_t> Gs;
        for (uint32_t G = g_min; G <= g_max; G += stride) Gs.push_back(G);
        for (uint32_t G : {g_min, g_min + 1u, g_max - 1u, g_max, 512u, 768u, 1024u, 1280u, 1536u}) Gs.push_back(G);
        std::sort(Gs.begin(), Gs.end());
        Gs.erase(std::unique(Gs.begin(), Gs.end()), Gs.end());
        {   // the frame count behind Q, and the two ends just outside the range
            uint32_t G = 0, g = 0;
            CHECK(quads_of(Q * kQuadFrames) == Q && quads_of(Q * kQuadFrames - 255u) == Q && quads_of(Q * kQuadFrames + 1u) == Q + 1u);
            CHECK(!groups_ok(Q, 0u) && !groups_ok(Q, g_max + 1u));
            if (g_min > 1u) CHECK(!groups_ok(Q, g_min - 1u));
        }
        for (uint32_t G : Gs) {
            uint32_t g = 0;
            if (!groups_ok(Q, G)) {
                CHECK(G < g_min || G > g_max);
                continue;
            }
            CHECK(G >= g_min && G <= g_max);
            ++grids;
            const uint32_t n_blocks = (Q + kQuadsPerBlock - 1u) / kQuadsPerBlock;
            owners_of_block.assign(n_blocks, 0u);
            uint32_t next = 0, n_lo = ~0u, n_hi = 0;
            for (g = 0; g < G; ++g) {
                const QuadRange wg = group_quads(g, G, Q);
                CHECK(wg.q0 == next);
                CHECK(wg.n >= kMinQuads && wg.n <= kMaxQuads);
                n_lo = wg.n < n_lo ? wg.n : n_lo;
                n_hi = wg.n > n_hi ? wg.n : n_hi;
                uint32_t wnext = wg.q0, w_lo = ~0u, w_hi = 0;
                for (uint32_t w = 0; w < kWaves; ++w) {
                    const QuadRange wv = wave_quads(wg, w);
                    CHECK(wv.q0 == wnext);
                    CHECK(wv.n >= 1u && wv.n <= 4u);
                    w_lo = wv.n < w_lo ? wv.n : w_lo;
                    w_hi = wv.n > w_hi ? wv.n : w_hi;
                    wnext = wv.q0 + wv.n;
                }
                CHECK(wnext == wg.q0 + wg.n);
                CHECK(w_hi - w_lo <= 1u);
                next = wg.q0 + wg.n;
                const uint32_t b0 = wg.q0 / kQuadsPerBlock, b1 = (next - 1u) / kQuadsPerBlock;
                CHECK(b1 < n_blocks && b1 - b0 <= 4u);   // (at most five blocks: what the kernel's peak stores assume)
                for (uint32_t b = b0; b <= b1; ++b) ++owners_of_block[b];
                // the last block continues in g + 1 exactly when g + 1 exists and starts inside it
                const bool cont = g + 1u < G && group_quads(g + 1u, G, Q).q0 / kQuadsPerBlock == b1 && group_quads(g + 1u, G, Q).q0 % kQuadsPerBlock != 0u;
                CHECK(tail_straddles(wg, Q) == cont);
                straddles += cont ? 1u : 0u;
                ++groups;
            }
            g = G;
            CHECK(next == Q);
            CHECK(n_hi - n_lo <= 1u);
            for (uint32_t b = 0; b < n_blocks; ++b) {
                g = b;   // (reported as the block)
                CHECK(owners_of_block[b] >= 1u && owners_of_block[b] <= 2u);
            }
        }
    }
    printf("asan_sum_partition done: %llu grids, %llu workgroups, %llu straddled blocks\n", grids, groups, straddles);
    return 0;
}
