// The wave's index into a looping source's packed table (termdaw_amd/csrc/sum_index.h) on the CPU, under AddressSanitizer /
// UBSan (tests/test_sum_index_host.py): for every loop length 1 .. 1 100 and a few thousand seeded ones up to 2^26, over
// values of t0 + wave_base from the whole 32-bit range (the top 1 024 among them)
//   - wave_start is x mod len, quad_step is 256 mod len, and four next_quad steps are (x + 256 q) mod len, against plain %;
//   - every lane of every quad reads inside the table: start + 255 < len + pad, and the table holds at least len + pad words,
//     a multiple of four;
//   - read out of a table built like k_sample_pack16 builds it (word i = frame i mod len), the 256 words of a quad ARE the
//     frames (x + 256 q + i) mod len.
// usage: asan_sum_index [len_lo len_hi]
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "sum_index.h"

#define CHECK(c)                                                                                            \
    do {                                                                                                    \
        if (!(c)) {                                                                                         \
            fprintf(stderr, "sum_index: %s fails at len=%u x=%u q=%d (line %d)\n", #c, len, x, q, __LINE__); \
            return 1;                                                                                       \
        }                                                                                                   \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // xorshift64*: seeded, the same cases on every run
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static int check_len(uint32_t len, bool tables, unsigned long long* cases) {
    using namespace tdsi;
    uint32_t x = 0;
    int q = 0;
    const uint32_t magic = len >= 2u ? (uint32_t)(0x100000000ull / len) : 0xFFFFFFFFu;   // (compile.cpp's)
    const uint32_t words = packed_words(len);
    CHECK(words % 4u == 0u && words >= len + kWavePad && words < len + kWavePad + 4u);
    const uint32_t step = quad_step(len, magic);
    CHECK(step == kQuadFrames % len);
    std::vector<uint32_t> table;
    if (tables) {
        table.resize(words);
        for (uint32_t i = 0; i < words; ++i) table[i] = i % len;
    }
    std::vector<uint32_t> xs;
    for (uint32_t i = 0; i < 1024u; ++i) xs.push_back(0xFFFFFFFFu - i);   // the top 1 024
    for (uint32_t i = 0; i < 64u; ++i) { xs.push_back(i); xs.push_back(len - 1u + i); xs.push_back(0x80000000u - 32u + i); }
    for (uint32_t k = 1; k <= 16u; ++k) { xs.push_back(k * len); xs.push_back(k * len - 1u); }   // (wraps mod 2^32 for long loops: any x is valid)
    for (uint32_t i = 0; i < 256u; ++i) xs.push_back(rnd());
    for (uint32_t i = 0; i < 64u; ++i) xs.push_back(rnd() & ~1023u);   // wave bases are multiples of 256
    for (uint32_t xv : xs) {
        x = xv;
        uint32_t i = wave_start(x, len, magic);
        for (q = 0; q <= 4; ++q) {
            CHECK(i == (uint32_t)(((uint64_t)x + 256ull * (uint64_t)q) % len));
            CHECK(i < len && (uint64_t)i + 255ull < (uint64_t)len + kWavePad && (uint64_t)i + 255ull < words);   // lane 63's last word
            if (tables)
                for (uint32_t l = 0; l < 64u; ++l)
                    for (uint32_t f = 0; f < 4u; ++f)
                        CHECK(table[i + 4u * l + f] == (uint32_t)(((uint64_t)x + 256ull * (uint64_t)q + 4u * l + f) % len));
            i = next_quad(i, step, len);
        }
        ++*cases;
    }
    return 0;
}

int main(int argc, char** argv) {
    const uint32_t lo = argc > 2 ? (uint32_t)atoi(argv[1]) : 1u, hi = argc > 2 ? (uint32_t)atoi(argv[2]) : 1100u;
    unsigned long long cases = 0, lens = 0;
    for (uint32_t len = lo; len <= hi; ++len, ++lens)
        if (check_len(len, true, &cases)) return 1;
    if (argc <= 2) {
        // seeded larger ones up to 2^26 (all magnitudes: a random width first), the powers of two and their neighbours
        for (int i = 0; i < 3000; ++i, ++lens) {
            const uint32_t bits = 11u + rnd() % 16u;   // 11 .. 26
            uint32_t len = (rnd() & ((1u << bits) - 1u)) | (1u << (bits - 1u));
            if (check_len(len, i % 100 == 0, &cases)) return 1;
        }
        for (uint32_t b = 11; b <= 26; ++b)
            for (int d = -1; d <= 1; ++d, ++lens)
                if (check_len((1u << b) + (uint32_t)d, false, &cases)) return 1;
    }
    printf("asan_sum_index done: %llu lengths, %llu starts\n", lens, cases);
    return 0;
}
