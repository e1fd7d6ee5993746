// Where a WAVE of the wide packed sum (sum_terms16w's quad shape, kernels.hip) starts reading a looping source, shared by the
// device code, the sample loader (engine.cpp: the size of a packed table) and a stand-alone CPU test (tests/asan_sum_index.cpp).
// A quad is 256 frames, lane l words 4 l .. 4 l + 3 of them: one load instruction of a wave reads 1 KB in one piece.  The packed
// table of a source is its loop followed by kWavePad wrap frames (word i = frame i mod len), so a quad that starts at ANY index
// below len is 256 consecutive words: no lane has to decide on which side of the loop's end it lies, and everything about the
// address but `16 bytes x lane` is uniform over the wave -- start, step and wrap are computed once per wave, from scalars.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define TD_SI_HD __host__ __device__ __forceinline__
#else
#define TD_SI_HD inline
#endif

namespace tdsi {

constexpr uint32_t kQuadFrames = 256;              // frames a wave reads with one load instruction
constexpr uint32_t kWavePad = kQuadFrames - 1u;    // wrap frames behind the loop: a quad may start at len - 1

// words of a packed table of `len` frames: the loop, the pad, rounded up to four words
TD_SI_HD uint32_t packed_words(uint32_t len) { return (len + kWavePad + 3u) & ~3u; }

TD_SI_HD uint32_t mul_hi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

// i < 2 len  ->  i mod len
TD_SI_HD uint32_t wrap_once(uint32_t i, uint32_t len) { return i >= len ? i - len : i; }

// x mod len for any 32-bit x, magic = floor(2^32 / len) (0xFFFFFFFF for len 1): the quotient is short by 1 at most
TD_SI_HD uint32_t wave_start(uint32_t x, uint32_t len, uint32_t magic) { return wrap_once(x - mul_hi(x, magic) * len, len); }

// 256 mod len: from one quad of a wave to its next
TD_SI_HD uint32_t quad_step(uint32_t len, uint32_t magic) { return wave_start(kQuadFrames, len, magic); }

// the next quad's index (i, step < len < 2^31)
TD_SI_HD uint32_t next_quad(uint32_t i, uint32_t step, uint32_t len) { return wrap_once(i + step, len); }

}  // namespace tdsi
