// What the effect mocks of the host-only sanitizer builds share (TEST INFRASTRUCTURE: mock_comp.cpp, mock_eq.cpp, mock_delay.cpp,
// mock_sat.cpp, mock_chorus.cpp, mock_reverb.cpp).  MOCK_NAME, defined by the mock in front of the include, is what die() says
// in front of its message.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "kernels.h"

// both ends of an array a descriptor points to: past an allocation is an AddressSanitizer report
static volatile unsigned char g_mock_sink;
static inline void touch(const void* p, size_t bytes) {
    if (!p || !bytes) return;
    const volatile unsigned char* b = (const volatile unsigned char*)p;
    g_mock_sink ^= b[0];
    g_mock_sink ^= b[bytes - 1];
}
static inline void touch_w(void* p, size_t bytes) {
    if (!p || !bytes) return;
    volatile unsigned char* b = (volatile unsigned char*)p;
    b[0] = b[0];
    b[bytes - 1] = b[bytes - 1];
}
[[noreturn]] static inline void die(const char* what) {
    fprintf(stderr, MOCK_NAME ": %s\n", what);
    abort();
}
// the term table of an effect vertex: kinds 0 .. 4 only (`other`: what to die with at any other kind)
static inline void touch_terms(const tdk::InTerm* ins, uint32_t k, uint32_t frames, const char* other) {
    touch(ins, (size_t)k * sizeof(tdk::InTerm));
    for (uint32_t i = 0; i < k; ++i) {
        const tdk::InTerm& t = ins[i];
        if (t.kind == 0u || t.kind == 4u) touch(t.p, (size_t)frames * sizeof(float2));
        else if (t.kind == 3u) touch(t.p, ((size_t)t.len + 15) * 4);
        else if (t.kind == 1u || t.kind == 2u) touch(t.p, ((size_t)t.len + 15) * sizeof(float2));
        else die(other);
    }
}
