// The counter-based stream u(seed, pixel, sample, dimension) (DESIGN.md "Random numbers"): integer mixers and one conversion,
// nothing of the device in it, so that shading.h and instances.h (the shutter's sample time) and the host programs of the
// tests draw the same numbers from one statement of the rule.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PATHED_STREAM_FN __host__ __device__ inline
#else
#define PATHED_STREAM_FN inline
#endif

namespace pathed {

// ---------------------------------------------------------------------------- rng
// Counter-based stream u(seed, pixel, sample, dimension); replaces the reference's
// shared, unseedable mt19937 (src/random_generator.cpp:4-6).  Two bijective 32-bit
// mixers keyed by pixel and sample, so no two (pixel, sample) pairs share a stream.

PATHED_STREAM_FN uint32_t mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

struct Rng {
    uint32_t k0, k1;
    uint32_t dimension;

    PATHED_STREAM_FN float next()
    {
        const uint32_t bits = mix32(k0 + mix32(k1 + dimension * 0x9e3779b9u));
        dimension++;
        // 24 bits scaled into [0, 1 - 2^-23): the range of the reference generator
        return (float)(bits >> 8) * 5.9604638e-08f;
    }
};

PATHED_STREAM_FN void makeKey(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t *k0, uint32_t *k1)
{
    *k0 = mix32(pixel ^ mix32((uint32_t)seed));
    *k1 = mix32(sample ^ mix32((uint32_t)(seed >> 32) ^ 0x9e3779b9u));
}

// The shutter (instances.h: sampleTime): a sample's time is its stream at this dimension.  No vertex owns it: vertexBase
// (shading.h) reaches it only past 5 * 10^8 vertices, and dimensions 0 and 1 are the camera jitter.
static const uint32_t kDimTime = 0xFFFFFFFFu;

}  // namespace pathed
