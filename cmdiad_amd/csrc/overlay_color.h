// Steps 2 and 3 of the render contract (docs/overlay.md) for one score: normalise, table index, background byte, blend.  Shared by
// overlay.hip and mesh.hip, which are both compiled with -ffp-contract=off: every floating-point step is one float64 operation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

enum { kBgNone = 0, kBgU8 = 1, kBgF32 = 2 };

// score -> k = floor(t * 255 + 0.5) with t = (s - lo) / d clamped to [0, 1] (d = hi - lo; d <= 0: a step at lo); a NaN score gives
// t = 0 and sets `nan`
__device__ __forceinline__ int overlay_index(double s, double lo, double d, bool& nan)
{
    double t;
    nan = s != s;
    if (nan) {
        t = 0.0;
    } else {
        t = d > 0.0 ? (s - lo) / d : (s > lo ? 1.0 : 0.0);
        t = !(t > 0.0) ? 0.0 : t;
        t = t > 1.0 ? 1.0 : t;
    }
    return (int)floor(t * 255.0 + 0.5);
}

// byte of a normalised float32 background value
__device__ __forceinline__ uint32_t bg_byte(float v, double mean, double stdv)
{
    double b = (double)v * stdv;
    b = b + mean;
    b = b * 255.0;
    b = floor(b + 0.5);
    b = !(b > 0.0) ? 0.0 : b;
    b = b > 255.0 ? 255.0 : b;
    return (uint32_t)(int)b;
}

__device__ __forceinline__ uint32_t blend(uint32_t c, uint32_t bg, uint32_t a) { return (c * a + bg * (255u - a) + 127u) / 255u; }

// table entry e = r | g << 8 | b << 16 | a << 24 over the background g (r | g << 8 | b << 16) -> r | g << 8 | b << 16
__device__ __forceinline__ uint32_t blend_rgb(uint32_t e, uint32_t g)
{
    const uint32_t c = e & 0xffffffu, a = e >> 24;
    return blend(c & 0xff, g & 0xff, a) | blend((c >> 8) & 0xff, (g >> 8) & 0xff, a) << 8 | blend(c >> 16, g >> 16, a) << 16;
}
