// An organised cloud beside maps of H x W: one float32 xyz per map pixel, addressed through two element strides, so the planar
// [n,3,H,W] and the interleaved [n,H,W,3] layout are one code path and give the same bits; the image stride is 3 H W in both.
// Shared by regions.hip (cmdiad_region_measure) and mesh.hip.
#pragma once
#include <hip/hip_runtime.h>

struct Cloud {
    const float* p;
    long long pix, ch;
};

struct Pt { float x, y, z; };

__device__ __forceinline__ Pt cloud_at(const Cloud& c, size_t img_base, int q)
{
    const float* at = c.p + img_base + (long long)q * c.pix;
    return {at[0], at[c.ch], at[2 * c.ch]};
}
__device__ __forceinline__ bool finite3(const Pt& p) { return fabsf(p.x) < INFINITY && fabsf(p.y) < INFINITY && fabsf(p.z) < INFINITY; }
// the reference's rule (all three coordinates non-zero; -0.0 is zero) and finite
__device__ __forceinline__ bool valid_pt(const Pt& p) { return p.x != 0.f && p.y != 0.f && p.z != 0.f && finite3(p); }

// planar (1, H W) or interleaved (3, 1): the only two stride pairs the entry points accept
inline bool cloud_strides_ok(long long pix_stride, long long ch_stride, long long HW)
{
    return (pix_stride == 1 && ch_stride == HW) || (pix_stride == 3 && ch_stride == 1);
}
