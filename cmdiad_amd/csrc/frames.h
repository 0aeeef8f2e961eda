// Host-side helpers shared by the launchers of the kernels that work on per-image maps (metrics, pr_metrics, regions, overlay,
// mesh, organize, sample_prep, eyecandies, tiff, png, preprocess): the limits of a batch of frames, the launch geometry of a
// pixel-per-lane kernel and the check of a HIP runtime call.  cmdiad_amd/ops.py states the same limits as FRAME_MAX_*;
// tests/test_frame_limits_cpu.py holds the two together.
#pragma once
#include "common.h"

constexpr int kMaxSide = 1 << 14;          // a side of an image: H * W fits an int, B * H * W * 3 a size_t
constexpr int kMaxImages = 65535;          // grid.y
constexpr int kMaxImagePixels = 1 << 24;   // H * W: the union-find indices and the labels of an image are ints
constexpr int kMaxTotal = 1 << 30;         // n * H * W, and the length of any list: every count fits an int / a uint32

// n frames of H x W
inline bool sizes_ok(int n, int H, int W)
{
    return n >= 0 && n <= kMaxImages && H >= 1 && W >= 1 && (long long)H * W <= kMaxImagePixels && (long long)n * H * W <= kMaxTotal;
}
inline bool side_ok(int v) { return v >= 1 && v <= kMaxSide; }

// one pixel per lane of 256-thread workgroups, the image in grid.y / two pixels per lane
inline dim3 pixel_grid(int pixels, int B) { return dim3((unsigned)((pixels + 255) / 256), (unsigned)B); }
inline unsigned blocks512(int n) { return (unsigned)((n + 511) / 512); }

// a HIP runtime call (a memset, a copy, a library call that returns hipError_t) inside the entry point `who`
#define CMDIAD_CHECK_HIP(who, call)                                                          \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            cmdiad_set_error("%s: %s: %s", (who), #call, hipGetErrorString(e_));             \
            return CMDIAD_ERR_LAUNCH;                                                        \
        }                                                                                    \
    } while (0)
