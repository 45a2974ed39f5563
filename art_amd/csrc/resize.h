// art_amd/csrc/resize.h -- argument block and tile geometry of the Lanczos resampler (resize.hip), shared with the C-ABI host code
// (api_resize.hip).  ImProcFunctions::Lanczos (rtengine/ipresize.cc:53-223).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace artgpu {

// One workgroup of 256 lanes resamples RS_ROWS destination rows of `tile_w` destination columns.  Its lanes own one source column each, so the
// horizontal taps of a tile's columns have to lie within RS_SPAN source columns: the host picks the largest tile_w that does (rs_tile_width).
constexpr int RS_ROWS = 16;
constexpr int RS_SPAN = 256;
constexpr int RS_PITCH = RS_SPAN + 1;          // floats between the LDS rows of two destination rows
constexpr int RS_MIN_TILE_W = 8;               // a scale whose support leaves fewer destination columns per tile is refused
constexpr int RS_MAX_TILE_W = 1024;

struct RsArgs {
    const float *src[3]; size_t sstride;       // three planes, rows of `sstride` floats
    float *dst[3]; size_t dstride;
    int sW, sH, dW, dH;
    int support;                               // floats per weight row
    int tile_w;                                // destination columns per workgroup
    const float *wv, *wh;                      // dH / dW rows of `support` normalised weights (tap ii0 / jj0 first)
    const int *ii0, *ii1, *jj0, *jj1;          // tap ranges, [first, last + 1); empty where first >= last + 1
};

// rows_fast: lanes of a wave run down the tile's rows in the horizontal stage (downscales); otherwise along its columns (upscales)
hipError_t launch_resize_lanczos(const RsArgs &a, bool rows_fast, hipStream_t s);

} // namespace artgpu
