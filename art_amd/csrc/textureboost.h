// art_amd/csrc/textureboost.h -- argument blocks of the texture-boost kernels (textureboost.hip) and the tool's host routines, shared with
// artgpu_api.hip.  (reference: rtengine/iptextureboost.cc:37-248; guidedfilter.cc:58-241; rescale.h:27-74; rt_algo.cc:733-775, 902-939)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "dehaze.h"

namespace artgpu {

constexpr int TB_MAX_K = 9;                // build_gaussian_kernel's size for a sigma below 1
constexpr int TB_MAX_PARTIALS = 64 * 1024; // the prepare pass's grid: at most 64 x 1024 workgroups, one minimum each
struct TbState { float minval; float pad[15]; };

// the Y plane the call reads and writes (rows of `stride` floats) and the planes it works in (rows of w floats)
struct TbPrepareArgs {
    const float *Y; size_t stride; int W, H;
    float *src, *mid; int w, h;            // w x h == W x H unless the rescale of L57-63 is taken
    float *partial;                        // one minimum per workgroup ...
    unsigned long long *partial_idx;       // ... and the raster index of the first pixel that holds it
};
struct TbConvArgs { const float *src; float *dst; int w, h; int K; float coef[TB_MAX_K * TB_MAX_K]; };
// the statistics grid of a self-guided filter on `mid`: plane 0 = I1 -> meanI -> mean a, plane 1 = I1 * I1 -> corrI -> mean b (DhGuided)
struct TbCombineArgs {
    float *src; const float *mid; int w, h;
    DhGuided gf;                           // the second filter's means: base = bilinear(mean a) * mid + bilinear(mean b)
    const TbState *st;
    float strength, strength2, blend;
    // the last iteration of a call that took no rescale: * 65535.f and the store into the Y plane, through the mask when `do_blend`
    int last;
    float *Y; size_t stride;
    int do_blend; const float *mask; size_t m_stride;      // mask == nullptr: 1.f
};
struct TbDownArgs {
    const float *src; int w, h;
    float *Y; size_t stride; int W, H;
    int do_blend; const float *mask; size_t m_stride;
};

hipError_t launch_tb_prepare(const TbPrepareArgs &a, TbState *st, hipStream_t s);        // L57-63, L85-101
hipError_t launch_tb_conv(const TbConvArgs &a, hipStream_t s);                           // Convolution::operator() as the direct sum
hipError_t launch_tb_gf_subsample(const float *mid, int w, int h, const DhGuided &gf, hipStream_t s);
hipError_t launch_tb_gf_ab(const DhGuided &gf, hipStream_t s);
hipError_t launch_tb_gf_finish(float *mid, int w, int h, const DhGuided &gf, hipStream_t s);     // the first filter's q, in place
hipError_t launch_tb_combine(const TbCombineArgs &a, hipStream_t s);                     // L131 (last step) and L136-156, L162-173
hipError_t launch_tb_downscale(const TbDownArgs &a, hipStream_t s);                      // L162-177 and the region's blend

// host side: build_gaussian_kernel (rt_algo.cc:902-939); returns K (odd), coef holds K * K values, row-major.  K > TB_MAX_K: coef untouched
int tb_gaussian_kernel(float sigma, float *coef);

} // namespace artgpu
