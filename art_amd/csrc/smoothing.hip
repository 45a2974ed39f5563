// art_amd/csrc/smoothing.hip -- the Smoothing tool's own passes on gfx950, modes GUIDED and NLMEANS
// (reference: rtengine/ipsmoothing.cc:902-1073 guidedSmoothing, :334-409 guided_smoothing, :411-434 find_region, :500-562 nlmeans_smoothing;
//  rtengine/guidedfilter.cc:80-265; Color::rgb2yuv / yuv2rgb color.h:783-796; Imagefloat::multiply imagefloat.cc:396-432).
//
// The statistics of the guided filter live on the w x h grid and run through the shared kernels (gf_subsample / gf_ab of guided.hip, hblur /
// vblur_combine of denoise.hip); what is here is everything that touches the image or a working plane: the masks' bounding boxes, the
// normalise passes, GUIDED's prepare and finish per channel setting (the last finish blends into the image), the self-guided statistics
// of channel LC (guide == source: two grid planes per channel instead of four), NLMEANS' crop / YUV split and its merge + blend.
// The normalise passes (x * (1.f / 65535.f) ahead of the regions, x * 65535.f behind them) are fused into a region's passes where every pixel
// still sees exactly one of each: a full-frame region that runs first reads the image through the first factor (src_norm / img_norm), one
// that runs last stores through the second (out_denorm); a cropped region at either end leaves that pass to sm_scale_kernel.
// All of it is streaming: every pass issues its loads first, then computes, then stores.
#include <hip/hip_runtime.h>
#include "devmath.h"
#include "devsleef.h"
#include "smoothing.h"

namespace artgpu {

namespace {

constexpr float SM_F1 = 1.f / 65535.f;     // normalizeFloatTo1's factor (imagefloat.cc:396-432)
constexpr int SM_BX = 64, SM_BY = 4;      // a workgroup covers 64 x 4 pixels: a wave reads 256 contiguous bytes of every plane it touches

__device__ __forceinline__ float sm_bilinear(const float *__restrict__ src, int W, int H, float x, float y)   // getBilinearValue (rescale.h:27-50)
{
    const int xi = min((int)x, W - 1), yi = min((int)y, H - 1);
    const float xf = x - xi, yf = y - yi;
    const int xi1 = min(xi + 1, W - 1), yi1 = min(yi + 1, H - 1);
    const float bl = src[(size_t)yi * W + xi], br = src[(size_t)yi * W + xi1];
    const float tl = src[(size_t)yi1 * W + xi], tr = src[(size_t)yi1 * W + xi1];
    const float b = xf * br + (1.f - xf) * bl;
    const float t = xf * tr + (1.f - xf) * tl;
    return yf * t + (1.f - yf) * b;
}

// Color::rgb2yuv / yuv2rgb with the double matrix (color.h:783-796): the products are double, the results float
__device__ __forceinline__ float sm_lum(float r, float g, float b, const double *ws1) { return (float)(r * ws1[0] + g * ws1[1] + b * ws1[2]); }
__device__ __forceinline__ void sm_yuv2rgb(float Y, float u, float v, float &R, float &G, float &B, const double *ws1)
{
    B = Y - u;
    R = v + Y;
    G = (float)((Y - R * ws1[0] - B * ws1[2]) / ws1[1]);
}

dim3 sm_grid(int w, int h) { return dim3((w + SM_BX - 1) / SM_BX, (h + SM_BY - 1) / SM_BY); }

} // namespace

// find_region (L411-434) for every mask of the call: integer minima / maxima, so the order of the lanes does not matter
__global__ void __launch_bounds__(256) sm_box_kernel(SmBoxArgs a)
{
    const int k = blockIdx.y;
    const float *m = a.mask[k];
    const size_t ms = a.stride[k];
    int x0 = a.W, y0 = a.H, x1 = -1, y1 = -1;
    const long long n = (long long)a.W * a.H;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
        const int y = (int)(t / a.W), x = (int)(t - (long long)y * a.W);
        if (m[(size_t)y * ms + x] > 0.f) {
            x0 = min(x0, x); x1 = max(x1, x);
            y0 = min(y0, y); y1 = max(y1, y);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x0 = min(x0, __shfl_xor(x0, o)); y0 = min(y0, __shfl_xor(y0, o));
        x1 = max(x1, __shfl_xor(x1, o)); y1 = max(y1, __shfl_xor(y1, o));
    }
    if ((threadIdx.x & 63) == 0 && x1 >= 0) {
        atomicMin(a.box + 4 * k + 0, x0); atomicMin(a.box + 4 * k + 1, y0);
        atomicMax(a.box + 4 * k + 2, x1); atomicMax(a.box + 4 * k + 3, y1);
    }
}

// normalizeFloatTo1 / normalizeFloatTo65535 (imagefloat.cc:396-432).  MODE 2: an empty region list, both in one pass
template <int MODE>
__global__ void __launch_bounds__(256) sm_scale_kernel(float *r, float *g, float *b, size_t stride, int W, int H)
{
    const int x = blockIdx.x * SM_BX + (threadIdx.x & (SM_BX - 1)), y = blockIdx.y * SM_BY + threadIdx.x / SM_BX;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * stride + x;
    float v0 = r[i], v1 = g[i], v2 = b[i];
    if (MODE == 0 || MODE == 2) { v0 *= SM_F1; v1 *= SM_F1; v2 *= SM_F1; }
    if (MODE == 1 || MODE == 2) { v0 *= 65535.f; v1 *= 65535.f; v2 *= 65535.f; }
    r[i] = v0; g[i] = v1; b[i] = v2;
}

// GUIDED, one iteration's first pass (L353-377, guidedfilter.cc:246-253): the kept input and the log guide for L and C, the three log channels
template <int CH>
__global__ void __launch_bounds__(256) sm_prepare_kernel(SmArgs a)
{
    const int x = blockIdx.x * SM_BX + (threadIdx.x & (SM_BX - 1)), y = blockIdx.y * SM_BY + threadIdx.x / SM_BX;
    if (x >= a.ww || y >= a.hh) return;
    const size_t si = (size_t)y * a.src_stride + x, t = (size_t)y * a.ww + x;
    float r = a.src[0][si], g = a.src[1][si], b = a.src[2][si];
    if (a.src_norm) { r *= SM_F1; g *= SM_F1; b *= SM_F1; }
    if (CH != SM_CH_LC) {
        a.in[0][t] = r; a.in[1][t] = g; a.in[2][t] = b;
        a.guide[t] = xlin2log(std_max(sm_lum(r, g, b, a.ws1), 0.f), 10.f);
    }
    a.chan[0][t] = xlin2log(std_max(r, 0.f), 10.f);
    a.chan[1][t] = xlin2log(std_max(g, 0.f), 10.f);
    a.chan[2][t] = xlin2log(std_max(b, 0.f), 10.f);
}

// GUIDED LC, guidedFilter(chan, chan, chan) (guidedfilter.cc:186-204): I1 == p1, so meanI == meanp and corrI == corrIp bit for bit and only
// {I1, I1 * I1} are kept per channel
__global__ void __launch_bounds__(256) sm_subsample_self_kernel(SmArgs a)
{
    const int x = blockIdx.x * SM_BX + (threadIdx.x & (SM_BX - 1)), y = blockIdx.y * SM_BY + threadIdx.x / SM_BX;
    if (x >= a.w || y >= a.h) return;
    const size_t nl = (size_t)a.w * a.h, t = (size_t)y * a.w + x;
    const bool same = a.w == a.ww && a.h == a.hh;
    const float col_scale = (float)a.ww / (float)a.w, row_scale = (float)a.hh / (float)a.h;
    const float fx = x * col_scale, fy = y * row_scale;
    float I1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) I1[c] = same ? a.chan[c][t] : sm_bilinear(a.chan[c], a.ww, a.hh, fx, fy);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a.low[(2 * c) * nl + t] = I1[c];
        a.low[(2 * c + 1) * nl + t] = I1[c] * I1[c];
    }
}

// ... after the two means per channel: a = covIp / (varI + eps), b = meanp - a * meanI (guidedfilter.cc:206-220) with covIp == varI's operands
__global__ void __launch_bounds__(256) sm_ab_self_kernel(SmArgs a)
{
    const int x = blockIdx.x * SM_BX + (threadIdx.x & (SM_BX - 1)), y = blockIdx.y * SM_BY + threadIdx.x / SM_BX;
    if (x >= a.w || y >= a.h) return;
    const size_t nl = (size_t)a.w * a.h, t = (size_t)y * a.w + x;
    float meanI[3], corrI[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { meanI[c] = a.low[(2 * c) * nl + t]; corrI[c] = a.low[(2 * c + 1) * nl + t]; }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float varI = corrI[c] - (meanI[c] * meanI[c]);
        const float covIp = corrI[c] - (meanI[c] * meanI[c]);
        const float av = covIp / (varI + a.epsilon);
        const float bv = meanI[c] - (av * meanI[c]);
        a.low[(2 * c) * nl + t] = av;
        a.low[(2 * c + 1) * nl + t] = bv;
    }
}

// GUIDED, one iteration's last pass: q = bilinear(mean a) * I + bilinear(mean b), xlog2lin(max(q, 0), 10) (guidedfilter.cc:225-240,258-264),
// the YUV recombination of L382-406; an iteration that is not the last stores the working planes, the last one blends into the image
// (L1050-1064) and stores nothing else
template <int CH, bool LAST>
__global__ void __launch_bounds__(256) sm_finish_kernel(SmArgs a)
{
    const int x = blockIdx.x * SM_BX + (threadIdx.x & (SM_BX - 1)), y = blockIdx.y * SM_BY + threadIdx.x / SM_BX;
    if (x >= a.ww || y >= a.hh) return;
    const size_t t = (size_t)y * a.ww + x, di = (size_t)y * a.stride + x;
    const float col_scale = (float)a.w / (float)a.ww, row_scale = (float)a.h / (float)a.hh;
    const float fx = x * col_scale, fy = y * row_scale;
    // loads first
    float I[3], in[3] = {0.f, 0.f, 0.f}, rgb[3] = {0.f, 0.f, 0.f}, m = 1.f;
    if (CH == SM_CH_LC) {
#pragma unroll
        for (int c = 0; c < 3; ++c) I[c] = a.chan[c][t];
    } else {
        I[0] = I[1] = I[2] = a.guide[t];
#pragma unroll
        for (int c = 0; c < 3; ++c) in[c] = a.in[c][t];
    }
    if (LAST) {
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = a.img[c][di];
        if (a.mask) m = a.mask[(size_t)y * a.mask_stride + x];
        if (a.img_norm) { rgb[0] *= SM_F1; rgb[1] *= SM_F1; rgb[2] *= SM_F1; }
    }
    float ma[3], mb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { ma[c] = sm_bilinear(a.a[c], a.w, a.h, fx, fy); mb[c] = sm_bilinear(a.b[c], a.w, a.h, fx, fy); }
    float o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float q = ma[c] * I[c] + mb[c];
        o[c] = xlog2lin(std_max(q, 0.f), 10.f);
    }
    if (CH != SM_CH_LC) {
        const float iY = sm_lum(in[0], in[1], in[2], a.ws1);
        float oY = sm_lum(o[0], o[1], o[2], a.ws1);
        float ou = oY - o[2], ov = o[0] - oY;
        if (CH == SM_CH_L) {
            ou = iY - in[2];
            ov = in[0] - iY;
        } else {
            const float bump = oY > 1e-5f ? iY / oY : 1.f;
            ou *= bump;
            ov *= bump;
            oY = iY;
        }
        sm_yuv2rgb(oY, ou, ov, o[0], o[1], o[2], a.ws1);
    }
    if (LAST) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = intp(m, o[c], rgb[c]);
            if (a.out_denorm) v *= 65535.f;
            a.img[c][di] = v;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.work[c][t] = o[c];
    }
}

// NLMEANS, first pass (L505-515, L530-541): L: iY -> work[0]; LC: the crop -> work[0..2]; C: the crop and iY -> in[0]
template <int CH>
__global__ void __launch_bounds__(256) sm_nlm_split_kernel(SmArgs a)
{
    const int x = blockIdx.x * SM_BX + (threadIdx.x & (SM_BX - 1)), y = blockIdx.y * SM_BY + threadIdx.x / SM_BX;
    if (x >= a.ww || y >= a.hh) return;
    const size_t si = (size_t)y * a.stride + x, t = (size_t)y * a.ww + x;
    float r = a.img[0][si], g = a.img[1][si], b = a.img[2][si];
    if (a.img_norm) { r *= SM_F1; g *= SM_F1; b *= SM_F1; }
    if (CH == SM_CH_L) {
        a.work[0][t] = sm_lum(r, g, b, a.ws1);
    } else {
        a.work[0][t] = r; a.work[1][t] = g; a.work[2][t] = b;
        if (CH == SM_CH_C) a.in[0][t] = sm_lum(r, g, b, a.ws1);
    }
}

// NLMEANS, last pass: the yuv2rgb of L519-528 (L) or L549-559 (C) and the blend of L1050-1064
template <int CH>
__global__ void __launch_bounds__(256) sm_nlm_merge_kernel(SmArgs a)
{
    const int x = blockIdx.x * SM_BX + (threadIdx.x & (SM_BX - 1)), y = blockIdx.y * SM_BY + threadIdx.x / SM_BX;
    if (x >= a.ww || y >= a.hh) return;
    const size_t di = (size_t)y * a.stride + x, t = (size_t)y * a.ww + x;
    float rgb[3], wk[3] = {0.f, 0.f, 0.f}, iY = 0.f, m = 1.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = a.img[c][di];
    if (a.img_norm) { rgb[0] *= SM_F1; rgb[1] *= SM_F1; rgb[2] *= SM_F1; }
    if (CH == SM_CH_L) {
        iY = a.work[0][t];
    } else {
        // (no working planes: a region whose filter does nothing -- r == 0, nlstrength == 0 -- still blends its untouched copy)
#pragma unroll
        for (int c = 0; c < 3; ++c) wk[c] = a.work[0] ? a.work[c][t] : rgb[c];
        if (CH == SM_CH_C) iY = a.in[0][t];
    }
    if (a.mask) m = a.mask[(size_t)y * a.mask_stride + x];
    if (CH == SM_CH_L) {
        const float Y = sm_lum(rgb[0], rgb[1], rgb[2], a.ws1);
        sm_yuv2rgb(iY, Y - rgb[2], rgb[0] - Y, wk[0], wk[1], wk[2], a.ws1);
    } else if (CH == SM_CH_C) {
        const float Y = sm_lum(wk[0], wk[1], wk[2], a.ws1);
        const float u = Y - wk[2], v = wk[0] - Y;
        sm_yuv2rgb(iY, u, v, wk[0], wk[1], wk[2], a.ws1);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = intp(m, wk[c], rgb[c]);
        if (a.out_denorm) v *= 65535.f;
        a.img[c][di] = v;
    }
}

hipError_t launch_sm_box(const SmBoxArgs &a, hipStream_t s)
{
    long long g = ((long long)a.W * a.H + 255) / 256;
    hipLaunchKernelGGL(sm_box_kernel, dim3((unsigned)(g < 2048 ? g : 2048), a.n), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_sm_scale(float *const img[3], size_t stride, int W, int H, int mode, hipStream_t s)
{
    if (mode == 0) hipLaunchKernelGGL(sm_scale_kernel<0>, sm_grid(W, H), dim3(256), 0, s, img[0], img[1], img[2], stride, W, H);
    else if (mode == 1) hipLaunchKernelGGL(sm_scale_kernel<1>, sm_grid(W, H), dim3(256), 0, s, img[0], img[1], img[2], stride, W, H);
    else hipLaunchKernelGGL(sm_scale_kernel<2>, sm_grid(W, H), dim3(256), 0, s, img[0], img[1], img[2], stride, W, H);
    return hipGetLastError();
}

#define SM_BY_CHANNEL(kernel, w, h)                                                                                         \
    do {                                                                                                                    \
        if (a.channel == SM_CH_L) hipLaunchKernelGGL(kernel<SM_CH_L>, sm_grid(w, h), dim3(256), 0, s, a);                   \
        else if (a.channel == SM_CH_C) hipLaunchKernelGGL(kernel<SM_CH_C>, sm_grid(w, h), dim3(256), 0, s, a);              \
        else hipLaunchKernelGGL(kernel<SM_CH_LC>, sm_grid(w, h), dim3(256), 0, s, a);                                       \
        return hipGetLastError();                                                                                           \
    } while (0)

hipError_t launch_sm_prepare(const SmArgs &a, hipStream_t s) { SM_BY_CHANNEL(sm_prepare_kernel, a.ww, a.hh); }
hipError_t launch_sm_nlm_split(const SmArgs &a, hipStream_t s) { SM_BY_CHANNEL(sm_nlm_split_kernel, a.ww, a.hh); }
hipError_t launch_sm_nlm_merge(const SmArgs &a, hipStream_t s) { SM_BY_CHANNEL(sm_nlm_merge_kernel, a.ww, a.hh); }
hipError_t launch_sm_subsample_self(const SmArgs &a, hipStream_t s) { hipLaunchKernelGGL(sm_subsample_self_kernel, sm_grid(a.w, a.h), dim3(256), 0, s, a); return hipGetLastError(); }
hipError_t launch_sm_ab_self(const SmArgs &a, hipStream_t s) { hipLaunchKernelGGL(sm_ab_self_kernel, sm_grid(a.w, a.h), dim3(256), 0, s, a); return hipGetLastError(); }

hipError_t launch_sm_finish(const SmArgs &a, hipStream_t s)
{
    const dim3 g = sm_grid(a.ww, a.hh);
    if (a.last) {
        if (a.channel == SM_CH_L) hipLaunchKernelGGL((sm_finish_kernel<SM_CH_L, true>), g, dim3(256), 0, s, a);
        else if (a.channel == SM_CH_C) hipLaunchKernelGGL((sm_finish_kernel<SM_CH_C, true>), g, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((sm_finish_kernel<SM_CH_LC, true>), g, dim3(256), 0, s, a);
    } else {
        if (a.channel == SM_CH_L) hipLaunchKernelGGL((sm_finish_kernel<SM_CH_L, false>), g, dim3(256), 0, s, a);
        else if (a.channel == SM_CH_C) hipLaunchKernelGGL((sm_finish_kernel<SM_CH_C, false>), g, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((sm_finish_kernel<SM_CH_LC, false>), g, dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

} // namespace artgpu
