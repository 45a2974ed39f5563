// art_amd/csrc/toneequalizer.hip -- the tone equalizer's own passes on gfx950
// (reference: rtengine/iptoneequalizer.cc:345-371 ImProcFunctions::toneEqualizer, :69-340 tone_eq; rtengine/guidedfilter.cc:225-271;
//  Color::rgbLuminance with the TMatrix, color.h; LUTf::operator[] float and vfloat, LUT.h:349-377,436-459).
//
// Everything with a window runs through the guided filter's shared launches (gf_subsample / gf_ab of guided.hip, hblur / vblur_combine of
// denoise.hip, gf_finish_plain for a regularising filter that is not the last); what is here is every pass that touches the image or a
// full-size Y plane.
// The reference stores the image three times (multiply(gain), the correction, multiply(1.f / gain)); here ((R * gain) * corr) * (1.f / gain)
// stays in registers, the same three roundings.  All passes are streaming: loads first, then arithmetic, then stores.  No kernel waits for
// another workgroup.
//
// The reference's SSE2 loop (L318-330) decides per group of four columns, counted from column 0 of the row: if any of the four Y is above
// 1.f all four take vprocess_pixel (the 4-lane xlogf / xexpf), otherwise all four take the vector table lookup; the W % 4 columns behind the
// last whole group take the scalar forms (L332-338).  Two forms of that rule are built (TeArgs::group_thread): one thread per group, and one
// pixel per lane with the decision taken from a ballot over the wave -- a wave starts at a column that is a multiple of 64, so its aligned
// lane quads are the row's groups; no lane leaves before the ballot, lanes past the row's end vote with Y = 0.
#include <hip/hip_runtime.h>
#include "devmath.h"
#include "devsleef.h"
#include "toneequalizer.h"

namespace artgpu {

namespace {

constexpr int TE_BX = 64, TE_BY = 4;      // a workgroup covers 64 x 4 threads: a wave works on one row

__device__ __forceinline__ float te_bilinear(const float *__restrict__ src, int W, int H, float x, float y)   // getBilinearValue (rescale.h:27-50)
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

// L123: LIM(Color::rgbLuminance(R, G, B, ws), 1e-5f, 32.f) -- double products and sum, narrowed once
__device__ __forceinline__ float te_lum(float r, float g, float b, const double *ws1)
{
    const float l = (float)(r * ws1[0] + g * ws1[1] + b * ws1[2]);
    return std_max(1e-5f, std_min(l, 32.f));
}

// L144-147: exp2(round(LIM(log2(max(Y, 1e-9f)), -16, 6) * 5.f) / 5.f), log2 and exp2 the scalar sleef forms of L75-86
__device__ __forceinline__ float te_posterise(float Y)
{
    const float l2 = xlogf_s(2.f);
    const float l = std_max(-16.f, std_min(xlogf_s(std_max(Y, 1e-9f)) / l2, 6.f));
    const float ll = roundf(l * 5.f) / 5.f;
    return pow_F(2.f, ll);
}

// process_pixel (L175-190): the scalar forms
__device__ __forceinline__ float te_corr_s(float y, const TeArgs &a)
{
    const float l2 = xlogf_s(2.f);
    const float luma = std_max(-14.f, std_min(xlogf_s(std_max(y, 0.f)) / l2, 4.f));
    float c = 0.f;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const float d = luma - (-16.f + 2.f * k);
        c += xexpf_s(-(d * d) / 4.f) * a.factors[k];
    }
    return c / a.w_sum;
}

// vprocess_pixel (L258-270), one lane: the 4-lane xlogf / xexpf, vminf(vmaxf(..)); xlog2v is the scalar xlogf(2.f) (L256)
__device__ __forceinline__ float te_corr_v(float y, const TeArgs &a)
{
    const float l2 = xlogf_s(2.f);
    const float y0 = y > 0.f ? y : 0.f;                          // vmaxf(y, zerov)
    const float l = xlogf_v(y0) / l2;
    const float lo = l > -14.f ? l : -14.f;                      // vmaxf(., vluma_lo)
    const float luma = lo < 4.f ? lo : 4.f;                      // vminf(., vluma_hi)
    float c = 0.f;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const float d = luma - (-16.f + 2.f * k);
        c += xexpf_v(-(d * d) / 4.f) * a.factors[k];
    }
    return c / a.w_sum;
}

__device__ __forceinline__ float te_corr_body(float Y, bool any, const TeArgs &a)     // L319-326
{
    return any ? te_corr_v(Y, a) : lutf_vlookup(a.lut, 65536, Y * 65535.f);
}
__device__ __forceinline__ float te_corr_tail(float Y, const TeArgs &a)               // L333-334
{
    return Y > 1.f ? te_corr_s(Y, a) : lutf_lookup<true>(a.lut, 65536, Y * 65535.f);
}

dim3 te_grid(int w, int h) { return dim3((w + TE_BX - 1) / TE_BX, (h + TE_BY - 1) / TE_BY); }

} // namespace

// L121-125, and what the next step wants of Y: the plane itself, guidedFilterLog's xlin2log(max(Y, 0), 10) (guidedfilter.cc:246-253), or --
// regularization > 1 without a detail filter (radius 0) -- Y2 and the posterised Y of L142-149
template <int MODE>
__global__ void __launch_bounds__(256) te_prepare_kernel(TeArgs a)
{
    const int x = blockIdx.x * TE_BX + (threadIdx.x & (TE_BX - 1)), y = blockIdx.y * TE_BY + threadIdx.x / TE_BX;
    if (x >= a.W || y >= a.H) return;
    const size_t si = (size_t)y * a.stride + x, t = (size_t)y * a.W + x;
    const float r = a.img[0][si] * a.gain, g = a.img[1][si] * a.gain, b = a.img[2][si] * a.gain;
    const float Y = te_lum(r, g, b, a.ws1);
    if (MODE == TE_PREP_LOG) a.Y[t] = xlin2log(std_max(Y, 0.f), 10.f);
    else if (MODE == TE_PREP_POSTERISE) { a.Y2[t] = Y; a.Y[t] = te_posterise(Y); }
    else a.Y[t] = Y;
}

// the detail filter's last pass: q = bilinear(mean a) * I + bilinear(mean b) (guidedfilter.cc:225-240), Y = xlog2lin(max(q, 0), 10) (L258-264);
// POST: regularization > 1, the same pass writes Y2 = Y and the posterised Y (L142-149)
template <bool POST>
__global__ void __launch_bounds__(256) te_detail_finish_kernel(TeArgs a)
{
    const int x = blockIdx.x * TE_BX + (threadIdx.x & (TE_BX - 1)), y = blockIdx.y * TE_BY + threadIdx.x / TE_BX;
    if (x >= a.W || y >= a.H) return;
    const size_t t = (size_t)y * a.W + x;
    const float col_scale = (float)a.w / (float)a.W, row_scale = (float)a.h / (float)a.H;
    const float fx = x * col_scale, fy = y * row_scale;
    const float I = a.Y[t];
    const float q = te_bilinear(a.ma, a.w, a.h, fx, fy) * I + te_bilinear(a.mb, a.w, a.h, fx, fy);
    const float Y = xlog2lin(std_max(q, 0.f), 10.f);
    if (POST) { a.Y2[t] = Y; a.Y[t] = te_posterise(Y); }
    else a.Y[t] = Y;
}

// L315-339 between the two multiply() calls of L356 / L368.  Where Y comes from -- TE_Y_PIXEL: regularization 0, from the pixel itself, no plane
// is kept; TE_Y_PLANE: the Y plane; TE_Y_UPSAMPLE: the last regularising filter's pointwise pass is done here, Y = bilinear(mean a) * Y2 +
// bilinear(mean b) (guidedfilter.cc:225-240, gf_finish_plain_kernel's expression), so that filter neither writes nor this pass reads a Y plane
enum { TE_Y_PIXEL = 0, TE_Y_PLANE = 1, TE_Y_UPSAMPLE = 2 };

template <int SRC>
__device__ __forceinline__ float te_load_y(const TeArgs &a, int x, int y)
{
    const size_t t = (size_t)y * a.W + x;
    if (SRC == TE_Y_PLANE) return a.Y[t];
    const float col_scale = (float)a.w / (float)a.W, row_scale = (float)a.h / (float)a.H;
    const float fx = x * col_scale, fy = y * row_scale;
    const float I = a.Y2[t];
    return te_bilinear(a.ma, a.w, a.h, fx, fy) * I + te_bilinear(a.mb, a.w, a.h, fx, fy);
}

template <int SRC, bool GROUP_THREAD>
__global__ void __launch_bounds__(256) te_apply_kernel(TeArgs a)
{
    constexpr bool DIRECT = SRC == TE_Y_PIXEL;
    const int lane = threadIdx.x & (TE_BX - 1), y = blockIdx.y * TE_BY + threadIdx.x / TE_BX;
    if (GROUP_THREAD) {
        const int x0 = (blockIdx.x * TE_BX + lane) * 4;
        if (x0 >= a.W || y >= a.H) return;
        const int n = min(4, a.W - x0);
        const size_t si = (size_t)y * a.stride + x0;
        float r[4], g[4], b[4], Y[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) {
                r[k] = a.img[0][si + k]; g[k] = a.img[1][si + k]; b[k] = a.img[2][si + k];
                if (!DIRECT) Y[k] = te_load_y<SRC>(a, x0 + k, y);
            }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) {
                r[k] *= a.gain; g[k] *= a.gain; b[k] *= a.gain;
                if (DIRECT) Y[k] = te_lum(r[k], g[k], b[k], a.ws1);
            }
        const bool any = Y[0] > 1.f || Y[1] > 1.f || Y[2] > 1.f || Y[3] > 1.f;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) {
                const float corr = n == 4 ? te_corr_body(Y[k], any, a) : te_corr_tail(Y[k], a);
                a.img[0][si + k] = (r[k] * corr) * a.igain;
                a.img[1][si + k] = (g[k] * corr) * a.igain;
                a.img[2][si + k] = (b[k] * corr) * a.igain;
            }
    } else {
        const int x = blockIdx.x * TE_BX + lane;
        const bool in = x < a.W && y < a.H;
        const size_t si = (size_t)y * a.stride + x;
        float r = 0.f, g = 0.f, b = 0.f, Y = 0.f;
        if (in) {
            r = a.img[0][si]; g = a.img[1][si]; b = a.img[2][si];
            if (!DIRECT) Y = te_load_y<SRC>(a, x, y);
            r *= a.gain; g *= a.gain; b *= a.gain;
            if (DIRECT) Y = te_lum(r, g, b, a.ws1);
        }
        // every lane of the wave is here: the four bits of this lane's aligned quad
        const unsigned long long above = __ballot(Y > 1.f);
        const bool any = ((above >> (lane & ~3)) & 0xfull) != 0;
        if (!in) return;
        const float corr = x < (a.W & ~3) ? te_corr_body(Y, any, a) : te_corr_tail(Y, a);
        a.img[0][si] = (r * corr) * a.igain;
        a.img[1][si] = (g * corr) * a.igain;
        a.img[2][si] = (b * corr) * a.igain;
    }
}

hipError_t launch_te_prepare(const TeArgs &a, hipStream_t s)
{
    const dim3 g = te_grid(a.W, a.H);
    if (a.mode == TE_PREP_LOG) hipLaunchKernelGGL(te_prepare_kernel<TE_PREP_LOG>, g, dim3(256), 0, s, a);
    else if (a.mode == TE_PREP_POSTERISE) hipLaunchKernelGGL(te_prepare_kernel<TE_PREP_POSTERISE>, g, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(te_prepare_kernel<TE_PREP_Y>, g, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_te_detail_finish(const TeArgs &a, hipStream_t s)
{
    const dim3 g = te_grid(a.W, a.H);
    if (a.mode) hipLaunchKernelGGL(te_detail_finish_kernel<true>, g, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(te_detail_finish_kernel<false>, g, dim3(256), 0, s, a);
    return hipGetLastError();
}

template <int SRC>
static hipError_t te_launch_apply(const TeArgs &a, hipStream_t s)
{
    if (a.group_thread) hipLaunchKernelGGL((te_apply_kernel<SRC, true>), te_grid((a.W + 3) / 4, a.H), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((te_apply_kernel<SRC, false>), te_grid(a.W, a.H), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_te_direct(const TeArgs &a, hipStream_t s) { return te_launch_apply<TE_Y_PIXEL>(a, s); }
hipError_t launch_te_apply(const TeArgs &a, hipStream_t s) { return a.upsample ? te_launch_apply<TE_Y_UPSAMPLE>(a, s) : te_launch_apply<TE_Y_PLANE>(a, s); }

} // namespace artgpu
