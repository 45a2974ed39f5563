// art_amd/csrc/textureboost.hip -- ImProcFunctions::textureBoost on gfx950 (reference: rtengine/iptextureboost.cc:37-248, ART's detail tool;
// guidedfilter.cc:58-241 for its guided filters, rescale.h:27-74 for its bilinear rescales, rt_algo.cc:733-775 / 902-939 for the
// gaussian of the sub-pixel radii).
//
// Every step is the reference's arithmetic in the reference's order (no device-side libm call, the one reduction is a minimum), so the
// kernels give its bits -- with one exception that is a definition, not an approximation: Convolution::operator() is an FFTW product in
// the reference; here it is the direct clamp-to-edge sum it computes, in fp32 and row-major order (see tb_conv_kernel).
// What the reference stores and reads again but a kernel can recompute is not stored: the upscaled input plane exists only inside the
// prepare pass, the second guided filter's output `base` only inside the combine pass, the * 65535.f plane only inside the last store.
// The box blurs are the shared hblur / vblur kernels of denoise.hip.
#include <hip/hip_runtime.h>
#include "devmath.h"
#include "textureboost.h"
#include "kernels.h"
#include <cmath>
#include <vector>

namespace artgpu {

namespace {

constexpr float TB_INF = __builtin_huge_valf();     // RT_INFINITY
constexpr float TB_LO = 1e-5f, TB_HI = 32.f;        // L75-76

// rt_math.h:54-64 folded over the plane in raster order (L92, L99): min(a, b) = b < a ? b : a keeps a when the two compare equal, so where a
// +0.0 and a -0.0 are both the plane's minimum the earlier pixel's is minval -- and minval is what L145 / L154 write into every pixel it wins.
// (v, vi): a pixel's value and its raster index in the work plane.  A NaN never replaces m, as before.
__device__ __forceinline__ void tb_min_first(float &m, unsigned long long &mi, float v, unsigned long long vi)
{
    if (v < m || (v == m && vi < mi)) { m = v; mi = vi; }
}
// the 256 (m, mi) of a workgroup folded into entry 0
__device__ __forceinline__ void tb_min_fold(float *lds, unsigned long long *ldi, int t, float m, unsigned long long mi)
{
    lds[t] = m; ldi[t] = mi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            float a = lds[t]; unsigned long long ai = ldi[t];
            tb_min_first(a, ai, lds[t + s], ldi[t + s]);
            lds[t] = a; ldi[t] = ai;
        }
        __syncthreads();
    }
}

// L85-101: v = src / 65535.f, mid = clamp(v), the workgroup's minimum of v.  With the rescale of L57-63, src is rescaleBilinear(Y) evaluated
// here.  Columns below 4 * (w / 4) clamp the way the reference's vector body does (vmaxf(vminf(v, hi), lo)), the others the way LIM does: the
// two part for a NaN only.
__global__ void __launch_bounds__(256) tb_prepare_kernel(TbPrepareArgs a)
{
    __shared__ float lds[256];
    __shared__ unsigned long long ldi[256];
    const bool same = a.w == a.W && a.h == a.H;
    const float col_scale = (float)a.W / (float)a.w, row_scale = (float)a.H / (float)a.h;
    const int wvec = (a.w / 4) * 4;
    float m = TB_INF;
    unsigned long long mi = ~0ull;
    FOR_IMAGE_XY(y, x, a.w, a.h) {
        const float s = same ? a.Y[(size_t)y * a.stride + x] : dh_bilinear(a.Y, a.stride, a.W, a.H, x * col_scale, y * row_scale);
        const float v = s / 65535.f;
        const size_t i = (size_t)y * a.w + x;
        a.src[i] = v;
        a.mid[i] = x < wvec ? sse_max(sse_min(v, TB_HI), TB_LO) : std_max(TB_LO, std_min(v, TB_HI));
        tb_min_first(m, mi, v, i);
    }
    const int t = threadIdx.x;
    tb_min_fold(lds, ldi, t, m, mi);
    if (t == 0) {
        a.partial[blockIdx.y * gridDim.x + blockIdx.x] = lds[0];
        a.partial_idx[blockIdx.y * gridDim.x + blockIdx.x] = ldi[0];
    }
}
__global__ void __launch_bounds__(256) tb_min_final_kernel(const float *partial, const unsigned long long *partial_idx, int n, TbState *st)
{
    __shared__ float lds[256];
    __shared__ unsigned long long ldi[256];
    float m = TB_INF;
    unsigned long long mi = ~0ull;
    for (int k = threadIdx.x; k < n; k += 256) tb_min_first(m, mi, partial[k], partial_idx[k]);
    const int t = threadIdx.x;
    tb_min_fold(lds, ldi, t, m, mi);
    if (t == 0) st->minval = lds[0];
}

// Convolution::operator() (rt_algo.cc:733-775, 887-893) for a K x K kernel: do_convolution pads by K / 2 with both ends clamped, multiplies the
// spectra and reads back at + 2 * (K / 2) of a padded plane no index wraps in, which is
//   dst[y][x] = sum over ky, kx of kernel[ky][kx] * src[clamp(y + K / 2 - ky)][clamp(x + K / 2 - kx)].
// Here that sum is taken directly, in fp32, ky-major from 0.f: the reference's own result differs from it by the FFT's rounding.
// A workgroup takes a 64 x 16 tile; the tile and its halo sit in LDS, a lane takes four rows of one column.
constexpr int TBC_TW = 64, TBC_TH = 16;
template <int K>
__global__ void __launch_bounds__(256) tb_conv_kernel(TbConvArgs a)
{
    constexpr int R = K / 2, LW = TBC_TW + 2 * R, LH = TBC_TH + 2 * R;
    __shared__ float tile[LH][LW + 1];
    const int x0 = blockIdx.x * TBC_TW, y0 = blockIdx.y * TBC_TH;
    for (int e = threadIdx.x; e < LW * LH; e += 256) {
        const int ly = e / LW, lx = e - ly * LW;
        const int sy = min(max(y0 + ly - R, 0), a.h - 1), sx = min(max(x0 + lx - R, 0), a.w - 1);
        tile[ly][lx] = a.src[(size_t)sy * a.w + sx];
    }
    __syncthreads();
    const int tx = threadIdx.x % TBC_TW, ty = threadIdx.x / TBC_TW;
    const int x = x0 + tx;
    if (x >= a.w) return;
#pragma unroll
    for (int q = 0; q < TBC_TH / 4; ++q) {
        const int ly = ty + 4 * q, y = y0 + ly;
        if (y >= a.h) break;
        float acc = 0.f;
#pragma unroll
        for (int ky = 0; ky < K; ++ky)
#pragma unroll
            for (int kx = 0; kx < K; ++kx) acc += a.coef[ky * K + kx] * tile[ly + 2 * R - ky][tx + 2 * R - kx];
        a.dst[(size_t)y * a.w + x] = acc;
    }
}

// guidedFilter(mid, mid, ., r, eps)'s I1 and I1 * I1 on the gf.w x gf.h grid (guidedfilter.cc:169-198): p1 is I1, so meanp / corrIp would
// repeat meanI / corrI bit for bit and are not built
__global__ void __launch_bounds__(256) tb_gf_subsample_kernel(const float *mid, int w, int h, DhGuided gf)
{
    const float col_scale = (float)w / (float)gf.w, row_scale = (float)h / (float)gf.h;
    const bool same = gf.w == w && gf.h == h;
    FOR_IMAGE_XY(y, x, gf.w, gf.h) {
        const size_t t = (size_t)y * gf.w + x;
        const float I1 = same ? mid[t] : dh_bilinear(mid, w, w, h, x * col_scale, y * row_scale);
        gf.low[t] = I1;
        gf.low[gf.nl + t] = I1 * I1;
    }
}
// a = covIp / (varI + epsilon), b = meanp - a * meanI (guidedfilter.cc:200-214) with p = I
__global__ void __launch_bounds__(256) tb_gf_ab_kernel(DhGuided gf)
{
    const size_t n = gf.nl;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x) {
        const float meanI = gf.low[t], corrI = gf.low[n + t];
        const float varI = corrI - (meanI * meanI);
        const float covIp = corrI - (meanI * meanI);
        const float av = covIp / (varI + gf.eps);
        gf.low[t] = av;
        gf.low[n + t] = meanI - (av * meanI);
    }
}
// q = rescaleBilinear(mean a) * I + rescaleBilinear(mean b) (guidedfilter.cc:225-240) with q == I == mid: pointwise in place
__global__ void __launch_bounds__(256) tb_gf_finish_kernel(float *mid, int w, int h, DhGuided gf)
{
    const float col_scale = (float)gf.w / (float)w, row_scale = (float)gf.h / (float)h;
    FOR_IMAGE_XY(y, x, w, h) {
        const size_t i = (size_t)y * w + x;
        mid[i] = dh_q(gf.low, gf.low + gf.nl, gf.w, gf.h, col_scale, y * row_scale, x, mid[i]);
    }
}

// intp(mask, v, old) into the Y plane (L234-240; mask == nullptr: the same arithmetic with 1.f), or the plain store of a call without a blend
__device__ __forceinline__ void tb_store(float *Y, size_t stride, int do_blend, const float *mask, size_t m_stride, int y, int x, float v)
{
    const size_t i = (size_t)y * stride + x;
    if (do_blend) {
        const float m = mask ? mask[(size_t)y * m_stride + x] : 1.f;
        v = intp(m, v, Y[i]);
    }
    Y[i] = v;
}

// the second guided filter's last step (base, never stored) and L136-156; on the last iteration of a call without a rescale also L162-173
// and the region's blend.  The reference's vector and scalar bodies are the same arithmetic but for the max, which parts for a NaN.
__global__ void __launch_bounds__(256) tb_combine_kernel(TbCombineArgs a)
{
    const float minval = a.st->minval;
    const float col_scale = (float)a.gf.w / (float)a.w, row_scale = (float)a.gf.h / (float)a.h;
    const float *ma = a.gf.low, *mb = a.gf.low + a.gf.nl;
    const int wvec = (a.w / 4) * 4;
    FOR_IMAGE_XY(y, x, a.w, a.h) {
        const size_t i = (size_t)y * a.w + x;
        const float v = a.src[i], m = a.mid[i];
        const float base = dh_q(ma, mb, a.gf.w, a.gf.h, col_scale, y * row_scale, x, m);
        const float d = (v - m) * a.strength;
        const float d2 = (m - base) * a.strength2;
        const float t = base + d + d2;
        const float o = intp(a.blend, x < wvec ? sse_max(t, minval) : std_max(t, minval), v);
        if (a.last) tb_store(a.Y, a.stride, a.do_blend, a.mask, a.m_stride, y, x, o * 65535.f);
        else a.src[i] = o;
    }
}

// L162-177: rescaleBilinear of src * 65535.f back to W x H (the product is formed per tap: the reference multiplies the plane first), then the
// region's blend
__global__ void __launch_bounds__(256) tb_downscale_kernel(TbDownArgs a)
{
    const float col_scale = (float)a.w / (float)a.W, row_scale = (float)a.h / (float)a.H;
    FOR_IMAGE_XY(y, x, a.W, a.H) {
        const float fx = x * col_scale, fy = y * row_scale;
        const int xi = min((int)fx, a.w - 1), yi = min((int)fy, a.h - 1);
        const float xf = fx - xi, yf = fy - yi;
        const int xi1 = min(xi + 1, a.w - 1), yi1 = min(yi + 1, a.h - 1);
        const float bl = a.src[(size_t)yi * a.w + xi] * 65535.f, br = a.src[(size_t)yi * a.w + xi1] * 65535.f;
        const float tl = a.src[(size_t)yi1 * a.w + xi] * 65535.f, tr = a.src[(size_t)yi1 * a.w + xi1] * 65535.f;
        const float b = xf * br + (1.f - xf) * bl;
        const float t = xf * tr + (1.f - xf) * tl;
        tb_store(a.Y, a.stride, a.do_blend, a.mask, a.m_stride, y, x, yf * t + (1.f - yf) * b);
    }
}

} // namespace

hipError_t launch_tb_prepare(const TbPrepareArgs &a, TbState *st, hipStream_t s)
{
    const int gx = (a.w + 255) / 256;
    const dim3 grid(gx > 64 ? 64 : gx, a.h > 1024 ? 1024 : a.h);          // grid.x * grid.y <= TB_MAX_PARTIALS
    hipLaunchKernelGGL(tb_prepare_kernel, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(tb_min_final_kernel, dim3(1), dim3(256), 0, s, a.partial, a.partial_idx, (int)(grid.x * grid.y), st);
    return hipGetLastError();
}
hipError_t launch_tb_conv(const TbConvArgs &a, hipStream_t s)
{
    const dim3 grid((a.w + TBC_TW - 1) / TBC_TW, (a.h + TBC_TH - 1) / TBC_TH);
    if (grid.y > 65535) return hipErrorInvalidValue;
    switch (a.K) {
    case 3: hipLaunchKernelGGL(tb_conv_kernel<3>, grid, dim3(256), 0, s, a); break;
    case 5: hipLaunchKernelGGL(tb_conv_kernel<5>, grid, dim3(256), 0, s, a); break;
    case 7: hipLaunchKernelGGL(tb_conv_kernel<7>, grid, dim3(256), 0, s, a); break;
    case 9: hipLaunchKernelGGL(tb_conv_kernel<9>, grid, dim3(256), 0, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
hipError_t launch_tb_gf_subsample(const float *mid, int w, int h, const DhGuided &gf, hipStream_t s)
{
    hipLaunchKernelGGL(tb_gf_subsample_kernel, image_grid(gf.w, gf.h), dim3(256), 0, s, mid, w, h, gf);
    return hipGetLastError();
}
hipError_t launch_tb_gf_ab(const DhGuided &gf, hipStream_t s)
{
    const size_t g = (gf.nl + 255) / 256;
    hipLaunchKernelGGL(tb_gf_ab_kernel, dim3((unsigned)(g < 16384 ? (g ? g : 1) : 16384)), dim3(256), 0, s, gf);
    return hipGetLastError();
}
hipError_t launch_tb_gf_finish(float *mid, int w, int h, const DhGuided &gf, hipStream_t s)
{
    hipLaunchKernelGGL(tb_gf_finish_kernel, image_grid(w, h), dim3(256), 0, s, mid, w, h, gf);
    return hipGetLastError();
}
hipError_t launch_tb_combine(const TbCombineArgs &a, hipStream_t s) { hipLaunchKernelGGL(tb_combine_kernel, image_grid(a.w, a.h), dim3(256), 0, s, a); return hipGetLastError(); }
hipError_t launch_tb_downscale(const TbDownArgs &a, hipStream_t s) { hipLaunchKernelGGL(tb_downscale_kernel, image_grid(a.W, a.H), dim3(256), 0, s, a); return hipGetLastError(); }

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------

// build_gaussian_kernel (rt_algo.cc:902-939): the float overloads of sqrt / log / exp, Simpson's rule over each pixel, the total in double
int tb_gaussian_kernel(float sigma, float *coef)
{
    const float threshold = 0.005f;
    const int sz = (int(std::floor(1 + 2 * std::sqrt(-2.f * (sigma * sigma) * std::log(threshold)))) + 1) | 1;
    if (sz > TB_MAX_K) return sz;
    const float two_sigma2 = 2.f * (sigma * sigma);
    const auto gauss = [two_sigma2](float x) -> float { return std::exp(-(x * x) / two_sigma2); };
    const auto gauss_integral = [&](float a, float b) -> float { return ((b - a) / 6.f) * (gauss(a) + 4.f * gauss((a + b) / 2.f) + gauss(b)); };
    std::vector<float> row(sz);
    const float halfsz = float(sz / 2);
    for (int i = 0; i < sz; ++i) {
        const float x = float(i) - halfsz;
        row[i] = gauss_integral(x - 0.5f, x + 0.5f);
    }
    double totd = 0.0;
    for (int i = 0; i < sz; ++i)
        for (int j = 0; j < sz; ++j) {
            const float val = row[i] * row[j];
            coef[i * sz + j] = val;
            totd += val;
        }
    const float tot = totd;
    for (int i = 0; i < sz * sz; ++i) coef[i] /= tot;
    return sz;
}

} // namespace artgpu
