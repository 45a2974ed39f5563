// art_amd/csrc/sharpen.hip -- capture sharpening on gfx950: ImProcFunctions::doSharpening for method "rld" (rtengine/ipsharpen.cc:144-229,
// 315-340,712-788), the GAUSS_DIV / GAUSS_MULT forms of gaussianBlur it is made of (gauss.cc:52-92,177-443,860-1146,1437-1523), markImpulse
// (rt_algo.cc:497-596), get_luminance / multiply (rt_algo.cc:942-976) and calcRadiusBayer (deconvautoradius.cc:39-96).
//
//   rl_iter<R>      one Richardson-Lucy iteration of the stencil regimes (R = 1, 2, 3: 3x3, 5x5, 7x7) in one kernel: a workgroup stages its
//                   64 x 32 tile of the estimate with a halo of 2R in LDS, forms l / blur(estimate) on tile + R in LDS (the DIV form, with
//                   its edge formulas and its ring of ones at image coordinates), multiplies the estimate by the blur of that (the MULT form)
//                   and runs check_stop.  The estimate ping-pongs between two planes: a neighbouring tile's DIV stage reads what this tile's
//                   MULT stage would overwrite.  Per pixel: estimate in (with halo, mostly L2), l, out in; estimate out; out only on a freeze.
//   gauss_div<R> / gauss_mult<R>   the same forms as kernels of their own (artgpu_gaussian_blur_ex; the two-kernel form of an iteration)
//   yvv_div / yvv_mult / rl_point  sigma > 1.15: the recurrences are the shared YvV kernels (nlmeans.hip), untouched; what
//                   gaussVerticalSsediv / gaussVerticalSsemult do with the blurred value is pointwise and runs behind them
//   impulse         the 25-term sum of |src - lpf| in row-major order, three column ranges, sign-bit test in the 4-wide group's columns
// Every sum is written in the reference's order and compiled with -ffp-contract=off: the results are the reference's bits.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include "devmath.h"
#include "devsleef.h"
#include "sharpen.h"

namespace artgpu {
namespace {

constexpr int RL_TW = 64, RL_TH = 32;      // tile of rl_iter_kernel

template <int R>
__device__ __forceinline__ float sh_stencil(const float *p, int st, const ShCoef &k)
{
    if constexpr (R == 1) {
        return k.c[2] * (p[-st - 1] + p[-st + 1] + p[st - 1] + p[st + 1]) + k.c[1] * (p[-st] + p[-1] + p[1] + p[st]) + k.c[0] * p[0];
    } else if constexpr (R == 2) {
        const float c21 = k.c[0], c20 = k.c[1], c11 = k.c[2], c10 = k.c[3], c00 = k.c[4];
        return c21 * (p[-2 * st - 1] + p[-2 * st + 1] + p[-st - 2] + p[-st + 2] + p[st - 2] + p[st + 2] + p[2 * st - 1] + p[2 * st + 1]) +
               c20 * (p[-2 * st] + p[-2] + p[2] + p[2 * st]) +
               c11 * (p[-st - 1] + p[-st + 1] + p[st - 1] + p[st + 1]) +
               c10 * (p[-st] + p[-1] + p[1] + p[st]) +
               c00 * p[0];
    } else {
        const float c31 = k.c[0], c30 = k.c[1], c22 = k.c[2], c21 = k.c[3], c20 = k.c[4], c11 = k.c[5], c10 = k.c[6], c00 = k.c[7];
        // (the c21 inside the c21 group is the reference's, gauss.cc:302 and 404)
        return c31 * (p[-3 * st - 1] + p[-3 * st + 1] + p[-st - 3] + p[-st + 3] + p[st - 3] + p[st + 3] + p[3 * st - 1] + p[3 * st + 1]) +
               c30 * (p[-3 * st] + p[-3] + p[3] + p[3 * st]) +
               c22 * (p[-2 * st - 2] + p[-2 * st + 2] + p[2 * st - 2] + p[2 * st + 2]) +
               c21 * (p[-2 * st - 1] + p[-2 * st + 1] * c21 + p[-st - 2] + p[-st + 2] + p[st - 2] + p[st + 2] + p[2 * st - 1] + p[2 * st + 1]) +
               c20 * (p[-2 * st] + p[-2] + p[2] + p[2 * st]) +
               c11 * (p[-st - 1] + p[-st + 1] + p[st - 1] + p[st + 1]) +
               c10 * (p[-st] + p[-1] + p[1] + p[st]) +
               c00 * p[0];
    }
}
// the blurred value at image position (i, j) as the 3x3 forms see it: corners the pixel itself, edges the 3-tap border kernel (gauss.cc:177-274)
__device__ __forceinline__ float sh_blur3(const float *p, int st, int i, int j, int W, int H, const ShCoef &k)
{
    const bool rowedge = i == 0 || i == H - 1, coledge = j == 0 || j == W - 1;
    if (rowedge) return coledge ? p[0] : k.b1 * (p[-1] + p[1]) + k.b0 * p[0];
    if (coledge) return k.b1 * (p[-st] + p[st]) + k.b0 * p[0];
    return sh_stencil<1>(p, st, k);
}
// GAUSS_DIV at (i, j): p = the blur's source at that pixel, d = divBuffer[i][j]
template <int R>
__device__ __forceinline__ float sh_div_at(const float *p, int st, float d, int i, int j, int W, int H, const ShCoef &k)
{
    if constexpr (R == 1) {
        const float v = sh_blur3(p, st, i, j, W, H, k);
        return std_max(d / (v > 0.f ? v : 1.f), 0.f);
    } else {
        if (i < R || i >= H - R || j < R || j >= W - R) return 1.f;         // the ring of ones (L296, L310, L318-327; L348, L359, L367-376)
        return d / std_max(sh_stencil<R>(p, st, k), 0.00001f);
    }
}
// GAUSS_MULT at (i, j): false where the form leaves dst alone (the ring of the 5x5 / 7x7 forms)
template <int R>
__device__ __forceinline__ bool sh_mult_at(const float *p, int st, int i, int j, int W, int H, const ShCoef &k, float &v)
{
    if constexpr (R == 1) { v = sh_blur3(p, st, i, j, W, H, k); return true; }
    else {
        if (i < R || i >= H - R || j < R || j >= W - R) return false;
        v = sh_stencil<R>(p, st, k);
        return true;
    }
}

// get_output / check_stop (ipsharpen.cc:176-196)
__device__ __forceinline__ float sh_get_output(float est, float l, float blend, unsigned char imp, float amount)
{
    if (est != est) return l;
    const float b = imp ? 0.f : blend * amount;
    return intp(b, std_max(est, 0.f), l);
}
__device__ __forceinline__ void sh_check_stop(const ShRlArgs &a, size_t p, float est, float l)
{
    const float o = a.out[p];
    if (o != o) {
        const float delta = l * 0.2f;
        if (fabsf(est - l) > delta) a.out[p] = sh_get_output(est, l, a.blend[p], a.impulse[p], a.amount);
    }
}

__global__ void __launch_bounds__(256) rl_init_kernel(float *lum, float *est, float *out, int W, int H)
{
    FOR_IMAGE_XY(y, x, W, H) {
        const size_t p = (size_t)y * W + x;
        const float l = lum[p] + 1000.f;
        lum[p] = l;
        est[p] = std_max(l, 0.f);
        out[p] = __builtin_nanf("");
    }
}

template <int R>
__global__ void __launch_bounds__(256) rl_iter_kernel(ShRlArgs a)
{
    constexpr int EW = RL_TW + 4 * R, EH = RL_TH + 4 * R, QW = RL_TW + 2 * R, QH = RL_TH + 2 * R;
    __shared__ float est[EH * EW];
    __shared__ float rat[QH * QW];
    const int W = a.W, H = a.H;
    const int x0 = blockIdx.x * RL_TW, y0 = blockIdx.y * RL_TH;
    for (int idx = threadIdx.x; idx < EH * EW; idx += 256) {
        const int r = idx / EW, c = idx - r * EW;
        const int gy = y0 - 2 * R + r, gx = x0 - 2 * R + c;
        est[idx] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? a.est_in[(size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    // the DIV form on tile + R: a position inside the image reads neighbours inside the image only, all of them inside the staged tile
    for (int idx = threadIdx.x; idx < QH * QW; idx += 256) {
        const int r = idx / QW, c = idx - r * QW;
        const int gy = y0 - R + r, gx = x0 - R + c;
        float q = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) q = sh_div_at<R>(&est[(r + R) * EW + c + R], EW, a.lum[(size_t)gy * W + gx], gy, gx, W, H, a.k);
        rat[idx] = q;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < RL_TH * RL_TW; idx += 256) {
        const int r = idx / RL_TW, c = idx - r * RL_TW;
        const int gy = y0 + r, gx = x0 + c;
        if (gy >= H || gx >= W) continue;
        const size_t p = (size_t)gy * W + gx;
        float e = est[(r + 2 * R) * EW + c + 2 * R], v;
        if (sh_mult_at<R>(&rat[(r + R) * QW + c + R], QW, gy, gx, W, H, a.k, v)) e = e * v;
        a.est_out[p] = e;
        sh_check_stop(a, p, e, a.lum[p]);
    }
}

// est *= ratio (mult), then check_stop: behind the YvV blur of the ratio, behind gauss_mult of the two-kernel form (mult == 0), and as the
// whole iteration where the blur is a copy
__global__ void __launch_bounds__(256) rl_point_kernel(ShRlArgs a, int mult)
{
    FOR_IMAGE_XY(y, x, a.W, a.H) {
        const size_t p = (size_t)y * a.W + x;
        float e = a.est_in[p];
        if (mult) { e = e * a.ratio[p]; a.est_out[p] = e; }
        sh_check_stop(a, p, e, a.lum[p]);
    }
}

__global__ void __launch_bounds__(256) rl_final_kernel(float *lum, const float *est, const float *out, const float *blend, const unsigned char *impulse, float amount, int W, int H)
{
    FOR_IMAGE_XY(y, x, W, H) {
        const size_t p = (size_t)y * W + x;
        float l = out[p];
        if (l != l) l = sh_get_output(est[p], lum[p], blend[p], impulse[p], amount);
        lum[p] = std_max(l - 1000.f, 0.f);
    }
}

template <int R>
__global__ void __launch_bounds__(256) gauss_div_kernel(const float *src, float *dst, const float *div, int W, int H, ShCoef k)
{
    FOR_IMAGE_XY(y, x, W, H) {
        const size_t p = (size_t)y * W + x;
        dst[p] = sh_div_at<R>(src + p, W, div[p], y, x, W, H, k);
    }
}
template <int R>
__global__ void __launch_bounds__(256) gauss_mult_kernel(const float *src, float *dst, int W, int H, ShCoef k)
{
    FOR_IMAGE_XY(y, x, W, H) {
        const size_t p = (size_t)y * W + x;
        float v;
        if (sh_mult_at<R>(src + p, W, y, x, W, H, k, v)) dst[p] = dst[p] * v;
    }
}
// gaussVerticalSsediv's stores (gauss.cc:1079-1140): the 8-column groups take _mm_max_ps against zero except in their last three rows,
// the columns behind them rtengine::max in every row
__global__ void __launch_bounds__(256) yvv_div_kernel(float *blur, const float *div, int W, int H)
{
    const int wvec = W - W % 8;
    FOR_IMAGE_XY(y, x, W, H) {
        const size_t p = (size_t)y * W + x;
        const float v = blur[p];
        const float q = div[p] / (v > 0.f ? v : 1.f);
        blur[p] = x < wvec ? (y >= H - 3 ? q : sse_max(q, 0.f)) : std_max(q, 0.f);
    }
}
__global__ void __launch_bounds__(256) yvv_mult_kernel(const float *blur, float *dst, int W, int H)
{
    FOR_IMAGE_XY(y, x, W, H) {
        const size_t p = (size_t)y * W + x;
        dst[p] = dst[p] * blur[p];
    }
}

__global__ void __launch_bounds__(256) sh_luminance_kernel(ShImage im, float w0, float w1, float w2, float *Y)
{
    FOR_IMAGE_XY(y, x, im.W, im.H) {
        const size_t i = (size_t)y * im.stride + x;
        Y[(size_t)y * im.W + x] = im.p[0][i] * w0 + im.p[1][i] * w1 + im.p[2][i] * w2;
    }
}
__global__ void __launch_bounds__(256) sh_hpf_kernel(const float *Y, float *lpf, int W, int H)
{
    FOR_IMAGE_XY(y, x, W, H) {
        const size_t p = (size_t)y * W + x;
        lpf[p] = fabsf(Y[p] - lpf[p]);
    }
}
// markImpulse's test (rt_algo.cc:534-592) on hpf = |src - lpf|
__global__ void __launch_bounds__(256) sh_impulse_kernel(const float *hpf, unsigned char *impulse, int W, int H, float thr)
{
    const int nvec = W - 5 > 2 ? 4 * ((W - 7 + 3) / 4) : 0;      // columns [2, 2 + nvec) are covered by the 4-wide loop
    FOR_IMAGE_XY(i, j, W, H) {
        const int i0 = max(0, i - 2), i1 = min(i + 2, H - 1);
        const int j0 = j < 2 ? 0 : j - 2, j1 = j >= W - 2 ? W - 1 : j + 2;
        float sum = 0.f;
        for (int r = i0; r <= i1; ++r)
            for (int c = j0; c <= j1; ++c) sum += hpf[(size_t)r * W + c];
        const float h = hpf[(size_t)i * W + j];
        unsigned char m;
        if (j >= 2 && j < 2 + nvec) m = (unsigned char)(__float_as_uint((sum - h) * thr - h) >> 31);       // _mm_movemask_ps
        else m = h > (sum - h) * thr ? 1 : 0;
        impulse[(size_t)i * W + j] = m;
    }
}
__global__ void __launch_bounds__(256) sh_corner_kernel(ShCornerArgs a)
{
    FOR_IMAGE_XY(y, x, a.W, a.H) {
        const int xx = x + a.ox - a.w2, yy = y + a.oy - a.h2;
        const float distance = sqrtf((float)(xx * xx + yy * yy));
        const float blend = 1.f - lim01(xexpf_s(-sqr(std_max(distance - a.r2, 0.f)) / a.sigma));
        const size_t p = (size_t)y * a.W + x;
        a.YY[p] = intp(blend, a.YY2[p], a.YY[p]);
    }
}
__global__ void __launch_bounds__(256) sh_multiply_kernel(ShImage im, const float *num, const float *den)
{
    FOR_IMAGE_XY(y, x, im.W, im.H) {
        const size_t p = (size_t)y * im.W + x, i = (size_t)y * im.stride + x;
        const float d = den[p];
        if (d > 0.f) {
            const float f = num[p] / d;
            im.p[0][i] *= f; im.p[1][i] *= f; im.p[2][i] *= f;
        }
    }
}
__global__ void __launch_bounds__(256) sh_count_kernel(const unsigned char *impulse, const float *out, size_t n, unsigned long long *counters)
{
    __shared__ unsigned cnt[2];
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    unsigned ci = 0, co = 0;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (size_t)gridDim.x * 256) {
        if (impulse && impulse[p]) ++ci;
        if (out) { const float o = out[p]; if (o == o) ++co; }
    }
    if (ci) atomicAdd(&cnt[0], ci);
    if (co) atomicAdd(&cnt[1], co);
    __syncthreads();
    if (threadIdx.x == 0 && cnt[0]) atomicAdd(&counters[0], (unsigned long long)cnt[0]);
    if (threadIdx.x == 1 && cnt[1]) atomicAdd(&counters[1], (unsigned long long)cnt[1]);
}

// max over a workgroup; every thread returns it
__device__ __forceinline__ float sh_block_max(float m, float *lds)
{
    lds[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) lds[threadIdx.x] = std_max(lds[threadIdx.x], lds[threadIdx.x + s]);
        __syncthreads();
    }
    return lds[0];
}
// calcRadiusBayer (deconvautoradius.cc:46-89) as a pure maximum: every pair of a green site with a diagonal neighbour that is positive, above
// the lower limit and not next to a clipped value gives maxVal / minVal
__global__ void __launch_bounds__(256) sh_radius_partial_kernel(const float *raw, size_t st, int W, int H, unsigned fc0, unsigned fc1, float lower, float upper, float *partial)
{
    __shared__ float lds[256];
    float m = 1.f;
    for (int row = 4 + blockIdx.x; row < H - 4; row += gridDim.x) {
        const float *r0 = raw + (size_t)row * st;
        for (int col = 5 + (int)(((row & 1) ? fc1 : fc0) & 1) + 2 * (int)threadIdx.x; col < W - 4; col += 512) {
            const float val00 = r0[col];
            if (!(val00 > 0.f)) continue;
            const float *rm = r0 - st, *rp = r0 + st, *rpp = r0 + 2 * st;
            const float val1m1 = rp[col - 1], val1p1 = rp[col + 1];
            const float up = std_max(std_max(rm[col - 1], rm[col + 1]), val1p1);       // rtengine::max(a, b, c) = max(max(a, b), max(c))
            const float maxVal0 = std_max(val00, val1m1);
            if (val1m1 > 0.f && maxVal0 > lower) {
                const float minVal = std_min(val00, val1m1);
                const bool clipped = maxVal0 == val00 ? up >= upper
                                                      : std_max(std_max(r0[col - 2], val00), std_max(rpp[col - 2], rpp[col])) >= upper;
                if (!clipped) m = std_max(m, maxVal0 / minVal);
            }
            const float maxVal1 = std_max(val00, val1p1);
            if (val1p1 > 0.f && maxVal1 > lower) {
                const float minVal = std_min(val00, val1p1);
                const bool clipped = maxVal1 == val00 ? up >= upper
                                                      : std_max(std_max(val00, r0[col + 2]), std_max(rpp[col], rpp[col + 2])) >= upper;
                if (!clipped) m = std_max(m, maxVal1 / minVal);
            }
        }
    }
    m = sh_block_max(m, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = m;
}
__global__ void __launch_bounds__(256) sh_radius_final_kernel(const float *partial, int n, float *result)
{
    __shared__ float lds[256];
    float m = 1.f;
    for (int k = threadIdx.x; k < n; k += 256) m = std_max(m, partial[k]);
    m = sh_block_max(m, lds);
    if (threadIdx.x == 0) result[0] = m;
}

dim3 rl_grid(int W, int H) { return dim3((W + RL_TW - 1) / RL_TW, (H + RL_TH - 1) / RL_TH); }

} // namespace

// pow_F (rtengine/sleef.h:1296-1299) = xexpf(b * xlogf(a)) in the scalar forms, on the host: devsleef.h's code with host bit casts
namespace {
inline float h_i2f(int i) { float f; std::memcpy(&f, &i, 4); return f; }
inline int h_f2i(float f) { int i; std::memcpy(&i, &f, 4); return i; }
inline float h_mla(float x, float y, float z) { return x * y + z; }
inline float h_ldexpk(float x, int q)
{
    int m = q >> 31;
    m = (((m + q) >> 6) - m) << 4;
    q = q - (m << 2);
    float u = h_i2f((m + 0x7f) << 23);
    u = u * u;
    x = x * u * u;
    u = h_i2f((q + 0x7f) << 23);
    return x * u;
}
inline float h_xexpf(float d)
{
    if (d <= -104.0f) return 0.0f;
    const int q = (int)lrintf(d * ART_R_LN2f);
    float s = h_mla((float)q, -ART_L2Uf, d);
    s = h_mla((float)q, -ART_L2Lf, s);
    float u = 0.00136324646882712841033936f;
    u = h_mla(u, s, 0.00836596917361021041870117f);
    u = h_mla(u, s, 0.0416710823774337768554688f);
    u = h_mla(u, s, 0.166665524244308471679688f);
    u = h_mla(u, s, 0.499999850988388061523438f);
    u = h_mla(s, h_mla(s, u, 1.f), 1.f);
    return h_ldexpk(u, q);
}
inline float h_xlogf(float d)
{
    float dd = d * 0.7071f;
    const bool small = dd < 5.421010862427522E-20f;
    dd = small ? 1.8446744073709552E19f * dd : dd;
    const int qe = (h_f2i(dd) >> 23) & 0xff;
    const int e = small ? qe - (64 + 0x7e) : qe - 0x7e;
    const float m = h_ldexpk(d, -e);
    const float x = (m - 1.0f) / (m + 1.0f);
    const float x2 = x * x;
    float t = 0.2371599674224853515625f;
    t = h_mla(t, x2, 0.285279005765914916992188f);
    t = h_mla(t, x2, 0.400005519390106201171875f);
    t = h_mla(t, x2, 0.666666567325592041015625f);
    t = h_mla(t, x2, 2.0f);
    float r = x * t + 0.693147180559945286226764f * (float)e;
    if (d == INFINITY) r = INFINITY;
    if (d < 0.f) r = NAN;
    if (d == 0.f) r = -INFINITY;
    return r;
}
} // namespace
float sh_pow_F(float a, float b) { return h_xexpf(b * h_xlogf(a)); }

int sh_regime(double sigma, ShCoef *k)
{
    *k = ShCoef{};
    if (sigma < 0.25) return SH_COPY;
    if (sigma < 0.6) {                                   // gauss.cc:1448-1461: doubles, passed as `const T`
        double c0 = 1.0;
        double c1 = exp(-0.5 * ((1.0 / sigma) * (1.0 / sigma)));
        double c2 = exp(-((1.0 / sigma) * (1.0 / sigma)));
        const double sum = c0 + 4.0 * (c1 + c2);
        c0 /= sum; c1 /= sum; c2 /= sum;
        double b1 = exp(-1.0 / (2.0 * sigma * sigma));
        const double bsum = 2.0 * b1 + 1.0;
        b1 /= bsum;
        const double b0 = 1.0 / bsum;
        k->c[0] = (float)c0; k->c[1] = (float)c1; k->c[2] = (float)c2; k->b0 = (float)b0; k->b1 = (float)b1;
        return SH_3X3;
    }
    if (sigma <= 1.15) {                                 // compute5x5kernel / compute7x7kernel (gauss.cc:52-92) take the sigma as float
        const bool five = sigma <= 0.84;
        const int R = five ? 2 : 3, n = 2 * R + 1;
        const float sf = (float)sigma;
        const double temp = -2.f * (sf * sf);
        const double lim = five ? (3.0 * 0.84) * (3.0 * 0.84) : (3.0 * 1.15) * (3.0 * 1.15);
        float kern[7][7];
        float sum = 0.f;
        for (int i = -R; i <= R; ++i)
            for (int j = -R; j <= R; ++j) {
                if ((i * i + j * j) <= lim) {
                    kern[i + R][j + R] = std::exp((i * i + j * j) / temp);
                    sum += kern[i + R][j + R];
                } else {
                    kern[i + R][j + R] = 0.f;
                }
            }
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) kern[i][j] /= sum;
        if (five) {
            k->c[0] = kern[0][1]; k->c[1] = kern[0][2]; k->c[2] = kern[1][1]; k->c[3] = kern[1][2]; k->c[4] = kern[2][2];
            return SH_5X5;
        }
        k->c[0] = kern[0][2]; k->c[1] = kern[0][3]; k->c[2] = kern[1][1]; k->c[3] = kern[1][2]; k->c[4] = kern[1][3];
        k->c[5] = kern[2][2]; k->c[6] = kern[2][3]; k->c[7] = kern[3][3];
        return SH_7X7;
    }
    return SH_YVV;
}

hipError_t launch_rl_init(float *lum, float *est, float *out, int W, int H, hipStream_t s)
{
    hipLaunchKernelGGL(rl_init_kernel, image_grid(W, H), dim3(256), 0, s, lum, est, out, W, H);
    return hipGetLastError();
}
hipError_t launch_rl_iter(const ShRlArgs &a, int regime, hipStream_t s)
{
    if (regime == SH_3X3) hipLaunchKernelGGL(rl_iter_kernel<1>, rl_grid(a.W, a.H), dim3(256), 0, s, a);
    else if (regime == SH_5X5) hipLaunchKernelGGL(rl_iter_kernel<2>, rl_grid(a.W, a.H), dim3(256), 0, s, a);
    else if (regime == SH_7X7) hipLaunchKernelGGL(rl_iter_kernel<3>, rl_grid(a.W, a.H), dim3(256), 0, s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
hipError_t launch_rl_point(const ShRlArgs &a, int mult, hipStream_t s)
{
    hipLaunchKernelGGL(rl_point_kernel, image_grid(a.W, a.H), dim3(256), 0, s, a, mult);
    return hipGetLastError();
}
hipError_t launch_rl_final(float *lum, const float *est, const float *out, const float *blend, const unsigned char *impulse, float amount, int W, int H, hipStream_t s)
{
    hipLaunchKernelGGL(rl_final_kernel, image_grid(W, H), dim3(256), 0, s, lum, est, out, blend, impulse, amount, W, H);
    return hipGetLastError();
}
hipError_t launch_gauss_div(const float *src, float *dst, const float *div, int W, int H, int regime, const ShCoef &k, hipStream_t s)
{
    if (regime == SH_3X3) hipLaunchKernelGGL(gauss_div_kernel<1>, image_grid(W, H), dim3(256), 0, s, src, dst, div, W, H, k);
    else if (regime == SH_5X5) hipLaunchKernelGGL(gauss_div_kernel<2>, image_grid(W, H), dim3(256), 0, s, src, dst, div, W, H, k);
    else if (regime == SH_7X7) hipLaunchKernelGGL(gauss_div_kernel<3>, image_grid(W, H), dim3(256), 0, s, src, dst, div, W, H, k);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
hipError_t launch_gauss_mult(const float *src, float *dst, int W, int H, int regime, const ShCoef &k, hipStream_t s)
{
    if (regime == SH_3X3) hipLaunchKernelGGL(gauss_mult_kernel<1>, image_grid(W, H), dim3(256), 0, s, src, dst, W, H, k);
    else if (regime == SH_5X5) hipLaunchKernelGGL(gauss_mult_kernel<2>, image_grid(W, H), dim3(256), 0, s, src, dst, W, H, k);
    else if (regime == SH_7X7) hipLaunchKernelGGL(gauss_mult_kernel<3>, image_grid(W, H), dim3(256), 0, s, src, dst, W, H, k);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
hipError_t launch_yvv_div(float *blur, const float *div, int W, int H, hipStream_t s)
{
    hipLaunchKernelGGL(yvv_div_kernel, image_grid(W, H), dim3(256), 0, s, blur, div, W, H);
    return hipGetLastError();
}
hipError_t launch_yvv_mult(const float *blur, float *dst, int W, int H, hipStream_t s)
{
    hipLaunchKernelGGL(yvv_mult_kernel, image_grid(W, H), dim3(256), 0, s, blur, dst, W, H);
    return hipGetLastError();
}
hipError_t launch_sh_luminance(const ShImage &im, const float ws1[3], float *Y, hipStream_t s)
{
    hipLaunchKernelGGL(sh_luminance_kernel, image_grid(im.W, im.H), dim3(256), 0, s, im, ws1[0], ws1[1], ws1[2], Y);
    return hipGetLastError();
}
hipError_t launch_sh_impulse(const float *Y, float *lpf, unsigned char *impulse, int W, int H, float thresh, hipStream_t s)
{
    const float impthr = std::max(1.f, 5.5f - thresh);
    const float impthrDiv24 = impthr / 24.0f;
    hipLaunchKernelGGL(sh_hpf_kernel, image_grid(W, H), dim3(256), 0, s, Y, lpf, W, H);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(sh_impulse_kernel, image_grid(W, H), dim3(256), 0, s, lpf, impulse, W, H, impthrDiv24);
    return hipGetLastError();
}
hipError_t launch_sh_corner(const ShCornerArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(sh_corner_kernel, image_grid(a.W, a.H), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_sh_multiply(const ShImage &im, const float *num, const float *den, hipStream_t s)
{
    hipLaunchKernelGGL(sh_multiply_kernel, image_grid(im.W, im.H), dim3(256), 0, s, im, num, den);
    return hipGetLastError();
}
hipError_t launch_sh_count(const unsigned char *impulse, const float *out, size_t n, unsigned long long *counters, hipStream_t s)
{
    const size_t g = (n + 255) / 256;
    hipLaunchKernelGGL(sh_count_kernel, dim3((unsigned)(g < 4096 ? (g ? g : 1) : 4096)), dim3(256), 0, s, impulse, out, n, counters);
    return hipGetLastError();
}
hipError_t launch_sh_radius(const float *raw, size_t stride, int W, int H, unsigned fc0, unsigned fc1, float lower, float upper, float *partial, float *result, hipStream_t s)
{
    const int rows = H - 8;
    const int np = rows < 1 ? 1 : (rows < SH_RADIUS_PARTIALS ? rows : SH_RADIUS_PARTIALS);
    hipLaunchKernelGGL(sh_radius_partial_kernel, dim3(np), dim3(256), 0, s, raw, stride, W, H, fc0, fc1, lower, upper, partial);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(sh_radius_final_kernel, dim3(1), dim3(256), 0, s, partial, np, result);
    return hipGetLastError();
}

} // namespace artgpu
