// art_amd/csrc/dehaze.hip -- ImProcFunctions::dehaze on gfx950 (reference: rtengine/ipdehaze.cc:64-512, the dark channel prior of
// He, Sun and Tang with a guided filter for the transmission map; rtengine/guidedfilter.cc:58-241; rtengine/rescale.h:27-92).
//
// The tool has no device-side libm call and no floating-point sum: its reductions are max and min, exact in any order for NaN-free
// input, so every kernel here gives the reference's bits.  What the reference stores and reads again but a kernel can recompute
// is not stored: the three self-guided channels R, G, B of extract_channels are evaluated where they are read (the thumbnail
// gather and the dark channel) from the quarter- to full-size mean a / mean b planes, the add_haze plane is the sign of a strength
// the recovery pass looks up again, and the last guided filter's output exists only inside the recovery pass.
// The box blurs are the shared hblur / vblur kernels of denoise.hip.
#include <hip/hip_runtime.h>
#include "devmath.h"
#include "devsleef.h"
#include "dehaze.h"
#include "kernels.h"
#include <algorithm>
#include <cmath>
#include <limits>
#include <mutex>
#include <vector>

namespace artgpu {

namespace {

constexpr float DH_INF = __builtin_huge_valf();     // RT_INFINITY_F

// rt_math.h:55-82
__device__ __forceinline__ float min3(float a, float b, float c) { return std_min(std_min(a, b), c); }
__device__ __forceinline__ float min4(float a, float b, float c, float d) { return std_min(std_min(a, b), std_min(c, d)); }
__device__ __forceinline__ float max3(float a, float b, float c) { return std_max(std_max(a, b), c); }
__device__ __forceinline__ float max4(float a, float b, float c, float d) { return std_max(std_max(a, b), std_max(c, d)); }

// the maximum / minimum of a 256-thread workgroup's values, in lane 0
__device__ __forceinline__ float block_max(float v, float *lds)
{
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) lds[t] = std_max(lds[t], lds[t + s]);
        __syncthreads();
    }
    const float r = lds[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ float block_min(float v, float *lds)
{
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) lds[t] = std_min(lds[t], lds[t + s]);
        __syncthreads();
    }
    const float r = lds[0];
    __syncthreads();
    return r;
}

// normalize (L64-80), the maximum: rows blockIdx.x, blockIdx.x + gridDim.x, ... -> partial[blockIdx.x]
__global__ void __launch_bounds__(256) dh_max_partial_kernel(DhImage im, float *partial)
{
    __shared__ float lds[256];
    float m = 0.f;
    for (int y = blockIdx.x; y < im.H; y += gridDim.x) {
        const size_t ro = (size_t)y * im.stride;
        for (int x = threadIdx.x; x < im.W; x += 256) m = max4(m, im.p[0][ro + x], im.p[1][ro + x], im.p[2][ro + x]);
    }
    m = block_max(m, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = m;
}
__global__ void __launch_bounds__(256) dh_max_final_kernel(const float *partial, int n, DhState *st)
{
    __shared__ float lds[256];
    float m = 0.f;
    for (int k = threadIdx.x; k < n; k += 256) m = std_max(m, partial[k]);
    m = block_max(m, lds);
    if (threadIdx.x == 0) {
        const float maxval = std_max(m * 2.f, 65535.f);
        st->maxval = maxval;
        st->inv_maxval = 1.f / maxval;
        st->black[0] = st->black[1] = st->black[2] = 0.f;
    }
}

// rescaleNearest (rescale.h:77-92) to ww x hh: of the image times 1 / maxval (subtract_black, L264-266), or of the three guided
// filters' outputs (L379-381)
__global__ void __launch_bounds__(256) dh_thumb_kernel(DhThumbArgs a)
{
    const float inv = a.st->inv_maxval;
    const float col_scale = (float)a.gf.w / (float)a.im.W, row_scale = (float)a.gf.h / (float)a.im.H;
    const size_t n = (size_t)a.ww * a.hh;
    FOR_IMAGE_XY(y, x, a.ww, a.hh) {
        const int sy = y * a.im.H / a.hh, sx = x * a.im.W / a.ww;
        const size_t si = (size_t)sy * a.im.stride + sx, di = (size_t)y * a.ww + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = a.im.p[c][si];
            a.thumb[c * n + di] = a.from_q ? dh_q(a.gf.low + (2 * c) * a.gf.nl, a.gf.low + (2 * c + 1) * a.gf.nl, a.gf.w, a.gf.h, col_scale, sy * row_scale, sx, v)
                                           : v * inv;
        }
    }
}

// subtract_black's black points (L273-285) from the blurred thumbnail planes: workgroup c takes plane c
__global__ void __launch_bounds__(256) dh_black_kernel(const float *thumb, int n, float scaling, DhState *st)
{
    __shared__ float lds[256];
    const float *p = thumb + (size_t)blockIdx.x * n;
    float m = DH_INF;
    for (int k = threadIdx.x; k < n; k += 256) m = std_min(m, p[k]);
    m = block_min(m, lds);
    if (threadIdx.x == 0) st->black[blockIdx.x] = std_max(0.f, m * scaling);
}

// Imagefloat::multiply(1.f / maxval) (L78) and subtract_black's pixel loop (L294-300) in one pass
__global__ void __launch_bounds__(256) dh_normalize_kernel(DhImage im, const DhState *st, int has_black)
{
    const float inv = st->inv_maxval;
    const float b0 = st->black[0], b1 = st->black[1], b2 = st->black[2];
    FOR_IMAGE_XY(y, x, im.W, im.H) {
        const size_t i = (size_t)y * im.stride + x;
        float r = im.p[0][i] * inv, g = im.p[1][i] * inv, b = im.p[2][i] * inv;
        if (has_black) { r = std_max(r - b0, 0.f); g = std_max(g - b1, 0.f); b = std_max(b - b2, 0.f); }
        im.p[0][i] = r; im.p[1][i] = g; im.p[2][i] = b;
    }
}

// restore (L83-86) on its own: the "no haze" return (L387-393)
__global__ void __launch_bounds__(256) dh_restore_kernel(DhImage im, const DhState *st)
{
    const float maxval = st->maxval;
    FOR_IMAGE_XY(y, x, im.W, im.H) {
        const size_t i = (size_t)y * im.stride + x;
        im.p[0][i] *= maxval; im.p[1][i] *= maxval; im.p[2][i] *= maxval;
    }
}

// guidedFilter's I1, p1 and their products on the w x h grid (guidedfilter.cc:186-204).  src == nullptr: the three self-guided filters
// of extract_channels (L233-246), where p1 is I1 and the planes of meanp / corrIp would repeat meanI / corrI bit for bit
__global__ void __launch_bounds__(256) dh_gf_subsample_kernel(DhImage im, const float *src, size_t src_stride, DhGuided gf)
{
    const float col_scale = (float)im.W / (float)gf.w, row_scale = (float)im.H / (float)gf.h;
    const bool same = gf.w == im.W && gf.h == im.H;
    FOR_IMAGE_XY(y, x, gf.w, gf.h) {
        const size_t t = (size_t)y * gf.w + x;
        const float fx = x * col_scale, fy = y * row_scale;
        if (!src) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float I1 = same ? im.p[c][(size_t)y * im.stride + x] : dh_bilinear(im.p[c], im.stride, im.W, im.H, fx, fy);
                gf.low[(2 * c) * gf.nl + t] = I1;
                gf.low[(2 * c + 1) * gf.nl + t] = I1 * I1;
            }
        } else {
            const float I1 = same ? im.p[2][(size_t)y * im.stride + x] : dh_bilinear(im.p[2], im.stride, im.W, im.H, fx, fy);      // guide: the blue plane (L443)
            const float p1 = same ? src[(size_t)y * src_stride + x] : dh_bilinear(src, src_stride, im.W, im.H, fx, fy);
            gf.low[t] = I1;
            gf.low[gf.nl + t] = I1 * I1;
            gf.low[2 * gf.nl + t] = p1;
            gf.low[3 * gf.nl + t] = I1 * p1;
        }
    }
}

// a = covIp / (varI + epsilon), b = meanp - a * meanI (guidedfilter.cc:206-220), written where the next blurs read them
__global__ void __launch_bounds__(256) dh_gf_ab_kernel(DhGuided gf, int self3)
{
    const size_t n = gf.nl;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x) {
        if (self3) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float meanI = gf.low[(2 * c) * n + t], corrI = gf.low[(2 * c + 1) * n + t];
                const float varI = corrI - (meanI * meanI);
                const float covIp = corrI - (meanI * meanI);          // corrIp - meanI * meanp with p = I
                const float av = covIp / (varI + gf.eps);
                gf.low[(2 * c) * n + t] = av;
                gf.low[(2 * c + 1) * n + t] = meanI - (av * meanI);
            }
        } else {
            const float meanI = gf.low[t], corrI = gf.low[n + t], meanp = gf.low[2 * n + t], corrIp = gf.low[3 * n + t];
            const float varI = corrI - (meanI * meanI);
            const float covIp = corrIp - (meanI * meanp);
            const float av = covIp / (varI + gf.eps);
            gf.low[2 * n + t] = av;
            gf.low[3 * n + t] = meanp - (av * meanI);
        }
    }
}

// get_dark_channel (L89-125), one value per patch.  A workgroup takes a row of patches, (256 / patch) of them at a time: a lane
// walks one pixel column of the patch row (coalesced along x), the patch's first lane then folds its `patch` columns.
// Without a non-positive ambient component the division is taken once per channel and patch: x -> x / a is monotonic for a > 0, so
// min(r / a) and min(r) / a are the same float.  FROMQ: the planes are the three guided filters' outputs, evaluated here.
template <bool FROMQ>
__global__ void __launch_bounds__(256) dh_dark_kernel(DhDarkArgs a)
{
    __shared__ float lds[3][256];
    const int p = a.patch, npb = 256 / p, seg = npb * p, tid = threadIdx.x;
    const int W = a.im.W, H = a.im.H;
    const float col_scale = FROMQ ? (float)a.gf.w / (float)W : 0.f, row_scale = FROMQ ? (float)a.gf.h / (float)H : 0.f;
    const bool divide = a.has_ambient && !a.per_pixel;
    for (int py = blockIdx.y; py < a.npy; py += gridDim.y) {
        const int y0 = py * p, y1 = min(y0 + p, H);
        for (int pb = blockIdx.x; pb * npb < a.npx; pb += gridDim.x) {
            const int x = pb * seg + tid;
            const bool active = tid < seg && x < W;
            float m0 = DH_INF, m1 = DH_INF, m2 = DH_INF;
            if (active) {
                for (int yy = y0; yy < y1; ++yy) {
                    const size_t i = (size_t)yy * a.im.stride + x;
                    float r = a.im.p[0][i], g = a.im.p[1][i], b = a.im.p[2][i];
                    if (FROMQ) {
                        const float ymrs = yy * row_scale;
                        r = dh_q(a.gf.low, a.gf.low + a.gf.nl, a.gf.w, a.gf.h, col_scale, ymrs, x, r);
                        g = dh_q(a.gf.low + 2 * a.gf.nl, a.gf.low + 3 * a.gf.nl, a.gf.w, a.gf.h, col_scale, ymrs, x, g);
                        b = dh_q(a.gf.low + 4 * a.gf.nl, a.gf.low + 5 * a.gf.nl, a.gf.w, a.gf.h, col_scale, ymrs, x, b);
                    }
                    if (a.per_pixel) {
                        r /= a.ambient[0]; g /= a.ambient[1]; b /= a.ambient[2];
                        m0 = min4(m0, r, g, b);
                    } else {
                        m0 = std_min(m0, r); m1 = std_min(m1, g); m2 = std_min(m2, b);
                    }
                }
            }
            lds[0][tid] = m0; lds[1][tid] = m1; lds[2][tid] = m2;
            __syncthreads();
            if (active && tid % p == 0) {
                const int cnt = min(p, W - x);
                for (int k = 1; k < cnt; ++k) { m0 = std_min(m0, lds[0][tid + k]); m1 = std_min(m1, lds[1][tid + k]); m2 = std_min(m2, lds[2][tid + k]); }
                if (divide) { m0 /= a.ambient[0]; m1 /= a.ambient[1]; m2 /= a.ambient[2]; }
                float val = a.per_pixel ? m0 : min3(m0, m1, m2);
                if (a.clip) val = lim01(val);
                a.grid[(size_t)py * a.npx + x / p] = val;
            }
            __syncthreads();
        }
    }
}

// std::fill of the patch value (L118-120): the exported dark channel's full-size plane
__global__ void __launch_bounds__(256) dh_expand_kernel(DhExpandArgs a)
{
    FOR_IMAGE_XY(y, x, a.W, a.H) a.dst[(size_t)y * a.dst_stride + x] = a.grid[(size_t)(y / a.patch) * a.npx + x / a.patch];
}

// t~ = 1 - |s| * dark, s = strength[Y * maxchan] (L429-436)
__global__ void __launch_bounds__(256) dh_transmission_kernel(DhTransArgs a)
{
    const float maxchan = a.st->maxval;
    FOR_IMAGE_XY(y, x, a.im.W, a.im.H) {
        const size_t i = (size_t)y * a.im.stride + x;
        const float r = a.im.p[0][i], g = a.im.p[1][i], b = a.im.p[2][i];
        const float Y = (float)(r * a.ws1[0] + g * a.ws1[1] + b * a.ws1[2]) * maxchan;
        const float s = lutf_lookup<true>(a.lut, 65536, Y);
        a.t[(size_t)y * a.im.W + x] = 1.f - fabsf(s) * a.grid[(size_t)(y / a.patch) * a.npx + x / a.patch];
    }
}

// the last guided filter's output t (L444), the recovery loop (L461-509) and restore (L511) in one pass
__global__ void __launch_bounds__(256) dh_recover_kernel(DhRecoverArgs a)
{
    const float maxchan = a.st->maxval;
    const float col_scale = (float)a.gf.w / (float)a.im.W, row_scale = (float)a.gf.h / (float)a.im.H;
    const float *ma = a.gf.low + 2 * a.gf.nl, *mb = a.gf.low + 3 * a.gf.nl;
    const float teps = 1e-6f;
    FOR_IMAGE_XY(y, x, a.im.W, a.im.H) {
        const size_t i = (size_t)y * a.im.stride + x;
        const float r = a.im.p[0][i], g = a.im.p[1][i], b = a.im.p[2][i];
        const float t = dh_q(ma, mb, a.gf.w, a.gf.h, col_scale, y * row_scale, x, b);
        const float tl = 1.f - min3(r / a.ambient[0], g / a.ambient[1], b / a.ambient[2]);
        const float mt = max3(t, a.t0, tl + teps);
        float o0 = r, o1 = g, o2 = b;
        if (a.show_depth_map) {
            o0 = o1 = o2 = lim01(1.f - mt);
        } else {
            const float Y = (float)(r * a.ws1[0] + g * a.ws1[1] + b * a.ws1[2]);
            const bool add_haze = lutf_lookup<true>(a.lut, 65536, Y * maxchan) < 0;
            if (a.luminance) {
                float YY = (Y - a.ambientY) / mt + a.ambientY;
                if (Y > 1e-5f) {
                    if (add_haze) YY = Y + Y - YY;
                    const float f = YY / Y;
                    o0 = r * f; o1 = g * f; o2 = b * f;
                }
            } else {
                const float rr = (r - a.ambient[0]) / mt + a.ambient[0];
                const float gg = (g - a.ambient[1]) / mt + a.ambient[1];
                const float bb = (b - a.ambient[2]) / mt + a.ambient[2];
                if (add_haze) { o0 = r + (r - rr); o1 = g + (g - gg); o2 = b + (b - bb); }
                else { o0 = rr; o1 = gg; o2 = bb; }
            }
        }
        a.im.p[0][i] = o0 * maxchan; a.im.p[1][i] = o1 * maxchan; a.im.p[2][i] = o2 * maxchan;
    }
}

} // namespace

hipError_t launch_dh_max(const DhImage &im, float *partial, int npartial, DhState *st, hipStream_t s)
{
    hipLaunchKernelGGL(dh_max_partial_kernel, dim3(npartial), dim3(256), 0, s, im, partial);
    hipLaunchKernelGGL(dh_max_final_kernel, dim3(1), dim3(256), 0, s, partial, npartial, st);
    return hipGetLastError();
}
hipError_t launch_dh_thumb(const DhThumbArgs &a, hipStream_t s) { hipLaunchKernelGGL(dh_thumb_kernel, image_grid(a.ww, a.hh), dim3(256), 0, s, a); return hipGetLastError(); }
hipError_t launch_dh_black(const float *thumb, int n, float scaling, DhState *st, hipStream_t s) { hipLaunchKernelGGL(dh_black_kernel, dim3(3), dim3(256), 0, s, thumb, n, scaling, st); return hipGetLastError(); }
hipError_t launch_dh_normalize(const DhImage &im, const DhState *st, int has_black, hipStream_t s) { hipLaunchKernelGGL(dh_normalize_kernel, image_grid(im.W, im.H), dim3(256), 0, s, im, st, has_black); return hipGetLastError(); }
hipError_t launch_dh_restore(const DhImage &im, const DhState *st, hipStream_t s) { hipLaunchKernelGGL(dh_restore_kernel, image_grid(im.W, im.H), dim3(256), 0, s, im, st); return hipGetLastError(); }
hipError_t launch_dh_gf_subsample(const DhImage &im, const float *src, size_t src_stride, const DhGuided &gf, hipStream_t s)
{
    hipLaunchKernelGGL(dh_gf_subsample_kernel, image_grid(gf.w, gf.h), dim3(256), 0, s, im, src, src_stride, gf);
    return hipGetLastError();
}
hipError_t launch_dh_gf_ab(const DhGuided &gf, int self3, hipStream_t s)
{
    const size_t g = (gf.nl + 255) / 256;
    hipLaunchKernelGGL(dh_gf_ab_kernel, dim3((unsigned)(g < 16384 ? (g ? g : 1) : 16384)), dim3(256), 0, s, gf, self3);
    return hipGetLastError();
}
hipError_t launch_dh_dark(const DhDarkArgs &a, bool from_q, hipStream_t s)
{
    const int npb = 256 / a.patch, gx = (a.npx + npb - 1) / npb;
    const dim3 grid(gx < 1 ? 1 : (gx > 1024 ? 1024 : gx), a.npy < 1 ? 1 : (a.npy > 32768 ? 32768 : a.npy));
    if (from_q) hipLaunchKernelGGL(dh_dark_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(dh_dark_kernel<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_dh_expand(const DhExpandArgs &a, hipStream_t s) { hipLaunchKernelGGL(dh_expand_kernel, image_grid(a.W, a.H), dim3(256), 0, s, a); return hipGetLastError(); }
hipError_t launch_dh_transmission(const DhTransArgs &a, hipStream_t s) { hipLaunchKernelGGL(dh_transmission_kernel, image_grid(a.im.W, a.im.H), dim3(256), 0, s, a); return hipGetLastError(); }
hipError_t launch_dh_recover(const DhRecoverArgs &a, hipStream_t s) { hipLaunchKernelGGL(dh_recover_kernel, image_grid(a.im.W, a.im.H), dim3(256), 0, s, a); return hipGetLastError(); }

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------

// the thumbnail of subtract_black and of the ambient estimate: the long side 200 for landscape frames; for portrait frames ww = 200 / r is
// the LARGER number (r < 1) and hh = 200, as the reference has it
void dh_thumb_size(int W, int H, int *ww, int *hh)
{
    constexpr int sizecap = 200;
    const float r = float(W) / float(H);
    *ww = r >= 1.f ? sizecap : (int)(float(sizecap) / r);
    *hh = r >= 1.f ? (int)(float(sizecap) / r) : sizecap;
}

// strength[i] = (FlatCurve(points, false).getVal(gamma2curve[i] / 65535.f) - 0.5f) * 1.3f with identity value 0.5 (L419-424);
// Color::gamma2curve: build_gamma2curve (hostluts.hip)
void dh_strength_lut(const double *pts, int npts, float lut[65536])
{
    static std::once_flag once;
    static std::vector<float> gamma2curve;
    std::call_once(once, [] { gamma2curve.resize(65536); build_gamma2curve(gamma2curve.data()); });
    std::vector<double> x, y, slope;
    const bool curve = flat_curve_polyline(pts, npts, false, 1000, 0.5, x, y, slope);
    for (int i = 0; i < 65536; ++i) {
        double v = 0.5;
        if (curve) {
            double t = gamma2curve[i] / 65535.f;
            if (t < x[0]) t += 1.0;
            unsigned lo = 0, hi = (unsigned)x.size() - 1;
            while (hi > 1 + lo) {
                const unsigned mid = (hi + lo) / 2;
                if (x[mid] > t) hi = mid; else lo = mid;
            }
            v = y[lo] + (t - x[lo]) * slope[lo];
        }
        lut[i] = (v - 0.5f) * 1.3f;
    }
}

// get_dark_channel(RR, GG, BB, D, 2, nullptr, false) and estimate_ambient_light (L128-230) on the thumbnail; returns max_t (< 0: no haze,
// ambient then stays zero)
float dh_estimate_ambient(const float *R, const float *G, const float *B, int W, int H, float ambient[3])
{
    ambient[0] = ambient[1] = ambient[2] = 0.f;
    if (W < 1 || H < 1) return -1.f;
    constexpr int patchsize = 2;
    const int npx = (W + 1) / 2, npy = (H + 1) / 2;
    std::vector<float> dark((size_t)npx * npy);
    for (int py = 0; py < npy; ++py)
        for (int px = 0; px < npx; ++px) {
            float val = std::numeric_limits<float>::infinity();
            for (int yy = py * 2; yy < std::min(py * 2 + 2, H); ++yy)
                for (int xx = px * 2; xx < std::min(px * 2 + 2, W); ++xx) {
                    const size_t i = (size_t)yy * W + xx;
                    const float m0 = R[i] < val ? R[i] : val, m1 = B[i] < G[i] ? B[i] : G[i];
                    val = m1 < m0 ? m1 : m0;
                }
            dark[(size_t)py * npx + px] = val;
        }
    const auto oog = [](float val, float high) { return (val < 0.f) || (val > high); };
    // get_percentile: the n-th smallest value, n = LIM<size_t>(size * prcnt, 1, size) with the product taken in float
    const auto percentile = [](std::vector<float> &q, float prcnt) {
        size_t n = (size_t)(q.size() * prcnt);
        n = n > q.size() ? q.size() : n;
        n = n < 1 ? 1 : n;
        std::nth_element(q.begin(), q.begin() + (n - 1), q.end());
        return q[n - 1];
    };
    std::vector<float> q;
    for (float d : dark)
        if (!oog(d, 1.f - 1e-5f)) q.push_back(d);
    if (q.empty()) return -1.f;
    const float darklim = percentile(q, 0.95);
    std::vector<int> patches;
    for (int k = 0; k < npx * npy; ++k)
        if (dark[k] >= darklim && !oog(dark[k], 1.f)) patches.push_back(k);
    q.clear();
    for (int k : patches) {
        const int x0 = (k % npx) * patchsize, y0 = (k / npx) * patchsize;
        for (int y = y0; y < std::min(y0 + patchsize, H); ++y)
            for (int x = x0; x < std::min(x0 + patchsize, W); ++x) q.push_back(R[(size_t)y * W + x] + G[(size_t)y * W + x] + B[(size_t)y * W + x]);
    }
    if (q.empty()) return -1.f;
    const float bright_lim = percentile(q, 0.95);
    double rr = 0, gg = 0, bb = 0;
    int n = 0;
    for (int k : patches) {
        const int x0 = (k % npx) * patchsize, y0 = (k / npx) * patchsize;
        for (int y = y0; y < std::min(y0 + patchsize, H); ++y)
            for (int x = x0; x < std::min(x0 + patchsize, W); ++x) {
                const float r = R[(size_t)y * W + x], g = G[(size_t)y * W + x], b = B[(size_t)y * W + x];
                if (r + g + b >= bright_lim) { rr += r; gg += g; bb += b; ++n; }
            }
    }
    n = std::max(n, 1);
    ambient[0] = rr / n;
    ambient[1] = gg / n;
    ambient[2] = bb / n;
    return darklim > 0 ? -1.125f * std::log(darklim) : std::log(std::numeric_limits<float>::max()) / 2;     // float overloads
}

} // namespace artgpu
