// art_amd/csrc/masks.hip -- rtengine::generateMasks' parametric path on gfx950 (reference: rtengine/masks.cc:1037-1516; 696-734
// contrast_threshold_mask, 737-802 mask_postprocess, 612-636 rgb2lab by image mode; color.h:1719-1754 huelab_to_huehsv2;
// flatcurves.cc:339-365 FlatCurve::getVal; rescale.h:27-74).
//
// Every step is the reference's arithmetic in the reference's order and precision (the product of the three curve values is a double product,
// the hue remap is double, the posterization's + 0.5 is double), so the kernels give its bits.  The guided filters, buildBlendMask and the
// gaussian are the shared ones (guided.hip, dualdemosaic.hip, nlmeans.hip), composed by artgpu_generate_masks.
//
// mk_fused_kernel reads the image once and writes the guide and one blend plane per region of its group.  It is bound by the curve searches
// (up to three binary searches over ~1000 doubles per region and pixel) and the two sleef calls, not by memory, so the polylines of the
// group sit in LDS: a persistent grid of about a thousand 512-thread workgroups fills them once each.
#include <hip/hip_runtime.h>
#include "devmath.h"
#include "devsleef.h"
#include "labdev.h"
#include "dehaze.h"
#include "masks.h"
#include "kernels.h"

namespace artgpu {

namespace {

extern __shared__ double mk_tab[];

// rgb2lab by mode (L612-636): RGB and LAB
template <typename A>
__device__ __forceinline__ void mk_lab(const A &a, int y, int x, float &l, float &la, float &lb)
{
    const size_t i = (size_t)y * a.im.stride + x;
    const float R = a.im.p[0][i], G = a.im.p[1][i], B = a.im.p[2][i];
    if (a.im.lab) { l = G; la = R; lb = B; }
    else rgb2lab_px(a.wp, a.cachef, a.cachefy, R, G, B, l, la, lb);
}

// Color::huelab_to_huehsv2 (color.h:1719-1754): nine linear pieces; the segment is found in float, the piece evaluated in double.  The
// eighteen double constants sit in constant memory: as immediates they would each hold a register pair for the whole pixel loop.
__constant__ double MK_HUE_SLOPE[9] = {0.11666, 0.1125, 0.2666, 0.1489, 0.23419, 0.16, 0.12143, 0.2125, 0.1};
__constant__ double MK_HUE_OFFSET[9] = {0.93, -0.0675, -0.2833, -0.04785, 1.1557, 0.948, 0.85928, 0.94125, 0.93};
__device__ __forceinline__ double huelab_to_huehsv2(float HH)
{
    int seg = -1;
    if (HH >= 0.f && HH < 0.6f) seg = 0;
    else if (HH >= 0.6f && HH < 1.4f) seg = 1;
    else if (HH >= 1.4f && HH < 2.f) seg = 2;
    else if (HH >= 2.f && HH <= 3.14159f) seg = 3;
    else if (HH >= -3.1416f && HH < -2.8f) seg = 4;
    else if (HH >= -2.8f && HH < -2.3f) seg = 5;
    else if (HH >= -2.3f && HH < -0.9f) seg = 6;
    else if (HH >= -0.9f && HH < -0.1f) seg = 7;
    else if (HH >= -0.1f && HH < 0.f) seg = 8;
    double hr = 0.0;
    if (seg >= 0) hr = MK_HUE_SLOPE[seg] * double(HH) + MK_HUE_OFFSET[seg];
    if (hr < 0.0) hr += 1.0;
    else if (hr > 1.0) hr -= 1.0;
    return hr;
}

// FlatCurve::getVal (flatcurves.cc:339-375) on a polyline in LDS; FCT_Empty returns identityValue
__device__ __forceinline__ double mk_curve_val(const MkCurve c, double t)
{
    if (c.n < 0) return 0.5;
    const int x = c.off, y = c.off + c.n, sl = c.off + 2 * c.n;
    if (t < mk_tab[x]) t += 1.0;
    unsigned lo = 0, hi = (unsigned)c.n - 1;
    while (hi > 1 + lo) {
        const unsigned mid = (hi + lo) / 2;
        if (mk_tab[x + mid] > t) hi = mid; else lo = mid;
    }
    return mk_tab[y + lo] + (t - mk_tab[x + lo]) * mk_tab[sl + lo];
}

__global__ void __launch_bounds__(256) mk_ll_kernel(MkLLArgs a)
{
    FOR_IMAGE_XY(y, x, a.im.w, a.im.h) {
        float l, la, lb;
        mk_lab(a, y, x, l, la, lb);
        l /= 32768.f;
        const size_t i = (size_t)y * a.im.w + x;
        a.guide[i] = l;
        a.LL[i] = roundf(l * 40.f) / 40.f;
    }
}

__global__ void __launch_bounds__(MK_THREADS) mk_fused_kernel(MkFusedArgs a)
{
    for (int i = threadIdx.x; i < a.tab_len; i += MK_THREADS) mk_tab[i] = a.tab[i];
    __syncthreads();
    constexpr float c_factor = 327.68f * (42000.f / 48000.f);
    const int w = a.im.w, h = a.im.h;
    const int x = blockIdx.x * MK_THREADS + threadIdx.x;       // the grid's x covers the row: only the rows are strided over
    if (x < w)
        for (int y = blockIdx.y; y < h; y += gridDim.y) {
            float l, la, lb;
            mk_lab(a, y, x, l, la, lb);
            l /= 32768.f; la /= 42000.f; lb /= 42000.f;
            const size_t i = (size_t)y * w + x;
            a.guide[i] = lim01(l);
            if (a.nreg == 0) continue;
            float c = sqrtf(la * la + lb * lb) / 327.68f;          // Color::Lab2Lch
            float hh = xatan2f_s(lb, la);
            c *= c_factor;
            c = xlin2log(c, 50.f);
            hh = (float)huelab_to_huehsv2(hh);
            hh += 1.f / 6.f;
            if (hh > 1.f) hh -= 1.f;
            hh = xlin2log(hh, 3.f);
            const float LLv = a.LL ? a.LL[i] : 0.f;
#pragma unroll 1
            for (int r = 0; r < a.nreg; ++r) {      // (not unrolled: the regions' parameters stay in the kernel's argument block until they are used)
                const float ll = a.LL ? intp(a.ldetail[r], LLv, l) : l;
                double v = (double)1.f;                              // DeltaEEvaluator of a disabled deltaE mask
                v = v * (a.curve[r][MK_HUE].n ? mk_curve_val(a.curve[r][MK_HUE], (double)hh) : (double)1.f);
                v = v * (a.curve[r][MK_CHROMA].n ? mk_curve_val(a.curve[r][MK_CHROMA], (double)c) : (double)1.f);
                v = v * (a.curve[r][MK_LIGHT].n ? mk_curve_val(a.curve[r][MK_LIGHT], (double)ll) : (double)1.f);
                a.out[r][i] = (float)v;
            }
        }
}

__global__ void __launch_bounds__(256) mk_tail_kernel(MkTailArgs a)
{
    FOR_IMAGE_XY(y, x, a.w, a.h) {
        const size_t i = (size_t)y * a.w + x;
        float m = a.fill_one ? 1.f : a.m[i];
        if (a.clamp) m = lim01(m);
        if (a.cthr) { const float f = a.cthr_neg ? 1.f - a.cthr[i] : a.cthr[i]; m *= f; }
        if (a.area) m *= a.area[(size_t)y * a.area_stride + x];
        if (a.post_p != 0.f) m = int(m * a.post_p + 0.5) / a.post_p;
        if (a.thr_out) a.thr_out[i] = m > 1e-4f ? 1.f : a.fillval;
        if (a.thr_in) m *= a.thr_in[i];
        if (a.inverted) m = 1.f - m;
        if (a.has_opacity) m *= a.opacity;
        a.m[i] = m;
    }
}

__global__ void __launch_bounds__(256) mk_rescale_kernel(const float *src, int sw, int sh, float *dst, int dw, int dh)
{
    const float col_scale = float(sw) / float(dw), row_scale = float(sh) / float(dh);
    FOR_IMAGE_XY(y, x, dw, dh) dst[(size_t)y * dw + x] = dh_bilinear(src, sw, sw, sh, x * col_scale, y * row_scale);
}

} // namespace

hipError_t launch_mk_ll(const MkLLArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(mk_ll_kernel, image_grid(a.im.w, a.im.h), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_mk_fused(const MkFusedArgs &a, hipStream_t s)
{
    const size_t lds = (size_t)a.tab_len * sizeof(double);
    if (lds > (size_t)MK_LDS_BYTES || a.nreg < 0 || a.nreg > MK_GROUP) return hipErrorInvalidValue;
    if (lds > 64 * 1024) {
        const hipError_t e = dyn_lds_once(reinterpret_cast<const void *>(mk_fused_kernel), MK_LDS_BYTES);
        if (e != hipSuccess) return e;
    }
    const int gx = (a.im.w + MK_THREADS - 1) / MK_THREADS;
    int gy = gx < 1024 ? 1024 / gx : 1;
    gy = a.im.h < gy ? a.im.h : gy;
    hipLaunchKernelGGL(mk_fused_kernel, dim3(gx, gy), dim3(MK_THREADS), lds, s, a);
    return hipGetLastError();
}
hipError_t launch_mk_tail(const MkTailArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(mk_tail_kernel, image_grid(a.w, a.h), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_mk_rescale(const float *src, int sw, int sh, float *dst, int dw, int dh, hipStream_t s)
{
    hipLaunchKernelGGL(mk_rescale_kernel, image_grid(dw, dh), dim3(256), 0, s, src, sw, sh, dst, dw, dh);
    return hipGetLastError();
}

} // namespace artgpu
