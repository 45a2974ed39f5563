// art_amd/csrc/creativegradients.hip -- ImProcFunctions::transformLuminanceOnly with creative = true (rtengine/iptransform.cc:987-1048): the
// graduated filter's and the vignette filter's factor of every pixel, and the three channel products; one lane per pixel, in place.
// calcGradientFactor (L761-812) and calcPCVignetteFactor (L898-983) are restated expression by expression; where the reference mixes types the
// conversions are spelled out: an int compared with or subtracted from a float becomes a float first, the fade distance is sqrtf of an int sum,
// and calcGradientFactor's last expression is evaluated in double and rounded to the float it returns.  The file is built with
// -ffp-contract=off; sqrtf and the divisions are correctly rounded.
#include "creativegradients.h"
#include "devmath.h"
#include "devsleef.h"

namespace artgpu {

namespace {

constexpr float CG_PI_F_2 = (float)1.57079632679489661923;          // rtengine::RT_PI_F_2

__device__ __forceinline__ float cg_pow3(float x) { return x * x * x; }
__device__ __forceinline__ float cg_pow4(float x) { return (x * x) * (x * x); }

// normn (L71-89).  sep = int(sepf) & ~1 with sepf in [2, 6], so n is 2, 4 or 6 for the first super-ellipse and 4, 6 or 8 for the second: the
// pow_F default never runs, and api_creativegradients.hip refuses what would reach it
__device__ __forceinline__ float cg_normn(float a, float b, int n)
{
    switch (n) {
    case 2: return sqrtf(a * a + b * b);
    case 4: return sqrtf(sqrtf(cg_pow4(a) + cg_pow4(b)));
    case 6: return sqrtf(xcbrtf_s(cg_pow3(a) * cg_pow3(a) + cg_pow3(b) * cg_pow3(b)));
    default: return sqrtf(sqrtf(sqrtf(cg_pow4(a) * cg_pow4(a) + cg_pow4(b) * cg_pow4(b))));     // 8
    }
}

// calcGradientFactor: the angle_is_zero branch is the other one with top_edge = top_edge_0
__device__ __forceinline__ float cg_gradient_factor(const CgDerived &gp, int x, int y)
{
    const int gy = gp.transpose ? x : y;
    float top_edge = gp.top_edge_0;
    if (!gp.angle_is_zero) {
        const int gx = gp.transpose ? gp.h - y - 1 : x;
        top_edge = gp.top_edge_0 - gp.ta * ((float)gx - gp.xc);
    }
    if ((float)gy < top_edge) return gp.topmul;
    if ((float)gy >= top_edge + gp.ys) return gp.botmul;
    float val = ((float)gy - top_edge) * gp.ys_inv;
    if (gp.bright_top) val = 1.f - val;
    val *= CG_PI_F_2;
    if (gp.scale < 1.f) val = cg_pow3(xsinf_s(val));
    else val = 1.f - cg_pow3(xcosf_s(val));
    return (float)((double)gp.scale + (double)val * (1.0 - (double)gp.scale));
}

// calcPCVignetteFactor
__device__ __forceinline__ float cg_pcvignette_factor(const CgDerived &pcv, int x, int y)
{
    float fo = 1.f;
    if (x < pcv.x1 || x > pcv.x2 || y < pcv.y1 || y > pcv.y2) {
        int dist_x = (x < pcv.x1) ? pcv.x1 - x : x - pcv.x2;
        int dist_y = (y < pcv.y1) ? pcv.y1 - y : y - pcv.y2;
        if (dist_x < 0) dist_x = 0;
        if (dist_y < 0) dist_y = 0;
        fo = sqrtf((float)(dist_x * dist_x + dist_y * dist_y)) * pcv.fadeout_mul;
        if (fo >= 1.f) return 1.f;
    }
    float a = fabsf((float)(x - pcv.ex) - (float)pcv.ew * 0.5f);
    float b = fabsf((float)(y - pcv.ey) - (float)pcv.eh * 0.5f);
    if (pcv.is_portrait) { const float t = a; a = b; b = t; }
    const float dist = cg_normn(a, b, 2);
    float cs = 1.0f, sn = 0.0f;
    if (dist != 0.0f) { cs = a / dist; sn = b / dist; }
    float dist_oe, dist_ie;
    if (pcv.is_super_ellipse_mode) {
        const float dist_oe1 = pcv.oe1_a * pcv.oe1_b / cg_normn(pcv.oe1_b * cs, pcv.oe1_a * sn, pcv.sep);
        const float dist_oe2 = pcv.oe2_a * pcv.oe2_b / cg_normn(pcv.oe2_b * cs, pcv.oe2_a * sn, pcv.sep + 2);
        const float dist_ie1 = pcv.ie1_mul * dist_oe1;
        const float dist_ie2 = pcv.ie2_mul * dist_oe2;
        dist_oe = dist_oe1 * (1.f - pcv.sepmix) + dist_oe2 * pcv.sepmix;
        dist_ie = dist_ie1 * (1.f - pcv.sepmix) + dist_ie2 * pcv.sepmix;
    } else {
        dist_oe = pcv.oe_a * pcv.oe_b / sqrtf(sqr(pcv.oe_b * cs) + sqr(pcv.oe_a * sn));
        dist_ie = pcv.ie_mul * dist_oe;
    }
    if (dist <= dist_ie) return 1.f;
    float val;
    if (dist >= dist_oe) {
        val = pcv.pcv_scale;
    } else {
        val = CG_PI_F_2 * (dist - dist_ie) / (dist_oe - dist_ie);
        if (pcv.pcv_scale < 1.f) val = cg_pow4(xcosf_s(val));
        else val = 1 - cg_pow4(xsinf_s(val));
        val = pcv.pcv_scale + val * (1.f - pcv.pcv_scale);
    }
    if (fo < 1.f) val = fo + val * (1.f - fo);
    return val;
}

} // namespace

// `factor` is the double 1.0 times each tool's float (L1022-1041) and a channel is float(double(pixel) * factor).  With one tool the factor is
// that float exactly and the double product of two floats is exact, so one float multiply rounds the same number once; with both the factor
// is the rounded-to-double product of the two and the channel product is rounded again: that form stays in double
template <bool GRAD, bool PCV>
__global__ void __launch_bounds__(256) cg_factor_kernel(CgArgs a)
{
    FOR_IMAGE_XY(y, x, a.w, a.h) {
        const size_t o = (size_t)y * a.stride + x;
        const float r = a.img[0][o], g = a.img[1][o], b = a.img[2][o];
        const int px = a.d.cx + x, py = a.d.cy + y;
        if (GRAD && PCV) {
            const double factor = (double)cg_gradient_factor(a.d, px, py) * (double)cg_pcvignette_factor(a.d, px, py);
            a.img[0][o] = (float)((double)r * factor); a.img[1][o] = (float)((double)g * factor); a.img[2][o] = (float)((double)b * factor);
        } else {
            const float f = GRAD ? cg_gradient_factor(a.d, px, py) : cg_pcvignette_factor(a.d, px, py);
            a.img[0][o] = r * f; a.img[1][o] = g * f; a.img[2][o] = b * f;
        }
    }
}

hipError_t launch_cg(const CgArgs &a, hipStream_t s)
{
    const dim3 grid = image_grid(a.w, a.h);
    if (a.d.apply_gradient && a.d.apply_pcvignette) hipLaunchKernelGGL((cg_factor_kernel<true, true>), grid, dim3(256), 0, s, a);
    else if (a.d.apply_gradient) hipLaunchKernelGGL((cg_factor_kernel<true, false>), grid, dim3(256), 0, s, a);
    else if (a.d.apply_pcvignette) hipLaunchKernelGGL((cg_factor_kernel<false, true>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace artgpu
