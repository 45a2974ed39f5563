// art_amd/csrc/sharpen.h -- argument blocks of the capture-sharpening kernels (sharpen.hip) and the stage's host routines, shared with
// artgpu_api.hip.  (reference: rtengine/ipsharpen.cc:144-229,315-340,712-788; gauss.cc:52-92,177-443,860-1146,1437-1523;
// rt_algo.cc:497-596,942-976; deconvautoradius.cc:39-96)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace artgpu {

// which blur gaussianBlur(src != dst, GAUSS_DIV / GAUSS_MULT) runs for a sigma (gauss.cc:1437-1523); the values are ARTGPU_SHARPEN_REGIME_*
enum { SH_COPY = 0, SH_3X3 = 1, SH_5X5 = 2, SH_7X7 = 3, SH_YVV = 4 };
// the stencil coefficients as the reference passes them to its kernels (floats):
//   SH_3X3: c = {c0, c1, c2}, b0, b1 (gauss.cc:1448-1461);  SH_5X5: c = {c21, c20, c11, c10, c00} (L337-341);
//   SH_7X7: c = {c31, c30, c22, c21, c20, c11, c10, c00} (L282-289)
struct ShCoef { float c[8]; float b0, b1; };
// regime of a sigma in [0.2, 25) and its coefficients (host; exp in double, the 5x5 / 7x7 sums in float, row-major)
int sh_regime(double sigma, ShCoef *k);
float sh_pow_F(float a, float b);      // pow_F (rtengine/sleef.h:1296-1299), the scalar sleef forms on the host

// one Richardson-Lucy iteration (ipsharpen.cc:202-213): planes of W * H floats
struct ShRlArgs {
    const float *est_in;           // tmpI
    float *est_out;                // tmpI after the iteration (the fused kernel ping-pongs; the pointwise forms work in place, est_out == est_in)
    float *ratio;                  // tmp: the two-kernel forms' l / blur(tmpI)
    const float *lum;              // luminance + 1000
    const float *blend;
    const unsigned char *impulse;
    float *out;                    // NaN until check_stop freezes the pixel
    int W, H;
    float amount;
    ShCoef k;
};
hipError_t launch_rl_init(float *lum, float *est, float *out, int W, int H, hipStream_t s);                 // L167-174
hipError_t launch_rl_iter(const ShRlArgs &a, int regime, hipStream_t s);                                    // DIV, MULT and check_stop in one kernel (stencil regimes)
hipError_t launch_rl_point(const ShRlArgs &a, int mult, hipStream_t s);                                     // est *= ratio (mult != 0), then check_stop
hipError_t launch_rl_final(float *lum, const float *est, const float *out, const float *blend, const unsigned char *impulse, float amount, int W, int H, hipStream_t s);   // L218-227
// the blur forms on their own (artgpu_gaussian_blur_ex; the two-kernel form of an iteration): stencil regimes, src != dst
hipError_t launch_gauss_div(const float *src, float *dst, const float *div, int W, int H, int regime, const ShCoef &k, hipStream_t s);
hipError_t launch_gauss_mult(const float *src, float *dst, int W, int H, int regime, const ShCoef &k, hipStream_t s);
// SH_YVV: what gaussVerticalSsediv / gaussVerticalSsemult do with the blurred value (`blur` = the shared YvV blur's result)
hipError_t launch_yvv_div(float *blur, const float *div, int W, int H, hipStream_t s);                      // blur = div / (blur > 0 ? blur : 1), max 0 where the reference has it
hipError_t launch_yvv_mult(const float *blur, float *dst, int W, int H, hipStream_t s);                     // dst *= blur

// the stage around the loop
struct ShImage { float *p[3]; size_t stride; int W, H; };
hipError_t launch_sh_luminance(const ShImage &im, const float ws1[3], float *Y, hipStream_t s);             // get_luminance
hipError_t launch_sh_impulse(const float *Y, float *lpf /* blurred Y on entry, |Y - lpf| on return */, unsigned char *impulse, int W, int H, float thresh, hipStream_t s);
struct ShCornerArgs { float *YY; const float *YY2; int W, H, ox, oy, w2, h2; float r2, sigma; };             // CornerBoostMask (L315-340), L769-774
hipError_t launch_sh_corner(const ShCornerArgs &a, hipStream_t s);
hipError_t launch_sh_multiply(const ShImage &im, const float *num, const float *den, hipStream_t s);        // rt_algo.cc:958-976
// counters[0] += impulse pixels, counters[1] += pixels whose `out` is not NaN (either pointer may be null); counters are zeroed by the caller
hipError_t launch_sh_count(const unsigned char *impulse, const float *out, size_t n, unsigned long long *counters, hipStream_t s);

// calcRadiusBayer's maximum (deconvautoradius.cc:39-89): result[0] = max(1, maxVal / minVal over the eligible pairs)
constexpr int SH_RADIUS_PARTIALS = 1024;
hipError_t launch_sh_radius(const float *raw, size_t stride, int W, int H, unsigned fc0, unsigned fc1, float lower, float upper, float *partial, float *result, hipStream_t s);

} // namespace artgpu
