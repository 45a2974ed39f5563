// tests/emul/sharpen_ref.cc -- CPU checker for artgpu_sharpening and its staged entry points: ImProcFunctions::doSharpening for method "rld"
// (rtengine/ipsharpen.cc:144-229,315-340,712-788), the GAUSS_DIV / GAUSS_MULT forms of gaussianBlur for src != dst (gauss.cc:52-92,177-443,
// 860-1146,1437-1523), markImpulse (rt_algo.cc:497-596), get_luminance / multiply (rt_algo.cc:942-976) and calcRadiusBayer
// (deconvautoradius.cc:39-96), restated serially on contiguous float planes, with counters for every branch.
// Test infrastructure only; built on first use with -ffp-contract=off (rtengine is built without contraction).
//
// gaussianBlur GAUSS_STANDARD (0.6 <= sigma < 25), xexpf and pow_F are liboracle's restatements (oracle_gaussian_blur, oracle_xexpf_s / _v,
// oracle_pow_F), not a third copy.  The DIV / MULT forms restated here are pinned to the compiled reference by tests/golden/gauss_divmult.npz.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

extern "C" {
void oracle_gaussian_blur(float *img, int W, int H, double sigma);
float oracle_xexpf_s(float d);
float oracle_xexpf_v(float d);
float oracle_pow_F(float a, float b);
}

namespace {
template <typename T> inline const T &rt_min(const T &a, const T &b) { return b < a ? b : a; }   // rt_math.h:55-58
template <typename T> inline const T &rt_max(const T &a, const T &b) { return a < b ? b : a; }   // rt_math.h:73-76
inline float rt_max3(float a, float b, float c) { return rt_max(rt_max(a, b), c); }
inline float rt_max4(float a, float b, float c, float d) { return rt_max(rt_max(a, b), rt_max(c, d)); }
inline float LIM01(float a) { return rt_max(0.f, rt_min(a, 1.f)); }
inline float SQR(float x) { return x * x; }
inline float intp(float a, float b, float c) { return a * b + (1.f - a) * c; }                   // rt_math.h:110-118
inline float sse_max(float x, float y) { return x > y ? x : y; }                                  // _mm_max_ps
const float RT_NAN_F = std::numeric_limits<float>::quiet_NaN();

struct Rows {       // float ** over a contiguous plane
    float *p; int W;
    float *operator[](int i) const { return p + (size_t)i * W; }
};

void compute7x7kernel(float sigma, float kernel[7][7])
{
    const double temp = -2.f * SQR(sigma);
    float sum = 0.f;
    for (int i = -3; i <= 3; ++i)
        for (int j = -3; j <= 3; ++j) {
            if ((i * i + j * j) <= (3.0 * 1.15) * (3.0 * 1.15)) {
                kernel[i + 3][j + 3] = std::exp((i * i + j * j) / temp);
                sum += kernel[i + 3][j + 3];
            } else {
                kernel[i + 3][j + 3] = 0.f;
            }
        }
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j < 7; ++j) kernel[i][j] /= sum;
}
void compute5x5kernel(float sigma, float kernel[5][5])
{
    const double temp = -2.f * SQR(sigma);
    float sum = 0.f;
    for (int i = -2; i <= 2; ++i)
        for (int j = -2; j <= 2; ++j) {
            if ((i * i + j * j) <= (3.0 * 0.84) * (3.0 * 0.84)) {
                kernel[i + 2][j + 2] = std::exp((i * i + j * j) / temp);
                sum += kernel[i + 2][j + 2];
            } else {
                kernel[i + 2][j + 2] = 0.f;
            }
        }
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 5; ++j) kernel[i][j] /= sum;
}

// gauss3x3div / gauss3x3mult (gauss.cc:177-274): DIV when div.p
void gauss3x3(Rows src, Rows dst, Rows div, int W, int H, float c0, float c1, float c2, float b0, float b1)
{
    const bool D = div.p != nullptr;
    auto put = [&](int i, int j, float v) {
        if (D) dst[i][j] = rt_max(div[i][j] / (v > 0.f ? v : 1.f), 0.f);
        else dst[i][j] *= v;
    };
    put(0, 0, src[0][0]);
    for (int j = 1; j < W - 1; j++) put(0, j, b1 * (src[0][j - 1] + src[0][j + 1]) + b0 * src[0][j]);
    put(0, W - 1, src[0][W - 1]);
    for (int i = 1; i < H - 1; i++) {
        put(i, 0, b1 * (src[i - 1][0] + src[i + 1][0]) + b0 * src[i][0]);
        for (int j = 1; j < W - 1; j++)
            put(i, j, c2 * (src[i - 1][j - 1] + src[i - 1][j + 1] + src[i + 1][j - 1] + src[i + 1][j + 1]) + c1 * (src[i - 1][j] + src[i][j - 1] + src[i][j + 1] + src[i + 1][j]) + c0 * src[i][j]);
        put(i, W - 1, b1 * (src[i - 1][W - 1] + src[i + 1][W - 1]) + b0 * src[i][W - 1]);
    }
    put(H - 1, 0, src[H - 1][0]);
    for (int j = 1; j < W - 1; j++) put(H - 1, j, b1 * (src[H - 1][j - 1] + src[H - 1][j + 1]) + b0 * src[H - 1][j]);
    put(H - 1, W - 1, src[H - 1][W - 1]);
}

// gauss5x5div / gauss5x5mult (gauss.cc:331-378,415-443)
void gauss5x5(Rows src, Rows dst, Rows div, int W, int H, float sigma, float *coef, long long *ring)
{
    float kernel[5][5];
    compute5x5kernel(sigma, kernel);
    const float c21 = kernel[0][1], c20 = kernel[0][2], c11 = kernel[1][1], c10 = kernel[1][2], c00 = kernel[2][2];
    if (coef) { coef[0] = c21; coef[1] = c20; coef[2] = c11; coef[3] = c10; coef[4] = c00; }
    const bool D = div.p != nullptr;
    for (int i = 2; i < H - 2; ++i) {
        if (D) dst[i][0] = dst[i][1] = 1.f;
        for (int j = 2; j < W - 2; ++j) {
            const float val = c21 * (src[i - 2][j - 1] + src[i - 2][j + 1] + src[i - 1][j - 2] + src[i - 1][j + 2] + src[i + 1][j - 2] + src[i + 1][j + 2] + src[i + 2][j - 1] + src[i + 2][j + 1]) +
                              c20 * (src[i - 2][j] + src[i][j - 2] + src[i][j + 2] + src[i + 2][j]) +
                              c11 * (src[i - 1][j - 1] + src[i - 1][j + 1] + src[i + 1][j - 1] + src[i + 1][j + 1]) +
                              c10 * (src[i - 1][j] + src[i][j - 1] + src[i][j + 1] + src[i + 1][j]) +
                              c00 * src[i][j];
            if (D) dst[i][j] = div[i][j] / std::max(val, 0.00001f);
            else dst[i][j] *= val;
        }
        if (D) dst[i][W - 2] = dst[i][W - 1] = 1.f;
    }
    if (D) {
        for (int i = 0; i < 2; ++i) for (int j = 0; j < W; ++j) dst[i][j] = 1.f;
        for (int i = H - 2; i < H; ++i) for (int j = 0; j < W; ++j) dst[i][j] = 1.f;
    }
    if (ring) *ring += (long long)W * H - (long long)(W - 4) * (H - 4);
}

// gauss7x7div / gauss7x7mult (gauss.cc:276-329,380-413), the doubled c21 included
void gauss7x7(Rows src, Rows dst, Rows div, int W, int H, float sigma, float *coef, long long *ring)
{
    float kernel[7][7];
    compute7x7kernel(sigma, kernel);
    const float c31 = kernel[0][2], c30 = kernel[0][3], c22 = kernel[1][1], c21 = kernel[1][2], c20 = kernel[1][3], c11 = kernel[2][2], c10 = kernel[2][3], c00 = kernel[3][3];
    if (coef) { coef[0] = c31; coef[1] = c30; coef[2] = c22; coef[3] = c21; coef[4] = c20; coef[5] = c11; coef[6] = c10; coef[7] = c00; }
    const bool D = div.p != nullptr;
    for (int i = 3; i < H - 3; ++i) {
        if (D) dst[i][0] = dst[i][1] = dst[i][2] = 1.f;
        for (int j = 3; j < W - 3; ++j) {
            const float val = c31 * (src[i - 3][j - 1] + src[i - 3][j + 1] + src[i - 1][j - 3] + src[i - 1][j + 3] + src[i + 1][j - 3] + src[i + 1][j + 3] + src[i + 3][j - 1] + src[i + 3][j + 1]) +
                              c30 * (src[i - 3][j] + src[i][j - 3] + src[i][j + 3] + src[i + 3][j]) +
                              c22 * (src[i - 2][j - 2] + src[i - 2][j + 2] + src[i + 2][j - 2] + src[i + 2][j + 2]) +
                              c21 * (src[i - 2][j - 1] + src[i - 2][j + 1] * c21 + src[i - 1][j - 2] + src[i - 1][j + 2] + src[i + 1][j - 2] + src[i + 1][j + 2] + src[i + 2][j - 1] + src[i + 2][j + 1]) +
                              c20 * (src[i - 2][j] + src[i][j - 2] + src[i][j + 2] + src[i + 2][j]) +
                              c11 * (src[i - 1][j - 1] + src[i - 1][j + 1] + src[i + 1][j - 1] + src[i + 1][j + 1]) +
                              c10 * (src[i - 1][j] + src[i][j - 1] + src[i][j + 1] + src[i + 1][j]) +
                              c00 * src[i][j];
            if (D) dst[i][j] = div[i][j] / std::max(val, 0.00001f);
            else dst[i][j] *= val;
        }
        if (D) dst[i][W - 3] = dst[i][W - 2] = dst[i][W - 1] = 1.f;
    }
    if (D) {
        for (int i = 0; i < 3; ++i) for (int j = 0; j < W; ++j) dst[i][j] = 1.f;
        for (int i = H - 3; i < H; ++i) for (int j = 0; j < W; ++j) dst[i][j] = 1.f;
    }
    if (ring) *ring += (long long)W * H - (long long)(W - 6) * (H - 6);
}

// gaussianBlurImpl's dispatch for src != dst and GAUSS_DIV (div.p) / GAUSS_MULT (gauss.cc:1437-1523).  Returns the regime 0 .. 4.
// sigma > 1.15: gaussHorizontalSse + gaussVerticalSsediv / gaussVerticalSsemult; the value they divide by / multiply with is the
// GAUSS_STANDARD blur's (the same recurrences, stored as float before the last step), then the store rules of L1079-1140 / L935-996.
int gaussian_blur(float *srcp, float *dstp, float *divp, int W, int H, double sigma, float *coef, long long *ring)
{
    const Rows src{srcp, W}, dst{dstp, W}, div{divp, W};
    if (sigma < 0.25) {
        if (srcp != dstp) std::memcpy(dstp, srcp, sizeof(float) * (size_t)W * H);
        return 0;
    }
    if (sigma < 0.6) {
        double c0 = 1.0;
        double c1 = exp(-0.5 * (1.0 / sigma) * (1.0 / sigma));
        double c2 = exp(-(1.0 / sigma) * (1.0 / sigma));
        const double sum = c0 + 4.0 * (c1 + c2);
        c0 /= sum; c1 /= sum; c2 /= sum;
        double b1 = exp(-1.0 / (2.0 * sigma * sigma));
        const double bsum = 2.0 * b1 + 1.0;
        b1 /= bsum;
        const double b0 = 1.0 / bsum;
        gauss3x3(src, dst, div, W, H, c0, c1, c2, b0, b1);
        return 1;
    }
    if (sigma <= 0.84) { gauss5x5(src, dst, div, W, H, sigma, coef, ring); return 2; }
    if (sigma <= 1.15) { gauss7x7(src, dst, div, W, H, sigma, coef, ring); return 3; }
    oracle_gaussian_blur(srcp, W, H, sigma);
    const int wvec = W - W % 8;
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) {
            const float v = src[i][j];
            if (divp) {
                const float q = div[i][j] / (v > 0.f ? v : 1.f);
                dst[i][j] = j < wvec ? (i >= H - 3 ? q : sse_max(q, 0.f)) : rt_max(q, 0.f);
            } else {
                dst[i][j] *= v;
            }
        }
    if (divp && srcp != dstp) { /* the reference's DIV form leaves src alone */ }
    return 4;
}
} // namespace

extern "C" {

struct sh_ref_params {           // the layout of artgpu_sharpening_params
    int32_t enabled, method, amount, deconvamount;
    double contrast, deconvradius, deconvCornerBoost;
    int32_t deconvCornerLatitude, offset_x, offset_y, full_width, full_height, pad_;
};
struct sh_ref_info {             // the layout of artgpu_sharpening_info
    double sigma;
    int32_t regime, early_out;
    float contrast_threshold;
    int32_t pad_;
    int64_t impulse_pixels, frozen_pixels;
};
struct sh_ref_counts {
    long long frozen_iter[20];                   // pixels check_stop froze in iteration k
    long long never_frozen;
    long long impulse_lo, impulse_vec, impulse_body, impulse_hi;   // impulses by column range: j < 2, the 4-wide loop, the scalar body, j >= W - 2
    long long est_nan, y_nonpos, ring_pixels, mask_low, mask_high;
    long long clip_rule_a, clip_rule_b;          // calcRadiusBayer: the two clipped-neighbourhood rules that rejected a pair
    long long pairs;                             // eligible pairs
};

// DIV (type 2) / MULT (type 1) on copies the caller owns: src is overwritten above sigma 1.15 (DIV as well here; the caller passes a copy).
// coef: the 5x5 / 7x7 kernel coefficients (room for 8) or null.
int sh_ref_gauss(float *src, float *dst, const float *div, int W, int H, double sigma, int type, float *coef)
{
    return gaussian_blur(src, dst, type == 2 ? const_cast<float *>(div) : nullptr, W, H, sigma, coef, nullptr);
}

// buildBlendMask(luminance, blend, W, H, contrastThreshold, 1.f, false, blur_radius) (rt_algo.cc:416-494)
void sh_ref_blend_mask(const float *L, float *blend, int W, int H, float contrastThreshold, float blur_radius)
{
    const size_t n = (size_t)W * H;
    if (contrastThreshold == 0.f) {
        for (size_t k = 0; k < n; ++k) blend[k] = 1.f;
        return;
    }
    const float scale = 0.0625f / 327.68f * 1.f;
    auto contrast_at = [&](int j, int i) {
        const float *p = L + (size_t)j * W + i;
        return sqrtf(SQR(p[1] - p[-1]) + SQR(p[W] - p[-W]) + SQR(p[2] - p[-2]) + SQR(p[2 * W] - p[-2 * W])) * scale;
    };
    for (int j = 2; j < H - 2; ++j) {
        int i = 2;
        for (; i < W - 5; i += 4)
            for (int k = 0; k < 4; ++k) blend[(size_t)j * W + i + k] = 1.f * (1.f / (1.f + oracle_xexpf_v(16.f - 16.f * contrast_at(j, i + k) / contrastThreshold)));
        for (; i < W - 2; ++i) blend[(size_t)j * W + i] = 1.f * (1.f / (1.f + oracle_xexpf_s(16.f - 16.f * contrast_at(j, i) / contrastThreshold)));
    }
    for (int j = 0; j < 2; ++j) for (int i = 2; i < W - 2; ++i) blend[(size_t)j * W + i] = blend[(size_t)2 * W + i];
    for (int j = H - 2; j < H; ++j) for (int i = 2; i < W - 2; ++i) blend[(size_t)j * W + i] = blend[(size_t)(H - 3) * W + i];
    for (int j = 0; j < H; ++j) {
        float *b = blend + (size_t)j * W;
        b[0] = b[1] = b[2];
        b[W - 2] = b[W - 1] = b[W - 3];
    }
    oracle_gaussian_blur(blend, W, H, blur_radius);
}

// markImpulse (rt_algo.cc:497-596)
void sh_ref_mark_impulse(const float *srcp, unsigned char *impulse, int width, int height, float thresh, sh_ref_counts *cn)
{
    std::vector<float> lpfv(srcp, srcp + (size_t)width * height);
    oracle_gaussian_blur(lpfv.data(), width, height, std::max(2.f, thresh - 1.f));
    const Rows src{const_cast<float *>(srcp), width}, lpf{lpfv.data(), width};
    const float impthr = std::max(1.f, 5.5f - thresh);
    const float impthrDiv24 = impthr / 24.0f;
    for (int i = 0; i < height; i++) {
        unsigned char *imp = impulse + (size_t)i * width;
        int i1, j1, j;
        float hpfabs, hfnbrave;
        for (j = 0; j < 2; j++) {
            hpfabs = fabs(src[i][j] - lpf[i][j]);
            for (i1 = std::max(0, i - 2), hfnbrave = 0; i1 <= std::min(i + 2, height - 1); i1++)
                for (j1 = 0; j1 <= j + 2; j1++) hfnbrave += fabs(src[i1][j1] - lpf[i1][j1]);
            imp[j] = (hpfabs > ((hfnbrave - hpfabs) * impthrDiv24));
            if (cn && imp[j]) ++cn->impulse_lo;
        }
        for (; j < width - 5; j += 4) {
            for (int k = 0; k < 4; ++k) {          // the four SSE lanes
                float sum = 0.f;
                const float h = fabsf(src[i][j + k] - lpf[i][j + k]);
                for (i1 = std::max(0, i - 2); i1 <= std::min(i + 2, height - 1); i1++)
                    for (j1 = j - 2; j1 <= j + 2; j1++) sum += fabsf(src[i1][j1 + k] - lpf[i1][j1 + k]);
                const float t = (sum - h) * impthrDiv24 - h;
                uint32_t bits;
                std::memcpy(&bits, &t, 4);
                imp[j + k] = (unsigned char)(bits >> 31);           // _mm_movemask_ps: the sign bit
                if (cn && imp[j + k]) ++cn->impulse_vec;
            }
        }
        for (; j < width - 2; j++) {
            hpfabs = fabs(src[i][j] - lpf[i][j]);
            for (i1 = std::max(0, i - 2), hfnbrave = 0; i1 <= std::min(i + 2, height - 1); i1++)
                for (j1 = j - 2; j1 <= j + 2; j1++) hfnbrave += fabs(src[i1][j1] - lpf[i1][j1]);
            imp[j] = (hpfabs > ((hfnbrave - hpfabs) * impthrDiv24));
            if (cn && imp[j]) ++cn->impulse_body;
        }
        for (; j < width; j++) {
            hpfabs = fabs(src[i][j] - lpf[i][j]);
            for (i1 = std::max(0, i - 2), hfnbrave = 0; i1 <= std::min(i + 2, height - 1); i1++)
                for (j1 = j - 2; j1 < width; j1++) hfnbrave += fabs(src[i1][j1] - lpf[i1][j1]);
            imp[j] = (hpfabs > ((hfnbrave - hpfabs) * impthrDiv24));
            if (cn && imp[j]) ++cn->impulse_hi;
        }
    }
}

// deconvsharpening (ipsharpen.cc:144-229).  Returns the early-out (0 none, 4 amount <= 0, 5 sigma < 0.2f); *regime the blur's.
int sh_ref_deconv(float *lum, const float *blend, const unsigned char *impulse, int W, int H, double sigma, float amount, int *regime, sh_ref_counts *cn,
                  long long *frozen_before_last)
{
    if (regime) *regime = -1;
    if (amount <= 0) return 4;
    const int maxiter = 20;
    const float delta_factor = 0.2f;
    if (sigma < 0.2f) return 5;
    const size_t n = (size_t)W * H;
    std::vector<float> tmp(n), tmpI(n), out(n), scratch(n);
    constexpr float offset = 1000.f;
    for (size_t p = 0; p < n; ++p) {
        lum[p] += offset;
        tmpI[p] = std::max(lum[p], 0.f);
        out[p] = RT_NAN_F;
    }
    const auto get_output = [&](size_t p) -> float {
        if (std::isnan(tmpI[p])) { if (cn) ++cn->est_nan; return lum[p]; }
        float b = impulse[p] ? 0.f : blend[p] * amount;
        return intp(b, std::max(tmpI[p], 0.0f), lum[p]);
    };
    long long frozen = 0;
    int rg = -1;
    for (int k = 0; k < maxiter; k++) {
        if (k == maxiter - 1 && frozen_before_last) *frozen_before_last = frozen;
        // gaussianBlur(tmpI, tmp, .., GAUSS_DIV, luminance): above 1.15 the horizontal pass writes tmp, tmpI stays
        scratch = tmpI;
        rg = gaussian_blur(scratch.data(), tmp.data(), lum, W, H, sigma, nullptr, cn && k == 0 ? &cn->ring_pixels : nullptr);
        // gaussianBlur(tmp, tmpI, .., GAUSS_MULT): above 1.15 tmp is filtered in place
        gaussian_blur(tmp.data(), tmpI.data(), nullptr, W, H, sigma, nullptr, nullptr);
        for (size_t p = 0; p < n; ++p) {
            if (std::isnan(out[p])) {
                float l = lum[p];
                float delta = l * delta_factor;
                if (std::abs(tmpI[p] - l) > delta) {
                    out[p] = get_output(p);
                    if (!std::isnan(out[p])) { ++frozen; if (cn) ++cn->frozen_iter[k]; }
                }
            }
        }
    }
    if (regime) *regime = rg;
    for (size_t p = 0; p < n; ++p) {
        float l = out[p];
        if (std::isnan(l)) { l = get_output(p); if (cn) ++cn->never_frozen; }
        lum[p] = std::max(l - offset, 0.f);
    }
    return 0;
}

// CornerBoostMask (ipsharpen.cc:315-340) on a W x H image at (ox, oy) of a fw x fh frame
void sh_ref_corner_mask(float *mask, int W, int H, int ox, int oy, int fw, int fh, int latitude)
{
    const int w2 = fw / 2, h2 = fh / 2;
    float radius = std::max(w2, h2);
    const float r2 = (radius - radius * LIM01(float(latitude) / 150.f)) / 2.f;
    const float sigma = 2.f * SQR(radius * 0.3f);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            int xx = x + ox - w2;
            int yy = y + oy - h2;
            float distance = std::sqrt(float(xx * xx + yy * yy));
            mask[(size_t)y * W + x] = 1.f - LIM01(oracle_xexpf_s((-SQR(std::max(distance - r2, 0.f)) / sigma)));
        }
}

// doSharpening (ipsharpen.cc:712-788), method rld.  Returns 0, or -4 where the library returns ARTGPU_EUNSUPPORTED.
int sh_ref_sharpening(float *r, float *g, float *b, int W, int H, const sh_ref_params *sp, const double *wsd, double scale, sh_ref_info *info, sh_ref_counts *cn)
{
    if (info) { std::memset(info, 0, sizeof *info); info->regime = -1; }
    if (!sp->enabled) { if (info) info->early_out = 1; return 0; }
    if (sp->amount < 1) { if (info) info->early_out = 2; return 0; }
    if (W < 8 || H < 8) { if (info) info->early_out = 3; return 0; }
    if (sp->method != 0) return -4;
    const size_t n = (size_t)W * H;
    const float ws1[3] = {(float)wsd[3], (float)wsd[4], (float)wsd[5]};
    float s_scale = std::sqrt(scale);
    float contrast = oracle_pow_F(sp->contrast / 100.f, 1.2f) * s_scale;
    const float blur_radius = 2.f / s_scale;
    if (!(blur_radius >= 0.6)) return -4;
    double sigma = sp->deconvradius / scale;
    float amount = sp->deconvamount / 100.f;
    float delta = sp->deconvCornerBoost / scale;
    auto ok = [](double s) { return s == s && !std::isinf(s) && s < 25.0; };
    if (!ok(sigma) || (delta > 0.01f && !ok(sigma + delta))) return -4;
    std::vector<float> Y(n), blend(n);
    for (size_t p = 0; p < n; ++p) {
        Y[p] = r[p] * ws1[0] + g[p] * ws1[1] + b[p] * ws1[2];
        if (cn && !(Y[p] > 0.f)) ++cn->y_nonpos;
    }
    sh_ref_blend_mask(Y.data(), blend.data(), W, H, contrast, blur_radius);
    if (cn) for (size_t p = 0; p < n; ++p) { if (blend[p] < 0.01f) ++cn->mask_low; if (blend[p] > 0.99f) ++cn->mask_high; }
    std::vector<unsigned char> impulse(n);
    sh_ref_mark_impulse(Y.data(), impulse.data(), W, H, 2.f, cn);
    std::vector<float> YY(Y);
    int regime = -1;
    long long frozen = 0;
    int early;
    if (delta > 0.01f) {
        std::vector<float> YY2(Y), mask(n);
        early = sh_ref_deconv(YY.data(), blend.data(), impulse.data(), W, H, sigma, amount, &regime, cn, &frozen);
        sh_ref_deconv(YY2.data(), blend.data(), impulse.data(), W, H, sigma + delta, amount, nullptr, nullptr, nullptr);
        int fw = sp->full_width > 0 ? sp->full_width : W;
        int fh = sp->full_height > 0 ? sp->full_height : H;
        sh_ref_corner_mask(mask.data(), W, H, sp->offset_x, sp->offset_y, fw, fh, sp->deconvCornerLatitude);
        for (size_t p = 0; p < n; ++p) YY[p] = intp(mask[p], YY2[p], YY[p]);
    } else {
        early = sh_ref_deconv(YY.data(), blend.data(), impulse.data(), W, H, sigma, amount, &regime, cn, &frozen);
    }
    for (size_t p = 0; p < n; ++p)
        if (Y[p] > 0.f) {
            const float f = YY[p] / Y[p];
            r[p] *= f; g[p] *= f; b[p] *= f;
        }
    if (info) {
        info->sigma = sigma; info->regime = regime; info->early_out = early; info->contrast_threshold = contrast;
        long long ni = 0;
        for (size_t p = 0; p < n; ++p) ni += impulse[p] ? 1 : 0;
        info->impulse_pixels = ni; info->frozen_pixels = frozen;
    }
    return 0;
}

// calcRadiusBayer (deconvautoradius.cc:39-96): serial != 0 the reference's loop as written (one thread), else the pure maximum over all
// eligible pairs (the library's contract).  Returns maxRatio; *radius the reference's formula.
float sh_ref_radius(const float *raw, int W, int H, float lowerLimit, float upperLimit, unsigned fc0, unsigned fc1, int serial, float *radius, sh_ref_counts *cn)
{
    const Rows rawData{const_cast<float *>(raw), W};
    const unsigned fc[2] = {fc0, fc1};
    float maxRatio = 1.f;
    for (int row = 4; row < H - 4; ++row) {
        for (int col = 5 + (fc[row & 1] & 1); col < W - 4; col += 2) {
            const float val00 = rawData[row][col];
            if (val00 > 0.f) {
                const float val1m1 = rawData[row + 1][col - 1];
                const float val1p1 = rawData[row + 1][col + 1];
                const float maxVal0 = std::max(val00, val1m1);
                if (val1m1 > 0.f && maxVal0 > lowerLimit) {
                    const float minVal = std::min(val00, val1m1);
                    if (!serial || maxVal0 > maxRatio * minVal) {
                        bool clipped = false;
                        if (maxVal0 == val00) {
                            if (rt_max3(rawData[row - 1][col - 1], rawData[row - 1][col + 1], val1p1) >= upperLimit) { clipped = true; if (cn) ++cn->clip_rule_a; }
                        } else {
                            if (rt_max4(rawData[row][col - 2], val00, rawData[row + 2][col - 2], rawData[row + 2][col]) >= upperLimit) { clipped = true; if (cn) ++cn->clip_rule_b; }
                        }
                        if (!clipped) {
                            if (cn) ++cn->pairs;
                            maxRatio = serial ? maxVal0 / minVal : std::max(maxRatio, maxVal0 / minVal);
                        }
                    }
                }
                const float maxVal1 = std::max(val00, val1p1);
                if (val1p1 > 0.f && maxVal1 > lowerLimit) {
                    const float minVal = std::min(val00, val1p1);
                    if (!serial || maxVal1 > maxRatio * minVal) {
                        if (maxVal1 == val00) {
                            if (rt_max3(rawData[row - 1][col - 1], rawData[row - 1][col + 1], val1p1) >= upperLimit) { if (cn) ++cn->clip_rule_a; continue; }
                        } else {
                            if (rt_max4(val00, rawData[row][col + 2], rawData[row + 2][col], rawData[row + 2][col + 2]) >= upperLimit) { if (cn) ++cn->clip_rule_b; continue; }
                        }
                        if (cn) ++cn->pairs;
                        maxRatio = serial ? maxVal1 / minVal : std::max(maxRatio, maxVal1 / minVal);
                    }
                }
            }
        }
    }
    if (radius) *radius = std::sqrt((1.f / (std::log(1.f / maxRatio) / 2.f)) / -2.f);
    return maxRatio;
}

float sh_ref_pow_F(float a, float b) { return oracle_pow_F(a, b); }

} // extern "C"
