// tests/emul/impulse_defringe_ref.cc -- CPU checker for artgpu_impulse_denoise and artgpu_defringe: markImpulse (rtengine/rt_algo.cc:497-596),
// impulse_nr (impulse_denoise.cc:33-174), gauss3x3 (gauss.cc:129-174, 1444-1461) and PF_correct_RT (PF_correct_RT.cc:44-205), restated serially
// on contiguous float planes of an image in LAB mode.  Test infrastructure only; built on first use with -ffp-contract=off (rtengine is built
// without contraction).
//
// gaussianBlur GAUSS_STANDARD from sigma 0.6, xatan2f and FlatCurve are liboracle's restatements (oracle_gaussian_blur, oracle_xatan2f,
// oracle_flat_curve_*), not another copy.
//
// Two things the reference leaves open are DEFINED here the way include/artgpu.h defines them:
//   chromave  is summed in a fixed order (chunks of 4096 pixels, 256 strided sub-sums of 16 per chunk folded pairwise at distances 32 .. 1
//             within each group of 64 and the four groups in order, the chunks' sums combined the same way);
//   order 0   every window of the averaging loop reads the tool's input a and b.  Orders 1 and 2 are two schedules the reference itself may
//             run: raster order in place (one thread), and 16-row chunks taken last to first, each in place.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

extern "C" {
void oracle_gaussian_blur(float *img, int W, int H, double sigma);
float oracle_xatan2f(float y, float x);
void *oracle_flat_curve_new(const double *pts, int npts, int periodic, int ppn, double identity);
double oracle_flat_curve_get(const void *h, double t);
void oracle_flat_curve_free(void *h);
}

namespace {

inline float SQR(float x) { return x * x; }

struct Rows {       // float ** over a contiguous plane
    float *p; int W;
    float *operator[](int i) const { return p + (size_t)i * W; }
};

// Color::huelab_to_huehsv2 (color.h:1719-1754)
double huelab_to_huehsv2(float HH)
{
    double hr = 0.0;
    if (HH >= 0.f && HH < 0.6f) hr = 0.11666 * double(HH) + 0.93;
    else if (HH >= 0.6f && HH < 1.4f) hr = 0.1125 * double(HH) - 0.0675;
    else if (HH >= 1.4f && HH < 2.f) hr = 0.2666 * double(HH) - 0.2833;
    else if (HH >= 2.f && HH <= 3.14159f) hr = 0.1489 * double(HH) - 0.04785;
    else if (HH >= -3.1416f && HH < -2.8f) hr = 0.23419 * double(HH) + 1.1557;
    else if (HH >= -2.8f && HH < -2.3f) hr = 0.16 * double(HH) + 0.948;
    else if (HH >= -2.3f && HH < -0.9f) hr = 0.12143 * double(HH) + 0.85928;
    else if (HH >= -0.9f && HH < -0.1f) hr = 0.2125 * double(HH) + 0.94125;
    else if (HH >= -0.1f && HH < 0.f) hr = 0.1 * double(HH) + 0.93;
    if (hr < 0.0) hr += 1.0;
    else if (hr > 1.0) hr -= 1.0;
    return hr;
}

// 256 values as a 256-thread workgroup adds them: each group of 64 folded at distances 32 .. 1, the four groups in order
double fold256(double *v)
{
    for (int w = 0; w < 4; ++w)
        for (int o = 32; o > 0; o >>= 1)
            for (int l = 0; l < o; ++l) v[w * 64 + l] += v[w * 64 + l + o];
    double s = v[0];
    for (int w = 1; w < 4; ++w) s += v[w * 64];
    return s;
}

// the double sum of n floats in the defined order
double ordered_sum(const float *x, size_t n)
{
    const size_t nchunk = (n + 4095) / 4096;
    std::vector<double> partial(nchunk);
    double v[256];
    for (size_t c = 0; c < nchunk; ++c) {
        for (int t = 0; t < 256; ++t) {
            double acc = 0.0;
            for (int k = 0; k < 16; ++k) {
                const size_t i = c * 4096 + t + (size_t)k * 256;
                if (i < n) acc += x[i];
            }
            v[t] = acc;
        }
        partial[c] = fold256(v);
    }
    for (int t = 0; t < 256; ++t) {
        double acc = 0.0;
        for (size_t p = t; p < nchunk; p += 256) acc += partial[p];
        v[t] = acc;
    }
    return fold256(v);
}

} // namespace

extern "C" {

// markImpulse (rt_algo.cc:497-596); returns the number of impish pixels
long long id_ref_mark_impulse(const float *srcp, unsigned char *impulse, int width, int height, float thresh)
{
    std::vector<float> lpfv(srcp, srcp + (size_t)width * height);
    oracle_gaussian_blur(lpfv.data(), width, height, std::max(2.f, thresh - 1.f));
    const Rows src{const_cast<float *>(srcp), width}, lpf{lpfv.data(), width};
    const float impthr = std::max(1.f, 5.5f - thresh);
    const float impthrDiv24 = impthr / 24.0f;
    long long count = 0;
    for (int i = 0; i < height; i++) {
        unsigned char *imp = impulse + (size_t)i * width;
        int i1, j1, j;
        float hpfabs, hfnbrave;
        for (j = 0; j < 2; j++) {
            hpfabs = fabs(src[i][j] - lpf[i][j]);
            for (i1 = std::max(0, i - 2), hfnbrave = 0; i1 <= std::min(i + 2, height - 1); i1++)
                for (j1 = 0; j1 <= j + 2; j1++) hfnbrave += fabs(src[i1][j1] - lpf[i1][j1]);
            imp[j] = (hpfabs > ((hfnbrave - hpfabs) * impthrDiv24));
        }
        for (; j < width - 5; j += 4)
            for (int k = 0; k < 4; ++k) {              // the four lanes of the SSE2 loop
                float sum = 0.f;
                const float h = fabsf(src[i][j + k] - lpf[i][j + k]);
                for (i1 = std::max(0, i - 2); i1 <= std::min(i + 2, height - 1); i1++)
                    for (j1 = j - 2; j1 <= j + 2; j1++) sum += fabsf(src[i1][j1 + k] - lpf[i1][j1 + k]);
                const float t = (sum - h) * impthrDiv24 - h;
                uint32_t bits;
                std::memcpy(&bits, &t, 4);
                imp[j + k] = (unsigned char)(bits >> 31);           // _mm_movemask_ps: the sign bit
            }
        for (; j < width - 2; j++) {
            hpfabs = fabs(src[i][j] - lpf[i][j]);
            for (i1 = std::max(0, i - 2), hfnbrave = 0; i1 <= std::min(i + 2, height - 1); i1++)
                for (j1 = j - 2; j1 <= j + 2; j1++) hfnbrave += fabs(src[i1][j1] - lpf[i1][j1]);
            imp[j] = (hpfabs > ((hfnbrave - hpfabs) * impthrDiv24));
        }
        for (; j < width; j++) {
            hpfabs = fabs(src[i][j] - lpf[i][j]);
            for (i1 = std::max(0, i - 2), hfnbrave = 0; i1 <= std::min(i + 2, height - 1); i1++)
                for (j1 = j - 2; j1 < width; j1++) hfnbrave += fabs(src[i1][j1] - lpf[i1][j1]);
            imp[j] = (hpfabs > ((hfnbrave - hpfabs) * impthrDiv24));
        }
        for (j = 0; j < width; ++j) count += imp[j] != 0;
    }
    return count;
}

// what ImProcFunctions::impulsedenoise derives (impulse_denoise.cc:185-187, rt_algo.cc:511-516): out = {thresh, sigma, impthr}
void id_ref_impulse_derived(int thresh_param, double scale, float out[3])
{
    const float t = thresh_param / scale;
    const float thresh = float(t / 20.0);
    out[0] = thresh;
    out[1] = std::max(2.f, thresh - 1.f);
    out[2] = std::max(1.f, 5.5f - thresh);
}

// impulse_nr (impulse_denoise.cc:33-174) on the planes of an image in LAB mode; `impish` (W * H bytes) receives the map.  backwards != 0 walks
// the rows and, within a row, the pixels last to first: the reference's schedule(dynamic,16) may take them in any order.  keeps: pixels whose
// norm was 0.  Returns the number of impish pixels.
long long id_ref_impulse_nr(float *Lp, float *ap, float *bp, int width, int height, float thresh, int backwards, unsigned char *impish, long long *keeps)
{
    const long long count = id_ref_mark_impulse(Lp, impish, width, height, thresh);
    const Rows lab_L{Lp, width}, lab_a{ap, width}, lab_b{bp, width};
    const float eps = 1.0;
    long long kept = 0;
    for (int ii = 0; ii < height; ii++) {
        const int i = backwards ? height - 1 - ii : ii;
        for (int jj = 0; jj < width; jj++) {
            const int j = backwards ? width - 1 - jj : jj;
            if (!impish[(size_t)i * width + j]) continue;
            // the three column loops differ in their bounds only (L94, L122, L150)
            const int lo = j < 2 ? 0 : j - 2, hi = j < width - 2 ? j + 2 : width - 1;
            float norm = 0.0;
            float wtdsum[3] = {0.0, 0.0, 0.0};
            for (int i1 = std::max(0, i - 2); i1 <= std::min(i + 2, height - 1); i1++)
                for (int j1 = lo; j1 <= hi; j1++) {
                    if (impish[(size_t)i1 * width + j1]) continue;
                    const float dirwt = 1 / (SQR(lab_L[i1][j1] - lab_L[i][j]) + eps);
                    wtdsum[0] += dirwt * lab_L[i1][j1];
                    wtdsum[1] += dirwt * lab_a[i1][j1];
                    wtdsum[2] += dirwt * lab_b[i1][j1];
                    norm += dirwt;
                }
            if (norm) {
                lab_L[i][j] = wtdsum[0] / norm;
                lab_a[i][j] = wtdsum[1] / norm;
                lab_b[i][j] = wtdsum[2] / norm;
            } else ++kept;
        }
    }
    if (keeps) *keeps = kept;
    return count;
}

// gaussianBlur's coefficients for the 3x3 form (gauss.cc:1448-1461), narrowed as the call narrows them: out = {c0, c1, c2, b0, b1}
void id_ref_gauss3x3_coef(double sigma, float out[5])
{
    double c0 = 1.0;
    double c1 = exp(-0.5 * ((1.0 / sigma) * (1.0 / sigma)));
    double c2 = exp(-((1.0 / sigma) * (1.0 / sigma)));
    const double sum = c0 + 4.0 * (c1 + c2);
    c0 /= sum; c1 /= sum; c2 /= sum;
    double b1 = exp(-1.0 / (2.0 * sigma * sigma));
    const double bsum = 2.0 * b1 + 1.0;
    b1 /= bsum;
    const double b0 = 1.0 / bsum;
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = b0; out[4] = b1;
}

// gauss3x3<float> (gauss.cc:129-174)
void id_ref_gauss3x3(const float *srcp, float *dstp, int W, int H, double sigma)
{
    float k[5];
    id_ref_gauss3x3_coef(sigma, k);
    const float c0 = k[0], c1 = k[1], c2 = k[2], b0 = k[3], b1 = k[4];
    const Rows src{const_cast<float *>(srcp), W}, dst{dstp, W};
    dst[0][0] = src[0][0];
    for (int j = 1; j < W - 1; j++) dst[0][j] = b1 * (src[0][j - 1] + src[0][j + 1]) + b0 * src[0][j];
    dst[0][W - 1] = src[0][W - 1];
    for (int i = 1; i < H - 1; i++) {
        dst[i][0] = b1 * (src[i - 1][0] + src[i + 1][0]) + b0 * src[i][0];
        for (int j = 1; j < W - 1; j++)
            dst[i][j] = c2 * (src[i - 1][j - 1] + src[i - 1][j + 1] + src[i + 1][j - 1] + src[i + 1][j + 1]) + c1 * (src[i - 1][j] + src[i][j - 1] + src[i][j + 1] + src[i + 1][j]) + c0 * src[i][j];
        dst[i][W - 1] = b1 * (src[i - 1][W - 1] + src[i + 1][W - 1]) + b0 * src[i][W - 1];
    }
    dst[H - 1][0] = src[H - 1][0];
    for (int j = 1; j < W - 1; j++) dst[H - 1][j] = b1 * (src[H - 1][j - 1] + src[H - 1][j + 1]) + b0 * src[H - 1][j];
    dst[H - 1][W - 1] = src[H - 1][W - 1];
}

// gaussianBlur(src, dst, W, H, sigma) for src != dst, GAUSS_STANDARD, sigma < 25 (gauss.cc:1437-1523); returns the form (0 copy, 1 3x3, 2 recursive)
int id_ref_gauss_standard(const float *src, float *dst, int W, int H, double sigma)
{
    if (sigma < 0.25) { std::memcpy(dst, src, (size_t)W * H * 4); return 0; }
    if (sigma < 0.6) { id_ref_gauss3x3(src, dst, W, H, sigma); return 1; }
    std::memcpy(dst, src, (size_t)W * H * 4);       // gaussHorizontalSse(src, dst) + gaussVerticalSse(dst, dst): the in-place filter's arithmetic
    oracle_gaussian_blur(dst, W, H, sigma);
    return 2;
}

struct id_ref_defringe_info {       // the layout of artgpu_defringe_info
    int32_t early_out, halfwin, blur, curve;
    double radius, chromave;
    float threshfactor;
    int32_t pad_;
    int64_t corrected_pixels;
};

// PF_correct_RT (PF_correct_RT.cc:44-205) on the a and b planes of an image in LAB mode.  order: see the head of this file.  `flagged` (W * H
// bytes, may be null) receives which pixels were corrected.  Returns 0, or -4 where the device path refuses (the radius, the window, the width).
int id_ref_defringe(float *ap, float *bp, int width, int height, double radius, int thresh, const double *huecurve, int nhuecurve, int order,
                    unsigned char *flagged, id_ref_defringe_info *info)
{
    *info = id_ref_defringe_info{};
    info->radius = radius;
    if (!std::isfinite(radius) || radius >= 25.0 || radius < 0.0) return -4;
    const int halfwin = std::ceil(2 * radius) + 1;
    info->halfwin = halfwin;
    if (halfwin > 11 || width < 2 * halfwin - 2) return -4;
    void *chCurve = nullptr;
    if (nhuecurve > 0 && int(huecurve[0]) > 0) chCurve = oracle_flat_curve_new(huecurve, nhuecurve, 1, 1000, 0.5);      // L48-50
    const size_t n = (size_t)width * height;
    const Rows a{ap, width}, b{bp, width};
    std::vector<float> fringe(n), tmpav(n), tmpbv(n);
    info->blur = id_ref_gauss_standard(ap, tmpav.data(), width, height, radius);
    id_ref_gauss_standard(bp, tmpbv.data(), width, height, radius);
    const Rows tmpa{tmpav.data(), width}, tmpb{tmpbv.data(), width};
    for (int i = 0; i < height; i++)
        for (int j = 0; j < width; j++) {
            float chromaChfactor = 1.f;
            if (chCurve) {
                const float HH = oracle_xatan2f(b[i][j], a[i][j]);
                float chparam = oracle_flat_curve_get(chCurve, huelab_to_huehsv2(HH)) - 0.5f;
                if (chparam < 0.f) chparam *= 2.f;
                chromaChfactor = SQR(1.f + chparam);
            }
            fringe[(size_t)i * width + j] = chromaChfactor * (SQR(a[i][j] - tmpa[i][j]) + SQR(b[i][j] - tmpb[i][j]));
        }
    if (chCurve) oracle_flat_curve_free(chCurve);
    double chromave = ordered_sum(fringe.data(), n);
    chromave /= height * width;
    info->chromave = chromave;
    if (flagged) std::memset(flagged, 0, n);
    if (!(chromave > 0.0)) return 0;
    for (size_t j = 0; j < n; j++) fringe[j] = 1.f / (fringe[j] + chromave);
    const float threshfactor = 1.f / (SQR(thresh / 33.f) * chromave * 5.0f + chromave);
    info->threshfactor = threshfactor;
    std::vector<float> ina, inb;
    if (order == 0) { ina.assign(ap, ap + n); inb.assign(bp, bp + n); }
    const Rows ra{order == 0 ? ina.data() : ap, width}, rb{order == 0 ? inb.data() : bp, width};       // what the windows read
    std::vector<int> rows;
    if (order == 2) { for (int c = (height - 1) / 16; c >= 0; --c) for (int i = c * 16; i < std::min(height, c * 16 + 16); ++i) rows.push_back(i); }
    else for (int i = 0; i < height; ++i) rows.push_back(i);
    long long corrected = 0;
    for (int i : rows)
        for (int j = 0; j < width; j++) {
            if (!(fringe[(size_t)i * width + j] < threshfactor)) continue;
            // the three column loops differ in their bounds only (L151, L171, L191)
            const int lo = j < halfwin - 1 ? 0 : j - halfwin + 1, hi = j < width - halfwin + 1 ? j + halfwin : width;
            float atot = 0.f, btot = 0.f, norm = 0.f;
            for (int i1 = std::max(0, i - halfwin + 1); i1 < std::min(height, i + halfwin); i1++)
                for (int j1 = lo; j1 < hi; j1++) {
                    const float wt = fringe[(size_t)i1 * width + j1];
                    atot += wt * ra[i1][j1];
                    btot += wt * rb[i1][j1];
                    norm += wt;
                }
            a[i][j] = atot / norm;
            b[i][j] = btot / norm;
            if (flagged) flagged[(size_t)i * width + j] = 1;
            ++corrected;
        }
    info->corrected_pixels = corrected;
    return 0;
}

// the double sum in the defined order, on its own
double id_ref_ordered_sum(const float *x, long long n) { return ordered_sum(x, (size_t)n); }

} // extern "C"
