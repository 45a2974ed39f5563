// tests/emul/textureboost_ref.cc -- CPU checker for artgpu_texture_boost: texture_boost and the region loop of ImProcFunctions::textureBoost
// (rtengine/iptextureboost.cc:37-248) restated serially, in the reference's order and with its intermediate planes (tmpY, mid, base all
// exist here), on contiguous float planes.  Test infrastructure only; built on first use with -ffp-contract=off (rtengine is built without
// contraction).
//
// rtengine::guidedFilter, rescaleBilinear, pow_F and Imagefloat::setMode(YUV / RGB) are liboracle's restatements (oracle_guided_filter,
// oracle_rescale_bilinear, oracle_pow_F, oracle_rgb_to_yuv / oracle_yuv_to_rgb), not a third copy.
// The reference's SSE2 bodies and scalar tails are selected by column: they part for a NaN only (vmaxf / vminf against std::max / std::min).
// Convolution::operator() (rt_algo.cc:733-899) is an FFTW product; by its index arithmetic it computes the clamp-to-edge sum
//   dst[y][x] = sum over ky, kx of kernel[ky][kx] * src[clamp(y + K / 2 - ky)][clamp(x + K / 2 - kx)],
// and this file DEFINES the stage as that sum in fp32, ky-major, from 0.f (tb_ref_conv); tb_ref_conv_double is the same sum in double.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

extern "C" {
void oracle_guided_filter(const float *guide, const float *src, float *dst, int W, int H, int r, float epsilon, int subsampling);
void oracle_rescale_bilinear(const float *src, int Ws, int Hs, float *dst, int Wd, int Hd);
float oracle_pow_F(float a, float b);
void oracle_rgb_to_yuv(float *const img[3], size_t s, int w, int h, const float ws[9]);
void oracle_yuv_to_rgb(float *const img[3], size_t s, int w, int h, const float ws[9]);
}

namespace {
inline float vminf(float x, float y) { return x < y ? x : y; }                  // _mm_min_ps (helpersse2.h:168-179)
inline float vmaxf(float x, float y) { return x > y ? x : y; }                  // _mm_max_ps
template <typename T> inline const T &rt_min(const T &a, const T &b) { return b < a ? b : a; }   // rt_math.h:55-58
template <typename T> inline const T &rt_max(const T &a, const T &b) { return a < b ? b : a; }   // rt_math.h:73-76
inline float LIM(float a, float b, float c) { return rt_max(b, rt_min(a, c)); }                     // rt_math.h:85-88
inline float intp(float a, float b, float c) { return a * b + (1.f - a) * c; }                     // rt_math.h:109-118
inline float SQR(float x) { return x * x; }
const float RT_INFINITY = std::numeric_limits<float>::infinity();
}

extern "C" {

struct tb_ref_region { double strength, detail_threshold; int32_t iterations; const float *mask; };   // mask: W * H floats or NULL (all ones)
struct tb_ref_info {             // the layout of artgpu_texture_boost_info
    int32_t radius, isguided, rescaled, work_w, work_h, kernel_size;
    float minval, strength, strength2;
};
struct tb_ref_counts {
    long long rescale, guided, convolution, minval_won, clamp_low, clamp_high, tail_columns, mask_partial;
};

// build_gaussian_kernel (rt_algo.cc:902-939); returns sz, coef holds sz * sz values when sz * sz <= cap
int tb_ref_gaussian_kernel(float sigma, float *coef, int cap)
{
    static constexpr float threshold = 0.005f;
    int sz = (int(std::floor(1 + 2 * std::sqrt(-2.f * SQR(sigma) * std::log(threshold)))) + 1) | 1;
    if (sz * sz > cap) return sz;
    const float two_sigma2 = 2.f * SQR(sigma);
    const auto gauss = [two_sigma2](float x) -> float { return std::exp(-SQR(x) / two_sigma2); };
    const auto gauss_integral = [&](float a, float b) -> float { return ((b - a) / 6.f) * (gauss(a) + 4.f * gauss((a + b) / 2.f) + gauss(b)); };
    std::vector<float> row(sz);
    const float halfsz = float(sz / 2);
    for (int i = 0; i < sz; ++i) {
        float x = float(i) - halfsz;
        float val = gauss_integral(x - 0.5f, x + 0.5f);
        row[i] = val;
    }
    double totd = 0.0;
    for (int i = 0; i < sz; ++i) {
        for (int j = 0; j < sz; ++j) {
            float val = row[i] * row[j];
            coef[i * sz + j] = val;
            totd += val;
        }
    }
    const float tot = totd;
    for (int i = 0; i < sz; ++i)
        for (int j = 0; j < sz; ++j) coef[i * sz + j] /= tot;
    return sz;
}

// the definition of the convolution stage (see the head of the file); src != dst
void tb_ref_conv(const float *src, float *dst, int W, int H, int K, const float *coef)
{
    const int kr = K / 2;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            float acc = 0.f;
            for (int ky = 0; ky < K; ++ky)
                for (int kx = 0; kx < K; ++kx) {
                    const int yy = std::min(std::max(y + kr - ky, 0), H - 1), xx = std::min(std::max(x + kr - kx, 0), W - 1);
                    acc += coef[ky * K + kx] * src[(size_t)yy * W + xx];
                }
            dst[(size_t)y * W + x] = acc;
        }
}
void tb_ref_conv_double(const float *src, double *dst, int W, int H, int K, const float *coef)
{
    const int kr = K / 2;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            double acc = 0.0;
            for (int ky = 0; ky < K; ++ky)
                for (int kx = 0; kx < K; ++kx) {
                    const int yy = std::min(std::max(y + kr - ky, 0), H - 1), xx = std::min(std::max(x + kr - kx, 0), W - 1);
                    acc += (double)coef[ky * K + kx] * (double)src[(size_t)yy * W + xx];
                }
            dst[(size_t)y * W + x] = acc;
        }
}

// texture_boost (L37-178) in place on a contiguous W x H plane.  Returns 0, or -1 (plane untouched) for what the device path does not
// support: the preview's gaussianBlur (!isguided && !high_detail), a gaussian above 9 x 9, iterations < 1, a guided filter whose
// subsampled grid would be empty.  `cn` is added to, not cleared.
int tb_ref_texture_boost(float *Yp, int W0, int H0, const tb_ref_region *pp, double scale, int high_detail, tb_ref_info *info, tb_ref_counts *cn)
{
    float full_radius = pp->detail_threshold * 3.5f;
    float fradius = full_radius / scale;
    int radius = std::max(int(fradius + 0.5f), 1);
    float delta = radius / fradius;

    float epsilon = 0.001f;
    float s = pp->strength >= 0 ? oracle_pow_F(pp->strength / 2.f, 0.3f) * 2.f : pp->strength;
    float strength = s >= 0 ? 1.f + s : 1.f / (1.f - s);
    float strength2 = s >= 0 ? 1.f + s / 4.f : 1.f / (1.f - s / 2.f);

    bool isguided = full_radius >= 1.f;

    int W = W0, H = H0;
    const bool rescaled = fradius > 1.f && delta > 1.01f;
    if (rescaled) {
        W = int(W * delta + 0.5f);
        H = int(H * delta + 0.5f);
    }
    float coef[81];
    int K = 0;
    if (pp->iterations < 1) return -1;
    if (!isguided) {
        if (!high_detail) return -1;
        K = tb_ref_gaussian_kernel(fradius, coef, 81);
        if (K > 9) return -1;
    }
    {
        const auto sub = [&](int r) {            // calculate_subsampling (guidedfilter.cc:58-75)
            if (r == 1 || std::max(W, H) <= 600) return 1;
            for (int q = 5; q > 0; --q)
                if (r % q == 0) return q;
            return 1;
        };
        const int s1 = isguided ? sub(radius) : 1, s2 = sub(radius * 4);
        if (W / s1 < 1 || H / s1 < 1 || W / s2 < 1 || H / s2 < 1) return -1;
    }
    const size_t N = (size_t)W * H;
    std::vector<float> tmpY;
    float *src = Yp;
    if (rescaled) {
        tmpY.resize(N);
        oracle_rescale_bilinear(Yp, W0, H0, tmpY.data(), W, H);
        src = tmpY.data();
        cn->rescale++;
    }
    std::vector<float> mid(N), base(N), conv;

    float minval = RT_INFINITY;
    constexpr float lo = 1e-5f;
    constexpr float hi = 32.f;
    for (int y = 0; y < H; ++y) {
        int x = 0;
        for (; x < W - 3; x += 4) {
            for (int k = 0; k < 4; ++k) {
                float v = src[(size_t)y * W + x + k] / 65535.f;
                src[(size_t)y * W + x + k] = v;
                mid[(size_t)y * W + x + k] = vmaxf(vminf(v, hi), lo);
                if (v < lo) cn->clamp_low++;
                if (v > hi) cn->clamp_high++;
            }
            const float *v = src + (size_t)y * W + x;
            minval = rt_min(rt_min(minval, v[0]), rt_min(rt_min(v[1], v[2]), v[3]));      // min(a, b, c, d, e): rt_math.h:54-64
        }
        for (; x < W; ++x) {
            float v = src[(size_t)y * W + x] / 65535.f;
            src[(size_t)y * W + x] = v;
            mid[(size_t)y * W + x] = LIM(v, lo, hi);
            if (v < lo) cn->clamp_low++;
            if (v > hi) cn->clamp_high++;
            minval = rt_min(minval, v);
            cn->tail_columns++;
        }
    }

    for (int i = 0; i < pp->iterations; ++i) {
        float blend = 1.f / std::pow(2.f, i);
        if (isguided) {
            oracle_guided_filter(mid.data(), mid.data(), mid.data(), W, H, radius, epsilon, 0);
            cn->guided++;
        } else {
            conv.resize(N);
            tb_ref_conv(mid.data(), conv.data(), W, H, K, coef);
            mid.swap(conv);
            cn->convolution++;
        }
        oracle_guided_filter(mid.data(), mid.data(), base.data(), W, H, radius * 4, epsilon / 10.f, 0);
        for (int y = 0; y < H; ++y) {
            int x = 0;
            for (; x < W - 3; x += 4) {
                for (int k = 0; k < 4; ++k) {
                    const size_t o = (size_t)y * W + x + k;
                    float vy = src[o], vm = mid[o], vb = base[o];
                    float d = (vy - vm) * strength;
                    float d2 = (vm - vb) * strength2;
                    if (vb + d + d2 < minval) cn->minval_won++;
                    src[o] = intp(blend, vmaxf(vb + d + d2, minval), vy);
                }
            }
            for (; x < W; ++x) {
                const size_t o = (size_t)y * W + x;
                float v = src[o];
                float d = v - mid[o];
                d *= strength;
                float d2 = mid[o] - base[o];
                d2 *= strength2;
                if (base[o] + d + d2 < minval) cn->minval_won++;
                src[o] = intp(blend, rt_max(base[o] + d + d2, minval), v);
            }
        }
    }
    for (size_t k = 0; k < N; ++k) src[k] = src[k] * 65535.f;
    if (src != Yp) oracle_rescale_bilinear(src, W, H, Yp, W0, H0);
    if (info) {
        info->radius = radius; info->isguided = isguided; info->rescaled = rescaled; info->work_w = W; info->work_h = H; info->kernel_size = K;
        info->minval = minval; info->strength = strength; info->strength2 = strength2;
    }
    return 0;
}

// ImProcFunctions::textureBoost (L198-242) in place on three contiguous W x H planes in RGB mode: setMode(YUV), the regions with
// strength != 0 in order with their blends, setMode(RGB) when to_rgb.  `regions` holds the enabled regions.  Returns 0, or -1 (planes
// untouched) when a region is unsupported.
int tb_ref_tool(float *r, float *g, float *b, int W, int H, const tb_ref_region *regions, int nregions, const double *ws, double scale, int high_detail,
                int to_rgb, tb_ref_info *info, tb_ref_counts *cn)
{
    const size_t N = (size_t)W * H;
    std::memset(info, 0, sizeof *info);
    std::memset(cn, 0, sizeof *cn);
    {
        tb_ref_counts scratch = {};
        std::vector<float> probe(N);
        for (int i = 0; i < nregions; ++i) {
            if (regions[i].strength == 0) continue;
            std::copy(g, g + N, probe.begin());
            if (tb_ref_texture_boost(probe.data(), W, H, &regions[i], scale, high_detail, nullptr, &scratch)) return -1;
        }
    }
    float wsf[9];
    for (int k = 0; k < 9; ++k) wsf[k] = (float)ws[k];
    float *img[3] = {r, g, b};
    oracle_rgb_to_yuv(img, W, W, H, wsf);
    std::vector<float> Y(g, g + N);
    for (int i = 0; i < nregions; ++i) {
        const tb_ref_region &reg = regions[i];
        if (reg.strength != 0) {
            tb_ref_texture_boost(Y.data(), W, H, &reg, scale, high_detail, info, cn);
            for (size_t k = 0; k < N; ++k) {
                const float blend = reg.mask ? reg.mask[k] : 1.f;
                if (blend > 0.f && blend < 1.f) cn->mask_partial++;
                float &YY = g[k];
                YY = intp(blend, Y[k], YY);
                Y[k] = YY;
            }
        }
    }
    if (to_rgb) oracle_yuv_to_rgb(img, W, W, H, wsf);
    return 0;
}

} // extern "C"
