// tests/emul/toneeq_ref.cc -- CPU checker for artgpu_tone_equalizer: ImProcFunctions::toneEqualizer (rtengine/iptoneequalizer.cc:345-371) and
// tone_eq (L69-340) restated serially on contiguous float planes, with every plane the reference has (the image times gain, Y, Y2, the
// image times 1.f / gain).  Test infrastructure only; built on first use with -ffp-contract=off.
//
// The leaves are liboracle's restatements: oracle_guided_filter (rtengine::guidedFilter; guidedFilterLog is written out around it),
// the scalar and 4-lane sleef forms (oracle_xlogf_s / _v, oracle_xexpf_s / _v, oracle_pow_F, oracle_xlin2log / oracle_xlog2lin) and the two
// LUTf lookups (oracle_lutf: operator[](float) of a clipping table; oracle_lutf_vec: operator[](vfloat)).  iptoneequalizer.cc itself needs
// improcfun.h and lcms2 and is not compiled anywhere: the loop is parity-unpinned, its leaves are pinned.
// The group-of-four body (L318-330) is written lane by lane with the 4-lane forms, the tail (L332-338) with the scalar ones.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

extern "C" {
void oracle_guided_filter(const float *guide, const float *src, float *dst, int W, int H, int r, float epsilon, int subsampling);
float oracle_xlin2log(float x, float base);
float oracle_xlog2lin(float x, float base);
float oracle_xlogf_s(float d);
float oracle_xlogf_v(float d);
float oracle_xexpf_s(float d);
float oracle_xexpf_v(float d);
float oracle_pow_F(float a, float b);
float oracle_lutf(const float *data, int size, float index);
float oracle_lutf_vec(const float *data, int size, float index);
}

extern "C" {
struct te_ref_params {             // the layout of artgpu_tone_equalizer_params
    int32_t enabled, bands[5], regularization, show_colormap;
    double pivot;
};
struct te_ref_info {               // the layout of artgpu_tone_equalizer_info
    float gain, w_sum, factors[12];
    int32_t filters, radius[3], subsampling[3], box_radius[3];
    float epsilon[3];
};
struct te_ref_counts {
    long long groups_analytic, groups_table, tail_above, tail_table, y_clamped_lo, y_clamped_hi, luma_clamped_lo, luma_clamped_hi;
    long long post_clamped_lo, post_clamped_hi, groups_one_lane;
};
}

namespace {

constexpr int MIN_SIZE = 5, MAX_BOX_RADIUS = 900;
const float centers[12] = {-16.0f, -14.0f, -12.0f, -10.0f, -8.0f, -6.0f, -4.0f, -2.0f, 0.0f, 2.0f, 4.0f, 6.0f};

inline float maxf(float a, float b) { return a < b ? b : a; }       // rtengine::max / std::max
inline float minf(float a, float b) { return b < a ? b : a; }
inline float limf(float v, float lo, float hi) { return maxf(lo, minf(v, hi)); }      // LIM (rt_math.h:85-88)
inline float vmaxf(float a, float b) { return a > b ? a : b; }     // _mm_max_ps: the second operand unless a > b
inline float vminf(float a, float b) { return a < b ? a : b; }     // _mm_min_ps

float log2_s(float x) { return oracle_xlogf_s(x) / oracle_xlogf_s(2); }               // L75-80
float exp2_s(float x) { return oracle_pow_F(2.f, x); }                                // L82-86
float gauss_s(float b, float x) { return oracle_xexpf_s((-((x - b) * (x - b)) / 4.0f)); }
float gauss_v(float b, float x) { return oracle_xexpf_v((-((x - b) * (x - b)) / 4.f)); }

int calculate_subsampling(int w, int h, int r)                       // guidedfilter.cc:58-75
{
    if (r == 1) return 1;
    if (std::max(w, h) <= 600) return 1;
    for (int s = 5; s > 0; --s)
        if (r % s == 0) return s;
    return std::max(2, std::min(r / 2, 4));
}

struct Tool {
    float factors[12], w_sum;
    te_ref_counts *cn;
    bool count;
    float process_pixel(float y) const                               // L175-190
    {
        const float l = log2_s(maxf(y, 0.f));
        if (count) { if (l < -14.f) ++cn->luma_clamped_lo; if (l > 4.f) ++cn->luma_clamped_hi; }
        const float luma = limf(l, -14.f, 4.f);
        float correction = 0.0f;
        for (int c = 0; c < 12; ++c) correction += gauss_s(centers[c], luma) * factors[c];
        correction /= w_sum;
        return correction;
    }
    float vprocess_pixel(float y) const                              // L258-270, one lane
    {
        const float l = oracle_xlogf_v(vmaxf(y, 0.f)) / oracle_xlogf_s(2.f);
        if (count) { if (l < -14.f) ++cn->luma_clamped_lo; if (l > 4.f) ++cn->luma_clamped_hi; }
        const float luma = vminf(vmaxf(l, -14.f), 4.f);
        float correction = 0.f;
        for (int c = 0; c < 12; ++c) correction += gauss_v(centers[c], luma) * factors[c];
        correction /= w_sum;
        return correction;
    }
};

void derive(const te_ref_params &p, te_ref_info *o)
{
    const auto conv = [](int v, float lo, float hi) -> float { const float f = v < 0 ? lo : hi; return exp2_s(float(v) / 100.f * f); };
    const float f[12] = {conv(p.bands[0], 2.f, 3.f), conv(p.bands[0], 2.f, 3.f), conv(p.bands[0], 2.f, 3.f), conv(p.bands[0], 2.f, 3.f), conv(p.bands[0], 2.f, 3.f),
                         conv(p.bands[1], 2.f, 3.f), conv(p.bands[2], 2.5f, 2.5f), conv(p.bands[3], 3.f, 2.f), conv(p.bands[4], 3.f, 2.f), conv(p.bands[4], 3.f, 2.f),
                         conv(p.bands[4], 3.f, 2.f), conv(p.bands[4], 3.f, 2.f)};
    std::copy(f, f + 12, o->factors);
    const float gain = 1.f / 65535.f * std::pow(2.f, -p.pivot);      // L354
    o->gain = gain;
    float w_sum = 0.f;
    for (int i = 0; i < 12; ++i) w_sum += gauss_s(centers[i], 0.f);
    o->w_sum = w_sum;
}

// one guidedFilter call of the tool: returns 1 where the device path does not run it
int plan_filter(int W, int H, int k, int r, float epsilon, te_ref_info *o)
{
    if (r <= 0) return 1;
    const int sub = calculate_subsampling(W, H, r), w = W / sub, h = H / sub;
    if (w < MIN_SIZE || h < MIN_SIZE) return 1;
    const float r1 = float(r) / sub;                                 // f_mean (guidedfilter.cc:160-167)
    int rad = r1;
    rad = std::max(0, std::min(rad, (std::min(w, h) - 1) / 2 - 1));
    if (rad > MAX_BOX_RADIUS) return 1;
    o->radius[k] = r; o->subsampling[k] = sub; o->box_radius[k] = rad; o->epsilon[k] = epsilon;
    ++o->filters;
    return 0;
}

int plan(const te_ref_params &p, int W, int H, double scale, te_ref_info *o)
{
    *o = te_ref_info{};
    if (p.show_colormap || p.regularization < 0 || p.regularization > 4 || !(scale >= 1.0) || std::isinf(scale)) return 1;
    derive(p, o);
    if (p.regularization == 0) return 0;
    const int detail = p.regularization > 0 ? 5 : 0;
    int radius = float(detail) / scale + 0.5f;                       // L128
    float epsilon = 0.01f + 0.002f * std::max(detail - 3, 0);
    if (radius > 0 && plan_filter(W, H, 0, radius, epsilon, o)) return 1;
    if (p.regularization > 1) {
        constexpr float base_epsilon = 0.004f;
        radius = 350.f / scale;
        epsilon = base_epsilon;
        if (plan_filter(W, H, 1, radius, epsilon, o)) return 1;
        const int reg = 5 - std::min(p.regularization, 4);
        if (reg > 1 && plan_filter(W, H, 2, radius * (reg - 1), epsilon / 100, o)) return 1;
    }
    return 0;
}

} // namespace

extern "C" {

int te_ref_sizes(int which) { return which == 0 ? (int)sizeof(te_ref_params) : (int)sizeof(te_ref_info); }

// the correction table and what goes with it, as tone_eq builds them
void te_ref_lut(const te_ref_params *p, float *lut, te_ref_info *info)
{
    te_ref_info o = {};
    derive(*p, &o);
    Tool t;
    std::copy(o.factors, o.factors + 12, t.factors);
    t.w_sum = o.w_sum; t.cn = nullptr; t.count = false;
    for (int i = 0; i < 65536; ++i) {
        float y = float(i) / 65535.f;
        lut[i] = t.process_pixel(y);
    }
    if (info) *info = o;
}

// 0: done; 1: unsupported on the device path (planes untouched); 2: bad arguments
int te_ref_tool(float *R, float *G, float *B, int W, int H, const te_ref_params *p, const double ws[9], double scale, te_ref_info *info, te_ref_counts *cn)
{
    te_ref_counts dummy = {};
    if (!cn) cn = &dummy;
    if (!p || !ws || W < 1 || H < 1 || std::isnan(scale)) return 2;
    if (!p->enabled) return 0;
    te_ref_info o;
    if (plan(*p, W, H, scale, &o)) return 1;
    if (info) *info = o;
    const size_t n = (size_t)W * H;
    const float gain = o.gain;
    for (size_t k = 0; k < n; ++k) { R[k] *= gain; G[k] *= gain; B[k] *= gain; }       // rgb->multiply(gain)
    std::vector<float> Y(n);
    for (size_t k = 0; k < n; ++k) {
        const float l = R[k] * ws[3] + G[k] * ws[4] + B[k] * ws[5];                  // Color::rgbLuminance with the TMatrix: double, narrowed once
        if (l < 1e-5f) ++cn->y_clamped_lo;
        if (l > 32.f) ++cn->y_clamped_hi;
        Y[k] = limf(l, 1e-5f, 32.f);
    }
    if (o.radius[0] > 0) {                                            // guidedFilterLog(10.f, Y, radius, epsilon) (guidedfilter.cc:244-271)
        for (size_t k = 0; k < n; ++k) Y[k] = oracle_xlin2log(maxf(Y[k], 0.f), 10.f);
        oracle_guided_filter(Y.data(), Y.data(), Y.data(), W, H, o.radius[0], o.epsilon[0], 0);
        for (size_t k = 0; k < n; ++k) Y[k] = oracle_xlog2lin(maxf(Y[k], 0.f), 10.f);
    }
    if (p->regularization > 1) {
        std::vector<float> Y2(n);
        for (size_t k = 0; k < n; ++k) {
            const float lg = log2_s(maxf(Y[k], 1e-9f));
            if (lg < centers[0]) ++cn->post_clamped_lo;
            if (lg > centers[11]) ++cn->post_clamped_hi;
            float l = limf(lg, centers[0], centers[11]);
            float ll = std::round(l * 5.f) / 5.f;
            Y2[k] = Y[k];
            Y[k] = exp2_s(ll);
        }
        oracle_guided_filter(Y2.data(), Y.data(), Y.data(), W, H, o.radius[1], o.epsilon[1], 0);
        if (o.radius[2] > 0) oracle_guided_filter(Y2.data(), Y.data(), Y.data(), W, H, o.radius[2], o.epsilon[2], 0);
    }
    Tool t;
    std::copy(o.factors, o.factors + 12, t.factors);
    t.w_sum = o.w_sum; t.cn = cn; t.count = false;
    std::vector<float> lut(65536);
    for (int i = 0; i < 65536; ++i) lut[i] = t.process_pixel(float(i) / 65535.f);
    t.count = true;
    for (int y = 0; y < H; ++y) {
        int x = 0;
        for (; x < W - 3; x += 4) {
            const float *cY = &Y[(size_t)y * W + x];
            const int above = (cY[0] > 1.f) + (cY[1] > 1.f) + (cY[2] > 1.f) + (cY[3] > 1.f);
            if (above) ++cn->groups_analytic; else ++cn->groups_table;
            if (above == 1) ++cn->groups_one_lane;
            for (int k = 0; k < 4; ++k) {
                const size_t i = (size_t)y * W + x + k;
                const float corr = above ? t.vprocess_pixel(cY[k]) : oracle_lutf_vec(lut.data(), 65536, cY[k] * 65535.f);
                R[i] *= corr; G[i] *= corr; B[i] *= corr;
            }
        }
        for (; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            const float cY = Y[i];
            if (cY > 1.f) ++cn->tail_above; else ++cn->tail_table;
            const float corr = cY > 1.f ? t.process_pixel(cY) : oracle_lutf(lut.data(), 65536, cY * 65535.f);
            R[i] *= corr; G[i] *= corr; B[i] *= corr;
        }
    }
    const float back = 1.f / gain;
    for (size_t k = 0; k < n; ++k) { R[k] *= back; G[k] *= back; B[k] *= back; }       // rgb->multiply(1.f / gain)
    return 0;
}

} // extern "C"
