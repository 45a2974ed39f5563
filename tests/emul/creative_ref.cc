// tests/emul/creative_ref.cc -- CPU checker for artgpu_soft_light, artgpu_black_and_white and artgpu_creative_gradients:
// ImProcFunctions::softLight (rtengine/ipsoftlight.cc:31-82), ImProcFunctions::blackAndWhite with computeBWMixerConstants (rtengine/ipbw.cc:50-365)
// and, in the second half of the file, ImProcFunctions::creativeGradients (rtengine/iptransform.cc), restated serially in the reference's own
// loop order.  Test infrastructure only; built on first use with -ffp-contract=off.
//
// The leaves are liboracle's restatements: oracle_lutf (LUTf::operator[](float) of a table that clips on both sides), oracle_lutf_noclip (of a
// table constructed with flags 0), oracle_lutf_vec (operator[](vfloat), one lane), oracle_pow_F (sleef.h's scalar pow_F) and the YUV mode switches
// of imagefloat.cc.  ipsoftlight.cc and ipbw.cc need the image classes, glibmm and the curve code and are not compiled anywhere: the loops
// are parity-unpinned, their leaves are pinned.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

extern "C" {
float oracle_lutf(const float *data, int size, float index);
float oracle_lutf_noclip(const float *data, int size, float index);
float oracle_lutf_vec(const float *data, int size, float index);
float oracle_pow_F(float a, float b);
void oracle_rgb_to_yuv(float *const img[3], size_t s, int w, int h, const float ws[9]);
void oracle_yuv_to_rgb(float *const img[3], size_t s, int w, int h, const float ws[9]);
}

extern "C" {
struct cr_sl_counts { long long below_zero, in_table, above_max, nan; };       // channel values by the branch of `apply` they take
struct cr_bw_counts { long long body, tail; };                                 // pixels of the 4-wide loop and of the scalar tail
struct cr_bw_mixer { float bwr, bwg, bwb, kcorec, filcor; double rrm, ggm, bbm; };
}

namespace {

struct Tables {
    std::vector<float> gamma, igamma;
    Tables() : gamma(65536), igamma(65536)
    {
        // Color::init (color.cc:239-255) with gamma2 / igamma2 (color.h:1122-1147)
        for (int i = 0; i < 65536; i++) {
            const double x = i / 65535.0;
            gamma[i] = x <= 0.003040 ? x * 12.92310 : 1.055 * std::exp(std::log(x) / 2.4) - 0.055;
        }
        for (int i = 0; i < 65536; i++) gamma[i] *= 65535.f;
        for (int i = 0; i < 65536; i++) {
            const double x = i / 65535.0;
            igamma[i] = x <= 0.039286 ? x / 12.92310 : std::exp(std::log((x + 0.055) / 1.055) * 2.4);
        }
        for (int i = 0; i < 65536; i++) igamma[i] *= 65535.f;
    }
};
const Tables &tables() { static const Tables t; return t; }

template <typename T> T intp(T a, T b, T c) { return a * b + (T(1) - a) * c; }     // rt_math.h:110-118

// ipsoftlight.cc:31-41
float sl(float blend, float x)
{
    const Tables &t = tables();
    float v = oracle_lutf_noclip(t.gamma.data(), 65536, x) / 65535.f;              // Color::gamma_srgb(float)
    float v2 = v * v;
    float v22 = v2 * 2.f;
    v = v2 + v22 - v22 * v;
    x = intp(blend, oracle_lutf_noclip(t.igamma.data(), 65536, v * 65535.f), x);    // Color::igamma_srgb(float)
    return x;
}

} // namespace

extern "C" {

// LUTf f(65536); f[i] = sl(blend, i) (L55-60)
void cr_soft_light_lut(int strength, float *f)
{
    const float blend = strength / 100.f;
    for (int i = 0; i < 65536; ++i) f[i] = sl(blend, i);
}

// softLight on three h x w planes with a row stride of `stride` floats; returns 0 when the tool does not run (L48-51)
int cr_soft_light(float *r, float *g, float *b, size_t stride, int w, int h, int enabled, int strength, cr_sl_counts *cn)
{
    std::memset(cn, 0, sizeof *cn);
    if (!(enabled && strength > 0)) return 0;
    std::vector<float> f(65536);
    cr_soft_light_lut(strength, f.data());
    const auto apply = [&](float x) -> float {
        if (x <= 65535.f) {
            if (x < 0.f) ++cn->below_zero; else ++cn->in_table;
            return oracle_lutf(f.data(), 65536, x);
        } else {
            if (x != x) ++cn->nan; else ++cn->above_max;
            return x;
        }
    };
    float *pl[3] = {r, g, b};
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            for (int c = 0; c < 3; ++c) pl[c][(size_t)y * stride + x] = apply(pl[c][(size_t)y * stride + x]);
    return 1;
}

// computeBWMixerConstants (ipbw.cc:50-211) with the setting and the filter as the reference's strings, algo "", kcorec = 1.f on entry (L258)
void cr_bw_mixer_constants(const char *setting_, const char *filter_, int mr, int mg, int mb, cr_bw_mixer *o)
{
    const std::string setting(setting_), filter(filter_);
    float mixerRed = float(mr), mixerGreen = float(mg), mixerBlue = float(mb);
    float kcorec = 1.f, filcor;
    double rrm, ggm, bbm;

    float somm;
    float som = mixerRed + mixerGreen + mixerBlue;
    if (som >= 0.f && som < 1.f) { som = 1.f; }
    if (som < 0.f && som > -1.f) { som = -1.f; }
    static const struct { const char *name; float v[3]; } presets[] = {
        {"NormalContrast", {43.f, 33.f, 30.f}}, {"Panchromatic", {33.3f, 33.3f, 33.3f}}, {"HyperPanchromatic", {41.f, 25.f, 34.f}},
        {"LowSensitivity", {27.f, 27.f, 46.f}}, {"HighSensitivity", {30.f, 28.f, 42.f}}, {"Orthochromatic", {0.f, 42.f, 58.f}},
        {"HighContrast", {40.f, 34.f, 60.f}}, {"Luminance", {30.f, 59.f, 11.f}}, {"Landscape", {66.f, 24.f, 10.f}},
        {"Portrait", {54.f, 44.f, 12.f}}, {"InfraRed", {-40.f, 200.f, -17.f}}};
    for (const auto &p : presets)
        if (setting == p.name) { mixerRed = p.v[0]; mixerGreen = p.v[1]; mixerBlue = p.v[2]; }
    if (setting == "RGB-Abs" || setting == "ROYGCBPM-Abs") { kcorec = som / 100.f; }
    rrm = mixerRed;
    ggm = mixerGreen;
    bbm = mixerBlue;
    somm = mixerRed + mixerGreen + mixerBlue;
    if (somm >= 0.f && somm < 1.f) { somm = 1.f; }
    if (somm < 0.f && somm > -1.f) { somm = -1.f; }
    mixerRed = mixerRed / somm;
    mixerGreen = mixerGreen / somm;
    mixerBlue = mixerBlue / somm;
    float filred = 1.f, filgreen = 1.f, filblue = 1.f;
    filcor = 1.f;
    static const struct { const char *name; float v[4]; } filters[] = {
        {"None", {1.f, 1.f, 1.f, 1.f}}, {"Red", {1.f, 0.05f, 0.f, 1.08f}}, {"Orange", {1.f, 0.6f, 0.f, 1.35f}}, {"Yellow", {1.f, 1.f, 0.05f, 1.23f}},
        {"YellowGreen", {0.6f, 1.f, 0.3f, 1.32f}}, {"Green", {0.2f, 1.f, 0.3f, 1.41f}}, {"Cyan", {0.05f, 1.f, 1.f, 1.23f}},
        {"Blue", {0.f, 0.05f, 1.f, 1.20f}}, {"Purple", {1.f, 0.05f, 1.f, 1.23f}}};
    for (const auto &p : filters)
        if (filter == p.name) { filred = p.v[0]; filgreen = p.v[1]; filblue = p.v[2]; filcor = p.v[3]; }
    mixerRed = mixerRed * filred;
    mixerGreen = mixerGreen * filgreen;
    mixerBlue = mixerBlue * filblue;
    if (mixerRed + mixerGreen + mixerBlue == 0) { mixerRed += 1.f; }
    mixerRed = filcor * mixerRed / (mixerRed + mixerGreen + mixerBlue);
    mixerGreen = filcor * mixerGreen / (mixerRed + mixerGreen + mixerBlue);
    mixerBlue = filcor * mixerBlue / (mixerRed + mixerGreen + mixerBlue);
    if (filter != "None") {
        som = mixerRed + mixerGreen + mixerBlue;
        if (som >= 0.f && som < 1.f) { som = 1.f; }
        if (som < 0.f && som > -1.f) { som = -1.f; }
        if (setting == "RGB-Abs") { kcorec = kcorec * som; }
    }
    o->bwr = mixerRed; o->bwg = mixerGreen; o->bwb = mixerBlue; o->kcorec = kcorec; o->filcor = filcor;
    o->rrm = rrm; o->ggm = ggm; o->bbm = bbm;
}

// blackAndWhite (L214-365) on three h x w planes.  ulut / vlut: the colour cast's tables, used when cast_bottom > 0; ws: the working-space
// matrix as floats (Imagefloat::ws_).  The image leaves in RGB mode when there is no cast and in YUV mode when there is one, as in the reference
void cr_black_and_white(float *r, float *g, float *b, size_t stride, int W, int H, const char *setting, const char *filter, const int mixer[3],
                        const int gamma[3], int cast_bottom, const float *ulut, const float *vlut, const float ws[9], cr_bw_counts *cn)
{
    std::memset(cn, 0, sizeof *cn);
    float bwrgam = float(gamma[0]), bwggam = float(gamma[1]), bwbgam = float(gamma[2]);
    float gamvalr = 125.f, gamvalg = 125.f, gamvalb = 125.f;
    if (bwrgam < 0) { gamvalr = 100.f; }
    if (bwggam < 0) { gamvalg = 100.f; }
    if (bwbgam < 0) { gamvalb = 100.f; }
    const float gammabwr = 1.f - bwrgam / gamvalr;
    const float gammabwg = 1.f - bwggam / gamvalg;
    const float gammabwb = 1.f - bwbgam / gamvalb;
    const bool hasgammabw = gammabwr != 1.f || gammabwg != 1.f || gammabwb != 1.f;
    cr_bw_mixer m;
    cr_bw_mixer_constants(setting, filter, mixer[0], mixer[1], mixer[2], &m);
    const float bwr = m.bwr, bwg = m.bwg, bwb = m.bwb, kcorec = m.kcorec;
    std::vector<float> gamma_r, gamma_g, gamma_b;
    if (hasgammabw) {
        gamma_r.resize(65536); gamma_g.resize(65536); gamma_b.resize(65536);
        for (int i = 0; i < 65536; ++i) {
            gamma_r[i] = oracle_pow_F(float(i) / 65535.f, gammabwr) * 65535.f;
            gamma_g[i] = oracle_pow_F(float(i) / 65535.f, gammabwg) * 65535.f;
            gamma_b[i] = oracle_pow_F(float(i) / 65535.f, gammabwb) * 65535.f;
        }
    }
    for (int y = 0; y < H; ++y) {
        float *rr = r + (size_t)y * stride, *gg = g + (size_t)y * stride, *bb = b + (size_t)y * stride;
        int x = 0;
        for (; x < W - 3; x += 4)
            for (int k = 0; k < 4; ++k) {
                float rv = rr[x + k], gv = gg[x + k], bv = bb[x + k];
                if (hasgammabw) {
                    rv = oracle_lutf_vec(gamma_r.data(), 65536, rv);
                    gv = oracle_lutf_vec(gamma_g.data(), 65536, gv);
                    bv = oracle_lutf_vec(gamma_b.data(), 65536, bv);
                }
                const float bw = ((bwr * rv + bwg * gv + bwb * bv) * kcorec);
                rr[x + k] = bw; gg[x + k] = bw; bb[x + k] = bw;
                ++cn->body;
            }
        for (; x < W; ++x) {
            float rv = rr[x], gv = gg[x], bv = bb[x];
            if (hasgammabw) {
                rv = oracle_lutf(gamma_r.data(), 65536, rv);
                gv = oracle_lutf(gamma_g.data(), 65536, gv);
                bv = oracle_lutf(gamma_b.data(), 65536, bv);
            }
            rr[x] = gg[x] = bb[x] = ((bwr * rv + bwg * gv + bwb * bv) * kcorec);
            ++cn->tail;
        }
    }
    if (cast_bottom > 0) {
        float *img[3] = {r, g, b};
        oracle_rgb_to_yuv(img, stride, W, H, ws);                                  // img->setMode(Imagefloat::Mode::YUV)
        for (int y = 0; y < H; ++y) {
            float *rr = r + (size_t)y * stride, *gg = g + (size_t)y * stride, *bb = b + (size_t)y * stride;
            int x = 0;
            for (; x < W - 3; x += 4)
                for (int k = 0; k < 4; ++k) {
                    const float yv = gg[x + k];
                    const float uv = oracle_lutf_vec(ulut, 65536, yv);
                    const float vv = oracle_lutf_vec(vlut, 65536, yv);
                    bb[x + k] = bb[x + k] + uv;
                    rr[x + k] = rr[x + k] + vv;
                }
            for (; x < W; ++x) {
                const float u = oracle_lutf(ulut, 65536, gg[x]);
                const float v = oracle_lutf(vlut, 65536, gg[x]);
                bb[x] += u;
                rr[x] += v;
            }
        }
    }
}

void cr_yuv_to_rgb(float *r, float *g, float *b, size_t stride, int W, int H, const float ws[9])
{
    float *img[3] = {r, g, b};
    oracle_yuv_to_rgb(img, stride, W, H, ws);
}

} // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------------------
// ImProcFunctions::creativeGradients (rtengine/iptransform.cc:1390-1408): calcGradientParams / calcGradientFactor (L677-812),
// calcPCVignetteParams / calcPCVignetteFactor (L828-983), normn / pown / pow3 / pow4 (L36-89) and the creative branch of
// transformLuminanceOnly (L987-1048), in the reference's own words.  Unqualified sqrt / fabs on a float are the float overloads, as in the
// reference's translation unit (<math.h> is in scope there).  The leaves: sleef.h's scalar xsinf (L993-1016), its scalar xcosf, which under
// SSE2 is lane 0 of sleefsseavx.h's vector form (L1024-1049; written with the intrinsics here), liboracle's xcbrtf and pow_F.
// ---------------------------------------------------------------------------------------------------------------------------------------
#include <emmintrin.h>
#include <math.h>
#include <algorithm>

extern "C" float oracle_xcbrtf(float d);

extern "C" {
struct cr_cg_params {               // the layout of artgpu_creative_gradients_params
    int32_t gradient_enabled; double gradient_degree; int32_t gradient_feather; double gradient_strength; int32_t gradient_center_x, gradient_center_y;
    int32_t pcvignette_enabled; double pcvignette_strength; int32_t pcvignette_feather, pcvignette_roundness, pcvignette_center_x, pcvignette_center_y;
    int32_t crop_enabled, crop_x, crop_y, crop_w, crop_h;
    int32_t offset_x, offset_y, full_width, full_height; double scale;
};
struct cr_cg_derived {              // the layout of artgpu_creative_gradient_derived
    int32_t apply_gradient, apply_pcvignette, cx, cy;
    int32_t angle_is_zero, transpose, bright_top, h;
    float ta, yc, xc, ys, ys_inv, scale, botmul, topmul, top_edge_0;
    float oe_a, oe_b, oe1_a, oe1_b, oe2_a, oe2_b, ie_mul, ie1_mul, ie2_mul, sepmix, feather;
    int32_t x1, x2, y1, y2, ex, ey, ew, eh, sep, is_super_ellipse_mode, is_portrait;
    float pcv_scale, fadeout_mul;
};
struct cr_cg_counts {
    long long g_top, g_bottom, g_ramp_sin, g_ramp_cos, g_angle_zero, g_angled, g_transposed;      // gradient: pixels by branch
    long long v_faded, v_fade_out, v_inside, v_outside, v_ramp_cos, v_ramp_sin, v_normn[4], v_portrait, v_dist_zero;   // vignette (v_normn: degrees 2, 4, 6, 8 of the super-ellipses)
};
}

namespace {

constexpr double RT_PI = 3.14159265358979323846;
constexpr float RT_PI_F_2 = 1.57079632679489661923;
constexpr float RT_1_PI_F = 0.31830988618379067154;
constexpr float PI4_Af = 0.78515625f, PI4_Bf = 0.00024127960205078125f, PI4_Cf = 6.3329935073852539062e-07f, PI4_Df = 4.9604681473525147339e-10f;

inline float mlaf(float x, float y, float z) { return x * y + z; }
inline int xrintf(float x) { return _mm_cvtss_si32(_mm_set_ss(x)); }

float xsinf(float d)
{
    int q;
    float u, s;
    q = xrintf(d * RT_1_PI_F);
    d = mlaf(q, -PI4_Af * 4, d);
    d = mlaf(q, -PI4_Bf * 4, d);
    d = mlaf(q, -PI4_Cf * 4, d);
    d = mlaf(q, -PI4_Df * 4, d);
    s = d * d;
    if ((q & 1) != 0) d = -d;
    u = 2.6083159809786593541503e-06f;
    u = mlaf(u, s, -0.0001981069071916863322258f);
    u = mlaf(u, s, 0.00833307858556509017944336f);
    u = mlaf(u, s, -0.166666597127914428710938f);
    u = mlaf(s, u * d, d);
    return u;
}

float xcosf(float dd)
{
    __m128 d = _mm_set_ss(dd);
    __m128i q = _mm_cvtps_epi32(_mm_sub_ps(_mm_mul_ps(d, _mm_set1_ps((float)0.318309886183790671537767526745028724)), _mm_set1_ps(0.5f)));
    q = _mm_add_epi32(_mm_add_epi32(q, q), _mm_set1_epi32(1));
    __m128 u = _mm_cvtepi32_ps(q);
    d = _mm_add_ps(_mm_mul_ps(u, _mm_set1_ps(-PI4_Af * 2)), d);
    d = _mm_add_ps(_mm_mul_ps(u, _mm_set1_ps(-PI4_Bf * 2)), d);
    d = _mm_add_ps(_mm_mul_ps(u, _mm_set1_ps(-PI4_Cf * 2)), d);
    d = _mm_add_ps(_mm_mul_ps(u, _mm_set1_ps(-PI4_Df * 2)), d);
    __m128 s = _mm_mul_ps(d, d);
    const __m128 keep = _mm_castsi128_ps(_mm_cmpeq_epi32(_mm_and_si128(q, _mm_set1_epi32(2)), _mm_set1_epi32(2)));
    const __m128 neg = _mm_xor_ps(_mm_castsi128_ps(_mm_set1_epi32((int)0x80000000)), d);
    d = _mm_or_ps(_mm_and_ps(keep, d), _mm_andnot_ps(keep, neg));
    u = _mm_set1_ps(2.6083159809786593541503e-06f);
    u = _mm_add_ps(_mm_mul_ps(u, s), _mm_set1_ps(-0.0001981069071916863322258f));
    u = _mm_add_ps(_mm_mul_ps(u, s), _mm_set1_ps(0.00833307858556509017944336f));
    u = _mm_add_ps(_mm_mul_ps(u, s), _mm_set1_ps(-0.166666597127914428710938f));
    u = _mm_add_ps(_mm_mul_ps(s, _mm_mul_ps(u, d)), d);
    return _mm_cvtss_f32(u);
}

float pow3(float x) { return x * x * x; }
float pow4(float x) { return (x * x) * (x * x); }
float pown(float x, int n)
{
    switch (n) {
    case 0: return 1;
    case 2: return x * x;
    case 4: return pow4(x);
    case 6: return (x * x) * pow4(x);
    case 8: return pow4(x) * pow4(x);
    default: return oracle_pow_F(x, n);
    }
}
float normn(float a, float b, int n)
{
    switch (n) {
    case 2: return sqrtf(a * a + b * b);
    case 4: return sqrtf(sqrtf(pow4(a) + pow4(b)));
    case 6: return sqrtf(oracle_xcbrtf(pow3(a) * pow3(a) + pow3(b) * pow3(b)));
    case 8: return sqrtf(sqrtf(sqrtf(pow4(a) * pow4(a) + pow4(b) * pow4(b))));
    default: return oracle_pow_F(pown(a, n) + pown(b, n), 1.f / n);
    }
}
template <typename T> T SQR(T x) { return x * x; }

struct grad_params {
    bool angle_is_zero, transpose, bright_top;
    float ta, yc, xc;
    float ys, ys_inv;
    float scale, botmul, topmul;
    float top_edge_0;
    int h;
};
struct GradientParams { bool enabled; double degree; int feather; double strength; int centerX; int centerY; };
struct PCVignetteParams { bool enabled; double strength; int feather; int roundness; int centerX; int centerY; };
struct CropParams { bool enabled; int x, y, w, h; };

void calcGradientParams(int oW, int oH, const GradientParams &gradient, struct grad_params &gp)
{
    int w = oW;
    int h = oH;
    double gradient_stops = gradient.strength;
    double gradient_span = gradient.feather / 100.0;
    double gradient_center_x = gradient.centerX / 200.0 + 0.5;
    double gradient_center_y = gradient.centerY / 200.0 + 0.5;
    double gradient_angle = gradient.degree / 180.0 * RT_PI;
    gradient_angle = fmod(gradient_angle, 2 * RT_PI);
    if (gradient_angle < 0.0) { gradient_angle += 2.0 * RT_PI; }
    gp.bright_top = false;
    gp.transpose = false;
    gp.angle_is_zero = false;
    gp.h = h;
    double cosgrad = cos(gradient_angle);
    if (fabs(cosgrad) < 0.707) {
        gp.transpose = true;
        gradient_angle += 0.5 * RT_PI;
        double gxc = gradient_center_x;
        gradient_center_x = 1.0 - gradient_center_y;
        gradient_center_y = gxc;
    }
    gradient_angle = fmod(gradient_angle, 2 * RT_PI);
    if (gradient_angle > 0.5 * RT_PI && gradient_angle < RT_PI) {
        gradient_angle += RT_PI;
        gp.bright_top = true;
    } else if (gradient_angle >= RT_PI && gradient_angle < 1.5 * RT_PI) {
        gradient_angle -= RT_PI;
        gp.bright_top = true;
    }
    if (fabs(gradient_angle) < 0.001 || fabs(gradient_angle - 2 * RT_PI) < 0.001) {
        gradient_angle = 0;
        gp.angle_is_zero = true;
    }
    if (gp.transpose) { gp.bright_top = !gp.bright_top; }
    if (gp.transpose) { int tmp = w; w = h; h = tmp; }
    gp.scale = 1.0 / pow(2, gradient_stops);
    if (gp.bright_top) { gp.topmul = 1.0; gp.botmul = gp.scale; }
    else { gp.topmul = gp.scale; gp.botmul = 1.0; }
    gp.ta = tan(gradient_angle);
    gp.xc = w * gradient_center_x;
    gp.yc = h * gradient_center_y;
    gp.ys = sqrt((float)h * h + (float)w * w) * (gradient_span / cos(gradient_angle));
    gp.ys_inv = 1.0 / gp.ys;
    gp.top_edge_0 = gp.yc - gp.ys / 2.0;
    if (gp.ys < 1.0 / h) {
        gp.ys_inv = 0;
        gp.ys = 0;
    }
}

// what a ramp pixel hands to the sleef call, for the fixture (tests/golden/make_golden_creative.py records them through these hooks)
struct Trace { float *sin_args, *cos_args; long long nsin, ncos, cap; };
thread_local Trace *g_trace = nullptr;
inline float t_sin(float v) { if (g_trace && g_trace->nsin < g_trace->cap) g_trace->sin_args[g_trace->nsin++] = v; return xsinf(v); }
inline float t_cos(float v) { if (g_trace && g_trace->ncos < g_trace->cap) g_trace->cos_args[g_trace->ncos++] = v; return xcosf(v); }

float calcGradientFactor(const struct grad_params &gp, int x, int y, cr_cg_counts *cn)
{
    if (gp.transpose) ++cn->g_transposed;
    if (gp.angle_is_zero) {
        ++cn->g_angle_zero;
        int gy = gp.transpose ? x : y;
        if (gy < gp.top_edge_0) {
            ++cn->g_top;
            return gp.topmul;
        } else if (gy >= gp.top_edge_0 + gp.ys) {
            ++cn->g_bottom;
            return gp.botmul;
        } else {
            float val = ((float)(gy - gp.top_edge_0) * gp.ys_inv);
            if (gp.bright_top) { val = 1.f - val; }
            val *= RT_PI_F_2;
            if (gp.scale < 1.f) { ++cn->g_ramp_sin; val = pow3(t_sin(val)); }
            else { ++cn->g_ramp_cos; val = 1.f - pow3(t_cos(val)); }
            return gp.scale + val * (1.0 - gp.scale);
        }
    } else {
        ++cn->g_angled;
        int gy = gp.transpose ? x : y;
        int gx = gp.transpose ? gp.h - y - 1 : x;
        float top_edge = gp.top_edge_0 - gp.ta * (gx - gp.xc);
        if (gy < top_edge) {
            ++cn->g_top;
            return gp.topmul;
        } else if (gy >= top_edge + gp.ys) {
            ++cn->g_bottom;
            return gp.botmul;
        } else {
            float val = ((float)(gy - top_edge) * gp.ys_inv);
            val = gp.bright_top ? 1.f - val : val;
            val *= RT_PI_F_2;
            if (gp.scale < 1.f) { ++cn->g_ramp_sin; val = pow3(t_sin(val)); }
            else { ++cn->g_ramp_cos; val = 1.f - pow3(t_cos(val)); }
            return gp.scale + val * (1.0 - gp.scale);
        }
    }
}

struct pcv_params {
    float oe_a, oe_b, oe1_a, oe1_b, oe2_a, oe2_b;
    float ie_mul, ie1_mul, ie2_mul;
    float sepmix, feather;
    int x1, x2, y1, y2;
    int ex, ey, ew, eh;
    int sep;
    bool is_super_ellipse_mode, is_portrait;
    float scale;
    float fadeout_mul;
};

void calcPCVignetteParams(int fW, int fH, int oW, int oH, const PCVignetteParams &pcvignette, const CropParams &crop, pcv_params &pcv)
{
    double roundness = pcvignette.roundness / 100.0;
    pcv.feather = pcvignette.feather / 100.0;
    if (crop.enabled) {
        float sW = float(oW) / fW;
        float sH = float(oH) / fH;
        pcv.ew = crop.w * sW;
        pcv.eh = crop.h * sH;
        pcv.x1 = crop.x * sW;
        pcv.y1 = crop.y * sH;
    } else {
        pcv.ew = oW;
        pcv.eh = oH;
        pcv.x1 = 0;
        pcv.y1 = 0;
    }
    float dW = pcvignette.centerX / 200.f * pcv.ew;
    float dH = pcvignette.centerY / 200.f * pcv.eh;
    pcv.ex = pcv.x1 + dW;
    pcv.ey = pcv.y1 + dH;
    pcv.x2 = pcv.x1 + pcv.ew + std::abs(dW);
    pcv.y2 = pcv.y1 + pcv.eh + std::abs(dH);
    pcv.fadeout_mul = 1.0 / (0.05 * sqrtf(oW * oW + oH * oH));
    float short_side = (pcv.ew < pcv.eh) ? pcv.ew : pcv.eh;
    float long_side = (pcv.ew > pcv.eh) ? pcv.ew : pcv.eh;
    pcv.sep = 2;
    pcv.sepmix = 0;
    pcv.oe_a = sqrt(2.0) * long_side * 0.5;
    pcv.oe_b = pcv.oe_a * short_side / long_side;
    pcv.ie_mul = (1.0 / sqrt(2.0)) * (1.0 - pcv.feather);
    pcv.is_super_ellipse_mode = false;
    pcv.is_portrait = (pcv.ew < pcv.eh);
    pcv.oe1_a = pcv.oe1_b = pcv.oe2_a = pcv.oe2_b = pcv.ie1_mul = pcv.ie2_mul = 0.f;       // (left unset by the reference when roundness >= 0.5, and unread then)
    if (roundness < 0.5) {
        pcv.is_super_ellipse_mode = true;
        float sepf = 2 + 4 * powf(1.0 - 2 * roundness, 1.3);
        pcv.sep = ((int)sepf) & ~0x1;
        pcv.sepmix = (sepf - pcv.sep) * 0.5;
        pcv.oe1_a = powf(2.0, 1.0 / pcv.sep) * long_side * 0.5;
        pcv.oe1_b = pcv.oe1_a * short_side / long_side;
        pcv.ie1_mul = (1.0 / powf(2.0, 1.0 / pcv.sep)) * (1.0 - pcv.feather);
        pcv.oe2_a = powf(2.0, 1.0 / (pcv.sep + 2)) * long_side * 0.5;
        pcv.oe2_b = pcv.oe2_a * short_side / long_side;
        pcv.ie2_mul = (1.0 / powf(2.0, 1.0 / (pcv.sep + 2))) * (1.0 - pcv.feather);
    }
    if (roundness > 0.5) {
        float rad = sqrtf(pcv.ew * pcv.ew + pcv.eh * pcv.eh) / 2.0;
        float diff_a = rad - pcv.oe_a;
        float diff_b = rad - pcv.oe_b;
        pcv.oe_a = pcv.oe_a + diff_a * 2 * (roundness - 0.5);
        pcv.oe_b = pcv.oe_b + diff_b * 2 * (roundness - 0.5);
    }
    pcv.scale = powf(2, -pcvignette.strength);
    if (pcvignette.strength >= 6.0) { pcv.scale = 0.0; }
}

inline void count_normn(cr_cg_counts *cn, int n) { if (n >= 2 && n <= 8 && !(n & 1)) ++cn->v_normn[n / 2 - 1]; }

float calcPCVignetteFactor(const pcv_params &pcv, int x, int y, cr_cg_counts *cn)
{
    float fo = 1.f;
    if (x < pcv.x1 || x > pcv.x2 || y < pcv.y1 || y > pcv.y2) {
        int dist_x = (x < pcv.x1) ? pcv.x1 - x : x - pcv.x2;
        int dist_y = (y < pcv.y1) ? pcv.y1 - y : y - pcv.y2;
        if (dist_x < 0) { dist_x = 0; }
        if (dist_y < 0) { dist_y = 0; }
        fo = sqrtf(dist_x * dist_x + dist_y * dist_y) * pcv.fadeout_mul;
        if (fo >= 1.f) {
            ++cn->v_fade_out;
            return 1.f;
        }
        ++cn->v_faded;
    }
    float a = fabs((x - pcv.ex) - pcv.ew * 0.5f);
    float b = fabs((y - pcv.ey) - pcv.eh * 0.5f);
    if (pcv.is_portrait) { ++cn->v_portrait; std::swap(a, b); }
    float dist = normn(a, b, 2);
    float dist_oe, dist_ie;
    struct { float x, y; } sincosval;
    if (dist == 0.0f) {
        ++cn->v_dist_zero;
        sincosval.y = 1.0f;
        sincosval.x = 0.0f;
    } else {
        sincosval.y = a / dist;
        sincosval.x = b / dist;
    }
    if (pcv.is_super_ellipse_mode) {
        count_normn(cn, pcv.sep); count_normn(cn, pcv.sep + 2);
        float dist_oe1 = pcv.oe1_a * pcv.oe1_b / normn(pcv.oe1_b * sincosval.y, pcv.oe1_a * sincosval.x, pcv.sep);
        float dist_oe2 = pcv.oe2_a * pcv.oe2_b / normn(pcv.oe2_b * sincosval.y, pcv.oe2_a * sincosval.x, pcv.sep + 2);
        float dist_ie1 = pcv.ie1_mul * dist_oe1;
        float dist_ie2 = pcv.ie2_mul * dist_oe2;
        dist_oe = dist_oe1 * (1.f - pcv.sepmix) + dist_oe2 * pcv.sepmix;
        dist_ie = dist_ie1 * (1.f - pcv.sepmix) + dist_ie2 * pcv.sepmix;
    } else {
        dist_oe = pcv.oe_a * pcv.oe_b / sqrtf(SQR(pcv.oe_b * sincosval.y) + SQR(pcv.oe_a * sincosval.x));
        dist_ie = pcv.ie_mul * dist_oe;
    }
    if (dist <= dist_ie) {
        ++cn->v_inside;
        return 1.f;
    }
    float val;
    if (dist >= dist_oe) {
        ++cn->v_outside;
        val = pcv.scale;
    } else {
        val = RT_PI_F_2 * (dist - dist_ie) / (dist_oe - dist_ie);
        if (pcv.scale < 1.f) { ++cn->v_ramp_cos; val = pow4(t_cos(val)); }
        else { ++cn->v_ramp_sin; val = 1 - pow4(t_sin(val)); }
        val = pcv.scale + val * (1.f - pcv.scale);
    }
    if (fo < 1.f) { val = fo + val * (1.f - fo); }
    return val;
}

struct Derived { bool applyGradient, applyPCVignetting; int cx, cy; grad_params gp; pcv_params pcv; };

// needsGradient / needsPCVignetting (L1354-1362), creativeGradients (L1390-1405), the head of transformLuminanceOnly (L991-1011) on a w x h image
Derived derive(const cr_cg_params *p, int w, int h)
{
    Derived d = {};
    const GradientParams gradient = {p->gradient_enabled != 0, p->gradient_degree, p->gradient_feather, p->gradient_strength, p->gradient_center_x, p->gradient_center_y};
    const PCVignetteParams pcvignette = {p->pcvignette_enabled != 0, p->pcvignette_strength, p->pcvignette_feather, p->pcvignette_roundness, p->pcvignette_center_x, p->pcvignette_center_y};
    const CropParams crop = {p->crop_enabled != 0, p->crop_x, p->crop_y, p->crop_w, p->crop_h};
    d.applyGradient = gradient.enabled && fabs(gradient.strength) > 1e-15;
    d.applyPCVignetting = pcvignette.enabled && fabs(pcvignette.strength) > 1e-15;
    d.cx = p->offset_x;
    d.cy = p->offset_y;
    int cw, ch;
    if (p->full_width < 0) { cw = w; ch = h; }
    else { cw = p->full_width; ch = p->full_height; }
    int fw = cw * p->scale;
    int fh = ch * p->scale;
    if (d.applyGradient) { calcGradientParams(cw, ch, gradient, d.gp); }
    if (d.applyPCVignetting) { calcPCVignetteParams(fw, fh, cw, ch, pcvignette, crop, d.pcv); }
    return d;
}

} // namespace

extern "C" {

void cr_xsinf(const float *x, float *y, size_t n) { for (size_t i = 0; i < n; ++i) y[i] = xsinf(x[i]); }
void cr_xcosf(const float *x, float *y, size_t n) { for (size_t i = 0; i < n; ++i) y[i] = xcosf(x[i]); }
void cr_xcbrtf(const float *x, float *y, size_t n) { for (size_t i = 0; i < n; ++i) y[i] = oracle_xcbrtf(x[i]); }
void cr_pow_F(const float *a, const float *b, float *y, size_t n) { for (size_t i = 0; i < n; ++i) y[i] = oracle_pow_F(a[i], b[i]); }

void cr_cg_derive(const cr_cg_params *p, int w, int h, cr_cg_derived *o)
{
    std::memset(o, 0, sizeof *o);
    const Derived d = derive(p, w, h);
    o->apply_gradient = d.applyGradient; o->apply_pcvignette = d.applyPCVignetting; o->cx = d.cx; o->cy = d.cy;
    if (d.applyGradient) {
        const grad_params &g = d.gp;
        o->angle_is_zero = g.angle_is_zero; o->transpose = g.transpose; o->bright_top = g.bright_top; o->h = g.h;
        o->ta = g.ta; o->yc = g.yc; o->xc = g.xc; o->ys = g.ys; o->ys_inv = g.ys_inv; o->scale = g.scale; o->botmul = g.botmul; o->topmul = g.topmul;
        o->top_edge_0 = g.top_edge_0;
    }
    if (d.applyPCVignetting) {
        const pcv_params &v = d.pcv;
        o->oe_a = v.oe_a; o->oe_b = v.oe_b; o->oe1_a = v.oe1_a; o->oe1_b = v.oe1_b; o->oe2_a = v.oe2_a; o->oe2_b = v.oe2_b;
        o->ie_mul = v.ie_mul; o->ie1_mul = v.ie1_mul; o->ie2_mul = v.ie2_mul; o->sepmix = v.sepmix; o->feather = v.feather;
        o->x1 = v.x1; o->x2 = v.x2; o->y1 = v.y1; o->y2 = v.y2; o->ex = v.ex; o->ey = v.ey; o->ew = v.ew; o->eh = v.eh; o->sep = v.sep;
        o->is_super_ellipse_mode = v.is_super_ellipse_mode; o->is_portrait = v.is_portrait; o->pcv_scale = v.scale; o->fadeout_mul = v.fadeout_mul;
    }
}

// The creative branch of transformLuminanceOnly on three h x w planes (rows of `stride` floats), in place.  gfac / vfac (or null): the two
// factor planes as the functions return them, w floats per row (1.f where a tool does not run).  sin_args / cos_args (or null, room for `cap`
// each): the arguments the ramp branches hand to xsinf / xcosf, in raster order; *nsin / *ncos: how many.  Returns 0 when nothing runs
int cr_creative_gradients(float *r, float *g, float *b, size_t stride, int w, int h, const cr_cg_params *p, float *gfac, float *vfac,
                          float *sin_args, float *cos_args, long long cap, long long *nsin, long long *ncos, cr_cg_counts *cn)
{
    std::memset(cn, 0, sizeof *cn);
    const Derived d = derive(p, w, h);
    if (nsin) { *nsin = 0; *ncos = 0; }
    if (!(d.applyGradient || d.applyPCVignetting)) return 0;
    Trace tr = {sin_args, cos_args, 0, 0, sin_args ? cap : 0};
    g_trace = sin_args ? &tr : nullptr;
    for (int y = 0; y < h; y++) {
        for (int x = 0; x < w; x++) {
            double factor = 1.0;
            float gf = 1.f, vf = 1.f;
            if (d.applyGradient) { gf = calcGradientFactor(d.gp, d.cx + x, d.cy + y, cn); factor *= gf; }
            if (d.applyPCVignetting) { vf = calcPCVignetteFactor(d.pcv, d.cx + x, d.cy + y, cn); factor *= vf; }
            if (gfac) gfac[(size_t)y * w + x] = gf;
            if (vfac) vfac[(size_t)y * w + x] = vf;
            const size_t o = (size_t)y * stride + x;
            if (r) {
                r[o] = r[o] * factor;
                g[o] = g[o] * factor;
                b[o] = b[o] * factor;
            }
        }
    }
    g_trace = nullptr;
    if (nsin) { *nsin = tr.nsin; *ncos = tr.ncos; }
    return 1;
}

} // extern "C"
