// tests/emul/colorcorrection_ref.cc -- CPU checker for artgpu_color_correction: the host derivation and the row loop of
// ImProcFunctions::colorCorrection (rtengine/ipcolorcorrection.cc:88-141, 280-414, 416-554, 610-767, 770-863) restated serially on
// contiguous float planes: per row and region the groups of four columns below 4 * (W / 4) with the group activation of L818-830 and the
// 4-wide CDL_v, then the remaining columns with the scalar CDL.  Test infrastructure only; built on first use with -ffp-contract=off.
//
// The sleef forms (scalar and 4-lane), the PQ tables and Imagefloat::setMode(YUV / RGB) are liboracle's restatements (oracle_xlogf_s / _v,
// oracle_xexpf_s / _v, oracle_pow_F, oracle_xlog2lin, oracle_xatan2f, oracle_xsincosf, oracle_pq_luts, oracle_rgb_to_yuv / oracle_yuv_to_rgb).
// What liboracle keeps static is restated here: Color::rgb2jzazbz / jzazbz2rgb (color.cc:37-86, 6706-6742), LUTf::operator[](float), and the
// double-precision Color::rgb2hsl / hsl2rgb / hue2rgb (color.cc:385-429, 456-473, 511-534).
// The reference file needs glibmm and lcms2 and is not compiled anywhere: the loop body is parity-unpinned, its leaves are pinned.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

extern "C" {
float oracle_xatan2f(float y, float x);
void oracle_xsincosf(float d, float *sn, float *cs);
void oracle_pq_luts(float *pq65536, float *pq_inv65536);
void oracle_rgb_to_yuv(float *const img[3], size_t s, int w, int h, const float ws[9]);
void oracle_yuv_to_rgb(float *const img[3], size_t s, int w, int h, const float ws[9]);
float oracle_xexpf_s(float d);
float oracle_xexpf_v(float d);
float oracle_xlogf_s(float d);
float oracle_xlogf_v(float d);
float oracle_pow_F(float a, float b);
float oracle_xlog2lin(float x, float base);
}

extern "C" {
struct cc_ref_region {            // the layout of artgpu_color_correction_region with contiguous W * H planes (or NULL) for the masks
    int32_t mode, rgbluminance;
    double a, b, in_saturation, out_saturation, hueshift, hsl_gamma;
    double slope[3], offset[3], power[3], pivot[3], compression[3];
    double hue[3], sat[3], factor[3];
    const float *lmask, *abmask;
};
struct cc_ref_info {              // the layout of artgpu_color_correction_info
    float abca, abcb;
    int32_t enabled, rgbmode;
    float slope[3], offset[3], power[3], pivot[3];
    float compression[3][2];
    float rhs;
    int64_t oor_pixels;
};
struct cc_ref_counts {
    long long groups_zero_lane, tail_skipped;
    long long px_yuv, px_jzazbz, px_rgb, px_rgbluminance, px_hsl;
    long long hue_hsl, hue_yuv, hue_jzazbz;
    long long pivot, compression_vector_clamp, compression_scalar_zero, compression_taken, gamma, rgbluminance;
    long long y_nonpositive, v_nonpositive, pq_low, pq_high;
};
}

namespace {

const float PI_F = 3.14159265358979323846;        // RT_PI_F
const float PI_F_180 = 0.017453292519943295769;   // RT_PI_F_180
enum { MODE_YUV = 0, MODE_RGB = 1, MODE_HSL = 2, MODE_JZAZBZ = 3, MODE_LUT = 4 };

template <typename T> inline T rt_min(T a, T b) { return b < a ? b : a; }     // rt_math.h:54-58
template <typename T> inline T rt_max(T a, T b) { return a < b ? b : a; }     // rt_math.h:72-76
inline float vmaxf(float x, float y) { return x > y ? x : y; }                // _mm_max_ps
inline float mix(float a, float b, float c) { return a * b + (1.f - a) * c; } // intp and vintpf: the same expression

struct Tables { std::vector<float> pq, pqi; Tables() : pq(65536), pqi(65536) { oracle_pq_luts(pq.data(), pqi.data()); } };
const Tables &tables() { static Tables t; return t; }

// LUTf::operator[](float) with flags 0 (LUT.h:436-459)
float lut_at(const std::vector<float> &d, float index)
{
    const int maxs = (int)d.size() - 2;
    int idx = (int)index;
    if (index < 0.f) return d[0];
    if (index > (float)maxs) idx = maxs;
    const float diff = index - (float)idx;
    const float p1 = d[idx], p2 = d[idx + 1] - p1;
    return p1 + p2 * diff;
}
float PQ(float X)
{
    X = std::max(X, 1e-10f);
    const float XX = std::pow(X * 1e-4f, 0.1593017578125f);
    return std::pow((0.8359375f + 18.8515625f * XX) / (1 + 18.6875f * XX), 134.034375f);
}
float PQ_inv(float X)
{
    X = std::max(X, 1e-10f);
    const float XX = std::pow(X, 7.460772656268214e-03f);
    return 1e4f * std::pow((0.8359375f - XX) / (18.6875f * XX - 18.8515625f), 6.277394636015326f);
}

struct Ctx {
    float ws[3][3], iws[3][3];
    cc_ref_counts *cn;
    bool oor;                     // the pixel in flight called PQ / PQ_inv with an argument above 1
};
void note_range(Ctx &c, float x)
{
    if (x < 0.f) ++c.cn->pq_low;
    else if (x > 1.f) { ++c.cn->pq_high; c.oor = true; }
}
float get_PQ(Ctx &c, float x)
{
    if (x >= 0.f && x <= 1.f) return lut_at(tables().pq, x * 65535.f);
    note_range(c, x);
    return PQ(x);
}
float get_PQ_inv(Ctx &c, float x)
{
    if (x >= 0.f && x <= 1.f) return lut_at(tables().pqi, x * 65535.f);
    note_range(c, x);
    return PQ_inv(x);
}
void mat3(const float M[3][3], float &X, float &Y, float &Z)          // dot_product(M, Vec3): sums from 0
{
    const float in[3] = {X, Y, Z};
    float out[3];
    for (int i = 0; i < 3; ++i) {
        out[i] = 0;
        for (int k = 0; k < 3; ++k) out[i] += M[i][k] * in[k];
    }
    X = out[0]; Y = out[1]; Z = out[2];
}
void rgb2jzazbz(Ctx &c, float R, float G, float B, float &Jz, float &az, float &bz)
{
    static const float D65[3][3] = {{0.9555766f, -0.0230393f, 0.0631636f}, {-0.0282895f, 1.0099416f, 0.0210077f}, {0.0122982f, -0.0204830f, 1.3299098f}};
    float X = c.ws[0][0] * R + c.ws[0][1] * G + c.ws[0][2] * B;
    float Y = c.ws[1][0] * R + c.ws[1][1] * G + c.ws[1][2] * B;
    float Z = c.ws[2][0] * R + c.ws[2][1] * G + c.ws[2][2] * B;
    mat3(D65, X, Y, Z);
    const float Lp = get_PQ(c, 0.674207838f * X + 0.382799340f * Y - 0.047570458f * Z);
    const float Mp = get_PQ(c, 0.149284160f * X + 0.739628340f * Y + 0.083327300f * Z);
    const float Sp = get_PQ(c, 0.070941080f * X + 0.174768000f * Y + 0.670970020f * Z);
    const float Iz = 0.5f * (Lp + Mp);
    az = 3.524000f * Lp - 4.066708f * Mp + 0.542708f * Sp;
    bz = 0.199076f * Lp + 1.096799f * Mp - 1.295875f * Sp;
    Jz = (0.44f * Iz) / (1.f - 0.56f * Iz) - 1.6295499532821566e-11f;
}
void jzazbz2rgb(Ctx &c, float Jz, float az, float bz, float &R, float &G, float &B)
{
    static const float D50[3][3] = {{1.0478112f, 0.0228866f, -0.0501270f}, {0.0295424f, 0.9904844f, -0.0170491f}, {-0.0092345f, 0.0150436f, 0.7521316f}};
    Jz = Jz + 1.6295499532821566e-11f;
    const float Iz = Jz / (0.44f + 0.56f * Jz);
    const float L = get_PQ_inv(c, Iz + 1.386050432715393e-1f * az + 5.804731615611869e-2f * bz);
    const float M = get_PQ_inv(c, Iz - 1.386050432715393e-1f * az - 5.804731615611891e-2f * bz);
    const float S = get_PQ_inv(c, Iz - 9.601924202631895e-2f * az - 8.118918960560390e-1f * bz);
    float X = +1.661373055774069e+00f * L - 9.145230923250668e-01f * M + 2.313620767186147e-01f * S;
    float Y = -3.250758740427037e-01f * L + 1.571847038366936e+00f * M - 2.182538318672940e-01f * S;
    float Z = -9.098281098284756e-02f * L - 3.127282905230740e-01f * M + 1.522766561305260e+00f * S;
    mat3(D50, X, Y, Z);
    R = c.iws[0][0] * X + c.iws[0][1] * Y + c.iws[0][2] * Z;
    G = c.iws[1][0] * X + c.iws[1][1] * Y + c.iws[1][2] * Z;
    B = c.iws[2][0] * X + c.iws[2][1] * Y + c.iws[2][2] * Z;
}

// Color::rgb2hsl / hue2rgb / hsl2rgb, scalar overloads
void rgb2hsl(float r, float g, float b, float &h, float &s, float &l)
{
    const double R = double(r) / 65535.0, G = double(g) / 65535.0, B = double(b) / 65535.0;
    const double m = rt_min(rt_min(R, G), B), M = rt_max(rt_max(R, G), B);
    const double C = M - m;
    const double l_ = (M + m) / 2.;
    l = float(l_);
    if (C < 0.00001 && C > -0.00001) { h = 0.f; s = 0.f; return; }
    s = l_ <= 0.5 ? float((M - m) / (M + m)) : float((M - m) / (2.0 - M - m));
    double h_;
    if (R == M) h_ = (G - B) / C;
    else if (G == M) h_ = 2. + (B - R) / C;
    else h_ = 4. + (R - G) / C;
    h = float(h_ / 6.0);
    if (h < 0.f) h += 1.f;
    if (h > 1.f) h -= 1.f;
}
double hue2rgb(double p, double q, double t)
{
    if (t < 0.) t += 6.;
    else if (t > 6.) t -= 6.;
    if (t < 1.) return p + (q - p) * t;
    if (t < 3.) return q;
    if (t < 4.) return p + (q - p) * (4. - t);
    return p;
}
void hsl2rgb(float h, float s, float l, float &r, float &g, float &b)
{
    if (s == 0) { r = g = b = 65535.0f * l; return; }
    const double h_ = h, s_ = s, l_ = l;
    const double m2 = l <= 0.5f ? l_ * (1.0 + s_) : l_ + s_ - l_ * s_;
    const double m1 = 2.0 * l_ - m2;
    r = float(65535.0 * hue2rgb(m1, m2, h_ * 6.0 + 2.0));
    g = float(65535.0 * hue2rgb(m1, m2, h_ * 6.0));
    b = float(65535.0 * hue2rgb(m1, m2, h_ * 6.0 - 2.0));
}
inline float lum(const Ctx &c, float r, float g, float b) { return r * c.ws[1][0] + g * c.ws[1][1] + b * c.ws[1][2]; }
inline void rgb2yuv(const Ctx &c, float r, float g, float b, float &Y, float &u, float &v) { Y = lum(c, r, g, b); u = Y - b; v = r - Y; }
inline void yuv2rgb(const Ctx &c, float Y, float u, float v, float &r, float &g, float &b)
{
    b = Y - u;
    r = v + Y;
    g = (Y - r * c.ws[1][0] - b * c.ws[1][2]) / c.ws[1][1];
}
inline void uv2hs(float u, float v, float &h, float &s) { s = std::sqrt(u * u + v * v); h = oracle_xatan2f(u, v); }      // Color::yuv2hsl
inline void hs2uv_polar(float h, float s, float &u, float &v) { float sn, cs; oracle_xsincosf(h, &sn, &cs); u = s * sn; v = s * cs; }   // Color::hsl2yuv

// the lambdas of L143-180
void yuv_to_jz(Ctx &c, float &Y, float &u, float &v)
{
    float R, G, B;
    yuv2rgb(c, Y, u, v, R, G, B);
    rgb2jzazbz(c, R / 65535.f, G / 65535.f, B / 65535.f, Y, v, u);
}
void jz_to_yuv(Ctx &c, float &Jz, float &bz, float &az)
{
    float R, G, B;
    jzazbz2rgb(c, Jz, az, bz, R, G, B);
    rgb2yuv(c, R * 65535.f, G * 65535.f, B * 65535.f, Jz, bz, az);
}
void yuv_to_hsl(Ctx &c, float Y, float u, float v, float &h, float &s, float &l)
{
    float R, G, B;
    yuv2rgb(c, Y, u, v, R, G, B);
    rgb2hsl(R, G, B, h, s, l);
    h *= 2.f * PI_F;
}
void hsl_to_yuv(Ctx &c, float h, float s, float l, float &Y, float &u, float &v)
{
    h /= (2.f * PI_F);
    if (h < 0.f) h += 1.f;
    else if (h > 1.f) h -= 1.f;
    float R, G, B;
    hsl2rgb(h, s, l, R, G, B);
    rgb2yuv(c, R, G, B, Y, u, v);
}

// the per-region scalars of L240-255
struct Derived {
    float abca, abcb, rs, rsout, slope[3], offset[3], power[3], pivot[3], comp[3][2], rhs, hslgamma;
    int rgbmode;
    bool enabled, jzazbz, hsl;
};
void hs2uv(const Ctx &c, float h, float s, float &u, float &v)        // L110-128
{
    if (h < 0.f) h += 1.f;
    else if (h > 1.f) h -= 1.f;
    float R, G, B;
    hsl2rgb(h, s, 0.5f, R, G, B);
    R /= 65535.f; G /= 65535.f; B /= 65535.f;
    float Y;
    rgb2yuv(c, R, G, B, Y, u, v);
    float s2;
    uv2hs(u, v, h, s2);
    hs2uv_polar(h, s, u, v);
}
inline float sgn(float a) { return float((0.f < a) - (a < 0.f)); }
inline float abcoord(float x) { return sgn(x) * oracle_xlog2lin(std::abs(x), 4.f); }
void derive(const Ctx &c, const cc_ref_region &r, Derived &d)
{
    d.abca = d.abcb = 0.f; d.rs = d.rsout = 1.f; d.enabled = d.jzazbz = d.hsl = false; d.rhs = 0.f; d.hslgamma = 1.f;
    for (int j = 0; j < 3; ++j) { d.slope[j] = 1.f; d.offset[j] = 0.f; d.power[j] = 1.f; d.pivot[j] = 1.f; d.comp[j][0] = d.comp[j][1] = 0.f; }
    d.rgbmode = int(r.mode != MODE_YUV && r.mode != MODE_JZAZBZ);
    if (d.rgbmode) {
        if (r.rgbluminance) d.rgbmode = 2;
        d.hsl = r.mode == MODE_HSL;
    } else {
        d.jzazbz = r.mode == MODE_JZAZBZ;
        float x = abcoord(float(r.a)), y = abcoord(float(r.b));
        const float h = std::atan2(y, x) / (2.f * PI_F);              // the float overload
        const float s = std::sqrt(x * x + y * y);
        float u, v;
        hs2uv(c, h, s, u, v);
        d.abca = v;
        d.abcb = u;
    }
    d.rs = 1.f + r.in_saturation / 100.f;
    d.rsout = 1.f + r.out_saturation / 100.f;
    if (r.mode == MODE_HSL) {
        for (int ch = 0; ch < 3; ++ch) {
            const float hue = (float(r.hue[ch]) / 180.f) * PI_F;
            const float sat = std::pow(float(r.sat[ch]) / 100.f, 2.5f);
            const float f = (r.factor[ch] / 100.f) + 1.f;
            float u, v, R, G, B;
            hs2uv(c, hue / (2 * PI_F), sat, u, v);
            yuv2rgb(c, 0.5f, u, v, R, G, B);
            R *= 2.f; G *= 2.f; B *= 2.f;
            const float rgb[3] = {R, G, B};
            for (int k = 0; k < 3; ++k) {
                if (ch == 0) d.slope[k] = rgb[k] * f;
                else if (ch == 1) d.offset[k] = rgb[k] + f - 2.f;
                else d.power[k] = (2.f - rgb[k]) * (2.f - f);
            }
            d.pivot[ch] = 1.f;
        }
        for (int k = 0; k < 3; ++k) d.enabled = d.enabled || d.slope[k] != 1.f || d.offset[k] != 0.f || d.power[k] != 1.f;
        d.hslgamma = r.hsl_gamma;
    } else {
        for (int k = 0; k < 3; ++k) {
            const int j = d.rgbmode ? k : 0;
            d.slope[k] = r.slope[j];
            d.offset[k] = r.offset[j];
            d.power[k] = 1.0 / r.power[j];
            d.pivot[k] = r.pivot[j];
            const double compr = r.compression[j] * 100.0;
            if (compr > 0) {
                d.comp[k][0] = compr;
                const double y0 = std::pow((d.slope[k] + d.offset[k]) / d.pivot[k], d.power[k]) * d.pivot[k];     // float operands: the float overload
                d.comp[k][1] = std::log(1.0 + y0 * compr) / d.slope[k];
            }
            d.enabled = d.enabled || d.slope[k] != 1.f || d.offset[k] != 0.f || d.power[k] != 1.f || d.comp[k][1] != 0.f;
        }
    }
    d.rhs = r.mode != MODE_RGB ? float(r.hueshift * PI_F_180) : 0.f;
}
bool finite_all(const Derived &d)
{
    bool ok = std::isfinite(d.abca) && std::isfinite(d.abcb) && std::isfinite(d.rs) && std::isfinite(d.rsout) && std::isfinite(d.rhs) &&
              std::isfinite(d.hslgamma) && std::isfinite(1.f / d.hslgamma);
    for (int k = 0; k < 3; ++k)
        ok = ok && std::isfinite(d.slope[k]) && std::isfinite(d.offset[k]) && std::isfinite(d.power[k]) && std::isfinite(d.pivot[k]) &&
             std::isfinite(d.comp[k][0]) && std::isfinite(d.comp[k][1]);
    return ok;
}

struct Tool {
    Ctx c;
    float fR, fG, fB;
    cc_ref_counts *cn;

    // the hue shift of one pixel (the 4-wide form loops over its lanes with exactly this, L622-649)
    void hue_shift(const Derived &d, float &Y, float &u, float &v)
    {
        float h, s;
        if (d.hsl) {
            float l;
            yuv_to_hsl(c, Y, u, v, h, s, l);
            h += d.rhs;
            hsl_to_yuv(c, h, s, l, Y, u, v);
            ++cn->hue_hsl;
        } else {
            if (d.jzazbz) yuv_to_jz(c, Y, u, v);
            uv2hs(u, v, h, s);
            h += d.rhs;
            hs2uv_polar(h, s, u, v);
            if (d.jzazbz) jz_to_yuv(c, Y, u, v);
            ++(d.jzazbz ? cn->hue_jzazbz : cn->hue_yuv);
        }
    }
    void count_mode(const Derived &d)
    {
        if (d.hsl) ++cn->px_hsl;
        else if (d.rgbmode == 2) ++cn->px_rgbluminance;
        else if (d.rgbmode) ++cn->px_rgb;
        else if (d.jzazbz) ++cn->px_jzazbz;
        else ++cn->px_yuv;
    }

    // CDL (L416-554)
    void cdl(const Derived &d, float &Y, float &u, float &v)
    {
        count_mode(d);
        if (d.rhs != 0.f) hue_shift(d, Y, u, v);
        if (d.rgbmode) {
            if (d.rs != 1.f) { u *= d.rs; v *= d.rs; }
            if (d.enabled) {
                float rgb[3];
                yuv2rgb(c, Y, u, v, rgb[0], rgb[1], rgb[2]);
                const bool use_gamma = d.hsl && d.hslgamma != 1.f;
                for (int i = 0; i < 3; ++i) {
                    float t = rgb[i] / 65535.f;
                    if (use_gamma && t > 0.f) { t = oracle_pow_F(t, 1.f / d.hslgamma); ++cn->gamma; }
                    t = t * d.slope[i] + d.offset[i] / 2.f;
                    if (t > 0.f) {
                        if (d.pivot[i] != 1.f) { t = oracle_pow_F(t / d.pivot[i], d.power[i]) * d.pivot[i]; ++cn->pivot; }
                        else t = oracle_pow_F(t, d.power[i]);
                        if (d.comp[i][0] != 0.f) { t = oracle_xlogf_s(t * d.comp[i][0] + 1.f) / d.comp[i][1]; ++cn->compression_taken; }
                    } else {
                        ++cn->v_nonpositive;
                        if (d.comp[i][0] != 0.f) ++cn->compression_scalar_zero;
                        t = 0.f;
                    }
                    if (use_gamma && t > 0.f) t = oracle_pow_F(t, d.hslgamma);
                    rgb[i] = t * 65535.f;
                }
                if (d.rgbmode != 2) {
                    rgb2yuv(c, rgb[0], rgb[1], rgb[2], Y, u, v);
                } else {
                    ++cn->rgbluminance;
                    float rr, gg, bb;
                    yuv2rgb(c, Y, u, v, rr, gg, bb);
                    const float Y1 = lum(c, rr + (rgb[0] - rr) * fR, gg + (rgb[1] - gg) * fG, bb + (rgb[2] - bb) * fB);
                    if (Y > 0.f) {
                        const float f = Y1 / Y;
                        u *= f;
                        v *= f;
                    } else {
                        ++cn->y_nonpositive;
                    }
                    Y = Y1;
                }
            }
            const float f = rt_max(Y, 0.f);
            u += f * d.abcb;
            v += f * d.abca;
            if (d.rsout != 1.f) { u *= d.rsout; v *= d.rsout; }
        } else {
            if (d.enabled) {
                float YY = (Y / 65535.f) * d.slope[0] + d.offset[0] / 2.f;
                if (YY > 0.f) {
                    if (d.pivot[0] != 1.f) { YY = oracle_pow_F(YY / d.pivot[0], d.power[0]) * d.pivot[0]; ++cn->pivot; }
                    else YY = oracle_pow_F(YY, d.power[0]);
                    if (d.comp[0][0] != 0.f) { YY = oracle_xlogf_s(YY * d.comp[0][0] + 1.f) / d.comp[0][1]; ++cn->compression_taken; }
                    YY *= 65535.f;
                } else {
                    ++cn->v_nonpositive;
                    if (d.comp[0][0] != 0.f) ++cn->compression_scalar_zero;
                    YY = 0.f;
                }
                if (Y > 0.f) {
                    const float f = YY / Y;
                    Y = YY;
                    u *= f;
                    v *= f;
                } else {
                    ++cn->y_nonpositive;
                    Y = YY;
                }
            }
            if (d.jzazbz) yuv_to_jz(c, Y, u, v);
            if (d.rs != 1.f) { u *= d.rs; v *= d.rs; }
            const float f = rt_max(Y, 0.f);
            u += f * d.abcb;
            v += f * d.abca;
            if (d.rsout != 1.f) { u *= d.rsout; v *= d.rsout; }
            if (d.jzazbz) jz_to_yuv(c, Y, u, v);
        }
    }

    static float vpow(float a, float b) { return oracle_xexpf_v(b * oracle_xlogf_v(a)); }      // pow_F on vfloat, one lane
    // slope .. compression of one channel on four lanes (L665-685 / L721-736)
    void chain4(const Derived &d, int i, float t[4])
    {
        for (int k = 0; k < 4; ++k) {
            t[k] = t[k] * d.slope[i] + d.offset[i] / 2.f;
            if (!(t[k] > 0.f)) ++cn->v_nonpositive;
        }
        for (int k = 0; k < 4; ++k) {
            if (d.pivot[i] != 1.f) { if (t[k] > 0.f) ++cn->pivot; t[k] = t[k] > 0.f ? vpow(t[k] / d.pivot[i], d.power[i]) * d.pivot[i] : 0.f; }
            else t[k] = t[k] > 0.f ? vpow(t[k], d.power[i]) : 0.f;
        }
        if (d.comp[i][0] != 0.f)
            for (int k = 0; k < 4; ++k) {
                if (!(t[k] > 0.f)) ++cn->compression_vector_clamp;
                else ++cn->compression_taken;
                t[k] = vmaxf(t[k], 0.f);
                t[k] = oracle_xlogf_v(t[k] * d.comp[i][0] + 1.f) / d.comp[i][1];
            }
    }
    // CDL_v (L610-767) on four lanes; oor[k] collects the lanes' PQ ranges
    void cdl4(const Derived &d, float Y[4], float u[4], float v[4], bool oor[4])
    {
        const auto per_lane = [&](auto fn) { for (int k = 0; k < 4; ++k) { c.oor = false; fn(k); oor[k] = oor[k] || c.oor; } };
        for (int k = 0; k < 4; ++k) count_mode(d);
        if (d.rhs != 0.f) per_lane([&](int k) { hue_shift(d, Y[k], u[k], v[k]); });
        if (d.rgbmode) {
            if (d.rs != 1.f) for (int k = 0; k < 4; ++k) { u[k] *= d.rs; v[k] *= d.rs; }
            if (d.enabled) {
                float rgb[3][4];
                for (int k = 0; k < 4; ++k) yuv2rgb(c, Y[k], u[k], v[k], rgb[0][k], rgb[1][k], rgb[2][k]);
                const bool use_gamma = d.hsl && d.hslgamma != 1.f;
                const float gamma = 1.f / d.hslgamma, igamma = d.hslgamma;
                for (int i = 0; i < 3; ++i) {
                    float t[4];
                    for (int k = 0; k < 4; ++k) {
                        t[k] = rgb[i][k] / 65535.f;
                        if (use_gamma && t[k] > 0.f) { t[k] = vpow(t[k], gamma); ++cn->gamma; }
                    }
                    chain4(d, i, t);
                    for (int k = 0; k < 4; ++k) {
                        if (use_gamma && t[k] > 0.f) t[k] = vpow(t[k], igamma);
                        rgb[i][k] = t[k] * 65535.f;
                    }
                }
                for (int k = 0; k < 4; ++k) {
                    if (d.rgbmode != 2) {
                        rgb2yuv(c, rgb[0][k], rgb[1][k], rgb[2][k], Y[k], u[k], v[k]);
                    } else {
                        ++cn->rgbluminance;
                        float rr, gg, bb;
                        yuv2rgb(c, Y[k], u[k], v[k], rr, gg, bb);
                        const float Y1 = lum(c, rr + (rgb[0][k] - rr) * fR, gg + (rgb[1][k] - gg) * fG, bb + (rgb[2][k] - bb) * fB);
                        if (Y[k] > 0.f) {
                            const float f = Y1 / Y[k];
                            u[k] *= f;
                            v[k] *= f;
                        } else {
                            ++cn->y_nonpositive;
                        }
                        Y[k] = Y1;
                    }
                }
            }
            for (int k = 0; k < 4; ++k) {
                const float f = vmaxf(Y[k], 0.f);
                u[k] += f * d.abcb;
                v[k] += f * d.abca;
                if (d.rsout != 1.f) { u[k] *= d.rsout; v[k] *= d.rsout; }
            }
        } else {
            if (d.enabled) {
                float YY[4];
                for (int k = 0; k < 4; ++k) YY[k] = Y[k] / 65535.f;
                chain4(d, 0, YY);
                for (int k = 0; k < 4; ++k) {
                    YY[k] *= 65535.f;
                    if (!(Y[k] > 0.f)) ++cn->y_nonpositive;
                    const float f = Y[k] > 0.f ? YY[k] / Y[k] : 1.f;
                    Y[k] = YY[k];
                    u[k] *= f;
                    v[k] *= f;
                }
            }
            if (d.jzazbz) per_lane([&](int k) { yuv_to_jz(c, Y[k], u[k], v[k]); });
            for (int k = 0; k < 4; ++k) {
                if (d.rs != 1.f) { u[k] *= d.rs; v[k] *= d.rs; }
                const float f = vmaxf(Y[k], 0.f);
                u[k] += f * d.abcb;
                v[k] += f * d.abca;
                if (d.rsout != 1.f) { u[k] *= d.rsout; v[k] *= d.rsout; }
            }
            if (d.jzazbz) per_lane([&](int k) { jz_to_yuv(c, Y[k], u[k], v[k]); });
        }
    }
};

} // namespace

extern "C" {

// ImProcFunctions::colorCorrection on three W x H planes in RGB mode, in place.  info: n entries or NULL; oor: W * H bytes or NULL (1: the
// pixel called PQ / PQ_inv with an argument above 1 in some region); cn: counters.  Returns 0, or -4 where artgpu_color_correction is
// documented to return ARTGPU_EUNSUPPORTED (planes untouched).
int cc_ref_tool(float *r, float *g, float *b, int W, int H, const cc_ref_region *regions, int n, const double *ws, const double *iws, int to_rgb,
                cc_ref_info *info, unsigned char *oor, cc_ref_counts *cn)
{
    Tool t;
    std::memset(cn, 0, sizeof *cn);
    t.cn = t.c.cn = cn;
    t.c.oor = false;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { t.c.ws[i][j] = ws[3 * i + j]; t.c.iws[i][j] = iws[3 * i + j]; }
    const float max_ws = rt_max(rt_max(t.c.ws[1][0], t.c.ws[1][1]), t.c.ws[1][2]);
    t.fR = max_ws / t.c.ws[1][0]; t.fG = max_ws / t.c.ws[1][1]; t.fB = max_ws / t.c.ws[1][2];
    std::vector<Derived> d(n);
    for (int i = 0; i < n; ++i) {
        if (regions[i].mode == MODE_LUT) return -4;
        if (regions[i].mode == MODE_HSL && !(regions[i].hsl_gamma > 0.0)) return -4;
        derive(t.c, regions[i], d[i]);
        if (!finite_all(d[i])) return -4;
    }
    const size_t np = (size_t)W * H;
    if (oor) std::memset(oor, 0, np);
    float *const img[3] = {r, g, b};
    const float wsf[9] = {t.c.ws[0][0], t.c.ws[0][1], t.c.ws[0][2], t.c.ws[1][0], t.c.ws[1][1], t.c.ws[1][2], t.c.ws[2][0], t.c.ws[2][1], t.c.ws[2][2]};
    oracle_rgb_to_yuv(img, W, W, H, wsf);                                  // rgb->setMode(YUV) (L770): Y = g plane, u = b plane, v = r plane
    for (int y = 0; y < H; ++y)
        for (int i = 0; i < n; ++i) {
            float *Yr = g + (size_t)y * W, *ur = b + (size_t)y * W, *vr = r + (size_t)y * W;
            const float *ab = regions[i].abmask ? regions[i].abmask + (size_t)y * W : nullptr;
            const float *lm = regions[i].lmask ? regions[i].lmask + (size_t)y * W : nullptr;
            int x = 0;
            for (; x < W - 3; x += 4) {                                    // L810-834
                float blend[4], lblend[4];
                bool some = false, zero_lane = false;
                for (int k = 0; k < 4; ++k) {
                    blend[k] = ab ? ab[x + k] : 1.f;
                    lblend[k] = lm ? lm[x + k] : 1.f;
                    some = some || blend[k] > 0.f || lblend[k] > 0.f;
                    zero_lane = zero_lane || !(blend[k] > 0.f || lblend[k] > 0.f);
                }
                if (!some) continue;
                if (zero_lane) ++cn->groups_zero_lane;
                float Yn[4], un[4], vn[4];
                bool lane_oor[4] = {false, false, false, false};
                for (int k = 0; k < 4; ++k) { Yn[k] = Yr[x + k]; un[k] = ur[x + k]; vn[k] = vr[x + k]; }
                t.cdl4(d[i], Yn, un, vn, lane_oor);
                for (int k = 0; k < 4; ++k) {
                    Yr[x + k] = mix(lblend[k], Yn[k], Yr[x + k]);
                    ur[x + k] = mix(blend[k], un[k], ur[x + k]);
                    vr[x + k] = mix(blend[k], vn[k], vr[x + k]);
                    if (oor && lane_oor[k]) oor[(size_t)y * W + x + k] = 1;
                }
            }
            for (; x < W; ++x) {                                           // L836-859
                const float blend = ab ? ab[x] : 1.f, lblend = lm ? lm[x] : 1.f;
                if (!(blend > 0.f || lblend > 0.f)) { ++cn->tail_skipped; continue; }
                float Yn = Yr[x], un = ur[x], vn = vr[x];
                t.c.oor = false;
                t.cdl(d[i], Yn, un, vn);
                Yr[x] = mix(lblend, Yn, Yr[x]);
                ur[x] = mix(blend, un, ur[x]);
                vr[x] = mix(blend, vn, vr[x]);
                if (oor && t.c.oor) oor[(size_t)y * W + x] = 1;
            }
        }
    if (to_rgb) oracle_yuv_to_rgb(img, W, W, H, wsf);
    long long noor = 0;
    for (size_t k = 0; oor && k < np; ++k) noor += oor[k];
    for (int i = 0; info && i < n; ++i) {
        cc_ref_info &o = info[i];
        std::memset(&o, 0, sizeof o);
        o.abca = d[i].abca; o.abcb = d[i].abcb; o.enabled = d[i].enabled; o.rgbmode = d[i].rgbmode; o.rhs = d[i].rhs; o.oor_pixels = noor;
        for (int k = 0; k < 3; ++k) {
            o.slope[k] = d[i].slope[k]; o.offset[k] = d[i].offset[k]; o.power[k] = d[i].power[k]; o.pivot[k] = d[i].pivot[k];
            o.compression[k][0] = d[i].comp[k][0]; o.compression[k][1] = d[i].comp[k][1];
        }
    }
    return 0;
}

} // extern "C"
