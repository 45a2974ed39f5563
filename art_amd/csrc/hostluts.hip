// hostluts.hip -- host-side construction of the small look-up tables the device stages take as inputs.  These are
// the counterparts of tables the reference also builds once on the host (no per-pixel work here):
//   FlatCurve (FCT_MinMaxCPoints) polyline     rtengine/flatcurves.cc:27-77,124-360, rtengine/curves.cc:98-132
//   NoiseCurve::Set -> 501-entry LUT + sum     rtengine/ipdenoise.cc:684-716
//   Color::cachef                              rtengine/color.cc:178,202-217
//   tone_eq's correction table                 rtengine/iptoneequalizer.cc:95-114,160-190,305-310 (scalar sleef forms, sleef.h)
//   Color::gamma2curve, Color::igammatab_srgb  rtengine/color.cc:239-255, color.h:1122-1144
#include "kernels.h"
#include "toneequalizer.h"
#include "filmgrain.h"
#include "blackwhite.h"
#include "creativegradients.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace artgpu {

namespace {

struct Polyline {
    std::vector<double> x, y, slope;
    void add(double px, double py) { x.push_back(px); y.push_back(py); }
    // Curve::fillDyByDx
    void finish()
    {
        slope.resize(x.size() - 1);
        for (size_t i = 0; i + 1 < x.size(); ++i) slope[i] = (y[i + 1] - y[i]) / (x[i + 1] - x[i]);
    }
    // FlatCurve::getVal, FCT_MinMaxCPoints branch
    double eval(double t) const
    {
        if (t < x[0]) t += 1.0;
        unsigned lo = 0, hi = (unsigned)x.size() - 1;
        while (hi > 1 + lo) {
            const unsigned mid = (hi + lo) / 2;
            if (x[mid] > t) hi = mid; else lo = mid;
        }
        return y[lo] + (t - x[lo]) * slope[lo];
    }
};

struct Knot { double x, y, left, right; };

// One sub-curve of FlatCurve::CtrlPoints_set: either a straight segment (2 points) or a quadratic Bezier (3 points).
struct SubCurve { double px[3], py[3]; bool linear; double length; };

double seg(double x0, double y0, double x1, double y1) { const double dx = x1 - x0, dy = y1 - y0; return std::sqrt(dx * dx + dy * dy); }

SubCurve line(double x0, double y0, double x1, double y1)
{
    SubCurve s = {{x0, x1, 0.}, {y0, y1, 0.}, true, 0.};
    s.length = seg(x0, y0, x1, y1);
    return s;
}
SubCurve bezier(double x0, double y0, double x1, double y1, double x2, double y2)
{
    SubCurve s = {{x0, x1, x2}, {y0, y1, y2}, false, 0.};
    s.length = seg(x0, y0, x1, y1);
    s.length += seg(x1, y1, x2, y2);
    return s;
}

// FlatCurve::CtrlPoints_set (flatcurves.cc:124-327)
bool build_polyline(const std::vector<Knot> &k, bool periodic, int ppn, Polyline &poly)
{
    const int nseg = (int)k.size() - 1;   // the caller appended the wrap-around knot for periodic curves
    std::vector<SubCurve> sc;
    double total = 0.;
    for (int i = 0; i < nseg; ++i) {
        const Knot &a = k[i], &b = k[i + 1];
        const bool start_linear = a.right == 0. || a.y == b.y;
        const bool end_linear = b.left == 0. || a.y == b.y;
        if (start_linear && end_linear) {
            sc.push_back(line(a.x, a.y, b.x, b.y));
            total += sc.back().length;
            continue;
        }
        double xp1 = start_linear ? a.x : (b.x - a.x) * a.right + a.x;
        double xp3 = end_linear ? b.x : (a.x - b.x) * b.left + b.x;
        const double xp2 = (xp1 + xp3) / 2.0, yp2 = (a.y + b.y) / 2.0;
        if (a.right + b.left > 1.0) xp1 = xp3 = xp2;
        sc.push_back(start_linear ? line(a.x, a.y, xp2, yp2) : bezier(a.x, a.y, xp1, a.y, xp2, yp2));
        total += sc.back().length;
        sc.push_back(end_linear ? line(xp2, yp2, b.x, b.y) : bezier(xp2, yp2, xp3, b.y, b.x, b.y));
        total += sc.back().length;
    }
    if (sc.empty()) return false;
    if (!periodic && sc[0].px[0] != 0.) poly.add(0., sc[0].py[0]);
    poly.add(sc[0].px[0], sc[0].py[0]);
    double last_y = sc[0].py[0];
    for (const SubCurve &s : sc) {
        if (s.linear) {
            poly.add(s.px[1], s.py[1]);
            last_y = s.py[1];
        } else {
            const int npoints = (int)(((double)ppn * s.length) / total);
            if (npoints < 0) return false;
            const double increment = 1.0 / (double)(npoints - 1);
            for (int q = 1; q < npoints - 1; ++q) {          // Curve::AddPolygons, firstPointIncluded == false
                const double t = q * increment;
                const double t2 = t * t;
                const double tr = 1. - t;
                const double tr2 = tr * tr;
                const double tr2t = tr * 2 * t;
                poly.add(tr2 * s.px[0] + tr2t * s.px[1] + t2 * s.px[2], tr2 * s.py[0] + tr2t * s.py[1] + t2 * s.py[2]);
            }
            poly.add(s.px[2], s.py[2]);
            last_y = s.py[2];
        }
    }
    poly.add(3.0, last_y);
    poly.finish();
    return true;
}

} // namespace

// FlatCurve(points, periodic, ppn): the polyline FlatCurve::getVal works on.  Returns false for an identity / empty curve.
bool flat_curve_polyline(const double *pts, int npts, bool periodic, int ppn, double identity, std::vector<double> &x, std::vector<double> &y, std::vector<double> &slope)
{
    if (!(npts > 4 && (int)pts[0] == 1 /* FCT_MinMaxCPoints */)) return false;
    const int n = (npts - 1) / 4;
    std::vector<Knot> k;
    for (int i = 0; i < n; ++i) k.push_back({pts[1 + 4 * i], pts[2 + 4 * i], pts[3 + 4 * i], pts[4 + 4 * i]});
    if (periodic) k.push_back({pts[1] + 1.0, pts[2], pts[3], pts[4]});
    bool identity_curve = true;
    for (const Knot &q : k)
        if (q.y >= identity + 1.e-7 || q.y <= identity - 1.e-7) { identity_curve = false; break; }
    if (identity_curve || n <= (periodic ? 1 : 0)) return false;
    Polyline poly;
    if (!build_polyline(k, periodic, ppn > 65500 ? 65500 : ppn, poly)) return false;
    x = poly.x; y = poly.y; slope = poly.slope;
    return true;
}

// FlatCurve(points, periodic, ppn) + setIdentityValue(identity), sampled at i/(nout-1).  Returns true if identity.
bool flat_curve_sample(const double *pts, int npts, bool periodic, int ppn, double identity, int nout, double *out)
{
    bool identity_curve = true;
    Polyline poly;
    if (npts > 4 && (int)pts[0] == 1 /* FCT_MinMaxCPoints */) {
        const int n = (npts - 1) / 4;
        std::vector<Knot> k;
        for (int i = 0; i < n; ++i) k.push_back({pts[1 + 4 * i], pts[2 + 4 * i], pts[3 + 4 * i], pts[4 + 4 * i]});
        if (periodic) k.push_back({pts[1] + 1.0, pts[2], pts[3], pts[4]});
        for (const Knot &q : k)
            if (q.y >= identity + 1.e-7 || q.y <= identity - 1.e-7) { identity_curve = false; break; }
        if (!identity_curve && n > (periodic ? 1 : 0)) {
            if (!build_polyline(k, periodic, ppn > 65500 ? 65500 : ppn, poly)) identity_curve = true;
        } else {
            identity_curve = true;
        }
    }
    for (int s = 0; s < nout; ++s) out[s] = identity_curve ? identity : poly.eval((double)s / (double)(nout - 1));
    return identity_curve;
}

// NoiseCurve::Set(const std::vector<double>&): returns the running float sum (0 when the curve is reset)
float noise_curve_lut(const double *pts, int npts, float lut[501])
{
    for (int i = 0; i < 501; ++i) lut[i] = 0.f;
    if (!(npts > 0 && pts[0] > 0. && pts[0] < 2.)) return 0.f;      // FCT_Linear < kind < FCT_Unchanged
    double v[501];
    if (flat_curve_sample(pts, npts, false, 1000 / 2, 0., 501, v)) return 0.f;
    float sum = 0.f;
    for (int i = 0; i < 501; ++i) {
        lut[i] = (float)v[i];
        if (lut[i] < 0.01f) lut[i] = 0.01f;
        sum += lut[i];
    }
    return sum;
}

// Color::cachef
void build_cachef(float *lut)
{
    const double kappa = 24389.0 / 27.0, eps = 216.0 / 24389.0;
    const float maxvalf = 65535.f;
    const int epsmaxint = (int)((double)maxvalf * eps);
    int i = 0;
    for (; i <= epsmaxint; i++) lut[i] = (float)(327.68 * ((kappa * i / maxvalf + 16.0) / 116.0));
    for (; i < 65536; i++) lut[i] = (float)(327.68 * std::cbrt((double)i / maxvalf));
}


// Color::cachefy (color.cc:219-234)
void build_cachefy(float *lut)
{
    const double kappa = 24389.0 / 27.0, eps = 216.0 / 24389.0;
    const float maxvalf = 65535.f;
    const int epsmaxint = (int)((double)maxvalf * eps);
    int i = 0;
    for (; i <= epsmaxint; i++) lut[i] = (float)(327.68 * (kappa * i / maxvalf));
    for (; i < 65536; i++) lut[i] = (float)(327.68 * (116.0 * std::cbrt((double)i / maxvalf) - 16.0));
}

// Color::denoiseGammaTab / denoiseIGammaTab (color.cc:278-292; gamma55 / igamma55, color.h:1155-1169)
void build_denoise_gamma_tabs(float *gtab, float *igtab)
{
    for (int i = 0; i < 65536; i++) {
        const double x = i / 65535.0;
        gtab[i] = (float)(65535.0 * (x <= 0.013189 ? x * 10.0 : 1.593503 * std::exp(std::log(x) / 5.5) - 0.593503));
        igtab[i] = (float)(65535.0 * (x <= 0.131889 ? x / 10.0 : std::exp(std::log((x + 0.593503) / 1.593503) * 5.5)));
    }
}

// Color::gammatab_srgb, which Color::gamma2curve shares (color.cc:241-244): gamma2(i / 65535.0) (color.h:1127) stored as float, then *= 65535.f
void build_gamma2curve(float *lut)
{
    for (int i = 0; i < 65536; ++i) {
        const double x = i / 65535.0;
        lut[i] = (float)(x <= 0.003040 ? x * 12.92310 : 1.055 * std::exp(std::log(x) / 2.4) - 0.055);
    }
    for (int i = 0; i < 65536; ++i) lut[i] *= 65535.f;
}

// Color::igammatab_srgb (color.cc:252-255): igamma2(i / 65535.0) (color.h:1144) stored as float, then *= 65535.f
void build_igammatab_srgb(float *lut)
{
    for (int i = 0; i < 65536; ++i) {
        const double x = i / 65535.0;
        lut[i] = (float)(x <= 0.039286 ? x / 12.92310 : std::exp(std::log((x + 0.055) / 1.055) * 2.4));
    }
    for (int i = 0; i < 65536; ++i) lut[i] *= 65535.f;
}

// Color::init jzazbz_pq_ / jzazbz_pq_inv_ (color.cc:323-326) with PQ / PQ_inv (color.cc:67-86): std::pow(float, float) is the
// host libm's powf, as in the reference
void build_pq_luts(float *pq, float *pq_inv)
{
    for (int i = 0; i < 65536; ++i) {
        const float v = (float)i / 65535.f;
        float X = std::max(v, 1e-10f);
        const float XX = std::pow(X * 1e-4f, 0.1593017578125f);
        pq[i] = std::pow((0.8359375f + 18.8515625f * XX) / (1 + 18.6875f * XX), 134.034375f);
        const float YY = std::pow(X, 7.460772656268214e-03f);
        pq_inv[i] = 1e4f * std::pow((0.8359375f - YY) / (18.6875f * YY - 18.8515625f), 6.277394636015326f);
    }
}

// ---------------------------------------------------------------- AUTOMATIC chrominance: the scalar part of the estimation
// ShrinkAll_info's per-band bookkeeping (FTblockDN.cc:1292-1334) over the 5 levels x 3 directions of one crop.
// mad_a / mad_b: SQR(MadRgb) of the a / b subbands in level-major order (what launch_mad leaves on the device).  out: chaut, maxredaut, maxblueaut, minredaut, minblueaut, Nb
void dninfo_band_stats(const float *mad_a, const float *mad_b, int nbands, bool aggressive, float out[6])
{
    const float reduc = aggressive ? static_cast<float>(0.9) : 1.f;
    float chau = 0.f, maxchred = 0.f, maxchblue = 0.f, minchred = 100000000.f, minchblue = 100000000.f;
    float chaut = 0.f, maxredaut = 0.f, maxblueaut = 0.f, minredaut = 0.f, minblueaut = 0.f;
    int nb = 0;
    for (int k = 0; k < nbands; ++k) {
        const float mada = mad_a[k], madb = mad_b[k];
        maxchred = mada > maxchred ? mada : maxchred;
        minchred = mada < minchred ? mada : minchred;
        maxredaut = std::sqrt(reduc * maxchred);
        minredaut = std::sqrt(reduc * minchred);
        maxchblue = madb > maxchblue ? madb : maxchblue;
        minchblue = madb < minchblue ? madb : minchblue;
        maxblueaut = std::sqrt(reduc * maxchblue);
        minblueaut = std::sqrt(reduc * minchblue);
        chau += (mada + madb);
        ++nb;
        chaut = std::sqrt(reduc * chau / (nb + nb));
    }
    out[0] = chaut; out[1] = maxredaut; out[2] = maxblueaut; out[3] = minredaut; out[4] = minblueaut; out[5] = (float)nb;
}

// calcautodn_info (ipdenoise.cc:66-206) for the arguments its one caller passes: levaut 0, mode 1 ("auto"), lissage 0
// (ipdenoise.cc:893,1003-1004).  Returns delta; chaut is updated in place like the reference's by-reference argument.
static float autodn_adjust(float &chaut, int Nb, float maxmax, float lumema, float chromina, float redyel, float skinc, float nsknc, bool aggressive)
{
    struct Step { float below; float scale; };
    chaut = (chaut * Nb - maxmax) / (Nb - 1);                        // drop the maximum from the mean
    const bool strong_colour = chromina > 3000.f;
    if ((redyel > 5000.f || skinc > 1000.f) && nsknc < 0.4f && strong_colour) chaut *= 0.45f;
    else if ((redyel > 12000.f || skinc > 1200.f) && nsknc < 0.3f && strong_colour) chaut *= 0.3f;
    if (chromina > 10000.f) chaut *= 0.8f;
    else if (chromina > 6000.f) chaut *= 0.9f;
    else if (chromina < 3000.f) chaut *= 1.5f;
    if (lumema < 2500.f) chaut *= 1.2f;
    else if (lumema < 5000.f) chaut *= 1.1f;
    else if (lumema > 20000.f) chaut *= 0.9f;
    if (chaut > 300.f) chaut = 0.714286f * chaut + 85.71428f;      // "low denoise"
    float delta = (maxmax - chaut) * (aggressive ? static_cast<float>(0.9) : 1.f);
    if (chaut < 400.f) {
        const bool low = chaut < 200.f;
        const float knee = low ? 200.f : 400.f;
        if (delta < knee) delta *= low ? 0.95f : 0.6f;
        else if (low && delta < 400.f) delta *= 0.7f;
        else delta = low ? 280.f : 200.f;
    } else {
        static const Step ladder[] = {{550.f, 0.3f}, {650.f, 0.2f}};
        float sc = 0.15f;
        for (const Step &st : ladder) if (chaut < st.below) { sc = st.scale; break; }
        delta *= sc;
    }
    if (chromina < 6000.f) delta *= 1.2f;
    if (lumema < 5000.f) delta *= 1.2f;
    return delta;
}

// The reduction over the nine crops (ipdenoise.cc:960-1072): autoNR 10, autoNRmax 40, multip = adjustr = lowdenoise = 1 (raw).
// info[k] = {chaut, maxredaut, maxblueaut, minredaut, minblueaut, chromina, lumema, redyel, skinc, nsknc, Nb}
void dninfo_reduce(const float info[9][16], bool aggressive, float ch_M[9], float max_r[9], float max_b[9], float out3[3])
{
    const float nrmax = 40.f, nr = 10.f;
    float up_r[9], up_b[9], dn_r[9], dn_b[9];
    for (int k = 0; k < 9; ++k) {
        ch_M[k] = 1.0f * info[k][0]; max_r[k] = 1.0f * info[k][1]; max_b[k] = 1.0f * info[k][2];
        const float min_r = 1.0f * info[k][3], min_b = 1.0f * info[k][4];
        const float delta = autodn_adjust(ch_M[k], (int)info[k][10], std::max(max_r[k], max_b[k]), info[k][6], info[k][5], info[k][7], info[k][8], info[k][9], aggressive);
        const bool red = max_r[k] > max_b[k];
        const float up = delta / (nrmax / 2.f);
        up_r[k] = red ? up : 0.f;
        up_b[k] = red ? 0.f : up;
        dn_b[k] = red ? -(ch_M[k] - min_b) / nrmax : 0.f;
        dn_r[k] = red ? 0.f : -(ch_M[k] - min_r) / nrmax;
    }
    float chM = 0.f, top_r = 0.f, top_b = 0.f, low_r = 100000000000.f, low_b = 100000000000.f;
    float mean_up_r = 0.f, mean_up_b = 0.f, mean_dn_r = 0.f, mean_dn_b = 0.f;
    for (int k = 0; k < 9; ++k) {
        chM += ch_M[k]; mean_up_b += up_b[k]; mean_up_r += up_r[k]; mean_dn_r += dn_r[k]; mean_dn_b += dn_b[k];
        if (up_r[k] > top_r) top_r = up_r[k];
        if (up_b[k] > top_b) top_b = up_b[k];
        if (dn_r[k] < low_r) low_r = dn_r[k];
        if (dn_b[k] < low_b) low_b = dn_b[k];
    }
    chM /= 9; mean_up_b /= 9; mean_up_r /= 9; mean_dn_b /= 9; mean_dn_r /= 9;
    float maxr, maxb;
    if (top_r > top_b) {
        maxr = mean_up_r + (top_r - mean_up_r) * 0.66f;
        maxb = mean_dn_b + (low_b - mean_dn_b) * 0.66f;
    } else {
        maxb = mean_up_b + (top_b - mean_up_b) * 0.66f;
        maxr = mean_dn_r + (low_r - mean_dn_r) * 0.66f;
    }
    out3[0] = chM / nr; out3[1] = maxr; out3[2] = maxb;
}

// ---------------------------------------------------------------- tone equalizer: the correction table
// The scalar xlogf / xexpf / pow_F of rtengine/sleef.h:938-966,1198-1265,1296-1300 on the host, statement for statement the forms devsleef.h
// holds for the device (this file is compiled with -ffp-contract=off as well).
namespace {

inline int hs_f2i(float f) { int i; std::memcpy(&i, &f, 4); return i; }
inline float hs_i2f(int i) { float f; std::memcpy(&f, &i, 4); return f; }
inline float hs_mla(float x, float y, float z) { return x * y + z; }
inline int hs_ilogbp1f(float d)
{
    const bool m = d < 5.421010862427522E-20f;
    d = m ? 1.8446744073709552E19f * d : d;
    const int q = (hs_f2i(d) >> 23) & 0xff;
    return m ? q - (64 + 0x7e) : q - 0x7e;
}
inline float hs_ldexpkf(float x, int q)
{
    int m = q >> 31;
    m = (((m + q) >> 6) - m) << 4;
    q = q - (m << 2);
    float u = hs_i2f((m + 0x7f) << 23);
    u = u * u;
    x = x * u * u;
    u = hs_i2f((q + 0x7f) << 23);
    return x * u;
}
float hs_xexpf(float d)
{
    if (d <= -104.0f) return 0.0f;
    const int q = (int)std::lrintf(d * 1.442695040888963407359924681001892137426645954152985934135449406931f);   // xrintf: to nearest even
    float s = hs_mla((float)q, -0.693145751953125f, d);
    s = hs_mla((float)q, -1.428606765330187045e-06f, s);
    float u = 0.00136324646882712841033936f;
    u = hs_mla(u, s, 0.00836596917361021041870117f);
    u = hs_mla(u, s, 0.0416710823774337768554688f);
    u = hs_mla(u, s, 0.166665524244308471679688f);
    u = hs_mla(u, s, 0.499999850988388061523438f);
    u = hs_mla(s, hs_mla(s, u, 1.f), 1.f);
    return hs_ldexpkf(u, q);
}
float hs_xlogf(float d)
{
    const int e = hs_ilogbp1f(d * 0.7071f);
    const float m = hs_ldexpkf(d, -e);
    float x = (m - 1.0f) / (m + 1.0f);
    const float x2 = x * x;
    float t = 0.2371599674224853515625f;
    t = hs_mla(t, x2, 0.285279005765914916992188f);
    t = hs_mla(t, x2, 0.400005519390106201171875f);
    t = hs_mla(t, x2, 0.666666567325592041015625f);
    t = hs_mla(t, x2, 2.0f);
    x = x * t + 0.693147180559945286226764f * (float)e;
    if (d == INFINITY) x = INFINITY;
    if (d < 0.f) x = NAN;
    if (d == 0.f) x = -INFINITY;
    return x;
}
inline float hs_pow_F(float a, float b) { return hs_xexpf(b * hs_xlogf(a)); }

} // namespace

// gain (iptoneequalizer.cc:354), factors (L95-114), w_sum (L167-170) and lut[i] = process_pixel(i / 65535.f) (L175-190, L305-310)
void te_build_lut(const int bands[5], double pivot, float *lut, float *gain, float *w_sum, float factors[12])
{
    const float l2 = hs_xlogf(2.f);
    const auto conv = [](int v, float lo, float hi) -> float { const float f = v < 0 ? lo : hi; return hs_pow_F(2.f, float(v) / 100.f * f); };
    const auto gauss = [](float b, float x) -> float { return hs_xexpf(-((x - b) * (x - b)) / 4.0f); };
    for (int c = 0; c < 12; ++c) {
        const int band = c < 5 ? 0 : (c < 8 ? c - 4 : 4);
        factors[c] = band < 2 ? conv(bands[band], 2.f, 3.f) : (band == 2 ? conv(bands[2], 2.5f, 2.5f) : conv(bands[band], 3.f, 2.f));
    }
    *gain = (float)(1.f / 65535.f * std::pow(2.f, -pivot));     // float * double, narrowed at the initialisation
    float ws = 0.f;
    for (int c = 0; c < 12; ++c) ws += gauss(-16.f + 2.f * c, 0.f);
    *w_sum = ws;
    if (!lut) return;
    for (int i = 0; i < 65536; ++i) {
        const float y = float(i) / 65535.f;
        const float l = hs_xlogf(y < 0.f ? 0.f : y) / l2;
        const float luma = std::max(-14.f, std::min(l, 4.f));
        float corr = 0.f;
        for (int c = 0; c < 12; ++c) corr += gauss(-16.f + 2.f * c, luma) * factors[c];
        lut[i] = corr / ws;
    }
}

// ---------------------------------------------------------------- film grain: the normal table, the cone, the jump maps
// RandomNumberGenerator (rng.h:31-57) stepped serially through NormalDistribution (rng.h:61-90), every conversion as written there.  Only
// bits 16..47 of the state are ever read and bit k of the next state depends on bits <= k, so the low 48 bits are the whole generator.
void build_grain_table(int seed, float *normd, uint64_t *state48)
{
    uint64_t st = (uint64_t)(uint32_t)seed & FG_MASK48;
    const auto randint = [&st](uint32_t upper_bound) -> uint32_t {
        st = (st * FG_LCG_A + FG_LCG_C) & FG_MASK48;
        return uint32_t(st >> 16U) % upper_bound;
    };
    const auto randfloat = [&randint]() -> float {
        const uint32_t ub = 2147483647u;                    // std::numeric_limits<int>::max()
        return float(randint(ub)) / float(ub);
    };
    const float mean = 0.f, std_dev = 1.f;
    float spare = 0.f;
    bool has_spare = false;
    for (int i = 0; i < FG_NORMD; ++i) {
        if (has_spare) {
            has_spare = false;
            normd[i] = spare * std_dev + mean;
        } else {
            double u, v, s;
            do {
                u = randfloat() * 2.f - 1.f;
                v = randfloat() * 2.f - 1.f;
                s = u * u + v * v;
            } while (s >= 1.f || s == 0.f);
            s = sqrtf(float(-2.f * hs_xlogf(float(s)) / s));     // xlogf takes a float; the quotient is double, sqrtf narrows it
            spare = float(v * s);
            has_spare = true;
            normd[i] = float(mean + std_dev * u * s);
        }
    }
    *state48 = st;
}

// the cone of ipsmoothing.cc:577-597
int build_grain_kernel(float radius, float *taps)
{
    if (!(radius > 0.f) || std::isinf(radius) || std::ceil(radius) > (float)FG_MAX_R) return 0;
    const int sz = int(std::ceil(radius)) * 2 + 1;
    const int c = sz / 2;
    double totd = 0.0;
    for (int i = 0; i < sz; ++i)
        for (int j = 0; j < sz; ++j) {
            const float r = (float)std::sqrt((double)((i - c) * (i - c) + (j - c) * (j - c)));       // std::sqrt(int): double, narrowed
            const float d = r - radius;
            taps[i * sz + j] = d < 0.f ? 1.f : std::max(1.f - d, 0.f);
            totd += taps[i * sz + j];
        }
    const float tot = (float)totd;
    for (int k = 0; k < sz * sz; ++k) taps[k] /= tot;
    return sz;
}

// 2^j steps as one affine map: the square of the map of 2^(j-1) steps
void build_grain_jump(FgJump *j)
{
    j->A[0] = FG_LCG_A; j->C[0] = FG_LCG_C;
    for (int b = 1; b < FG_JUMP_BITS; ++b) {
        j->A[b] = (j->A[b - 1] * j->A[b - 1]) & FG_MASK48;
        j->C[b] = (j->A[b - 1] * j->C[b - 1] + j->C[b - 1]) & FG_MASK48;
    }
}

// ---------------------------------------------------------------- soft light's table, black-and-white's mixer constants and gamma tables
namespace {
// LUTf::operator[](float) (LUT.h:436-459) on the host; clip: LUT_CLIP_BELOW | LUT_CLIP_ABOVE set (the constructor's default) or neither (flags 0)
float hs_lutf(const float *data, int size, float index, bool clip)
{
    const int maxs = size - 2;
    int idx = (int)index;
    if (index < 0.f || !(index == index)) {
        if (clip) return data[0];
        idx = 0;
    } else if (index > (float)maxs) {
        if (clip) return data[size - 1];
        idx = maxs;
    }
    const float diff = index - (float)idx;
    const float p1 = data[idx];
    const float p2 = data[idx + 1] - p1;
    return p1 + p2 * diff;
}
} // namespace

// ImProcFunctions::softLight's LUTf f (ipsoftlight.cc:31-41, 55-60): f[i] = sl(blend, i).  Color::gamma_srgb / igamma_srgb are float-indexed
// lookups in gammatab_srgb / igammatab_srgb, tables with flags 0 (color.cc:183-185): index 65535 goes through the extrapolating branch
void build_soft_light_lut(int strength, float *lut)
{
    std::vector<float> gam(65536), igam(65536);
    build_gamma2curve(gam.data());
    build_igammatab_srgb(igam.data());
    const float blend = strength / 100.f;
    for (int i = 0; i < 65536; ++i) {
        float x = i;
        float v = hs_lutf(gam.data(), 65536, x, false) / 65535.f;
        const float v2 = v * v;
        const float v22 = v2 * 2.f;
        v = v2 + v22 - v22 * v;                                                   // Pegtop's formula
        const float b = hs_lutf(igam.data(), 65536, v * 65535.f, false);
        lut[i] = blend * b + (1.f - blend) * x;                                   // intp (rt_math.h:110-118)
    }
}

// computeBWMixerConstants (ipbw.cc:50-211) with algo "" as blackAndWhite calls it, statement by statement.  L192-194 are part of the
// definition: each of the three uses the mixer values the line before it has already overwritten.  kcorec comes in as 1.f (L258)
void bw_mixer_constants(int setting, int filter, float mixerRed, float mixerGreen, float mixerBlue, BwMixer *o)
{
    static const float presets[BW_NPRESETS][3] = {{43.f, 33.f, 30.f}, {33.3f, 33.3f, 33.3f}, {41.f, 25.f, 34.f}, {27.f, 27.f, 46.f}, {30.f, 28.f, 42.f}, {0.f, 42.f, 58.f},
                                                  {40.f, 34.f, 60.f}, {30.f, 59.f, 11.f}, {66.f, 24.f, 10.f}, {54.f, 44.f, 12.f}, {-40.f, 200.f, -17.f}};
    static const float filters[BW_NFILTERS][4] = {{1.f, 1.f, 1.f, 1.f}, {1.f, 0.05f, 0.f, 1.08f}, {1.f, 0.6f, 0.f, 1.35f}, {1.f, 1.f, 0.05f, 1.23f}, {0.6f, 1.f, 0.3f, 1.32f},
                                                  {0.2f, 1.f, 0.3f, 1.41f}, {0.05f, 1.f, 1.f, 1.23f}, {0.f, 0.05f, 1.f, 1.20f}, {1.f, 0.05f, 1.f, 1.23f}};
    float kcorec = 1.f;
    float somm;
    float som = mixerRed + mixerGreen + mixerBlue;
    if (som >= 0.f && som < 1.f) som = 1.f;
    if (som < 0.f && som > -1.f) som = -1.f;
    if (setting >= 0 && setting < BW_NPRESETS) {
        mixerRed = presets[setting][0];
        mixerGreen = presets[setting][1];
        mixerBlue = presets[setting][2];
    }
    if (setting == BW_RGB_ABS || setting == BW_ROYGCBPM_ABS) kcorec = som / 100.f;
    o->rrm = mixerRed;
    o->ggm = mixerGreen;
    o->bbm = mixerBlue;
    somm = mixerRed + mixerGreen + mixerBlue;
    if (somm >= 0.f && somm < 1.f) somm = 1.f;
    if (somm < 0.f && somm > -1.f) somm = -1.f;
    mixerRed = mixerRed / somm;
    mixerGreen = mixerGreen / somm;
    mixerBlue = mixerBlue / somm;
    float filred = 1.f, filgreen = 1.f, filblue = 1.f, filcor = 1.f;
    if (filter >= 0 && filter < BW_NFILTERS) {
        filred = filters[filter][0];
        filgreen = filters[filter][1];
        filblue = filters[filter][2];
        filcor = filters[filter][3];
    }
    mixerRed = mixerRed * filred;
    mixerGreen = mixerGreen * filgreen;
    mixerBlue = mixerBlue * filblue;
    if (mixerRed + mixerGreen + mixerBlue == 0) mixerRed += 1.f;
    mixerRed = filcor * mixerRed / (mixerRed + mixerGreen + mixerBlue);
    mixerGreen = filcor * mixerGreen / (mixerRed + mixerGreen + mixerBlue);
    mixerBlue = filcor * mixerBlue / (mixerRed + mixerGreen + mixerBlue);
    if (filter != 0) {
        som = mixerRed + mixerGreen + mixerBlue;
        if (som >= 0.f && som < 1.f) som = 1.f;
        if (som < 0.f && som > -1.f) som = -1.f;
        if (setting == BW_RGB_ABS) kcorec = kcorec * som;
    }
    o->bwr = mixerRed; o->bwg = mixerGreen; o->bwb = mixerBlue; o->kcorec = kcorec; o->filcor = filcor;
}

// blackAndWhite's gamma exponent of one channel (ipbw.cc:225-251) and its table (L268-272)
float bw_gamma_of(int gam)
{
    const float bwgam = float(gam);
    const float gamval = bwgam < 0 ? 100.f : 125.f;
    return 1.f - bwgam / gamval;
}
void build_bw_gamma_table(float gamma, float *lut)
{
    for (int i = 0; i < 65536; ++i) lut[i] = hs_pow_F(float(i) / 65535.f, gamma) * 65535.f;
}

// ---------------------------------------------------------------- the graduated filter's and the vignette filter's derived parameters
// calcGradientParams (iptransform.cc:677-758), statement by statement.  Unqualified sqrt / fabs / cos / tan / fmod / pow are the overloads the
// reference's translation unit sees (rtengine.h pulls in <math.h> through lcms2.h, so the global names carry the float overloads): sqrt of the
// float sum is the float one, everything on gradient_angle is double
void cg_gradient_params(int oW, int oH, const CgInput &gradient, CgDerived *gp)
{
    constexpr double RT_PI = 3.14159265358979323846;
    int w = oW;
    int h = oH;
    double gradient_stops = gradient.strength;
    double gradient_span = gradient.feather / 100.0;
    double gradient_center_x = gradient.center_x / 200.0 + 0.5;
    double gradient_center_y = gradient.center_y / 200.0 + 0.5;
    double gradient_angle = gradient.degree / 180.0 * RT_PI;
    gradient_angle = std::fmod(gradient_angle, 2 * RT_PI);
    if (gradient_angle < 0.0) gradient_angle += 2.0 * RT_PI;
    bool bright_top = false, transpose = false, angle_is_zero = false;
    gp->h = h;
    double cosgrad = std::cos(gradient_angle);
    if (std::fabs(cosgrad) < 0.707) {
        transpose = true;
        gradient_angle += 0.5 * RT_PI;
        double gxc = gradient_center_x;
        gradient_center_x = 1.0 - gradient_center_y;
        gradient_center_y = gxc;
    }
    gradient_angle = std::fmod(gradient_angle, 2 * RT_PI);
    if (gradient_angle > 0.5 * RT_PI && gradient_angle < RT_PI) {
        gradient_angle += RT_PI;
        bright_top = true;
    } else if (gradient_angle >= RT_PI && gradient_angle < 1.5 * RT_PI) {
        gradient_angle -= RT_PI;
        bright_top = true;
    }
    if (std::fabs(gradient_angle) < 0.001 || std::fabs(gradient_angle - 2 * RT_PI) < 0.001) {
        gradient_angle = 0;
        angle_is_zero = true;
    }
    if (transpose) bright_top = !bright_top;
    if (transpose) { int tmp = w; w = h; h = tmp; }
    gp->scale = 1.0 / std::pow(2.0, gradient_stops);           // pow(int, double) promotes the 2
    if (bright_top) { gp->topmul = 1.0; gp->botmul = gp->scale; }
    else { gp->topmul = gp->scale; gp->botmul = 1.0; }
    gp->ta = std::tan(gradient_angle);
    gp->xc = w * gradient_center_x;
    gp->yc = h * gradient_center_y;
    gp->ys = std::sqrt((float)h * h + (float)w * w) * (gradient_span / std::cos(gradient_angle));     // float sqrt, double product
    gp->ys_inv = 1.0 / gp->ys;
    gp->top_edge_0 = gp->yc - gp->ys / 2.0;
    if (gp->ys < 1.0 / h) {
        gp->ys_inv = 0;
        gp->ys = 0;
    }
    gp->bright_top = bright_top; gp->transpose = transpose; gp->angle_is_zero = angle_is_zero;
}

// calcPCVignetteParams (L828-895): powf is the host libm's, as in the reference; the int fields truncate their float expressions
void cg_pcvignette_params(int fW, int fH, int oW, int oH, const CgInput &pcvignette, CgDerived *pcv)
{
    double roundness = pcvignette.pcv_roundness / 100.0;
    pcv->feather = pcvignette.pcv_feather / 100.0;
    if (pcvignette.crop_enabled) {
        float sW = float(oW) / fW;
        float sH = float(oH) / fH;
        pcv->ew = pcvignette.crop_w * sW;
        pcv->eh = pcvignette.crop_h * sH;
        pcv->x1 = pcvignette.crop_x * sW;
        pcv->y1 = pcvignette.crop_y * sH;
    } else {
        pcv->ew = oW;
        pcv->eh = oH;
        pcv->x1 = 0;
        pcv->y1 = 0;
    }
    float dW = pcvignette.pcv_center_x / 200.f * pcv->ew;
    float dH = pcvignette.pcv_center_y / 200.f * pcv->eh;
    pcv->ex = pcv->x1 + dW;
    pcv->ey = pcv->y1 + dH;
    pcv->x2 = pcv->x1 + pcv->ew + std::abs(dW);
    pcv->y2 = pcv->y1 + pcv->eh + std::abs(dH);
    pcv->fadeout_mul = 1.0 / (0.05 * sqrtf(oW * oW + oH * oH));
    float short_side = (pcv->ew < pcv->eh) ? pcv->ew : pcv->eh;
    float long_side = (pcv->ew > pcv->eh) ? pcv->ew : pcv->eh;
    pcv->sep = 2;
    pcv->sepmix = 0;
    pcv->oe_a = std::sqrt(2.0) * long_side * 0.5;
    pcv->oe_b = pcv->oe_a * short_side / long_side;
    pcv->ie_mul = (1.0 / std::sqrt(2.0)) * (1.0 - pcv->feather);
    pcv->is_super_ellipse_mode = 0;
    pcv->is_portrait = (pcv->ew < pcv->eh);
    if (roundness < 0.5) {
        pcv->is_super_ellipse_mode = 1;
        float sepf = 2 + 4 * powf(1.0 - 2 * roundness, 1.3);
        pcv->sep = ((int)sepf) & ~0x1;
        pcv->sepmix = (sepf - pcv->sep) * 0.5;
        pcv->oe1_a = powf(2.0, 1.0 / pcv->sep) * long_side * 0.5;
        pcv->oe1_b = pcv->oe1_a * short_side / long_side;
        pcv->ie1_mul = (1.0 / powf(2.0, 1.0 / pcv->sep)) * (1.0 - pcv->feather);
        pcv->oe2_a = powf(2.0, 1.0 / (pcv->sep + 2)) * long_side * 0.5;
        pcv->oe2_b = pcv->oe2_a * short_side / long_side;
        pcv->ie2_mul = (1.0 / powf(2.0, 1.0 / (pcv->sep + 2))) * (1.0 - pcv->feather);
    }
    if (roundness > 0.5) {
        float rad = sqrtf(pcv->ew * pcv->ew + pcv->eh * pcv->eh) / 2.0;
        float diff_a = rad - pcv->oe_a;
        float diff_b = rad - pcv->oe_b;
        pcv->oe_a = pcv->oe_a + diff_a * 2 * (roundness - 0.5);
        pcv->oe_b = pcv->oe_b + diff_b * 2 * (roundness - 0.5);
    }
    pcv->pcv_scale = powf(2, -pcvignette.pcv_strength);
    if (pcvignette.pcv_strength >= 6.0) pcv->pcv_scale = 0.0;
}

} // namespace artgpu
