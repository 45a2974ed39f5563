// tests/emul/masks_ref.cc -- CPU checker for artgpu_generate_masks: the parametric path of rtengine::generateMasks (rtengine/masks.cc:
// 1037-1516 with contrast_threshold_mask L696-734, mask_postprocess L737-802 and the by-mode rgb2lab L612-636) restated serially on
// contiguous float planes, with a counter for every branch.  Test infrastructure only; built on first use with -ffp-contract=off (rtengine
// is built without contraction).
//
// The guided filter, FlatCurve, Color::rgb2lab, xatan2f, xlin2log, xexpf, rescaleBilinear and gaussianBlur are liboracle's restatements
// (oracle_guided_filter, oracle_flat_curve_*, oracle_rgb2lab, oracle_xatan2f, oracle_xlin2log, oracle_xexpf_s / _v,
// oracle_rescale_bilinear, oracle_gaussian_blur), not a second copy.  buildBlendMask is restated here because liboracle's takes neither
// the blur radius nor the luminance factor.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

extern "C" {
void *oracle_flat_curve_new(const double *pts, int npts, int periodic, int ppn, double identity);
int oracle_flat_curve_is_identity(const void *h);
double oracle_flat_curve_get(const void *h, double t);
void oracle_flat_curve_free(void *h);
void oracle_rgb2lab(float R, float G, float B, float *l, float *a, float *b, const float ws[9]);
float oracle_xatan2f(float y, float x);
float oracle_xlin2log(float x, float base);
float oracle_xexpf_s(float d);
float oracle_xexpf_v(float d);
void oracle_rescale_bilinear(const float *src, int Ws, int Hs, float *dst, int Wd, int Hd);
void oracle_guided_filter(const float *guide, const float *src, float *dst, int W, int H, int r, float epsilon, int subsampling);
void oracle_gaussian_blur(float *img, int W, int H, double sigma);
}

namespace {
template <typename T> inline const T &rt_min(const T &a, const T &b) { return b < a ? b : a; }   // rt_math.h:55-58
template <typename T> inline const T &rt_max(const T &a, const T &b) { return a < b ? b : a; }   // rt_math.h:73-76
inline float LIM01(float a) { return rt_max(0.f, rt_min(a, 1.f)); }
inline int LIMi(int v, int lo, int hi) { return rt_max(lo, rt_min(v, hi)); }
inline float SQR(float x) { return x * x; }
inline float intp(float a, float b, float c) { return a * b + (1.f - a) * c; }                   // rt_math.h:110-118
}

extern "C" {

struct mk_ref_mask {            // artgpu_mask_params with `area` as a contiguous W x H plane
    int32_t parametric_enabled, lightness_detail;
    const double *hue, *chromaticity, *lightness;
    int32_t nhue, nchromaticity, nlightness, contrast_threshold;
    double blur;
    const float *area;
    int32_t posterization, smoothing, inverted, opacity;
    int32_t deltae_enabled, drawn_enabled, external_enabled, linked_enabled, curve_is_identity, show_mask;
};
struct mk_ref_info {            // the layout of artgpu_masks_info
    int32_t has_mask, has_lmask, ll_radius_small, ll_radius, blurred, r1, r2, cthr_w, cthr_h, smoothing_radius;
};
enum { MK_REF_MAX_REGIONS = 8 };
struct mk_ref_counts {
    long long hue_segment[10];                       // pixels per piece of huelab_to_huehsv2; [9]: none of them (hr stays 0)
    long long hue_fix_low, hue_fix_high;             // its own hr < 0 / hr > 1 corrections
    long long hue_wraps;                             // h + 1/6 > 1
    long long curve_evals[MK_REF_MAX_REGIONS][3];    // FlatCurve::getVal calls per region: hue, chromaticity, lightness
    long long curve_identity;                        // of which on a curve the constructor found to be the identity
    long long guide_low, guide_high;                 // LIM01(l) clamped
    long long clamp_low, clamp_high;                 // the LIM01 behind the guided blur
    long long blurred_regions, filled_planes;
    long long ll_built, ll_read;                     // the lightness-detail plane was built / pixels that read it
    long long cthr_rescaled, cthr_plain, cthr_negative;
    long long area_pixels;
    long long poster_level[31];                      // int(m * p + 0.5) values hit
    long long thr_fill, thr_one;                     // threshold plane: fillval / 1.f
    long long inverted_planes, opacity_planes;
};

static const double DEFAULT_HUE[9] = {1, 0.166666667, 1., 0.35, 0.35, 0.8287775246, 1., 0.35, 0.35};
static const double DEFAULT_CL[9] = {1, 0., 1., 0.35, 0.35, 1., 1., 0.35, 0.35};

static bool curve_present(const mk_ref_mask &m, const double *pts, int n, const double *dflt)
{
    if (!m.parametric_enabled) return false;
    if (!pts || n <= 0) return false;                 // empty
    if (pts[0] == 0) return false;                    // FCT_Linear
    if (n == 9 && std::equal(pts, pts + 9, dflt)) return false;
    return true;
}

// Color::huelab_to_huehsv2 (color.h:1719-1754)
static double hue_remap(float HH, mk_ref_counts *cn)
{
    double hr = 0.0;
    int seg = 9;
    if (HH >= 0.f && HH < 0.6f) { hr = 0.11666 * double(HH) + 0.93; seg = 0; }
    else if (HH >= 0.6f && HH < 1.4f) { hr = 0.1125 * double(HH) - 0.0675; seg = 1; }
    else if (HH >= 1.4f && HH < 2.f) { hr = 0.2666 * double(HH) - 0.2833; seg = 2; }
    else if (HH >= 2.f && HH <= 3.14159f) { hr = 0.1489 * double(HH) - 0.04785; seg = 3; }
    else if (HH >= -3.1416f && HH < -2.8f) { hr = 0.23419 * double(HH) + 1.1557; seg = 4; }
    else if (HH >= -2.8f && HH < -2.3f) { hr = 0.16 * double(HH) + 0.948; seg = 5; }
    else if (HH >= -2.3f && HH < -0.9f) { hr = 0.12143 * double(HH) + 0.85928; seg = 6; }
    else if (HH >= -0.9f && HH < -0.1f) { hr = 0.2125 * double(HH) + 0.94125; seg = 7; }
    else if (HH >= -0.1f && HH < 0.f) { hr = 0.1 * double(HH) + 0.93; seg = 8; }
    ++cn->hue_segment[seg];
    if (hr < 0.0) { hr += 1.0; ++cn->hue_fix_low; }
    else if (hr > 1.0) { hr -= 1.0; ++cn->hue_fix_high; }
    return hr;
}

// buildBlendMask(luminance, blend, W, H, thr, 1.f, false, blur_radius, luminance_factor) (rt_algo.cc:416-494), thr != 0
static void blend_mask(const float *L, float *blend, int W, int H, float thr, float blur_radius, float luminance_factor)
{
    const float scale = 0.0625f / 327.68f * luminance_factor;
    auto contrast_at = [&](int j, int i) {
        const float *p = L + (size_t)j * W + i;
        return sqrtf(SQR(p[1] - p[-1]) + SQR(p[W] - p[-W]) + SQR(p[2] - p[-2]) + SQR(p[2 * W] - p[-2 * W])) * scale;
    };
    for (int j = 2; j < H - 2; ++j) {
        int i = 2;
        for (; i < W - 5; i += 4)
            for (int k = 0; k < 4; ++k) blend[(size_t)j * W + i + k] = 1.f * (1.f / (1.f + oracle_xexpf_v(16.f - 16.f * contrast_at(j, i + k) / thr)));
        for (; i < W - 2; ++i) blend[(size_t)j * W + i] = 1.f * (1.f / (1.f + oracle_xexpf_s(16.f - 16.f * contrast_at(j, i) / thr)));
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

// mode: 0 RGB, 1 LAB.  r, g, b: contiguous W x H planes.  Lmask / abmask: n planes of W x H floats each, or null.  always_ll != 0: build the
// lightness-detail plane whenever Lmask is asked for, as the reference does (the default builds it only when a lightness curve reads it).
// Returns 0, -1 (bad argument) or -4 (not on the device path: deltaE, drawn, external, linked masks, a mask curve, show_mask, YUV / XYZ).
int mk_ref_generate(const float *r, const float *g, const float *b, int W, int H, int mode, const double *ws, const mk_ref_mask *masks, int n,
                    int full_width, int full_height, double scale, float *Lmask, float *abmask, int always_ll, mk_ref_info *info, mk_ref_counts *cn)
{
    mk_ref_counts local;
    if (!cn) cn = &local;
    std::memset(cn, 0, sizeof *cn);
    if (!r || !g || !b || W < 1 || H < 1 || !masks || n < 1 || n > MK_REF_MAX_REGIONS || !(scale > 0.0) || (!Lmask && !abmask)) return -1;
    if (mode == 2 || mode == 3) return -4;
    if (mode != 0 && mode != 1) return -1;
    if (mode == 0 && !ws) return -1;
    for (int i = 0; i < n; ++i) {
        const mk_ref_mask &m = masks[i];
        if (m.deltae_enabled || m.drawn_enabled || m.external_enabled || m.linked_enabled || !m.curve_is_identity || m.show_mask) return -4;
        if (m.posterization < 0) return -1;
    }
    const size_t np = (size_t)W * H;
    float wp[9] = {};
    if (mode == 0) for (int k = 0; k < 9; ++k) wp[k] = (float)ws[k];
    auto lab = [&](size_t k, float &l, float &a, float &bb) {
        if (mode == 1) { l = g[k]; a = r[k]; bb = b[k]; }
        else oracle_rgb2lab(r[k], g[k], b[k], &l, &a, &bb, wp);
    };

    // which curves exist (L1059-1084)
    std::vector<void *> hm(n, nullptr), cm(n, nullptr), lm(n, nullptr);
    std::vector<float> ldetail(n, 0.f);
    bool has_mask = false, any_light = false;
    for (int i = 0; i < n; ++i) {
        const mk_ref_mask &m = masks[i];
        if (curve_present(m, m.hue, m.nhue, DEFAULT_HUE)) { hm[i] = oracle_flat_curve_new(m.hue, m.nhue, 1, 1000, 0.5); has_mask = true; }
        if (curve_present(m, m.chromaticity, m.nchromaticity, DEFAULT_CL)) { cm[i] = oracle_flat_curve_new(m.chromaticity, m.nchromaticity, 0, 1000, 0.5); has_mask = true; }
        if (curve_present(m, m.lightness, m.nlightness, DEFAULT_CL)) {
            lm[i] = oracle_flat_curve_new(m.lightness, m.nlightness, 0, 1000, 0.5);
            has_mask = true; any_light = true;
            ldetail[i] = LIM01(float(m.lightness_detail) / 100.f);
        }
        if (m.opacity < 100) has_mask = true;
    }
    const bool has_lmask = Lmask != nullptr;
    const bool build_ll = has_lmask && (any_light || always_ll);

    std::vector<float> guide(np), LL;
    int ll_r_small = 0, ll_r = 0;
    if (build_ll) {                                                     // L1113-1137
        ++cn->ll_built;
        LL.resize(np);
        for (size_t k = 0; k < np; ++k) {
            float l, a, bb;
            lab(k, l, a, bb);
            l /= 32768.f;
            guide[k] = l;
            LL[k] = std::round(l * 40.f) / 40.f;
        }
        const float radius = std::max(std::max(full_width, W), std::max(full_height, H)) / 30.f;
        ll_r = (int)radius;
        ll_r_small = (int)(10.f / scale);
        if (ll_r_small > 0) oracle_guided_filter(guide.data(), guide.data(), guide.data(), W, H, ll_r_small, 0.01f, 0);
        oracle_guided_filter(guide.data(), LL.data(), LL.data(), W, H, ll_r, 0.001f, 0);
    }

    const float c_factor = 327.68f * (42000.f / 48000.f);
    for (size_t k = 0; k < np; ++k) {                                   // L1171-1241
        float l, a, bb;
        lab(k, l, a, bb);
        l /= 32768.f; a /= 42000.f; bb /= 42000.f;
        guide[k] = LIM01(l);
        if (l < 0.f) ++cn->guide_low;
        if (l > 1.f) ++cn->guide_high;
        if (!has_mask) continue;
        float c = sqrtf(a * a + bb * bb) / 327.68f;
        float h = oracle_xatan2f(bb, a);
        c *= c_factor;
        c = oracle_xlin2log(c, 50.f);
        h = (float)hue_remap(h, cn);
        h += 1.f / 6.f;
        if (h > 1.f) { h -= 1.f; ++cn->hue_wraps; }
        h = oracle_xlin2log(h, 3.f);
        for (int i = 0; i < n; ++i) {
            // the reference: ll = has_lmask ? intp(ldetail, LL, l) : l, read by the lightness curve only
            float ll = l;
            if (has_lmask && (lm[i] || always_ll)) { ll = intp(ldetail[i], LL[k], l); if (lm[i]) ++cn->ll_read; }
            double v = (double)1.f;
            void *const cv[3] = {hm[i], cm[i], lm[i]};
            const double at[3] = {(double)h, (double)c, (double)ll};
            for (int q = 0; q < 3; ++q) {
                if (!cv[q]) { v = v * (double)1.f; continue; }
                v = v * oracle_flat_curve_get(cv[q], at[q]);
                ++cn->curve_evals[i][q];
                if (oracle_flat_curve_is_identity(cv[q])) ++cn->curve_identity;
            }
            const float blend = (float)v;
            if (Lmask) Lmask[(size_t)i * np + k] = blend;
            if (abmask) abmask[(size_t)i * np + k] = blend;
        }
    }
    for (int i = 0; i < n; ++i)
        for (void *cv : {hm[i], cm[i], lm[i]})
            if (cv) oracle_flat_curve_free(cv);

    float *sets[2] = {abmask, Lmask};
    if (full_width < 0) full_width = W;
    if (full_height < 0) full_height = H;
    std::vector<float> amask, thr;
    for (int i = 0; i < n; ++i) {
        const mk_ref_mask &m = masks[i];
        mk_ref_info inf = {};
        inf.has_mask = has_mask; inf.has_lmask = has_lmask && any_light; inf.smoothing_radius = -1;
        if (inf.has_lmask) { inf.ll_radius_small = ll_r_small; inf.ll_radius = ll_r; }
        if (has_mask) {                                                 // L1244-1295
            float blur = m.parametric_enabled ? (float)m.blur : 0.f;
            if (blur > -10.f) {
                blur = blur < 0.f ? -1.f / blur : 1.f + blur;
                const int r1 = std::max(int(4 / scale * blur + 0.5), 1), r2 = std::max(int(25 / scale * blur + 0.5), 1);
                inf.blurred = 1; inf.r1 = r1; inf.r2 = r2;
                ++cn->blurred_regions;
                if (abmask) oracle_guided_filter(guide.data(), abmask + (size_t)i * np, abmask + (size_t)i * np, W, H, r1, 0.001f, 0);
                if (Lmask) oracle_guided_filter(guide.data(), Lmask + (size_t)i * np, Lmask + (size_t)i * np, W, H, r2, 0.0001f, 0);
            }
            for (float *set : sets) {
                if (!set) continue;
                float *p = set + (size_t)i * np;
                for (size_t k = 0; k < np; ++k) {
                    if (p[k] < 0.f) ++cn->clamp_low;
                    if (p[k] > 1.f) ++cn->clamp_high;
                    p[k] = LIM01(p[k]);
                }
            }
        } else {
            for (float *set : sets)
                if (set) { std::fill(set + (size_t)i * np, set + (size_t)(i + 1) * np, 1.f); ++cn->filled_planes; }
        }
        if (m.parametric_enabled && m.contrast_threshold != 0) {        // contrast_threshold_mask (L696-734)
            amask.assign(np, 0.f);
            float fscale = (float)scale;
            const float s = float(std::max(W, H)) / 1920.f;
            int ww = W, hh = H;
            std::vector<float> tmpsrc, tmpdst;
            const float *src = guide.data();
            float *dst = amask.data();
            if (s > 1.f) {
                fscale *= s;
                ww = W / s; hh = H / s;
                tmpsrc.resize((size_t)ww * hh); tmpdst.resize((size_t)ww * hh);
                oracle_rescale_bilinear(guide.data(), W, H, tmpsrc.data(), ww, hh);
                src = tmpsrc.data(); dst = tmpdst.data();
                ++cn->cthr_rescaled;
            } else {
                ++cn->cthr_plain;
            }
            const float s_scale = std::sqrt(fscale);
            const float thresh = float(std::abs(m.contrast_threshold)) / 100.f * s_scale;
            const float bl = std::max(m.blur, 2.0) / s_scale;
            blend_mask(src, dst, ww, hh, thresh, bl, 32768.f);
            if (dst != amask.data()) oracle_rescale_bilinear(dst, ww, hh, amask.data(), W, H);
            inf.cthr_w = ww; inf.cthr_h = hh;
            const bool neg = m.contrast_threshold < 0;
            if (neg) ++cn->cthr_negative;
            for (float *set : sets) {
                if (!set) continue;
                float *p = set + (size_t)i * np;
                for (size_t k = 0; k < np; ++k) { const float f = neg ? 1.f - amask[k] : amask[k]; p[k] *= f; }
            }
        }
        if (m.area)                                                     // generate_area_mask's plane (L1380-1393)
            for (float *set : sets) {
                if (!set) continue;
                float *p = set + (size_t)i * np;
                for (size_t k = 0; k < np; ++k) p[k] *= m.area[k];
                cn->area_pixels += (long long)np;
            }
        for (float *set : sets) {                                       // mask_postprocess (L737-802) with an identity curve
            if (!set || !m.posterization) continue;
            float *p = set + (size_t)i * np;
            static const float pp[] = {30.f, 20.f, 10.f, 5.f, 3.f, 2.f};
            const float pv = pp[LIMi(m.posterization, 0, 6) - 1];
            for (size_t k = 0; k < np; ++k) {
                const int lv = int(p[k] * pv + 0.5);
                if (lv >= 0 && lv <= 30) ++cn->poster_level[lv];
                p[k] = lv / pv;
            }
            if (m.smoothing) {
                const float radius_coeff = 10.f * (101.f - float(LIMi(m.smoothing, 0, 100)));
                const float radius = std::max(full_width, full_height) / radius_coeff;
                const float lo = 0.0f, hi = 0.25f;
                const float f = LIM01(float(m.smoothing) / 100.f);
                const float f2 = std::max(f - lo, 0.f) / (hi - lo);
                const float fillval = LIM01((f < lo ? 0.f : (f > hi ? 1.f : (f2 < 0.5f ? 2.f * SQR(f2) : 1.f - 2.f * SQR(1.f - f2)))));
                thr.resize(np);
                for (size_t k = 0; k < np; ++k) {
                    const bool one = p[k] > 1e-4f;
                    thr[k] = one ? 1.f : fillval;
                    ++(one ? cn->thr_one : cn->thr_fill);
                }
                inf.smoothing_radius = (int)radius;
                oracle_guided_filter(guide.data(), p, p, W, H, (int)radius, 0.015f, 0);
                for (size_t k = 0; k < np; ++k) p[k] *= thr[k];
            }
        }
        if (m.inverted)
            for (float *set : sets) {
                if (!set) continue;
                float *p = set + (size_t)i * np;
                for (size_t k = 0; k < np; ++k) p[k] = 1.f - p[k];
                ++cn->inverted_planes;
            }
        if (m.opacity < 100) {
            const float ob = LIM01(float(m.opacity) / 100.f);
            for (float *set : sets) {
                if (!set) continue;
                float *p = set + (size_t)i * np;
                for (size_t k = 0; k < np; ++k) p[k] *= ob;
                ++cn->opacity_planes;
            }
        }
        if (info) info[i] = inf;
    }
    return 0;
}

} // extern "C"
