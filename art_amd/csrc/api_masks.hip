// art_amd/csrc/api_masks.hip -- region masks behind the C ABI: rtengine::generateMasks, parametric path (masks.cc:1037-1516): the plan of everything
// it decides before its first pixel loop, and the passes on a device image.  The kernels are masks.hip's.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace {

// one rtengine::guidedFilter call as artgpu_guided_filter will run it: decided in the plan, so that nothing starts before everything fits
struct MkFilter { int on, r; };

// ParametricMask's default curves (procparams.cc:1014-1053)
const double MK_DEFAULT_HUE[9] = {1 /* FCT_MinMaxCPoints */, 0.166666667, 1., 0.35, 0.35, 0.8287775246, 1., 0.35, 0.35};
const double MK_DEFAULT_CL[9] = {1, 0., 1., 0.35, 0.35, 1., 1., 0.35, 0.35};

// L1068-1080: enabled, not empty, not FCT_Linear, not the default
bool mk_curve_present(const artgpu_mask_params &m, const double *pts, int n, const double *dflt)
{
    if (!m.parametric_enabled || !pts || n <= 0 || pts[0] == 0 /* FCT_Linear */) return false;
    return !(n == 9 && std::equal(pts, pts + 9, dflt));
}
int mk_filter_check(artgpu_ctx *ctx, int W, int H, int r, const char *who, const char *what)
{
    const GfGrid grid = gf_grid(W, H, r);
    const int sub = grid.sub, w = grid.w, h = grid.h, rad = grid.rad;
    if (w < 1 || h < 1) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: %s: a %dx%d image has a side shorter than the guided filter's subsampling %d", who, what, W, H, sub);
    if (rad > HBLUR_MAX_RADIUS) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: %s: box radius %d (radius %d / subsampling %d) is above the %d the blur kernels hold in LDS", who, what, rad, r, sub, HBLUR_MAX_RADIUS);
    return ARTGPU_OK;
}

} // namespace

namespace artgpu { namespace api {

// everything generateMasks decides before its first pixel loop, and every reason not to run
int mk_plan(artgpu_ctx *ctx, int W, int H, int mode, const double *ws, const artgpu_mask_params *masks, int n, int full_w, int full_h, double scale,
            bool want_L, bool want_ab, const char *who, MkPlan *pl, artgpu_masks_info *info)
{
    if (!masks || n <= 0 || !(scale > 0.0) || (!want_L && !want_ab)) return fail(ctx, ARTGPU_EINVAL, "%s: bad arguments", who);
    if (mode != ARTGPU_MASKS_MODE_RGB && mode != ARTGPU_MASKS_MODE_LAB) {
        if (mode == ARTGPU_MASKS_MODE_YUV || mode == ARTGPU_MASKS_MODE_XYZ) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: image mode %d (RGB and LAB are on the device path)", who, mode);
        return fail(ctx, ARTGPU_EINVAL, "%s: image mode %d", who, mode);
    }
    if (mode == ARTGPU_MASKS_MODE_RGB && !ws) return fail(ctx, ARTGPU_EINVAL, "%s: RGB mode needs the working-space matrix", who);
    if (W < ARTGPU_MASKS_MIN_SIZE || H < ARTGPU_MASKS_MIN_SIZE)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: %dx%d is below %dx%d", who, W, H, ARTGPU_MASKS_MIN_SIZE, ARTGPU_MASKS_MIN_SIZE);
    *pl = MkPlan{};
    pl->W = W; pl->H = H; pl->lab = mode == ARTGPU_MASKS_MODE_LAB; pl->want_L = want_L; pl->want_ab = want_ab;
    pl->reg.resize(n);
    bool any_light = false;
    int rc;
    for (int i = 0; i < n; ++i) {
        const artgpu_mask_params &m = masks[i];
        MkRegionPlan &r = pl->reg[i];
        if (m.deltae_enabled) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: the deltaE mask (cmsCIE2000DeltaE) is not on the device path", who, i);
        if (m.drawn_enabled || m.external_enabled || m.linked_enabled) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: drawn, external and linked masks are not on the device path", who, i);
        if (!m.curve_is_identity) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: a mask curve other than the identity is not on the device path", who, i);
        if (m.show_mask) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: show_mask is not on the device path", who, i);
        if (m.nhue < 0 || m.nchromaticity < 0 || m.nlightness < 0 || m.posterization < 0) return fail(ctx, ARTGPU_EINVAL, "%s: region %d: negative curve length or posterization", who, i);
        if (m.area && (!plane_ok(m.area) || m.area->w != W || m.area->h != H)) return fail(ctx, ARTGPU_EINVAL, "%s: the area plane of region %d must be a %dx%d plane", who, i, W, H);
        const double *pts[3] = {m.hue, m.chromaticity, m.lightness};
        const int npts[3] = {m.nhue, m.nchromaticity, m.nlightness};
        for (int k = 0; k < 3; ++k) {
            r.curve[k] = MkCurve{0, 0};
            if (!mk_curve_present(m, pts[k], npts[k], k == MK_HUE ? MK_DEFAULT_HUE : MK_DEFAULT_CL)) continue;
            pl->has_mask = 1;
            std::vector<double> x, y, sl;
            if (flat_curve_polyline(pts[k], npts[k], k == MK_HUE, 1000 /* CURVES_MIN_POLY_POINTS */, 0.5, x, y, sl)) {
                r.curve[k] = MkCurve{(int)r.tab.size(), (int)x.size()};
                r.tab.insert(r.tab.end(), x.begin(), x.end());
                r.tab.insert(r.tab.end(), y.begin(), y.end());
                r.tab.insert(r.tab.end(), sl.begin(), sl.end());
            } else {
                r.curve[k] = MkCurve{0, -1};        // FCT_Empty: getVal returns identityValue
            }
            if (k == MK_LIGHT) {
                any_light = true;
                const float d = float(m.lightness_detail) / 100.f;
                r.ldetail = d < 0.f ? 0.f : (d > 1.f ? 1.f : d);
            }
        }
        if (r.tab.size() * sizeof(double) > (size_t)MK_LDS_BYTES) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: the curves' polylines (%zu bytes) do not fit LDS", who, i, r.tab.size() * 8);
        if (m.opacity < 100) pl->has_mask = 1;
    }
    pl->need_ll = want_L && any_light;
    if (pl->need_ll) {
        const int m1 = full_w > W ? full_w : W, m2 = full_h > H ? full_h : H;
        const float radius = (m1 > m2 ? m1 : m2) / 30.f;
        pl->ll_r = (int)radius;
        pl->ll_r_small = (int)(10.f / scale);
        if (pl->ll_r_small > 0 && (rc = mk_filter_check(ctx, W, H, pl->ll_r_small, who, "lightness detail"))) return rc;
        if ((rc = mk_filter_check(ctx, W, H, pl->ll_r, who, "lightness detail"))) return rc;
    }
    if (full_w < 0) full_w = W;
    if (full_h < 0) full_h = H;
    pl->need_guide = pl->has_mask;
    for (int i = 0; i < n; ++i) {
        const artgpu_mask_params &m = masks[i];
        MkRegionPlan &r = pl->reg[i];
        float blur = m.parametric_enabled ? (float)m.blur : 0.f;
        if (pl->has_mask && blur > -10.f) {
            blur = blur < 0.f ? -1.f / blur : 1.f + blur;
            r.blurred = 1;
            r.r1 = std::max(int(4 / scale * blur + 0.5), 1);
            r.r2 = std::max(int(25 / scale * blur + 0.5), 1);
            if (want_ab && (rc = mk_filter_check(ctx, W, H, r.r1, who, "ab mask blur"))) return rc;
            if (want_L && (rc = mk_filter_check(ctx, W, H, r.r2, who, "L mask blur"))) return rc;
        }
        if (m.parametric_enabled && m.contrast_threshold != 0) {        // contrast_threshold_mask (L696-734)
            float fscale = (float)scale;
            const int d = std::max(W, H);
            const float s = float(d) / 1920.f;
            r.cthr = 1; r.cthr_neg = m.contrast_threshold < 0; r.cw = W; r.ch = H;
            if (s > 1.f) { fscale *= s; r.cw = W / s; r.ch = H / s; }
            const float s_scale = std::sqrt(fscale);
            r.cthr_thresh = float(std::abs(m.contrast_threshold)) / 100.f * s_scale;
            r.cthr_blur = std::max(m.blur, 2.0) / s_scale;
            if (r.cw < 8 || r.ch < 8) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: the contrast threshold's %dx%d plane is below 8x8", who, i, r.cw, r.ch);
            pl->need_guide = 1;
        }
        if (m.posterization) {                                          // mask_postprocess (L737-802)
            static const float pp[] = {30.f, 20.f, 10.f, 5.f, 3.f, 2.f};
            r.post_p = pp[std::min(std::max(m.posterization, 0), 6) - 1];
            if (m.smoothing) {
                const float radius_coeff = 10.f * (101.f - float(std::min(std::max(m.smoothing, 0), 100)));
                const float radius = std::max(full_w, full_h) / radius_coeff;
                r.smooth = 1; r.smooth_r = (int)radius;
                const float l = 0.0f, h = 0.25f;
                const float f0 = float(m.smoothing) / 100.f, f = f0 < 0.f ? 0.f : (f0 > 1.f ? 1.f : f0);
                const float f2 = std::max(f - l, 0.f) / (h - l);
                const float v = f < l ? 0.f : (f > h ? 1.f : (f2 < 0.5f ? 2.f * (f2 * f2) : 1.f - 2.f * ((1.f - f2) * (1.f - f2))));
                r.fillval = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
                if ((rc = mk_filter_check(ctx, W, H, r.smooth_r, who, "mask smoothing"))) return rc;
                pl->need_guide = 1;
            }
        }
        r.inverted = m.inverted ? 1 : 0;
        if (m.opacity < 100) {
            const float b = float(m.opacity) / 100.f;
            r.has_opacity = 1; r.opacity = b < 0.f ? 0.f : (b > 1.f ? 1.f : b);
        }
    }
    if (info)
        for (int i = 0; i < n; ++i) {
            const MkRegionPlan &r = pl->reg[i];
            info[i] = artgpu_masks_info{pl->has_mask, pl->need_ll, pl->need_ll ? pl->ll_r_small : 0, pl->need_ll ? pl->ll_r : 0, r.blurred, r.r1, r.r2,
                                        r.cthr ? r.cw : 0, r.cthr ? r.ch : 0, r.smooth ? r.smooth_r : -1};
        }
    return ARTGPU_OK;
}

// generateMasks on a device image (rows of `stride` floats), enqueued on ctx->stream.  Lout / about: n contiguous W x H device planes each,
// or nullptr.  `masks` is read for the area planes only.
int masks_dev(artgpu_ctx *ctx, float *const img[3], size_t stride, const double *ws, const artgpu_mask_params *masks, const MkPlan &pl,
              float *Lout, float *about)
{
    const int W = pl.W, H = pl.H, n = (int)pl.reg.size();
    const size_t np = (size_t)W * H;
    float *work, *cplanes = nullptr, *tabs = nullptr;
    int rc;
    // guide | LL | thr | one blend plane per region
    if ((rc = pool_get(ctx, P_MK_WORK, (size_t)(3 + (pl.has_mask ? n : 0)) * np * 4, &work))) return rc;
    float *guide = work, *LL = work + np, *thr = work + 2 * np, *blend = work + 3 * np;
    MkImage im = {{img[0], img[1], img[2]}, stride, W, H, pl.lab};
    float wp[9] = {};
    if (!pl.lab) {
        for (int k = 0; k < 9; ++k) wp[k] = (float)ws[k];
        if ((rc = lab_tabs_dev(ctx, &tabs))) return rc;
    }
    if (pl.need_ll) {                                                   // L1113-1137
        MkLLArgs a = {};
        a.im = im; std::copy(wp, wp + 9, a.wp); a.cachef = tabs; a.cachefy = tabs ? tabs + 65536 : nullptr; a.guide = guide; a.LL = LL;
        HIPCHK(ctx, launch_mk_ll(a, ctx->stream));
        if (pl.ll_r_small > 0 && (rc = guided_filter_dev(ctx, guide, guide, guide, W, W, H, pl.ll_r_small, 0.01f, 0, "generate_masks"))) return rc;
        if ((rc = guided_filter_dev(ctx, guide, LL, LL, W, W, H, pl.ll_r, 0.001f, 0, "generate_masks"))) return rc;
    }
    if (pl.need_guide) {                                                // L1171-1241, MK_GROUP regions (and MK_LDS_BYTES of polylines) per launch
        MkFusedArgs a = {};
        a.im = im; std::copy(wp, wp + 9, a.wp); a.cachef = tabs; a.cachefy = tabs ? tabs + 65536 : nullptr; a.guide = guide;
        a.LL = pl.need_ll ? LL : nullptr;
        if (!pl.has_mask) {
            HIPCHK(ctx, launch_mk_fused(a, ctx->stream));
        } else {
            size_t total = 0;
            for (const MkRegionPlan &r : pl.reg) total += r.tab.size();
            float *tabf;
            if ((rc = pool_get(ctx, P_MK_TAB, total * 8 + 64, &tabf))) return rc;
            double *dtab = reinterpret_cast<double *>(tabf);
            std::vector<double> host;
            host.reserve(total);
            for (const MkRegionPlan &r : pl.reg) host.insert(host.end(), r.tab.begin(), r.tab.end());
            if (total && (rc = h2d_table(ctx, dtab, host.data(), total * 8))) return rc;
            size_t base = 0;
            for (int i0 = 0; i0 < n;) {
                a.nreg = 0; a.tab = dtab + base; a.tab_len = 0;
                while (i0 + a.nreg < n && a.nreg < MK_GROUP) {
                    const MkRegionPlan &r = pl.reg[i0 + a.nreg];
                    if (a.nreg && ((size_t)a.tab_len + r.tab.size()) * 8 > (size_t)MK_LDS_BYTES) break;
                    for (int k = 0; k < 3; ++k) a.curve[a.nreg][k] = MkCurve{r.curve[k].off + a.tab_len, r.curve[k].n};
                    a.ldetail[a.nreg] = r.ldetail;
                    a.out[a.nreg] = blend + (size_t)(i0 + a.nreg) * np;
                    a.tab_len += (int)r.tab.size();
                    ++a.nreg;
                }
                HIPCHK(ctx, launch_mk_fused(a, ctx->stream));
                base += a.tab_len; i0 += a.nreg;
            }
        }
    }
    for (int i = 0; i < n; ++i) {
        const MkRegionPlan &r = pl.reg[i];
        const float *cthr = nullptr;
        if (r.cthr) {                                                   // contrast_threshold_mask (L696-734)
            const size_t ns = (size_t)r.cw * r.ch;
            if ((rc = pool_get(ctx, P_MK_CTHR, (np + 3 * ns) * 4, &cplanes))) return rc;
            float *full = cplanes, *src = cplanes + np, *dst = src + ns, *gtmp = dst + ns;
            const bool rescaled = r.cw != W || r.ch != H;
            if (rescaled) HIPCHK(ctx, launch_mk_rescale(guide, W, H, src, r.cw, r.ch, ctx->stream));
            DualArgs da = {};
            da.L = rescaled ? src : guide; da.blend = rescaled ? dst : full; da.w = r.cw; da.h = r.ch; da.threshold = r.cthr_thresh;
            HIPCHK(ctx, launch_blend_mask_lum(da, 32768.f, ctx->stream));
            if ((rc = gaussian_dev(ctx, da.blend, gtmp, r.cw, r.ch, (double)r.cthr_blur))) return rc;
            if (rescaled) HIPCHK(ctx, launch_mk_rescale(dst, r.cw, r.ch, full, W, H, ctx->stream));
            cthr = full;
        }
        const float *area = nullptr; size_t area_stride = 0;
        if ((rc = bind_plane(ctx, masks[i].area, P_MK_AREA, &area, &area_stride))) return rc;
        for (int which = 0; which < 2; ++which) {                       // abmask first, like L1264-1269
            float *out = which == 0 ? about : Lout;
            if (!out) continue;
            out += (size_t)i * np;
            if (pl.has_mask) {
                float *b = blend + (size_t)i * np;
                if (r.blurred) {
                    if ((rc = guided_filter_dev(ctx, guide, b, out, W, W, H, which == 0 ? r.r1 : r.r2, which == 0 ? 0.001f : 0.0001f, 0, "generate_masks"))) return rc;
                } else {
                    HIPCHK(ctx, hipMemcpyAsync(out, b, np * 4, hipMemcpyDeviceToDevice, ctx->stream));
                }
            }
            MkTailArgs t = {};
            t.m = out; t.w = W; t.h = H; t.fill_one = !pl.has_mask; t.clamp = pl.has_mask;
            t.cthr = cthr; t.cthr_neg = r.cthr_neg; t.area = area; t.area_stride = area_stride; t.post_p = r.post_p;
            if (r.smooth) { t.thr_out = thr; t.fillval = r.fillval; }
            else { t.inverted = r.inverted; t.has_opacity = r.has_opacity; t.opacity = r.opacity; }
            HIPCHK(ctx, launch_mk_tail(t, ctx->stream));
            if (r.smooth) {                                             // L772-799, then L1438-1467
                if ((rc = guided_filter_dev(ctx, guide, out, out, W, W, H, r.smooth_r, 0.015f, 0, "generate_masks"))) return rc;
                MkTailArgs t2 = {};
                t2.m = out; t2.w = W; t2.h = H; t2.thr_in = thr; t2.inverted = r.inverted; t2.has_opacity = r.has_opacity; t2.opacity = r.opacity;
                HIPCHK(ctx, launch_mk_tail(t2, ctx->stream));
            }
        }
    }
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_generate_masks(artgpu_ctx *ctx, const artgpu_rgb *img, int mode, const double ws[9], const artgpu_mask_params *masks, int n,
                          int full_w, int full_h, double scale, artgpu_plane *Lmask, artgpu_plane *abmask, artgpu_masks_info *info)
{
    StageScope scope_(ctx, "generateMasks");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !plane_ok(&img->r)) return fail(ctx, ARTGPU_EINVAL, "generate_masks: bad image");
    const int W = img->r.w, H = img->r.h;
    MkPlan pl;
    int rc;
    if ((rc = mk_plan(ctx, W, H, mode, ws, masks, n, full_w, full_h, scale, Lmask != nullptr, abmask != nullptr, "generate_masks", &pl, info))) return rc;
    for (artgpu_plane *set : {Lmask, abmask})
        for (int i = 0; set && i < n; ++i)
            if (!plane_ok(&set[i]) || set[i].w != W || set[i].h != H) return fail(ctx, ARTGPU_EINVAL, "generate_masks: output plane %d must be a %dx%d plane", i, W, H);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "generate_masks"))) return rc;
    const size_t np = (size_t)W * H;
    float *outs;
    if ((rc = pool_get(ctx, P_MK_OUT, (size_t)n * np * 4 * ((Lmask ? 1 : 0) + (abmask ? 1 : 0)), &outs))) return rc;
    float *Lout = Lmask ? outs : nullptr, *about = abmask ? outs + (Lmask ? (size_t)n * np : 0) : nullptr;
    if ((rc = masks_dev(ctx, d.p, d.stride, ws, masks, pl, Lout, about))) return rc;
    for (int i = 0; i < n; ++i) {
        if (Lmask && (rc = pool_to_plane(ctx, Lout + (size_t)i * np, &Lmask[i]))) return rc;
        if (abmask && (rc = pool_to_plane(ctx, about + (size_t)i * np, &abmask[i]))) return rc;
    }
    return ARTGPU_OK;
}

} // extern "C"
