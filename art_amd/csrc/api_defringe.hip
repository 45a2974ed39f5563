// art_amd/csrc/api_defringe.hip -- ImProcFunctions::defringe behind the C ABI: the gates, the derived parameters and every refusal, the two blurs in
// the form gaussianBlur(src != dst, GAUSS_STANDARD) takes for the radius, and PF_correct_RT between the two mode switches.  The kernels are
// defringe.hip's; nothing travels through the host between them.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace {

constexpr size_t DF_STATE_BYTES = 64;        // P_DF_STATE: the DfState, the hue curve's polyline (DF_CURVE_LDS_BYTES), the sum's partials
static_assert(sizeof(DfState) <= DF_STATE_BYTES, "the state block");

} // namespace

namespace artgpu { namespace api {

int df_plan(artgpu_ctx *ctx, int W, int H, const artgpu_defringe_params *p, double scale, const char *who, DfPlan *pl)
{
    *pl = DfPlan{};
    pl->thresh = p->threshold;
    if (!p->enabled) { pl->early = 1; return ARTGPU_OK; }
    if (W < 8 || H < 8) { pl->early = 2; return ARTGPU_OK; }
    if (!(scale > 0.0) || std::isinf(scale)) return fail(ctx, ARTGPU_EINVAL, "%s: scale must be positive", who);
    if (p->nhuecurve < 0 || (p->nhuecurve > 0 && !p->huecurve)) return fail(ctx, ARTGPU_EINVAL, "%s: bad hue curve", who);
    if (p->radius < 0.0) return fail(ctx, ARTGPU_EINVAL, "%s: negative radius %g", who, p->radius);
    const double radius = p->radius / scale;
    if (!std::isfinite(radius) || radius >= 25.0) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: radius %g (scale %g) is not finite or not below 25", who, radius, scale);
    pl->radius = radius;
    pl->halfwin = std::ceil(2 * radius) + 1;
    if (pl->halfwin > DF_MAX_HALFWIN)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: radius %g at scale %g needs a window of %d, the averaging kernel holds %d (radius / scale <= %d)", who, p->radius,
                    scale, 2 * pl->halfwin - 1, 2 * DF_MAX_HALFWIN - 1, DF_MAX_HALO / 2);
    if (W < 2 * pl->halfwin - 2)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: width %d below %d: the reference's first column loop then reads past the row", who, W, 2 * pl->halfwin - 2);
    if ((long long)W * H > 0x7fffffffll) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: more than 2^31 - 1 pixels", who);
    if (radius < 0.25) pl->blur = DF_BLUR_COPY;
    else if (radius < 0.6) {
        pl->blur = DF_BLUR_3X3;
        const double sigma = radius;
        double c0 = 1.0, c1 = exp(-0.5 * ((1.0 / sigma) * (1.0 / sigma))), c2 = exp(-((1.0 / sigma) * (1.0 / sigma)));
        const double sum = c0 + 4.0 * (c1 + c2);
        c0 /= sum; c1 /= sum; c2 /= sum;
        double b1 = exp(-1.0 / (2.0 * sigma * sigma));
        const double bsum = 2.0 * b1 + 1.0;
        b1 /= bsum;
        const double b0 = 1.0 / bsum;
        pl->c0 = c0; pl->c1 = c1; pl->c2 = c2; pl->b0 = b0; pl->b1 = b1;
    } else pl->blur = DF_BLUR_YVV;
    if (p->nhuecurve > 0 && int(p->huecurve[0]) > 0 /* FCT_Linear */) {
        std::vector<double> x, y, sl;
        if (flat_curve_polyline(p->huecurve, p->nhuecurve, true, 1000 /* CURVES_MIN_POLY_POINTS */, 0.5, x, y, sl)) {
            pl->curve_n = (int)x.size();
            pl->tab = x;
            pl->tab.insert(pl->tab.end(), y.begin(), y.end());
            pl->tab.insert(pl->tab.end(), sl.begin(), sl.end());
            if (pl->tab.size() * sizeof(double) > (size_t)DF_CURVE_LDS_BYTES)
                return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: the hue curve's polyline (%zu bytes) does not fit LDS", who, pl->tab.size() * 8);
        } else pl->curve_n = -1;
    }
    return ARTGPU_OK;
}

int defringe_dev(artgpu_ctx *ctx, const DevRGB &d, const DfPlan &pl, const double ws[9], const double *iws, int already_lab, int to_rgb,
                 artgpu_defringe_info *info)
{
    const int W = d.w, H = d.h;
    const size_t n = (size_t)W * H, rowb = (size_t)W * 4;
    const int nchunk = (int)((n + DF_CHUNK - 1) / DF_CHUNK);
    float *sp, *stf;
    int rc;
    if ((rc = pool_get(ctx, P_SH_PLANES, 4 * n * 4, &sp)) || (rc = pool_get(ctx, P_DF_STATE, DF_STATE_BYTES + DF_CURVE_LDS_BYTES + (size_t)nchunk * 8, &stf))) return rc;
    float *tmpa = sp, *tmpb = sp + n, *fringe = sp + 2 * n, *gtmp = sp + 3 * n;
    DfState *st = reinterpret_cast<DfState *>(stf);
    double *curve = reinterpret_cast<double *>(reinterpret_cast<char *>(stf) + DF_STATE_BYTES), *partial = curve + DF_CURVE_LDS_BYTES / 8;
    if (pl.curve_n > 0 && (rc = h2d_table(ctx, curve, pl.tab.data(), pl.tab.size() * 8))) return rc;
    if (!already_lab && (rc = lab_switch_dev(ctx, d, ws, true))) return rc;
    const DfImage im = {d.p[0], d.p[2], d.stride, W, H};
    // gaussianBlur(lab->r.ptrs, tmpa, ..) / (lab->b.ptrs, tmpb, ..) (L66-67)
    float *const src[2] = {im.a, im.b}, *const dst[2] = {tmpa, tmpb};
    for (int k = 0; k < 2; ++k) {
        if (pl.blur == DF_BLUR_3X3) {
            HIPCHK(ctx, launch_df_gauss3x3(src[k], d.stride, dst[k], W, H, pl.c0, pl.c1, pl.c2, pl.b0, pl.b1, ctx->stream));
        } else {
            HIPCHK(ctx, hipMemcpy2DAsync(dst[k], rowb, src[k], d.stride * 4, rowb, H, hipMemcpyDeviceToDevice, ctx->stream));
            if (pl.blur == DF_BLUR_YVV && (rc = gaussian_dev(ctx, dst[k], gtmp, W, H, pl.radius))) return rc;
        }
    }
    const DfChromaArgs ca = {im, tmpa, tmpb, fringe, partial, curve, pl.curve_n};
    HIPCHK(ctx, launch_df_chroma(ca, ctx->stream));
    HIPCHK(ctx, launch_df_finish(partial, nchunk, W, H, pl.thresh, st, ctx->stream));
    const DfAverageArgs aa = {im, fringe, tmpa, tmpb, pl.halfwin, st};
    HIPCHK(ctx, launch_df_average(aa, ctx->stream));
    HIPCHK(ctx, launch_df_scatter(aa, ctx->stream));
    if (to_rgb && (rc = lab_switch_dev(ctx, d, iws, false))) return rc;
    if (info) {
        DfState host = {};
        HIPCHK(ctx, hipMemcpyAsync(&host, st, sizeof host, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        info->chromave = host.chromave; info->threshfactor = host.threshfactor; info->corrected_pixels = (int64_t)host.corrected;
    }
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_defringe(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_defringe_params *params, const double *ws, const double *iws, double scale, int from_lab,
                    int to_rgb, artgpu_defringe_info *info)
{
    StageScope scope_(ctx, "ImProcFunctions::defringe");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !params || (!from_lab && !ws) || (to_rgb && !iws)) return fail(ctx, ARTGPU_EINVAL, "defringe: null argument");
    if (info) *info = artgpu_defringe_info{};
    if (!plane_ok(&img->r)) return fail(ctx, ARTGPU_EINVAL, "defringe: bad plane");
    DfPlan pl;
    int rc;
    if ((rc = df_plan(ctx, img->r.w, img->r.h, params, scale, "defringe", &pl))) return rc;
    if (info) { info->early_out = pl.early; info->halfwin = pl.halfwin; info->blur = pl.blur; info->curve = pl.curve_n > 0 ? 1 : pl.curve_n; info->radius = pl.radius; }
    if (pl.early) return ARTGPU_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "defringe"))) return rc;
    if ((rc = defringe_dev(ctx, d, pl, ws, iws, from_lab, to_rgb, info))) return rc;
    return unbind_rgb(ctx, img, &d);
}

} // extern "C"
