// art_amd/csrc/api_toneequalizer.hip -- ImProcFunctions::toneEqualizer (rtengine/iptoneequalizer.cc:345-371, tone_eq L69-340) behind the C ABI:
// the plan, the table, the launch sequence.  The kernels are toneequalizer.hip's and, for everything with a window, the guided filter's.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace {

// one rtengine::guidedFilter call of the tool as guided_filter_stats will run it: calculate_subsampling, the statistics grid, f_mean's radius
int te_plan_filter(artgpu_ctx *ctx, int W, int H, int k, int r, float epsilon, const char *who, artgpu_tone_equalizer_info *pl)
{
    static const char *const name[3] = {"detail filter", "first regularising filter", "second regularising filter"};
    if (r <= 0) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: the %s would run with radius %d", who, name[k], r);
    const GfGrid grid = gf_grid(W, H, r);
    const int sub = grid.sub, w = grid.w, h = grid.h, rad = grid.rad;
    if (w < ARTGPU_SMOOTHING_MIN_SIZE || h < ARTGPU_SMOOTHING_MIN_SIZE)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: the %s of a %dx%d image has a %dx%d statistics grid, below %d", who, name[k], W, H, w, h, ARTGPU_SMOOTHING_MIN_SIZE);
    if (rad > HBLUR_MAX_RADIUS)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: the %s: box radius %d (radius %d / subsampling %d) is above the %d the blur kernels hold in LDS", who, name[k], rad, r, sub, HBLUR_MAX_RADIUS);
    pl->radius[k] = r; pl->subsampling[k] = sub; pl->box_radius[k] = rad; pl->epsilon[k] = epsilon;
    ++pl->filters;
    return ARTGPU_OK;
}

// the correction table on the device: built when the bands change, uploaded when it is not where it was
int te_table(artgpu_ctx *ctx, const artgpu_tone_equalizer_params *p, const float **out)
{
    float *dev;
    int rc;
    if ((rc = pool_get(ctx, P_TE_LUT, 65536 * 4, &dev))) return rc;
    const bool same = ctx->te_lut_host.size() == 65536 && std::equal(p->bands, p->bands + 5, ctx->te_lut_bands);
    if (!same) {
        artgpu_tone_equalizer_info i;
        ctx->te_lut_host.resize(65536);
        te_build_lut(p->bands, p->pivot, ctx->te_lut_host.data(), &i.gain, &i.w_sum, i.factors);
        std::copy(p->bands, p->bands + 5, ctx->te_lut_bands);
    }
    if (!same || ctx->te_lut_dev != dev) {
        ctx->te_lut_dev = nullptr;
        if ((rc = h2d_table(ctx, dev, ctx->te_lut_host.data(), 65536 * 4))) return rc;
        ctx->te_lut_dev = dev;
    }
    *out = dev;
    return ARTGPU_OK;
}

} // namespace

namespace artgpu { namespace api {

// every reason not to run, and what the call derives (L127-129, L150-157, L354): nothing is launched
int te_check(artgpu_ctx *ctx, int W, int H, const artgpu_tone_equalizer_params *p, const double *ws, double scale, const char *who, artgpu_tone_equalizer_info *pl)
{
    if (!p || !ws || W < 1 || H < 1 || std::isnan(scale)) return fail(ctx, ARTGPU_EINVAL, "%s: bad arguments", who);
    *pl = artgpu_tone_equalizer_info{};
    if (p->show_colormap) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: show_colormap is not on the device path (PREVIEW pipeline, lcms2)", who);
    if (p->regularization < 0 || p->regularization > 4) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: regularization %d is outside 0 .. 4", who, p->regularization);
    if (!(scale >= 1.0) || std::isinf(scale)) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: scale %g (below 1) is not on the device path", who, scale);
    te_build_lut(p->bands, p->pivot, nullptr, &pl->gain, &pl->w_sum, pl->factors);
    if (p->regularization == 0) return ARTGPU_OK;
    int rc;
    const int detail = 5;
    const int radius = float(detail) / scale + 0.5f;                    // L128 (double arithmetic, truncated)
    const float epsilon = 0.01f + 0.002f * std::max(detail - 3, 0);     // L129
    if (radius > 0 && (rc = te_plan_filter(ctx, W, H, 0, radius, epsilon, who, pl))) return rc;
    if (p->regularization > 1) {
        constexpr float base_epsilon = 0.004f;
        const int r = 350.f / scale;                                    // L150
        if ((rc = te_plan_filter(ctx, W, H, 1, r, base_epsilon, who, pl))) return rc;
        const int reg = 5 - std::min(p->regularization, 4);
        if (reg > 1 && (rc = te_plan_filter(ctx, W, H, 2, r * (reg - 1), base_epsilon / 100, who, pl))) return rc;
    }
    return ARTGPU_OK;
}

// the tool on device planes (rows of `stride` floats) in RGB mode, after te_check; enqueued on ctx->stream
int tone_equalizer_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const artgpu_tone_equalizer_params *p, const double ws[9],
                       const artgpu_tone_equalizer_info &pl, const char *who)
{
    int rc;
    TeArgs a = {};
    for (int k = 0; k < 3; ++k) { a.img[k] = planes[k]; a.ws1[k] = ws[3 + k]; }
    a.stride = stride; a.W = W; a.H = H;
    a.gain = pl.gain; a.igain = 1.f / pl.gain; a.w_sum = pl.w_sum;
    for (int k = 0; k < 12; ++k) a.factors[k] = pl.factors[k];
    a.group_thread = ctx->shared.opt_te_group_thread;
    if ((rc = te_table(ctx, p, &a.lut))) return rc;
    const bool detail = pl.radius[0] > 0, post = p->regularization > 1;
    if (!detail && !post) {                                             // regularization 0 (or 1 at a scale that leaves no detail radius): Y stays in registers
        HIPCHK(ctx, launch_te_direct(a, ctx->stream));
        return ARTGPU_OK;
    }
    const size_t n = (size_t)W * H;
    float *big;
    if ((rc = pool_get(ctx, P_TE_PLANES, (post ? 2 : 1) * n * 4, &big))) return rc;
    a.Y = big; a.Y2 = post ? big + n : nullptr;
    a.mode = detail ? TE_PREP_LOG : TE_PREP_POSTERISE;
    HIPCHK(ctx, launch_te_prepare(a, ctx->stream));
    if (detail) {       // guidedFilterLog(10.f, Y, radius, epsilon): self-guided, so the plain statistics with guide == src
        GuidedArgs g;
        if ((rc = guided_filter_stats(ctx, a.Y, a.Y, W, H, pl.radius[0], pl.epsilon[0], pl.subsampling[0], who, &g))) return rc;
        a.ma = g.low[2]; a.mb = g.low[5]; a.w = g.w; a.h = g.h; a.mode = post ? 1 : 0;
        HIPCHK(ctx, launch_te_detail_finish(a, ctx->stream));
    }
    // guidedFilter(Y2, Y, Y, ..) once or twice; the last one's pointwise pass moves into te_apply (option te_fuse_upsample), which then reads Y2
    // and the statistics grid instead of a Y plane that this filter would have to write first
    const int last = post ? (pl.radius[2] > 0 ? 2 : 1) : 0;
    for (int k = 1; k <= last; ++k) {
        if (k == last && ctx->shared.opt_te_fuse_upsample) {
            GuidedArgs g;
            if ((rc = guided_filter_stats(ctx, a.Y2, a.Y, W, H, pl.radius[k], pl.epsilon[k], pl.subsampling[k], who, &g))) return rc;
            a.ma = g.low[2]; a.mb = g.low[5]; a.w = g.w; a.h = g.h; a.upsample = 1;
        } else if ((rc = guided_filter_dev(ctx, a.Y2, a.Y, a.Y, (size_t)W, W, H, pl.radius[k], pl.epsilon[k], pl.subsampling[k], who))) return rc;
    }
    HIPCHK(ctx, launch_te_apply(a, ctx->stream));
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_tone_equalizer_lut(const artgpu_tone_equalizer_params *p, float *lut, artgpu_tone_equalizer_info *info)
{
    if (!p || (!lut && !info)) return ARTGPU_EINVAL;
    artgpu_tone_equalizer_info i = {};
    te_build_lut(p->bands, p->pivot, lut, &i.gain, &i.w_sum, i.factors);
    if (info) { info->gain = i.gain; info->w_sum = i.w_sum; std::copy(i.factors, i.factors + 12, info->factors); }
    return ARTGPU_OK;
}

int artgpu_tone_equalizer(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_tone_equalizer_params *p, const double ws[9], double scale, artgpu_tone_equalizer_info *info)
{
    StageScope scope_(ctx, "ImProcFunctions::toneEqualizer");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !plane_ok(&img->r) || !p) return fail(ctx, ARTGPU_EINVAL, "tone_equalizer: bad arguments");
    if (!p->enabled) return ARTGPU_OK;                                  // L347
    artgpu_tone_equalizer_info pl;
    int rc;
    if ((rc = te_check(ctx, img->r.w, img->r.h, p, ws, scale, "tone_equalizer", &pl))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "tone_equalizer"))) return rc;
    if ((rc = tone_equalizer_dev(ctx, d.p, d.stride, d.w, d.h, p, ws, pl, "tone_equalizer"))) return rc;
    if (info) *info = pl;
    return unbind_rgb(ctx, img, &d);
}

int artgpu_set_pipeline_tone_equalizer(artgpu_ctx *ctx, const artgpu_tone_equalizer_params *p)
{
    if (!ctx) return ARTGPU_EINVAL;
    ctx->shared.pipe_te_on = p != nullptr;
    ctx->shared.pipe_te = p ? *p : artgpu_tone_equalizer_params{};
    return ARTGPU_OK;
}

} // extern "C"
