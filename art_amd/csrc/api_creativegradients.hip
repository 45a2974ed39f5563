// art_amd/csrc/api_creativegradients.hip -- ImProcFunctions::creativeGradients (rtengine/iptransform.cc:1390-1408) behind the C ABI: which of
// the two filters run, the geometry, the derived parameters (hostluts.hip's cg_gradient_params / cg_pcvignette_params), the launch.  The kernel
// is creativegradients.hip's.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

static_assert(sizeof(CgDerived) == sizeof(artgpu_creative_gradient_derived), "CgDerived is the layout of artgpu_creative_gradient_derived");

namespace {

// the reference squares pixel distances and sizes in int (L855, L883, L920): with every coordinate below 2^15 the sums stay below 2^31
constexpr int CG_MAX_COORD = 32767;

// needsGradient / needsPCVignetting (L1354-1362), the geometry of creativeGradients (L1394-1405), the two derivations
void cg_derive(const artgpu_creative_gradients_params *p, int w, int h, CgDerived *d)
{
    *d = CgDerived{};
    const bool grad = p->gradient_enabled && std::fabs(p->gradient_strength) > 1e-15;
    const bool pcv = p->pcvignette_enabled && std::fabs(p->pcvignette_strength) > 1e-15;
    d->cx = p->offset_x; d->cy = p->offset_y;
    int cw, ch;
    if (p->full_width < 0) { cw = w; ch = h; }
    else { cw = p->full_width; ch = p->full_height; }
    const int fw = cw * p->scale;
    const int fh = ch * p->scale;
    CgInput in = {};
    in.degree = p->gradient_degree; in.strength = p->gradient_strength; in.feather = p->gradient_feather;
    in.center_x = p->gradient_center_x; in.center_y = p->gradient_center_y;
    in.pcv_strength = p->pcvignette_strength; in.pcv_feather = p->pcvignette_feather; in.pcv_roundness = p->pcvignette_roundness;
    in.pcv_center_x = p->pcvignette_center_x; in.pcv_center_y = p->pcvignette_center_y;
    in.crop_enabled = p->crop_enabled; in.crop_x = p->crop_x; in.crop_y = p->crop_y; in.crop_w = p->crop_w; in.crop_h = p->crop_h;
    if (grad) { cg_gradient_params(cw, ch, in, d); d->apply_gradient = 1; }
    if (pcv) { cg_pcvignette_params(fw, fh, cw, ch, in, d); d->apply_pcvignette = 1; }
}

// what is malformed (0 = fine, 1 = EINVAL, 2 = EUNSUPPORTED), for the C entry that has no context to report to as well
int cg_refusal(const artgpu_creative_gradients_params *p, int w, int h, const char **why)
{
    *why = "bad arguments";
    if (!p || w < 1 || h < 1) return 1;
    if (!std::isfinite(p->gradient_degree) || !std::isfinite(p->gradient_strength) || !std::isfinite(p->pcvignette_strength) || !std::isfinite(p->scale) || !(p->scale > 0.0)) return 1;
    if (p->full_width >= 0 && (p->full_width < 1 || p->full_height < 1)) return 1;
    const bool pcv = p->pcvignette_enabled && std::fabs(p->pcvignette_strength) > 1e-15;
    if (pcv && p->crop_enabled && (p->crop_w < 1 || p->crop_h < 1 || p->crop_x < 0 || p->crop_y < 0)) return 1;
    *why = "a feather or roundness outside 0 .. 100 (the super-ellipse degree would leave 2 .. 8)";
    if (pcv && (p->pcvignette_roundness < 0 || p->pcvignette_roundness > 100 || p->pcvignette_feather < 0 || p->pcvignette_feather > 100)) return 2;
    if (p->gradient_feather < 0 || p->gradient_feather > 100) return 2;
    *why = "a size, offset or crop beyond 32767 (the reference squares them in int)";
    const int cw = p->full_width < 0 ? w : p->full_width, ch = p->full_width < 0 ? h : p->full_height;
    const double fw = cw * p->scale, fh = ch * p->scale;
    if (cw > CG_MAX_COORD || ch > CG_MAX_COORD || fw > CG_MAX_COORD || fh > CG_MAX_COORD || fw < 1.0 || fh < 1.0 || p->offset_x < 0 || p->offset_y < 0 ||
        (long long)p->offset_x + w > CG_MAX_COORD || (long long)p->offset_y + h > CG_MAX_COORD)
        return 2;
    if (pcv && p->crop_enabled && ((long long)p->crop_x + p->crop_w > CG_MAX_COORD || (long long)p->crop_y + p->crop_h > CG_MAX_COORD)) return 2;
    return 0;
}

} // namespace

namespace artgpu { namespace api {

int cg_check(artgpu_ctx *ctx, int W, int H, const artgpu_creative_gradients_params *p, const char *who, CgDerived *d)
{
    *d = CgDerived{};
    const char *why;
    const int bad = cg_refusal(p, W, H, &why);
    if (bad) return fail(ctx, bad == 1 ? ARTGPU_EINVAL : ARTGPU_EUNSUPPORTED, "%s: %s", who, why);
    cg_derive(p, W, H, d);
    // normn's cases 2, 4, 6, 8 are all the kernel has
    if (d->apply_pcvignette && d->is_super_ellipse_mode && d->sep != 2 && d->sep != 4 && d->sep != 6)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: super-ellipse degree %d is not on the device path", who, d->sep);
    return ARTGPU_OK;
}

int creative_gradients_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const CgDerived &d)
{
    if (!d.apply_gradient && !d.apply_pcvignette) return ARTGPU_OK;
    CgArgs a = {};
    for (int k = 0; k < 3; ++k) a.img[k] = planes[k];
    a.stride = stride; a.w = W; a.h = H; a.d = d;
    HIPCHK(ctx, launch_cg(a, ctx->stream));
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_creative_gradients(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_creative_gradients_params *params)
{
    StageScope scope_(ctx, "ImProcFunctions::creativeGradients");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !plane_ok(&img->r)) return fail(ctx, ARTGPU_EINVAL, "creative_gradients: bad image");
    int rc;
    CgDerived d;
    if ((rc = cg_check(ctx, img->r.w, img->r.h, params, "creative_gradients", &d))) return rc;
    if (!d.apply_gradient && !d.apply_pcvignette) return ARTGPU_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB b;
    if ((rc = bind_rgb(ctx, img, 4, true, &b, "creative_gradients")) || (rc = creative_gradients_dev(ctx, b.p, b.stride, b.w, b.h, d))) return rc;
    return unbind_rgb(ctx, img, &b);
}

int artgpu_creative_gradient_params(const artgpu_creative_gradients_params *params, int w, int h, artgpu_creative_gradient_derived *out)
{
    const char *why;
    if (!out) return ARTGPU_EINVAL;
    const int bad = cg_refusal(params, w, h, &why);
    if (bad) return bad == 1 ? ARTGPU_EINVAL : ARTGPU_EUNSUPPORTED;
    CgDerived d;
    cg_derive(params, w, h, &d);
    std::memcpy(out, &d, sizeof d);
    return ARTGPU_OK;
}

int artgpu_set_pipeline_creative_gradients(artgpu_ctx *ctx, const artgpu_creative_gradients_params *params)
{
    if (!ctx) return ARTGPU_EINVAL;
    ctx->shared.pipe_cg_on = params ? 1 : 0;
    ctx->shared.pipe_cg = params ? *params : artgpu_creative_gradients_params{};
    return ARTGPU_OK;
}

} // extern "C"
