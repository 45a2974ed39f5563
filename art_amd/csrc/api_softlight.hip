// art_amd/csrc/api_softlight.hip -- ImProcFunctions::softLight (rtengine/ipsoftlight.cc:31-82) behind the C ABI: the table (hostluts.hip's
// build_soft_light_lut) kept per strength, the launch.  The kernel is the tone curve's (pixelops.hip) with PixArgs::keep_above set.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace {

constexpr int SL_GUI_MAX = 100;            // strength: 0 .. 100 (rtgui/softlight.cc)

// the table of `strength` in P_SL_LUT: built when the strength changes, uploaded when it was built or the slot moved
int sl_lut_dev(artgpu_ctx *ctx, int strength, const float **out)
{
    float *dev;
    int rc;
    if ((rc = pool_get(ctx, P_SL_LUT, 65536 * 4, &dev))) return rc;
    const bool same = ctx->sl_lut_host.size() == 65536 && ctx->sl_lut_strength == strength;
    if (!same) {
        ctx->sl_lut_host.resize(65536);
        build_soft_light_lut(strength, ctx->sl_lut_host.data());
        ctx->sl_lut_strength = strength;
    }
    if (!same || ctx->sl_lut_dev != dev) {
        ctx->sl_lut_dev = nullptr;
        if ((rc = h2d_table(ctx, dev, ctx->sl_lut_host.data(), 65536 * 4))) return rc;
        ctx->sl_lut_dev = dev;
    }
    *out = dev;
    return ARTGPU_OK;
}

} // namespace

namespace artgpu { namespace api {

int sl_check(artgpu_ctx *ctx, const artgpu_soft_light_params *p, const char *who, SlPlan *pl)
{
    *pl = SlPlan{};
    if (!p) return fail(ctx, ARTGPU_EINVAL, "%s: bad arguments", who);
    if (!p->enabled || p->strength <= 0) return ARTGPU_OK;                            // ipsoftlight.cc:48-51
    if (p->strength > SL_GUI_MAX) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: strength %d outside 0 .. %d", who, p->strength, SL_GUI_MAX);
    pl->on = 1; pl->strength = p->strength;
    return ARTGPU_OK;
}

int soft_light_dev(artgpu_ctx *ctx, const DevRGB &d, const SlPlan &pl)
{
    if (!pl.on) return ARTGPU_OK;
    int rc;
    const float *lut;
    if ((rc = sl_lut_dev(ctx, pl.strength, &lut))) return rc;
    PixArgs a = {};
    for (int k = 0; k < 3; ++k) a.dst[k] = d.p[k];
    a.dst_stride = d.stride; a.w = d.w; a.h = d.h;
    a.whitept = 1.f; a.lut = lut; a.keep_above = 1;
    a.no_lds_lut = !ctx->shared.opt_lut_lds; a.cu_reserve = cu_reserve_of(ctx);
    HIPCHK(ctx, launch_tone_std(a, ctx->stream));
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_soft_light(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_soft_light_params *params)
{
    StageScope scope_(ctx, "ImProcFunctions::softLight");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !plane_ok(&img->r)) return fail(ctx, ARTGPU_EINVAL, "soft_light: bad image");
    int rc;
    SlPlan pl;
    if ((rc = sl_check(ctx, params, "soft_light", &pl))) return rc;
    if (!pl.on) return ARTGPU_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "soft_light")) || (rc = soft_light_dev(ctx, d, pl))) return rc;
    return unbind_rgb(ctx, img, &d);
}

int artgpu_soft_light_lut(int strength, float *lut)
{
    if (!lut) return ARTGPU_EINVAL;
    build_soft_light_lut(strength, lut);
    return ARTGPU_OK;
}

int artgpu_set_pipeline_soft_light(artgpu_ctx *ctx, const artgpu_soft_light_params *params)
{
    if (!ctx) return ARTGPU_EINVAL;
    ctx->shared.pipe_sl_on = params ? 1 : 0;
    ctx->shared.pipe_sl = params ? *params : artgpu_soft_light_params{};
    return ARTGPU_OK;
}

} // extern "C"
