// art_amd/csrc/api_blackwhite.hip -- ImProcFunctions::blackAndWhite (rtengine/ipbw.cc:214-365) behind the C ABI: the mixer constants and
// gamma tables (hostluts.hip), the caller's colour-cast tables, the launch.  The kernel is blackwhite.hip's.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace {

constexpr int BW_MIXER_MIN = -100, BW_MIXER_MAX = 200, BW_GAMMA_MIN = -100, BW_GAMMA_MAX = 100;    // rtgui/blackwhite.cc

// table `k` of P_BW_TAB holds `host` (65536 floats): copied into the context's own copy and uploaded unless that copy and the slot still hold it
int bw_table_dev(artgpu_ctx *ctx, float *tabs, int k, const float *host)
{
    std::vector<float> &own = ctx->bw_tab_host[k];
    if (own.size() == 65536 && std::memcmp(own.data(), host, 65536 * 4) == 0) return ARTGPU_OK;
    own.assign(host, host + 65536);
    const int rc = h2d_table(ctx, tabs + (size_t)k * 65536, own.data(), 65536 * 4);
    if (rc) own.clear();
    return rc;
}

} // namespace

namespace artgpu { namespace api {

int bw_check(artgpu_ctx *ctx, const artgpu_black_and_white_params *p, const double *ws, const char *who, BwPlan *pl)
{
    *pl = BwPlan{};
    if (!p) return fail(ctx, ARTGPU_EINVAL, "%s: bad arguments", who);
    if (!p->enabled) return ARTGPU_OK;                                                 // ipbw.cc:216-218
    if (p->setting < 0 || p->setting >= ARTGPU_BW_SETTING_COUNT || p->filter < 0 || p->filter >= ARTGPU_BW_FILTER_COUNT)
        return fail(ctx, ARTGPU_EINVAL, "%s: setting %d / filter %d", who, p->setting, p->filter);
    if (p->cast_bottom > 0 && (!p->ulut || !p->vlut || !ws)) return fail(ctx, ARTGPU_EINVAL, "%s: a colour cast needs ulut, vlut and ws", who);
    const int mix[3] = {p->mixer_red, p->mixer_green, p->mixer_blue}, gam[3] = {p->gamma_red, p->gamma_green, p->gamma_blue};
    for (int k = 0; k < 3; ++k) {
        if (mix[k] < BW_MIXER_MIN || mix[k] > BW_MIXER_MAX) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: mixer value %d outside %d .. %d", who, mix[k], BW_MIXER_MIN, BW_MIXER_MAX);
        if (gam[k] < BW_GAMMA_MIN || gam[k] > BW_GAMMA_MAX) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: gamma %d outside %d .. %d", who, gam[k], BW_GAMMA_MIN, BW_GAMMA_MAX);
        pl->gam[k] = bw_gamma_of(gam[k]);
    }
    pl->hasgamma = pl->gam[0] != 1.f || pl->gam[1] != 1.f || pl->gam[2] != 1.f;       // L253
    bw_mixer_constants(p->setting, p->filter, float(p->mixer_red), float(p->mixer_green), float(p->mixer_blue), &pl->mix);
    if (p->cast_bottom > 0) { pl->ulut = p->ulut; pl->vlut = p->vlut; }
    pl->on = 1;
    return ARTGPU_OK;
}

int black_and_white_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const double *ws, const BwPlan &pl, int to_rgb)
{
    if (!pl.on) return ARTGPU_OK;
    int rc;
    BwArgs a = {};
    for (int k = 0; k < 3; ++k) a.img[k] = planes[k];
    a.stride = stride; a.w = W; a.h = H;
    a.bwr = pl.mix.bwr; a.bwg = pl.mix.bwg; a.bwb = pl.mix.bwb; a.kcorec = pl.mix.kcorec;
    if (pl.hasgamma || pl.ulut) {
        float *tabs;
        if ((rc = pool_get(ctx, P_BW_TAB, (size_t)5 * 65536 * 4, &tabs))) return rc;
        if (ctx->bw_tab_dev != tabs)                                                   // a fresh or moved slot holds none of the five tables
            for (std::vector<float> &own : ctx->bw_tab_host) own.clear();
        ctx->bw_tab_dev = tabs;
        if (pl.hasgamma) {
            std::vector<float> t(65536);
            for (int k = 0; k < 3; ++k) {
                if (ctx->bw_tab_host[k].size() != 65536 || ctx->bw_gam_key[k] != pl.gam[k]) {
                    build_bw_gamma_table(pl.gam[k], t.data());
                    ctx->bw_tab_host[k].clear();
                    if ((rc = bw_table_dev(ctx, tabs, k, t.data()))) return rc;
                    ctx->bw_gam_key[k] = pl.gam[k];
                }
                a.gamma[k] = tabs + (size_t)k * 65536;
            }
        }
        if (pl.ulut) {
            if ((rc = bw_table_dev(ctx, tabs, 3, pl.ulut)) || (rc = bw_table_dev(ctx, tabs, 4, pl.vlut))) return rc;
            a.ulut = tabs + (size_t)3 * 65536; a.vlut = tabs + (size_t)4 * 65536;
            for (int k = 0; k < 3; ++k) a.ws1[k] = (float)ws[3 + k];
            a.to_rgb = to_rgb ? 1 : 0;
        }
    }
    HIPCHK(ctx, launch_bw(a, ctx->stream));
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_black_and_white(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_black_and_white_params *params, const double ws[9])
{
    StageScope scope_(ctx, "ImProcFunctions::blackAndWhite");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !plane_ok(&img->r)) return fail(ctx, ARTGPU_EINVAL, "black_and_white: bad image");
    int rc;
    BwPlan pl;
    if ((rc = bw_check(ctx, params, ws, "black_and_white", &pl))) return rc;
    if (!pl.on) return ARTGPU_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "black_and_white")) || (rc = black_and_white_dev(ctx, d.p, d.stride, d.w, d.h, ws, pl, 1))) return rc;
    return unbind_rgb(ctx, img, &d);
}

int artgpu_bw_mixer_constants(int setting, int filter, int mixer_red, int mixer_green, int mixer_blue, artgpu_bw_mixer *out)
{
    if (!out || setting < 0 || setting >= ARTGPU_BW_SETTING_COUNT || filter < 0 || filter >= ARTGPU_BW_FILTER_COUNT) return ARTGPU_EINVAL;
    BwMixer m;
    bw_mixer_constants(setting, filter, float(mixer_red), float(mixer_green), float(mixer_blue), &m);
    *out = artgpu_bw_mixer{m.bwr, m.bwg, m.bwb, m.kcorec, m.filcor, m.rrm, m.ggm, m.bbm};
    return ARTGPU_OK;
}

int artgpu_set_pipeline_black_and_white(artgpu_ctx *ctx, const artgpu_black_and_white_params *params)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (params && params->cast_bottom > 0 && (!params->ulut || !params->vlut)) return fail(ctx, ARTGPU_EINVAL, "set_pipeline_black_and_white: a colour cast needs ulut and vlut");
    ctx->shared.pipe_bw_on = params ? 1 : 0;
    ctx->shared.pipe_bw = params ? *params : artgpu_black_and_white_params{};
    ctx->pipe_bw_tabs.clear();
    ctx->shared.pipe_bw.ulut = ctx->shared.pipe_bw.vlut = nullptr;
    if (params && params->cast_bottom > 0) {
        ctx->pipe_bw_tabs.assign(params->ulut, params->ulut + 65536);
        ctx->pipe_bw_tabs.insert(ctx->pipe_bw_tabs.end(), params->vlut, params->vlut + 65536);
        ctx->shared.pipe_bw.ulut = ctx->pipe_bw_tabs.data();
        ctx->shared.pipe_bw.vlut = ctx->pipe_bw_tabs.data() + 65536;
    }
    return ARTGPU_OK;
}

} // extern "C"
