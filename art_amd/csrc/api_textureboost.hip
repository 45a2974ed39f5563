// art_amd/csrc/api_textureboost.hip -- ImProcFunctions::textureBoost behind the C ABI: the per-region plan, texture_boost on the Y plane and the
// region loop between the two mode switches.  The kernels are textureboost.hip's.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace {

// 0, or the code with the message set
int tb_plan(artgpu_ctx *ctx, int W, int H, const artgpu_texture_boost_region *r, double scale, int high_detail, const char *who, TbPlan *pl)
{
    if (!std::isfinite(r->strength) || !std::isfinite(r->detail_threshold) || !(r->detail_threshold > 0.0))
        return fail(ctx, ARTGPU_EINVAL, "%s: strength %g / detail threshold %g", who, r->strength, r->detail_threshold);
    if (r->iterations < 1) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: %d iterations (the reference then only divides and multiplies by 65535)", who, r->iterations);
    *pl = TbPlan{};
    const float full_radius = r->detail_threshold * 3.5f;
    const float fradius = full_radius / scale;
    const int radius = std::max(int(fradius + 0.5f), 1);
    const float delta = radius / fradius;
    const float s = r->strength >= 0 ? sh_pow_F(r->strength / 2.f, 0.3f) * 2.f : r->strength;
    pl->strength = s >= 0 ? 1.f + s : 1.f / (1.f - s);
    pl->strength2 = s >= 0 ? 1.f + s / 4.f : 1.f / (1.f - s / 2.f);
    pl->radius = radius;
    pl->isguided = full_radius >= 1.f ? 1 : 0;
    pl->w = W; pl->h = H;
    if (fradius > 1.f && delta > 1.01f) {
        pl->rescaled = 1;
        pl->w = int(W * delta + 0.5f);
        pl->h = int(H * delta + 0.5f);
    }
    if (!pl->isguided) {
        if (!high_detail) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: detail threshold %g without high_detail (gaussianBlur at a sub-pixel sigma is not on the device path)", who, r->detail_threshold);
        pl->K = tb_gaussian_kernel(fradius, pl->coef);
        if (pl->K > TB_MAX_K) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: sigma %g needs a %dx%d gaussian, the kernels hold %dx%d", who, fradius, pl->K, pl->K, TB_MAX_K, TB_MAX_K);
    } else {
        { const GfGrid g = gf_grid(pl->w, pl->h, radius); pl->w1 = g.w; pl->h1 = g.h; pl->rad1 = g.rad; }
    }
    { const GfGrid g = gf_grid(pl->w, pl->h, radius * 4); pl->w2 = g.w; pl->h2 = g.h; pl->rad2 = g.rad; }
    if ((pl->isguided && (pl->w1 < 1 || pl->h1 < 1)) || pl->w2 < 1 || pl->h2 < 1)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: a %dx%d plane has a side shorter than the guided filter's subsampling", who, pl->w, pl->h);
    if (pl->rad1 > HBLUR_MAX_RADIUS || pl->rad2 > HBLUR_MAX_RADIUS)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: box radius %d is above the %d the blur kernels hold in LDS", who, std::max(pl->rad1, pl->rad2), HBLUR_MAX_RADIUS);
    return ARTGPU_OK;
}

// one self-guided filter's statistics on `mid`: the grid ends as mean a / mean b
int tb_guided_stats(artgpu_ctx *ctx, const float *mid, int w, int h, const DhGuided &gf, int rad, float *tmp)
{
    int rc;
    HIPCHK(ctx, launch_tb_gf_subsample(mid, w, h, gf, ctx->stream));
    if ((rc = box_blur_planes(ctx, gf.low, tmp, 2, gf.nl, gf.w, gf.h, rad))) return rc;
    HIPCHK(ctx, launch_tb_gf_ab(gf, ctx->stream));
    return box_blur_planes(ctx, gf.low, tmp, 2, gf.nl, gf.w, gf.h, rad);
}

// texture_boost (iptextureboost.cc:37-178) on a device Y plane (rows of `stride` floats), enqueued on ctx->stream without a host wait;
// do_blend: the region loop's intp(mask, Y, YY) (L234-240) is part of the last store
int texture_boost_region_dev(artgpu_ctx *ctx, float *Y, size_t stride, int W, int H, const TbPlan &pl, int iterations, int do_blend,
                                    const artgpu_plane *mask, TbState **state)
{
    const size_t nw = (size_t)pl.w * pl.h, nl1 = pl.isguided ? (size_t)pl.w1 * pl.h1 : 0, nl2 = (size_t)pl.w2 * pl.h2;
    const size_t nlow = 2 * std::max(nl1, nl2);
    float *planes, *low, *tmp, *stf;
    int rc;
    if ((rc = pool_get(ctx, P_TB_PLANES, (pl.isguided ? 2 : 3) * nw * 4, &planes)) || (rc = pool_get(ctx, P_TB_LOW, nlow * 4, &low)) ||
        (rc = pool_get(ctx, P_TB_TMP, nlow * 4, &tmp)) || (rc = pool_get(ctx, P_TB_STATE, (sizeof(TbState) / 4 + 3 * TB_MAX_PARTIALS) * 4, &stf)))      // state | minima | their 64-bit indices
        return rc;
    TbState *st = reinterpret_cast<TbState *>(stf);
    *state = st;
    float *src = planes, *mid = planes + nw, *spare = planes + 2 * nw;      // (spare: the convolution's other plane)
    const float *mk = nullptr;
    size_t m_stride = 0;
    if (do_blend && (rc = bind_plane(ctx, mask, P_TB_MASK, &mk, &m_stride))) return rc;
    TbPrepareArgs pa = {Y, stride, W, H, src, mid, pl.w, pl.h, stf + sizeof(TbState) / 4,
                        reinterpret_cast<unsigned long long *>(stf + sizeof(TbState) / 4 + TB_MAX_PARTIALS)};
    HIPCHK(ctx, launch_tb_prepare(pa, st, ctx->stream));
    for (int i = 0; i < iterations; ++i) {
        if (pl.isguided) {
            const DhGuided g1 = {low, nl1, pl.w1, pl.h1, 0.001f};
            if ((rc = tb_guided_stats(ctx, mid, pl.w, pl.h, g1, pl.rad1, tmp))) return rc;
            HIPCHK(ctx, launch_tb_gf_finish(mid, pl.w, pl.h, g1, ctx->stream));
        } else {
            TbConvArgs ca = {};
            ca.src = mid; ca.dst = spare; ca.w = pl.w; ca.h = pl.h; ca.K = pl.K;
            std::copy(pl.coef, pl.coef + pl.K * pl.K, ca.coef);
            HIPCHK(ctx, launch_tb_conv(ca, ctx->stream));
            std::swap(mid, spare);
        }
        const DhGuided g2 = {low, nl2, pl.w2, pl.h2, 0.001f / 10.f};
        if ((rc = tb_guided_stats(ctx, mid, pl.w, pl.h, g2, pl.rad2, tmp))) return rc;
        TbCombineArgs cb = {};
        cb.src = src; cb.mid = mid; cb.w = pl.w; cb.h = pl.h; cb.gf = g2; cb.st = st;
        cb.strength = pl.strength; cb.strength2 = pl.strength2; cb.blend = std::ldexp(1.f, -i);      // 1.f / std::pow(2.f, i)
        cb.last = (i == iterations - 1 && !pl.rescaled) ? 1 : 0;
        cb.Y = Y; cb.stride = stride; cb.do_blend = do_blend; cb.mask = mk; cb.m_stride = m_stride;
        HIPCHK(ctx, launch_tb_combine(cb, ctx->stream));
    }
    if (pl.rescaled) {
        const TbDownArgs da = {src, pl.w, pl.h, Y, stride, W, H, do_blend, mk, m_stride};
        HIPCHK(ctx, launch_tb_downscale(da, ctx->stream));
    }
    return ARTGPU_OK;
}

// what `info` reports of a region that ran; the minimum costs the call's one host wait
int tb_fill_info(artgpu_ctx *ctx, const TbPlan &pl, const TbState *st, artgpu_texture_boost_info *info)
{
    float minval;
    HIPCHK(ctx, hipMemcpyAsync(&minval, &st->minval, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    info->radius = pl.radius; info->isguided = pl.isguided; info->rescaled = pl.rescaled; info->work_w = pl.w; info->work_h = pl.h;
    info->kernel_size = pl.K; info->minval = minval; info->strength = pl.strength; info->strength2 = pl.strength2;
    return ARTGPU_OK;
}

} // namespace

namespace artgpu { namespace api {

// the region list of the whole tool: a plan per region that runs (strength != 0, L227), in order
int tb_check(artgpu_ctx *ctx, int W, int H, const artgpu_texture_boost_region *regions, int nregions, const double *ws, double scale, int high_detail,
                    const char *who, std::vector<TbPlan> *plans)
{
    if (nregions < 0 || (nregions > 0 && !regions) || !ws || !(scale > 0.0)) return fail(ctx, ARTGPU_EINVAL, "%s: bad arguments", who);
    plans->clear();
    for (int r = 0; r < nregions; ++r) {
        const artgpu_plane *m = regions[r].mask;
        if (m && (!plane_ok(m) || m->w != W || m->h != H)) return fail(ctx, ARTGPU_EINVAL, "%s: the mask of region %d must be a %dx%d plane", who, r, W, H);
        if (regions[r].strength == 0) continue;
        TbPlan pl;
        int rc;
        if ((rc = tb_plan(ctx, W, H, &regions[r], scale, high_detail, who, &pl))) return rc;
        plans->push_back(pl);
    }
    return ARTGPU_OK;
}

// ImProcFunctions::textureBoost (L198-242) on device planes in RGB mode: setMode(YUV), the regions that run, setMode(RGB) when asked for.
// already_yuv: the tool ahead (colorCorrection) left the image in YUV mode, where the reference's setMode(YUV) does nothing
int texture_boost_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const artgpu_texture_boost_region *regions, int nregions,
                             const double ws[9], const std::vector<TbPlan> &plans, int to_rgb, artgpu_texture_boost_info *info, int already_yuv)
{
    PixArgs ya = {};                                                   // Imagefloat::setMode (yuv_mode_kernel: do_clip 0 = to YUV, 1 = to RGB)
    for (int k = 0; k < 3; ++k) { ya.dst[k] = planes[k]; ya.mul[k] = (float)ws[3 + k]; }
    ya.dst_stride = stride; ya.w = W; ya.h = H;
    if (!already_yuv) HIPCHK(ctx, launch_yuv_mode(ya, ctx->stream));
    int rc;
    size_t k = 0;
    TbState *st = nullptr;
    for (int r = 0; r < nregions; ++r) {
        if (regions[r].strength == 0) continue;
        if ((rc = texture_boost_region_dev(ctx, planes[1], stride, W, H, plans[k], regions[r].iterations, 1, regions[r].mask, &st))) return rc;
        ++k;
    }
    if (info && k > 0 && (rc = tb_fill_info(ctx, plans[k - 1], st, info))) return rc;
    if (to_rgb) {
        ya.do_clip = 1;
        HIPCHK(ctx, launch_yuv_mode(ya, ctx->stream));
    }
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_texture_boost_plane(artgpu_ctx *ctx, artgpu_plane *Y, const artgpu_texture_boost_region *region, double scale, int high_detail,
                               artgpu_texture_boost_info *info)
{
    StageScope scope_(ctx, "texture_boost");
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(Y) || !region || !(scale > 0.0)) return fail(ctx, ARTGPU_EINVAL, "texture_boost_plane: bad arguments");
    if (info) *info = artgpu_texture_boost_info{};
    TbPlan pl;
    int rc;
    if ((rc = tb_plan(ctx, Y->w, Y->h, region, scale, high_detail, "texture_boost_plane", &pl))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    float *work = Y->p;
    size_t stride = (size_t)(Y->row_stride_bytes / 4);
    if (!Y->on_device) {
        if ((rc = plane_to_pool(ctx, Y, P_TB_Y, &work))) return rc;
        stride = Y->w;
    }
    TbState *st = nullptr;
    if ((rc = texture_boost_region_dev(ctx, work, stride, Y->w, Y->h, pl, region->iterations, 0, nullptr, &st))) return rc;
    if (info && (rc = tb_fill_info(ctx, pl, st, info))) return rc;
    return Y->on_device ? ARTGPU_OK : pool_to_plane(ctx, work, Y);
}

int artgpu_texture_boost(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_texture_boost_region *regions, int nregions, const double ws[9], double scale,
                         int high_detail, int to_rgb, artgpu_texture_boost_info *info)
{
    StageScope scope_(ctx, "ImProcFunctions::textureBoost");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !plane_ok(&img->r)) return fail(ctx, ARTGPU_EINVAL, "texture_boost: bad image");
    if (info) *info = artgpu_texture_boost_info{};
    std::vector<TbPlan> plans;
    int rc;
    if ((rc = tb_check(ctx, img->r.w, img->r.h, regions, nregions, ws, scale, high_detail, "texture_boost", &plans))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "texture_boost"))) return rc;
    if ((rc = texture_boost_dev(ctx, d.p, d.stride, d.w, d.h, regions, nregions, ws, plans, to_rgb, info))) return rc;
    return unbind_rgb(ctx, img, &d);
}

} // extern "C"
