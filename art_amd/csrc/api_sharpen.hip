// art_amd/csrc/api_sharpen.hip -- capture sharpening behind the C ABI: ImProcFunctions::doSharpening, method "rld", the RL deconvolution and the typed
// gaussian blur on their own, and the auto radius.  The kernels are sharpen.hip's.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace {

constexpr size_t SH_COUNTER_BYTES = 64;      // P_SH_BYTES: two 64-bit counters, then the impulse map

bool sharpen_sigma_ok(double sigma) { return sigma == sigma && !std::isinf(sigma) && sigma < 25.0; }

// deconvsharpening on a contiguous device plane; `work`: five planes (estimate x 2, ratio, out, the gaussian's forward buffer).
// counters (device, zeroed; may be null): [1] += the pixels frozen before the last iteration.  *early / *regime for artgpu_sharpening_info.
int rl_dev(artgpu_ctx *ctx, float *lum, const float *blend, const unsigned char *impulse, int W, int H, double sigma, float amount, float *work,
                  unsigned long long *counters, int *early, int *regime)
{
    *regime = -1; *early = 0;
    if (amount <= 0) { *early = 4; return ARTGPU_OK; }                               // L146-148
    if (sigma < 0.2f) { *early = 5; return ARTGPU_OK; }                              // L154-156
    const size_t n = (size_t)W * H;
    ShRlArgs a = {};
    const int rg = sh_regime(sigma, &a.k);
    *regime = rg;
    float *est = work, *other = work + n, *ratio = work + 2 * n, *out = work + 3 * n, *gtmp = work + 4 * n;
    a.ratio = ratio; a.lum = lum; a.blend = blend; a.impulse = impulse; a.out = out; a.W = W; a.H = H; a.amount = amount;
    int rc;
    HIPCHK(ctx, launch_rl_init(lum, est, out, W, H, ctx->stream));
    for (int it = 0; it < 20; ++it) {
        if (rg == SH_COPY) {
            // gaussianBlur copies whatever the type: the estimate never changes, and neither does check_stop's verdict after the first iteration
            if (it == 0) { a.est_in = est; a.est_out = est; HIPCHK(ctx, launch_rl_point(a, 0, ctx->stream)); }
        } else if (rg == SH_YVV) {
            HIPCHK(ctx, hipMemcpyAsync(ratio, est, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
            if ((rc = gaussian_dev(ctx, ratio, gtmp, W, H, sigma))) return rc;
            HIPCHK(ctx, launch_yvv_div(ratio, lum, W, H, ctx->stream));
            if ((rc = gaussian_dev(ctx, ratio, gtmp, W, H, sigma))) return rc;
            a.est_in = est; a.est_out = est;
            HIPCHK(ctx, launch_rl_point(a, 1, ctx->stream));
        } else if (ctx->shared.opt_sharpen_fused) {
            a.est_in = est; a.est_out = other;
            HIPCHK(ctx, launch_rl_iter(a, rg, ctx->stream));
            std::swap(est, other);
        } else {
            HIPCHK(ctx, launch_gauss_div(est, ratio, lum, W, H, rg, a.k, ctx->stream));
            HIPCHK(ctx, launch_gauss_mult(ratio, est, W, H, rg, a.k, ctx->stream));
            a.est_in = est; a.est_out = est;
            HIPCHK(ctx, launch_rl_point(a, 0, ctx->stream));
        }
        if (it == 18 && counters) HIPCHK(ctx, launch_sh_count(nullptr, out, n, counters, ctx->stream));
    }
    HIPCHK(ctx, launch_rl_final(lum, est, out, blend, impulse, amount, W, H, ctx->stream));
    return ARTGPU_OK;
}

int sharpen_scratch(artgpu_ctx *ctx, size_t n, int nplanes, float **planes, unsigned long long **counters, unsigned char **impulse)
{
    float *bytes;
    int rc;
    if ((rc = pool_get(ctx, P_SH_PLANES, (size_t)nplanes * n * 4, planes)) || (rc = pool_get(ctx, P_SH_BYTES, SH_COUNTER_BYTES + n, &bytes))) return rc;
    *counters = reinterpret_cast<unsigned long long *>(bytes);
    *impulse = reinterpret_cast<unsigned char *>(bytes) + SH_COUNTER_BYTES;
    return ARTGPU_OK;
}

int sharpen_read_counters(artgpu_ctx *ctx, const unsigned long long *counters, artgpu_sharpening_info *info)
{
    unsigned long long host[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(host, counters, sizeof host, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    info->impulse_pixels = (int64_t)host[0];
    info->frozen_pixels = (int64_t)host[1];
    return ARTGPU_OK;
}

} // namespace

namespace artgpu { namespace api {

int sharpen_check(artgpu_ctx *ctx, int W, int H, const artgpu_sharpening_params *p, double scale, const char *who, SharpenPlan *pl)
{
    *pl = SharpenPlan{};
    if (!p->enabled) { pl->early = 1; return ARTGPU_OK; }
    if (p->amount < 1) { pl->early = 2; return ARTGPU_OK; }
    if (W < 8 || H < 8) { pl->early = 3; return ARTGPU_OK; }
    if (p->method != ARTGPU_SHARPEN_RLD) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: only the rld method is on the device path (method %d)", who, p->method);
    if (!(scale > 0.0) || std::isinf(scale)) return fail(ctx, ARTGPU_EINVAL, "%s: scale must be positive", who);
    const float s_scale = std::sqrt(scale);                                          // L726-729
    pl->contrast = sh_pow_F(p->contrast / 100.f, 1.2f) * s_scale;
    pl->blur_radius = 2.f / s_scale;
    if (!(pl->blur_radius >= 0.6)) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: mask blur radius %g (scale %g) below the shared gaussian's range", who, (double)pl->blur_radius, scale);
    pl->sigma = p->deconvradius / scale;                                             // L756-759
    pl->amount = p->deconvamount / 100.f;
    pl->delta = p->deconvCornerBoost / scale;
    pl->boost = pl->delta > 0.01f ? 1 : 0;
    if (!sharpen_sigma_ok(pl->sigma) || (pl->boost && !sharpen_sigma_ok(pl->sigma + pl->delta)))
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: deconvolution radius %g (corner boost %g) is not finite or not below 25", who, pl->sigma, (double)pl->delta);
    return ARTGPU_OK;
}

// doSharpening on device planes (rows of `stride` floats), enqueued on ctx->stream; the host waits only to fill `info`
int sharpen_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const artgpu_sharpening_params *p, const double ws[9],
                       const SharpenPlan &pl, artgpu_sharpening_info *info)
{
    if (info) { info->early_out = pl.early; info->regime = -1; }
    if (pl.early) return ARTGPU_OK;
    const size_t n = (size_t)W * H;
    float *sp;
    unsigned long long *counters;
    unsigned char *impulse;
    int rc;
    if ((rc = sharpen_scratch(ctx, n, pl.boost ? SHP_NPLANES : SHP_NPLANES - 1, &sp, &counters, &impulse))) return rc;
    float *Y = sp + SHP_Y * n, *blend = sp + SHP_BLEND * n, *YY = sp + SHP_YY * n, *lpf = sp + SHP_RATIO * n, *gtmp = sp + SHP_GTMP * n;
    ShImage im = {{planes[0], planes[1], planes[2]}, stride, W, H};
    const float ws1[3] = {(float)ws[3], (float)ws[4], (float)ws[5]};                 // TMatrix is float (iccstore.h:38)
    HIPCHK(ctx, launch_sh_luminance(im, ws1, Y, ctx->stream));
    // buildBlendMask(Y, blend, W, H, contrast, 1.f, false, 2.f / s_scale) (rt_algo.cc:416-494)
    DualArgs da = {};
    da.L = Y; da.blend = blend; da.w = W; da.h = H; da.threshold = pl.contrast;
    HIPCHK(ctx, launch_blend_mask(da, ctx->stream));
    if (pl.contrast != 0.f && (rc = gaussian_dev(ctx, blend, gtmp, W, H, pl.blur_radius))) return rc;
    // markImpulse(W, H, Y, impulse, 2.f): the low-pass is gaussianBlur(src, lpf, max(2.f, thresh - 1.f))
    HIPCHK(ctx, hipMemcpyAsync(lpf, Y, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if ((rc = gaussian_dev(ctx, lpf, gtmp, W, H, std::max(2.f, 2.f - 1.f)))) return rc;
    HIPCHK(ctx, launch_sh_impulse(Y, lpf, impulse, W, H, 2.f, ctx->stream));
    if (info) {
        HIPCHK(ctx, hipMemsetAsync(counters, 0, SH_COUNTER_BYTES, ctx->stream));
        HIPCHK(ctx, launch_sh_count(impulse, nullptr, n, counters, ctx->stream));
    }
    HIPCHK(ctx, hipMemcpyAsync(YY, Y, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    int early = 0, regime = -1;
    if ((rc = rl_dev(ctx, YY, blend, impulse, W, H, pl.sigma, pl.amount, sp + SHP_EST_A * n, info ? counters : nullptr, &early, &regime))) return rc;
    if (pl.boost) {
        float *YY2 = sp + SHP_YY2 * n;
        int e2, r2;
        HIPCHK(ctx, hipMemcpyAsync(YY2, Y, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
        if ((rc = rl_dev(ctx, YY2, blend, impulse, W, H, pl.sigma + pl.delta, pl.amount, sp + SHP_EST_A * n, nullptr, &e2, &r2))) return rc;
        const int fw = p->full_width > 0 ? p->full_width : W, fh = p->full_height > 0 ? p->full_height : H;
        ShCornerArgs ca = {};
        ca.YY = YY; ca.YY2 = YY2; ca.W = W; ca.H = H; ca.ox = p->offset_x; ca.oy = p->offset_y; ca.w2 = fw / 2; ca.h2 = fh / 2;
        const float radius = std::max(ca.w2, ca.h2);                                 // CornerBoostMask (L317-323)
        const float lat = float(p->deconvCornerLatitude) / 150.f;
        ca.r2 = (radius - radius * std::max(0.f, std::min(lat, 1.f))) / 2.f;
        ca.sigma = 2.f * ((radius * 0.3f) * (radius * 0.3f));
        HIPCHK(ctx, launch_sh_corner(ca, ctx->stream));
    }
    HIPCHK(ctx, launch_sh_multiply(im, YY, Y, ctx->stream));
    if (info) {
        info->sigma = pl.sigma; info->regime = regime; info->early_out = early; info->contrast_threshold = pl.contrast;
        if ((rc = sharpen_read_counters(ctx, counters, info))) return rc;
    }
    return ARTGPU_OK;
}

int plane_into(artgpu_ctx *ctx, const artgpu_plane *pl, float *dst)
{
    const size_t rowb = (size_t)pl->w * 4;
    HIPCHK(ctx, hipMemcpy2DAsync(dst, rowb, pl->p, (size_t)pl->row_stride_bytes, rowb, pl->h, pl->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    return ARTGPU_OK;
}

// calcRadiusBayer's maximum of a device CFA plane into result[0] (P_SH_STATE), enqueued; no wait
int auto_radius_dev(artgpu_ctx *ctx, const float *raw, size_t stride, int W, int H, uint32_t filters, float lower, float upper, float **result)
{
    float *st;
    int rc;
    if ((rc = pool_get(ctx, P_SH_STATE, (SH_RADIUS_PARTIALS + 16) * 4, &st))) return rc;
    const auto FC = [&](unsigned row, unsigned col) { return (filters >> ((((row << 1) & 14u) + (col & 1u)) << 1)) & 3u; };
    const unsigned fc0 = filters ? FC(0, 0) : 0u, fc1 = filters ? FC(1, 0) : 0u;     // deconvautoradius.cc:207, 240
    HIPCHK(ctx, launch_sh_radius(raw, stride, W, H, fc0, fc1, lower, upper, st + 16, st, ctx->stream));
    *result = st;
    return ARTGPU_OK;
}

float auto_radius_of(float maxRatio) { return std::sqrt((1.f / (std::log(1.f / maxRatio) / 2.f)) / -2.f); }   // L90

} } // namespace artgpu::api

extern "C" {

int artgpu_sharpening(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_sharpening_params *params, const double ws[9], double scale, artgpu_sharpening_info *info)
{
    StageScope scope_(ctx, "ImProcFunctions::sharpening");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !params || !ws) return fail(ctx, ARTGPU_EINVAL, "sharpening: null argument");
    if (info) { *info = artgpu_sharpening_info{}; info->regime = -1; }
    if (!plane_ok(&img->r)) return fail(ctx, ARTGPU_EINVAL, "sharpening: bad plane");
    SharpenPlan pl;
    int rc;
    if ((rc = sharpen_check(ctx, img->r.w, img->r.h, params, scale, "sharpening", &pl))) return rc;
    if (pl.early) { if (info) info->early_out = pl.early; return ARTGPU_OK; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "sharpening"))) return rc;
    if ((rc = sharpen_dev(ctx, d.p, d.stride, d.w, d.h, params, ws, pl, info))) return rc;
    return unbind_rgb(ctx, img, &d);
}

int artgpu_rl_deconvolution(artgpu_ctx *ctx, artgpu_plane *luminance, const artgpu_plane *blend, const uint8_t *impulse, double sigma, float amount,
                            artgpu_sharpening_info *info)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(luminance) || !plane_ok(blend) || !impulse || blend->w != luminance->w || blend->h != luminance->h)
        return fail(ctx, ARTGPU_EINVAL, "rl_deconvolution: bad planes");
    if (info) { *info = artgpu_sharpening_info{}; info->regime = -1; info->sigma = sigma; }
    if (amount <= 0) { if (info) info->early_out = 4; return ARTGPU_OK; }
    if (sigma < 0.2f) { if (info) info->early_out = 5; return ARTGPU_OK; }
    if (!sharpen_sigma_ok(sigma)) return fail(ctx, ARTGPU_EUNSUPPORTED, "rl_deconvolution: sigma %g is not finite or not below 25", sigma);
    const int W = luminance->w, H = luminance->h;
    if (W < 8 || H < 8) return fail(ctx, ARTGPU_EUNSUPPORTED, "rl_deconvolution: plane smaller than 8x8");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H;
    float *sp;
    unsigned long long *counters;
    unsigned char *imp;
    int rc;
    if ((rc = sharpen_scratch(ctx, n, SHP_NPLANES - 1, &sp, &counters, &imp))) return rc;
    float *lum = sp + SHP_YY * n, *bl = sp + SHP_BLEND * n;
    if ((rc = plane_into(ctx, luminance, lum)) || (rc = plane_into(ctx, blend, bl))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(imp, impulse, n, luminance->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    if (info) {
        HIPCHK(ctx, hipMemsetAsync(counters, 0, SH_COUNTER_BYTES, ctx->stream));
        HIPCHK(ctx, launch_sh_count(imp, nullptr, n, counters, ctx->stream));
    }
    int early, regime;
    if ((rc = rl_dev(ctx, lum, bl, imp, W, H, sigma, amount, sp + SHP_EST_A * n, info ? counters : nullptr, &early, &regime))) return rc;
    if (info) {
        info->regime = regime; info->early_out = early;
        if ((rc = sharpen_read_counters(ctx, counters, info))) return rc;
    }
    return pool_to_plane(ctx, lum, luminance);
}

int artgpu_gaussian_blur_ex(artgpu_ctx *ctx, artgpu_plane *src, artgpu_plane *dst, const artgpu_plane *div, double sigma, int gausstype)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(src) || !plane_ok(dst) || dst->w != src->w || dst->h != src->h || src->p == dst->p) return fail(ctx, ARTGPU_EINVAL, "gaussian_blur_ex: bad planes (src != dst)");
    if (gausstype != ARTGPU_GAUSS_MULT && gausstype != ARTGPU_GAUSS_DIV)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "gaussian_blur_ex: GAUSS_MULT or GAUSS_DIV (GAUSS_STANDARD: artgpu_gaussian_blur)");
    const bool is_div = gausstype == ARTGPU_GAUSS_DIV;
    if (is_div && (!plane_ok(div) || div->w != src->w || div->h != src->h)) return fail(ctx, ARTGPU_EINVAL, "gaussian_blur_ex: GAUSS_DIV needs the divisor plane");
    if (!sharpen_sigma_ok(sigma)) return fail(ctx, ARTGPU_EUNSUPPORTED, "gaussian_blur_ex: sigma %g is not finite or not below 25", sigma);
    const int W = src->w, H = src->h;
    if (W < 8 || H < 8) return fail(ctx, ARTGPU_EUNSUPPORTED, "gaussian_blur_ex: plane smaller than 8x8");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H;
    float *sp;
    int rc;
    if ((rc = pool_get(ctx, P_SH_PLANES, 4 * n * 4, &sp))) return rc;
    float *s = sp, *d = sp + n, *v = sp + 2 * n, *gtmp = sp + 3 * n;
    if ((rc = plane_into(ctx, src, s))) return rc;
    ShCoef k;
    const int rg = sh_regime(sigma, &k);
    if (rg == SH_COPY) return pool_to_plane(ctx, s, dst);                            // GAUSS_SKIP ignores the type (gauss.cc:1437-1443)
    if (is_div) { if ((rc = plane_into(ctx, div, v))) return rc; }
    else if ((rc = plane_into(ctx, dst, d))) return rc;
    if (rg == SH_YVV) {
        if ((rc = gaussian_dev(ctx, s, gtmp, W, H, sigma))) return rc;
        if (is_div) { HIPCHK(ctx, launch_yvv_div(s, v, W, H, ctx->stream)); return pool_to_plane(ctx, s, dst); }
        HIPCHK(ctx, launch_yvv_mult(s, d, W, H, ctx->stream));
        if ((rc = pool_to_plane(ctx, s, src))) return rc;                            // the reference filters src in place here
        return pool_to_plane(ctx, d, dst);
    }
    if (is_div) HIPCHK(ctx, launch_gauss_div(s, d, v, W, H, rg, k, ctx->stream));
    else HIPCHK(ctx, launch_gauss_mult(s, d, W, H, rg, k, ctx->stream));
    return pool_to_plane(ctx, d, dst);
}

int artgpu_deconv_auto_radius(artgpu_ctx *ctx, const artgpu_plane *raw, uint32_t filters, float lower_limit, float clip_val, float *radius, float *max_ratio)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(raw) || !radius) return fail(ctx, ARTGPU_EINVAL, "deconv_auto_radius: bad argument");
    if (filters == 9) return fail(ctx, ARTGPU_EUNSUPPORTED, "deconv_auto_radius: X-Trans (calcRadiusXtrans) is not on the device path");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const float *dev = raw->p;
    size_t stride = (size_t)(raw->row_stride_bytes / 4);
    int rc;
    if (!raw->on_device) {
        float *cp;
        if ((rc = plane_to_pool(ctx, raw, P_SH_PLANES, &cp))) return rc;
        dev = cp; stride = raw->w;
    }
    float *res;
    if ((rc = auto_radius_dev(ctx, dev, stride, raw->w, raw->h, filters, lower_limit, clip_val, &res))) return rc;
    float mr = 1.f;
    HIPCHK(ctx, hipMemcpyAsync(&mr, res, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (max_ratio) *max_ratio = mr;
    *radius = auto_radius_of(mr);
    return ARTGPU_OK;
}

} // extern "C"
