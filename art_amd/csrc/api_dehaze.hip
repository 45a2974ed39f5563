// art_amd/csrc/api_dehaze.hip -- ImProcFunctions::dehaze behind the C ABI: the plan, the dark-channel haze removal with its one host wait for the
// thumbnail, the dark-channel test hook, and the host-only strength table and ambient estimate.  The kernels are dehaze.hip's.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace {

// the strength table of the last curve seen: a batch passes the same curve for every frame, and 65536 curve evaluations on the host
// would otherwise be the longest step of the call
const float *dehaze_strength_cached(const artgpu_dehaze_params *p, std::vector<float> &out)
{
    static std::mutex m;
    static std::vector<double> pts;
    static std::vector<float> lut;
    std::lock_guard<std::mutex> lk(m);
    const std::vector<double> now(p->strength, p->strength + p->nstrength);
    if (lut.empty() || now != pts) {
        lut.resize(65536);
        dh_strength_lut(p->strength, p->nstrength, lut.data());
        pts = now;
    }
    out = lut;
    return out.data();
}

} // namespace

namespace artgpu { namespace api {

// what the call cannot do, before anything is touched: 0, or the code with the message set
int dehaze_check(artgpu_ctx *ctx, int W, int H, const artgpu_dehaze_params *p, const double *ws, double scale, const char *who, DehazePlan *pl)
{
    if (!p || !ws || !(scale > 0.0) || p->nstrength < 0 || (p->nstrength > 0 && !p->strength)) return fail(ctx, ARTGPU_EINVAL, "%s: bad arguments", who);
    dh_thumb_size(W, H, &pl->ww, &pl->hh);
    const int lo = pl->ww < pl->hh ? pl->ww : pl->hh, hi = pl->ww < pl->hh ? pl->hh : pl->ww;
    pl->brad = hi / 20 > 1 ? hi / 20 : 1;
    if (p->blackpoint && lo < 2 * pl->brad + 1)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: black point on a %dx%d frame: the %dx%d thumbnail is narrower than its box blur (radius %d)", who, W, H, pl->ww, pl->hh, pl->brad);
    const int r1 = std::max((int)(5 / scale), 2);
    { const GfGrid g = gf_grid(W, H, r1); pl->w1 = g.w; pl->h1 = g.h; pl->rad1 = g.rad; }
    pl->patch = std::max(std::max(W, H) / 600, 2);
    { const GfGrid g = gf_grid(W, H, pl->patch * 4); pl->w2 = g.w; pl->h2 = g.h; pl->rad2 = g.rad; }
    if (pl->w1 < 1 || pl->h1 < 1 || pl->w2 < 1 || pl->h2 < 1)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: a %dx%d frame has a side shorter than the guided filter's subsampling", who, W, H);
    if (pl->patch > DH_MAX_PATCH || pl->rad1 > HBLUR_MAX_RADIUS || pl->rad2 > HBLUR_MAX_RADIUS || pl->brad > HBLUR_MAX_RADIUS)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: a %dx%d frame is beyond the patch / box radius the kernels hold in LDS", who, W, H);
    pl->npx = (W + pl->patch - 1) / pl->patch; pl->npy = (H + pl->patch - 1) / pl->patch;
    return ARTGPU_OK;
}

// ImProcFunctions::dehaze on device planes (rows of `stride` floats), enqueued on ctx->stream; the host waits once, for the thumbnail
int dehaze_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const artgpu_dehaze_params *p, const double ws[9],
               const DehazePlan &pl, artgpu_dehaze_info *info)
{
    DhImage im = {{planes[0], planes[1], planes[2]}, stride, W, H};
    const size_t n = (size_t)W * H, nl1 = (size_t)pl.w1 * pl.h1, nl2 = (size_t)pl.w2 * pl.h2, nt = (size_t)pl.ww * pl.hh;
    const size_t nlow = std::max(6 * nl1, 4 * nl2);
    const int npartial = H < DH_MAX_PARTIALS ? H : DH_MAX_PARTIALS;
    float *stf, *thumb, *low, *tmp, *T, *grid;
    int rc;
    if ((rc = pool_get(ctx, P_DH_STATE, (64 + DH_MAX_PARTIALS + 65536) * 4, &stf)) || (rc = pool_get(ctx, P_DH_THUMB, (6 * nt + 16) * 4, &thumb)) ||
        (rc = pool_get(ctx, P_DH_LOW, nlow * 4, &low)) || (rc = pool_get(ctx, P_DH_TMP, nlow * 4, &tmp)) || (rc = pool_get(ctx, P_DH_T, n * 4, &T)) ||
        (rc = pool_get(ctx, P_DH_DARK, (size_t)pl.npx * pl.npy * 4, &grid)))
        return rc;
    DhState *st = reinterpret_cast<DhState *>(stf);
    float *partial = stf + 64, *lut_dev = stf + 64 + DH_MAX_PARTIALS;
    // normalize, subtract_black (L325, L346-348)
    HIPCHK(ctx, launch_dh_max(im, partial, npartial, st, ctx->stream));
    DhThumbArgs ta = {};
    ta.im = im; ta.st = st; ta.thumb = thumb; ta.ww = pl.ww; ta.hh = pl.hh;
    if (p->blackpoint) {
        HIPCHK(ctx, launch_dh_thumb(ta, ctx->stream));
        if ((rc = box_blur_planes(ctx, thumb, thumb + 3 * nt, 3, nt, pl.ww, pl.hh, pl.brad))) return rc;
        HIPCHK(ctx, launch_dh_black(thumb, (int)nt, float(p->blackpoint) / 100.f, st, ctx->stream));
    }
    HIPCHK(ctx, launch_dh_normalize(im, st, p->blackpoint ? 1 : 0, ctx->stream));
    // extract_channels (L369): the statistics of the three self-guided filters; their outputs are evaluated where they are read
    DhGuided g1 = {low, nl1, pl.w1, pl.h1, 1e-1f};
    HIPCHK(ctx, launch_dh_gf_subsample(im, nullptr, 0, g1, ctx->stream));
    if ((rc = box_blur_planes(ctx, low, tmp, 6, nl1, pl.w1, pl.h1, pl.rad1))) return rc;
    HIPCHK(ctx, launch_dh_gf_ab(g1, 1, ctx->stream));
    if ((rc = box_blur_planes(ctx, low, tmp, 6, nl1, pl.w1, pl.h1, pl.rad1))) return rc;
    // the thumbnail (L372-381) and the state block come to the host: the call's one wait
    std::vector<float> host(3 * nt + 8);
    if (nt) {
        ta.gf = g1; ta.from_q = 1;
        HIPCHK(ctx, launch_dh_thumb(ta, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(host.data(), thumb, 3 * nt * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipMemcpyAsync(host.data() + 3 * nt, st, sizeof(DhState), hipMemcpyDeviceToHost, ctx->stream));
    std::vector<float> lut_store;
    const float *lut = dehaze_strength_cached(p, lut_store);         // (while the device works)
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const DhState hs = *reinterpret_cast<const DhState *>(host.data() + 3 * nt);
    float ambient[3];
    const float max_t = dh_estimate_ambient(host.data(), host.data() + nt, host.data() + 2 * nt, pl.ww, pl.hh, ambient);
    const float depth = -float(p->depth) / 100.f;
    const float teps = 1e-6f;
    const float t0 = max_t < 0.f ? 0.f : std::max(teps, std::exp(depth * max_t));           // L453-455, the float overload
    if (info) {
        info->haze_detected = max_t < 0.f ? 0 : 1;
        info->patchsize = pl.patch; info->small_w = pl.ww; info->small_h = pl.hh;
        info->maxval = hs.maxval; info->max_t = max_t; info->t0 = t0;
        for (int k = 0; k < 3; ++k) { info->black[k] = hs.black[k]; info->ambient[k] = ambient[k]; }
    }
    if (max_t < 0.f) {                                                // L387-393: probably no haze at all
        HIPCHK(ctx, launch_dh_restore(im, st, ctx->stream));
        return ARTGPU_OK;
    }
    if ((rc = h2d_table(ctx, lut_dev, lut, 65536 * 4))) return rc;
    // the dark channel (L404) and the transmission estimate (L429-436)
    DhDarkArgs da = {};
    da.im = im; da.gf = g1; da.grid = grid; da.patch = pl.patch; da.npx = pl.npx; da.npy = pl.npy;
    da.has_ambient = 1; da.clip = 1;
    da.per_pixel = (ambient[0] > 0.f && ambient[1] > 0.f && ambient[2] > 0.f) ? 0 : 1;
    for (int k = 0; k < 3; ++k) da.ambient[k] = ambient[k];
    HIPCHK(ctx, launch_dh_dark(da, true, ctx->stream));
    DhTransArgs tr = {};
    tr.im = im; tr.st = st; tr.grid = grid; tr.patch = pl.patch; tr.npx = pl.npx; tr.lut = lut_dev; tr.t = T;
    for (int k = 0; k < 3; ++k) tr.ws1[k] = ws[3 + k];
    HIPCHK(ctx, launch_dh_transmission(tr, ctx->stream));
    // guidedFilter(B, t~, t, 4 * patchsize, 1e-5f) (L438-445): its last step is the first of the recovery pass
    DhGuided g2 = {low, nl2, pl.w2, pl.h2, 1e-5f};
    HIPCHK(ctx, launch_dh_gf_subsample(im, T, (size_t)W, g2, ctx->stream));
    if ((rc = box_blur_planes(ctx, low, tmp, 4, nl2, pl.w2, pl.h2, pl.rad2))) return rc;
    HIPCHK(ctx, launch_dh_gf_ab(g2, 0, ctx->stream));
    if ((rc = box_blur_planes(ctx, low + 2 * nl2, tmp, 2, nl2, pl.w2, pl.h2, pl.rad2))) return rc;
    DhRecoverArgs ra = {};
    ra.im = im; ra.st = st; ra.gf = g2; ra.lut = lut_dev; ra.t0 = t0;
    for (int k = 0; k < 3; ++k) { ra.ws1[k] = ws[3 + k]; ra.ambient[k] = ambient[k]; }
    ra.ambientY = (float)(ambient[0] * ws[3] + ambient[1] * ws[4] + ambient[2] * ws[5]);
    ra.show_depth_map = p->show_depth_map ? 1 : 0; ra.luminance = p->luminance ? 1 : 0;
    HIPCHK(ctx, launch_dh_recover(ra, ctx->stream));
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_dehaze_strength_lut(const double *points, int npoints, float lut[65536])
{
    if (!lut || npoints < 0 || (npoints > 0 && !points)) return ARTGPU_EINVAL;
    dh_strength_lut(points, npoints, lut);
    return ARTGPU_OK;
}

int artgpu_dehaze_estimate_ambient(const float *R, const float *G, const float *B, int ww, int hh, float ambient[3], float *max_t)
{
    if (!R || !G || !B || ww < 1 || hh < 1 || !ambient || !max_t) return ARTGPU_EINVAL;
    *max_t = dh_estimate_ambient(R, G, B, ww, hh, ambient);
    return ARTGPU_OK;
}

int artgpu_dehaze(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_dehaze_params *params, const double ws[9], double scale, artgpu_dehaze_info *info)
{
    StageScope scope_(ctx, "ImProcFunctions::dehaze");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !params) return fail(ctx, ARTGPU_EINVAL, "dehaze: null argument");
    if (info) *info = artgpu_dehaze_info{};
    if (!params->enabled) return ARTGPU_OK;                           // L315-320
    if (!plane_ok(&img->r)) return fail(ctx, ARTGPU_EINVAL, "dehaze: bad plane");
    DehazePlan pl;
    int rc;
    if ((rc = dehaze_check(ctx, img->r.w, img->r.h, params, ws, scale, "dehaze", &pl))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "dehaze"))) return rc;
    if ((rc = dehaze_dev(ctx, d.p, d.stride, d.w, d.h, params, ws, pl, info))) return rc;
    return unbind_rgb(ctx, img, &d);
}

int artgpu_dehaze_dark_channel(artgpu_ctx *ctx, const artgpu_rgb *rgb, int patchsize, const float *ambient, int clip, artgpu_plane *dst)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!rgb || !plane_ok(dst) || !plane_ok(&rgb->r) || dst->w != rgb->r.w || dst->h != rgb->r.h) return fail(ctx, ARTGPU_EINVAL, "dehaze_dark_channel: bad plane");
    if (patchsize < 1 || patchsize > DH_MAX_PATCH) return fail(ctx, ARTGPU_EINVAL, "dehaze_dark_channel: patch size 1..%d", DH_MAX_PATCH);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    int rc;
    if ((rc = bind_rgb(ctx, rgb, 4, true, &d, "dehaze_dark_channel"))) return rc;
    DhDarkArgs da = {};
    da.im = DhImage{{d.p[0], d.p[1], d.p[2]}, d.stride, d.w, d.h};
    da.patch = patchsize; da.npx = (d.w + patchsize - 1) / patchsize; da.npy = (d.h + patchsize - 1) / patchsize;
    da.has_ambient = ambient ? 1 : 0; da.clip = clip ? 1 : 0;
    if (ambient) {
        for (int k = 0; k < 3; ++k) da.ambient[k] = ambient[k];
        da.per_pixel = (ambient[0] > 0.f && ambient[1] > 0.f && ambient[2] > 0.f) ? 0 : 1;
    }
    float *out = dst->p;
    size_t out_stride = (size_t)(dst->row_stride_bytes / 4);
    if ((rc = pool_get(ctx, P_DH_DARK, (size_t)da.npx * da.npy * 4, &da.grid))) return rc;
    if (!dst->on_device) {
        if ((rc = pool_get(ctx, P_DH_T, (size_t)d.w * d.h * 4, &out))) return rc;
        out_stride = d.w;
    }
    HIPCHK(ctx, launch_dh_dark(da, false, ctx->stream));
    DhExpandArgs ea = {da.grid, patchsize, da.npx, out, out_stride, d.w, d.h};
    HIPCHK(ctx, launch_dh_expand(ea, ctx->stream));
    return dst->on_device ? ARTGPU_OK : pool_to_plane(ctx, out, dst);
}

} // extern "C"
