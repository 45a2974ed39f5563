// art_amd/csrc/api_colorcorrection.hip -- colour correction behind the C ABI: ImProcFunctions::colorCorrection (ipcolorcorrection.cc:39-866),
// and the PQ tables it shares with the NEUTRAL tone curve.  The kernels are colorcorrection.hip's.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace artgpu { namespace api {

// the PQ tables of Color::init (P_PQ: forward, inverse, then the NEUTRAL curve's four hue anchors, which belong to the tables' lifetime)
int pq_tables_dev(artgpu_ctx *ctx, float **out)
{
    float *pq;
    int rc;
    const bool fresh = ctx->pool[P_PQ] == nullptr;
    if ((rc = pool_get(ctx, P_PQ, (2 * 65536 + 64) * 4, &pq))) return rc;
    if (fresh) {
        std::vector<float> host(2 * 65536);
        build_pq_luts(host.data(), host.data() + 65536);
        HIPCHK(ctx, hipMemcpyAsync(pq, host.data(), host.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        NeutralArgs a = {};
        a.pq = pq; a.pq_inv = pq + 65536; a.hues = pq + 2 * 65536;
        HIPCHK(ctx, launch_neutral_hues(a, ctx->stream));
    }
    *out = pq;
    return ARTGPU_OK;
}

int cc_check(artgpu_ctx *ctx, int W, int H, const artgpu_color_correction_region *regions, int nregions, const double *ws, const double *iws, bool read_masks,
             const char *who, CcPlan *pl)
{
    if (nregions < 0 || (nregions > 0 && !regions) || !ws || !iws) return fail(ctx, ARTGPU_EINVAL, "%s: bad arguments", who);
    for (int k = 0; k < 9; ++k) { pl->ws[k] = (float)ws[k]; pl->iws[k] = (float)iws[k]; }      // TMatrix -> float ws[3][3], once (L94-108)
    cc_luminance_factors(pl->ws, &pl->fR, &pl->fG, &pl->fB);
    pl->regs.assign(nregions, CcRegion{});
    pl->any_jz = false;
    for (int i = 0; i < nregions; ++i) {
        const artgpu_color_correction_region &r = regions[i];
        if (r.mode == ARTGPU_CC_LUT) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: LUT mode (CLUT files) is not on the device path", who, i);
        if (r.mode < ARTGPU_CC_YUV || r.mode > ARTGPU_CC_LUT) return fail(ctx, ARTGPU_EINVAL, "%s: region %d: mode %d", who, i, r.mode);
        if (r.mode == ARTGPU_CC_HSL && !(r.hsl_gamma > 0.0)) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: hsl_gamma %g", who, i, r.hsl_gamma);
        CcRegionParams p;
        p.mode = r.mode; p.rgbluminance = r.rgbluminance;
        p.a = r.a; p.b = r.b; p.in_saturation = r.in_saturation; p.out_saturation = r.out_saturation; p.hueshift = r.hueshift; p.hsl_gamma = r.hsl_gamma;
        for (int c = 0; c < 3; ++c) {
            p.slope[c] = r.slope[c]; p.offset[c] = r.offset[c]; p.power[c] = r.power[c]; p.pivot[c] = r.pivot[c]; p.compression[c] = r.compression[c];
            p.hue[c] = r.hue[c]; p.sat[c] = r.sat[c]; p.factor[c] = r.factor[c];
        }
        cc_derive_region(p, pl->ws, &pl->regs[i]);
        if (!cc_region_finite(pl->regs[i]))
            return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: a derived scalar is not finite (power 0, pivot 0 or a value out of range)", who, i);
        pl->any_jz = pl->any_jz || pl->regs[i].jzazbz;
        for (const artgpu_plane *m : {r.lmask, r.abmask})
            if (read_masks && m && (!plane_ok(m) || m->w != W || m->h != H)) return fail(ctx, ARTGPU_EINVAL, "%s: region %d: a mask must be a %dx%d plane", who, i, W, H);
    }
    if (!std::isfinite(pl->fR) || !std::isfinite(pl->fG) || !std::isfinite(pl->fB)) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: the working space's luminance row", who);
    return ARTGPU_OK;
}

// the tool on device planes (rows of `stride` floats) in RGB mode, or in YUV mode with `from_yuv`; enqueued on ctx->stream, one host wait with `info`
int color_correction_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const artgpu_color_correction_region *regions,
                         const CcPlan &pl, int from_yuv, int to_rgb, artgpu_color_correction_info *info)
{
    const int n = (int)pl.regs.size();
    const size_t np = (size_t)W * H;
    int rc;
    std::vector<CcRegion> regs = pl.regs;
    // lmask0, abmask0, lmask1, ...: one plane may serve as both masks, and several regions may share one
    std::vector<const artgpu_plane *> masks(2 * n);
    std::vector<const float *> mp(2 * n); std::vector<size_t> ms(2 * n);
    for (int i = 0; i < n; ++i) { masks[2 * i] = regions[i].lmask; masks[2 * i + 1] = regions[i].abmask; }
    if ((rc = bind_planes(ctx, W, H, masks.data(), 2 * n, P_CC_MASK, mp.data(), ms.data()))) return rc;
    for (int i = 0; i < n; ++i) { regs[i].lmask = mp[2 * i]; regs[i].l_stride = ms[2 * i]; regs[i].abmask = mp[2 * i + 1]; regs[i].ab_stride = ms[2 * i + 1]; }
    CcArgs a = {};
    for (int k = 0; k < 3; ++k) a.img[k] = planes[k];
    a.stride = stride; a.w = W; a.h = H;
    for (int k = 0; k < 9; ++k) { a.ws[k] = pl.ws[k]; a.iws[k] = pl.iws[k]; }
    a.fR = pl.fR; a.fG = pl.fG; a.fB = pl.fB;
    if (pl.any_jz) {
        float *pq;
        if ((rc = pq_tables_dev(ctx, &pq))) return rc;
        a.pq = pq; a.pq_inv = pq + 65536;
        cc_pq_low(&a.pq_low, &a.pq_inv_low);
    }
    unsigned long long *count = nullptr;
    if (info && pl.any_jz) {
        float *buf;
        if ((rc = pool_get(ctx, P_CC_OOR, 64 + np, &buf))) return rc;
        HIPCHK(ctx, hipMemsetAsync(buf, 0, 64 + np, ctx->stream));
        count = reinterpret_cast<unsigned long long *>(buf);
        a.oor = reinterpret_cast<unsigned char *>(buf) + 64;
    }
    // launches: up to CC_MAX_REGIONS regions each, cut earlier where Jzazbz and the HSL hue shift would meet (they share no instantiation).
    // The tool is in place and pointwise, so the launches compose: the first does setMode(YUV), the last setMode(RGB)
    int first = 0;
    do {
        int cnt = 0, need = 0;
        while (first + cnt < n && cnt < CC_MAX_REGIONS && cc_need_fits(need | cc_region_need(regs[first + cnt]))) need |= cc_region_need(regs[first + cnt++]);
        for (int k = 0; k < cnt; ++k) a.r[k] = regs[first + k];
        a.nregions = cnt;
        a.from_yuv = first > 0 ? 1 : from_yuv;
        a.to_rgb = first + cnt == n ? to_rgb : 0;
        HIPCHK(ctx, launch_cc(a, need, ctx->stream));
        first += cnt;
    } while (first < n);
    if (info) {
        long long oor = 0;
        if (count) {
            HIPCHK(ctx, launch_cc_count(a.oor, np, count, ctx->stream));
            unsigned long long c = 0;
            HIPCHK(ctx, hipMemcpyAsync(&c, count, 8, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            oor = (long long)c;
        }
        for (int i = 0; i < n; ++i) {
            const CcRegion &r = pl.regs[i];
            artgpu_color_correction_info &o = info[i];
            o = artgpu_color_correction_info{};
            o.abca = r.abca; o.abcb = r.abcb; o.enabled = r.enabled; o.rgbmode = r.rgbmode; o.rhs = r.rhs; o.oor_pixels = oor;
            for (int c = 0; c < 3; ++c) {
                o.slope[c] = r.slope[c]; o.offset[c] = r.offset[c]; o.power[c] = r.power[c]; o.pivot[c] = r.pivot[c];
                o.compression[c][0] = r.comp[c][0]; o.compression[c][1] = r.comp[c][1];
            }
        }
    }
    return ARTGPU_OK;
}

} } // namespace artgpu::api

namespace {

int color_correction_entry(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_color_correction_region *regions, int nregions, const double ws[9], const double iws[9],
                           int from_yuv, int to_rgb, artgpu_color_correction_info *info)
{
    StageScope scope_(ctx, "ImProcFunctions::colorCorrection");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !plane_ok(&img->r)) return fail(ctx, ARTGPU_EINVAL, "color_correction: bad image");
    CcPlan pl;
    int rc;
    if ((rc = cc_check(ctx, img->r.w, img->r.h, regions, nregions, ws, iws, true, "color_correction", &pl))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "color_correction"))) return rc;
    if ((rc = color_correction_dev(ctx, d.p, d.stride, d.w, d.h, regions, pl, from_yuv, to_rgb, info))) return rc;
    return unbind_rgb(ctx, img, &d);
}

} // namespace

extern "C" {

int artgpu_color_correction(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_color_correction_region *regions, int nregions, const double ws[9],
                            const double iws[9], int to_rgb, artgpu_color_correction_info *info)
{
    return color_correction_entry(ctx, img, regions, nregions, ws, iws, 0, to_rgb, info);
}

int artgpu_color_correction_yuv(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_color_correction_region *regions, int nregions, const double ws[9],
                                const double iws[9], int to_rgb, artgpu_color_correction_info *info)
{
    return color_correction_entry(ctx, img, regions, nregions, ws, iws, 1, to_rgb, info);
}

} // extern "C"
