// art_amd/csrc/api_pixelops.hip -- the pixel passes behind the C ABI, in the order a frame meets them: getImage and the colour matrix,
// exposure, the tone curves (STD and NEUTRAL), the Lab mode switches, histogram and adjustments, log encoding, the HSL equalizer, channel
// mixer, rgb2out, scanlines, saturation / vibrance, the RGB curves, and the raw pre-stage's scaleColors.  One launch each; the kernels are
// pixelops.hip's, tonecurve.hip's, lab.hip's, logenc.hip's and hsl.hip's.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace {

// the 65536-entry curve of a tone-curve call -> ctx->lut.  The same curve frame after frame (a batch) is uploaded once: a copy from
// pageable host memory stalls the stream and the enqueueing thread for ~60 us each time.
int upload_curve(artgpu_ctx *ctx, const float *lut65536)
{
    int rc = ensure(ctx, &ctx->lut, &ctx->lut_bytes, 65536 * sizeof(float));
    if (rc) return rc;
    if (ctx->lut_host.size() == 65536 && std::memcmp(ctx->lut_host.data(), lut65536, 65536 * sizeof(float)) == 0) return ARTGPU_OK;
    ctx->lut_host.assign(lut65536, lut65536 + 65536);
    // from the context's own copy: the caller's array may change as soon as this call returns
    hipError_t e = hipMemcpyAsync(ctx->lut, ctx->lut_host.data(), 65536 * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        ctx->lut_host.clear();      // the cache only describes ctx->lut after a copy that succeeded
        return fail(ctx, ARTGPU_EHIP, "tone curve upload failed: %s", hipGetErrorString(e));
    }
    return ARTGPU_OK;
}

int lab_mode_switch(artgpu_ctx *ctx, artgpu_rgb *img, const double m[9], bool to_lab, const char *who)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !m) return fail(ctx, ARTGPU_EINVAL, "%s: null argument", who);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    int rc;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, who))) return rc;
    if ((rc = lab_switch_dev(ctx, d, m, to_lab))) return rc;
    return unbind_rgb(ctx, img, &d);
}

// artgpu_get_image and artgpu_get_image_skip
int get_image_entry(artgpu_ctx *ctx, const artgpu_rgb *planes, int sx1, int sy1, int skip, const float mul[3], int do_clip, const double *mat, artgpu_rgb *image)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!planes || !image || !mul) return fail(ctx, ARTGPU_EINVAL, "get_image: null argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB src, dst;
    int rc;
    if ((rc = bind_rgb(ctx, planes, 1, true, &src, "get_image(planes)")) || (rc = bind_rgb(ctx, image, 4, false, &dst, "get_image(image)")) ||
        (rc = get_image_dev(ctx, src, dst, sx1, sy1, skip, mul, do_clip, mat)))
        return rc;
    return unbind_rgb(ctx, image, &dst);
}

} // namespace

namespace artgpu { namespace api {

int get_image_dev(artgpu_ctx *ctx, const DevRGB &src, const DevRGB &dst, int sx1, int sy1, int skip, const float mul[3], int do_clip, const double *mat)
{
    if (skip < 1 || skip > src.w || skip > src.h) return fail(ctx, ARTGPU_EINVAL, "get_image: skip %d", skip);
    // transformRect (rawimagesource.cc:745-747): the caller's image is ceil(crop / skip); the last window may be pulled back inside
    if (sx1 < 0 || sy1 < 0 || sx1 + (dst.w - 1) * skip >= src.w || sy1 + (dst.h - 1) * skip >= src.h)
        return fail(ctx, ARTGPU_EINVAL, "get_image: crop %dx%d+%d+%d (skip %d) outside the %dx%d planes", dst.w, dst.h, sx1, sy1, skip, src.w, src.h);
    PixArgs a = {};
    for (int k = 0; k < 3; ++k) { a.src[k] = src.p[k]; a.dst[k] = dst.p[k]; a.mul[k] = mul[k]; }
    a.src_stride = src.stride; a.dst_stride = dst.stride;
    a.sx1 = sx1; a.sy1 = sy1; a.w = dst.w; a.h = dst.h;
    a.skip = skip; a.src_w = src.w; a.src_h = src.h;
    a.has_mul = 1; a.do_clip = do_clip ? 1 : 0;
    a.has_mat = mat ? 1 : 0;
    if (mat) for (int k = 0; k < 9; ++k) a.mat[k] = mat[k];
    HIPCHK(ctx, launch_get_image_convert(a, ctx->stream));
    return ARTGPU_OK;
}

int exposure_dev(artgpu_ctx *ctx, const DevRGB &d, float exp_scale, float black)
{
    PixArgs a = {};
    for (int k = 0; k < 3; ++k) a.dst[k] = d.p[k];
    a.dst_stride = d.stride; a.w = d.w; a.h = d.h;
    a.exp_scale = exp_scale; a.black = black;
    HIPCHK(ctx, launch_exposure(a, ctx->stream));
    return ARTGPU_OK;
}

int tone_curve_check(artgpu_ctx *ctx, int mode, float whitept)
{
    if (mode != ARTGPU_TONE_STD) return fail(ctx, ARTGPU_EUNSUPPORTED, "tone_curve: curve mode %d is not on the device path", mode);
    if (!(whitept > 0.f)) return fail(ctx, ARTGPU_EINVAL, "tone_curve: whitept %g", (double)whitept);
    if (whitept > 1.f && ctx->shared.curve_tail_kind == ARTGPU_CURVE_TAIL_HOST)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "tone_curve: whitept %g needs the curve beyond the LUT (artgpu_set_curve_tail)", (double)whitept);
    return ARTGPU_OK;
}

int tone_curve_dev(artgpu_ctx *ctx, const DevRGB &d, const float *lut65536, float whitept, int filmlike_clip)
{
    int rc;
    PixArgs a = {};
    for (int k = 0; k < 3; ++k) a.dst[k] = d.p[k];
    a.dst_stride = d.stride; a.w = d.w; a.h = d.h;
    a.do_clip = filmlike_clip ? 1 : 0; a.whitept = whitept;
    a.tail_kind = ctx->shared.curve_tail_kind == ARTGPU_CURVE_TAIL_HOST ? 0 : ctx->shared.curve_tail_kind; a.tail_y = ctx->shared.curve_tail_y; a.tail_pc = ctx->shared.curve_tail_pc;
    if (lut65536) {
        if ((rc = upload_curve(ctx, lut65536))) return rc;
        a.lut = ctx->lut;
    }
    a.no_lds_lut = !ctx->shared.opt_lut_lds; a.cu_reserve = cu_reserve_of(ctx);
    HIPCHK(ctx, launch_tone_std(a, ctx->stream));
    return ARTGPU_OK;
}

int tone_neutral_check(artgpu_ctx *ctx, const float *lut65536, float whitecoeff)
{
    if (!lut65536 || !(whitecoeff > 0.f)) return fail(ctx, ARTGPU_EINVAL, "tone_curve_neutral: null/invalid argument");
    return ARTGPU_OK;
}

int tone_neutral_dev(artgpu_ctx *ctx, const DevRGB &d, const float *lut65536, float whitecoeff, const artgpu_neutral_state *st)
{
    int rc;
    float *pq;
    if ((rc = pq_tables_dev(ctx, &pq))) return rc;
    if ((rc = upload_curve(ctx, lut65536))) return rc;
    NeutralArgs a = {};
    for (int k = 0; k < 3; ++k) a.img[k] = d.p[k];
    a.stride = d.stride; a.w = d.w; a.h = d.h;
    a.lut = ctx->lut; a.pq = pq; a.pq_inv = pq + 65536; a.hues = pq + 2 * 65536;
    for (int k = 0; k < 9; ++k) { a.ws[k] = (float)st->ws[k]; a.iws[k] = (float)st->iws[k]; a.to_out[k] = st->to_out[k]; a.to_work[k] = st->to_work[k]; }
    a.whitecoeff = whitecoeff;
    a.tail_kind = ctx->shared.curve_tail_kind == ARTGPU_CURVE_TAIL_HOST ? 0 : ctx->shared.curve_tail_kind; a.tail_y = ctx->shared.curve_tail_y; a.tail_pc = ctx->shared.curve_tail_pc;
    a.no_lds_lut = !ctx->shared.opt_lut_lds; a.cu_reserve = cu_reserve_of(ctx);
    HIPCHK(ctx, launch_tone_neutral(a, ctx->stream));
    return ARTGPU_OK;
}

int lab_switch_dev(artgpu_ctx *ctx, const DevRGB &d, const double m[9], bool to_lab)
{
    float *tabs;
    int rc = lab_tabs_dev(ctx, &tabs);
    if (rc) return rc;
    LabArgs a = {};
    for (int k = 0; k < 3; ++k) a.img[k] = d.p[k];
    a.stride = d.stride; a.w = d.w; a.h = d.h;
    for (int k = 0; k < 9; ++k) { a.ws[k] = (float)m[k]; a.iws[k] = (float)m[k]; }
    a.cachef = tabs; a.cachefy = tabs + 65536;
    HIPCHK(ctx, to_lab ? launch_rgb_to_lab(a, ctx->stream) : launch_lab_to_rgb(a, ctx->stream));
    return ARTGPU_OK;
}

int lab_to_yuv_dev(artgpu_ctx *ctx, const DevRGB &d, const double iws[9])
{
    LabArgs a = {};
    for (int k = 0; k < 3; ++k) a.img[k] = d.p[k];
    a.stride = d.stride; a.w = d.w; a.h = d.h;
    for (int k = 0; k < 9; ++k) a.iws[k] = (float)iws[k];
    HIPCHK(ctx, launch_lab_to_yuv(a, ctx->stream));
    return ARTGPU_OK;
}

int scale_args_fill(artgpu_ctx *ctx, int w, int h, int src_is_u16, uint32_t filters, const int32_t *xtrans, const float cblacksom[4], const float scale_mul[4],
                    const char *who, ScaleArgs *a)
{
    a->w = w; a->h = h; a->src_u16 = src_is_u16 ? 1 : 0;
    a->bayer = xtrans ? 0 : 1;
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) {
            int v;
            if (xtrans) v = xtrans[r * 6 + c];
            else v = (filters >> ((((r << 1) & 14) + (c & 1)) << 1)) & 3;      // RawImage::FC, period 2 tiles the 6x6 map
            if (v < 0 || v > 2) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: three-colour CFAs only", who);
            a->cfa[r * 6 + c] = v;
        }
    for (int k = 0; k < 4; ++k) { a->cblacksom[k] = cblacksom[k]; a->scale_mul[k] = scale_mul[k]; }
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_get_image(artgpu_ctx *ctx, const artgpu_rgb *planes, int sx1, int sy1, const float mul[3],
                     int do_clip, const double *mat, artgpu_rgb *image)
{
    StageScope scope_(ctx, "RawImageSource::getImage");
    return get_image_entry(ctx, planes, sx1, sy1, 1, mul, do_clip, mat, image);
}

int artgpu_get_image_skip(artgpu_ctx *ctx, const artgpu_rgb *planes, int sx1, int sy1, int skip, const float mul[3],
                          int do_clip, const double *mat, artgpu_rgb *image)
{
    return get_image_entry(ctx, planes, sx1, sy1, skip, mul, do_clip, mat, image);
}

int artgpu_convert_color_space(artgpu_ctx *ctx, artgpu_rgb *image, const double mat[9])
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!image || !mat) return fail(ctx, ARTGPU_EINVAL, "convert_color_space: null argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    int rc = bind_rgb(ctx, image, 4, true, &d, "convert_color_space");
    if (rc) return rc;
    PixArgs a = {};
    for (int k = 0; k < 3; ++k) { a.src[k] = d.p[k]; a.dst[k] = d.p[k]; }
    a.src_stride = d.stride; a.dst_stride = d.stride; a.w = d.w; a.h = d.h;
    a.has_mul = 0; a.has_mat = 1;
    for (int k = 0; k < 9; ++k) a.mat[k] = mat[k];
    HIPCHK(ctx, launch_get_image_convert(a, ctx->stream));
    return unbind_rgb(ctx, image, &d);
}

int artgpu_exposure(artgpu_ctx *ctx, artgpu_rgb *image, float exp_scale, float black)
{
    StageScope scope_(ctx, "ImProcFunctions::expcomp");
    if (!ctx) return ARTGPU_EINVAL;
    if (!image) return fail(ctx, ARTGPU_EINVAL, "exposure: null image");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    int rc;
    if ((rc = bind_rgb(ctx, image, 4, true, &d, "exposure")) || (rc = exposure_dev(ctx, d, exp_scale, black))) return rc;
    return unbind_rgb(ctx, image, &d);
}

int artgpu_tone_curve(artgpu_ctx *ctx, artgpu_rgb *image, int mode, const float *lut65536, float whitept, int filmlike_clip)
{
    StageScope scope_(ctx, "ImProcFunctions::toneCurve");
    if (!ctx) return ARTGPU_EINVAL;
    if (!image) return fail(ctx, ARTGPU_EINVAL, "tone_curve: null image");
    int rc;
    if ((rc = tone_curve_check(ctx, mode, whitept))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, image, 4, true, &d, "tone_curve")) || (rc = tone_curve_dev(ctx, d, lut65536, whitept, filmlike_clip))) return rc;
    return unbind_rgb(ctx, image, &d);
}

int artgpu_rgb_to_lab(artgpu_ctx *ctx, artgpu_rgb *img, const double ws[9]) { return lab_mode_switch(ctx, img, ws, true, "rgb_to_lab"); }
int artgpu_lab_to_rgb(artgpu_ctx *ctx, artgpu_rgb *img, const double iws[9]) { return lab_mode_switch(ctx, img, iws, false, "lab_to_rgb"); }

int artgpu_lab_to_yuv(artgpu_ctx *ctx, artgpu_rgb *img, const double iws[9])
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !iws) return fail(ctx, ARTGPU_EINVAL, "lab_to_yuv: null argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    int rc;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "lab_to_yuv")) || (rc = lab_to_yuv_dev(ctx, d, iws))) return rc;
    return unbind_rgb(ctx, img, &d);
}

int artgpu_lab_histogram(artgpu_ctx *ctx, const artgpu_rgb *img, uint32_t hist[65536])
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !hist) return fail(ctx, ARTGPU_EINVAL, "lab_histogram: null argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    artgpu_rgb tmp = *img;
    int rc = bind_rgb(ctx, &tmp, 4, true, &d, "lab_histogram");
    if (rc) return rc;
    float *h;
    if ((rc = pool_get(ctx, P_HISTO, 65536 * 4, &h))) return rc;
    LabArgs a = {};
    for (int k = 0; k < 3; ++k) a.img[k] = d.p[k];
    a.stride = d.stride; a.w = d.w; a.h = d.h; a.hist = reinterpret_cast<unsigned *>(h);
    HIPCHK(ctx, hipMemsetAsync(h, 0, 65536 * 4, ctx->stream));
    HIPCHK(ctx, launch_lab_hist(a, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(hist, h, 65536 * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ARTGPU_OK;
}

int artgpu_lab_adjustments(artgpu_ctx *ctx, artgpu_rgb *img, const float *lcurve, const float *acurve, const float *bcurve, float chroma)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !lcurve || !acurve || !bcurve) return fail(ctx, ARTGPU_EINVAL, "lab_adjustments: null argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    int rc = bind_rgb(ctx, img, 4, true, &d, "lab_adjustments");
    if (rc) return rc;
    float *luts;
    constexpr size_t NL = 32772;       // lcurve padded to a multiple of four floats
    if ((rc = pool_get(ctx, P_PIPE_R, (NL + 2 * 65536) * 4, &luts))) return rc;
    if ((rc = h2d_table(ctx, luts, lcurve, 32770 * 4)) || (rc = h2d_table(ctx, luts + NL, acurve, 65536 * 4)) || (rc = h2d_table(ctx, luts + NL + 65536, bcurve, 65536 * 4))) return rc;
    LabArgs a = {};
    for (int k = 0; k < 3; ++k) a.img[k] = d.p[k];
    a.stride = d.stride; a.w = d.w; a.h = d.h;
    a.lcurve = luts; a.acurve = luts + NL; a.bcurve = luts + NL + 65536; a.chroma = chroma;
    HIPCHK(ctx, launch_lab_adjust(a, ctx->stream));
    rc = unbind_rgb(ctx, img, &d);
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));     // the caller's LUTs may go out of scope
    return ARTGPU_OK;
}

int artgpu_log_encoding(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_logenc_params *p, const double ws[9], int full_width, int full_height)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !p || !ws) return fail(ctx, ARTGPU_EINVAL, "log_encoding: null argument");
    if (!p->enabled) return ARTGPU_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LogEncArgs a = {};
    a.gray = std::pow(2.f, -(float)p->gain + std::log2(0.18f));                                   // ev2gray (L119-122)
    a.shadows_range = (float)p->black_ev;
    a.dynamic_range = (float)std::max(p->white_ev - p->black_ev, 0.5);
    const float b = p->target_gray > 1 && p->target_gray < 100 && a.dynamic_range > 0
        ? logenc_find_gray((float)(std::abs(p->black_ev) / a.dynamic_range), (float)(p->target_gray / 100.f)) : 0.f;
    a.linbase = b < 0.f ? 0.f : b;
    a.satcontrol = p->satcontrol ? 1 : 0;
    {   // highlight compression (L148-156): the constants with the host's libm like the reference, the per-pixel curve on the device
        a.hlcompr = p->highlight_compression > 0 ? 1 : 0;
        const float hf = float(p->highlight_compression) / 100.f;
        a.hlcompr_factor = hf < 0.f ? 0.f : (hf > 1.f ? 1.f : hf);
        constexpr float compr_l = 1.01f, compr_t = 0.8f;
        a.compr_p = std::max(a.hlcompr_factor, 0.1f);
        a.compr_s = (compr_l - compr_t) / std::pow(std::pow((1.f - compr_t) / (compr_l - compr_t), -a.compr_p) - 1.f, 1.f / a.compr_p);
    }
    { const float bl = float(p->regularization) / 100.f; a.blend = bl < 0.f ? 0.f : (bl > 1.f ? 1.f : bl); }
    for (int k = 0; k < 3; ++k) a.ws1[k] = ws[3 + k];
    DevRGB d;
    int rc = bind_rgb(ctx, img, 4, true, &d, "log_encoding");
    if (rc) return rc;
    for (int k = 0; k < 3; ++k) a.img[k] = d.p[k];
    a.stride = d.stride; a.w = d.w; a.h = d.h;
    if (p->regularization == 0) {
        HIPCHK(ctx, launch_logenc_direct(a, ctx->stream));
    } else {
        const size_t n = (size_t)d.w * d.h;
        float *Y, *Y2;
        if ((rc = pool_get(ctx, P_DMASK, n * 4, &Y)) || (rc = pool_get(ctx, P_CCMAP, n * 4, &Y2))) return rc;
        a.Y = Y; a.Y2 = Y2;
        HIPCHK(ctx, launch_logenc_prepare(a, ctx->stream));
        const int m1 = full_width > d.w ? full_width : d.w, m2 = full_height > d.h ? full_height : d.h;
        const float radius = (m1 > m2 ? m1 : m2) / 30.f;
        artgpu_plane guide = {Y2, d.w, d.h, (int64_t)d.w * 4, 1}, ypl = {Y, d.w, d.h, (int64_t)d.w * 4, 1};
        if ((rc = artgpu_guided_filter(ctx, &guide, &ypl, &ypl, (int)radius, 0.005f, 0))) return rc;
        HIPCHK(ctx, launch_logenc_blend(a, ctx->stream));
    }
    return unbind_rgb(ctx, img, &d);
}

int artgpu_hsl_equalizer(artgpu_ctx *ctx, artgpu_rgb *img, const double *hcurve, int nh, const double *scurve, int ns,
                         const double *lcurve, int nl, int smoothing, const double ws[9], double scale, int to_rgb)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !ws || !(scale >= 1.0)) return fail(ctx, ARTGPU_EINVAL, "hsl_equalizer: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the four polylines: saturation, luminance, hue (periodic, 1000 / scale points) and the fixed coefficient curve of L125-129
    static const double coeff_pts[9] = {1 /* FCT_MinMaxCPoints */, 0.25, 0.0, 0.5, 0.18, 1, 1, 0, 0.35};
    const double *pts[4] = {scurve, lcurve, hcurve, coeff_pts};
    const int npts[4] = {ns, nl, nh, 9};
    std::vector<double> px[4], py[4], ps[4];
    bool active[4];
    const int ppn = (int)(1000 / scale);
    for (int k = 0; k < 4; ++k) active[k] = pts[k] && flat_curve_polyline(pts[k], npts[k], true, k == 3 ? 1000 : ppn, 0.5, px[k], py[k], ps[k]);
    if (!active[3]) return fail(ctx, ARTGPU_EHIP, "hsl_equalizer: internal curve");
    DevRGB d;
    int rc = bind_rgb(ctx, img, 4, true, &d, "hsl_equalizer");
    if (rc) return rc;
    size_t total = 0;
    for (int k = 0; k < 4; ++k) if (active[k]) total += px[k].size() * 2 + ps[k].size();
    float *tabf, *mask;
    if ((rc = pool_get(ctx, P_PIPE_G, total * 8 + 64, &tabf)) || (rc = pool_get(ctx, P_DMASK, (size_t)d.w * d.h * 4, &mask))) return rc;
    std::vector<double> host(total);
    HslArgs a = {};
    {
        size_t off = 0;
        double *dev = reinterpret_cast<double *>(tabf);
        for (int k = 0; k < 4; ++k) {
            if (!active[k]) continue;
            const size_t n = px[k].size();
            std::copy(px[k].begin(), px[k].end(), host.begin() + off); a.curve[k].x = dev + off; off += n;
            std::copy(py[k].begin(), py[k].end(), host.begin() + off); a.curve[k].y = dev + off; off += n;
            std::copy(ps[k].begin(), ps[k].end(), host.begin() + off); a.curve[k].slope = dev + off; off += ps[k].size();
            a.curve[k].n = (int)n;
        }
        HIPCHK(ctx, hipMemcpyAsync(dev, host.data(), total * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    for (int k = 0; k < 3; ++k) { a.img[k] = d.p[k]; a.ws1[k] = (float)ws[3 + k]; }
    a.stride = d.stride; a.w = d.w; a.h = d.h; a.mask = mask; a.to_rgb = to_rgb ? 1 : 0;
    HIPCHK(ctx, launch_hsl_prepare(a, ctx->stream));
    const float sm = smoothing / 10.f;
    const float smooth = std::pow(10.f, sm < 0.f ? 0.f : (sm > 1.f ? 1.f : sm)) - 1.f;            // L93
    const int radius_small = (int)(4 / scale * smooth + 0.5), radius_large = (int)(25 / scale * smooth + 0.5);
    artgpu_plane guide = {d.p[1], d.w, d.h, (int64_t)d.stride * 4, 1};                             // Y
    artgpu_plane mpl = {mask, d.w, d.h, (int64_t)d.w * 4, 1};
    const int order[3] = {0, 1, 2};                 // saturation, luminance, hue: the reference's order
    for (int k : order) {
        if (!active[k]) continue;
        a.which = k;
        HIPCHK(ctx, launch_hsl_mask(a, ctx->stream));
        const int radius = k == 1 ? radius_large : radius_small;
        const float eps = k == 1 ? 0.0001f : 0.001f;
        if (radius > 0 && (rc = artgpu_guided_filter(ctx, &guide, &mpl, &mpl, radius, eps, 0))) return rc;
        HIPCHK(ctx, launch_hsl_apply(a, ctx->stream));
    }
    HIPCHK(ctx, launch_hsl_finish(a, ctx->stream));
    rc = unbind_rgb(ctx, img, &d);
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // host vector with the polylines goes out of scope
    return ARTGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// NEUTRAL tone curve
// ---------------------------------------------------------------------------------------------
int artgpu_tone_curve_neutral(artgpu_ctx *ctx, artgpu_rgb *image, const float *lut65536, float whitecoeff, const artgpu_neutral_state *st)
{
    StageScope scope_(ctx, "ImProcFunctions::toneCurve (NEUTRAL)");
    if (!ctx) return ARTGPU_EINVAL;
    int rc;
    if ((rc = tone_neutral_check(ctx, image && st ? lut65536 : nullptr, whitecoeff))) return rc;      // (one message for every argument)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, image, 4, true, &d, "tone_curve_neutral")) || (rc = tone_neutral_dev(ctx, d, lut65536, whitecoeff, st))) return rc;
    return unbind_rgb(ctx, image, &d);
}

// ---------------------------------------------------------------------------------------------
// N4: channel mixer, RGB curves
// ---------------------------------------------------------------------------------------------
int artgpu_channel_mixer(artgpu_ctx *ctx, artgpu_rgb *image, const float m[9])
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!image || !m) return fail(ctx, ARTGPU_EINVAL, "channel_mixer: null argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    int rc = bind_rgb(ctx, image, 4, true, &d, "channel_mixer");
    if (rc) return rc;
    MixArgs a = {};
    for (int k = 0; k < 3; ++k) a.dst[k] = d.p[k];
    a.stride = d.stride; a.w = d.w; a.h = d.h;
    for (int k = 0; k < 9; ++k) a.m[k] = m[k];
    HIPCHK(ctx, launch_channel_mixer(a, ctx->stream));
    return unbind_rgb(ctx, image, &d);
}

int artgpu_rgb2out_matrix(artgpu_ctx *ctx, const artgpu_rgb *src, artgpu_rgb *dst, const float matrix[9], int trc_linear,
                          const float *lut, int lutsz)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!src || !dst || !matrix) return fail(ctx, ARTGPU_EINVAL, "rgb2out_matrix: null argument");
    if (!trc_linear && (!lut || lutsz < 2)) return fail(ctx, ARTGPU_EINVAL, "rgb2out_matrix: a non-linear TRC needs its LUT");
    if (lut && (lutsz < 2 || lutsz > 65536)) return fail(ctx, ARTGPU_EINVAL, "rgb2out_matrix: lutsz %d", lutsz);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB s, d;
    int rc = bind_rgb(ctx, src, 1, true, &s, "rgb2out_matrix(src)");
    if (rc) return rc;
    if ((rc = bind_rgb(ctx, dst, 4, false, &d, "rgb2out_matrix(dst)"))) return rc;
    if (s.w != d.w || s.h != d.h) return fail(ctx, ARTGPU_EINVAL, "rgb2out_matrix: size mismatch");
    float *tab;
    if ((rc = pool_get(ctx, P_PIPE_R, (65536 + 16) * 4, &tab))) return rc;
    OutArgs a = {};
    for (int k = 0; k < 3; ++k) { a.src[k] = s.p[k]; a.dst[k] = d.p[k]; }
    a.src_stride = s.stride; a.dst_stride = d.stride; a.w = s.w; a.h = s.h;
    for (int k = 0; k < 9; ++k) a.m[k] = matrix[k];
    a.linear = trc_linear ? 1 : 0;
    a.unsupported = reinterpret_cast<int *>(tab + 65536);
    HIPCHK(ctx, hipMemsetAsync(a.unsupported, 0, 4, ctx->stream));
    if (lut) {
        if ((rc = h2d_table(ctx, tab, lut, (size_t)lutsz * 4))) return rc;
        a.lut = tab; a.lutsz = lutsz;
    }
    HIPCHK(ctx, launch_rgb2out_matrix(a, ctx->stream));
    int bad = 0;
    HIPCHK(ctx, hipMemcpyAsync(&bad, a.unsupported, 4, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = unbind_rgb(ctx, dst, &d))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (bad) return fail(ctx, ARTGPU_EUNSUPPORTED, "rgb2out_matrix: %d channel values above 1 need ARTOutputProfile::eval (lcms2/libm) on the host", bad);
    return ARTGPU_OK;
}

int artgpu_get_scanlines(artgpu_ctx *ctx, const artgpu_rgb *img, int bps, int is_float, void *dst, int64_t dst_row_stride_bytes, int dst_on_device)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !dst) return fail(ctx, ARTGPU_EINVAL, "get_scanlines: null argument");
    const bool okfmt = is_float ? (bps == 16 || bps == 32) : (bps == 8 || bps == 16);
    if (!okfmt) return fail(ctx, ARTGPU_EINVAL, "get_scanlines: bps %d / is_float %d", bps, is_float);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB s;
    int rc = bind_rgb(ctx, img, 4, true, &s, "get_scanlines");
    if (rc) return rc;
    const size_t rowb = (size_t)s.w * 3 * (bps / 8);
    if (dst_row_stride_bytes < (int64_t)rowb) return fail(ctx, ARTGPU_EINVAL, "get_scanlines: row stride %lld < %zu", (long long)dst_row_stride_bytes, rowb);
    OutArgs a = {};
    for (int k = 0; k < 3; ++k) a.src[k] = s.p[k];
    a.src_stride = s.stride; a.w = s.w; a.h = s.h; a.bps = bps; a.is_float = is_float ? 1 : 0;
    float *stage = nullptr;
    if (dst_on_device) { a.out = static_cast<unsigned char *>(dst); a.out_stride_bytes = (size_t)dst_row_stride_bytes; }
    else {
        if ((rc = pool_get(ctx, P_TMP, rowb * s.h + 16, &stage))) return rc;
        a.out = reinterpret_cast<unsigned char *>(stage); a.out_stride_bytes = rowb;
    }
    HIPCHK(ctx, launch_scanlines(a, ctx->stream));
    if (!dst_on_device) {
        HIPCHK(ctx, hipMemcpy2DAsync(dst, (size_t)dst_row_stride_bytes, stage, rowb, rowb, s.h, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return ARTGPU_OK;
}

int artgpu_saturation_vibrance(artgpu_ctx *ctx, artgpu_rgb *image, int saturation, int vibrance, const double ws[9])
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!image || !ws) return fail(ctx, ARTGPU_EINVAL, "saturation_vibrance: null argument");
    if (!saturation && !vibrance) return ARTGPU_OK;            // ipsaturation.cc:45-46
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    int rc = bind_rgb(ctx, image, 4, true, &d, "saturation_vibrance");
    if (rc) return rc;
    SatArgs a = {};
    for (int k = 0; k < 3; ++k) { a.dst[k] = d.p[k]; a.ws1[k] = ws[3 + k]; }
    a.stride = d.stride; a.w = d.w; a.h = d.h;
    a.saturation = 1.f + saturation / 100.f;
    a.vibrance = 1.f - vibrance / 1000.f;
    a.vib = vibrance ? 1 : 0;
    HIPCHK(ctx, launch_saturation_vibrance(a, ctx->stream));
    return unbind_rgb(ctx, image, &d);
}

int artgpu_rgb_curves(artgpu_ctx *ctx, artgpu_rgb *image, const float *rcurve, const float *gcurve, const float *bcurve)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!image) return fail(ctx, ARTGPU_EINVAL, "rgb_curves: null argument");
    if (!rcurve && !gcurve && !bcurve) return ARTGPU_OK;    // all identity: the reference skips the loop (iprgbcurves.cc:110)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    int rc = bind_rgb(ctx, image, 4, true, &d, "rgb_curves");
    if (rc) return rc;
    // The tables live in a pool slot of their own: the host-side cache below describes what the slot holds, so nothing else may write it
    // (P_PIPE_R, where they used to be, is also labAdjustments' curves, rgb2out's TRC table and the pipeline's red plane).
    float *tabs;
    if (ctx->pool_bytes[P_RGBCURVES] < (size_t)3 * 65536 * 4)
        for (int k = 0; k < 3; ++k) ctx->rgbcurve_host[k].clear();           // a fresh allocation holds nothing
    if ((rc = pool_get(ctx, P_RGBCURVES, 3 * 65536 * 4, &tabs))) return rc;
    const float *host[3] = {rcurve, gcurve, bcurve};
    MixArgs a = {};
    for (int k = 0; k < 3; ++k) {
        a.dst[k] = d.p[k];
        if (host[k]) {
            // one rule for every look-up table that crosses the boundary (artgpu.h "Host look-up tables"): the call keeps its own copy and
            // the caller's array is free when the call returns; the same table call after call is uploaded once
            std::vector<float> &own = ctx->rgbcurve_host[k];
            if (own.size() != 65536 || std::memcmp(own.data(), host[k], 65536 * 4) != 0) {
                own.assign(host[k], host[k] + 65536);
                hipError_t e = hipMemcpyAsync(tabs + (size_t)k * 65536, own.data(), 65536 * 4, hipMemcpyHostToDevice, ctx->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
                if (e != hipSuccess) { own.clear(); return fail(ctx, ARTGPU_EHIP, "rgb_curves: curve upload failed: %s", hipGetErrorString(e)); }
            }
            a.lut[k] = tabs + (size_t)k * 65536;
        }
    }
    a.stride = d.stride; a.w = d.w; a.h = d.h;
    HIPCHK(ctx, launch_rgb_curves(a, ctx->stream));
    rc = unbind_rgb(ctx, image, &d);
    if (rc) return rc;
    return ARTGPU_OK;      // (host LUT lifetime: see "Host look-up tables" in artgpu.h)
}

// ---------------------------------------------------------------------------------------------
// raw pre-stage (N2): copyOriginalPixels + scaleColors
// ---------------------------------------------------------------------------------------------
int artgpu_scale_colors(artgpu_ctx *ctx, const void *src, int32_t w, int32_t h, int64_t src_row_stride_bytes, int32_t src_is_u16,
                        int32_t src_on_device, uint32_t filters, const int32_t *xtrans, const float cblacksom[4],
                        const float scale_mul[4], artgpu_plane *dst, float chmax[4])
{
    if (!ctx) return ARTGPU_EINVAL;
    const int esz = src_is_u16 ? 2 : 4;
    if (!src || !dst || !plane_ok(dst) || !cblacksom || !scale_mul || w <= 0 || h <= 0 || dst->w != w || dst->h != h ||
        src_row_stride_bytes < (int64_t)w * esz || src_row_stride_bytes % esz)
        return fail(ctx, ARTGPU_EINVAL, "scale_colors: bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    ScaleArgs a = {};
    // source: device pointer as is, host buffer staged (2 or 4 bytes per pixel over PCIe)
    if (src_on_device) { a.src = src; a.src_stride = (size_t)(src_row_stride_bytes / esz); }
    else {
        float *st;
        if ((rc = pool_get(ctx, P_PIPE_B, (size_t)w * h * esz, &st))) return rc;
        HIPCHK(ctx, hipMemcpy2DAsync(st, (size_t)w * esz, src, (size_t)src_row_stride_bytes, (size_t)w * esz, h, hipMemcpyHostToDevice, ctx->stream));
        a.src = st; a.src_stride = w;
    }
    float *out;
    if (dst->on_device) { out = dst->p; a.dst_stride = (size_t)(dst->row_stride_bytes / 4); }
    else { if ((rc = pool_get(ctx, P_PIPE_G, (size_t)w * h * 4, &out))) return rc; a.dst_stride = w; }
    a.dst = out;
    if ((rc = scale_args_fill(ctx, w, h, src_is_u16, filters, xtrans, cblacksom, scale_mul, "scale_colors", &a))) return rc;
    float *mx;
    if ((rc = pool_get(ctx, P_MAD, 3 * 32 * 4, &mx))) return rc;
    a.chmax_bits = reinterpret_cast<int *>(mx);
    HIPCHK(ctx, hipMemsetAsync(mx, 0, 4 * sizeof(int), ctx->stream));
    HIPCHK(ctx, launch_scale_colors(a, ctx->stream));
    if (!dst->on_device)
        HIPCHK(ctx, hipMemcpy2DAsync(dst->p, (size_t)dst->row_stride_bytes, out, (size_t)w * 4, (size_t)w * 4, h, hipMemcpyDeviceToHost, ctx->stream));
    if (chmax) {
        float host[4];
        HIPCHK(ctx, hipMemcpyAsync(host, mx, 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        chmax[0] = host[0]; chmax[1] = host[1]; chmax[2] = host[2]; chmax[3] = host[1];
    } else if (!dst->on_device) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return ARTGPU_OK;
}

} // extern "C"
