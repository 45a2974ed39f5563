// art_amd/csrc/api_resize.hip -- the Resize tool behind the C ABI: ImProcFunctions::Lanczos (rtengine/ipresize.cc:53-223), resizeScale
// (L226-297) and the pipe's setting.  The kernel is resize.hip's; the weight tables are built here, on the host, with the reference's float
// expressions (this file is compiled with -ffp-contract=off like every other).
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace {

// xsinf (sleef.h:993-1016): the scalar form, xrintf being cvtss2si (round to nearest even) under SSE2
inline float rs_mla(float x, float y, float z) { return x * y + z; }
float rs_xsinf(float d)
{
    const int q = (int)std::nearbyintf(d * (float)0.318309886183790671538);
    d = rs_mla((float)q, -0.78515625f * 4, d);
    d = rs_mla((float)q, -0.00024127960205078125f * 4, d);
    d = rs_mla((float)q, -6.3329935073852539062e-07f * 4, d);
    d = rs_mla((float)q, -4.9604681473525147339e-10f * 4, d);
    const float s = d * d;
    if ((q & 1) != 0) d = -d;
    float u = 2.6083159809786593541503e-06f;
    u = rs_mla(u, s, -0.0001981069071916863322258f);
    u = rs_mla(u, s, 0.00833307858556509017944336f);
    u = rs_mla(u, s, -0.166666597127914428710938f);
    return rs_mla(s, u * d, d);
}

// Lanc (ipresize.cc:38-48)
float rs_lanc(float x, float a)
{
    if (x * x < 1e-6f) return 1.0f;
    if (x * x > a * a) return 0.0f;
    x = static_cast<float>(3.14159265358979323846) * x;
    return a * rs_xsinf(x) * rs_xsinf(x / a) / (x * x);
}

// Phase 1 of Lanczos (L83-109) for one direction: n destination positions over `len` source positions.  w: n rows of `support` floats
// (entries behind a row's taps are 0; the reference leaves them unread), first / last: the tap ranges
void rs_weights(int n, int len, float scale, int support, float *w, int *first, int *last)
{
    const float delta = 1.0f / scale;
    const float a = 3.0f;
    const float sc = std::min(scale, 1.0f);
    for (int j = 0; j < n; j++) {
        const float x0 = (static_cast<float>(j) + 0.5f) * delta - 0.5f;
        float *wj = w + (size_t)j * support;
        float ws = 0.0f;
        first[j] = std::max(0, static_cast<int>(floorf(x0 - a / sc)) + 1);
        last[j] = std::min(len, static_cast<int>(floorf(x0 + a / sc)) + 1);
        for (int k = 0; k < support; k++) wj[k] = 0.0f;
        for (int jj = first[j]; jj < last[j] && jj - first[j] < support; jj++) {
            const int k = jj - first[j];
            const float z = sc * (x0 - static_cast<float>(jj));
            wj[k] = rs_lanc(z, a);
            ws += wj[k];
        }
        for (int k = 0; k < last[j] - first[j] && k < support; k++) wj[k] /= ws;
    }
}

// the largest tile width (destination columns per workgroup) whose columns' taps lie within RS_SPAN source columns in every tile; 0: none
int rs_tile_width(const int *jj0, const int *jj1, int dW, int sW)
{
    for (int tw = std::min(RS_MAX_TILE_W, dW); tw >= 1; --tw) {
        bool fits = true;
        for (int c0 = 0; c0 < dW && fits; c0 += tw) {
            const int c1 = std::min(c0 + tw, dW), lo = std::min(jj0[c0], sW), hi = std::max(std::min(jj1[c1 - 1], sW), lo);
            fits = hi - lo <= RS_SPAN;
        }
        if (fits) return tw;
    }
    return 0;
}

bool rs_scale_ok(float scale) { return std::isfinite(scale) && scale > 0.f && scale != 1.0f; }

} // namespace

namespace artgpu { namespace api {

// The host copy of the tables, as 4-byte words: [ii0 dH | ii1 dH | jj0 dW | jj1 dW | wv dH x support | wh dW x support]
int rs_check(artgpu_ctx *ctx, int sW, int sH, int dW, int dH, float scale, const char *who)
{
    if (!rs_scale_ok(scale)) return fail(ctx, ARTGPU_EINVAL, "%s: scale %g (1 is \"no resize\"; it has to be finite and positive)", who, (double)scale);
    if (sW < 1 || sH < 1 || dW < 1 || dH < 1) return fail(ctx, ARTGPU_EINVAL, "%s: %dx%d -> %dx%d", who, sW, sH, dW, dH);
    const int key[4] = {sW, sH, dW, dH};
    if (!ctx->rs_host.empty() && !memcmp(key, ctx->rs_key, sizeof key) && !memcmp(&scale, &ctx->rs_key_scale, 4)) return ARTGPU_OK;
    const float sc = std::min(scale, 1.0f);
    const float fsupport = 2.0f * 3.0f / sc;
    if (!(fsupport < (float)(2 * RS_SPAN))) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: scale %g needs %g taps per pixel", who, (double)scale, (double)fsupport);
    const int support = static_cast<int>(fsupport) + 1;
    std::vector<int> tab((size_t)2 * dH + 2 * dW + (size_t)support * (dH + dW));
    int *ii0 = tab.data(), *ii1 = ii0 + dH, *jj0 = ii1 + dH, *jj1 = jj0 + dW;
    float *wv = reinterpret_cast<float *>(jj1 + dW), *wh = wv + (size_t)support * dH;
    rs_weights(dH, sH, scale, support, wv, ii0, ii1);
    rs_weights(dW, sW, scale, support, wh, jj0, jj1);
    for (int i = 0; i < dH; ++i)
        if (ii1[i] - ii0[i] > support) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: row %d has more taps than the support (%d)", who, i, support);
    for (int j = 0; j < dW; ++j)
        if (jj1[j] - jj0[j] > support) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: column %d has more taps than the support (%d)", who, j, support);
    const int tw = rs_tile_width(jj0, jj1, dW, sW);
    if (tw < std::min(RS_MIN_TILE_W, dW))
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: scale %g: the taps of %d neighbouring columns (support %d) do not lie within %d source columns", who,
                    (double)scale, RS_MIN_TILE_W, support, RS_SPAN);
    ctx->rs_host.swap(tab);
    memcpy(ctx->rs_key, key, sizeof key); ctx->rs_key_scale = scale;
    ctx->rs_support = support; ctx->rs_tile_w = tw;
    ctx->rs_dev = nullptr;
    return ARTGPU_OK;
}

int resize_dev(artgpu_ctx *ctx, const DevRGB &src, const DevRGB &dst, float scale, const double *m_in, const double *m_out)
{
    const int sW = src.w, sH = src.h, dW = dst.w, dH = dst.h;
    const int key[4] = {sW, sH, dW, dH};
    if (ctx->rs_host.empty() || memcmp(key, ctx->rs_key, sizeof key) || memcmp(&scale, &ctx->rs_key_scale, 4))
        return fail(ctx, ARTGPU_EINVAL, "resize: the tables were built for another call");
    float *dev;
    int rc = pool_get(ctx, P_RS_TAB, ctx->rs_host.size() * 4, &dev);
    if (rc) return rc;
    if (ctx->rs_dev != dev) {
        ctx->rs_dev = nullptr;
        if ((rc = h2d_table(ctx, dev, ctx->rs_host.data(), ctx->rs_host.size() * 4))) return rc;
        ctx->rs_dev = dev;
    }
    if (m_in && (rc = lab_switch_dev(ctx, src, m_in, true))) return rc;
    RsArgs a = {};
    for (int k = 0; k < 3; ++k) { a.src[k] = src.p[k]; a.dst[k] = dst.p[k]; }
    a.sstride = src.stride; a.dstride = dst.stride;
    a.sW = sW; a.sH = sH; a.dW = dW; a.dH = dH;
    a.support = ctx->rs_support; a.tile_w = ctx->rs_tile_w;
    const int *words = reinterpret_cast<const int *>(dev);
    a.ii0 = words; a.ii1 = a.ii0 + dH; a.jj0 = a.ii1 + dH; a.jj1 = a.jj0 + dW;
    a.wv = reinterpret_cast<const float *>(a.jj1 + dW); a.wh = a.wv + (size_t)a.support * dH;
    HIPCHK(ctx, launch_resize_lanczos(a, scale < 1.0f, ctx->stream));
    if (m_out && (rc = lab_switch_dev(ctx, dst, m_out, false))) return rc;
    return ARTGPU_OK;
}

bool pipeline_resize(const artgpu_ctx *ctx, int w, int h, int *imw, int *imh, float *scale)
{
    const artgpu_ctx::Shared &s = ctx->shared;
    *imw = w; *imh = h; *scale = 1.0f;
    if (!s.pipe_rs_on || !s.pipe_rs.enabled) return false;
    (void)artgpu_resize_scale(&s.pipe_rs, w, h, imw, imh, scale);
    // simpleprocess.cc:406-407
    if (*scale < 1.0f || (*scale > 1.0f && (s.pipe_rs.allow_upscaling || s.pipe_rs.dataspec == 0))) return true;
    *imw = w; *imh = h;
    return false;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_resize_scale(const artgpu_resize_params *p, int fw, int fh, int *imw, int *imh, float *scale)
{
    if (!imw || !imh || !scale) return ARTGPU_EINVAL;
    *imw = fw; *imh = fh; *scale = 1.0f;
    if (!p || !p->enabled) return ARTGPU_OK;
    const int refw = fw, refh = fh;
    double dScale;
    switch (p->dataspec) {
    case 1: dScale = (double)p->width / (double)refw; break;
    case 2: dScale = (double)p->height / (double)refh; break;
    case 3:
        if ((double)refw / (double)refh > (double)p->width / (double)p->height) dScale = (double)p->width / (double)refw;
        else dScale = (double)p->height / (double)refh;
        dScale = (dScale > 1.0 && !p->allow_upscaling) ? 1.0 : dScale;
        break;
    default: dScale = p->scale; break;
    }
    if (fabs(dScale - 1.0) <= 1e-5) return ARTGPU_OK;
    *imw = (int)((double)refw * dScale + 0.5);
    *imh = (int)((double)refh * dScale + 0.5);
    *scale = (float)dScale;
    return ARTGPU_OK;
}

int artgpu_resize_lanczos(artgpu_ctx *ctx, artgpu_rgb *src, artgpu_rgb *dst, float scale, int mode, const double ws[9], const double iws[9])
{
    StageScope scope_(ctx, "ImProcFunctions::Lanczos");
    if (!ctx) return ARTGPU_EINVAL;
    if (!src || !dst || !plane_ok(&src->r) || !plane_ok(&dst->r)) return fail(ctx, ARTGPU_EINVAL, "resize_lanczos: bad arguments");
    if (mode != ARTGPU_RESIZE_PLANES && mode != ARTGPU_RESIZE_RGB) return fail(ctx, ARTGPU_EINVAL, "resize_lanczos: mode %d", mode);
    if (mode == ARTGPU_RESIZE_RGB && (!ws || !iws)) return fail(ctx, ARTGPU_EINVAL, "resize_lanczos: RGB mode needs ws and iws");
    int rc;
    if ((rc = rs_check(ctx, src->r.w, src->r.h, dst->r.w, dst->r.h, scale, "resize_lanczos"))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB s, d;
    if ((rc = bind_rgb(ctx, src, 4, true, &s, "resize_lanczos(src)")) || (rc = bind_rgb(ctx, dst, 1, false, &d, "resize_lanczos(dst)"))) return rc;
    const bool rgb = mode == ARTGPU_RESIZE_RGB;
    if ((rc = resize_dev(ctx, s, d, scale, rgb ? ws : nullptr, rgb ? iws : nullptr))) return rc;
    return unbind_rgb(ctx, dst, &d);
}

int artgpu_set_pipeline_resize(artgpu_ctx *ctx, const artgpu_resize_params *p)
{
    if (!ctx) return ARTGPU_EINVAL;
    ctx->shared.pipe_rs_on = p ? 1 : 0;
    ctx->shared.pipe_rs = p ? *p : artgpu_resize_params{};
    return ARTGPU_OK;
}

} // extern "C"
