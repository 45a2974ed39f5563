// art_amd/csrc/api_wavelet.hip -- wavelet_decomposition behind the C ABI: the decomposition handle of the public entry points and the
// pool-backed decomposition (DevDecomp, api_internal.h) that RGB_denoise and local contrast run.  The kernels are wavelet.hip's; MadRgb is
// denoise.hip's.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

struct artgpu_wavelet {
    int w = 0, h = 0, w2 = 0, h2 = 0, nlevels = 0;
    float *bands = nullptr;   // nlevels * 3 * n floats
    float *lowpass[2] = {nullptr, nullptr};
    int cur = 0;              // lowpass[cur] is coeff0
    size_t n = 0;
    float *band(int l, int dir) const { return bands + ((size_t)l * 3 + (dir - 1)) * n; }
};

namespace artgpu { namespace api {

int wavelet_skip(int level) { return level <= 1 ? 1 : 1 << (level - 1); }

int decompose_dev(artgpu_ctx *ctx, DevDecomp &d, const float *src, hipStream_t st, size_t src_stride)
{
    if (!st) st = ctx->stream;
    WaveArgs a = {};
    a.w = d.w; a.h = d.h; a.w2 = d.w2; a.h2 = d.h2;
    if (d.cnt) HIPCHK(ctx, hipMemsetAsync(d.cnt, 0, (size_t)3 * d.nlevels * MAD_FOLD_NB * sizeof(int), st));
    for (int l = 0; l < d.nlevels; ++l) {
        a.cnt = d.cnt ? d.cnt + (size_t)l * 3 * MAD_FOLD_NB : nullptr;
        a.b1 = d.band(l, 1); a.b2 = d.band(l, 2); a.b3 = d.band(l, 3);
        if (l == 0) {
            a.src = src; a.src_stride = src_stride ? src_stride : (size_t)d.w; a.lo = d.low[0]; d.cur = 0;
            a.cnt_grid = d.g0;
            HIPCHK(ctx, d.cnt ? launch_wavelet_analysis0_count(a, st) : launch_wavelet_analysis0(a, st));
        } else {
            a.src = d.low[d.cur]; a.lo = d.low[d.cur ^ 1]; a.skip = wavelet_skip(l);
            a.cnt_grid = d.g1;
            HIPCHK(ctx, d.cnt ? launch_wavelet_haar_analysis_count(a, st) : launch_wavelet_haar_analysis(a, st));
            d.cur ^= 1;
        }
    }
    return ARTGPU_OK;
}

int reconstruct_dev(artgpu_ctx *ctx, DevDecomp &d, float *dst, hipStream_t st)
{
    if (!st) st = ctx->stream;
    WaveArgs a = {};
    a.w = d.w; a.h = d.h; a.w2 = d.w2; a.h2 = d.h2; a.blend = 1.f;
    for (int l = d.nlevels - 1; l > 0; --l) {
        a.src = d.low[d.cur]; a.lo = d.low[d.cur ^ 1];
        a.b1 = d.band(l, 1); a.b2 = d.band(l, 2); a.b3 = d.band(l, 3); a.skip = wavelet_skip(l);
        HIPCHK(ctx, launch_wavelet_haar_synthesis(a, st));
        d.cur ^= 1;
    }
    a.src = d.low[d.cur];
    a.b1 = d.band(0, 1); a.b2 = d.band(0, 2); a.b3 = d.band(0, 3);
    a.dst = dst; a.dst_stride = d.w;
    HIPCHK(ctx, launch_wavelet_synthesis0(a, st));
    return ARTGPU_OK;
}

} } // namespace artgpu::api

// a decomposition handle's end: behind whatever the context's stream still does with its buffers
static void wavelet_release(artgpu_ctx *ctx, artgpu_wavelet *wv)
{
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
    if (wv->bands) (void)hipFree(wv->bands);
    if (wv->lowpass[0]) (void)hipFree(wv->lowpass[0]);
    if (wv->lowpass[1]) (void)hipFree(wv->lowpass[1]);
    delete wv;
}

extern "C" {

int artgpu_wavelet_decompose(artgpu_ctx *ctx, const artgpu_plane *src, int maxlvl, artgpu_wavelet **out)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(src) || !out || maxlvl < 1 || maxlvl > 9) return fail(ctx, ARTGPU_EINVAL, "wavelet_decompose: bad arguments");
    *out = nullptr;
    const int w = src->w, h = src->h, w2 = (w + 1) / 2, h2 = (h + 1) / 2;
    if ((w2 < h2 ? w2 : h2) < 2 * wavelet_skip(maxlvl - 1) || w < 8 || h < 8)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "wavelet_decompose: %dx%d too small for %d levels", w, h, maxlvl);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const float *dsrc = src->p;
    size_t sstride = (size_t)(src->row_stride_bytes / 4);
    if (!src->on_device) {
        int rc = ensure(ctx, &ctx->stage[0], &ctx->stage_bytes[0], (size_t)w * h * 4);
        if (rc) return rc;
        HIPCHK(ctx, hipMemcpy2DAsync(ctx->stage[0], (size_t)w * 4, src->p, (size_t)src->row_stride_bytes, (size_t)w * 4, h, hipMemcpyHostToDevice, ctx->stream));
        dsrc = ctx->stage[0];
        sstride = w;
    }
    artgpu_wavelet *wv = new (std::nothrow) artgpu_wavelet;
    if (!wv) return fail(ctx, ARTGPU_ENOMEM, "wavelet_decompose: out of host memory");
    wv->w = w; wv->h = h; wv->w2 = w2; wv->h2 = h2; wv->nlevels = maxlvl; wv->n = (size_t)w2 * h2;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&wv->bands), (size_t)maxlvl * 3 * wv->n * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&wv->lowpass[0]), wv->n * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&wv->lowpass[1]), wv->n * sizeof(float));
    if (e != hipSuccess) {
        wavelet_release(ctx, wv);
        return fail(ctx, ARTGPU_ENOMEM, "wavelet_decompose: hipMalloc failed: %s", hipGetErrorString(e));
    }
    WaveArgs a = {};
    a.w = w; a.h = h; a.w2 = w2; a.h2 = h2;
    for (int l = 0; l < maxlvl; ++l) {
        a.b1 = wv->band(l, 1); a.b2 = wv->band(l, 2); a.b3 = wv->band(l, 3);
        hipError_t le;
        if (l == 0) {
            a.src = dsrc; a.src_stride = sstride; a.lo = wv->lowpass[0];
            wv->cur = 0;
            le = launch_wavelet_analysis0(a, ctx->stream);
        } else {
            a.src = wv->lowpass[wv->cur]; a.lo = wv->lowpass[wv->cur ^ 1]; a.skip = wavelet_skip(l);
            le = launch_wavelet_haar_analysis(a, ctx->stream);
            wv->cur ^= 1;
        }
        if (le != hipSuccess) {
            wavelet_release(ctx, wv);
            return fail(ctx, ARTGPU_EHIP, "wavelet_decompose: launch failed: %s", hipGetErrorString(le));
        }
    }
    if (!src->on_device) {
        const hipError_t se = hipStreamSynchronize(ctx->stream);
        if (se != hipSuccess) {
            wavelet_release(ctx, wv);
            return fail(ctx, ARTGPU_EHIP, "wavelet_decompose: %s", hipGetErrorString(se));
        }
    }
    *out = wv;
    return ARTGPU_OK;
}

int artgpu_wavelet_info(const artgpu_wavelet *wv, int32_t *w2, int32_t *h2, int32_t *nlevels)
{
    if (!wv) return ARTGPU_EINVAL;
    if (w2) *w2 = wv->w2;
    if (h2) *h2 = wv->h2;
    if (nlevels) *nlevels = wv->nlevels;
    return ARTGPU_OK;
}

int artgpu_wavelet_get_band(artgpu_ctx *ctx, const artgpu_wavelet *wv, int level, int dir, float *dst, int on_device)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!wv || !dst || dir < 0 || dir > 3 || (dir > 0 && (level < 0 || level >= wv->nlevels))) return fail(ctx, ARTGPU_EINVAL, "wavelet_get_band: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const float *p = dir == 0 ? wv->lowpass[wv->cur] : wv->band(level, dir);
    HIPCHK(ctx, hipMemcpyAsync(dst, p, wv->n * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    if (!on_device) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ARTGPU_OK;
}

int artgpu_wavelet_set_band(artgpu_ctx *ctx, artgpu_wavelet *wv, int level, int dir, const float *src, int on_device)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!wv || !src || dir < 0 || dir > 3 || (dir > 0 && (level < 0 || level >= wv->nlevels))) return fail(ctx, ARTGPU_EINVAL, "wavelet_set_band: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    float *p = dir == 0 ? wv->lowpass[wv->cur] : wv->band(level, dir);
    HIPCHK(ctx, hipMemcpyAsync(p, src, wv->n * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    if (!on_device) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ARTGPU_OK;
}

int artgpu_wavelet_reconstruct(artgpu_ctx *ctx, artgpu_wavelet *wv, artgpu_plane *dst, float blend)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!wv || !plane_ok(dst) || dst->w != wv->w || dst->h != wv->h) return fail(ctx, ARTGPU_EINVAL, "wavelet_reconstruct: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    float *ddst = dst->p;
    size_t dstride = (size_t)(dst->row_stride_bytes / 4);
    if (!dst->on_device) {
        int rc = ensure(ctx, &ctx->stage[0], &ctx->stage_bytes[0], (size_t)wv->w * wv->h * 4);
        if (rc) return rc;
        // dst participates in the blend (dst*(1-blend) + blend*4*tot): bring the host contents over
        HIPCHK(ctx, hipMemcpy2DAsync(ctx->stage[0], (size_t)wv->w * 4, dst->p, (size_t)dst->row_stride_bytes, (size_t)wv->w * 4, wv->h, hipMemcpyHostToDevice, ctx->stream));
        ddst = ctx->stage[0];
        dstride = wv->w;
    }
    WaveArgs a = {};
    a.w = wv->w; a.h = wv->h; a.w2 = wv->w2; a.h2 = wv->h2; a.blend = blend;
    for (int l = wv->nlevels - 1; l > 0; --l) {
        a.src = wv->lowpass[wv->cur]; a.lo = wv->lowpass[wv->cur ^ 1];
        a.b1 = wv->band(l, 1); a.b2 = wv->band(l, 2); a.b3 = wv->band(l, 3); a.skip = wavelet_skip(l);
        HIPCHK(ctx, launch_wavelet_haar_synthesis(a, ctx->stream));
        wv->cur ^= 1;
    }
    a.src = wv->lowpass[wv->cur];
    a.b1 = wv->band(0, 1); a.b2 = wv->band(0, 2); a.b3 = wv->band(0, 3);
    a.dst = ddst; a.dst_stride = dstride;
    HIPCHK(ctx, launch_wavelet_synthesis0(a, ctx->stream));
    if (!dst->on_device) {
        HIPCHK(ctx, hipMemcpy2DAsync(dst->p, (size_t)dst->row_stride_bytes, ddst, (size_t)wv->w * 4, (size_t)wv->w * 4, wv->h, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return ARTGPU_OK;
}

int artgpu_wavelet_free(artgpu_ctx *ctx, artgpu_wavelet *wv)
{
    if (!wv) return ARTGPU_EINVAL;
    wavelet_release(ctx, wv);
    return ARTGPU_OK;
}

int artgpu_wavelet_mad(artgpu_ctx *ctx, const artgpu_wavelet *wv, float *mad_sqr)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!wv || !mad_sqr) return fail(ctx, ARTGPU_EINVAL, "wavelet_mad: null argument");
    if (wv->n > 0x7fffffff) return fail(ctx, ARTGPU_EUNSUPPORTED, "wavelet_mad: band larger than an int holds (MadRgb's datalen is an int)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int nsub = 3 * wv->nlevels;
    float *histo_f, *mad;
    int rc;
    if ((rc = pool_get(ctx, P_HISTO, (size_t)nsub * (65536 + MAD_SCRATCH_INTS_PER_BAND) * 4, &histo_f)) || (rc = pool_get(ctx, P_MAD, 3 * 32 * 4, &mad))) return rc;
    HIPCHK(ctx, launch_mad(wv->bands, wv->n, nsub, reinterpret_cast<int *>(histo_f), mad, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(mad_sqr, mad, (size_t)nsub * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ARTGPU_OK;
}

} // extern "C"
