// art_amd/csrc/api_localcontrast.hip -- ImProcFunctions::localContrast behind the C ABI: the regions' wavelet decomposition, statistics, remap and
// blend on the L plane, and the host-only curve table.  The kernels are localcontrast.hip's, the decomposition is api_wavelet.hip's.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace artgpu { namespace api {

// what the call cannot do, before anything is touched: 0, or the code with the message set
int local_contrast_check(artgpu_ctx *ctx, int w, int h, const artgpu_local_contrast_region *regions, int nregions, double scale, const char *who)
{
    if (nregions < 0 || (nregions > 0 && !regions)) return fail(ctx, ARTGPU_EINVAL, "%s: bad region list", who);
    for (int r = 0; r < nregions; ++r) {
        const artgpu_plane *m = regions[r].mask;
        if (m && (!plane_ok(m) || m->w != w || m->h != h)) return fail(ctx, ARTGPU_EINVAL, "%s: the mask of region %d must be a %dx%d plane", who, r, w, h);
    }
    if (scale != 1.0) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: scale %g (the skip form of the wavelet is not on the device path)", who, scale);
    if (w < ARTGPU_LOCAL_CONTRAST_MIN_SIZE || h < ARTGPU_LOCAL_CONTRAST_MIN_SIZE)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: %dx%d is below %dx%d", who, w, h, ARTGPU_LOCAL_CONTRAST_MIN_SIZE, ARTGPU_LOCAL_CONTRAST_MIN_SIZE);
    const int nl = lc_wavelet_levels(w, h), w2 = (w + 1) / 2, h2 = (h + 1) / 2;
    if ((w2 < h2 ? w2 : h2) < 2 * wavelet_skip(nl - 1))       // the wavelet kernels' own limit: never reached by the level rule from 8x8 up
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: %dx%d too small for %d wavelet levels on the device path", who, w, h, nl);
    return ARTGPU_OK;
}

// the regions of ImProcFunctions::localContrast (L463-481) on a device L plane (rows of `stride` floats), enqueued on ctx->stream; per
// region the host waits once, for the statistics block it computes the constants of L372-380 from
int local_contrast_dev(artgpu_ctx *ctx, float *L, size_t stride, int w, int h, const artgpu_local_contrast_region *regions, int nregions,
                              artgpu_local_contrast_info *info)
{
    DevDecomp d = {};
    d.w = w; d.h = h; d.w2 = (w + 1) / 2; d.h2 = (h + 1) / 2; d.nlevels = lc_wavelet_levels(w, h);
    d.n = (size_t)d.w2 * d.h2;
    if (d.n > 0x7fffffff) return fail(ctx, ARTGPU_EUNSUPPORTED, "local_contrast: band larger than an int holds (the reference's W_L * H_L is an int)");
    const int nbands = 3 * d.nlevels, nchunk = (int)((d.n + LC_CHUNK - 1) / LC_CHUNK);
    // statistics block: results | curve | partial sums | counts | maxima | minima
    const size_t res_bytes = 32 * sizeof(LcSegStats), curve_bytes = 512 * 4, np = (size_t)(nbands + 1) * nchunk;
    float *Lnew, *stats;
    int rc;
    if ((rc = pool_get(ctx, P_LC_BANDS, (size_t)nbands * d.n * 4, &d.bands)) || (rc = pool_get(ctx, P_LC_LOW0, d.n * 4, &d.low[0])) ||
        (rc = pool_get(ctx, P_LC_LOW1, d.n * 4, &d.low[1])) || (rc = pool_get(ctx, P_LC_NEW, (size_t)w * h * 4, &Lnew)) ||
        (rc = pool_get(ctx, P_LC_STATS, res_bytes + curve_bytes + np * (8 + 4 + 4 + 4), &stats)))
        return rc;
    char *sb = reinterpret_cast<char *>(stats);
    LcStatArgs sa = {};
    sa.bands = d.bands; sa.n = d.n; sa.nbands = nbands; sa.nchunk = nchunk;
    sa.res = reinterpret_cast<LcSegStats *>(sb);
    float *curve_dev = reinterpret_cast<float *>(sb + res_bytes);
    sa.psum = reinterpret_cast<double *>(sb + res_bytes + curve_bytes);
    sa.pcnt = reinterpret_cast<int *>(sa.psum + np);
    sa.pmax = reinterpret_cast<float *>(sa.pcnt + np);
    sa.pmin = sa.pmax + np;
    for (int r = 0; r < nregions; ++r) {
        const artgpu_local_contrast_region &reg = regions[r];
        const bool contrast_on = (float)reg.contrast != 0;
        if ((rc = decompose_dev(ctx, d, L, nullptr, stride))) return rc;
        if (reg.curve && (rc = h2d_table(ctx, curve_dev, reg.curve, 501 * 4))) return rc;
        sa.coeff0 = contrast_on ? d.low[d.cur] : nullptr;
        HIPCHK(ctx, launch_lc_stats(sa, ctx->stream));
        LcSegStats res[32];
        const int nseg = nbands + (contrast_on ? 1 : 0);
        HIPCHK(ctx, hipMemcpyAsync(res, sa.res, (size_t)nseg * sizeof(LcSegStats), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));             // the region's one host wait
        LcRemapArgs ra = {};
        LcHostInfo hi;
        lc_host_constants(res, d.nlevels, d.n, reg.contrast, &ra, &hi);
        ra.bands = d.bands; ra.coeff0 = d.low[d.cur]; ra.n = d.n; ra.nlevels = d.nlevels; ra.curve = reg.curve ? curve_dev : nullptr;
        HIPCHK(ctx, launch_lc_remap(ra, ctx->stream));
        if ((rc = reconstruct_dev(ctx, d, Lnew))) return rc;
        LcBlendArgs ba = {};
        ba.L = L; ba.l_stride = stride; ba.Lnew = Lnew; ba.w = w; ba.h = h;
        if ((rc = bind_plane(ctx, reg.mask, P_LC_MASK, &ba.mask, &ba.m_stride))) return rc;
        HIPCHK(ctx, launch_lc_blend(ba, ctx->stream));
        if (info && r == nregions - 1) {
            info->nlevels = d.nlevels;
            info->ave = hi.ave; info->min0 = hi.min0; info->max0 = hi.max0;
            for (int k = 0; k < 10; ++k) { info->mean[k] = hi.mean[k]; info->sigma[k] = hi.sigma[k]; info->maxp[k] = hi.maxp[k]; }
        }
    }
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_local_contrast_curve_lut(const double *points, int npoints, float lut[501], int *is_set)
{
    if (!lut || !is_set || npoints < 0 || (npoints > 0 && !points)) return ARTGPU_EINVAL;
    *is_set = lc_curve_lut(points, npoints, lut) ? 1 : 0;
    return ARTGPU_OK;
}

int artgpu_local_contrast(artgpu_ctx *ctx, artgpu_plane *L, const artgpu_local_contrast_region *regions, int nregions, double scale,
                          artgpu_local_contrast_info *info)
{
    StageScope scope_(ctx, "ImProcFunctions::localContrast");
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(L)) return fail(ctx, ARTGPU_EINVAL, "local_contrast: bad plane");
    int rc;
    if ((rc = local_contrast_check(ctx, L->w, L->h, regions, nregions, scale, "local_contrast"))) return rc;
    if (info) *info = artgpu_local_contrast_info{};
    if (nregions == 0) return ARTGPU_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (L->on_device) return local_contrast_dev(ctx, L->p, (size_t)(L->row_stride_bytes / 4), L->w, L->h, regions, nregions, info);
    float *work;
    if ((rc = plane_to_pool(ctx, L, P_LC_L, &work)) || (rc = local_contrast_dev(ctx, work, L->w, L->w, L->h, regions, nregions, info))) return rc;
    return pool_to_plane(ctx, work, L);
}

} // extern "C"
