// art_amd/csrc/api_cacorrect.hip -- raw CA correction behind the C ABI: CA_correct_RT on a Bayer CFA plane ahead of the demosaic (the colour map,
// the block grid and its scratch, the iterations with the colour-shift guard).  The kernels are cacorrect.hip's, the guard's gaussian is the shared one.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace artgpu { namespace api {

// Bayer 2x2 colour map of `filters` for the CA correction: FC packed as CaArgs::cfa; false for X-Trans, a fourth colour or a
// pattern without one green per row and column
bool ca_cfa(uint32_t filters, unsigned *cfa)
{
    if (filters == 9) return false;
    unsigned f[2][2], packed = 0;
    for (int r = 0; r < 2; ++r)
        for (int c = 0; c < 2; ++c) {
            f[r][c] = (filters >> ((((r << 1) & 14) + (c & 1)) << 1)) & 3;
            if (f[r][c] == 3) return false;
            packed |= f[r][c] << ((r * 2 + c) * 2);
        }
    for (int k = 0; k < 2; ++k)
        if ((f[k][0] == 1) == (f[k][1] == 1) || (f[0][k] == 1) == (f[1][k] == 1)) return false;
    *cfa = packed;
    return true;
}

// CA_correct_RT on a contiguous-or-strided device CFA plane, enqueued on ctx->stream (no synchronisation unless fit_out)
int ca_correct_dev(artgpu_ctx *ctx, float *raw, size_t stride, int W, int H, unsigned cfa, const artgpu_ca_params *p, double *fit_out)
{
    constexpr int ts = 128, border2 = 16, cb = 2;
    CaArgs a = {};
    a.raw = raw; a.stride = stride; a.W = W; a.H = H; a.width = W + (W & 1); a.cfa = cfa;
    const int vz1 = (H + border2) % (ts - border2) == 0 ? 1 : 0;
    const int hz1 = (a.width + border2) % (ts - border2) == 0 ? 1 : 0;
    a.vblsz = (int)ceil((float)(H + border2) / (ts - border2) + 2 + vz1);
    a.hblsz = (int)ceil((float)(a.width + border2) / (ts - border2) + 2 + hz1);
    a.ntv = (H + 8 + (ts - border2) - 1) / (ts - border2);
    a.nth = (W + 8 + (ts - border2) - 1) / (ts - border2);
    a.fw = (W + 1 - 2 * cb) / 2; a.fh = (H + 1 - 2 * cb) / 2;
    a.autoCA = p->autocorrect ? 1 : 0;
    a.cared = p->red; a.cablue = p->blue;
    const int iterations = a.autoCA ? (p->iterations > 1 ? p->iterations : 1) : 1;
    const bool guard = p->avoid_colour_shift != 0;
    const size_t half = (size_t)H * a.width / 2, nb = (size_t)a.vblsz * a.hblsz, ninner = (size_t)(a.vblsz - 2) * (a.hblsz - 2);
    const size_t fplane = (size_t)a.fw * a.fh;
    float *halfp, *blk, *grd = nullptr;
    int rc;
    if ((rc = pool_get(ctx, P_CA_HALF, 2 * half * 4, &halfp)) || (rc = pool_get(ctx, P_CA_BLK, (144 + nb * 5 + ninner * 8 + 4) * 4, &blk)))
        return rc;
    if (guard && (rc = pool_get(ctx, P_CA_GUARD, ((size_t)a.fw * (H - 2 * cb) + 3 * fplane) * 4, &grd))) return rc;
    a.Gtmp = halfp; a.RawDataTmp = halfp + half;
    a.fit = reinterpret_cast<double *>(blk);                       // 64 doubles first: 8-byte aligned
    a.words = reinterpret_cast<int *>(blk + 128);
    a.blockwt = blk + 144; a.blockshifts = a.blockwt + ((nb + 3) & ~(size_t)3); a.blockfit = a.blockshifts + 4 * nb;
    if (guard) { a.oldraw = grd; a.red = grd + (size_t)a.fw * (H - 2 * cb); a.blue = a.red + fplane; }
    // the reference zeroes blockwt / blockshifts once per call (L208); Gtmp (never written in manual mode) and fitparams (only
    // partly written by a linear fit) are zeroed here so that every value the device reads is defined
    HIPCHK(ctx, hipMemsetAsync(halfp, 0, half * 4, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(blk, 0, (144 + ((nb + 3) & ~(size_t)3) + 4 * nb) * 4, ctx->stream));
    HIPCHK(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a.words), 1, 2, ctx->stream));       // run, processpasstwo
    HIPCHK(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a.words + 2), 4, 1, ctx->stream));   // polyord
    if (guard) HIPCHK(ctx, launch_ca_capture(a, ctx->stream));
    for (int it = 0; it < iterations; ++it) {
        HIPCHK(ctx, launch_ca_iteration(a, ctx->stream));
        if (guard) {
            HIPCHK(ctx, launch_ca_factors(a, ctx->stream));
            if ((rc = gaussian_dev(ctx, a.red, a.blue + fplane, a.fw, a.fh, 30.0)) || (rc = gaussian_dev(ctx, a.blue, a.blue + fplane, a.fw, a.fh, 30.0)))
                return rc;
            HIPCHK(ctx, launch_ca_apply(a, ctx->stream));
        }
        HIPCHK(ctx, launch_ca_step(a, ctx->stream));
    }
    if (fit_out) {
        HIPCHK(ctx, hipMemcpyAsync(fit_out, a.fit, 64 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_raw_ca_correct(artgpu_ctx *ctx, artgpu_plane *raw, uint32_t filters, const artgpu_ca_params *p, double fit_out[64])
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(raw) || !p) return fail(ctx, ARTGPU_EINVAL, "raw_ca_correct: bad argument");
    unsigned cfa;
    if (!ca_cfa(filters, &cfa)) return fail(ctx, ARTGPU_EUNSUPPORTED, "raw_ca_correct: RGB Bayer patterns only (filters 0x%08x)", filters);
    if (raw->w < 64 || raw->h < 64) return fail(ctx, ARTGPU_EUNSUPPORTED, "raw_ca_correct: frame smaller than 64x64");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    if (raw->on_device) return ca_correct_dev(ctx, raw->p, (size_t)(raw->row_stride_bytes / 4), raw->w, raw->h, cfa, p, fit_out);
    float *work;
    if ((rc = pool_get(ctx, P_CA_RAW, (size_t)raw->w * raw->h * 4, &work))) return rc;
    HIPCHK(ctx, hipMemcpy2DAsync(work, (size_t)raw->w * 4, raw->p, (size_t)raw->row_stride_bytes, (size_t)raw->w * 4, raw->h, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = ca_correct_dev(ctx, work, raw->w, raw->w, raw->h, cfa, p, fit_out))) return rc;
    return pool_to_plane(ctx, work, raw);
}

} // extern "C"
