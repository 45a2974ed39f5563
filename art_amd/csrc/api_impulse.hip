// art_amd/csrc/api_impulse.hip -- ImProcFunctions::impulsedenoise behind the C ABI: the gates and derived parameters, markImpulse on the L plane
// (sharpen.hip's launchers behind the shared gaussian) and impulse_nr's correction between the two mode switches.  The kernel is impulse.hip's.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace {

constexpr size_t IMP_COUNTER_BYTES = 64;     // P_SH_BYTES: the 64-bit counter, then the impulse map

} // namespace

namespace artgpu { namespace api {

ImpPlan imp_plan(int W, int H, const artgpu_impulse_denoise_params *p, double scale)
{
    ImpPlan pl = {};
    if (!p->enabled) { pl.early = 1; return pl; }
    if (W < 8 || H < 8) { pl.early = 2; return pl; }
    if (!(scale >= 0.5)) { pl.early = 3; return pl; }
    const float t = p->thresh / scale;
    pl.thresh = float(t / 20.0);
    pl.sigma = std::max(2.f, pl.thresh - 1.f);
    pl.impthr = std::max(1.f, 5.5f - pl.thresh);
    return pl;
}

int impulse_denoise_dev(artgpu_ctx *ctx, const DevRGB &d, const ImpPlan &pl, const double ws[9], const double *iws, int already_lab, int to_rgb,
                        artgpu_impulse_denoise_info *info)
{
    const int W = d.w, H = d.h;
    const size_t n = (size_t)W * H, rowb = (size_t)W * 4;
    float *sp, *bytes;
    int rc;
    if ((rc = pool_get(ctx, P_SH_PLANES, 3 * n * 4, &sp)) || (rc = pool_get(ctx, P_SH_BYTES, IMP_COUNTER_BYTES + n, &bytes))) return rc;
    unsigned long long *counter = reinterpret_cast<unsigned long long *>(bytes);
    unsigned char *impish = reinterpret_cast<unsigned char *>(bytes) + IMP_COUNTER_BYTES;
    float *L = sp, *lpf = sp + n, *gtmp = sp + 2 * n;
    if (!already_lab && (rc = lab_switch_dev(ctx, d, ws, true))) return rc;
    // markImpulse(width, height, lab_L, impish, thresh) on a contiguous copy of the L plane
    HIPCHK(ctx, hipMemcpy2DAsync(L, rowb, d.p[1], d.stride * 4, rowb, H, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(lpf, L, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if ((rc = gaussian_dev(ctx, lpf, gtmp, W, H, pl.sigma))) return rc;
    HIPCHK(ctx, launch_sh_impulse(L, lpf, impish, W, H, pl.thresh, ctx->stream));
    if (info) {
        HIPCHK(ctx, hipMemsetAsync(counter, 0, IMP_COUNTER_BYTES, ctx->stream));
        HIPCHK(ctx, launch_sh_count(impish, nullptr, n, counter, ctx->stream));
    }
    const ImpArgs a = {d.p[1], d.p[0], d.p[2], d.stride, impish, W, H};
    HIPCHK(ctx, launch_imp_correct(a, ctx->stream));
    if (to_rgb && (rc = lab_switch_dev(ctx, d, iws, false))) return rc;
    if (info) {
        unsigned long long host = 0;
        HIPCHK(ctx, hipMemcpyAsync(&host, counter, sizeof host, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        info->impulse_pixels = (int64_t)host;
    }
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_impulse_denoise(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_impulse_denoise_params *params, const double ws[9], const double *iws,
                           double scale, int to_rgb, artgpu_impulse_denoise_info *info)
{
    StageScope scope_(ctx, "ImProcFunctions::impulsedenoise");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !params || !ws || (to_rgb && !iws)) return fail(ctx, ARTGPU_EINVAL, "impulse_denoise: null argument");
    if (info) *info = artgpu_impulse_denoise_info{};
    if (!plane_ok(&img->r)) return fail(ctx, ARTGPU_EINVAL, "impulse_denoise: bad plane");
    const ImpPlan pl = imp_plan(img->r.w, img->r.h, params, scale);
    if (info) { info->early_out = pl.early; info->thresh = pl.thresh; info->sigma = pl.sigma; info->impthr = pl.impthr; }
    if (pl.early) return ARTGPU_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    int rc;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "impulse_denoise"))) return rc;
    if ((rc = impulse_denoise_dev(ctx, d, pl, ws, iws, 0, to_rgb, info))) return rc;
    return unbind_rgb(ctx, img, &d);
}

} // extern "C"
