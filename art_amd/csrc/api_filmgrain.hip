// art_amd/csrc/api_filmgrain.hip -- ImProcFunctions::filmGrain (rtengine/ipgrain.cc:33-98) and the NOISE regions of guidedSmoothing
// (rtengine/ipsmoothing.cc:565-695, :933-1067) behind the C ABI: the region derivation, add_noise's scalars and tables, the working area, the
// launches.  The kernel is filmgrain.hip's, the table builders are hostluts.hip's, the crop rule and the mask boxes are the Smoothing tool's.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace {

constexpr int FG_GUI_MAX = 100;                    // strength, coarseness: 0 .. 100 (rtgui/smoothing.cc:348,351; rtgui/grain.cc:51)
constexpr int FG_ISO_MIN = 100, FG_ISO_MAX = 6400; // rtgui/grain.cc:47

// what add_noise derives from a region before it reads a pixel (L572-597, L611-612)
struct FgRegion {
    int channel, strength, coarseness, seed, sz;
    float sf, radius, c;
    float taps[FG_MAX_TAPS];
};

inline float fg_lim01(float a) { return std::max(0.f, std::min(a, 1.f)); }

bool fg_region(int strength, int coarseness, int channel, double scale, FgRegion *r)
{
    r->channel = channel; r->strength = strength; r->coarseness = coarseness;
    r->sf = (float)(fg_lim01(float(strength) / (channel == SM_CH_L ? 200.f : 100.f)) / scale);
    r->radius = (float)((0.5f + 1.75f * float(coarseness) / 100.f) / scale);
    r->seed = 42 + channel + coarseness;
    const float c01 = float(coarseness) / 100.f;
    r->c = 655.35f / (20.f + std::pow(c01, 0.5f) * 80.f);
    r->sz = build_grain_kernel(r->radius, r->taps);
    return r->sz != 0;
}

// the arguments every NOISE region shares: EINVAL for what is malformed, EUNSUPPORTED for what the device path does not take
int fg_check_region(artgpu_ctx *ctx, int strength, int coarseness, int channel, const double *ws, double scale, const char *who, FgRegion *r)
{
    if (!ws || !(scale > 0.0) || std::isinf(scale)) return fail(ctx, ARTGPU_EINVAL, "%s: bad arguments", who);
    if (channel < ARTGPU_SMOOTHING_LUMINANCE || channel > ARTGPU_SMOOTHING_RGB) return fail(ctx, ARTGPU_EINVAL, "%s: channel %d", who, channel);
    if (strength < 0 || strength > FG_GUI_MAX || coarseness < 0 || coarseness > FG_GUI_MAX)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: strength %d / coarseness %d outside 0 .. %d", who, strength, coarseness, FG_GUI_MAX);
    if (!(scale >= 1.0)) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: scale %g (below 1: the kernel would be larger than 7 x 7) is not on the device path", who, scale);
    if (!fg_region(strength, coarseness, channel, scale, r)) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: a kernel of radius %g is not on the device path", who, (double)r->radius);
    return ARTGPU_OK;
}

int fg_check_area(artgpu_ctx *ctx, int ww, int hh, const char *who)
{
    if (3ull * (unsigned long long)ww * (unsigned long long)hh >= (1ull << 32))
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: a %dx%d working area has 2^32 / 3 pixels or more (draw numbers are 32-bit)", who, ww, hh);
    return ARTGPU_OK;
}

// One region: the tables into sub-slot `slot` of P_FG_TAB, the launch.  src / dst: at the working area's first pixel, never the same planes
int fg_region_dev(artgpu_ctx *ctx, const FgRegion &r, int slot, const float *const src[3], size_t src_stride, float *const dst[3], size_t dst_stride,
                  const float *mask, size_t mask_stride, int ww, int hh, const double *ws, bool norm_in, bool denorm_out)
{
    int rc;
    float *tabs;
    if ((rc = pool_get(ctx, P_FG_TAB, ARTGPU_FILM_GRAIN_MAX_REGIONS * FG_TAB_BYTES, &tabs))) return rc;
    char *tab = reinterpret_cast<char *>(tabs) + (size_t)slot * FG_TAB_BYTES;
    std::vector<float> host(FG_TAB_BYTES / 4, 0.f);
    FgArgs a = {};
    build_grain_table(r.seed, host.data(), &a.state);
    std::memcpy(host.data() + FG_NORMD, r.taps, sizeof r.taps);
    build_grain_jump(reinterpret_cast<FgJump *>(host.data() + FG_TAB_FLOATS));
    if ((rc = h2d_table(ctx, tab, host.data(), FG_TAB_BYTES))) return rc;
    for (int k = 0; k < 3; ++k) { a.src[k] = src[k]; a.dst[k] = dst[k]; a.ws1[k] = ws[3 + k]; }
    a.src_stride = src_stride; a.dst_stride = dst_stride; a.mask = mask; a.mask_stride = mask_stride;
    a.tab = reinterpret_cast<const float *>(tab);
    a.sf = r.sf; a.c = r.c; a.ww = ww; a.hh = hh; a.channel = r.channel; a.r = r.sz / 2;
    a.norm_in = norm_in ? 1 : 0; a.denorm_out = denorm_out ? 1 : 0;
    // four workgroups fit a CU (at most 118 vector registers, 27.9 KB of LDS): one resident round, each workgroup a chunk of neighbouring tiles
    HIPCHK(ctx, launch_fg_region(a, ctx->shared.opt_fg_grid > 0 ? ctx->shared.opt_fg_grid : (ctx->num_cus > 0 ? ctx->num_cus : 256) * 4, ctx->stream));
    return ARTGPU_OK;
}

int fg_copy_planes(artgpu_ctx *ctx, float *const dst[3], size_t dst_stride, const float *const src[3], size_t src_stride, int w, int h)
{
    for (int k = 0; k < 3; ++k)
        HIPCHK(ctx, hipMemcpy2DAsync(dst[k], dst_stride * 4, src[k], src_stride * 4, (size_t)w * 4, h, hipMemcpyDeviceToDevice, ctx->stream));
    return ARTGPU_OK;
}

// artgpu_add_noise on device planes: the working area from the mask, the region into P_FG_WORK, the area copied back
int add_noise_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const FgRegion &r, const artgpu_plane *mask, const double *ws, bool first, bool last)
{
    int rc;
    std::vector<const float *> mp;
    std::vector<size_t> ms;
    std::vector<int> boxes;
    if ((rc = sm_mask_boxes(ctx, W, H, &mask, 1, &mp, &ms, &boxes))) return rc;
    SmRegionPlan area = {};
    if (!sm_working_area(W, H, mask ? boxes.data() : nullptr, &area)) {            // no mask pixel above zero: only the normalise passes
        if (first || last) HIPCHK(ctx, launch_sm_scale(planes, stride, W, H, first && last ? 2 : first ? 0 : 1, ctx->stream));
        return ARTGPU_OK;
    }
    if ((rc = fg_check_area(ctx, area.ww, area.hh, "add_noise"))) return rc;
    const size_t nw = (size_t)area.ww * area.hh, off = (size_t)area.y0 * stride + area.x0;
    float *work;
    if ((rc = pool_get(ctx, P_FG_WORK, 3 * nw * 4, &work))) return rc;
    // a full-frame region takes the normalise pass at either end into its own loads / stores; a cropped one leaves them to sm_scale_kernel
    const bool fuse = !area.cropped;
    if (first && !fuse) HIPCHK(ctx, launch_sm_scale(planes, stride, W, H, 0, ctx->stream));
    const float *src[3] = {planes[0] + off, planes[1] + off, planes[2] + off};
    float *box[3] = {planes[0] + off, planes[1] + off, planes[2] + off};
    float *dst[3] = {work, work + nw, work + 2 * nw};
    if ((rc = fg_region_dev(ctx, r, 0, src, stride, dst, area.ww, mp[0] ? mp[0] + (size_t)area.y0 * ms[0] + area.x0 : nullptr, ms[0], area.ww, area.hh, ws,
                            first && fuse, last && fuse)) ||
        (rc = fg_copy_planes(ctx, box, stride, dst, area.ww, area.ww, area.hh)))
        return rc;
    if (last && !fuse) HIPCHK(ctx, launch_sm_scale(planes, stride, W, H, 1, ctx->stream));
    return ARTGPU_OK;
}

} // namespace

namespace artgpu { namespace api {

int fg_check(artgpu_ctx *ctx, int W, int H, const artgpu_film_grain_params *p, const double *ws, double scale, int output_pipeline, const char *who, FgPlan *pl)
{
    *pl = FgPlan{};
    pl->scale = scale;
    if (!p) return fail(ctx, ARTGPU_EINVAL, "%s: bad arguments", who);
    if (!p->enabled) return ARTGPU_OK;                                               // ipgrain.cc:90-92
    if (!ws || !(scale > 0.0) || std::isinf(scale)) return fail(ctx, ARTGPU_EINVAL, "%s: bad arguments", who);
    if (p->iso < FG_ISO_MIN || p->iso > FG_ISO_MAX || p->strength < 0 || p->strength > FG_GUI_MAX)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: iso %d outside %d .. %d or strength %d outside 0 .. %d", who, p->iso, FG_ISO_MIN, FG_ISO_MAX, p->strength, FG_GUI_MAX);
    int rc;
    if (!(scale >= 1.0)) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: scale %g (below 1: the kernel would be larger than 7 x 7) is not on the device path", who, scale);
    if ((rc = fg_check_area(ctx, W, H, who))) return rc;
    // ProcParamsOverride (ipgrain.cc:40-69)
    constexpr int iso_min = 20, iso_max = 6400;
    const int coarseness = fg_lim01(float(p->iso - iso_min + 1) / float(iso_max - iso_min)) * 100.f + 0.5f;
    const int nlevels = output_pipeline ? 3 : int(std::ceil(3 / scale));
    artgpu_film_grain_info &o = pl->info;
    const auto add = [&](int channel, int strength, int coarse) -> int {
        FgRegion r;
        if ((rc = fg_check_region(ctx, strength, coarse, channel, ws, scale, who, &r))) return rc;
        o.region[o.nregions++] = artgpu_film_grain_region_info{r.channel, r.strength, r.coarseness, r.seed, r.sz, r.sf};
        return ARTGPU_OK;
    };
    if (p->color && (rc = add(ARTGPU_SMOOTHING_CHROMINANCE, p->strength / 2, coarseness / 2))) return rc;
    for (int i = 0; i < nlevels; ++i)
        if ((rc = add(ARTGPU_SMOOTHING_LUMINANCE, p->strength / (nlevels - i), coarseness / (i + 1)))) return rc;
    return ARTGPU_OK;
}

// Every region is the frame (no masks), so the regions ping-pong between the image and P_FG_WORK instead of copying back after each; an
// odd count ends with one copy.  The first region's loads normalise, the last region's stores scale back
int film_grain_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const double ws[9], const FgPlan &pl)
{
    const int n = pl.info.nregions;
    if (n == 0) return ARTGPU_OK;
    int rc;
    const size_t np = (size_t)W * H;
    float *work;
    if ((rc = pool_get(ctx, P_FG_WORK, 3 * np * 4, &work))) return rc;
    float *img[3] = {planes[0], planes[1], planes[2]}, *tmp[3] = {work, work + np, work + 2 * np};
    bool in_img = true;
    for (int i = 0; i < n; ++i) {
        const artgpu_film_grain_region_info &g = pl.info.region[i];
        FgRegion r;
        if (!fg_region(g.strength, g.coarseness, g.channel, pl.scale, &r)) return fail(ctx, ARTGPU_EUNSUPPORTED, "film_grain: region %d", i);
        float *const *src = in_img ? img : tmp, *const *dst = in_img ? tmp : img;
        if ((rc = fg_region_dev(ctx, r, i, src, in_img ? stride : (size_t)W, dst, in_img ? (size_t)W : stride, nullptr, 0, W, H, ws, i == 0, i == n - 1))) return rc;
        in_img = !in_img;
    }
    return in_img ? ARTGPU_OK : fg_copy_planes(ctx, img, stride, tmp, W, W, H);
}

} } // namespace artgpu::api

extern "C" {

int artgpu_film_grain(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_film_grain_params *params, const double ws[9], double scale, int output_pipeline,
                      artgpu_film_grain_info *info)
{
    StageScope scope_(ctx, "ImProcFunctions::filmGrain");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !plane_ok(&img->r)) return fail(ctx, ARTGPU_EINVAL, "film_grain: bad image");
    int rc;
    FgPlan pl;
    if ((rc = fg_check(ctx, img->r.w, img->r.h, params, ws, scale, output_pipeline, "film_grain", &pl))) return rc;
    if (info) *info = pl.info;
    if (pl.info.nregions == 0) return ARTGPU_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "film_grain"))) return rc;
    if ((rc = film_grain_dev(ctx, d.p, d.stride, d.w, d.h, ws, pl))) return rc;
    return unbind_rgb(ctx, img, &d);
}

int artgpu_add_noise(artgpu_ctx *ctx, artgpu_rgb *img, int strength, int coarseness, int channel, const artgpu_plane *mask, const double ws[9],
                     double scale, int first, int last)
{
    StageScope scope_(ctx, "add_noise");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !plane_ok(&img->r)) return fail(ctx, ARTGPU_EINVAL, "add_noise: bad image");
    if (mask && (!plane_ok(mask) || mask->w != img->r.w || mask->h != img->r.h))
        return fail(ctx, ARTGPU_EINVAL, "add_noise: the mask must be a %dx%d plane", img->r.w, img->r.h);
    int rc;
    FgRegion r;
    if ((rc = fg_check_region(ctx, strength, coarseness, channel, ws, scale, "add_noise", &r))) return rc;
    if (!mask && (rc = fg_check_area(ctx, img->r.w, img->r.h, "add_noise"))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "add_noise"))) return rc;
    if ((rc = add_noise_dev(ctx, d.p, d.stride, d.w, d.h, r, mask, ws, first != 0, last != 0))) return rc;
    return unbind_rgb(ctx, img, &d);
}

int artgpu_grain_table(int seed, float *normd, float *kernel, int *sz, float radius, uint64_t *state)
{
    if (seed <= 0 || !normd || !state) return ARTGPU_EINVAL;
    if (kernel) {
        float taps[FG_MAX_TAPS] = {};
        const int n = build_grain_kernel(radius, taps);
        if (!n || !sz) return ARTGPU_EINVAL;
        std::memcpy(kernel, taps, sizeof taps);
        *sz = n;
    }
    build_grain_table(seed, normd, state);
    return ARTGPU_OK;
}

int artgpu_grain_indices(artgpu_ctx *ctx, uint64_t state, int64_t first, int64_t n, uint32_t *out)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!out || first < 0 || n < 1 || n > (1 << 24) || first + n > (1ll << 32) || state > FG_MASK48) return fail(ctx, ARTGPU_EINVAL, "grain_indices: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    float *tabs, *idx;
    if ((rc = pool_get(ctx, P_FG_TAB, ARTGPU_FILM_GRAIN_MAX_REGIONS * FG_TAB_BYTES, &tabs)) || (rc = pool_get(ctx, P_FG_IDX, (size_t)n * 4, &idx))) return rc;
    FgJump j;
    build_grain_jump(&j);
    if ((rc = h2d_table(ctx, tabs + FG_TAB_FLOATS, &j, sizeof j))) return rc;
    HIPCHK(ctx, launch_fg_indices(tabs, state, (uint64_t)first, (int)n, reinterpret_cast<uint32_t *>(idx), ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(out, idx, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ARTGPU_OK;
}

int artgpu_set_pipeline_film_grain(artgpu_ctx *ctx, const artgpu_film_grain_params *params)
{
    if (!ctx) return ARTGPU_EINVAL;
    ctx->shared.pipe_fg_on = params ? 1 : 0;
    ctx->shared.pipe_fg = params ? *params : artgpu_film_grain_params{};
    return ARTGPU_OK;
}

} // extern "C"
