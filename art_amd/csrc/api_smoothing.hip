// art_amd/csrc/api_smoothing.hip -- smoothing behind the C ABI: ImProcFunctions::guidedSmoothing, modes GUIDED and NLMEANS: the regions' plans, their
// blend planes and boxes (which film grain's NOISE regions share), the region passes.  The kernels are smoothing.hip's.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace {

// floats of P_SM_PLANES a region needs
size_t sm_region_floats(const SmRegionPlan &p)
{
    const size_t nw = (size_t)p.ww * p.hh;
    if (p.skipped == ARTGPU_SMOOTHING_SKIP_EMPTY || p.skipped == ARTGPU_SMOOTHING_SKIP_RADIUS) return 0;
    if (p.mode == ARTGPU_SMOOTHING_GUIDED) return ((p.channel == SM_CH_LC ? 3 : 7) + (p.iterations > 1 ? 3 : 0)) * nw;
    return (p.channel == SM_CH_L ? 1 : p.channel == SM_CH_LC ? (p.skipped ? 0 : 3) : 4) * nw;
}

// one region on the normalised device image; `mask`: the region's blend plane on the device (rows of mstride floats) or nullptr
// norm_in: the image is not normalised yet and this (full-frame) region does it; denorm_out: this (full-frame) region stores * 65535.f
int sm_region_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, const SmRegionPlan &p, const float *mask, size_t mstride, const double *ws, double scale, float *big,
                  bool norm_in, bool denorm_out)
{
    int rc;
    const size_t nw = (size_t)p.ww * p.hh, off = (size_t)p.y0 * stride + p.x0;
    SmArgs a = {};
    for (int k = 0; k < 3; ++k) { a.img[k] = planes[k] + off; a.ws1[k] = ws[3 + k]; }
    a.stride = stride;
    a.mask = mask ? mask + (size_t)p.y0 * mstride + p.x0 : nullptr; a.mask_stride = mstride;
    a.ww = p.ww; a.hh = p.hh; a.channel = p.channel;
    a.img_norm = norm_in ? 1 : 0; a.out_denorm = denorm_out ? 1 : 0;
    if (p.mode == ARTGPU_SMOOTHING_GUIDED) {
        if (p.skipped) {                                              // r == 0: working == rgb, blended all the same (L1050-1064)
            a.channel = SM_CH_LC;
            HIPCHK(ctx, launch_sm_nlm_merge(a, ctx->stream));
            return ARTGPU_OK;
        }
        const bool self = p.channel == SM_CH_LC;
        const size_t nl = (size_t)p.w * p.h;
        float *low, *tmp, *q = big;
        if ((rc = pool_get(ctx, P_TMP, 8 * nl * 4, &low)) || (rc = pool_get(ctx, P_LIN, 8 * nl * 4, &tmp))) return rc;
        if (!self) { for (int k = 0; k < 3; ++k) { a.in[k] = q; q += nw; } a.guide = q; q += nw; }
        for (int k = 0; k < 3; ++k) { a.chan[k] = q; q += nw; }
        if (p.iterations > 1) for (int k = 0; k < 3; ++k) { a.work[k] = q; q += nw; }
        a.w = p.w; a.h = p.h; a.epsilon = p.epsilon; a.low = low;
        for (int k = 0; k < 3; ++k) { a.a[k] = self ? low + (2 * k) * nl : low + (2 + k) * nl; a.b[k] = self ? low + (2 * k + 1) * nl : low + (5 + k) * nl; }
        GuidedArgs g = {};
        g.W = p.ww; g.H = p.hh; g.w = p.w; g.h = p.h; g.epsilon = p.epsilon; g.guide = a.guide;
        for (int k = 0; k < 3; ++k) g.chan[k] = a.chan[k];
        for (int k = 0; k < 8; ++k) g.low[k] = low + k * nl;
        for (int it = 0; it < p.iterations; ++it) {
            for (int k = 0; k < 3; ++k) a.src[k] = it == 0 ? a.img[k] : a.work[k];
            a.src_stride = it == 0 ? stride : (size_t)p.ww;
            a.src_norm = it == 0 && norm_in ? 1 : 0;
            a.last = it == p.iterations - 1;
            HIPCHK(ctx, launch_sm_prepare(a, ctx->stream));
            if (self) {
                HIPCHK(ctx, launch_sm_subsample_self(a, ctx->stream));
                if ((rc = box_blur_planes(ctx, low, tmp, 6, nl, p.w, p.h, p.rad))) return rc;        // mean I, corr I per channel
                HIPCHK(ctx, launch_sm_ab_self(a, ctx->stream));
                if ((rc = box_blur_planes(ctx, low, tmp, 6, nl, p.w, p.h, p.rad))) return rc;        // mean a, mean b per channel
            } else {
                HIPCHK(ctx, launch_gf_subsample(g, ctx->stream));
                if ((rc = box_blur_planes(ctx, low, tmp, 8, nl, p.w, p.h, p.rad))) return rc;        // meanI, corrI, meanp[3], corrIp[3]
                HIPCHK(ctx, launch_gf_ab(g, ctx->stream));
                if ((rc = box_blur_planes(ctx, low + 2 * nl, tmp, 6, nl, p.w, p.h, p.rad))) return rc;   // mean a[3], mean b[3]
            }
            HIPCHK(ctx, launch_sm_finish(a, ctx->stream));
        }
        return ARTGPU_OK;
    }
    // NLMEANS
    float *q = big;
    const int nplanes = p.channel == SM_CH_L ? 1 : 3;
    if (!(p.skipped && p.channel == SM_CH_LC)) {
        for (int k = 0; k < nplanes; ++k) { a.work[k] = q; q += nw; }
        if (p.channel == SM_CH_C) a.in[0] = q;
        HIPCHK(ctx, launch_sm_nlm_split(a, ctx->stream));
        if (!p.skipped)
            for (int it = 0; it < p.iterations; ++it)
                for (int k = 0; k < nplanes; ++k)
                    if ((rc = nlm_plane_dev(ctx, a.work[k], p.ww, p.hh, 1.f, p.nlstrength, p.nldetail, (float)scale))) return rc;
    }
    HIPCHK(ctx, launch_sm_nlm_merge(a, ctx->stream));
    return ARTGPU_OK;
}

} // namespace

namespace artgpu { namespace api {

// everything that does not depend on a mask's box: what the pipe checks before any stage runs
int sm_check(artgpu_ctx *ctx, int W, int H, const artgpu_smoothing_region *regions, int nregions, const double *ws, double scale, bool read_masks, const char *who)
{
    if (nregions < 0 || (nregions > 0 && !regions) || !ws || !(scale > 0.0) || std::isinf(scale)) return fail(ctx, ARTGPU_EINVAL, "%s: bad arguments", who);
    for (int i = 0; i < nregions; ++i) {
        const artgpu_smoothing_region &r = regions[i];
        if (r.mode < ARTGPU_SMOOTHING_GUIDED || r.mode > ARTGPU_SMOOTHING_WAVELETS) return fail(ctx, ARTGPU_EINVAL, "%s: region %d: mode %d", who, i, r.mode);
        if (r.channel < ARTGPU_SMOOTHING_LUMINANCE || r.channel > ARTGPU_SMOOTHING_RGB) return fail(ctx, ARTGPU_EINVAL, "%s: region %d: channel %d", who, i, r.channel);
        if (r.mode != ARTGPU_SMOOTHING_GUIDED && r.mode != ARTGPU_SMOOTHING_NLMEANS)
            return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: mode %d is not on the device path (only GUIDED and NLMEANS are)", who, i, r.mode);
        if (r.iterations < 1) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: iterations %d", who, i, r.iterations);
        if (r.mode == ARTGPU_SMOOTHING_NLMEANS && r.nlstrength != 0 && !(scale >= 1.0))
            return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: NL-means at scale %g (below 1) is not on the device path", who, i, scale);
        if (read_masks && r.mask && (!plane_ok(r.mask) || r.mask->w != W || r.mask->h != H)) return fail(ctx, ARTGPU_EINVAL, "%s: region %d: the mask must be a %dx%d plane", who, i, W, H);
    }
    return ARTGPU_OK;
}

// the working area of a region from its box (inclusive maxima as the reduction leaves them; nullptr: a NULL mask, the frame), L948-980: the
// box, or the frame unless the box is under half of it.  false: no mask pixel above zero, skipped = ARTGPU_SMOOTHING_SKIP_EMPTY
bool sm_working_area(int W, int H, const int *box, SmRegionPlan *pl)
{
    if (box && box[2] < box[0]) { pl->skipped = ARTGPU_SMOOTHING_SKIP_EMPTY; return false; }
    int min_x = box ? box[0] : 0, min_y = box ? box[1] : 0, max_x = box ? box[2] + 1 : W, max_y = box ? box[3] + 1 : H;
    int ww = max_x - min_x, hh = max_y - min_y;
    if (ww * hh < (W * H) / 2) pl->cropped = 1;                    // L957 (int arithmetic, as there)
    else { min_x = 0; min_y = 0; max_x = W; max_y = H; ww = W; hh = H; }
    pl->x0 = min_x; pl->y0 = min_y; pl->x1 = max_x; pl->y1 = max_y; pl->ww = ww; pl->hh = hh;
    return true;
}

// one region's plan from its box
int sm_plan_region(artgpu_ctx *ctx, int W, int H, const artgpu_smoothing_region &r, const int *box, double scale, const char *who, int i, SmRegionPlan *pl)
{
    *pl = SmRegionPlan{};
    pl->mode = r.mode; pl->channel = r.channel; pl->iterations = r.iterations; pl->nlstrength = r.nlstrength; pl->nldetail = r.nldetail;
    if (!sm_working_area(W, H, box, pl)) return ARTGPU_OK;
    const int ww = pl->ww, hh = pl->hh;
    if (r.mode == ARTGPU_SMOOTHING_GUIDED) {
        pl->epsilon = (float)std::max(0.001f * std::pow(2.0, (double)-r.epsilon), 1e-6);        // L1040: a double narrowed at the call
        const int rr = (int)std::round(r.radius / scale);             // L348
        pl->r = rr > 0 ? rr : 0;
        if (pl->r == 0) { pl->skipped = ARTGPU_SMOOTHING_SKIP_RADIUS; return ARTGPU_OK; }
        const GfGrid grid = gf_grid(ww, hh, pl->r);                   // calculate_subsampling, f_mean (guidedfilter.cc:58-75, 160-167)
        pl->sub = grid.sub; pl->w = grid.w; pl->h = grid.h;
        if (pl->w < ARTGPU_SMOOTHING_MIN_SIZE || pl->h < ARTGPU_SMOOTHING_MIN_SIZE)
            return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: a %dx%d working plane leaves a %dx%d statistics grid, below %d", who, i, ww, hh, pl->w, pl->h, ARTGPU_SMOOTHING_MIN_SIZE);
        pl->rad = grid.rad;
        if (pl->rad > HBLUR_MAX_RADIUS)
            return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: box radius %d (r / subsampling) is above the %d the blur kernels hold in LDS", who, i, pl->rad, HBLUR_MAX_RADIUS);
    } else {
        if (r.nlstrength == 0) { pl->skipped = ARTGPU_SMOOTHING_SKIP_STRENGTH; return ARTGPU_OK; }
        if (ww < 32 || hh < 32) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: NL-means on a %dx%d working plane, smaller than 32x32", who, i, ww, hh);
        if ((unsigned long long)(ww + 14) * (unsigned long long)(hh + 14) >= (1ull << 30))
            return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: NL-means on a %dx%d working plane exceeds 2^30 pixels", who, i, ww, hh);
    }
    return ARTGPU_OK;
}

// The blend planes of a call's regions on the device and find_region (L411-434) of each: host planes are staged (P_SM_MASK), every mask's box
// comes from one pass (SM_MAX_BOX_REGIONS planes per launch) and one host wait for 4 ints per mask.  mp / ms: per region the plane and its row
// stride in floats (nullptr: all ones); boxes: 4 ints per region that has a mask, in region order
int sm_mask_boxes(artgpu_ctx *ctx, int W, int H, const artgpu_plane *const *masks, int n, std::vector<const float *> *mp_out, std::vector<size_t> *ms_out,
                  std::vector<int> *boxes_out)
{
    int rc;
    std::vector<const float *> &mp = *mp_out;
    std::vector<size_t> &ms = *ms_out;
    std::vector<int> &boxes = *boxes_out;
    mp.assign(n, nullptr); ms.assign(n, 0);
    if ((rc = bind_planes(ctx, W, H, masks, n, P_SM_MASK, mp.data(), ms.data()))) return rc;
    std::vector<int> masked;
    for (int i = 0; i < n; ++i)
        if (masks[i]) masked.push_back(i);
    // find_region of every mask: one pass (SM_MAX_BOX_REGIONS planes per launch), one wait for 4 ints per mask
    boxes.assign(4 * masked.size(), 0);
    if (!masked.empty()) {
        for (size_t k = 0; k < masked.size(); ++k) { boxes[4 * k] = W; boxes[4 * k + 1] = H; boxes[4 * k + 2] = -1; boxes[4 * k + 3] = -1; }
        float *bx;
        if ((rc = pool_get(ctx, P_SM_BOX, boxes.size() * 4, &bx))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(bx, boxes.data(), boxes.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        for (size_t k0 = 0; k0 < masked.size(); k0 += SM_MAX_BOX_REGIONS) {
            SmBoxArgs b = {};
            b.n = (int)std::min(masked.size() - k0, (size_t)SM_MAX_BOX_REGIONS); b.W = W; b.H = H; b.box = reinterpret_cast<int *>(bx) + 4 * k0;
            for (int k = 0; k < b.n; ++k) { b.mask[k] = mp[masked[k0 + k]]; b.stride[k] = ms[masked[k0 + k]]; }
            HIPCHK(ctx, launch_sm_box(b, ctx->stream));
        }
        HIPCHK(ctx, hipMemcpyAsync(boxes.data(), bx, boxes.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return ARTGPU_OK;
}

// the tool on device planes (rows of `stride` floats) in RGB mode; enqueued on ctx->stream, one host wait when a region has a mask
int smoothing_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const artgpu_smoothing_region *regions, int n, const double *ws, double scale,
                  artgpu_smoothing_info *info, const char *who)
{
    int rc;
    std::vector<const artgpu_plane *> masks(n);
    for (int i = 0; i < n; ++i) masks[i] = regions[i].mask;
    std::vector<const float *> mp;
    std::vector<size_t> ms;
    std::vector<int> boxes;
    if ((rc = sm_mask_boxes(ctx, W, H, masks.data(), n, &mp, &ms, &boxes))) return rc;
    // the whole plan, before any kernel writes the image
    std::vector<SmRegionPlan> plans(n);
    size_t need = 0;
    for (int i = 0, k = 0; i < n; ++i) {
        if ((rc = sm_plan_region(ctx, W, H, regions[i], regions[i].mask ? &boxes[4 * k++] : nullptr, scale, who, i, &plans[i]))) return rc;
        need = std::max(need, sm_region_floats(plans[i]));
    }
    float *big = nullptr;
    if (need && (rc = pool_get(ctx, P_SM_PLANES, need * 4, &big))) return rc;
    int first = -1, last = -1;
    for (int i = 0; i < n; ++i)
        if (plans[i].skipped != ARTGPU_SMOOTHING_SKIP_EMPTY) { if (first < 0) first = i; last = i; }
    if (first < 0) {
        HIPCHK(ctx, launch_sm_scale(planes, stride, W, H, 2, ctx->stream));        // normalizeFloatTo1, normalizeFloatTo65535 (L938, L1067)
    } else {
        // a full-frame region at either end takes that end's normalise pass into its own passes (every pixel still sees exactly one of each)
        const bool fuse_in = !plans[first].cropped, fuse_out = !plans[last].cropped;
        if (!fuse_in) HIPCHK(ctx, launch_sm_scale(planes, stride, W, H, 0, ctx->stream));
        for (int i = 0; i < n; ++i)
            if (plans[i].skipped != ARTGPU_SMOOTHING_SKIP_EMPTY &&
                (rc = sm_region_dev(ctx, planes, stride, plans[i], mp[i], ms[i], ws, scale, big, fuse_in && i == first, fuse_out && i == last)))
                return rc;
        if (!fuse_out) HIPCHK(ctx, launch_sm_scale(planes, stride, W, H, 1, ctx->stream));
    }
    if (info)
        for (int i = 0; i < n; ++i) {
            const SmRegionPlan &p = plans[i];
            artgpu_smoothing_info &o = info[i];
            o = artgpu_smoothing_info{};
            o.r = p.r; o.epsilon = p.epsilon; o.min_x = p.x0; o.min_y = p.y0; o.max_x = p.x1; o.max_y = p.y1; o.cropped = p.cropped; o.work_w = p.ww; o.work_h = p.hh;
            o.subsampling = p.sub; o.box_radius = p.rad; o.skipped = p.skipped;
        }
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_smoothing(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_smoothing_region *regions, int nregions, const double ws[9], double scale,
                     artgpu_smoothing_info *info)
{
    StageScope scope_(ctx, "ImProcFunctions::guidedSmoothing");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !plane_ok(&img->r)) return fail(ctx, ARTGPU_EINVAL, "smoothing: bad image");
    int rc;
    if ((rc = sm_check(ctx, img->r.w, img->r.h, regions, nregions, ws, scale, true, "smoothing"))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "smoothing"))) return rc;
    if ((rc = smoothing_dev(ctx, d.p, d.stride, d.w, d.h, regions, nregions, ws, scale, info, "smoothing"))) return rc;
    return unbind_rgb(ctx, img, &d);
}

} // extern "C"
