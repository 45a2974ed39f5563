// art_amd/csrc/api_filters.hip -- the filters several stages share, behind the C ABI: rtengine::guidedFilter and the denoise tool's
// guided chroma smoothing, gaussianBlur, the detail mask, denoise::NLMeans.  The kernels are guided.hip's, shrinkblur.hip's box blurs,
// nlmeans.hip's and nlm_sweep.hip's.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace {

// calculateYvVFactors<double> + M rescaling (gauss.cc:94-126,556-562)
void yvv_factors(double sigma, GaussArgs &g, bool double_path = false)
{
    double q;
    if (sigma < 2.5) q = 3.97156 - 4.14554 * std::sqrt(1.0 - 0.26891 * sigma);
    else q = 0.98711 * sigma - 0.96330;
    const double b0 = 1.57825 + 2.44413 * q + 1.4281 * q * q + 0.422205 * q * q * q;
    double b1 = 2.44413 * q + 2.85619 * q * q + 1.26661 * q * q * q;
    double b2 = -1.4281 * q * q - 1.26661 * q * q * q;
    double b3 = 0.422205 * q * q * q;
    g.B = 1.0 - (b1 + b2 + b3) / b0;
    b1 /= b0; b2 /= b0; b3 /= b0;
    double *M = g.M;
    M[0] = -b3 * b1 + 1.0 - b3 * b3 - b2;
    M[1] = (b3 + b1) * (b2 + b3 * b1);
    M[2] = b3 * (b1 + b3 * b2);
    M[3] = b1 + b3 * b2;
    M[4] = -(b2 - 1.0) * (b2 + b3 * b1);
    M[5] = -(b3 * b1 + b3 * b3 + b2 - 1.0) * b3;
    M[6] = b3 * b1 + b2 + b1 * b1 - b2 * b2;
    M[7] = b1 * b2 + b3 * b2 * b2 - b1 * b3 * b3 - b3 * b3 * b3 - b3 * b2 + b3;
    M[8] = b3 * (b1 + b3 * b2);
    for (int i = 0; i < 9; ++i) {
        if (double_path) {           // gaussHorizontal<T> / gaussVertical<T> normalise differently (gauss.cc:674-677 vs 559-563)
            M[i] /= (1.0 + b1 - b2 + b3) * (1.0 + b2 + (b1 - b3) * b3);
        } else {
            M[i] *= (1.0 + b2 + (b1 - b3) * b3);
            M[i] /= (1.0 + b1 - b2 + b3) * (1.0 - b1 - b2 - b3);
        }
        g.Mf[i] = (float)M[i];
    }
    g.b[0] = b1; g.b[1] = b2; g.b[2] = b3;
    g.Bf = (float)g.B; g.bf[0] = (float)b1; g.bf[1] = (float)b2; g.bf[2] = (float)b3;
}

} // namespace

namespace artgpu { namespace api {

int gf_subsampling(int w, int h, int r)   // calculate_subsampling (guidedfilter.cc:58-75)
{
    if (r == 1) return 1;
    if ((w > h ? w : h) <= 600) return 1;
    for (int s = 5; s > 0; --s)
        if (r % s == 0) return s;
    const int t = r / 2;
    return t < 2 ? 2 : (t > 4 ? 4 : t);
}

// the statistics grid of one rtengine::guidedFilter call on a W x H plane and f_mean's box radius on it (guidedfilter.cc:160-167):
// rad = LIM(int(float(r) / sub), 0, (min(w, h) - 1) / 2 - 1), which is 0 for a grid without pixels.  Checks nothing: every caller has
// its own size limits, its HBLUR_MAX_RADIUS check and its message
GfGrid gf_grid(int W, int H, int r, int subsampling)
{
    GfGrid g;
    g.sub = subsampling > 0 ? subsampling : gf_subsampling(W, H, r);
    g.w = W / g.sub; g.h = H / g.sub;
    const int hi = ((g.w < g.h ? g.w : g.h) - 1) / 2 - 1;
    int rad = (int)(float(r) / g.sub);
    rad = rad < hi ? rad : hi;
    g.rad = rad > 0 ? rad : 0;
    return g;
}

// `count` planes of w x h floats, n apart: boxblur(float**, float**, radius, W, H) (boxblur.h:318) in place through `tmp`, enqueued on ctx->stream
int box_blur_planes(artgpu_ctx *ctx, float *planes, float *tmp, int count, size_t n, int w, int h, int rad)
{
    if (rad == 0) return ARTGPU_OK;
    BlurArgs bl = {};
    bl.n = n; bl.w = w; bl.h = h; bl.steady_div = 1; bl.plain = 1;
    for (int l = 0; l < 10; ++l) bl.rad[l] = rad;
    bl.src = planes; bl.dst = tmp;
    HIPCHK(ctx, launch_hblur(bl, count, ctx->stream));
    bl.src = tmp; bl.dst = planes;
    HIPCHK(ctx, launch_vblur_combine(bl, count, ctx->stream));
    return ARTGPU_OK;
}

// rtengine::guidedFilter (guidedfilter.cc:80-241) on contiguous device planes (rows of W floats) up to mean a / mean b on the statistics grid
// (g->low[2], g->low[5]): the caller runs the last, pointwise pass (launch_gf_finish_plain with g->q, or one of its own).  Enqueued on
// ctx->stream; scratch: the statistics grid in P_TMP / P_LIN
int guided_filter_stats(artgpu_ctx *ctx, const float *guide, const float *src, int W, int H, int r, float epsilon, int subsampling, const char *who, GuidedArgs *gout)
{
    const GfGrid grid = gf_grid(W, H, r, subsampling);
    GuidedArgs &g = *gout;
    g = GuidedArgs{};
    g.W = W; g.H = H; g.w = grid.w; g.h = grid.h; g.epsilon = epsilon; g.nch = 1;
    if (g.w < 1 || g.h < 1) return fail(ctx, ARTGPU_EINVAL, "%s: subsampling %d leaves no pixels", who, grid.sub);
    const size_t nl = (size_t)g.w * g.h;
    float *low, *tmp;
    int rc;
    if ((rc = pool_get(ctx, P_TMP, 8 * nl * 4, &low)) || (rc = pool_get(ctx, P_LIN, 8 * nl * 4, &tmp))) return rc;
    g.guide = const_cast<float *>(guide); g.chan[0] = const_cast<float *>(src);
    // the four planes the single-channel statistics use lie next to each other, so that one blur launch takes them all (a grid plane of a
    // subsampled frame is a few dozen workgroups: plane after plane the chip idles); the slots of channels 1 and 2 follow them, unused
    static const int order[8] = {0, 1, 2, 5, 3, 4, 6, 7};
    for (int k = 0; k < 8; ++k) g.low[order[k]] = low + k * nl;
    const int rad = grid.rad;
    if (rad > HBLUR_MAX_RADIUS) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: box radius %d (r / subsampling) is above the %d the blur kernels hold in LDS", who, rad, HBLUR_MAX_RADIUS);
    HIPCHK(ctx, launch_gf_subsample(g, ctx->stream));
    // low[0] I1 -> meanI, low[1] I1*I1 -> corrI, low[2] p1 -> meanp, low[5] I1*p1 -> corrIp
    if ((rc = box_blur_planes(ctx, g.low[0], tmp, 4, nl, g.w, g.h, rad))) return rc;
    HIPCHK(ctx, launch_gf_ab(g, ctx->stream));
    if ((rc = box_blur_planes(ctx, g.low[2], tmp, 2, nl, g.w, g.h, rad))) return rc;   // mean a, mean b
    return ARTGPU_OK;
}

// ... and the whole filter: q with rows of q_stride floats; q may be `guide` or `src` (the last pass is pointwise)
int guided_filter_dev(artgpu_ctx *ctx, const float *guide, const float *src, float *q, size_t q_stride, int W, int H, int r, float epsilon, int subsampling,
                      const char *who)
{
    GuidedArgs g;
    int rc;
    if ((rc = guided_filter_stats(ctx, guide, src, W, H, r, epsilon, subsampling, who, &g))) return rc;
    g.q = q; g.q_stride = q_stride;
    HIPCHK(ctx, launch_gf_finish_plain(g, ctx->stream));
    return ARTGPU_OK;
}

int gaussian_dev(artgpu_ctx *ctx, float *img, float *tmp, int W, int H, double sigma)
{
    // gaussianBlur's dispatch for src == dst (gauss.cc:1436-1523; the box-blur approximation above it is only taken for
    // sigma > 2 of the frame width, far off this path)
    if (!(sigma == sigma) || W < 8 || H < 8) return fail(ctx, ARTGPU_EUNSUPPORTED, "gaussian_blur: sigma %g / size %dx%d not on the device path", sigma, W, H);
    if (sigma < 0.25) return ARTGPU_OK;                 // GAUSS_SKIP: no filtering
    if (sigma < 0.6) {                                  // GAUSS_3X3_LIMIT: separated 3-tap kernel, coefficients in double, passed as float
        double c1 = exp(-1.0 / (2.0 * sigma * sigma));
        const double csum = 2.0 * c1 + 1.0;
        c1 /= csum;
        const double c0 = 1.0 / csum;
        HIPCHK(ctx, launch_gaussian3(img, tmp, W, H, (float)c0, (float)c1, ctx->stream));
        return ARTGPU_OK;
    }
    GaussArgs g = {};
    g.img = img; g.tmp = tmp; g.W = W; g.H = H;
    if (sigma >= 25.0) {                    // GAUSS_DOUBLE (gauss.cc:1393,1520-1523): all-double recursion
        float *t64;
        int rc = pool_get(ctx, P_GAUSS64, (size_t)W * H * sizeof(double), &t64);
        if (rc) return rc;
        g.tmp64 = reinterpret_cast<double *>(t64);
        yvv_factors(sigma, g, true);
    } else {
        yvv_factors((double)(float)sigma, g);   // the Sse functions take `const float sigma`
    }
    HIPCHK(ctx, launch_gaussian(g, ctx->stream));
    return ARTGPU_OK;
}

int detail_mask_dev(artgpu_ctx *ctx, const float *src, size_t src_stride, float *mask, int W, int H,
                    float scaling, float threshold, float ceiling, float factor, float blur, float *scratch /* >= W*H + 2*(W/4)*(H/4) */)
{
    MaskArgs m = {};
    m.src = src; m.src_stride = src_stride; m.mask = mask; m.W = W; m.H = H; m.w4 = W / 4; m.h4 = H / 4;
    m.L2 = scratch + (size_t)W * H; m.m2 = m.L2 + (size_t)m.w4 * m.h4;
    m.scaling = scaling; m.threshold = threshold; m.ceiling = ceiling; m.factor = factor;
    HIPCHK(ctx, launch_detail_mask(m, ctx->stream));
    return gaussian_dev(ctx, mask, scratch, W, H, blur);
}

int nlm_check(artgpu_ctx *ctx, int W, int H)
{
    if (W < 32 || H < 32) return fail(ctx, ARTGPU_EUNSUPPORTED, "nlmeans: image smaller than 32x32");
    // (the tile kernel addresses a plane through 32-bit byte offsets)
    if ((unsigned long long)(W + 14) * (unsigned long long)(H + 14) >= (1ull << 30)) return fail(ctx, ARTGPU_EUNSUPPORTED, "nlmeans: image of %dx%d exceeds 2^30 pixels", W, H);
    return ARTGPU_OK;
}

// denoise::NLMeans (nlmeans.cc:44-320) on a contiguous device plane (rows of W floats), in place; enqueued on ctx->stream.  The caller has checked
// strength != 0, nlm_check and scale >= 1.  Scratch: P_TMP, P_LIN, P_BLOCKS
int nlm_plane_dev(artgpu_ctx *ctx, float *work, int W, int H, float normcoeff, int strength, int detail_thresh, float scale)
{
    NlmArgs a = {};
    a.search_radius = int(std::ceil(5.f / scale));
    a.patch_radius = int(std::ceil(2.f / scale));
    const float t = std::pow(float(strength) / 100.f, 0.9f) / 10.f / scale;
    a.h2 = t * t;
    float amount = float(detail_thresh) / 100.f;
    amount = amount < 0.f ? 0.f : (amount > 0.99f ? 0.99f : amount);   // LIM(x, 0, 0.99)
    a.border = a.search_radius + a.patch_radius;
    a.W = W; a.H = H; a.WW = W + 2 * a.border; a.HH = H + 2 * a.border; a.factor = normcoeff;
    a.ntiles_x = int(std::ceil(float(a.WW) / (150 - 2 * a.border)));
    a.ntiles_y = int(std::ceil(float(a.HH) / (150 - 2 * a.border)));
    float *scratch, *pad;
    int rc = ARTGPU_OK;
    if ((rc = pool_get(ctx, P_TMP, (size_t)W * H * 4 * 2 + 8192 * 4, &a.mask))) return rc;
    a.SW = a.mask + (size_t)W * H; a.explut = a.SW + (size_t)W * H;
    if ((rc = pool_get(ctx, P_LIN, ((size_t)W * H + 2 * (size_t)(W / 4) * (H / 4)) * 4, &scratch))) return rc;
    if ((rc = pool_get(ctx, P_BLOCKS, (size_t)a.WW * a.HH * 4, &pad))) return rc;
    if ((rc = detail_mask_dev(ctx, work, W, a.mask, W, H, normcoeff, 1e-3f * normcoeff, normcoeff, amount, 2.f / scale, scratch))) return rc;
    a.img = work; a.img_stride = W; a.src = pad;
    HIPCHK(ctx, launch_nlm(a, ctx->stream));
    return ARTGPU_OK;
}

// ... on any plane, after nlm_check
int nlm_dev(artgpu_ctx *ctx, artgpu_plane *img, float normcoeff, int strength, int detail_thresh, float scale)
{
    const int W = img->w, H = img->h;
    float *work;
    // a contiguous device plane is worked on where it lies (the kernels read the padded copy `pad` and the mask, and write the plane): two plane
    // copies less per call, 0.16 ms of a 45 MP frame; anything else goes through a contiguous working copy
    const bool in_place = img->on_device && img->row_stride_bytes == (int64_t)W * 4;
    int rc = ARTGPU_OK;
    if (in_place) work = img->p;
    else if ((rc = plane_to_pool(ctx, img, P_SF, &work))) return rc;
    if ((rc = nlm_plane_dev(ctx, work, W, H, normcoeff, strength, detail_thresh, scale))) return rc;
    return in_place ? ARTGPU_OK : pool_to_plane(ctx, work, img);
}

// the radius the guided chroma smoothing works with at `scale`: rounded, never negative
static int dgs_radius(int guided_chroma_radius, double scale)
{
    const int r = (int)std::round(guided_chroma_radius / scale);
    return r > 0 ? r : 0;
}

int denoise_guided_smoothing_check(artgpu_ctx *ctx, int W, int H, int guided_chroma_radius, double scale)
{
    const int r = dgs_radius(guided_chroma_radius, scale);
    const GfGrid grid = gf_grid(W, H, r);
    if (r == 0 || grid.w < 8 || grid.h < 8) return fail(ctx, ARTGPU_EUNSUPPORTED, "denoise_guided_smoothing: radius/scale combination not on the device path");
    return ARTGPU_OK;
}

int denoise_guided_smoothing_dev(artgpu_ctx *ctx, const DevRGB &d, const double ws[9], int guided_chroma_radius, double scale)
{
    const int W = d.w, H = d.h;
    int rc;
    GuidedArgs g = {};
    for (int k = 0; k < 3; ++k) { g.rgb[k] = d.p[k]; g.ws1[k] = ws[3 + k]; }
    g.stride = d.stride; g.W = W; g.H = H; g.epsilon = 0.001f;
    const GfGrid grid = gf_grid(W, H, dgs_radius(guided_chroma_radius, scale));
    g.w = grid.w; g.h = grid.h;
    const size_t n = (size_t)W * H, nl = (size_t)g.w * g.h;
    float *big, *low, *tmp;
    if ((rc = pool_get(ctx, P_SF, 7 * n * 4, &big)) || (rc = pool_get(ctx, P_TMP, 8 * nl * 4, &low)) || (rc = pool_get(ctx, P_LIN, 8 * nl * 4, &tmp))) return rc;
    for (int k = 0; k < 3; ++k) { g.in[k] = big + k * n; g.chan[k] = big + (3 + k) * n; }
    g.guide = big + 6 * n;
    for (int k = 0; k < 8; ++k) g.low[k] = low + k * nl;
    HIPCHK(ctx, launch_gf_prepare(g, ctx->stream));
    HIPCHK(ctx, launch_gf_subsample(g, ctx->stream));
    if ((rc = box_blur_planes(ctx, low, tmp, 8, nl, g.w, g.h, grid.rad))) return rc;              // meanI, corrI, meanp[3], corrIp[3]
    HIPCHK(ctx, launch_gf_ab(g, ctx->stream));
    if ((rc = box_blur_planes(ctx, low + 2 * nl, tmp, 6, nl, g.w, g.h, grid.rad))) return rc;     // mean a[3], mean b[3]
    HIPCHK(ctx, launch_gf_finish(g, ctx->stream));
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

// ---------------------------------------------------------------------------------------------
// guided chroma smoothing
// ---------------------------------------------------------------------------------------------
int artgpu_denoise_guided_smoothing(artgpu_ctx *ctx, artgpu_rgb *img, const double ws[9], int guided_chroma_radius, double scale)
{
    StageScope scope_(ctx, "denoise::denoiseGuidedSmoothing");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !ws || !(scale >= 1.0)) return fail(ctx, ARTGPU_EINVAL, "denoise_guided_smoothing: bad arguments");
    if (guided_chroma_radius == 0) return ARTGPU_OK;   // ipsmoothing.cc:877-879
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    int rc;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "denoise_guided_smoothing")) || (rc = denoise_guided_smoothing_check(ctx, d.w, d.h, guided_chroma_radius, scale)) ||
        (rc = denoise_guided_smoothing_dev(ctx, d, ws, guided_chroma_radius, scale)))
        return rc;
    return unbind_rgb(ctx, img, &d);
}

int artgpu_guided_filter(artgpu_ctx *ctx, const artgpu_plane *guide, const artgpu_plane *src, artgpu_plane *dst, int r, float epsilon, int subsampling)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!guide || !src || !dst || !plane_ok(guide) || !plane_ok(src) || !plane_ok(dst)) return fail(ctx, ARTGPU_EINVAL, "guided_filter: bad plane");
    const int W = src->w, H = src->h;
    if (guide->w != W || guide->h != H || dst->w != W || dst->h != H || r < 0) return fail(ctx, ARTGPU_EINVAL, "guided_filter: size mismatch / negative radius");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H;
    float *big;
    int rc;
    if ((rc = pool_get(ctx, P_SF, 3 * n * 4, &big))) return rc;
    const size_t rowb = (size_t)W * 4;
    HIPCHK(ctx, hipMemcpy2DAsync(big, rowb, guide->p, (size_t)guide->row_stride_bytes, rowb, H, guide->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpy2DAsync(big + n, rowb, src->p, (size_t)src->row_stride_bytes, rowb, H, src->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    if ((rc = guided_filter_dev(ctx, big, big + n, big + 2 * n, (size_t)W, W, H, r, epsilon, subsampling, "guided_filter"))) return rc;
    HIPCHK(ctx, hipMemcpy2DAsync(dst->p, (size_t)dst->row_stride_bytes, big + 2 * n, rowb, rowb, H, dst->on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    if (!dst->on_device) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ARTGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// gaussian blur, detail mask, NL-means
// ---------------------------------------------------------------------------------------------
int artgpu_gaussian_blur(artgpu_ctx *ctx, artgpu_plane *img, double sigma)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(img)) return fail(ctx, ARTGPU_EINVAL, "gaussian_blur: bad plane");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    float *work, *tmp;
    int rc = plane_to_pool(ctx, img, P_SF, &work);
    if (rc) return rc;
    if ((rc = pool_get(ctx, P_TMP, (size_t)img->w * img->h * 4, &tmp))) return rc;
    if ((rc = gaussian_dev(ctx, work, tmp, img->w, img->h, sigma))) return rc;
    return pool_to_plane(ctx, work, img);
}

int artgpu_detail_mask(artgpu_ctx *ctx, const artgpu_plane *src, artgpu_plane *mask, float scaling, float threshold,
                       float ceiling, float factor, float blur)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(src) || !plane_ok(mask) || mask->w != src->w || mask->h != src->h) return fail(ctx, ARTGPU_EINVAL, "detail_mask: bad planes");
    if (src->w < 32 || src->h < 32) return fail(ctx, ARTGPU_EUNSUPPORTED, "detail_mask: image smaller than 32x32");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int W = src->w, H = src->h;
    float *in, *m, *scratch;
    int rc = plane_to_pool(ctx, src, P_SF, &in);
    if (rc) return rc;
    if ((rc = pool_get(ctx, P_TMP, (size_t)W * H * 4, &m))) return rc;
    if ((rc = pool_get(ctx, P_LIN, ((size_t)W * H + 2 * (size_t)(W / 4) * (H / 4)) * 4, &scratch))) return rc;
    if ((rc = detail_mask_dev(ctx, in, W, m, W, H, scaling, threshold, ceiling, factor, blur, scratch))) return rc;
    return pool_to_plane(ctx, m, mask);
}

int artgpu_nlmeans(artgpu_ctx *ctx, artgpu_plane *img, float normcoeff, int strength, int detail_thresh, float scale)
{
    StageScope scope_(ctx, "denoise::NLMeans");
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(img) || !(scale >= 1.f)) return fail(ctx, ARTGPU_EINVAL, "nlmeans: bad arguments");
    if (!strength) return ARTGPU_OK;                       // nlmeans.cc:52-54
    int rc = nlm_check(ctx, img->w, img->h);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return nlm_dev(ctx, img, normcoeff, strength, detail_thresh, scale);
}

} // extern "C"
