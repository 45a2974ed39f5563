// tests/emul/smoothing_ref.cc -- CPU checker for artgpu_smoothing: the region loop of ImProcFunctions::guidedSmoothing
// (rtengine/ipsmoothing.cc:902-1073), find_region (L411-434), guided_smoothing (L334-409) and nlmeans_smoothing (L500-562) restated serially
// on contiguous float planes, with every intermediate plane the reference has (the working copy, iR / iG / iB, the guide, iY).
// Test infrastructure only; built on first use with -ffp-contract=off.
//
// The leaves are liboracle's restatements: oracle_guided_filter (rtengine::guidedFilter; guidedFilterLog is written out around it with
// oracle_xlin2log / oracle_xlog2lin exactly as oracle_guided_filter_log does, so that q can be counted before the exponential),
// oracle_nlmeans (denoise::NLMeans), and Color::rgb2yuv / yuv2rgb with the double matrix as oracle_denoise_guided_smoothing states them.
// ipsmoothing.cc itself needs improcfun.h and FFTW and is not compiled anywhere: the loop is parity-unpinned, its leaves are pinned, and
// tests/test_smoothing_checker.py ties GUIDED C to oracle_denoise_guided_smoothing bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

extern "C" {
void oracle_guided_filter(const float *guide, const float *src, float *dst, int W, int H, int r, float epsilon, int subsampling);
void oracle_nlmeans(float *img, int W, int H, float normcoeff, int strength, int detail_thresh, float scale);
float oracle_xlin2log(float x, float base);
float oracle_xlog2lin(float x, float base);
}

extern "C" {
struct sm_ref_region {            // the layout of artgpu_smoothing_region with a contiguous W * H plane (or NULL) for the mask
    int32_t mode, channel, radius, epsilon;
    double sigma;
    int32_t iterations, nldetail;
    double falloff;
    int32_t nlstrength, numblades;
    double angle, curvature, offset;
    int32_t noise_strength, noise_coarseness;
    double halation_size, halation_color, wav_strength;
    int32_t wav_levels, pad_;
    double wav_gamma;
    const float *mask;
};
struct sm_ref_info {              // the layout of artgpu_smoothing_info
    int32_t r;
    float epsilon;
    int32_t min_x, min_y, max_x, max_y, cropped, work_w, work_h, subsampling, box_radius, skipped;
};
struct sm_ref_counts {
    long long cropped, full_frame, skipped_radius, skipped_strength, skipped_empty;
    long long bump_one, chan_clamped, q_clamped, mask_between, mask_zero_in_box;
};
}

namespace {

enum { GUIDED = 0, NLMEANS = 3, WAVELETS = 8, CH_L = 0, CH_C = 1, CH_LC = 2 };
enum { SKIP_RADIUS = 1, SKIP_STRENGTH = 2, SKIP_EMPTY = 3 };
constexpr int MIN_SIZE = 5, MAX_BOX_RADIUS = 900;

inline float maxf(float a, float b) { return a < b ? b : a; }       // rtengine::max

int calculate_subsampling(int w, int h, int r)                       // guidedfilter.cc:58-75
{
    if (r == 1) return 1;
    if (std::max(w, h) <= 600) return 1;
    for (int s = 5; s > 0; --s)
        if (r % s == 0) return s;
    return std::max(2, std::min(r / 2, 4));         // LIM(r / 2, 2, 4)
}

struct Yuv {
    const double *ws;                                                // TMatrix row 1 at ws[3..5]
    float lum(float r, float g, float b) const { return r * ws[3] + g * ws[4] + b * ws[5]; }                 // Color::rgbLuminance (double products)
    void rgb2yuv(float r, float g, float b, float &Y, float &u, float &v) const { Y = lum(r, g, b); u = Y - b; v = r - Y; }
    void yuv2rgb(float Y, float u, float v, float &r, float &g, float &b) const
    {
        b = Y - u;
        r = v + Y;
        g = (Y - r * ws[3] - b * ws[5]) / ws[4];
    }
};

// find_region (L411-434)
void find_region(const float *mask, int W, int H, int &min_x, int &min_y, int &max_x, int &max_y)
{
    min_x = W - 1; min_y = H - 1; max_x = 0; max_y = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            if (mask[(size_t)y * W + x] > 0.f) {
                min_x = std::min(min_x, x); max_x = std::max(max_x, x);
                min_y = std::min(min_y, y); max_y = std::max(max_y, y);
            }
    ++max_x;
    ++max_y;
}

// guidedFilterLog(guide, 10.f, chan, r, epsilon) (guidedfilter.cc:244-265); guide may be chan
void guided_filter_log(const float *guide, float *chan, int W, int H, int r, float eps, sm_ref_counts *cn)
{
    const size_t n = (size_t)W * H;
    for (size_t k = 0; k < n; ++k) {
        if (chan[k] < 0.f) ++cn->chan_clamped;
        chan[k] = oracle_xlin2log(maxf(chan[k], 0.f), 10.f);
    }
    oracle_guided_filter(guide, chan, chan, W, H, r, eps, 0);
    for (size_t k = 0; k < n; ++k) {
        if (chan[k] < 0.f) ++cn->q_clamped;
        chan[k] = oracle_xlog2lin(maxf(chan[k], 0.f), 10.f);
    }
}

// guided_smoothing (L334-409) with r > 0
void guided_smoothing(float *R, float *G, float *B, int W, int H, const Yuv &yuv, int chan, int r, float epsilon, sm_ref_counts *cn)
{
    const size_t n = (size_t)W * H;
    std::vector<float> iR(R, R + n), iG(G, G + n), iB(B, B + n);
    if (chan == CH_LC) {
        guided_filter_log(R, R, W, H, r, epsilon, cn);
        guided_filter_log(G, G, W, H, r, epsilon, cn);
        guided_filter_log(B, B, W, H, r, epsilon, cn);
        return;
    }
    std::vector<float> guide(n);
    for (size_t k = 0; k < n; ++k) guide[k] = oracle_xlin2log(maxf(yuv.lum(R[k], G[k], B[k]), 0.f), 10.f);
    guided_filter_log(guide.data(), R, W, H, r, epsilon, cn);
    guided_filter_log(guide.data(), G, W, H, r, epsilon, cn);
    guided_filter_log(guide.data(), B, W, H, r, epsilon, cn);
    for (size_t k = 0; k < n; ++k) {
        float iY, iu, iv, oY, ou, ov;
        yuv.rgb2yuv(iR[k], iG[k], iB[k], iY, iu, iv);
        yuv.rgb2yuv(R[k], G[k], B[k], oY, ou, ov);
        if (chan == CH_L) {
            ou = iu;
            ov = iv;
        } else {
            if (!(oY > 1e-5f)) ++cn->bump_one;
            const float bump = oY > 1e-5f ? iY / oY : 1.f;
            ou *= bump;
            ov *= bump;
            oY = iY;
        }
        yuv.yuv2rgb(oY, ou, ov, R[k], G[k], B[k]);
    }
}

// nlmeans_smoothing (L500-562)
void nlmeans_smoothing(float *R, float *G, float *B, int W, int H, const Yuv &yuv, int chan, int strength, int detail, int iterations, double scale)
{
    const size_t n = (size_t)W * H;
    std::vector<float> iY;
    if (chan == CH_L) {
        iY.resize(n);
        for (size_t k = 0; k < n; ++k) { float u, v; yuv.rgb2yuv(R[k], G[k], B[k], iY[k], u, v); }
        for (int i = 0; i < iterations; ++i) oracle_nlmeans(iY.data(), W, H, 1.f, strength, detail, (float)scale);
        for (size_t k = 0; k < n; ++k) {
            float Y, u, v;
            yuv.rgb2yuv(R[k], G[k], B[k], Y, u, v);
            yuv.yuv2rgb(iY[k], u, v, R[k], G[k], B[k]);
        }
        return;
    }
    if (chan == CH_C) {
        iY.resize(n);
        for (size_t k = 0; k < n; ++k) { float u, v; yuv.rgb2yuv(R[k], G[k], B[k], iY[k], u, v); }
    }
    for (int i = 0; i < iterations; ++i) {
        oracle_nlmeans(R, W, H, 1.f, strength, detail, (float)scale);
        oracle_nlmeans(G, W, H, 1.f, strength, detail, (float)scale);
        oracle_nlmeans(B, W, H, 1.f, strength, detail, (float)scale);
    }
    if (chan == CH_C)
        for (size_t k = 0; k < n; ++k) {
            float Y, u, v;
            yuv.rgb2yuv(R[k], G[k], B[k], Y, u, v);
            yuv.yuv2rgb(iY[k], u, v, R[k], G[k], B[k]);
        }
}

struct Plan { sm_ref_info info; int w, h; };

// what the call derives per region before it touches the image; returns 1 for what the device path does not support
int plan_region(const sm_ref_region &r, int W, int H, const int *box /* find_region's and `no pixel above zero`, or nullptr for a NULL mask */, double scale, Plan *pl)
{
    *pl = Plan{};
    sm_ref_info &o = pl->info;
    int min_x = 0, min_y = 0, max_x = W, max_y = H;
    if (box) {
        min_x = box[0]; min_y = box[1]; max_x = box[2]; max_y = box[3];
        if (box[4]) { o.skipped = SKIP_EMPTY; return 0; }                                // (undefined in the reference: skipped here)
    }
    int ww = max_x - min_x, hh = max_y - min_y;
    if (ww * hh < (W * H) / 2) o.cropped = 1;                                           // L957
    else { min_x = 0; min_y = 0; max_x = W; max_y = H; ww = W; hh = H; }
    o.min_x = min_x; o.min_y = min_y; o.max_x = max_x; o.max_y = max_y; o.work_w = ww; o.work_h = hh;
    if (r.mode == GUIDED) {
        o.epsilon = std::max(0.001f * std::pow(2, -r.epsilon), 1e-6);                   // L1040
        o.r = std::max(int(std::round(r.radius / scale)), 0);                          // L348
        if (o.r == 0) { o.skipped = SKIP_RADIUS; return 0; }
        o.subsampling = calculate_subsampling(ww, hh, o.r);
        pl->w = ww / o.subsampling; pl->h = hh / o.subsampling;
        if (pl->w < MIN_SIZE || pl->h < MIN_SIZE) return 1;
        const float r1 = float(o.r) / o.subsampling;                                    // f_mean (guidedfilter.cc:160-167)
        int rad = r1;
        const int hi = (std::min(pl->w, pl->h) - 1) / 2 - 1;
        rad = std::max(0, std::min(rad, hi));                                           // LIM(rad, 0, hi)
        o.box_radius = rad;
        if (rad > MAX_BOX_RADIUS) return 1;
    } else {
        if (r.nlstrength == 0) { o.skipped = SKIP_STRENGTH; return 0; }
        if (ww < 32 || hh < 32) return 1;
        if ((unsigned long long)(ww + 14) * (unsigned long long)(hh + 14) >= (1ull << 30)) return 1;
        if (!(scale >= 1.0)) return 1;
    }
    return 0;
}

} // namespace

extern "C" {

int sm_ref_sizes(int which) { return which == 0 ? (int)sizeof(sm_ref_region) : (int)sizeof(sm_ref_info); }

// 0: done; 1: unsupported on the device path (planes untouched); 2: bad arguments
int sm_ref_tool(float *R, float *G, float *B, int W, int H, const sm_ref_region *regions, int n, const double ws[9], double scale, sm_ref_info *info,
                sm_ref_counts *cn)
{
    sm_ref_counts dummy = {};
    if (!cn) cn = &dummy;
    if (n < 0 || !(scale > 0.0)) return 2;
    const size_t np = (size_t)W * H;
    const Yuv yuv = {ws};
    std::vector<Plan> plans(n);
    for (int i = 0; i < n; ++i) {
        const sm_ref_region &r = regions[i];
        if (r.mode < GUIDED || r.mode > WAVELETS || r.channel < CH_L || r.channel > CH_LC) return 2;
        if (r.mode != GUIDED && r.mode != NLMEANS) return 1;
        if (r.iterations < 1) return 1;
        if (r.mode == NLMEANS && r.nlstrength != 0 && !(scale >= 1.0)) return 1;
    }
    for (int i = 0; i < n; ++i) {                                     // (all masks exist before the region loop, L929)
        int box[5] = {0, 0, 0, 0, 0};
        if (regions[i].mask) {
            find_region(regions[i].mask, W, H, box[0], box[1], box[2], box[3]);
            box[4] = std::none_of(regions[i].mask, regions[i].mask + np, [](float m) { return m > 0.f; });
        }
        if (plan_region(regions[i], W, H, regions[i].mask ? box : nullptr, scale, &plans[i])) return 1;
    }
    const float f1 = 1.f / 65535.f;
    float *img[3] = {R, G, B};
    for (int c = 0; c < 3; ++c)
        for (size_t k = 0; k < np; ++k) img[c][k] *= f1;              // normalizeFloatTo1 (L938)
    for (int i = 0; i < n; ++i) {
        const sm_ref_region &r = regions[i];
        const sm_ref_info &o = plans[i].info;
        if (info) info[i] = o;
        if (o.skipped == SKIP_EMPTY) { ++cn->skipped_empty; continue; }
        ++(o.cropped ? cn->cropped : cn->full_frame);
        const int ww = o.work_w, hh = o.work_h;
        const size_t nw = (size_t)ww * hh;
        std::vector<float> work[3];                                   // `working` (L957-980)
        for (int c = 0; c < 3; ++c) {
            work[c].resize(nw);
            for (int y = 0; y < hh; ++y) std::memcpy(&work[c][(size_t)y * ww], &img[c][(size_t)(y + o.min_y) * W + o.min_x], sizeof(float) * ww);
        }
        if (r.mode == NLMEANS) {
            if (r.nlstrength == 0) ++cn->skipped_strength;
            nlmeans_smoothing(work[0].data(), work[1].data(), work[2].data(), ww, hh, yuv, r.channel, r.nlstrength, r.nldetail, r.iterations, scale);
        } else {
            if (o.r == 0) ++cn->skipped_radius;
            else
                for (int it = 0; it < r.iterations; ++it) guided_smoothing(work[0].data(), work[1].data(), work[2].data(), ww, hh, yuv, r.channel, o.r, o.epsilon, cn);
        }
        for (int y = o.min_y; y < o.max_y; ++y)                       // L1050-1064
            for (int x = o.min_x; x < o.max_x; ++x) {
                const size_t k = (size_t)y * W + x, t = (size_t)(y - o.min_y) * ww + (x - o.min_x);
                const float m = r.mask ? r.mask[k] : 1.f;
                if (m > 0.f && m < 1.f) ++cn->mask_between;
                if (m == 0.f) ++cn->mask_zero_in_box;
                for (int c = 0; c < 3; ++c) img[c][k] = m * work[c][t] + (1.f - m) * img[c][k];     // intp
            }
    }
    for (int c = 0; c < 3; ++c)
        for (size_t k = 0; k < np; ++k) img[c][k] *= 65535.f;         // normalizeFloatTo65535 (L1067)
    return 0;
}

} // extern "C"
