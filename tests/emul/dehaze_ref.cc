// tests/emul/dehaze_ref.cc -- CPU checker for artgpu_dehaze: ImProcFunctions::dehaze (rtengine/ipdehaze.cc:64-512) restated serially,
// in the reference's order and with its intermediate planes (R, G, B, dark, add_haze, t all exist here), on contiguous float planes.
// Test infrastructure only; built on first use with -ffp-contract=off (rtengine is built without contraction).
//
// rtengine::guidedFilter, boxblur (boxblur.h:318), FlatCurve and LUTf::operator[](float) are liboracle's restatements
// (oracle_guided_filter, oracle_boxblur_ring, oracle_flat_curve_*, oracle_lutf), not a third copy.
// std::log / std::exp in ipdehaze.cc are qualified and take floats: the float overloads.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <queue>
#include <utility>
#include <vector>

extern "C" {
void oracle_boxblur_ring(float *img, int radius, int W, int H);
void oracle_guided_filter(const float *guide, const float *src, float *dst, int W, int H, int r, float epsilon, int subsampling);
void *oracle_flat_curve_new(const double *pts, int npts, int periodic, int ppn, double identity);
double oracle_flat_curve_get(const void *h, double t);
void oracle_flat_curve_free(void *h);
float oracle_lutf(const float *data, int size, float index);
}

namespace {
template <typename T> inline const T &rt_min(const T &a, const T &b) { return b < a ? b : a; }   // rt_math.h:55-58
template <typename T> inline const T &rt_max(const T &a, const T &b) { return a < b ? b : a; }   // rt_math.h:73-76
inline float rt_min3(float a, float b, float c) { return rt_min(rt_min(a, b), c); }                 // min(min(a, b), min(c))
inline float rt_min4(float a, float b, float c, float d) { return rt_min(rt_min(a, b), rt_min(c, d)); }
inline float rt_max4(float a, float b, float c, float d) { return rt_max(rt_max(a, b), rt_max(c, d)); }
inline float LIM01(float a) { return rt_max(0.f, rt_min(a, 1.f)); }
const float RT_INFINITY_F = std::numeric_limits<float>::infinity();

inline float rgbLuminance(float r, float g, float b, const double *ws) { return r * ws[3] + g * ws[4] + b * ws[5]; }   // color.h:204-207
}

extern "C" {

struct dh_ref_params { int32_t show_depth_map, depth, luminance, blackpoint; };
struct dh_ref_info {             // the layout of artgpu_dehaze_info
    int32_t haze_detected, patchsize, small_w, small_h;
    float maxval, black[3], ambient[3], max_t, t0;
};
struct dh_ref_hand { int32_t use; float ambient[3], max_t, maxval, black[3]; };
struct dh_ref_counts {
    long long add_haze, y_small, won_t, won_t0, won_tl, dark_clipped_low, dark_clipped_high, partial_patches, no_haze, depth_below, depth_above;
};

void dh_ref_thumb_size(int W, int H, int *ww, int *hh)
{
    constexpr int sizecap = 200;
    float r = float(W) / float(H);
    *ww = r >= 1.f ? sizecap : float(sizecap) / r;
    *hh = r >= 1.f ? float(sizecap) / r : sizecap;
}

// L419-424 with Color::gamma2curve of color.cc:241-244
void dh_ref_strength_lut(const double *pts, int npts, float *strength)
{
    std::vector<float> gamma2curve(65536);
    for (int i = 0; i < 65536; i++) {
        const double x = i / 65535.0;
        gamma2curve[i] = x <= 0.003040 ? x * 12.92310 : 1.055 * exp(log(x) / 2.4) - 0.055;
    }
    for (int i = 0; i < 65536; i++) gamma2curve[i] *= 65535.f;
    // FlatCurve(points, false): kind stays FCT_Empty for fewer than five values or another curve type; identity value 0.5
    const bool minmax = npts > 4 && (int)pts[0] == 1;
    void *curve = oracle_flat_curve_new(minmax ? pts : nullptr, npts, 0, 1000, 0.5);
    for (int i = 0; i < 65536; ++i) strength[i] = (oracle_flat_curve_get(curve, gamma2curve[i] / 65535.f) - 0.5f) * 1.3f;
    oracle_flat_curve_free(curve);
}

// get_dark_channel (L89-125)
int dh_ref_dark_channel(const float *R, const float *G, const float *B, int W, int H, int patchsize, const float *ambient, int clip, float *dst,
                        dh_ref_counts *cn)
{
    for (int y = 0; y < H; y += patchsize) {
        const int pH = rt_min(y + patchsize, H);
        for (int x = 0; x < W; x += patchsize) {
            float val = RT_INFINITY_F;
            const int pW = rt_min(x + patchsize, W);
            if (cn && (pH - y < patchsize || pW - x < patchsize)) cn->partial_patches++;
            for (int yy = y; yy < pH; ++yy) {
                for (int xx = x; xx < pW; ++xx) {
                    float r = R[(size_t)yy * W + xx];
                    float g = G[(size_t)yy * W + xx];
                    float b = B[(size_t)yy * W + xx];
                    if (ambient) {
                        r /= ambient[0];
                        g /= ambient[1];
                        b /= ambient[2];
                    }
                    val = rt_min4(val, r, g, b);
                }
            }
            if (clip) {
                if (cn && val < 0.f) cn->dark_clipped_low++;
                if (cn && val > 1.f) cn->dark_clipped_high++;
                val = LIM01(val);
            }
            for (int yy = y; yy < pH; ++yy) std::fill(dst + (size_t)yy * W + x, dst + (size_t)yy * W + pW, val);
        }
    }
    return (W / patchsize + ((W % patchsize) > 0)) * (H / patchsize + ((H % patchsize) > 0));
}

// estimate_ambient_light (L128-230) behind get_dark_channel(RR, GG, BB, D, 2, nullptr, false) (L385-386); ambient stays zero on -1
float dh_ref_estimate_ambient(const float *R, const float *G, const float *B, int W, int H, float ambient[3])
{
    ambient[0] = ambient[1] = ambient[2] = 0.f;
    std::vector<float> dark((size_t)W * H);
    const int patchsize = 2;
    const int npatches = dh_ref_dark_channel(R, G, B, W, H, patchsize, nullptr, 0, dark.data(), nullptr);
    const auto get_percentile = [](std::priority_queue<float> &q, float prcnt) -> float {
        size_t n = rt_max<size_t>(1, rt_min<size_t>(q.size() * prcnt, q.size()));
        while (q.size() > n) q.pop();
        return q.top();
    };
    const auto OOG = [](float val, float high) -> bool { return (val < 0.f) || (val > high); };
    float darklim = RT_INFINITY_F;
    {
        std::priority_queue<float> p;
        for (int y = 0; y < H; y += patchsize)
            for (int x = 0; x < W; x += patchsize)
                if (!OOG(dark[(size_t)y * W + x], 1.f - 1e-5f)) p.push(dark[(size_t)y * W + x]);
        if (p.empty()) return -1.f;
        darklim = get_percentile(p, 0.95);
    }
    std::vector<std::pair<int, int>> patches;
    patches.reserve(npatches);
    for (int y = 0; y < H; y += patchsize)
        for (int x = 0; x < W; x += patchsize)
            if (dark[(size_t)y * W + x] >= darklim && !OOG(dark[(size_t)y * W + x], 1.f)) patches.push_back(std::make_pair(x, y));
    float bright_lim = RT_INFINITY_F;
    {
        std::priority_queue<float> l;
        for (auto &p : patches) {
            const int pW = rt_min(p.first + patchsize, W);
            const int pH = rt_min(p.second + patchsize, H);
            for (int y = p.second; y < pH; ++y)
                for (int x = p.first; x < pW; ++x) l.push(R[(size_t)y * W + x] + G[(size_t)y * W + x] + B[(size_t)y * W + x]);
        }
        if (l.empty()) return -1.f;
        bright_lim = get_percentile(l, 0.95);
    }
    double rr = 0, gg = 0, bb = 0;
    int n = 0;
    for (auto &p : patches) {
        const int pW = rt_min(p.first + patchsize, W);
        const int pH = rt_min(p.second + patchsize, H);
        for (int y = p.second; y < pH; ++y) {
            for (int x = p.first; x < pW; ++x) {
                float r = R[(size_t)y * W + x];
                float g = G[(size_t)y * W + x];
                float b = B[(size_t)y * W + x];
                if (r + g + b >= bright_lim) {
                    rr += r;
                    gg += g;
                    bb += b;
                    ++n;
                }
            }
        }
    }
    n = std::max(n, 1);
    ambient[0] = rr / n;
    ambient[1] = gg / n;
    ambient[2] = bb / n;
    return darklim > 0 ? -1.125f * std::log(darklim) : std::log(std::numeric_limits<float>::max()) / 2;
}

static void rescale_nearest(const float *src, int sW, int sH, float *dst, int dW, int dH)       // rescale.h:77-92
{
    for (int y = 0; y < dH; ++y) {
        int sy = y * sH / dH;
        for (int x = 0; x < dW; ++x) {
            int sx = x * sW / dW;
            dst[(size_t)y * dW + x] = src[(size_t)sy * sW + sx];
        }
    }
}

// ImProcFunctions::dehaze (L306-512) in place on three contiguous W x H planes.  hand (may be NULL, or use == 0): maxval, black, ambient and
// max_t to use in place of the checker's own.  Returns 0, or -1 where the reference would read out of bounds (planes untouched).
int dh_ref_dehaze(float *ir, float *ig, float *ib, int W, int H, const double *pts, int npts, const dh_ref_params *params, const double *ws,
                  double scale, const dh_ref_hand *hand, dh_ref_info *info, dh_ref_counts *cn)
{
    const size_t N = (size_t)W * H;
    const bool handed = hand && hand->use;
    std::memset(info, 0, sizeof *info);
    std::memset(cn, 0, sizeof *cn);
    int ww, hh;
    dh_ref_thumb_size(W, H, &ww, &hh);
    const int bradius = std::max(std::max(ww, hh) / 20, 1);
    if (params->blackpoint && std::min(ww, hh) < 2 * bradius + 1) return -1;
    float *img[3] = {ir, ig, ib};
    // normalize (L64-80)
    float maxval = 0.f;
    for (size_t k = 0; k < N; ++k) maxval = rt_max4(maxval, ir[k], ig[k], ib[k]);
    maxval = rt_max(maxval * 2.f, 65535.f);
    if (handed) maxval = hand->maxval;
    {
        const float f = 1.f / maxval;
        for (int c = 0; c < 3; ++c)
            for (size_t k = 0; k < N; ++k) img[c][k] *= f;
    }
    const float maxchan = maxval;
    float black[3] = {0.f, 0.f, 0.f};
    if (params->blackpoint) {                                                   // subtract_black (L249-301)
        black[0] = black[1] = black[2] = RT_INFINITY_F;
        std::vector<float> t[3];
        for (int c = 0; c < 3; ++c) {
            t[c].resize((size_t)ww * hh);
            rescale_nearest(img[c], W, H, t[c].data(), ww, hh);
            oracle_boxblur_ring(t[c].data(), bradius, ww, hh);
        }
        for (int y = 0; y < hh; ++y)
            for (int x = 0; x < ww; ++x)
                for (int c = 0; c < 3; ++c) black[c] = std::min(black[c], t[c][(size_t)y * ww + x]);
        const float scaling = float(params->blackpoint) / 100.f;
        for (int c = 0; c < 3; ++c) black[c] = std::max(0.f, black[c] * scaling);
        if (handed)
            for (int c = 0; c < 3; ++c) black[c] = hand->black[c];
        for (size_t k = 0; k < N; ++k)
            for (int c = 0; c < 3; ++c) img[c][k] = std::max(img[c][k] - black[c], 0.f);
    }
    int patchsize = rt_max(int(5 / scale), 2);
    float ambient[3];
    float max_t = 0.f;
    std::vector<float> dark(N), G(N), B(N);
    float *R = dark.data();                                                     // "R and dark can safely use the same buffer"
    oracle_guided_filter(ir, ir, R, W, H, patchsize, 1e-1, 0);                  // extract_channels (L233-246)
    oracle_guided_filter(ig, ig, G.data(), W, H, patchsize, 1e-1, 0);
    oracle_guided_filter(ib, ib, B.data(), W, H, patchsize, 1e-1, 0);
    {
        std::vector<float> RR((size_t)ww * hh), GG((size_t)ww * hh), BB((size_t)ww * hh);
        rescale_nearest(R, W, H, RR.data(), ww, hh);
        rescale_nearest(G.data(), W, H, GG.data(), ww, hh);
        rescale_nearest(B.data(), W, H, BB.data(), ww, hh);
        max_t = dh_ref_estimate_ambient(RR.data(), GG.data(), BB.data(), ww, hh, ambient);
        if (handed) {
            max_t = hand->max_t;
            for (int c = 0; c < 3; ++c) ambient[c] = hand->ambient[c];
        }
    }
    patchsize = rt_max(rt_max(W, H) / 600, 2);
    info->patchsize = patchsize; info->small_w = ww; info->small_h = hh; info->maxval = maxval; info->max_t = max_t;
    for (int c = 0; c < 3; ++c) { info->black[c] = black[c]; info->ambient[c] = ambient[c]; }
    if (max_t < 0.f) {                                                          // L387-393
        cn->no_haze = 1;
        for (int c = 0; c < 3; ++c)
            for (size_t k = 0; k < N; ++k) img[c][k] *= maxchan;
        return 0;
    }
    info->haze_detected = 1;
    dh_ref_dark_channel(R, G.data(), B.data(), W, H, patchsize, ambient, 1, dark.data(), cn);      // dst aliases R: a patch is read before it is filled
    std::vector<unsigned char> add_haze(N);
    std::vector<float> strength(65536);
    dh_ref_strength_lut(pts, npts, strength.data());
    for (size_t k = 0; k < N; ++k) {
        float Y = rgbLuminance(ir[k], ig[k], ib[k], ws) * maxchan;
        float s = oracle_lutf(strength.data(), 65536, Y);
        add_haze[k] = s < 0;
        dark[k] = 1.f - std::abs(s) * dark[k];
    }
    const int radius = patchsize * 4;
    const float epsilon = 1e-5;
    float *t = dark.data();
    oracle_guided_filter(ib, dark.data(), t, W, H, radius, epsilon, 0);
    float depth = -float(params->depth) / 100.f;
    const float teps = 1e-6f;
    const float t0 = rt_max(teps, std::exp(depth * max_t));
    info->t0 = t0;
    const bool luminance = params->luminance;
    const float ambientY = rgbLuminance(ambient[0], ambient[1], ambient[2], ws);
    for (size_t k = 0; k < N; ++k) {
        float rgb[3] = {ir[k], ig[k], ib[k]};
        float tl = 1.f - rt_min3(rgb[0] / ambient[0], rgb[1] / ambient[1], rgb[2] / ambient[2]);
        const float m1 = rt_max(t[k], t0), m2 = tl + teps;
        float mt = rt_max(m1, m2);
        if (m1 < m2) cn->won_tl++;
        else if (t[k] < t0) cn->won_t0++;
        else cn->won_t++;
        if (params->show_depth_map) {
            if (1.f - mt < 0.f) cn->depth_below++;
            if (1.f - mt > 1.f) cn->depth_above++;
            ir[k] = ig[k] = ib[k] = LIM01(1.f - mt);
        } else if (luminance) {
            float Y = rgbLuminance(rgb[0], rgb[1], rgb[2], ws);
            float YY = (Y - ambientY) / mt + ambientY;
            if (Y > 1e-5f) {
                if (add_haze[k]) {
                    YY = Y + Y - YY;
                    cn->add_haze++;
                }
                float f = YY / Y;
                ir[k] = rgb[0] * f;
                ig[k] = rgb[1] * f;
                ib[k] = rgb[2] * f;
            } else {
                cn->y_small++;
            }
        } else {
            float r = (rgb[0] - ambient[0]) / mt + ambient[0];
            float g = (rgb[1] - ambient[1]) / mt + ambient[1];
            float b = (rgb[2] - ambient[2]) / mt + ambient[2];
            if (add_haze[k]) {
                cn->add_haze++;
                ir[k] += (ir[k] - r);
                ig[k] += (ig[k] - g);
                ib[k] += (ib[k] - b);
            } else {
                ir[k] = r;
                ig[k] = g;
                ib[k] = b;
            }
        }
    }
    for (int c = 0; c < 3; ++c)
        for (size_t k = 0; k < N; ++k) img[c][k] *= maxchan;                    // restore (L83-86)
    return 0;
}

} // extern "C"
