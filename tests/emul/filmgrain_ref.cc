// tests/emul/filmgrain_ref.cc -- CPU checker for artgpu_film_grain / artgpu_add_noise / artgpu_grain_table / artgpu_grain_indices:
// ImProcFunctions::filmGrain's region derivation (rtengine/ipgrain.cc:40-69), add_noise (rtengine/ipsmoothing.cc:565-695) and the frame
// guidedSmoothing puts around a NOISE region (L933-1067), restated serially.  Test infrastructure only; built on first use with
// -ffp-contract=off.  Written independently of the library's host code.
//
// The generator is rng.h's as it stands: a 64-bit state, the mask ~(2ULL << 48), stepping only -- no 48-bit shortcut and no jump-ahead,
// which are the library's business and what the tests compare against this.  xlogf is liboracle's scalar form.
// Two definitions: the draws are taken in the single-threaded raster order; Convolution is the direct sum
// acc = acc + k[i][j] * nb[clamp(y + i - c)][clamp(x + j - c)] in fp32, i outer, j inner.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

extern "C" float oracle_xlogf_s(float d);

namespace {

struct Rng {                                        // rng.h:31-57
    uint64_t seed_;
    explicit Rng(uint32_t seed) : seed_(seed) {}
    uint64_t next() const { return ((seed_ * 25214903917ULL) + 11U) & ~(2ULL << 48); }
    uint32_t randint(uint32_t upper_bound = std::numeric_limits<uint32_t>::max())
    {
        seed_ = next();
        return uint32_t(seed_ >> 16U) % upper_bound;
    }
    float randfloat()
    {
        uint32_t ub = std::numeric_limits<int>::max();
        return float(randint(ub)) / float(ub);
    }
};

struct Normal {                                     // rng.h:61-90, mean 0, std_dev 1
    const float mean_ = 0, std_dev_ = 1;
    float spare_ = 0;
    bool has_spare_ = false;
    float operator()(Rng &rng)
    {
        if (has_spare_) {
            has_spare_ = false;
            return spare_ * std_dev_ + mean_;
        }
        double u, v, s;
        do {
            u = rng.randfloat() * 2.f - 1.f;
            v = rng.randfloat() * 2.f - 1.f;
            s = u * u + v * v;
        } while (s >= 1.f || s == 0.f);
        s = sqrtf(-2.f * oracle_xlogf_s(s) / s);
        spare_ = v * s;
        has_spare_ = true;
        return mean_ + std_dev_ * u * s;
    }
};

constexpr uint32_t NORMD = 5233;

inline float lim01(float a) { return std::max(0.f, std::min(a, 1.f)); }
inline float intp(float a, float b, float c) { return a * b + (1.f - a) * c; }
inline float lum(float r, float g, float b, const double *ws) { return r * ws[3] + g * ws[4] + b * ws[5]; }
inline void rgb2yuv(float r, float g, float b, float &Y, float &u, float &v, const double *ws)
{
    Y = lum(r, g, b, ws);
    u = Y - b;
    v = r - Y;
}
inline void yuv2rgb(float Y, float u, float v, float &r, float &g, float &b, const double *ws)
{
    b = Y - u;
    r = v + Y;
    g = (Y - r * ws[3] - b * ws[5]) / ws[4];
}

int cone(float radius, std::vector<float> &k)
{
    const int sz = int(std::ceil(radius)) * 2 + 1;
    k.assign((size_t)sz * sz, 0.f);
    const int c = sz / 2;
    double totd = 0.0;
    for (int i = 0; i < sz; ++i)
        for (int j = 0; j < sz; ++j) {
            float r = std::sqrt((i - c) * (i - c) + (j - c) * (j - c));
            float d = r - radius;
            k[i * sz + j] = d < 0.f ? 1.f : std::max(1.f - d, 0.f);
            totd += k[i * sz + j];
        }
    const float tot = totd;
    for (float &t : k) t /= tot;
    return sz;
}

void direct_sum(const std::vector<float> &nb, int W, int H, const std::vector<float> &k, int sz, std::vector<float> &out)
{
    const int c = sz / 2;
    out.resize(nb.size());
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            float acc = 0.f;
            for (int i = 0; i < sz; ++i)
                for (int j = 0; j < sz; ++j) {
                    const int yy = std::min(std::max(y + i - c, 0), H - 1), xx = std::min(std::max(x + j - c, 0), W - 1);
                    acc = acc + k[i * sz + j] * nb[(size_t)yy * W + xx];
                }
            out[(size_t)y * W + x] = acc;
        }
}

// add_noise on three contiguous W x H planes; chan: 0 L, 1 C, 2 LC (the enum's order, L327-331)
void add_noise(float *R, float *G, float *B, int W, int H, const double *ws, int strength, int coarseness, double scale, int chan)
{
    const size_t n = (size_t)W * H;
    const float sf = lim01(float(strength) / (chan == 0 ? 200.f : 100.f)) / scale;
    const float radius = (0.5f + 1.75f * float(coarseness) / 100.f) / scale;
    Rng rng(42 + chan + coarseness);
    std::vector<float> kernel;
    const int sz = cone(radius, kernel);
    float normd[NORMD];
    Normal d;
    for (uint32_t i = 0; i < NORMD; ++i) normd[i] = d(rng);

    const auto noise = [&](float *a, int ch) {
        const float chan_sd[5] = {1.f, 0.7f, 1.f, 1.3f};
        const float c01 = float(coarseness) / 100.f;
        const float c = 655.35f / (20.f + std::pow(c01, 0.5f) * 80.f);
        const float sd = chan_sd[ch];
        std::vector<float> noisebuf(n), conv;
        for (size_t t = 0; t < n; ++t) {
            float v = a[t];
            float mu = std::max(v, 0.f) * c;
            float r = normd[rng.randint(NORMD)] * sd;
            float m = mu + sqrtf(mu) * r;
            noisebuf[t] = m / c - v;
        }
        direct_sum(noisebuf, W, H, kernel, sz, conv);
        for (size_t t = 0; t < n; ++t) a[t] = std::max(a[t] + sf * conv[t], 0.f);
    };

    if (chan == 2) {
        noise(R, 1); noise(G, 2); noise(B, 3);
    } else if (chan == 0) {
        for (size_t t = 0; t < n; ++t) rgb2yuv(R[t], G[t], B[t], G[t], R[t], B[t], ws);
        noise(G, 0);
        for (size_t t = 0; t < n; ++t) yuv2rgb(G[t], R[t], B[t], R[t], G[t], B[t], ws);
    } else {
        std::vector<float> Y(n);
        for (size_t t = 0; t < n; ++t) { float u, v; rgb2yuv(R[t], G[t], B[t], Y[t], u, v, ws); }
        noise(R, 1); noise(G, 2); noise(B, 3);
        for (size_t t = 0; t < n; ++t) {
            float l, u, v;
            rgb2yuv(R[t], G[t], B[t], l, u, v, ws);
            yuv2rgb(Y[t], u, v, R[t], G[t], B[t], ws);
        }
    }
}

} // namespace

extern "C" {

// the table and the full 64-bit state behind it
void fg_ref_table(int seed, float *normd, uint64_t *state)
{
    Rng rng(seed);
    Normal d;
    for (uint32_t i = 0; i < NORMD; ++i) normd[i] = d(rng);
    *state = rng.seed_;
}

// randint(5233) of draws skip .. skip + n - 1 counted from `state`, stepping serially
void fg_ref_draws(uint64_t state, long long skip, long long n, uint32_t *out)
{
    Rng rng(1);
    rng.seed_ = state;
    for (long long i = 0; i < skip; ++i) rng.seed_ = rng.next();
    for (long long i = 0; i < n; ++i) out[i] = rng.randint(NORMD);
}

// how many of n draws differ between the 64-bit generator and a plain LCG mod 2^48 started from the same state's low 48 bits
long long fg_ref_stream48_mismatches(uint64_t state, long long n)
{
    Rng rng(1);
    rng.seed_ = state;
    uint64_t s48 = state & ((1ULL << 48) - 1);
    long long bad = 0;
    for (long long i = 0; i < n; ++i) {
        const uint32_t a = rng.randint(NORMD);
        s48 = (s48 * 25214903917ULL + 11ULL) & ((1ULL << 48) - 1);
        const uint32_t b = uint32_t(s48 >> 16) % NORMD;
        bad += a != b;
    }
    return bad;
}

int fg_ref_kernel(float radius, float *taps)
{
    std::vector<float> k;
    const int sz = cone(radius, k);
    std::memcpy(taps, k.data(), k.size() * 4);
    return sz;
}

// the direct sum in fp32 (out), in float64 (out64) and sum |k * x| per pixel (absum)
void fg_ref_conv(const float *nb, int W, int H, const float *k, int sz, float *out, double *out64, double *absum)
{
    std::vector<float> src(nb, nb + (size_t)W * H), kk(k, k + sz * sz), o;
    direct_sum(src, W, H, kk, sz, o);
    std::memcpy(out, o.data(), o.size() * 4);
    const int c = sz / 2;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            double acc = 0.0, ab = 0.0;
            for (int i = 0; i < sz; ++i)
                for (int j = 0; j < sz; ++j) {
                    const int yy = std::min(std::max(y + i - c, 0), H - 1), xx = std::min(std::max(x + j - c, 0), W - 1);
                    const double t = (double)k[i * sz + j] * (double)nb[(size_t)yy * W + xx];
                    acc += t; ab += std::fabs(t);
                }
            out64[(size_t)y * W + x] = acc; absum[(size_t)y * W + x] = ab;
        }
}

// filmGrain's regions: out[5 * i ..] = channel, strength, coarseness, seed, sz; sf[i].  Returns their number
int fg_ref_regions(int iso, int strength, int color, int output_pipeline, double scale, int *out, float *sf)
{
    constexpr int iso_min = 20;
    constexpr int iso_max = 6400;
    int coarseness = lim01(float(iso - iso_min + 1) / float(iso_max - iso_min)) * 100.f + 0.5f;
    const int nlevels = output_pipeline ? 3 : int(std::ceil(3 / scale));
    int n = 0;
    const auto add = [&](int chan, int st, int co) {
        std::vector<float> k;
        const float radius = (0.5f + 1.75f * float(co) / 100.f) / scale;
        out[5 * n] = chan; out[5 * n + 1] = st; out[5 * n + 2] = co; out[5 * n + 3] = 42 + chan + co; out[5 * n + 4] = cone(radius, k);
        sf[n] = lim01(float(st) / (chan == 0 ? 200.f : 100.f)) / scale;
        ++n;
    };
    if (color) add(1, strength / 2, coarseness / 2);
    for (int i = 0; i < nlevels; ++i) add(0, strength / (nlevels - i), coarseness / (i + 1));
    return n;
}

// guidedSmoothing over n NOISE regions on three contiguous W x H planes, in place.  regions[3 * i ..] = strength, coarseness, channel;
// masks[i]: a W x H plane or NULL (all ones).  first / last: the normalise passes at either end.  boxes (or NULL): 5 ints per region,
// min_x, min_y, max_x, max_y (exclusive) and whether the region was cropped
void fg_ref_smoothing_noise(float *r, float *g, float *b, int W, int H, const double *ws, double scale, int n, const int *regions, const float *const *masks,
                            int first, int last, int *boxes)
{
    const size_t np = (size_t)W * H;
    float *img[3] = {r, g, b};
    if (first)
        for (float *p : img)
            for (size_t t = 0; t < np; ++t) p[t] *= 1.f / 65535.f;
    for (int i = 0; i < n; ++i) {
        const float *blend = masks ? masks[i] : nullptr;
        int min_x = W - 1, min_y = H - 1, max_x = 0, max_y = 0;
        if (blend) {
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                    if (blend[(size_t)y * W + x] > 0.f) {
                        min_x = std::min(min_x, x); max_x = std::max(max_x, x);
                        min_y = std::min(min_y, y); max_y = std::max(max_y, y);
                    }
        } else { min_x = 0; min_y = 0; max_x = W - 1; max_y = H - 1; }
        ++max_x; ++max_y;
        int ww = max_x - min_x, hh = max_y - min_y;
        int cropped = 1;
        if (!(ww * hh < (W * H) / 2)) { min_x = 0; min_y = 0; max_x = W; max_y = H; ww = W; hh = H; cropped = 0; }
        if (boxes) { boxes[5 * i] = min_x; boxes[5 * i + 1] = min_y; boxes[5 * i + 2] = max_x; boxes[5 * i + 3] = max_y; boxes[5 * i + 4] = cropped; }
        std::vector<float> wk[3];
        for (int c = 0; c < 3; ++c) {
            wk[c].resize((size_t)ww * hh);
            for (int y = min_y; y < max_y; ++y)
                for (int x = min_x; x < max_x; ++x) wk[c][(size_t)(y - min_y) * ww + (x - min_x)] = img[c][(size_t)y * W + x];
        }
        add_noise(wk[0].data(), wk[1].data(), wk[2].data(), ww, hh, ws, regions[3 * i], regions[3 * i + 1], scale, regions[3 * i + 2]);
        for (int c = 0; c < 3; ++c)
            for (int y = min_y; y < max_y; ++y)
                for (int x = min_x; x < max_x; ++x) {
                    const size_t t = (size_t)y * W + x;
                    img[c][t] = intp(blend ? blend[t] : 1.f, wk[c][(size_t)(y - min_y) * ww + (x - min_x)], img[c][t]);
                }
    }
    if (last)
        for (float *p : img)
            for (size_t t = 0; t < np; ++t) p[t] *= 65535.f;
}

} // extern "C"
