// tests/emul/resize_ref.cc -- CPU checker for artgpu_resize_lanczos / artgpu_resize_scale: ImProcFunctions::Lanczos (rtengine/ipresize.cc:53-223)
// restated serially, row by row with the reference's three line buffers, and ImProcFunctions::resizeScale (L226-297) without its crop
// branches.  Test infrastructure only; built on first use with -ffp-contract=off.
//
// The leaves: xsinf in its scalar form (sleef.h:993-1016, xrintf = cvtss2si under SSE2), restated from the header's arithmetic and pinned
// by tests/golden/lanczos.npz (recorded from the reference's own header); Imagefloat's mode switches are liboracle's.  The 4-wide body of the
// vertical pass (L159-175) is the scalar tail's arithmetic (L181-195) under -ffp-contract=off: one loop stands for both.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include <xmmintrin.h>

extern "C" {
void oracle_image_rgb_to_lab(float *const img[3], int W, int H, const double ws[9]);
void oracle_image_lab_to_rgb(float *const img[3], int W, int H, const double iws[9]);

struct rs_ref_params {             // the layout of artgpu_resize_params
    int32_t enabled, dataspec;
    double scale;
    int32_t width, height, allow_upscaling;
};
struct rs_ref_counts {
    long long clip_left, clip_right, clip_top, clip_bottom;   // destination columns / rows whose tap range max(0, .) / min(len, .) cut
    long long empty_cols, empty_rows;                         // ... and those without a tap
    long long lanc_one, lanc_zero, lanc_sinc;                 // Lanc's three branches
};
}

namespace {

rs_ref_counts *g_cn = nullptr;
std::vector<float> *g_args = nullptr;      // every argument xsinf is called with, in call order

inline int xrintf(float x) { return _mm_cvt_ss2si(_mm_set_ss(x)); }
inline float mlaf(float x, float y, float z) { return x * y + z; }

float xsinf(float d)
{
    if (g_args) g_args->push_back(d);
    int q = xrintf(d * 0.318309886183790671538f);
    d = mlaf(q, -0.78515625f * 4, d);
    d = mlaf(q, -0.00024127960205078125f * 4, d);
    d = mlaf(q, -6.3329935073852539062e-07f * 4, d);
    d = mlaf(q, -4.9604681473525147339e-10f * 4, d);
    float s = d * d;
    if ((q & 1) != 0) d = -d;
    float u = 2.6083159809786593541503e-06f;
    u = mlaf(u, s, -0.0001981069071916863322258f);
    u = mlaf(u, s, 0.00833307858556509017944336f);
    u = mlaf(u, s, -0.166666597127914428710938f);
    u = mlaf(s, u * d, d);
    return u;
}

float Lanc(float x, float a)
{
    if (x * x < 1e-6f) {
        if (g_cn) g_cn->lanc_one++;
        return 1.0f;
    } else if (x * x > a * a) {
        if (g_cn) g_cn->lanc_zero++;
        return 0.0f;
    } else {
        if (g_cn) g_cn->lanc_sinc++;
        x = static_cast<float>(3.14159265358979323846) * x;
        return a * xsinf(x) * xsinf(x / a) / (x * x);
    }
}

int support_of(float scale)
{
    const float sc = std::min(scale, 1.0f);
    return static_cast<int>(2.0f * 3.0f / sc) + 1;
}

// one destination position's taps and normalised weights (L86-108 / L133-152); w: `support` floats that keep what earlier positions left
// behind the taps, as the reference's buffers do
void taps(int j, int len, float scale, int support, float *w, int *first, int *last, long long *clip_lo, long long *clip_hi, long long *empty)
{
    const float delta = 1.0f / scale;
    const float a = 3.0f;
    const float sc = std::min(scale, 1.0f);
    float x0 = (static_cast<float>(j) + 0.5f) * delta - 0.5f;
    float ws = 0.0f;
    const int lo = static_cast<int>(floorf(x0 - a / sc)) + 1, hi = static_cast<int>(floorf(x0 + a / sc)) + 1;
    *first = std::max(0, lo);
    *last = std::min(len, hi);
    if (clip_lo && lo < 0) ++*clip_lo;
    if (clip_hi && hi > len) ++*clip_hi;
    if (empty && *first >= *last) ++*empty;
    for (int jj = *first; jj < *last; jj++) {
        int k = jj - *first;
        float z = sc * (x0 - static_cast<float>(jj));
        w[k] = Lanc(z, a);
        ws += w[k];
    }
    for (int k = 0; k < support; k++) w[k] /= ws;
}

void lanczos(float *const src[3], int sW, int sH, float *const dst[3], int dW, int dH, float scale, rs_ref_counts *cn)
{
    g_cn = cn;
    const int support = support_of(scale);
    std::vector<float> wwh((size_t)support * dW, 0.f);
    std::vector<int> jj0(dW), jj1(dW);
    const float *sL = src[1], *sa = src[0], *sb = src[2];          // L = g, a = r, b = b
    float *dL = dst[1], *da = dst[0], *db = dst[2];
    for (int j = 0; j < dW; j++)
        taps(j, sW, scale, support, wwh.data() + (size_t)j * support, &jj0[j], &jj1[j], cn ? &cn->clip_left : nullptr, cn ? &cn->clip_right : nullptr,
             cn ? &cn->empty_cols : nullptr);
    std::vector<float> lL(sW), la(sW), lb(sW), w(support, 0.f);
    for (int i = 0; i < dH; i++) {
        int ii0, ii1;
        taps(i, sH, scale, support, w.data(), &ii0, &ii1, cn ? &cn->clip_top : nullptr, cn ? &cn->clip_bottom : nullptr, cn ? &cn->empty_rows : nullptr);
        for (int j = 0; j < sW; j++) {
            float L = 0.0f, a = 0.0f, b = 0.0f;
            for (int ii = ii0; ii < ii1; ii++) {
                int k = ii - ii0;
                L += w[k] * sL[(size_t)ii * sW + j];
                a += w[k] * sa[(size_t)ii * sW + j];
                b += w[k] * sb[(size_t)ii * sW + j];
            }
            lL[j] = L; la[j] = a; lb[j] = b;
        }
        for (int j = 0; j < dW; j++) {
            const float *wh = wwh.data() + (size_t)support * j;
            float L = 0.0f, a = 0.0f, b = 0.0f;
            for (int jj = jj0[j]; jj < jj1[j]; jj++) {
                int k = jj - jj0[j];
                L += wh[k] * lL[jj];
                a += wh[k] * la[jj];
                b += wh[k] * lb[jj];
            }
            dL[(size_t)i * dW + j] = L; da[(size_t)i * dW + j] = a; db[(size_t)i * dW + j] = b;
        }
    }
    g_cn = nullptr;
}

} // namespace

extern "C" {

int rs_ref_sizes(int which) { return which == 0 ? (int)sizeof(rs_ref_params) : (int)sizeof(rs_ref_counts); }

void rs_ref_xsinf(const float *x, float *y, size_t n) { for (size_t i = 0; i < n; ++i) y[i] = xsinf(x[i]); }

int rs_ref_support(float scale) { return support_of(scale); }

// the normalised weight rows of n destination positions over len source positions (entries behind a row's taps: 0), their tap ranges, and --
// args != NULL -- the first nargs arguments xsinf was called with; returns how many there were
long long rs_ref_weights(int n, int len, float scale, float *w, int *first, int *last, float *args, long long nargs)
{
    const int support = support_of(scale);
    std::vector<float> seen, row(support, 0.f);
    g_args = &seen;
    for (int j = 0; j < n; ++j) {
        taps(j, len, scale, support, row.data(), &first[j], &last[j], nullptr, nullptr, nullptr);
        for (int k = 0; k < support; ++k) w[(size_t)j * support + k] = k < last[j] - first[j] ? row[k] : 0.f;
    }
    g_args = nullptr;
    for (long long i = 0; args && i < nargs && i < (long long)seen.size(); ++i) args[i] = seen[i];
    return (long long)seen.size();
}

// mode 0: the three planes as they are; 1: setMode(LAB) on a copy of src, the resampler, setMode(RGB) on dst.  Planes are dense
int rs_ref_lanczos(const float *sr, const float *sg, const float *sb, int sW, int sH, float *dr, float *dg, float *db, int dW, int dH, float scale, int mode,
                   const double *ws, const double *iws, rs_ref_counts *cn)
{
    if (sW < 1 || sH < 1 || dW < 1 || dH < 1 || !(scale > 0.f) || !std::isfinite(scale)) return 1;
    const size_t n = (size_t)sW * sH;
    std::vector<float> copy(3 * n);
    std::memcpy(copy.data(), sr, n * 4); std::memcpy(copy.data() + n, sg, n * 4); std::memcpy(copy.data() + 2 * n, sb, n * 4);
    float *src[3] = {copy.data(), copy.data() + n, copy.data() + 2 * n}, *dst[3] = {dr, dg, db};
    if (mode == 1) oracle_image_rgb_to_lab(src, sW, sH, ws);
    if (cn) std::memset(cn, 0, sizeof *cn);
    lanczos(src, sW, sH, dst, dW, dH, scale, cn);
    if (mode == 1) oracle_image_lab_to_rgb(dst, dW, dH, iws);
    return 0;
}

// ImProcFunctions::resizeScale without a crop: the factor in double from the data spec, the 1e-5 rule, the rounded size
float rs_ref_scale(const rs_ref_params *params, int fw, int fh, int *imw, int *imh)
{
    *imw = fw; *imh = fh;
    if (!params || !params->enabled) return 1.0f;
    const double by_width = (double)params->width / (double)fw, by_height = (double)params->height / (double)fh;
    double f;
    if (params->dataspec == 1) f = by_width;
    else if (params->dataspec == 2) f = by_height;
    else if (params->dataspec == 3) {
        // the box: the side that binds is the one the frame's aspect ratio exceeds the box's on
        f = (double)fw / (double)fh > (double)params->width / (double)params->height ? by_width : by_height;
        if (f > 1.0 && !params->allow_upscaling) f = 1.0;
    } else f = params->scale;
    if (fabs(f - 1.0) <= 1e-5) return 1.0f;
    *imw = (int)((double)fw * f + 0.5);
    *imh = (int)((double)fh * f + 0.5);
    return (float)f;
}

} // extern "C"
