// art_amd/csrc/colorcorrection.hip -- ImProcFunctions::colorCorrection on gfx950 (reference: rtengine/ipcolorcorrection.cc:39-866, ART's
// colour-grading tool; color.cc:385-429, 456-473, 511-534 for the double-precision HSL pair, 6691-6742 for yuv2hsl / hsl2yuv and Jzazbz).
//
// The tool is pointwise, so it is ONE pass: a lane reads its pixel's three planes, does setMode(YUV) in registers, applies every region
// of the launch in order (reading the region's abmask / Lmask value), does setMode(RGB) when asked for and writes the three planes:
// 24 B/px and up to 8 B/px per region, however many regions there are.
//
// The reference's SSE2 build runs CDL_v on the columns below 4 * (W / 4) and the scalar CDL on the rest (L808-860); the two differ in bits:
//   * a group of four columns is processed when ANY of its lanes has blend > 0 or lblend > 0 (L818-820), and then every lane gets
//     intp(blend, new, old), lanes with a zero blend included; a tail column with both blends zero is skipped (L844);
//   * pow_F and xlogf are the vector sleef forms in the body and the scalar ones in the tail;
//   * the compression clamps with vmaxf(v, 0) and takes the logarithm of every lane in the body (L683-684), the tail writes 0.f (L473);
//   * vmaxf(Y, 0) against max(Y, 0.f) (L711 / L498), which part for a NaN and for -0.f.
// A lane is one pixel; the four lanes of an aligned quad of a wavefront are one group of the reference (the workgroup's first column is
// a multiple of 256), and the group's "any" is four bits of the wavefront's ballot.  Every step is the reference's arithmetic in the
// reference's order; the one exception is PQ / PQ_inv of an argument above 1 (super-white), the device's powf (see jzazbzdev.h).
#include <hip/hip_runtime.h>
#include "devmath.h"
#include "devsleef.h"
#define LIBMPOWF_OPAQUE        // see libmpowf.h
#include "jzazbzdev.h"
#include "colorcorrection.h"
#include <cmath>
#include <cstring>

namespace artgpu {

namespace {

constexpr float CC_2PI = 2.f * (float)3.14159265358979323846;       // 2.f * RT_PI_F

template <bool VEC> __device__ __forceinline__ float cc_pow(float a, float b) { return VEC ? xexpf_v(b * xlogf_v(a)) : xexpf_s(b * xlogf_s(a)); }
template <bool VEC> __device__ __forceinline__ float cc_max0(float Y) { return VEC ? sse_max(Y, 0.f) : std_max(Y, 0.f); }

// The two matrices and the luminance factors, one copy per lane in vector registers.  As kernel arguments they sit in 21 scalar registers
// for the whole pixel loop, next to the region's scalars and the tables' pointers, and the Jzazbz instantiations spilled scalar registers;
// the kernels use less than half of the vector file.
struct CcLane { float ws[9], iws[9], fR, fG, fB; };
__device__ __forceinline__ float cc_vgpr(float s)
{
    float v;
    asm("v_mov_b32 %0, %1" : "=v"(v) : "s"(s));
    return v;
}
__device__ __forceinline__ CcLane cc_lane(const CcArgs &a)
{
    CcLane k;
#pragma unroll
    for (int i = 0; i < 9; ++i) { k.ws[i] = cc_vgpr(a.ws[i]); k.iws[i] = cc_vgpr(a.iws[i]); }
    k.fR = cc_vgpr(a.fR); k.fG = cc_vgpr(a.fG); k.fB = cc_vgpr(a.fB);
    return k;
}

// Color::yuv2rgb / rgb2yuv (color.h:783-811): the scalar and the vector overloads are the same arithmetic
__device__ __forceinline__ void cc_yuv2rgb(float Y, float u, float v, float &r, float &g, float &b, const float *ws)
{
    b = Y - u;
    r = v + Y;
    g = (Y - r * ws[3] - b * ws[5]) / ws[4];
}
__device__ __forceinline__ float cc_luminance(float r, float g, float b, const float *ws) { return r * ws[3] + g * ws[4] + b * ws[5]; }
__device__ __forceinline__ void cc_rgb2yuv(float r, float g, float b, float &Y, float &u, float &v, const float *ws)
{
    Y = cc_luminance(r, g, b, ws);
    u = Y - b;
    v = r - Y;
}

// get_PQ / get_PQ_inv (color.cc:6708-6730) on the host-built tables.  Below 0 PQ clamps its argument to 1e-10f first: a constant, taken
// from the host like the tables.  Above 1 it is a powf per pixel, recorded in *oor (NaN takes the same call and stays NaN).
struct CcPq {
    const float *tab; float low; bool *oor;
    __device__ __forceinline__ float operator()(float x) const
    {
        if (x >= 0.f && x <= 1.f) return lut_noclip(tab, x * 65535.f);
        if (x < 0.f) return low;
        if (x > 1.f) *oor = true;
        return dev_PQ(x);
    }
};
struct CcPqInv {
    const float *tab; float low; bool *oor;
    __device__ __forceinline__ float operator()(float x) const
    {
        if (x >= 0.f && x <= 1.f) return lut_noclip(tab, x * 65535.f);
        if (x < 0.f) return low;
        if (x > 1.f) *oor = true;
        return dev_PQ_inv(x);
    }
};
// the yuv2jzazbz / jzazbz2yuv lambdas (L143-157): Y <-> Jz, u <-> bz, v <-> az
__device__ __forceinline__ void cc_yuv2jzazbz(const CcArgs &a, const CcLane &k, bool *oor, float &Y, float &u, float &v)
{
    float R, G, B;
    cc_yuv2rgb(Y, u, v, R, G, B, k.ws);
    rgb2jzazbz_dev(CcPq{a.pq, a.pq_low, oor}, R / 65535.f, G / 65535.f, B / 65535.f, Y, v, u, k.ws);
}
__device__ __forceinline__ void cc_jzazbz2yuv(const CcArgs &a, const CcLane &k, bool *oor, float &Jz, float &bz, float &az)
{
    float R, G, B;
    jzazbz2rgb_dev(CcPqInv{a.pq_inv, a.pq_inv_low, oor}, Jz, az, bz, R, G, B, k.iws);
    cc_rgb2yuv(R * 65535.f, G * 65535.f, B * 65535.f, Jz, bz, az, k.ws);
}

// Color::rgb2hsl / hue2rgb / hsl2rgb, the scalar overloads (color.cc:385-429, 456-473, 511-534): double arithmetic
__device__ __forceinline__ double cc_dmin(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double cc_dmax(double a, double b) { return a < b ? b : a; }
__device__ __forceinline__ void cc_rgb2hsl(float r, float g, float b, float &h, float &s, float &l)
{
    const double var_R = double(r) / 65535.0, var_G = double(g) / 65535.0, var_B = double(b) / 65535.0;
    const double m = cc_dmin(cc_dmin(var_R, var_G), var_B);
    const double M = cc_dmax(cc_dmax(var_R, var_G), var_B);
    const double C = M - m;
    const double l_ = (M + m) / 2.;
    l = float(l_);
    if (C < 0.00001 && C > -0.00001) {
        h = 0.f;
        s = 0.f;
    } else {
        double h_;
        if (l_ <= 0.5) s = float((M - m) / (M + m));
        else s = float((M - m) / (2.0 - M - m));
        if (var_R == M) h_ = (var_G - var_B) / C;
        else if (var_G == M) h_ = 2. + (var_B - var_R) / C;
        else h_ = 4. + (var_R - var_G) / C;
        h = float(h_ / 6.0);
        if (h < 0.f) h += 1.f;
        if (h > 1.f) h -= 1.f;
    }
}
__device__ __forceinline__ double cc_hue2rgb(double p, double q, double t)
{
    if (t < 0.) t += 6.;
    else if (t > 6.) t -= 6.;
    if (t < 1.) return p + (q - p) * t;
    else if (t < 3.) return q;
    else if (t < 4.) return p + (q - p) * (4. - t);
    return p;
}
__device__ __forceinline__ void cc_hsl2rgb(float h, float s, float l, float &r, float &g, float &b)
{
    if (s == 0) {
        r = g = b = 65535.0f * l;
    } else {
        const double h_ = double(h), s_ = double(s), l_ = double(l);
        const double m2 = l <= 0.5f ? l_ * (1.0 + s_) : l_ + s_ - l_ * s_;
        const double m1 = 2.0 * l_ - m2;
        r = float(65535.0 * cc_hue2rgb(m1, m2, h_ * 6.0 + 2.0));
        g = float(65535.0 * cc_hue2rgb(m1, m2, h_ * 6.0));
        b = float(65535.0 * cc_hue2rgb(m1, m2, h_ * 6.0 - 2.0));
    }
}

// one channel of the slope / offset / power / pivot / compression chain after v * slope + offset / 2.f: L463-474 (VEC: L675-685)
template <bool VEC>
__device__ __forceinline__ float cc_chain(float v, float power, float pivot, float c0, float c1)
{
    if (VEC) {
        if (pivot != 1.f) v = v > 0.f ? cc_pow<true>(v / pivot, power) * pivot : 0.f;
        else v = v > 0.f ? cc_pow<true>(v, power) : 0.f;
        if (c0 != 0.f) {
            v = sse_max(v, 0.f);
            v = xlogf_v(v * c0 + 1.f) / c1;
        }
    } else {
        if (v > 0.f) {
            if (pivot != 1.f) v = cc_pow<false>(v / pivot, power) * pivot;
            else v = cc_pow<false>(v, power);
            if (c0 != 0.f) v = xlogf_s(v * c0 + 1.f) / c1;
        } else {
            v = 0.f;
        }
    }
    return v;
}

// CDL (L416-554) for VEC = false, one lane of CDL_v (L610-767) for VEC = true
template <bool VEC, int NEED>
__device__ __forceinline__ void cc_cdl(const CcArgs &a, const CcLane &k, const CcRegion &r, bool *oor, float &Y, float &u, float &v)
{
    if (NEED & CC_NEED_HUE) {
        if (r.rhs != 0.f) {
            float h, s;
            if ((NEED & CC_NEED_HSL) && r.hsl) {
                float l, R, G, B;
                cc_yuv2rgb(Y, u, v, R, G, B, k.ws);                 // yuv2hsl (L159-166)
                cc_rgb2hsl(R, G, B, h, s, l);
                h *= CC_2PI;
                h += r.rhs;
                h /= CC_2PI;                                        // hsl2yuv (L168-180)
                if (h < 0.f) h += 1.f;
                else if (h > 1.f) h -= 1.f;
                cc_hsl2rgb(h, s, l, R, G, B);
                cc_rgb2yuv(R, G, B, Y, u, v, k.ws);
            } else {
                if ((NEED & CC_NEED_JZ) && r.jzazbz) cc_yuv2jzazbz(a, k, oor, Y, u, v);
                s = sqrtf(u * u + v * v);                           // Color::yuv2hsl
                h = xatan2f_s(u, v);
                h += r.rhs;
                float sn, cs;
                xsincosf_v(h, sn, cs);                              // Color::hsl2yuv
                u = s * sn;
                v = s * cs;
                if ((NEED & CC_NEED_JZ) && r.jzazbz) cc_jzazbz2yuv(a, k, oor, Y, u, v);
            }
        }
    }
    if (r.rgbmode) {
        if (r.rs != 1.f) { u *= r.rs; v *= r.rs; }
        if (r.enabled) {
            float rgb[3];
            cc_yuv2rgb(Y, u, v, rgb[0], rgb[1], rgb[2], k.ws);
            const bool use_gamma = r.hsl && r.gamma != 1.f;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                float t = rgb[i] / 65535.f;
                if (use_gamma && t > 0.f) t = cc_pow<VEC>(t, r.igamma);
                t = t * r.slope[i] + r.offset[i] / 2.f;
                t = cc_chain<VEC>(t, r.power[i], r.pivot[i], r.comp[i][0], r.comp[i][1]);
                if (use_gamma && t > 0.f) t = cc_pow<VEC>(t, r.gamma);
                rgb[i] = t * 65535.f;
            }
            if (r.rgbmode != 2) {
                cc_rgb2yuv(rgb[0], rgb[1], rgb[2], Y, u, v, k.ws);
            } else {
                float rr, gg, bb;
                cc_yuv2rgb(Y, u, v, rr, gg, bb, k.ws);
                const float Y1 = cc_luminance(rr + (rgb[0] - rr) * k.fR, gg + (rgb[1] - gg) * k.fG, bb + (rgb[2] - bb) * k.fB, k.ws);
                if (Y > 0.f) {
                    const float f = Y1 / Y;
                    u *= f;
                    v *= f;
                }
                Y = Y1;
            }
        }
        const float f = cc_max0<VEC>(Y);
        u += f * r.abcb;
        v += f * r.abca;
        if (r.rsout != 1.f) { u *= r.rsout; v *= r.rsout; }
    } else {
        if (r.enabled) {
            float YY = (Y / 65535.f) * r.slope[0] + r.offset[0] / 2.f;
            if (VEC) {
                YY = cc_chain<true>(YY, r.power[0], r.pivot[0], r.comp[0][0], r.comp[0][1]);
                YY *= 65535.f;
                const float f = Y > 0.f ? YY / Y : 1.f;
                Y = YY;
                u *= f;
                v *= f;
            } else {
                if (YY > 0.f) {
                    YY = cc_chain<false>(YY, r.power[0], r.pivot[0], r.comp[0][0], r.comp[0][1]);
                    YY *= 65535.f;
                } else {
                    YY = 0.f;
                }
                if (Y > 0.f) {
                    const float f = YY / Y;
                    Y = YY;
                    u *= f;
                    v *= f;
                } else {
                    Y = YY;
                }
            }
        }
        if ((NEED & CC_NEED_JZ) && r.jzazbz) cc_yuv2jzazbz(a, k, oor, Y, u, v);
        if (r.rs != 1.f) { u *= r.rs; v *= r.rs; }
        const float f = cc_max0<VEC>(Y);
        u += f * r.abcb;
        v += f * r.abca;
        if (r.rsout != 1.f) { u *= r.rsout; v *= r.rsout; }
        if ((NEED & CC_NEED_JZ) && r.jzazbz) cc_jzazbz2yuv(a, k, oor, Y, u, v);
    }
}

// The whole tool on one launch's regions.  Columns are taken 256 at a time by a workgroup, every lane of it running the same trips (a
// lane past the right edge reads the last column and stores nothing), so that the ballot below sees whole groups.
template <int NEED>
__global__ void __launch_bounds__(256) cc_apply_kernel(CcArgs a)
{
    const CcLane k = cc_lane(a);
    const int wvec = (a.w / 4) * 4;
    const int quad = (int)(threadIdx.x & 63u) & ~3;
    for (int y = blockIdx.y; y < a.h; y += gridDim.y)
        for (int x0 = blockIdx.x * 256; x0 < a.w; x0 += gridDim.x * 256) {
            const int x = x0 + (int)threadIdx.x;
            const bool in = x < a.w;
            const int xc = in ? x : a.w - 1;
            const size_t o = (size_t)y * a.stride + xc;
            float Y, u, v;
            if (a.from_yuv) {
                v = a.img[0][o]; Y = a.img[1][o]; u = a.img[2][o];
            } else {                                                // Imagefloat::setMode(YUV) (imagefloat.cc:700-725)
                const float r = a.img[0][o], g = a.img[1][o], b = a.img[2][o];
                cc_rgb2yuv(r, g, b, Y, u, v, k.ws);
            }
            bool oor = false;
            for (int i = 0; i < a.nregions; ++i) {
                const CcRegion &r = a.r[i];
                const float blend = r.abmask ? r.abmask[(size_t)y * r.ab_stride + xc] : 1.f;
                const float lblend = r.lmask ? r.lmask[(size_t)y * r.l_stride + xc] : 1.f;
                const bool mine = in && (blend > 0.f || lblend > 0.f);
                const unsigned long long group = (__ballot(mine) >> quad) & 0xfull;      // L818-820
                const bool vec = x < wvec;
                if (vec ? group != 0 : mine) {
                    float Yn = Y, un = u, vn = v;
                    if (vec) cc_cdl<true, NEED>(a, k, r, &oor, Yn, un, vn);
                    else cc_cdl<false, NEED>(a, k, r, &oor, Yn, un, vn);
                    Y = intp(lblend, Yn, Y);                        // L827-829 / L851-853: vintpf and intp are the same arithmetic
                    u = intp(blend, un, u);
                    v = intp(blend, vn, v);
                }
            }
            if (!in) continue;
            if (a.to_rgb) {                                         // Imagefloat::setMode(RGB) (imagefloat.cc:779-804)
                float r, g, b;
                cc_yuv2rgb(Y, u, v, r, g, b, k.ws);
                a.img[0][o] = r; a.img[1][o] = g; a.img[2][o] = b;
            } else {
                a.img[0][o] = v; a.img[1][o] = Y; a.img[2][o] = u;
            }
            if ((NEED & CC_NEED_JZ) && a.oor && oor) a.oor[(size_t)y * a.w + x] = 1;
        }
}

__global__ void __launch_bounds__(256) cc_count_kernel(const unsigned char *oor, size_t n, unsigned long long *count)
{
    __shared__ unsigned int lds[256];
    unsigned int c = 0;
    for (size_t k = blockIdx.x * (size_t)256 + threadIdx.x; k < n; k += (size_t)gridDim.x * 256) c += oor[k] != 0;
    const int t = threadIdx.x;
    lds[t] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) lds[t] += lds[t + s];
        __syncthreads();
    }
    if (t == 0 && lds[0]) atomicAdd(count, (unsigned long long)lds[0]);
}

} // namespace

hipError_t launch_cc(const CcArgs &a, int need, hipStream_t s)
{
    if (a.w <= 0 || a.h <= 0 || a.nregions < 0 || a.nregions > CC_MAX_REGIONS) return hipErrorInvalidValue;
    const int gx = (a.w + 255) / 256;
    const dim3 grid(gx > 64 ? 64 : gx, a.h > 32768 ? 32768 : a.h);
    // Four instantiations: plain, + the yuv hue shift, + Jzazbz (tables), + the HSL hue shift (fp64).  Jzazbz and the HSL hue shift never
    // share one: together they spill scalar registers, so the caller cuts the region list between them (cc_need_fits)
    constexpr int HUE = CC_NEED_HUE, JZ = CC_NEED_HUE | CC_NEED_JZ, HSL = CC_NEED_HUE | CC_NEED_HSL;
    const bool jz = need & CC_NEED_JZ, hsl = need & CC_NEED_HSL;
    if ((jz && hsl) || (jz && (!a.pq || !a.pq_inv))) return hipErrorInvalidValue;
    if (jz) hipLaunchKernelGGL(cc_apply_kernel<JZ>, grid, dim3(256), 0, s, a);
    else if (hsl) hipLaunchKernelGGL(cc_apply_kernel<HSL>, grid, dim3(256), 0, s, a);
    else if (need & CC_NEED_HUE) hipLaunchKernelGGL(cc_apply_kernel<HUE>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(cc_apply_kernel<0>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_cc_count(const unsigned char *oor, size_t n, unsigned long long *count, hipStream_t s)
{
    const size_t g = (n + 255) / 256;
    hipLaunchKernelGGL(cc_count_kernel, dim3((unsigned)(g < 1024 ? (g ? g : 1) : 1024)), dim3(256), 0, s, oor, n, count);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// host side: the per-region scalars (L88-141, L280-368, L411-414)
// ---------------------------------------------------------------------------------------------
namespace {

// the scalar sleef forms the derivation calls (rtengine/sleef.h: xlogf, xexpf, xatan2f; xsincosf under SSE2 is lane 0 of the vector form),
// restated for the host from devsleef.h's device forms: the same operations in the same order, unfused
inline float h_i2f(int32_t i) { float f; std::memcpy(&f, &i, 4); return f; }
inline int32_t h_f2i(float f) { int32_t i; std::memcpy(&i, &f, 4); return i; }
inline float h_mla(float x, float y, float z) { return x * y + z; }
inline int h_ilogbp1f(float d)
{
    const bool m = d < 5.421010862427522E-20f;
    d = m ? 1.8446744073709552E19f * d : d;
    const int q = (h_f2i(d) >> 23) & 0xff;
    return m ? q - (64 + 0x7e) : q - 0x7e;
}
inline float h_ldexpkf(float x, int q)
{
    int m = q >> 31;
    m = (((m + q) >> 6) - m) << 4;
    q = q - (m << 2);
    float u = h_i2f((m + 0x7f) << 23);
    u = u * u;
    x = x * u * u;
    u = h_i2f((q + 0x7f) << 23);
    return x * u;
}
inline float h_xlogf(float d)
{
    const int e = h_ilogbp1f(d * 0.7071f);
    const float m = h_ldexpkf(d, -e);
    float x = (m - 1.0f) / (m + 1.0f);
    const float x2 = x * x;
    float t = 0.2371599674224853515625f;
    t = h_mla(t, x2, 0.285279005765914916992188f);
    t = h_mla(t, x2, 0.400005519390106201171875f);
    t = h_mla(t, x2, 0.666666567325592041015625f);
    t = h_mla(t, x2, 2.0f);
    x = x * t + 0.693147180559945286226764f * (float)e;
    if (d == INFINITY) x = INFINITY;
    if (d < 0.f) x = NAN;
    if (d == 0.f) x = -INFINITY;
    return x;
}
inline float h_xexpf(float d)
{
    if (d <= -104.0f) return 0.0f;
    const int q = (int)std::rint(d * ART_R_LN2f);
    float s = h_mla((float)q, -ART_L2Uf, d);
    s = h_mla((float)q, -ART_L2Lf, s);
    float u = 0.00136324646882712841033936f;
    u = h_mla(u, s, 0.00836596917361021041870117f);
    u = h_mla(u, s, 0.0416710823774337768554688f);
    u = h_mla(u, s, 0.166665524244308471679688f);
    u = h_mla(u, s, 0.499999850988388061523438f);
    u = h_mla(s, h_mla(s, u, 1.f), 1.f);
    return h_ldexpkf(u, q);
}
inline float h_xlog2lin(float x, float base) { return (h_xexpf(x * h_xlogf(base)) - 1.f) / (base - 1.f); }
inline float h_mulsign(float x, float y) { return h_i2f(h_f2i(x) ^ (h_f2i(y) & (int32_t)0x80000000)); }
inline float h_atan2kf(float y, float x)
{
    float q = 0.f;
    if (x < 0) { x = -x; q = -2.f; }
    if (y > x) { const float t = x; x = y; y = -t; q += 1.f; }
    const float s = y / x;
    float t = s * s;
    float u = 0.00282363896258175373077393f;
    u = h_mla(u, t, -0.0159569028764963150024414f);
    u = h_mla(u, t, 0.0425049886107444763183594f);
    u = h_mla(u, t, -0.0748900920152664184570312f);
    u = h_mla(u, t, 0.106347933411598205566406f);
    u = h_mla(u, t, -0.142027363181114196777344f);
    u = h_mla(u, t, 0.199926957488059997558594f);
    u = h_mla(u, t, -0.333331018686294555664062f);
    t = u * t;
    t = h_mla(t, s, s);
    return h_mla(q, (float)1.57079632679489661923, t);
}
inline float h_xatan2f(float y, float x)
{
    const float PI_F = (float)3.14159265358979323846;
    float r = h_atan2kf(std::fabs(y), x);
    r = h_mulsign(r, x);
    const float sgx = std::copysign(1.f, x);
    if (std::isinf(x) || x == 0) r = PI_F / 2 - (std::isinf(x) ? (sgx * (float)(PI_F * .5f)) : 0);
    if (std::isinf(y)) r = PI_F / 2 - (std::isinf(x) ? (sgx * (float)(PI_F * .25f)) : 0);
    if (y == 0) r = (sgx == -1 ? PI_F : 0);
    return (x != x) || (y != y) ? NAN : h_mulsign(r, y);
}
inline void h_xsincosf(float d, float &sn, float &cs)
{
    const int q = (int)std::rint(d * (float)0.63661977236758134308);
    float u = (float)q, s = d;
    s = h_mla(u, -0.78515625f * 2, s);
    s = h_mla(u, -0.00024127960205078125f * 2, s);
    s = h_mla(u, -6.3329935073852539062e-07f * 2, s);
    s = h_mla(u, -4.9604681473525147339e-10f * 2, s);
    const float t = s;
    s = s * s;
    u = -0.000195169282960705459117889f;
    u = h_mla(u, s, 0.00833215750753879547119141f);
    u = h_mla(u, s, -0.166666537523269653320312f);
    u = (u * s) * t;
    const float rx = t + u;
    u = -2.71811842367242206819355e-07f;
    u = h_mla(u, s, 2.47990446951007470488548e-05f);
    u = h_mla(u, s, -0.00138888787478208541870117f);
    u = h_mla(u, s, 0.0416666641831398010253906f);
    u = h_mla(u, s, -0.5f);
    const float ry = 1.f + s * u;
    float x = (q & 1) == 0 ? rx : ry, y = (q & 1) == 0 ? ry : rx;
    if ((q & 2) == 2) x = -x;
    if (((q + 1) & 2) == 2) y = -y;
    if (std::isinf(d)) x = y = NAN;
    sn = x; cs = y;
}

inline double h_hue2rgb(double p, double q, double t)
{
    if (t < 0.) t += 6.;
    else if (t > 6.) t -= 6.;
    if (t < 1.) return p + (q - p) * t;
    else if (t < 3.) return q;
    else if (t < 4.) return p + (q - p) * (4. - t);
    return p;
}
inline void h_hsl2rgb(float h, float s, float l, float &r, float &g, float &b)
{
    if (s == 0) {
        r = g = b = 65535.0f * l;
    } else {
        const double h_ = double(h), s_ = double(s), l_ = double(l);
        const double m2 = l <= 0.5f ? l_ * (1.0 + s_) : l_ + s_ - l_ * s_;
        const double m1 = 2.0 * l_ - m2;
        r = float(65535.0 * h_hue2rgb(m1, m2, h_ * 6.0 + 2.0));
        g = float(65535.0 * h_hue2rgb(m1, m2, h_ * 6.0));
        b = float(65535.0 * h_hue2rgb(m1, m2, h_ * 6.0 - 2.0));
    }
}
// hs2uv (L110-128)
void h_hs2uv(float h, float s, float &u, float &v, const float ws[9])
{
    if (h < 0.f) h += 1.f;
    else if (h > 1.f) h -= 1.f;
    float R, G, B;
    h_hsl2rgb(h, s, 0.5f, R, G, B);
    R /= 65535.f;
    G /= 65535.f;
    B /= 65535.f;
    const float Y = R * ws[3] + G * ws[4] + B * ws[5];
    u = Y - B;
    v = R - Y;
    h = h_xatan2f(u, v);                        // Color::yuv2hsl (its s is not used)
    float sn, cs;
    h_xsincosf(h, sn, cs);                      // Color::hsl2yuv
    u = s * sn;
    v = s * cs;
}
inline float h_sgn(float a) { return (float)((0.f < a) - (a < 0.f)); }
inline float h_abcoord(float x) { return h_sgn(x) * h_xlog2lin(std::abs(x), 4.f); }      // L88-92

} // namespace

void cc_derive_region(const CcRegionParams &p, const float ws[9], CcRegion *out)
{
    const float RT_PI_F = (float)3.14159265358979323846, RT_PI_F_180 = (float)0.017453292519943295769;
    CcRegion &r = *out;
    // reset (L257-278)
    r.abca = r.abcb = 0.f; r.rs = r.rsout = 1.f; r.enabled = 0; r.jzazbz = 0; r.hsl = 0; r.rhs = 0.f;
    for (int j = 0; j < 3; ++j) { r.slope[j] = 1.f; r.offset[j] = 0.f; r.power[j] = 1.f; r.pivot[j] = 1.f; r.comp[j][0] = r.comp[j][1] = 0.f; }
    r.gamma = 1.f;
    const bool mode_yuv = p.mode == 0, mode_rgb = p.mode == 1, mode_hsl = p.mode == 2, mode_jz = p.mode == 3;
    r.rgbmode = !mode_yuv && !mode_jz;
    if (r.rgbmode) {
        if (p.rgbluminance) r.rgbmode = 2;
        r.hsl = mode_hsl;
    } else {
        r.jzazbz = mode_jz;
        // abcoord2 (L130-141).  `atan2(y, x)` on two floats: with <math.h> included by the C++ library's wrapper (lcms2.h, glib) the global
        // atan2 is the overload set of std::atan2, so this is the float one
        const float x = h_abcoord((float)p.a), y = h_abcoord((float)p.b);
        float h = std::atan2(y, x) / (2.f * RT_PI_F);
        const float s = std::sqrt(x * x + y * y);
        float u, v;
        h_hs2uv(h, s, u, v, ws);
        r.abca = v;
        r.abcb = u;
    }
    r.rs = 1.f + p.in_saturation / 100.f;
    r.rsout = 1.f + p.out_saturation / 100.f;
    if (mode_hsl) {
        for (int c = 0; c < 3; ++c) {
            const float hue = (float(p.hue[c]) / 180.f) * RT_PI_F;
            const float sat = std::pow(float(p.sat[c]) / 100.f, 2.5f);
            const float f = (p.factor[c] / 100.f) + 1.f;
            float u, v;
            h_hs2uv(hue / (2 * RT_PI_F), sat, u, v, ws);
            float B = 0.5f - u, R = v + 0.5f;                        // Color::yuv2rgb(0.5f, u, v, ...)
            float G = (0.5f - R * ws[3] - B * ws[5]) / ws[4];
            R *= 2.f;
            G *= 2.f;
            B *= 2.f;
            if (c == 0) { r.slope[0] = R * f; r.slope[1] = G * f; r.slope[2] = B * f; }
            else if (c == 1) { r.offset[0] = R + f - 2.f; r.offset[1] = G + f - 2.f; r.offset[2] = B + f - 2.f; }
            else { r.power[0] = (2.f - R) * (2.f - f); r.power[1] = (2.f - G) * (2.f - f); r.power[2] = (2.f - B) * (2.f - f); }
            r.pivot[c] = 1.f;
        }
        for (int c = 0; c < 3; ++c)
            if (r.slope[c] != 1.f || r.offset[c] != 0.f || r.power[c] != 1.f) r.enabled = 1;
        r.gamma = p.hsl_gamma;
    } else {
        for (int c = 0; c < 3; ++c) {
            const int j = r.rgbmode ? c : 0;
            r.slope[c] = p.slope[j];
            r.offset[c] = p.offset[j];
            r.power[c] = 1.0 / p.power[j];
            r.pivot[c] = p.pivot[j];
            const double compr = p.compression[j] * 100.0;
            if (compr > 0) {
                r.comp[c][0] = compr;
                // std::pow on float operands is the float overload; its product with the float pivot is what the double y0 holds
                const double y0 = std::pow((r.slope[c] + r.offset[c]) / r.pivot[c], r.power[c]) * r.pivot[c];
                r.comp[c][1] = std::log(1.0 + y0 * compr) / r.slope[c];
            } else {
                r.comp[c][0] = r.comp[c][1] = 0;
            }
            if (r.slope[c] != 1.f || r.offset[c] != 0.f || r.power[c] != 1.f || r.comp[c][1] != 0.f) r.enabled = 1;
        }
    }
    r.rhs = mode_rgb ? 0.f : (float)(p.hueshift * RT_PI_F_180);
    r.igamma = 1.f / r.gamma;
}

bool cc_region_finite(const CcRegion &r)
{
    bool ok = std::isfinite(r.abca) && std::isfinite(r.abcb) && std::isfinite(r.rs) && std::isfinite(r.rsout) && std::isfinite(r.rhs) &&
              std::isfinite(r.gamma) && std::isfinite(r.igamma);
    for (int j = 0; j < 3; ++j)
        ok = ok && std::isfinite(r.slope[j]) && std::isfinite(r.offset[j]) && std::isfinite(r.power[j]) && std::isfinite(r.pivot[j]) &&
             std::isfinite(r.comp[j][0]) && std::isfinite(r.comp[j][1]);
    return ok;
}

void cc_luminance_factors(const float ws[9], float *fR, float *fG, float *fB)
{
    const float m01 = ws[3] < ws[4] ? ws[4] : ws[3];           // max(a, b, c) = max(max(a, b), c) (rt_math.h:72-82)
    const float max_ws = m01 < ws[5] ? ws[5] : m01;
    *fR = max_ws / ws[3];
    *fG = max_ws / ws[4];
    *fB = max_ws / ws[5];
}

void cc_pq_low(float *pq_low, float *pq_inv_low)
{
    volatile float Xv = 1e-10f;                 // (evaluated by the C library at run time like the tables' entries, not folded by the compiler)
    const float X = Xv;
    const float XX = std::pow(X * 1e-4f, 0.1593017578125f);
    *pq_low = std::pow((0.8359375f + 18.8515625f * XX) / (1 + 18.6875f * XX), 134.034375f);
    const float YY = std::pow(X, 7.460772656268214e-03f);
    *pq_inv_low = 1e4f * std::pow((0.8359375f - YY) / (18.6875f * YY - 18.8515625f), 6.277394636015326f);
}

} // namespace artgpu
