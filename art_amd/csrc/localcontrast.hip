// art_amd/csrc/localcontrast.hip -- ImProcFunctions::localContrast on gfx950: what local_contrast_wavelets does between its
// wavelet_decomposition and its reconstruct (rtengine/iplocalcontrast.cc:251-420), and the mask blend (L474-480).
//
//   statistics   eval_avg / eval_sigma of every detail band (L97-189) and the sum / min / max of coeff0 (L287-313).  Every sum is a
//                double, as in the reference, taken in an order that depends on the band size alone:
//                  chunk c of a segment = its coefficients [c * LC_CHUNK, (c + 1) * LC_CHUNK);
//                  thread t of the workgroup that owns the chunk adds coefficients c * LC_CHUNK + t + 256 k, k = 0 .. 15, in that order;
//                  the 64 lanes of a wave are folded at distances 32, 16, 8, 4, 2, 1, the four waves added in wave order;
//                  the chunk's partial goes to memory with an ordinary store, and one workgroup combines a segment's partials the
//                  same way (thread t adds partials t + 256 k in ascending k, then the same fold).
//                Which workgroup owns a chunk changes nothing, there is no atomic: the same band gives the same bits on every run and
//                for every grid.  averagePlus = (float)(sum / count) is finished on the device (IEEE double division, narrowing), so
//                the variance pass follows without the host.
//   remaps       the contrast remap of coeff0 (L328-345) and the curve remap of the bands (L386-414), one launch for all segments;
//                the 501-entry curve sits in LDS, the per-level constants (host libm, L372-380) arrive as kernel arguments.
//   blend        rgb->g = intp(mask, L_new, l) (L474-480); without a mask the same arithmetic with 1.f.
// Traffic per region: every band is read three times (average, variance, remap) and written once, coeff0 read twice and written once.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include "devmath.h"
#include "devsleef.h"
#include "kernels.h"

namespace artgpu {

namespace {

constexpr int LC_T = 256;                       // threads per workgroup
constexpr int LC_PER = LC_CHUNK / LC_T;         // coefficients per thread and chunk
static_assert(LC_CHUNK % LC_T == 0, "a chunk is a whole number of workgroup rows");

struct LcAcc { double s; int cnt; float mx, mn; };

__device__ __forceinline__ LcAcc lc_fold(LcAcc a, const LcAcc &b)
{
    a.s += b.s; a.cnt += b.cnt;
    a.mx = a.mx < b.mx ? b.mx : a.mx;
    a.mn = b.mn < a.mn ? b.mn : a.mn;
    return a;
}
// lanes at distances 32 .. 1, then the four waves in order: thread 0 returns the workgroup's value
__device__ __forceinline__ LcAcc lc_block_reduce(LcAcc v, LcAcc *sh)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        LcAcc w;
        w.s = __shfl_down(v.s, o); w.cnt = __shfl_down(v.cnt, o); w.mx = __shfl_down(v.mx, o); w.mn = __shfl_down(v.mn, o);
        v = lc_fold(v, w);
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();                            // sh may still be read by thread 0 from the previous use
    if ((threadIdx.x & 63) == 0) sh[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) { v = sh[0]; for (int k = 1; k < LC_T / 64; ++k) v = lc_fold(v, sh[k]); }
    return v;
}

// partials of one pass.  SIGMA == false: sums, counts, maxima (and coeff0's minimum); true: the variance sums around res[seg].avg
template <bool SIGMA>
__global__ void __launch_bounds__(LC_T) lc_partials_kernel(LcStatArgs a)
{
    __shared__ LcAcc sh[LC_T / 64];
    const int seg = blockIdx.y;
    const bool c0 = seg == a.nbands;
    const float *x = c0 ? a.coeff0 : a.bands + (size_t)seg * a.n;
    const float avg = SIGMA ? a.res[seg].avg : 0.f;
    for (int ch = blockIdx.x; ch < a.nchunk; ch += gridDim.x) {
        const size_t base = (size_t)ch * LC_CHUNK + threadIdx.x;
        float v[LC_PER];
#pragma unroll
        for (int k = 0; k < LC_PER; ++k) {
            const size_t i = base + (size_t)k * LC_T;
            v[k] = i < a.n ? x[i] : 0.f;
        }
        LcAcc acc = {0.0, 0, 0.f, FLT_MAX};
        if (c0) {
#pragma unroll
            for (int k = 0; k < LC_PER; ++k) {
                if (base + (size_t)k * LC_T < a.n) {
                    acc.s += v[k];                                   // avedbl += wl0[i]
                    acc.mn = v[k] < acc.mn ? v[k] : acc.mn;          // min(lminL, wl0[i])
                    acc.mx = acc.mx < v[k] ? v[k] : acc.mx;          // max(lmaxL, wl0[i])
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < LC_PER; ++k) {
                if (v[k] >= 5.f) {                                   // thres; the 0 of a lane past the end never counts
                    if (SIGMA) {
                        acc.s += sqr(v[k] - avg);                    // the float SQR, widened
                    } else {
                        acc.s += v[k];
                        if (v[k] > acc.mx) acc.mx = v[k];
                    }
                    ++acc.cnt;
                }
            }
        }
        acc = lc_block_reduce(acc, sh);
        if (threadIdx.x == 0) {
            const size_t p = (size_t)seg * a.nchunk + ch;
            a.psum[p] = acc.s;
            if (!SIGMA) { a.pcnt[p] = acc.cnt; a.pmax[p] = acc.mx; a.pmin[p] = acc.mn; }
        }
    }
}

// one workgroup: the partials of every segment in index order
template <bool SIGMA>
__global__ void __launch_bounds__(LC_T) lc_combine_kernel(LcStatArgs a, int nseg)
{
    __shared__ LcAcc sh[LC_T / 64];
    for (int seg = 0; seg < nseg; ++seg) {
        LcAcc acc = {0.0, 0, 0.f, FLT_MAX};
        for (int p = threadIdx.x; p < a.nchunk; p += LC_T) {
            const size_t q = (size_t)seg * a.nchunk + p;
            LcAcc b = {a.psum[q], 0, 0.f, FLT_MAX};
            if (!SIGMA) { b.cnt = a.pcnt[q]; b.mx = a.pmax[q]; b.mn = a.pmin[q]; }
            acc = lc_fold(acc, b);
        }
        acc = lc_block_reduce(acc, sh);
        if (threadIdx.x == 0) {
            LcSegStats &r = a.res[seg];
            if (SIGMA) {
                r.vari = acc.s;
            } else {
                r.sum = acc.s; r.vari = 0.0; r.cnt = acc.cnt; r.maxv = acc.mx; r.minv = acc.mn;
                r.avg = acc.cnt > 0 ? (float)(acc.s / acc.cnt) : 0.f;          // averagePlus = averaP / countP (L145-149)
            }
        }
    }
}

__global__ void __launch_bounds__(LC_T) lc_remap_kernel(LcRemapArgs a)
{
    __shared__ float curve[501];
    const int seg = blockIdx.y;
    const size_t step = (size_t)gridDim.x * LC_T;
    if (seg == 3 * a.nlevels) {
        // contrast remap of coeff0 (L328-345)
        if (!a.c0_on) return;
        const float ave = a.ave, ah = a.ah, bh = a.bh, al = a.al, bl = a.bl;
        for (size_t i = (size_t)blockIdx.x * LC_T + threadIdx.x; i < a.n; i += step) {
            float w = a.coeff0[i];
            if (w < 32768.f) {
                float prov;
                if (w > ave) {
                    const float kh = ah * (w / 327.68f) + bh;
                    prov = w;
                    w = ave + kh * (w - ave);
                } else {
                    const float kl = al * (w / 327.68f) + bl;
                    prov = w;
                    w = ave - kl * (ave - w);
                }
                const float diflc = w - prov;       // both roundings of the reference are kept
                a.coeff0[i] = prov + diflc;
            }
        }
        return;
    }
    const LcLevelConst c = a.lv[seg / 3];
    if (!c.on) return;                              // MaxP > 0 && mean != 0 && sigma != 0 (L371)
    const bool has_curve = a.curve != nullptr;
    if (has_curve) {
        for (int i = threadIdx.x; i < 501; i += LC_T) curve[i] = a.curve[i];
        __syncthreads();
    }
    float *x = a.bands + (size_t)seg * a.n;
    for (size_t i = (size_t)blockIdx.x * LC_T + threadIdx.x; i < a.n; i += step) {
        const float val = x[i];
        if (val != val) continue;                   // std::isnan(val): left alone (L390-394)
        const float av = fabsf(val);
        float absciss;
        if (av >= c.thr) {                          // for max
            const float valcour = xlogf_s(av);
            const float valc = valcour - c.logmax;
            const float vald = valc * c.rap;
            absciss = xexpf_s(vald);
        } else if (av >= c.mean) {
            absciss = c.asig * av + c.bsig;
        } else {
            absciss = c.amean * av;
        }
        const float kc = (has_curve ? lutf_lookup<true>(curve, 501, absciss * 500.f) : 0.f) - 0.5f;
        const float reduceeffect = kc <= 0.f ? 1.f : 1.5f;
        float kinterm = 1.f + reduceeffect * kc;
        kinterm = kinterm <= 0.f ? 0.01f : kinterm;
        x[i] = val * kinterm;
    }
}

__global__ void __launch_bounds__(256) lc_blend_kernel(LcBlendArgs a)
{
    FOR_IMAGE_XY(y, x, a.w, a.h) {
        const size_t o = (size_t)y * a.l_stride + x;
        const float m = a.mask ? a.mask[(size_t)y * a.m_stride + x] : 1.f;
        a.L[o] = intp(m, a.Lnew[(size_t)y * a.w + x], a.L[o]);
    }
}

int lc_grid_x(long long items, long long per_block)
{
    const long long g = (items + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

} // namespace

hipError_t launch_lc_stats(const LcStatArgs &a, hipStream_t s)
{
    const int nseg = a.nbands + (a.coeff0 ? 1 : 0);
    const int gx = lc_grid_x(a.nchunk, 1);
    hipLaunchKernelGGL(lc_partials_kernel<false>, dim3(gx, nseg), dim3(LC_T), 0, s, a);
    hipLaunchKernelGGL(lc_combine_kernel<false>, dim3(1), dim3(LC_T), 0, s, a, nseg);
    hipLaunchKernelGGL(lc_partials_kernel<true>, dim3(gx, a.nbands), dim3(LC_T), 0, s, a);
    hipLaunchKernelGGL(lc_combine_kernel<true>, dim3(1), dim3(LC_T), 0, s, a, a.nbands);
    return hipGetLastError();
}

hipError_t launch_lc_remap(const LcRemapArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(lc_remap_kernel, dim3(lc_grid_x((long long)a.n, 4 * LC_T), 3 * a.nlevels + 1), dim3(LC_T), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_lc_blend(const LcBlendArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(lc_blend_kernel, image_grid(a.w, a.h), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- host side ----

// wavelet_level = 7, lowered while (1 << wavelet_level) >= min(W, H) and > 1 (L256-260)
int lc_wavelet_levels(int w, int h)
{
    int level = 7;
    const int dim = w < h ? w : h;
    while ((1 << level) >= dim && level > 1) --level;
    return level;
}

// WavOpacityCurveWL::Set(const std::vector<double>&) (L85-94 -> L71-83): false = the LUT stays unset
bool lc_curve_lut(const double *pts, int npts, float lut[501])
{
    for (int i = 0; i < 501; ++i) lut[i] = 0.f;
    if (!(npts > 0 && pts[0] > 0. && pts[0] < 2.)) return false;     // FCT_Linear < kind < FCT_Unchanged
    double v[501];
    if (flat_curve_sample(pts, npts, false, 1000 / 2, 0., 501, v)) return false;   // pCurve.isIdentity()
    for (int i = 0; i < 501; ++i) lut[i] = (float)v[i];
    return true;
}

// log(MaxP[level]), log(insigma), log(rapX) (L373-376) take a float and are assigned to a float.  Which overload they reach depends
// on the headers in front of them: rtengine's own chain from iplocalcontrast.cc reaches <cmath> only, which declares the float
// overload in namespace std and leaves ::log(double) the one candidate of the unqualified call inside namespace rtengine -- the
// argument is widened, the double result narrowed.  (Only a system header that includes <math.h> itself would add `using std::log`
// to the global namespace and make it logf; lcms2.h includes stdio.h, limits.h, time.h and stddef.h.)  tests/emul/local_contrast_ref.cc
// states the same conclusion and makes the same call.
static float lc_log(float x) { return (float)std::log((double)x); }

void lc_host_constants(const LcSegStats *res, int nlevels, size_t n, double contrast_d, LcRemapArgs *ra, LcHostInfo *info)
{
    *info = LcHostInfo{};
    const float contrast = (float)contrast_d;                       // const float contrast = params.contrast (L268)
    ra->c0_on = 0;
    if (contrast != 0) {
        const LcSegStats &c = res[3 * nlevels];
        const float maxh = 2.5f, maxl = 2.5f;
        const float multL = contrast * (maxl - 1.f) / 100.f + 1.f;
        const float multH = contrast * (maxh - 1.f) / 100.f + 1.f;
        float max0 = c.maxv, min0 = c.minv;
        info->max0 = max0; info->min0 = min0;
        max0 /= 327.68f;
        min0 /= 327.68f;
        const float ave = (float)(c.sum / double((int)n));          // W_L * H_L is an int
        const float av = ave / 327.68f;
        const float ah = (multH - 1.f) / (av - max0);
        const float bh = 1.f - max0 * ah;
        const float al = (multL - 1.f) / (av - min0);
        const float bl = 1.f - min0 * al;
        info->ave = ave;
        ra->c0_on = max0 > 0.0 ? 1 : 0;
        ra->ave = ave; ra->ah = ah; ra->bh = bh; ra->al = al; ra->bl = bl;
    }
    for (int level = 0; level < nlevels; ++level) {
        // eval_level (L199-231): the three directions in order, then / 3
        float AvL = 0.f, SL = 0.f, maxLP = 0.f;
        for (int dir = 1; dir < 4; ++dir) {
            const LcSegStats &b = res[3 * level + dir - 1];
            const float sigP = b.cnt > 0 ? (float)std::sqrt(b.vari / b.cnt) : 0.f;   // sigmaPlus = sqrt(variP / countP) (L178-182)
            AvL += b.avg;
            SL += sigP;
            maxLP += b.maxv;
        }
        AvL /= 3;
        SL /= 3;
        maxLP /= 3;
        info->mean[level] = AvL; info->sigma[level] = SL; info->maxp[level] = maxLP;
        LcLevelConst &c = ra->lv[level];
        c = LcLevelConst{};
        if (maxLP > 0.f && AvL != 0.f && SL != 0.f) {               // L371-380
            const float insigma = 0.666f;
            const float logmax = lc_log(maxLP);
            const float rapX = (AvL + SL) / maxLP;
            const float inx = lc_log(insigma);
            const float iny = lc_log(rapX);
            c.on = 1;
            c.mean = AvL;
            c.thr = AvL + SL;
            c.logmax = logmax;
            c.rap = inx / iny;
            c.asig = 0.166f / SL;
            c.bsig = 0.5f - c.asig * AvL;
            c.amean = 0.5f / AvL;
        }
    }
}

} // namespace artgpu
