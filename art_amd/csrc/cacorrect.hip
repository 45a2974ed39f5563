// art_amd/csrc/cacorrect.hip -- raw CA correction on the CFA (RawImageSource::CA_correct_RT, rtengine/CA_correct_RT.cc:122-1384),
// one frame, Bayer only.  Kernels of one iteration, enqueued by artgpu_raw_ca_correct without a synchronisation:
//   ca_pass1_kernel  workgroup per 128x128 tile (step 112): normalise, directional G at R/B sites (-> Gtmp), the high / low pass
//                    filters and the six coefficient sums -> CAshift, blockwt, blockshifts (L303-686)
//   ca_fit_kernel    one workgroup: block sums in tile raster order, blockvar, border blocks, 3x3 medians, rejection, polymat /
//                    shiftmat in double, numblox rules, LinEqSolve -> fitparams, processpasstwo (L693-837)
//   ca_pass2_kernel  workgroup per tile: shifted G, interpolated colour difference, overshoot rule -> RawDataTmp (L846-1250)
//   ca_copyback_kernel, and the colour-shift guard: ca_factors / ca_factor_fill / (gaussian, sigma 30) / ca_apply (L1276-1352)
// The device words (run, processpasstwo, polyord) carry the reference's control flow between launches: a stage whose word says
// the iteration does not run returns at once.
//
// LDS plan (gfx950: 160 KB per CU).  The reference's tile buffer is 320 KB in pass 1 (rgb[0..2] + six filter planes) and 192 KB in
// pass 2 (rgb[0..2] + grbdiff + gshift).  Only rgb[0] / rgb[1] / rgb[2] live on chip, at the reference's offsets in its buffer,
// the 64-byte pads between them included (128.1 KB, zeroed per tile like the reference's memset); the filter planes (pass 1) and
// grbdiff / gshift (pass 2) are recomputed at every use from those, with the reference's expressions, which gives the stored values'
// bits.  The layout is part of the semantics: the pass-1 border fills of frames with H % 112 or W % 112 in 1..7 write past a plane
// (a row wraps into the next one, a plane's last rows into the pad and the next plane), and manual shifts of more than a few pixels
// make pass 2 read G above / below its plane, in rgb[0] / rgb[2] -- both deterministic in the reference, both restated here.
#include "kernels.h"

namespace artgpu {
namespace {

constexpr int TS = 128, TSH = 64, BORDER = 8, BORDER2 = 16, CB = 2;
constexpr int CA_NT = 256;
constexpr int CA_LANE_FLOATS = 112 * 6 * 4, CA_TAIL_FLOATS = 112 * 3 * 6;
// float offsets of rgb[0] / rgb[1] / rgb[2] in the reference's buffer (CA_correct_RT.cc:270-272: 64-byte pads) and its planes' end
constexpr int RGB0 = 0, RGB1 = TS * TSH + 16, RGB2 = TS * TS + TS * TSH + 32, CA_PLANES = RGB2 + TS * TSH;
constexpr int CA_PLANES_BYTES = CA_PLANES * 4;
// manual shifts are held at +-MAX_MANUAL_SHIFT px: up to there every G read of pass 2 stays inside rgb[0] .. rgb[2]
constexpr float MAX_MANUAL_SHIFT = 60.f;
// pass-2 G reads: sites 6..121 of the tile (rows and columns) moved by at most 60
static_assert(RGB1 + (6 - 60) * TS + 6 - 60 >= 0 && RGB1 + (121 + 60) * TS + 121 + 60 < CA_PLANES, "pass-2 G reads stay in the planes");
constexpr int CA_PASS1_LDS = CA_PLANES_BYTES + (CA_LANE_FLOATS + CA_TAIL_FLOATS) * 4 + 112 * 4;
constexpr int CA_PASS2_LDS = CA_PLANES_BYTES;
static_assert(CA_PASS1_LDS <= 160 * 1024, "pass-1 LDS");
constexpr float EPS = 1e-5f, EPS2 = 1e-10f;

struct Tile {
    int top, left, vblock, hblock, rr1, cc1, rrmin, rrmax, ccmin, ccmax;
};
__device__ __forceinline__ Tile tile_box(const CaArgs &a, int tv, int th)
{
    Tile t;
    t.top = -BORDER + tv * (TS - BORDER2);
    t.left = -BORDER + th * (TS - BORDER2);
    t.vblock = tv + 1;
    t.hblock = th + 1;
    const int wlim = a.width - (a.W & 1);
    const int bottom = min(t.top + TS, a.H + BORDER);
    const int right = min(t.left + TS, wlim + BORDER);
    t.rr1 = bottom - t.top;
    t.cc1 = right - t.left;
    t.rrmin = t.top < 0 ? BORDER : 0;
    t.rrmax = bottom > a.H ? a.H - t.top : t.rr1;
    t.ccmin = t.left < 0 ? BORDER : 0;
    t.ccmax = right > wlim ? wlim - t.left : t.cc1;
    return t;
}
__device__ __forceinline__ int fc(const CaArgs &a, int r, int c) { return (a.cfa >> (((r & 1) * 2 + (c & 1)) * 2)) & 3; }
__device__ __forceinline__ float SQR(float x) { return x * x; }
__device__ __forceinline__ float intp(float a, float b, float c) { return a * b + (1.f - a) * c; }
__device__ __forceinline__ float fmin_(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float fmax_(float a, float b) { return a < b ? b : a; }
__device__ __forceinline__ float RAW(const CaArgs &a, int r, int c) { return a.raw[(size_t)r * a.stride + c]; }

// the tile's rgb[0] / rgb[1] / rgb[2] in LDS at the reference's offsets (an offset by arithmetic, not an indexed array of
// pointers in scratch).  put() indexes like the reference, past the end of a row or a plane included; a write beyond rgb[2]
// (the pass-1 bottom fill of rgb[2] for H % 112 in 1..7) lands in the reference's rbhpfh plane at entries the filter loop writes
// again before anything reads them, and is dropped here.
struct Planes {
    float *base;
    __device__ __forceinline__ int off(int c) const { return c == 0 ? RGB0 : c == 1 ? RGB1 : RGB2; }
    __device__ __forceinline__ float *pl(int c) const { return base + off(c); }
    __device__ __forceinline__ void put(int c, int rr, int cc, float v) const
    {
        const int i = off(c) + ((rr * TS + cc) >> ((c & 1) ^ 1));
        if (i >= 0 && i < CA_PLANES) base[i] = v;
    }
    __device__ __forceinline__ float get(int c, int rr, int cc) const { return pl(c)[(rr * TS + cc) >> ((c & 1) ^ 1)]; }
};
__device__ __forceinline__ Planes planes(float *lds)
{
    Planes P;
    P.base = lds;
    return P;
}
__device__ __forceinline__ void zero_lds(float *lds, int n)
{
    for (int i = threadIdx.x; i < n; i += blockDim.x) lds[i] = 0.f;
}

// directional G at a non-green site (L441-470 / L1013-1036: the vector and scalar forms agree)
__device__ __forceinline__ float g_interp(const Planes &P, int c, int indx)
{
    const float *g = P.pl(1), *n = P.pl(c);
    const float wtu = 1.f / SQR(EPS + fabsf(g[indx + TS] - g[indx - TS]) + fabsf(n[indx >> 1] - n[(indx - 2 * TS) >> 1]) + fabsf(g[indx - TS] - g[indx - 3 * TS]));
    const float wtd = 1.f / SQR(EPS + fabsf(g[indx - TS] - g[indx + TS]) + fabsf(n[indx >> 1] - n[(indx + 2 * TS) >> 1]) + fabsf(g[indx + TS] - g[indx + 3 * TS]));
    const float wtl = 1.f / SQR(EPS + fabsf(g[indx + 1] - g[indx - 1]) + fabsf(n[indx >> 1] - n[(indx - 2) >> 1]) + fabsf(g[indx - 1] - g[indx - 3]));
    const float wtr = 1.f / SQR(EPS + fabsf(g[indx - 1] - g[indx + 1]) + fabsf(n[indx >> 1] - n[(indx + 2) >> 1]) + fabsf(g[indx + 1] - g[indx + 3]));
    return (wtu * g[indx - TS] + wtd * g[indx + TS] + wtl * g[indx - 1] + wtr * g[indx + 1]) / (wtu + wtd + wtl + wtr);
}

// ------------------------------------------------------------------------------------------------ pass 1
// Gtmp at (row, col) is written by every tile whose G interpolation covers it (rows top + 3 .. top + rr1 - 4, columns left + 3 ..
// left + cc1 - 4).  Overlapping tiles compute the same value, except where a pass-1 border fill has written past a plane (H % 112
// or W % 112 in 1..7) -- then the reference's result depends on which thread writes last.  The single-thread order defines it:
// the last tile in raster order that covers the sample, i.e. the last tile row covering `row`, and in it the last tile covering `col`.
__device__ __forceinline__ int gtmp_owner_row(const CaArgs &a, int row)
{
    for (int tv = min(a.ntv - 1, (row + 5) / (TS - BORDER2)); tv > 0; --tv) {
        const int top = -BORDER + tv * (TS - BORDER2), rr1 = min(top + TS, a.H + BORDER) - top;
        if (row >= top + 3 && row < top + rr1 - 3) return tv;
    }
    return 0;
}
__device__ __forceinline__ int gtmp_owner_col(const CaArgs &a, int col)
{
    for (int th = min(a.nth - 1, (col + 5) / (TS - BORDER2)); th > 0; --th) {
        const int left = -BORDER + th * (TS - BORDER2), cc1 = min(left + TS, a.W + BORDER) - left;
        if (col >= left + 3 && col < min(left + cc1 - 3, a.width)) return th;
    }
    return 0;
}
// end of the 4-lane body of the filter loop (L495: cc < cc1 - 10) in row rr
__device__ __forceinline__ int filt_vend(const CaArgs &a, int rr, int cc1)
{
    const int c0 = 4 + (fc(a, rr, 2) & 1);
    return c0 < cc1 - 10 ? c0 + 8 * ((cc1 - 10 - c0 + 7) / 8) : c0;
}
// rbhpfv (s = 4 * TS) / rbhpfh (s = 4) at tile index indx; vec: the 4-lane body's association (L500-508), else the scalar tail's
__device__ __forceinline__ float rbhpf(const Planes &P, int c, int indx, int s, bool vec)
{
    const float *G = P.pl(1), *n = P.pl(c);
    const float g0 = G[indx], c0 = n[indx >> 1];
    const float gp = G[indx + s], cp = n[(indx + s) >> 1], gm = G[indx - s], cm = n[(indx - s) >> 1];
    if (vec) return fabsf(fabsf((g0 - c0) - (gp - cp)) + fabsf(gm - cm - g0 + c0) - fabsf(gm - cm - gp + cp));
    return fabsf(fabsf((g0 - c0) - (gp - cp)) + fabsf((gm - cm) - (g0 - c0)) - fabsf((gm - cm) - (gp - cp)));
}
// rblpf / grblpf along step s (2 * TS or 2)
__device__ __forceinline__ void lpf(const Planes &P, int c, int indx, int s, float &rblpf, float &grblpf)
{
    const float *G = P.pl(1), *n = P.pl(c);
    const float glpf = (2.f * G[indx] + G[indx + s] + G[indx - s]);
    const float clpf = (2.f * n[indx >> 1] + n[(indx + s) >> 1] + n[(indx - s) >> 1]);
    rblpf = 0.25f * fabsf(glpf - clpf);
    grblpf = 0.25f * (glpf + clpf);
}
// the six coefficient terms of a site of the coefficient loop (L567-623); vec: 4-lane body form of gdiff
__device__ __forceinline__ void coeff_terms(const CaArgs &a, const Planes &P, int rr, int cc, int cc1, bool vec, float t[6])
{
    const int c = fc(a, rr, cc);
    const float *G = P.pl(1), *n = P.pl(c);
    const int indx = rr * TS + cc, h = indx >> 1;
    // filter values at the sites the weights read: (rr, cc), (rr, cc +- 2), (rr +- 2, cc)
    const int ve0 = filt_vend(a, rr, cc1), vem = filt_vend(a, rr - 2, cc1), vep = filt_vend(a, rr + 2, cc1);
    const float hv0 = rbhpf(P, c, indx, 4 * TS, cc < ve0), hvp = rbhpf(P, c, indx + 2, 4 * TS, cc + 2 < ve0), hvm = rbhpf(P, c, indx - 2, 4 * TS, cc - 2 < ve0);
    const float hh0 = rbhpf(P, c, indx, 4, cc < ve0), hhp = rbhpf(P, c, indx + 2 * TS, 4, cc < vep), hhm = rbhpf(P, c, indx - 2 * TS, 4, cc < vem);
    float lvm, glvm, lvp, glvp, lhm, glhm, lhp, glhp;
    lpf(P, c, indx - 2 * TS, 2 * TS, lvm, glvm);
    lpf(P, c, indx + 2 * TS, 2 * TS, lvp, glvp);
    lpf(P, c, indx - 2, 2, lhm, glhm);
    lpf(P, c, indx + 2, 2, lhp, glhp);
    const float deltgrb = n[h] - G[indx];
    float gdiffv, gdiffh;
    if (vec) {
        const float temp1 = 0.3f * (G[indx + TS + 1] - G[indx - TS - 1]);
        const float temp2 = 0.3f * (G[indx - TS + 1] - G[indx + TS - 1]);
        gdiffv = (G[indx + TS] - G[indx - TS]) + (temp1 - temp2);
        gdiffh = (G[indx + 1] - G[indx - 1]) + (temp1 + temp2);
    } else {
        gdiffv = (G[indx + TS] - G[indx - TS]) + 0.3f * (G[indx + TS + 1] - G[indx - TS + 1] + G[indx + TS - 1] - G[indx - TS - 1]);
        gdiffh = (G[indx + 1] - G[indx - 1]) + 0.3f * (G[indx + 1 + TS] - G[indx - 1 + TS] + G[indx + 1 - TS] - G[indx - 1 - TS]);
    }
    const float gwv = (hv0 + 0.5f * (hvp + hvm)) * (glvm + glvp) / (EPS + 0.1f * (glvm + glvp) + lvm + lvp);
    const float gwh = (hh0 + 0.5f * (hhp + hhm)) * (glhm + glhp) / (EPS + 0.1f * (glhm + glhp) + lhm + lhp);
    t[0] = gwv * deltgrb * deltgrb;
    t[1] = gwv * gdiffv * deltgrb;
    t[2] = gwv * gdiffv * gdiffv;
    t[3] = gwh * deltgrb * deltgrb;
    t[4] = gwh * gdiffh * deltgrb;
    t[5] = gwh * gdiffh * gdiffh;
}

__global__ void __launch_bounds__(CA_NT) ca_pass1_kernel(CaArgs a)
{
    if (!a.words[0]) return;
    extern __shared__ float lds[];
    const Planes P = planes(lds);
    float *lane = lds + CA_PLANES;                         // [row - 8][k][l]
    float *tail = lane + CA_LANE_FLOATS;                   // [row - 8][t][k]
    int *ntail = reinterpret_cast<int *>(tail + CA_TAIL_FLOATS);
    const Tile t = tile_box(a, blockIdx.y, blockIdx.x);
    const int rr1 = t.rr1, cc1 = t.cc1, top = t.top, left = t.left, tid = threadIdx.x;
    zero_lds(lds, CA_PLANES);
    __syncthreads();
    // loader (L325-352): the 4-lane body stores all 8 samples of a step into rgb[1], the scalar parts the green ones only
    {
        const int nr = t.rrmax - t.rrmin, nc = t.ccmax - t.ccmin;
        for (int i = tid; i < nr * nc; i += CA_NT) {
            const int rr = t.rrmin + i / nc, cc = t.ccmin + i % nc;
            const int cst = t.ccmin + (fc(a, rr, t.ccmin) == 1 ? 1 : 0);
            const int vend = cst < t.ccmax - 7 ? cst + 8 * ((t.ccmax - 7 - cst + 7) / 8) : cst;
            const float v = RAW(a, rr + top, cc + left) / 65535.f;
            const int c = fc(a, rr, cc);
            P.put(c, rr, cc, v);
            if (c != 1 && cc >= cst && cc < vend) P.pl(1)[rr * TS + cc] = v;
        }
    }
    __syncthreads();
    // border fills (L354-426), one phase each in the reference's order: for H % 112 or W % 112 in 1..7 a fill writes past its rows /
    // plane into samples that a later fill reads or writes
    const bool ftop = t.rrmin > 0, fbot = t.rrmax < rr1, flef = t.ccmin > 0, frig = t.ccmax < cc1;
    const int ncm = t.ccmax - t.ccmin, nrm = t.rrmax - t.rrmin;
    if (ftop) {
        for (int i = tid; i < BORDER * ncm; i += CA_NT) {
            const int rr = i / ncm, cc = t.ccmin + i % ncm, c = fc(a, rr, cc);
            P.put(c, rr, cc, P.get(c, BORDER2 - rr, cc));
        }
        __syncthreads();
    }
    if (fbot) {
        for (int i = tid; i < BORDER * ncm; i += CA_NT) {
            const int rr = i / ncm, cc = t.ccmin + i % ncm;
            P.put(fc(a, rr, cc), t.rrmax + rr, cc, RAW(a, a.H - rr - 2, left + cc) / 65535.f);
        }
        __syncthreads();
    }
    if (flef) {
        for (int i = tid; i < nrm * BORDER; i += CA_NT) {
            const int rr = t.rrmin + i / BORDER, cc = i % BORDER, c = fc(a, rr, cc);
            P.put(c, rr, cc, P.get(c, rr, BORDER2 - cc));
        }
        __syncthreads();
    }
    if (frig) {
        for (int i = tid; i < nrm * BORDER; i += CA_NT) {
            const int rr = t.rrmin + i / BORDER, cc = i % BORDER;
            P.put(fc(a, rr, cc), rr, t.ccmax + cc, RAW(a, top + rr, a.width - cc - 2) / 65535.f);
        }
        __syncthreads();
    }
    // corners: top-left, bottom-right, top-right, bottom-left
    for (int k = 0; k < 4; ++k) {
        const bool on = k == 0 ? ftop && flef : k == 1 ? fbot && frig : k == 2 ? ftop && frig : fbot && flef;
        if (!on) continue;
        if (tid < BORDER * BORDER) {
            const int rr = tid / BORDER, cc = tid % BORDER, c = fc(a, rr, cc);
            const int r_dst = (k == 0 || k == 2) ? rr : t.rrmax + rr, c_dst = (k == 0 || k == 3) ? cc : t.ccmax + cc;
            const int r_src = (k == 0 || k == 2) ? BORDER2 - rr : a.H - rr - 2, c_src = (k == 0 || k == 3) ? BORDER2 - cc : a.width - cc - 2;
            P.put(c, r_dst, c_dst, RAW(a, r_src, c_src) / 65535.f);
        }
        __syncthreads();
    }
    // G at R/B sites (reads green sites only) and Gtmp (L435-485)
    {
        const int nrow = rr1 - 6, nsite = TSH;
        for (int i = tid; i < nrow * nsite; i += CA_NT) {
            const int rr = 3 + i / nsite;
            const int cc = 3 + (fc(a, rr, 3) & 1) + 2 * (i % nsite);
            if (cc >= cc1 - 3) continue;
            const int indx = rr * TS + cc;
            const float g = g_interp(P, fc(a, rr, cc), indx);
            P.pl(1)[indx] = g;
            const int row = rr + top, col = cc + left;
            if (row >= 0 && row < a.H && col >= 0 && col < a.width && gtmp_owner_row(a, row) == (int)blockIdx.y && gtmp_owner_col(a, col) == (int)blockIdx.x)
                a.Gtmp[((size_t)row * a.width + col) >> 1] = g;
        }
    }
    __syncthreads();
    // coefficient sums (L556-629): lane l of a row sums the sites cc0 + 8k + 2l of the 4-lane body; the scalar tail's terms are
    // kept per site; one thread per (dir, k) then folds the rows in order
    {
        const int nrow = rr1 - 16;
        for (int i = tid; i < nrow * 7; i += CA_NT) {
            const int r = i / 7, j = i % 7, rr = 8 + r;
            const int cc0 = 8 + (fc(a, rr, 2) & 1);
            const int nvec = cc0 < cc1 - 14 ? (cc1 - 14 - cc0 + 7) / 8 : 0;
            const int ct = cc0 + 8 * nvec;
            float tt[6];
            if (j < 4) {
                float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                for (int k = 0; k < nvec; ++k) {
                    coeff_terms(a, P, rr, cc0 + 8 * k + 2 * j, cc1, true, tt);
                    for (int q = 0; q < 6; ++q) acc[q] += tt[q];
                }
                for (int q = 0; q < 6; ++q) lane[(r * 6 + q) * 4 + j] = acc[q];
            } else {
                const int tix = j - 4, cc = ct + 2 * tix;
                if (tix == 0) ntail[r] = cc1 - 8 > ct ? (cc1 - 8 - ct + 1) / 2 : 0;
                if (cc < cc1 - 8) {
                    coeff_terms(a, P, rr, cc, cc1, false, tt);
                    for (int q = 0; q < 6; ++q) tail[(r * 3 + tix) * 6 + q] = tt[q];
                }
            }
        }
        __syncthreads();
        __shared__ float coeff[6][2];
        if (tid < 6) {
            float s0 = 0.f, s1 = 0.f;
            for (int r = 0; r < nrow; ++r) {
                const int rr = 8 + r, cix = fc(a, rr, 8 + (fc(a, rr, 2) & 1)) >> 1;
                const float *l = lane + (r * 6 + tid) * 4;
                float v = cix ? s1 : s0;
                v += (l[0] + l[2]) + (l[1] + l[3]);
                for (int q = 0; q < ntail[r]; ++q) v += tail[(r * 3 + q) * 6 + tid];
                if (cix) s1 = v; else s0 = v;
            }
            coeff[tid][0] = s0;
            coeff[tid][1] = s1;
        }
        __syncthreads();
        if (tid == 0) {
            float cf[2][3][2];
            for (int d = 0; d < 2; ++d)
                for (int k = 0; k < 3; ++k)
                    for (int c = 0; c < 2; ++c) {
                        float v = coeff[d * 3 + k][c] * 0.25f;
                        if (k == 1) v *= 0.3125f;
                        else if (k == 2) v *= SQR(0.3125f);
                        cf[d][k][c] = v;
                    }
            const int blk = t.vblock * a.hblsz + t.hblock;
            float sh[2][2], wt = 0.f;
            for (int c = 0; c < 2; c++)
                for (int d = 0; d < 2; d++) {
                    if (cf[d][2][c] > EPS2) { sh[c][d] = cf[d][1][c] / cf[d][2][c]; wt = cf[d][2][c] / (EPS + cf[d][0][c]); }
                    else { sh[c][d] = 17.0f; wt = 0.f; }
                }
            a.blockwt[blk] = wt;
            reinterpret_cast<float4 *>(a.blockshifts)[blk] = make_float4(sh[0][0], sh[0][1], sh[1][0], sh[1][1]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ fit
constexpr int FIT_NT = 1024;
__device__ __forceinline__ float median9(float a[9])
{
    float tmp;
#define MN(x, y) fmin_(x, y)
#define MX(x, y) fmax_(x, y)
    tmp = MN(a[1], a[2]); a[2] = MX(a[1], a[2]); a[1] = tmp;
    tmp = MN(a[4], a[5]); a[5] = MX(a[4], a[5]); a[4] = tmp;
    tmp = MN(a[7], a[8]); a[8] = MX(a[7], a[8]); a[7] = tmp;
    tmp = MN(a[0], a[1]); a[1] = MX(a[0], a[1]); a[0] = tmp;
    tmp = MN(a[3], a[4]); a[4] = MX(a[3], a[4]); a[3] = tmp;
    tmp = MN(a[6], a[7]); a[7] = MX(a[6], a[7]); a[6] = tmp;
    tmp = MN(a[1], a[2]); a[2] = MX(a[1], a[2]); a[1] = tmp;
    tmp = MN(a[4], a[5]); a[5] = MX(a[4], a[5]); a[4] = tmp;
    tmp = MN(a[7], a[8]); a[8] = MX(a[7], a[8]);
    a[3] = MX(a[0], a[3]);
    a[5] = MN(a[5], a[8]);
    a[7] = MX(a[4], tmp);
    tmp = MN(a[4], tmp);
    a[6] = MX(a[3], a[6]);
    a[4] = MX(a[1], tmp);
    a[2] = MN(a[2], a[5]);
    a[4] = MN(a[4], a[7]);
    tmp = MN(a[4], a[2]);
    a[2] = MX(a[4], a[2]);
    a[4] = MX(a[6], tmp);
    return MN(a[4], a[2]);
#undef MN
#undef MX
}
// LinEqSolve (L42-114), pivot search kept as written (the signed element becomes the running maximum)
__device__ bool lin_eq_solve(int n, double *m, double *v, double *x)
{
    for (int k = 0; k < n - 1; k++) {
        double mx = fabs(m[k * n + k]);
        int p = k;
        for (int i = k + 1; i < n; i++)
            if (mx < fabs(m[i * n + k])) { mx = m[i * n + k]; p = i; }
        if (p != k) {
            for (int i = k; i < n; i++) { const double s = m[k * n + i]; m[k * n + i] = m[p * n + i]; m[p * n + i] = s; }
            const double s = v[k]; v[k] = v[p]; v[p] = s;
        }
        if (m[k * n + k] == 0.) return false;
        for (int j = k + 1; j < n; j++) {
            const double f = -m[j * n + k] / m[k * n + k];
            for (int i = k; i < n; i++) m[j * n + i] = m[j * n + i] + f * m[k * n + i];
            v[j] = v[j] + f * v[k];
        }
    }
    for (int k = n - 1; k >= 0; k--) {
        x[k] = v[k];
        for (int i = k + 1; i < n; i++) x[k] -= (m[k * n + i] * x[i]);
        x[k] = x[k] / m[k * n + k];
    }
    return true;
}
__device__ __forceinline__ double ipow(int b, int e)
{
    double r = 1.0;
    for (int i = 0; i < e; ++i) r *= b;
    return r;
}

__global__ void __launch_bounds__(FIT_NT) ca_fit_kernel(CaArgs a)
{
    if (!a.words[0]) return;
    constexpr int CH = FIT_NT;
    __shared__ float stage[CH * 8];
    __shared__ double polymat[4][256], shiftmat[4][16];
    __shared__ float sums[3][4], blockvar[4];
    __shared__ int numblox[2], pp_s, fail_s;
    const int tid = threadIdx.x;
    const int hblsz = a.hblsz, vblsz = a.vblsz, ntiles = a.ntv * a.nth;
    float4 *bs = reinterpret_cast<float4 *>(a.blockshifts);
    // block sums in tile raster order: thread q = dir * 2 + c
    float s_ave = 0.f, s_sq = 0.f, s_den = 0.f;
    for (int base = 0; base < ntiles; base += CH) {
        const int n = min(CH, ntiles - base);
        if (tid < n) {
            const int ti = base + tid, blk = (ti / a.nth + 1) * hblsz + ti % a.nth + 1;
            const float4 v = bs[blk];
            stage[tid * 4 + 0] = v.x; stage[tid * 4 + 1] = v.y; stage[tid * 4 + 2] = v.z; stage[tid * 4 + 3] = v.w;
        }
        __syncthreads();
        if (tid < 4) {
            const int dir = tid >> 1, c = tid & 1;
            for (int i = 0; i < n; ++i) {
                const float sh = stage[i * 4 + c * 2 + dir];
                if (fabsf(sh) < 2.0f) { s_ave += sh; s_sq += SQR(sh); s_den += 1; }
            }
        }
        __syncthreads();
    }
    if (tid < 4) { sums[0][tid] = s_ave; sums[1][tid] = s_sq; sums[2][tid] = s_den; }
    if (tid < 2) numblox[tid] = 0;
    __syncthreads();
    if (tid == 0) {
        int pp = 1;
        for (int dir = 0; dir < 2; dir++)
            for (int c = 0; c < 2; c++) {
                const int q = dir * 2 + c;
                if (sums[2][q]) blockvar[q] = sums[1][q] / sums[2][q] - SQR(sums[0][q] / sums[2][q]);
                else { pp = 0; break; }
            }
        pp_s = pp;
        fail_s = 0;
    }
    __syncthreads();
    if (!pp_s) {
        if (tid == 0) { a.words[1] = 0; a.words[2] = 4; }
        return;
    }
    // border blocks (L725-741): left / right columns, then top / bottom rows (corners from the filled columns)
    for (int vb = 1 + tid; vb < vblsz - 1; vb += FIT_NT) {
        bs[vb * hblsz] = bs[vb * hblsz + 2];
        bs[vb * hblsz + hblsz - 1] = bs[vb * hblsz + hblsz - 3];
    }
    __syncthreads();
    for (int hb = tid; hb < hblsz; hb += FIT_NT) {
        bs[hb] = bs[2 * hblsz + hb];
        bs[(vblsz - 1) * hblsz + hb] = bs[(vblsz - 3) * hblsz + hb];
    }
    __syncthreads();
    // 3x3 medians and the rejection rule per inner block -> a.blockfit[blk] = {bst[c][dir], accept[c]}
    const int nbh = hblsz - 2, nblk = (vblsz - 2) * nbh;
    for (int i = tid; i < nblk; i += FIT_NT) {
        const int vb = 1 + i / nbh, hb = 1 + i % nbh;
        float out[6];
        for (int c = 0; c < 2; c++) {
            float bst[2];
            for (int dir = 0; dir < 2; dir++) {
                float p[9];
                int k = 0;
                for (int dv = -1; dv <= 1; ++dv)
                    for (int dh = -1; dh <= 1; ++dh) {
                        const float4 v = bs[(vb + dv) * hblsz + hb + dh];
                        const int e = c * 2 + dir;
                        p[k++] = e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w;
                    }
                bst[dir] = median9(p);
            }
            const bool rej = SQR(bst[0]) > 8.f * blockvar[c] || SQR(bst[1]) > 8.f * blockvar[2 + c];
            out[c * 2] = bst[0]; out[c * 2 + 1] = bst[1];
            out[4 + c] = rej ? 0.f : 1.f;
            if (!rej) atomicAdd(&numblox[c], 1);
        }
        float *f = a.blockfit + (size_t)i * 8;
        for (int q = 0; q < 6; ++q) f[q] = out[q];
        f[6] = a.blockwt[vb * hblsz + hb];
    }
    __syncthreads();
    // polymat / shiftmat (L786-805): one accumulator per thread, blocks in order
    double acc0 = 0.0, acc1 = 0.0;
    const int e_a = tid, e_b = tid + FIT_NT;
    for (int base = 0; base < nblk; base += CH) {
        const int n = min(CH, nblk - base);
        if (tid < n) {
            const float *f = a.blockfit + (size_t)(base + tid) * 8;
            for (int q = 0; q < 7; ++q) stage[tid * 8 + q] = f[q];
        }
        __syncthreads();
        for (int pass = 0; pass < 2; ++pass) {
            const int e = pass ? e_b : e_a;
            if (e >= 4 * 272) continue;
            const int cd = e / 272, q = e % 272, c = cd >> 1, dir = cd & 1;
            double acc = pass ? acc1 : acc0;
            if (q < 256) {
                const int ij = q >> 4, mn = q & 15, i = ij >> 2, j = ij & 3, m = mn >> 2, nn = mn & 3;
                for (int b = 0; b < n; ++b) {
                    const float *f = stage + b * 8;
                    if (f[4 + c] == 0.f) continue;
                    const int blk = base + b, vb = 1 + blk / nbh, hb = 1 + blk % nbh;
                    acc += ipow(vb, i + m) * ipow(hb, j + nn) * (double)f[6];
                }
            } else {
                const int s = q - 256, i = s >> 2, j = s & 3;
                for (int b = 0; b < n; ++b) {
                    const float *f = stage + b * 8;
                    if (f[4 + c] == 0.f) continue;
                    const int blk = base + b, vb = 1 + blk / nbh, hb = 1 + blk % nbh;
                    acc += ipow(vb, i) * ipow(hb, j) * (double)f[c * 2 + dir] * (double)f[6];
                }
            }
            if (pass) acc1 = acc; else acc0 = acc;
        }
        __syncthreads();
    }
    for (int pass = 0; pass < 2; ++pass) {
        const int e = pass ? e_b : e_a;
        if (e >= 4 * 272) continue;
        const int cd = e / 272, q = e % 272;
        if (q < 256) polymat[cd][q] = pass ? acc1 : acc0;
        else shiftmat[cd][q - 256] = pass ? acc1 : acc0;
    }
    __syncthreads();
    const int nb = min(numblox[0], numblox[1]);
    const int polyord = nb < 32 ? 2 : 4, numpar = polyord * polyord;
    const bool pp = nb >= 10;
    if (pp && tid < 4) {
        double x[16];
        if (lin_eq_solve(numpar, polymat[tid], shiftmat[tid], x)) {
            for (int k = 0; k < numpar; ++k) a.fit[tid * 16 + k] = x[k];
        } else {
            atomicOr(&fail_s, 1);
        }
    }
    __syncthreads();
    if (tid == 0) { a.words[1] = (pp && !fail_s) ? 1 : 0; a.words[2] = polyord; }
}

// ------------------------------------------------------------------------------------------------ pass 2
__global__ void __launch_bounds__(CA_NT) ca_pass2_kernel(CaArgs a)
{
    if (!a.words[0] || !a.words[1]) return;
    extern __shared__ float lds[];
    const Planes P = planes(lds);
    float *G = P.pl(1);
    const Tile t = tile_box(a, blockIdx.y, blockIdx.x);
    const int rr1 = t.rr1, cc1 = t.cc1, top = t.top, left = t.left, tid = threadIdx.x;
    const int width = a.width;
    zero_lds(lds, CA_PLANES);
    __syncthreads();
    {
        const int nr = t.rrmax - t.rrmin, nc = t.ccmax - t.ccmin;
        for (int i = tid; i < nr * nc; i += CA_NT) {
            const int rr = t.rrmin + i / nc, cc = t.ccmin + i % nc, row = rr + top, col = cc + left, c = fc(a, rr, cc);
            P.put(c, rr, cc, RAW(a, row, col) / 65535.f);
            if ((c & 1) == 0) G[rr * TS + cc] = a.Gtmp[((size_t)row * width + col) >> 1];
        }
    }
    __syncthreads();
    // border fills (L909-1001)
    const int nb_r = min(BORDER, rr1 - t.rrmax), nb_c = min(BORDER, cc1 - t.ccmax);
    for (int i = tid; i < BORDER * TS; i += CA_NT) {
        const int rr = i / TS, cc = i % TS;
        if (cc >= t.ccmin && cc < t.ccmax) {
            const int c = fc(a, rr, cc);
            if (t.rrmin > 0) {
                P.put(c, rr, cc, P.get(c, BORDER2 - rr, cc));
                G[rr * TS + cc] = G[(BORDER2 - rr) * TS + cc];
            }
            if (t.rrmax < rr1 && rr < nb_r) {
                P.put(c, t.rrmax + rr, cc, RAW(a, a.H - rr - 2, left + cc) / 65535.f);
                if ((c & 1) == 0) G[(t.rrmax + rr) * TS + cc] = a.Gtmp[((size_t)(a.H - rr - 2) * width + left + cc) >> 1];
            }
        }
        if (cc < BORDER) {
            const int c = fc(a, rr, cc);
            if (t.rrmin > 0 && t.ccmin > 0) {
                P.put(c, rr, cc, RAW(a, BORDER2 - rr, BORDER2 - cc) / 65535.f);
                if ((c & 1) == 0) G[rr * TS + cc] = a.Gtmp[((size_t)(BORDER2 - rr) * width + BORDER2 - cc) >> 1];
            }
            if (t.rrmax < rr1 && t.ccmax < cc1 && rr < nb_r && cc < nb_c) {
                P.put(c, t.rrmax + rr, t.ccmax + cc, RAW(a, a.H - rr - 2, width - cc - 2) / 65535.f);
                if ((c & 1) == 0) G[(t.rrmax + rr) * TS + t.ccmax + cc] = a.Gtmp[((size_t)(a.H - rr - 2) * width + (width - cc - 2)) >> 1];
            }
            if (t.rrmin > 0 && t.ccmax < cc1 && cc < nb_c) {
                P.put(c, rr, t.ccmax + cc, RAW(a, BORDER2 - rr, width - cc - 2) / 65535.f);
                if ((c & 1) == 0) G[rr * TS + t.ccmax + cc] = a.Gtmp[((size_t)(BORDER2 - rr) * width + (width - cc - 2)) >> 1];
            }
            if (t.rrmax < rr1 && t.ccmin > 0 && rr < nb_r) {
                P.put(c, t.rrmax + rr, cc, RAW(a, a.H - rr - 2, BORDER2 - cc) / 65535.f);
                if ((c & 1) == 0) G[(t.rrmax + rr) * TS + cc] = a.Gtmp[((size_t)(a.H - rr - 2) * width + (BORDER2 - cc)) >> 1];
            }
        }
    }
    for (int i = tid; i < TS * BORDER; i += CA_NT) {
        const int rr = i / BORDER, cc = i % BORDER;
        if (rr < t.rrmin || rr >= t.rrmax) continue;
        const int c = fc(a, rr, cc);
        if (t.ccmin > 0) {
            P.put(c, rr, cc, P.get(c, rr, BORDER2 - cc));
            G[rr * TS + cc] = G[rr * TS + BORDER2 - cc];
        }
        if (t.ccmax < cc1 && cc < nb_c) {
            P.put(c, rr, t.ccmax + cc, RAW(a, top + rr, width - cc - 2) / 65535.f);
            if ((c & 1) == 0) G[rr * TS + t.ccmax + cc] = a.Gtmp[((size_t)(top + rr) * width + (width - cc - 2)) >> 1];
        }
    }
    __syncthreads();
    if (!a.autoCA) {   // manual: G at R/B sites recomputed (L1004-1037), first site 3 + fc(rr, 1)
        const int nrow = rr1 - 6;
        for (int i = tid; i < nrow * TSH; i += CA_NT) {
            const int rr = 3 + i / TSH;
            const int cc = 3 + fc(a, rr, 1) + 2 * (i % TSH);
            if (cc >= cc1 - 3) continue;
            G[rr * TS + cc] = g_interp(P, fc(a, rr, cc), rr * TS + cc);
        }
        __syncthreads();
    }
    // shift parameters of the tile (L1040-1089)
    float lbs[2][2];
    if (!a.autoCA) {
        const float hfrac = -((float)(t.hblock - 0.5) / (a.hblsz - 2) - 0.5);
        const float vfrac = -((float)(t.vblock - 0.5) / (a.vblsz - 2) - 0.5) * a.H / width;
        lbs[0][0] = 2 * vfrac * a.cared;
        lbs[0][1] = 2 * hfrac * a.cared;
        lbs[1][0] = 2 * vfrac * a.cablue;
        lbs[1][1] = 2 * hfrac * a.cablue;
        // no limit in the reference (L1040-1046); beyond +-MAX_MANUAL_SHIFT its reads would leave rgb[0] .. rgb[2] (ART's sliders stay
        // far inside: |shift| <= 8 * H / W)
        for (int p = 0; p < 2; ++p)
            for (int q = 0; q < 2; ++q) lbs[p][q] = fmax_(-MAX_MANUAL_SHIFT, fmin_(lbs[p][q], MAX_MANUAL_SHIFT));
    } else {
        const int polyord = a.words[2];
        lbs[0][0] = lbs[0][1] = lbs[1][0] = lbs[1][1] = 0.f;
        double pv = 1.0;
        for (int i = 0; i < polyord; i++) {
            double ph = pv;
            for (int j = 0; j < polyord; j++) {
                lbs[0][0] += ph * a.fit[0 * 16 + polyord * i + j];
                lbs[0][1] += ph * a.fit[1 * 16 + polyord * i + j];
                lbs[1][0] += ph * a.fit[2 * 16 + polyord * i + j];
                lbs[1][1] += ph * a.fit[3 * 16 + polyord * i + j];
                ph *= t.hblock;
            }
            pv *= t.vblock;
        }
        constexpr float bslim = 3.99f;
        for (int p = 0; p < 2; ++p)
            for (int q = 0; q < 2; ++q) lbs[p][q] = fmax_(-bslim, fmin_(lbs[p][q], bslim));
    }
    int svf[2], svc[2], shf[2], shc[2], d0[2], d1[2];
    float svfrac[2], shfrac[2];
    for (int k = 0; k < 2; ++k) {
        svf[k] = (int)floorf(lbs[k][0]);
        svc[k] = (int)ceilf(lbs[k][0]);
        if (lbs[k][0] < 0.f) { const int s = svf[k]; svf[k] = svc[k]; svc[k] = s; }
        svfrac[k] = fabsf(lbs[k][0] - svf[k]);
        shf[k] = (int)floorf(lbs[k][1]);
        shc[k] = (int)ceilf(lbs[k][1]);
        if (lbs[k][1] < 0.f) { const int s = shf[k]; shf[k] = shc[k]; shc[k] = s; }
        shfrac[k] = fabsf(lbs[k][1] - shf[k]);
        d0[k] = lbs[k][0] > 0 ? 2 : -2;
        d1[k] = lbs[k][1] > 0 ? 2 : -2;
    }
    // correction (L1091-1218) and the write to RawDataTmp (L1221-1235); grbdiff / gshift at the four sites a site reads are
    // recomputed from the bilinear G (L1102-1127), rgb[c] is read before any site changes it
    const int nrow = rr1 - 16;
    for (int i = tid; i < nrow * TSH; i += CA_NT) {
        const int rr = 8 + i / TSH;
        const int cc = 8 + (fc(a, rr, 2) & 1) + 2 * (i % TSH);
        if (cc >= cc1 - 8) continue;
        const int c = fc(a, rr, cc);
        const bool k = c >> 1;                  // per-colour parameters by select: no dynamically indexed private arrays
        const float *n = P.pl(c);
        const int D0 = k ? d0[1] : d0[0], D1 = k ? d1[1] : d1[0];
        const int SVF = k ? svf[1] : svf[0], SVC = k ? svc[1] : svc[0], SHF = k ? shf[1] : shf[0], SHC = k ? shc[1] : shc[0];
        const float SHFRAC = k ? shfrac[1] : shfrac[0], SVFRAC = k ? svfrac[1] : svfrac[0];
        float gi[4], gd[4];
        const int pr[4] = {rr, rr, rr - D0, rr - D0}, pc[4] = {cc, cc - D1, cc, cc - D1};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int r0 = pr[s], c0 = pc[s];
            const float hfl = intp(SHFRAC, G[(r0 + SVF) * TS + c0 + SHC], G[(r0 + SVF) * TS + c0 + SHF]);
            const float hce = intp(SHFRAC, G[(r0 + SVC) * TS + c0 + SHC], G[(r0 + SVC) * TS + c0 + SHF]);
            const float gint = intp(SVFRAC, hce, hfl);
            gi[s] = gint;
            gd[s] = gint - n[(r0 * TS + c0) >> 1];
        }
        const float hf2 = SHFRAC / 2.f, vf2 = SVFRAC / 2.f;
        const int indx = rr * TS + cc;
        const float gv = G[indx], cv = n[indx >> 1];
        float out = cv;
        const float grbdiffold = gv - cv;
        const float hfl = intp(hf2, gd[1], gd[0]);
        const float hce = intp(hf2, gd[3], gd[2]);
        float grbdiffint = intp(vf2, hce, hfl);
        const float RBint = gv - grbdiffint;
        if (fabsf(RBint - cv) < 0.25f * (RBint + cv)) {
            if (fabsf(grbdiffold) > fabsf(grbdiffint)) out = RBint;
        } else {
            const float p0 = 1.f / (EPS + fabsf(gv - gi[0]));
            const float p1 = 1.f / (EPS + fabsf(gv - gi[1]));
            const float p2 = 1.f / (EPS + fabsf(gv - gi[2]));
            const float p3 = 1.f / (EPS + fabsf(gv - gi[3]));
            grbdiffint = (p0 * gd[0] + p1 * gd[1] + p2 * gd[2] + p3 * gd[3]) / (p0 + p1 + p2 + p3);
            if (fabsf(grbdiffold) > fabsf(grbdiffint)) out = gv - grbdiffint;
        }
        if (grbdiffold * grbdiffint < 0) out = gv - 0.5f * (grbdiffold + grbdiffint);
        const int row = rr + top;
        if (((left + cc) >> 1) < ((cc1 - BORDER + left) >> 1)) a.RawDataTmp[(size_t)row * (width >> 1) + ((left + cc) >> 1)] = 65535.f * out;
    }
}

__global__ void ca_copyback_kernel(CaArgs a)
{
    if (!a.words[0] || !a.words[1]) return;
    const int row = CB + blockIdx.y;
    const int col = CB + (fc(a, row, 0) & 1) + 2 * (blockIdx.x * blockDim.x + threadIdx.x);
    if (row >= a.H - CB || col >= a.width - CB) return;
    const float v = a.RawDataTmp[((size_t)row * a.width + col) >> 1];
    a.raw[(size_t)row * a.stride + col] = v > 0.f ? v : 0.f;
}

// ------------------------------------------------------------------------------------------------ colour-shift guard
__global__ void ca_capture_kernel(CaArgs a)
{
    const int i = CB + blockIdx.y;
    const int j = CB + (fc(a, i, 0) & 1) + 2 * (blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= a.H - CB || j >= a.W - CB) return;
    a.oldraw[(size_t)(i - CB) * a.fw + (j - CB) / 2] = RAW(a, i, j);
}
__global__ void ca_factors_kernel(CaArgs a)
{
    if (!a.words[0]) return;
    const int i = blockIdx.y;
    const int first = fc(a, i, 0) & 1;
    const int j = first + 2 * (blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= a.W - 2 * CB) return;
    float *ng = fc(a, i, first) == 0 ? a.red : a.blue;
    const float nv = RAW(a, i + CB, j + CB), ov = a.oldraw[(size_t)i * a.fw + j / 2];
    ng[(size_t)(i / 2) * a.fw + j / 2] = (nv <= 1.f || ov <= 1.f) ? 1.f : fmax_(0.5f, fmin_(ov / nv, 2.f));
}
__global__ void __launch_bounds__(256) ca_factor_fill_kernel(CaArgs a)
{
    if (!a.words[0]) return;
    const int fw = a.fw, fh = a.fh;
    if (a.H % 2)
        for (int j = threadIdx.x; j < fw; j += blockDim.x) {
            a.red[(size_t)(fh - 1) * fw + j] = a.red[(size_t)(fh - 2) * fw + j];
            a.blue[(size_t)(fh - 1) * fw + j] = a.blue[(size_t)(fh - 2) * fw + j];
        }
    __syncthreads();
    if (a.W % 2) {
        const int ngRow = 1 - (fc(a, 0, 0) & 1);
        const int ngCol = fc(a, ngRow, 0) & 1;
        float *ng = fc(a, ngRow, ngCol) == 0 ? a.red : a.blue;
        for (int i = threadIdx.x; i < fh; i += blockDim.x) ng[(size_t)i * fw + fw - 1] = ng[(size_t)i * fw + fw - 2];
    }
}
__global__ void ca_apply_kernel(CaArgs a)
{
    if (!a.words[0]) return;
    const int i = blockIdx.y;
    const int first = fc(a, i, 0) & 1;
    const int j = first + 2 * (blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= a.W - 2 * CB) return;
    const float *ng = fc(a, i, first) == 0 ? a.red : a.blue;
    a.raw[(size_t)(i + CB) * a.stride + j + CB] *= ng[(size_t)(i / 2) * a.fw + j / 2];
}
// end of an iteration: the next one runs if this one ran pass 2 (the loop condition `it < iterations && processpasstwo`)
__global__ void ca_step_kernel(CaArgs a)
{
    if (threadIdx.x == 0) a.words[0] = a.words[0] && a.words[1];
}

} // namespace

hipError_t launch_ca_capture(const CaArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(ca_capture_kernel, dim3((a.W / 2 + 127) / 128, a.H - 2 * CB), dim3(128), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_ca_iteration(const CaArgs &a, hipStream_t s)
{
    const dim3 tiles(a.nth, a.ntv);
    if (a.autoCA) {
        if (hipError_t e = dyn_lds_once(reinterpret_cast<const void *>(&ca_pass1_kernel), CA_PASS1_LDS); e != hipSuccess) return e;
        hipLaunchKernelGGL(ca_pass1_kernel, tiles, dim3(CA_NT), CA_PASS1_LDS, s, a);
        hipLaunchKernelGGL(ca_fit_kernel, dim3(1), dim3(FIT_NT), 0, s, a);
    }
    if (hipError_t e = dyn_lds_once(reinterpret_cast<const void *>(&ca_pass2_kernel), CA_PASS2_LDS); e != hipSuccess) return e;
    hipLaunchKernelGGL(ca_pass2_kernel, tiles, dim3(CA_NT), CA_PASS2_LDS, s, a);
    hipLaunchKernelGGL(ca_copyback_kernel, dim3((a.width / 2 + 127) / 128, a.H - 2 * CB), dim3(128), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_ca_factors(const CaArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(ca_factors_kernel, dim3((a.W / 2 + 127) / 128, a.H - 2 * CB), dim3(128), 0, s, a);
    hipLaunchKernelGGL(ca_factor_fill_kernel, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_ca_apply(const CaArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(ca_apply_kernel, dim3((a.W / 2 + 127) / 128, a.H - 2 * CB), dim3(128), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_ca_step(const CaArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(ca_step_kernel, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}

} // namespace artgpu
