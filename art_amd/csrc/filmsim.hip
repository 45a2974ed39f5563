// art_amd/csrc/filmsim.hip -- ImProcFunctions::filmSimulation's pixel pass on gfx950: the HaldCLUT path of CLUTApplication
// (reference: rtengine/clutstore.cc:1502-1615 CLUTApplication::do_apply, :178-288 HaldCLUT::getRGB in its __SSE2__ form, :104-131
//  getClutValues; Color::rgbxyz / Color::xyz2rgb in their vfloat and double-matrix overloads, color.cc:826-894; Color::gamma_srgbclipped /
//  Color::igamma_srgb, color.h:1288-1299, i.e. LUTf::operator[](float), LUT.h:436-459, of a table that clips on both sides and of one that
//  clips on neither).
//
// One pixel per lane, one kernel, in place: 24 B/px of image.  Per pixel six interpolated lookups into the two 65536-entry tables and four
// 16-byte reads of the CLUT -- an entry and its red neighbour lie next to each other, so the eight corners of the cell are four reads, as
// in the reference.  The four are issued together, ahead of the first interpolation: each is a miss of its own for a pixel that lands in a
// cell its neighbours do not share.  No LDS: neither a gamma table (256 KB) nor the CLUT (2 .. 134 MB) fits.
//
// The reference converts between the working and the CLUT's profile four columns at a time with float matrices (L1518-1532, L1581-1595)
// and the W % 4 columns behind them one at a time with the double matrices (L1536-1544, L1599-1607): which form a pixel gets depends on
// its column alone, counted from column 0 of the row.
#include <hip/hip_runtime.h>
#include "devsleef.h"
#include "filmsim.h"

namespace artgpu {

namespace {

constexpr int FS_BX = 64, FS_BY = 4;      // a workgroup covers 64 x 4 pixels: a wave works on one row

// vintpf (sleefsseavx.h:1435-1442)
__device__ __forceinline__ float fs_intp(float a, float b, float c) { return a * b + (1.f - a) * c; }

// Color::rgbxyz then Color::xyz2rgb: the vfloat overloads with float matrices (body) or the scalar ones with double matrices (tail)
__device__ __forceinline__ void fs_convert(float &r, float &g, float &b, bool body, const float *m1, const float *m2, const double *d1, const double *d2)
{
    if (body) {
        const float x = m1[0] * r + m1[1] * g + m1[2] * b;
        const float y = m1[3] * r + m1[4] * g + m1[5] * b;
        const float z = m1[6] * r + m1[7] * g + m1[8] * b;
        r = m2[0] * x + m2[1] * y + m2[2] * z;
        g = m2[3] * x + m2[4] * y + m2[5] * z;
        b = m2[6] * x + m2[7] * y + m2[8] * z;
    } else {
        const float x = (float)(d1[0] * r + d1[1] * g + d1[2] * b);
        const float y = (float)(d1[3] * r + d1[4] * g + d1[5] * b);
        const float z = (float)(d1[6] * r + d1[7] * g + d1[8] * b);
        r = (float)(d2[0] * x + d2[1] * y + d2[2] * z);
        g = (float)(d2[3] * x + d2[4] * y + d2[5] * z);
        b = (float)(d2[6] * x + d2[7] * y + d2[8] * z);
    }
}

// LUTf::operator[](float) of a table constructed with flags 0 (Color::igammatab_srgb): it extrapolates past either end
__device__ __forceinline__ float fs_lut_noclip(const float *__restrict__ data, float index)
{
    int idx;
    if (index < 0.f || !(index == index)) idx = 0;
    else if (index > 65534.f) idx = 65534;
    else idx = (int)index;
    const float diff = index - (float)idx;
    const float p1 = data[idx];
    const float p2 = data[idx + 1] - p1;
    return p1 + p2 * diff;
}

// getClutValues (clutstore.cc:105-131): the 16 bytes at an entry, i.e. the entry and the next one in red
struct __attribute__((aligned(8))) FsPair { unsigned short v[8]; };

} // namespace

template <bool SAME_PROFILE>
__global__ void __launch_bounds__(256) filmsim_kernel(FsArgs a)
{
    const int x = blockIdx.x * FS_BX + (threadIdx.x & (FS_BX - 1)), y = blockIdx.y * FS_BY + threadIdx.x / FS_BX;
    if (x >= a.W || y >= a.H) return;
    const size_t si = (size_t)y * a.stride + x;
    float r = a.img[0][si], g = a.img[1][si], b = a.img[2][si];
    const bool body = x < (a.W & ~3);
    if (!SAME_PROFILE) fs_convert(r, g, b, body, a.mf[FS_WORK2XYZ], a.mf[FS_XYZ2CLUT], a.md[FS_WORK2XYZ], a.md[FS_XYZ2CLUT]);
    // Color::gamma_srgbclipped (L1557-1559)
    r = lutf_lookup<true>(a.gam, 65536, r);
    g = lutf_lookup<true>(a.gam, 65536, g);
    b = lutf_lookup<true>(a.gam, 65536, b);
    // HaldCLUT::getRGB: the cell (L196-200) and the position inside it (L250-251).  The encoded values are not negative, so the unsigned
    // conversion of L196 and the truncating one of L251 see the same number
    const float tr = r * a.flm1, tg = g * a.flm1, tb = b * a.flm1;
    const float cr = tr < a.flm2 ? tr : a.flm2, cg = tg < a.flm2 ? tg : a.flm2, cb = tb < a.flm2 ? tb : a.flm2;
    const unsigned red = (unsigned)cr, green = (unsigned)cg, blue = (unsigned)cb;
    const float fr = tr - (float)(int)red, fg = tg - (float)(int)green, fb = tb - (float)(int)blue;
    const unsigned level = a.level, level_square = level * level;
    const unsigned color = red + green * level + blue * level_square;     // at most level^3 - 2: the neighbour in red is the last entry
    const auto pair_at = [&](unsigned entry) -> FsPair { return *reinterpret_cast<const FsPair *>(a.clut + 4 * (size_t)entry); };
    const FsPair p00 = pair_at(color), p10 = pair_at(color + level), p01 = pair_at(color + level_square), p11 = pair_at(color + level + level_square);
    float in[3] = {r, g, b}, res[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t1 = fs_intp(fr, (float)p00.v[4 + c], (float)p00.v[c]);        // L258
        const float t2 = fs_intp(fr, (float)p10.v[4 + c], (float)p10.v[c]);        // L263
        float out = fs_intp(fg, t2, t1);                                           // L267
        const float u1 = fs_intp(fr, (float)p01.v[4 + c], (float)p01.v[c]);        // L272
        const float u2 = fs_intp(fr, (float)p11.v[4 + c], (float)p11.v[c]);        // L277
        const float u = fs_intp(fg, u2, u1);                                       // L279
        out = fs_intp(fb, u, out);                                                 // L283
        res[c] = fs_intp(a.strength, out, in[c]);                                  // L285
    }
    // Color::igamma_srgb (L1570-1572)
    r = fs_lut_noclip(a.igam, res[0]);
    g = fs_lut_noclip(a.igam, res[1]);
    b = fs_lut_noclip(a.igam, res[2]);
    if (!SAME_PROFILE) fs_convert(r, g, b, body, a.mf[FS_CLUT2XYZ], a.mf[FS_XYZ2WORK], a.md[FS_CLUT2XYZ], a.md[FS_XYZ2WORK]);
    a.img[0][si] = r; a.img[1][si] = g; a.img[2][si] = b;
}

hipError_t launch_filmsim(const FsArgs &a, bool same_profile, hipStream_t s)
{
    const dim3 grid((a.W + FS_BX - 1) / FS_BX, (a.H + FS_BY - 1) / FS_BY);
    if (same_profile) hipLaunchKernelGGL(filmsim_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(filmsim_kernel<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace artgpu
