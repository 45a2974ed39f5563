// art_amd/csrc/jzazbzdev.h -- Color::rgb2jzazbz / jzazbz2rgb on the device (reference: rtengine/color.cc:48-86, 6706-6742 and color.h:1765-1778),
// shared by the NEUTRAL tone curve (tonecurve.hip) and the colour correction (colorcorrection.hip), as labdev.h shares Color::rgb2lab.
// The PQ tables are the host-built ones (build_pq_luts: Color::init's jzazbz_pq_ / jzazbz_pq_inv_); an argument outside [0, 1] takes
// PQ / PQ_inv themselves, a per-pixel powf with the bits of the host's libm (libmpowf.h; the tests keep their tolerance there).  The two conversions take the table
// lookup as a callable, so that a kernel decides where its tables live and what else a lookup records.
#pragma once
#include <hip/hip_runtime.h>
#include "devmath.h"
#include "devsleef.h"
#include "libmpowf.h"

namespace artgpu {

__device__ __forceinline__ float dev_PQ(float X)
{
    X = std_max(X, 1e-10f);
    const float XX = libm_powf(X * 1e-4f, 0.1593017578125f);
    return libm_powf((0.8359375f + 18.8515625f * XX) / (1 + 18.6875f * XX), 134.034375f);
}
__device__ __forceinline__ float dev_PQ_inv(float X)
{
    X = std_max(X, 1e-10f);
    const float XX = libm_powf(X, 7.460772656268214e-03f);
    return 1e4f * libm_powf((0.8359375f - XX) / (18.6875f * XX - 18.8515625f), 6.277394636015326f);
}
// LUTf::operator[](float), flags 0, index >= 0 here
__device__ __forceinline__ float lut_noclip(const float *__restrict__ data, float index)
{
    int idx = (int)index;
    if (index < 0.f || !(index == index)) idx = 0;
    else if (index > 65534.f) idx = 65534;
    const float diff = index - (float)idx;
    const float p1 = data[idx], p2 = data[idx + 1] - p1;
    return p1 + p2 * diff;
}
// the forward PQ table: six lookups per pixel, the hottest of the kernel's three 256 KB tables.  `lds` != nullptr: entries
// [0, LUT_LDS_N) are resident in LDS (the persistent launch shape of tonecurve.hip), the rest and the other two tables come from L2.
struct PqTab { const float *g; const float *lds; };
__device__ __forceinline__ float get_pq(const PqTab pq, float x)
{
    if (!(x >= 0.f && x <= 1.f)) return dev_PQ(x);
    if (!pq.lds) return lut_noclip(pq.g, x * 65535.f);
    const float index = x * 65535.f;
    int idx = (int)index;
    if (index > 65534.f) idx = 65534;
    const float diff = index - (float)idx;
    float p1, q;
    if (idx + 1 < LUT_LDS_N) { lds_cfloat *l = (lds_cfloat *)pq.lds; p1 = l[idx]; q = l[idx + 1]; }     // (LDS-qualified: ds_read, not flat_load)
    else { p1 = pq.g[idx]; q = pq.g[idx + 1]; }
    const float p2 = q - p1;
    return p1 + p2 * diff;
}
__device__ __forceinline__ float get_pq_inv(const float *__restrict__ pqi, float x) { return (x >= 0.f && x <= 1.f) ? lut_noclip(pqi, x * 65535.f) : dev_PQ_inv(x); }

// dot_product(Mat33, Vec3) (linalgebra.h:226-239): accumulates from 0
__device__ __forceinline__ void mat_vec(const float *m, const float v[3], float r[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float acc = 0;
        acc += m[3 * i + 0] * v[0];
        acc += m[3 * i + 1] * v[1];
        acc += m[3 * i + 2] * v[2];
        r[i] = acc;
    }
}
// Color::rgb2jzazbz: rgbxyz, XYZ_D50_to_D65, xyz2jzazbz.  pq(x) is get_PQ
template <class PQ>
__device__ __forceinline__ void rgb2jzazbz_dev(const PQ &pq, float R, float G, float B, float &Jz, float &az, float &bz, const float *ws)
{
    const float D[9] = {0.9555766f, -0.0230393f, 0.0631636f, -0.0282895f, 1.0099416f, 0.0210077f, 0.0122982f, -0.0204830f, 1.3299098f};
    float v[3] = {ws[0] * R + ws[1] * G + ws[2] * B, ws[3] * R + ws[4] * G + ws[5] * B, ws[6] * R + ws[7] * G + ws[8] * B}, d[3];
    mat_vec(D, v, d);
    const float X = d[0], Y = d[1], Z = d[2];
    const float Lp = pq(0.674207838f * X + 0.382799340f * Y - 0.047570458f * Z);
    const float Mp = pq(0.149284160f * X + 0.739628340f * Y + 0.083327300f * Z);
    const float Sp = pq(0.070941080f * X + 0.174768000f * Y + 0.670970020f * Z);
    const float Iz = 0.5f * (Lp + Mp);
    az = 3.524000f * Lp - 4.066708f * Mp + 0.542708f * Sp;
    bz = 0.199076f * Lp + 1.096799f * Mp - 1.295875f * Sp;
    Jz = (0.44f * Iz) / (1.f - 0.56f * Iz) - 1.6295499532821566e-11f;
}
// Color::jzazbz2rgb: jzazbz2xyz, XYZ_D65_to_D50, xyz2rgb.  pqi(x) is get_PQ_inv
template <class PQI>
__device__ __forceinline__ void jzazbz2rgb_dev(const PQI &pqi, float Jz, float az, float bz, float &R, float &G, float &B, const float *iws)
{
    const float D[9] = {1.0478112f, 0.0228866f, -0.0501270f, 0.0295424f, 0.9904844f, -0.0170491f, -0.0092345f, 0.0150436f, 0.7521316f};
    Jz = Jz + 1.6295499532821566e-11f;
    const float Iz = Jz / (0.44f + 0.56f * Jz);
    const float L = pqi(Iz + 1.386050432715393e-1f * az + 5.804731615611869e-2f * bz);
    const float M = pqi(Iz - 1.386050432715393e-1f * az - 5.804731615611891e-2f * bz);
    const float S = pqi(Iz - 9.601924202631895e-2f * az - 8.118918960560390e-1f * bz);
    float v[3], d[3];
    v[0] = +1.661373055774069e+00f * L - 9.145230923250668e-01f * M + 2.313620767186147e-01f * S;
    v[1] = -3.250758740427037e-01f * L + 1.571847038366936e+00f * M - 2.182538318672940e-01f * S;
    v[2] = -9.098281098284756e-02f * L - 3.127282905230740e-01f * M + 1.522766561305260e+00f * S;
    mat_vec(D, v, d);
    R = iws[0] * d[0] + iws[1] * d[1] + iws[2] * d[2];
    G = iws[3] * d[0] + iws[4] * d[1] + iws[5] * d[2];
    B = iws[6] * d[0] + iws[7] * d[1] + iws[8] * d[2];
}
// Color::rgb2jzczhz / jzczhz2rgb (color.h:1780-1804) with the tables of a PqTab
__device__ __forceinline__ void rgb2jzczhz(const PqTab pq, float R, float G, float B, float &Jz, float &cz, float &hz, const float *ws)
{
    float az, bz;
    rgb2jzazbz_dev([pq](float x) { return get_pq(pq, x); }, R, G, B, Jz, az, bz, ws);
    cz = sqrtf(bz * bz + az * az);
    hz = xatan2f_s(bz, az);
}
__device__ __forceinline__ void jzczhz2rgb(const float *__restrict__ pqi, float Jz, float cz, float hz, float &R, float &G, float &B, const float *iws)
{
    float sn, cs;
    xsincosf_v(hz, sn, cs);
    const float bz = cz * sn, az = cz * cs;
    jzazbz2rgb_dev([pqi](float x) { return get_pq_inv(pqi, x); }, Jz, az, bz, R, G, B, iws);
}

} // namespace artgpu
