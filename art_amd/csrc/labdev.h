// art_amd/csrc/labdev.h -- Color::rgb2lab of one pixel on the device, shared by denoise.hip (LAB colour space of RGB_denoise) and masks.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "devsleef.h"

namespace artgpu {

// Color::computeXYZ2Lab (color.cc:1247-1259)
__device__ __forceinline__ float xyz2lab_f(const float *__restrict__ cachef, float f)
{
    if (f != f) return f;
    if (f < 0.f) return (float)(327.68 * (((24389.0 / 27.0) * (double)f / (double)65535.f + 16.0) / 116.0));
    if (f > 65535.f) return 327.68f * xcbrtf_s(f / 65535.f);
    return lutf_lookup<false>(cachef, 65536, f);
}
// Color::rgb2lab with a float matrix = rgbxyz + XYZ2Lab (color.h:630-636, color.cc:1262-1275,1382-1397)
__device__ __forceinline__ void rgb2lab_px(const float *wpi, const float *__restrict__ cachef, const float *__restrict__ cachefy, float R, float G, float B,
                                           float &l, float &la, float &lb)
{
    const float X = wpi[0] * R + wpi[1] * G + wpi[2] * B, Y = wpi[3] * R + wpi[4] * G + wpi[5] * B, Z = wpi[6] * R + wpi[7] * G + wpi[8] * B;
    const float x = X / 0.9642f, z = Z / 0.8249f, y = Y;
    const float fx = xyz2lab_f(cachef, x), fy = xyz2lab_f(cachef, y), fz = xyz2lab_f(cachef, z);
    if (y != y) l = y;
    else if (y < 0.f) l = (float)(327.68 * ((24389.0 / 27.0) * (double)y / (double)65535.f));
    else if (y > 65535.f) l = 327.68f * (116.f * xcbrtf_s(y / 65535.f) - 16.f);
    else l = lutf_lookup<false>(cachefy, 65536, y);
    la = 500.0f * (fx - fy);
    lb = 200.0f * (fy - fz);
}

} // namespace artgpu
