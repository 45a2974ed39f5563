// art_amd/csrc/impulse.h -- argument block of the impulse noise reduction's correction kernel (impulse.hip), shared with api_impulse.hip.
// (reference: rtengine/impulse_denoise.cc:33-189; markImpulse itself is sharpen.hip's launch_sh_impulse)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace artgpu {

// the correction's tile: IMP_TILE_W x IMP_TILE_H pixels per 256-thread workgroup, the impulse map of the tile and a halo of 2 in LDS
constexpr int IMP_TILE_W = 64, IMP_TILE_H = 16, IMP_HALO = 2;
constexpr int IMP_LDS_BYTES = (IMP_TILE_H + 2 * IMP_HALO) * (IMP_TILE_W + 2 * IMP_HALO) + IMP_TILE_W * IMP_TILE_H * 2 + 17 * 4;

// an image in LAB mode (rows of `stride` floats; L = the g plane, a = r, b = b) and markImpulse's map (rows of W bytes)
struct ImpArgs { float *L, *a, *b; size_t stride; const unsigned char *impish; int W, H; };
// impulse_nr's loop behind markImpulse (impulse_denoise.cc:84-168), in place, one launch
hipError_t launch_imp_correct(const ImpArgs &a, hipStream_t s);

} // namespace artgpu
