// art_amd/csrc/filmsim.h -- argument block of the film simulation pass (filmsim.hip), shared with the C-ABI host code (api_filmsim.hip).
// CLUTApplication's HaldCLUT path (rtengine/clutstore.cc:1063-1112, 1464-1484, 1502-1615) over HaldCLUT::getRGB (clutstore.cc:178-288).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace artgpu {

enum { FS_WORK2XYZ = 0, FS_XYZ2CLUT, FS_CLUT2XYZ, FS_XYZ2WORK };

struct FsArgs {
    float *img[3]; size_t stride;          // R, G, B in place (rows of `stride` floats)
    int W, H;
    const float *gam, *igam;               // Color::gamma2curve's and Color::igammatab_srgb's 65536 values (device; read through L2)
    const unsigned short *clut;            // level^3 RGBX entries, red fastest, and one padding entry (device; 8-byte aligned)
    unsigned level;                        // entries per axis
    float flm1, flm2;                      // float(level - 1) / 65535.0f, float(level - 2)
    float strength;
    float mf[4][9];                        // FS_*: the matrices rounded to float (the 4-wide body); read only without SAME_PROFILE
    double md[4][9];                       // ... and as they came (the scalar tail)
};

hipError_t launch_filmsim(const FsArgs &a, bool same_profile, hipStream_t s);

} // namespace artgpu
