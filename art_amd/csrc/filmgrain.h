// art_amd/csrc/filmgrain.h -- argument block and launch geometry of the film grain kernel (filmgrain.hip), shared with the C-ABI host code.
// ImProcFunctions::filmGrain (rtengine/ipgrain.cc:33-98) = guidedSmoothing's NOISE regions (rtengine/ipsmoothing.cc:565-695 add_noise,
// :933-1067 the frame around it), the generator of rtengine/rng.h:31-57.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace artgpu {

constexpr int FG_NORMD = 5233;              // normd_size (ipsmoothing.cc:600)
constexpr int FG_MAX_R = 3;                 // sz = 2 * r + 1 <= 7: scale >= 1 keeps radius <= 2.25
constexpr int FG_MAX_TAPS = (2 * FG_MAX_R + 1) * (2 * FG_MAX_R + 1);
constexpr int FG_TAB_FLOATS = FG_NORMD + FG_MAX_TAPS;      // one region's device table: normd, the sz * sz normalised taps, then an FgJump
// A workgroup of 256 lanes owns FG_TILE_W x FG_TILE_H pixels of the working area; a lane updates FG_PX pixels of one row, and fills runs of
// FG_RUN noise values of one row of the (FG_TILE_W + 2r) x (FG_TILE_H + 2r) tile: one jump-ahead, then one step per pixel
constexpr int FG_TILE_W = 64, FG_TILE_H = 16, FG_PX = 4, FG_RUN = 7;
constexpr int FG_LDS_STRIDE = 71;           // floats per tile row (>= FG_TILE_W + 2 * FG_MAX_R): 71 mod 64 = 7 puts the four rows a wave reads on disjoint banks
constexpr int FG_JUMP_BITS = 48;            // maps the host derives
constexpr int FG_JUMP_USED = 33;            // ... and the kernels hold in LDS: a draw number is below 2^32, so at most 2^32 steps
// LDS of the region kernel: (FG_NORMD + FG_MAX_TAPS + (FG_TILE_H + 2 * FG_MAX_R) * FG_LDS_STRIDE) * 4 + FG_JUMP_USED * 16 = 27904 bytes, 27944 as laid out
constexpr uint64_t FG_MASK48 = (1ULL << 48) - 1;
constexpr uint64_t FG_LCG_A = 25214903917ULL, FG_LCG_C = 11ULL;      // rng.h:53-54

// 2^j steps of the generator's low 48 bits as one affine map: s -> A[j] * s + C[j] (mod 2^48)
struct FgJump { uint64_t A[FG_JUMP_BITS], C[FG_JUMP_BITS]; };
constexpr size_t FG_TAB_BYTES = FG_TAB_FLOATS * 4 + sizeof(FgJump);
static_assert((FG_TAB_FLOATS * 4) % 8 == 0, "the jump maps behind the floats are 64-bit words");

struct FgArgs {
    const float *src[3]; size_t src_stride;     // what the region reads, at the working area's first pixel (rows of src_stride floats)
    float *dst[3]; size_t dst_stride;           // where the blended result goes (never the planes it reads: a workgroup reads its neighbours' pixels)
    const float *mask; size_t mask_stride;      // blend plane at the working area's first pixel, or nullptr = all ones
    const float *tab;                           // FG_TAB_BYTES: see FG_TAB_FLOATS
    double ws1[3];                              // working-space matrix row 1 (TMatrix, double)
    uint64_t state;                             // the generator's low 48 bits after the table's construction
    float sf, c;                                // ipsmoothing.cc:572, :612
    int ww, hh, channel, r;                     // working area, SM_CH_*, sz / 2
    int norm_in, denorm_out;                    // src is the image before normalizeFloatTo1 / dst is stored * 65535.f
};

hipError_t launch_fg_region(const FgArgs &a, int max_workgroups, hipStream_t s);
hipError_t launch_fg_indices(const float *tab, uint64_t state, uint64_t first, int n, uint32_t *out, hipStream_t s);

// host side (hostluts.hip): the generator stepped serially through NormalDistribution (rng.h:61-90), the cone, the jump table
void build_grain_table(int seed, float *normd /* FG_NORMD */, uint64_t *state48);
int build_grain_kernel(float radius, float *taps /* FG_MAX_TAPS */);       // returns sz, or 0 when sz would exceed 7 or radius is not finite
void build_grain_jump(FgJump *j);

} // namespace artgpu
