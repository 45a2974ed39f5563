// art_amd/csrc/defringe.h -- argument blocks of the defringe kernels (defringe.hip), shared with api_defringe.hip.
// (reference: rtengine/PF_correct_RT.cc:44-218; gauss.cc:129-174 gauss3x3, 1444-1475)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace artgpu {

// which blur gaussianBlur(src != dst, GAUSS_STANDARD) runs for the radius; the values are ARTGPU_DEFRINGE_BLUR_*
enum { DF_BLUR_COPY = 0, DF_BLUR_3X3 = 1, DF_BLUR_YVV = 2 };

// The averaging kernel's tile: DF_TILE x DF_TILE pixels per 256-thread workgroup, with a halo of halfwin - 1 <= DF_MAX_HALO on every side.
// wt, a and b of tile + halo sit in LDS, with the list of the tile's flagged pixels and the waves' counts:
//   3 * (32 + 20)^2 * 4 + 1024 * 2 + 17 * 4 = 34564 bytes, four workgroups per CU (160 KB).
constexpr int DF_TILE = 32, DF_MAX_HALO = 10, DF_MAX_HALFWIN = DF_MAX_HALO + 1;
constexpr int DF_SIDE = DF_TILE + 2 * DF_MAX_HALO;
constexpr int DF_LDS_BYTES = 3 * DF_SIDE * DF_SIDE * 4 + DF_TILE * DF_TILE * 2 + 17 * 4;
constexpr int DF_CURVE_LDS_BYTES = 64 * 1024;      // df_chroma_kernel: the hue curve's polyline (x, y, dyByDx as doubles)
constexpr int DF_CHUNK = 4096;                     // pixels behind one partial of chromave: the unit of the sum's fixed order (LC_CHUNK's rule)

// what the tool keeps on the device between its kernels: nothing of it travels through the host unless `info` is asked for
struct DfState {
    double chromave;               // sum / (H * W)
    float threshfactor;
    int run;                       // chromave > 0.0
    unsigned long long corrected;  // pixels with wt < threshfactor
};

struct DfImage { float *a, *b; size_t stride; int W, H; };      // the LAB image's r and b planes, rows of `stride` floats

// gauss3x3<float> (gauss.cc:129-174): dst (rows of W floats) from src (rows of `stride` floats)
hipError_t launch_df_gauss3x3(const float *src, size_t stride, float *dst, int W, int H, float c0, float c1, float c2, float b0, float b1, hipStream_t s);

// L73-114: chroma of every pixel into `fringe`, one double partial per DF_CHUNK pixels into `partial`
struct DfChromaArgs {
    DfImage im;
    const float *tmpa, *tmpb;      // the blurred planes, rows of W floats
    float *fringe;                 // W * H
    double *partial;               // ceil(W * H / DF_CHUNK)
    const double *curve; int n;    // the hue curve's polyline: poly_x[n], poly_y[n], dyByDx[n - 1]; n == 0: no curve; n < 0: FCT_Empty (getVal = 0.5)
};
hipError_t launch_df_chroma(const DfChromaArgs &a, hipStream_t s);
// L117-129: the partials in their fixed order, chromave, threshfactor, run; zeroes the count
hipError_t launch_df_finish(const double *partial, int npartial, int W, int H, int thresh, DfState *st, hipStream_t s);
// L142-203 with every window reading the tool's input a and b: the new values of the flagged pixels go to newa / newb (the dead blurred planes)
struct DfAverageArgs {
    DfImage im;
    const float *fringe;           // chroma (wt is derived from it while a tile is loaded)
    float *newa, *newb;            // rows of W floats
    int halfwin;
    DfState *st;
};
hipError_t launch_df_average(const DfAverageArgs &a, hipStream_t s);
// ... and from there into the image, behind the averaging kernel
hipError_t launch_df_scatter(const DfAverageArgs &a, hipStream_t s);

} // namespace artgpu
