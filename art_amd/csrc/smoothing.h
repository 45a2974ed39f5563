// art_amd/csrc/smoothing.h -- argument blocks of the Smoothing tool's own passes (smoothing.hip), shared with the C-ABI host code.
// ImProcFunctions::guidedSmoothing (rtengine/ipsmoothing.cc:902-1073), modes GUIDED and NLMEANS.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace artgpu {

constexpr int SM_MAX_BOX_REGIONS = 64;      // mask planes one box-reduction launch takes
enum { SM_CH_L = 0, SM_CH_C = 1, SM_CH_LC = 2 };   // ipsmoothing.cc:327-331 (SmoothingParams::Region::Channel's order)

// find_region (L411-434) of up to SM_MAX_BOX_REGIONS mask planes in one launch: box[4 * k ..] = {min_x, min_y, max_x, max_y}, inclusive,
// initialised by the kernel's caller to {W, H, -1, -1}
struct SmBoxArgs {
    const float *mask[SM_MAX_BOX_REGIONS];
    size_t stride[SM_MAX_BOX_REGIONS];
    int *box;
    int W, H, n;
};

// one region's working set.  The working planes are ww x hh, contiguous; the image and the mask are addressed at the box's offset
struct SmArgs {
    float *img[3]; size_t stride;           // the normalised image (rows of `stride` floats), already offset to the box's first pixel
    const float *mask; size_t mask_stride;  // blend plane at the box's first pixel, or nullptr = all ones
    const float *src[3]; size_t src_stride; // what this iteration reads: the image (first iteration) or `work`
    float *work[3];                         // what an iteration that is not the last writes; NLMEANS: the planes the filter runs on
    float *in[3];                           // GUIDED L / C: the iteration's input, kept for the recombination; NLMEANS L / C: in[0] = iY
    float *guide;                           // GUIDED L / C: xlin2log(max(Y, 0), 10)
    float *chan[3];                         // GUIDED: xlin2log(max(channel, 0), 10)
    float *a[3], *b[3];                     // GUIDED: mean a / mean b on the w x h grid
    float *low;                             // GUIDED LC: 6 grid planes {I1, I1 * I1} per channel -> {mean I, corr I} -> {a, b}
    double ws1[3];                          // working-space matrix row 1 (TMatrix, double)
    float epsilon;
    int ww, hh, w, h;                       // working size, statistics grid
    int channel, last;
    int src_norm;                           // GUIDED prepare: `src` is the image before normalizeFloatTo1 (the first iteration of a region that fuses it)
    int img_norm, out_denorm;               // the passes that read / blend into the image: it is not normalised yet / is stored * 65535.f
};

hipError_t launch_sm_box(const SmBoxArgs &a, hipStream_t s);
hipError_t launch_sm_scale(float *const img[3], size_t stride, int W, int H, int mode, hipStream_t s);   // 0: * (1 / 65535); 1: * 65535; 2: both
hipError_t launch_sm_prepare(const SmArgs &a, hipStream_t s);
hipError_t launch_sm_subsample_self(const SmArgs &a, hipStream_t s);
hipError_t launch_sm_ab_self(const SmArgs &a, hipStream_t s);
hipError_t launch_sm_finish(const SmArgs &a, hipStream_t s);
hipError_t launch_sm_nlm_split(const SmArgs &a, hipStream_t s);
hipError_t launch_sm_nlm_merge(const SmArgs &a, hipStream_t s);

} // namespace artgpu
