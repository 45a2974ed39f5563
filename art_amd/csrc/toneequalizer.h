// art_amd/csrc/toneequalizer.h -- argument block of the tone equalizer's own passes (toneequalizer.hip), shared with the C-ABI host code.
// ImProcFunctions::toneEqualizer / tone_eq (rtengine/iptoneequalizer.cc:69-371).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace artgpu {

enum { TE_PREP_Y = 0, TE_PREP_LOG = 1, TE_PREP_POSTERISE = 2 };   // te_prepare: Y; xlin2log(max(Y, 0), 10); Y2 = Y and the posterised Y

struct TeArgs {
    float *img[3]; size_t stride;          // R, G, B in place (rows of `stride` floats)
    int W, H;
    float *Y, *Y2;                         // W x H, contiguous
    const float *lut;                      // the 65536-entry correction table (device; read through L2)
    const float *ma, *mb;                  // te_detail_finish, te_apply with `upsample`: mean a / mean b on the w x h statistics grid
    int w, h;
    double ws1[3];                         // working-space matrix row 1 (TMatrix, double)
    float gain, igain;                     // 1.f / 65535.f * 2^-pivot narrowed to float; 1.f / gain
    float w_sum, factors[12];
    int mode;                              // te_prepare: TE_PREP_*; te_detail_finish: != 0 also writes Y2 and the posterised Y
    int upsample;                          // te_apply: Y is not read but made from Y2 and ma / mb on the w x h grid (the last regularising filter's last pass)
    int group_thread;                      // te_direct / te_apply: 1: one thread per group of four columns; 0: one pixel per lane, the decision by ballot
};

// hostluts.hip: gain, factors, w_sum and (lut != nullptr) the 65536-entry table with the host's scalar sleef forms
void te_build_lut(const int bands[5], double pivot, float *lut, float *gain, float *w_sum, float factors[12]);

hipError_t launch_te_direct(const TeArgs &a, hipStream_t s);          // regularization 0: the whole tool in one pass
hipError_t launch_te_prepare(const TeArgs &a, hipStream_t s);
hipError_t launch_te_detail_finish(const TeArgs &a, hipStream_t s);
hipError_t launch_te_apply(const TeArgs &a, hipStream_t s);

} // namespace artgpu
