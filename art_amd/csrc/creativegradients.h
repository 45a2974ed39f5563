// art_amd/csrc/creativegradients.h -- ImProcFunctions::creativeGradients (rtengine/iptransform.cc:1390-1408): what the kernel file, the
// derivation (hostluts.hip) and the host side (api_creativegradients.hip) share.  One pass of 24 B/px: no LDS, no scratch plane.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace artgpu {

constexpr int CG_LDS_BYTES = 0;            // the kernels declare no LDS (tests/test_creative_resources.py)

// grad_params and pcv_params (iptransform.cc:668-675, 815-825) as the kernel takes them by value: the layout of artgpu_creative_gradient_derived
struct CgDerived {
    int32_t apply_gradient, apply_pcvignette;
    int32_t cx, cy;
    int32_t angle_is_zero, transpose, bright_top, h;
    float ta, yc, xc, ys, ys_inv, scale, botmul, topmul, top_edge_0;
    float oe_a, oe_b, oe1_a, oe1_b, oe2_a, oe2_b, ie_mul, ie1_mul, ie2_mul, sepmix, feather;
    int32_t x1, x2, y1, y2, ex, ey, ew, eh, sep, is_super_ellipse_mode, is_portrait;
    float pcv_scale, fadeout_mul;
};
// what the derivation reads (the fields of artgpu_creative_gradients_params, which this header does not see)
struct CgInput {
    double degree, strength; int feather, center_x, center_y;                            // GradientParams
    double pcv_strength; int pcv_feather, pcv_roundness, pcv_center_x, pcv_center_y;     // PCVignetteParams
    int crop_enabled, crop_x, crop_y, crop_w, crop_h;                                    // CropParams
};

struct CgArgs {
    float *img[3];             // r, g, b planes, in place
    size_t stride;             // floats
    int w, h;
    CgDerived d;
};

void cg_gradient_params(int oW, int oH, const CgInput &in, CgDerived *d);
void cg_pcvignette_params(int fW, int fH, int oW, int oH, const CgInput &in, CgDerived *d);
hipError_t launch_cg(const CgArgs &a, hipStream_t s);

} // namespace artgpu
