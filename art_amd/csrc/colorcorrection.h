// art_amd/csrc/colorcorrection.h -- argument block of the colour-correction kernel (colorcorrection.hip) and the tool's host-side derivation,
// shared with artgpu_api.hip.  (reference: rtengine/ipcolorcorrection.cc:39-866; color.cc:385-429, 456-473, 511-534, 6691-6742)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace artgpu {

constexpr int CC_MAX_REGIONS = 4;          // regions per launch: the tool is in place, a longer list is further launches

// what L280-414 derive for one region, in the reference's types (float; the flags are its char / bool arrays)
struct CcRegion {
    float slope[3], offset[3], power[3], pivot[3];     // rslope, roffset, rpower (1.0 / power), rpivot
    float comp[3][2];                                  // rcompression
    float abca, abcb, rs, rsout, rhs;
    float gamma, igamma;                               // hslgamma and 1.f / hslgamma
    int32_t enabled, rgbmode, jzazbz, hsl;
    const float *lmask, *abmask;                       // Lmask / abmask planes (rows of l_stride / ab_stride floats); nullptr: all ones
    size_t l_stride, ab_stride;
};
struct CcArgs {
    float *img[3];                         // r, g, b planes = v, Y, u in YUV mode (Imagefloat's layout)
    size_t stride; int w, h;
    int from_yuv, to_rgb;                  // the image is already in YUV mode / leaves in RGB mode
    int nregions;
    float ws[9], iws[9];                   // TMatrix rounded to float once (L94-108)
    float fR, fG, fB;                      // L411-414
    const float *pq, *pq_inv;              // build_pq_luts' tables (Jzazbz regions only)
    float pq_low, pq_inv_low;              // PQ(x) and PQ_inv(x) for x < 0: both clamp to 1e-10f first, a constant (host libm, like the tables)
    unsigned char *oor;                    // w * h flags or nullptr: the pixel took a per-pixel powf (a PQ / PQ_inv argument above 1)
    CcRegion r[CC_MAX_REGIONS];
};
// which code a launch carries (the kernel is instantiated per combination)
enum { CC_NEED_HUE = 1, CC_NEED_JZ = 2, CC_NEED_HSL = 4 };
// what a region needs of the above; and whether one launch can carry `need` (Jzazbz and the HSL hue shift have no common instantiation)
inline int cc_region_need(const CcRegion &r)
{
    int need = r.jzazbz ? CC_NEED_JZ : 0;
    if (r.rhs != 0.f) need |= r.hsl ? (CC_NEED_HUE | CC_NEED_HSL) : CC_NEED_HUE;
    return need;
}
inline bool cc_need_fits(int need) { return !((need & CC_NEED_JZ) && (need & CC_NEED_HSL)); }

hipError_t launch_cc(const CcArgs &a, int need, hipStream_t s);
hipError_t launch_cc_count(const unsigned char *oor, size_t n, unsigned long long *count, hipStream_t s);   // *count += set flags

// one ColorCorrectionParams::Region as the host derivation reads it
struct CcRegionParams {
    int mode;                  // 0 YUV, 1 RGB, 2 HSL, 3 JZAZBZ (ARTGPU_CC_*)
    int rgbluminance;
    double a, b, in_saturation, out_saturation, hueshift, hsl_gamma;
    double slope[3], offset[3], power[3], pivot[3], compression[3];
    double hue[3], sat[3], factor[3];
};
// L88-141 and L280-368 for one region; ws is the float working-space matrix.  Masks and strides are left alone.
void cc_derive_region(const CcRegionParams &p, const float ws[9], CcRegion *out);
// every derived scalar is finite
bool cc_region_finite(const CcRegion &r);
// L411-414
void cc_luminance_factors(const float ws[9], float *fR, float *fG, float *fB);
// PQ / PQ_inv below 0 (color.cc:67-84 with X = 1e-10f)
void cc_pq_low(float *pq_low, float *pq_inv_low);

} // namespace artgpu
