// art_amd/csrc/masks.h -- argument blocks of the region-mask kernels (masks.hip), shared with artgpu_api.hip.
// (reference: rtengine/masks.cc:1037-1516 generateMasks, its parametric path; 696-734 contrast_threshold_mask; 737-802 mask_postprocess;
// 612-636 rgb2lab by image mode)
//
// What the reference computes and never reads is not computed: its lightness-detail plane LL (L1113-1137) exists whenever an L mask is
// asked for, but only a region with a lightness curve reads it (L1230-1231: for every other region `ll` feeds no curve).  Here LL is built
// only when an L mask is asked for AND some region has a lightness curve; the planes are the same bits either way.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace artgpu {

constexpr int MK_GROUP = 4;                 // regions one launch of the fused pass evaluates
constexpr int MK_THREADS = 512;
constexpr int MK_LDS_BYTES = 144 * 1024;    // polylines of one group; a FlatCurve of 1000 polygon points is 24 KB (x, y, dyByDx)

// one FlatCurve's polyline inside the group's table: doubles [off, off + n) = poly_x, [off + n, off + 2n) = poly_y, then n - 1 of dyByDx.
// n == 0: no curve (the factor is 1.f); n < 0: a curve FlatCurve's constructor found to be the identity (getVal returns identityValue, 0.5)
struct MkCurve { int off, n; };
enum { MK_HUE = 0, MK_CHROMA, MK_LIGHT };

struct MkImage { const float *p[3]; size_t stride; int w, h; int lab; };   // lab: Imagefloat::Mode::LAB (L = g, a = r, b = b), else RGB

// L1113-1130: guide = L / 32768.f (not clamped), LL = round(l * 40.f) / 40.f
struct MkLLArgs {
    MkImage im;
    float wp[9]; const float *cachef, *cachefy;
    float *guide, *LL;                      // w * h each
};
// L1171-1241
struct MkFusedArgs {
    MkImage im;
    float wp[9]; const float *cachef, *cachefy;
    float *guide;                           // LIM01(l), w * h
    const float *LL;                        // nullptr: ll = l (L1230)
    const double *tab; int tab_len;         // the group's polylines, tab_len doubles (<= MK_LDS_BYTES / 8)
    int nreg;                               // 0: only the guide is written (no region has a mask)
    MkCurve curve[MK_GROUP][3];
    float ldetail[MK_GROUP];
    float *out[MK_GROUP];                   // blend, w * h
};
// everything pointwise behind the guided blur, in the reference's order; every step is optional:
//   fill (L1302) | LIM01 (L1274-1294) -> * threshold plane or * (1.f - it) (L1365-1375) -> * area (L1384-1392) -> posterize (L747-759)
//   -> [thr_out = m > 1e-4f ? 1.f : fillval (L785-789)] -> [* thr_in (L794-798)] -> 1.f - m (L1438-1451) -> * opacity (L1453-1467)
struct MkTailArgs {
    float *m; int w, h;                     // the plane, rows of w floats, in place
    int fill_one, clamp;
    const float *cthr; int cthr_neg;        // contrast_threshold_mask's plane (rows of w floats)
    const float *area; size_t area_stride;
    float post_p;                           // 0.f: no posterization
    float *thr_out; float fillval;
    const float *thr_in;
    int inverted, has_opacity; float opacity;
};

hipError_t launch_mk_ll(const MkLLArgs &a, hipStream_t s);
hipError_t launch_mk_fused(const MkFusedArgs &a, hipStream_t s);
hipError_t launch_mk_tail(const MkTailArgs &a, hipStream_t s);
// launch_blend_mask (dualdemosaic.hip) with buildBlendMask's luminance_factor: contrast_threshold_mask passes 32768.f (L727)
struct DualArgs;
hipError_t launch_blend_mask_lum(const DualArgs &a, float lum_factor, hipStream_t s);
// rescaleBilinear (rescale.h:53-74) between contiguous planes
hipError_t launch_mk_rescale(const float *src, int sw, int sh, float *dst, int dw, int dh, hipStream_t s);

} // namespace artgpu
