// art_amd/csrc/dehaze.h -- argument blocks of the dehaze kernels (dehaze.hip) and the tool's host routines, shared with artgpu_api.hip.
// (reference: rtengine/ipdehaze.cc:64-512; guidedfilter.cc:58-241 for the statistics grid of the guided filters)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace artgpu {

// what the call keeps on the device between its kernels (normalize L64-80, subtract_black L259-285)
struct DhState {
    float inv_maxval;      // 1.f / maxval: Imagefloat::multiply's factor
    float maxval;          // max(2 * max(r, g, b), 65535)
    float black[3];        // max(0, min(blurred thumbnail) * percent / 100); zeros without a black point
    float pad[3];
};
struct DhImage { float *p[3]; size_t stride; int W, H; };      // Imagefloat planes, rows of `stride` floats
// the statistics grid of rtengine::guidedFilter: planes of w * h floats at low + k * nl
//   three self-guided filters (extract_channels): plane 2c = I1 -> meanI -> mean a, plane 2c + 1 = I1 * I1 -> corrI -> mean b
//   one filter with its own source: 0 = I1 -> meanI, 1 = I1 * I1 -> corrI, 2 = p1 -> meanp -> mean a, 3 = I1 * p1 -> corrIp -> mean b
struct DhGuided { float *low; size_t nl; int w, h; float eps; };
struct DhThumbArgs {
    DhImage im; const DhState *st; DhGuided gf;
    float *thumb; int ww, hh;          // three planes of ww * hh floats
    int from_q;                        // 0: the normalised image (subtract_black); 1: the guided filters' output (L379-381)
};
struct DhDarkArgs {
    DhImage im; DhGuided gf;           // FROMQ: q_c = bilinear(mean a_c) * im_c + bilinear(mean b_c), never stored
    float *grid;                       // one value per patch, rows of npx
    int patch, npx, npy;
    int has_ambient, per_pixel, clip;  // per_pixel: a non-positive ambient component, the division stays inside the minimum
    float ambient[3];
};
struct DhExpandArgs { const float *grid; int patch, npx; float *dst; size_t dst_stride; int W, H; };
struct DhTransArgs {
    DhImage im; const DhState *st;
    const float *grid; int patch, npx;
    const float *lut;                  // strength, 65536 entries
    double ws1[3];
    float *t;                          // W * H
};
struct DhRecoverArgs {
    DhImage im; const DhState *st; DhGuided gf;
    const float *lut; double ws1[3];
    float ambient[3], ambientY, t0;
    int show_depth_map, luminance;
};

// (shared with textureboost.hip, whose guided filters end the same way)
// getBilinearValue (rescale.h:27-50) on a plane with rows of `stride` floats
__device__ __forceinline__ float dh_bilinear(const float *__restrict__ src, size_t stride, int W, int H, float x, float y)
{
    const int xi = min((int)x, W - 1), yi = min((int)y, H - 1);
    const float xf = x - xi, yf = y - yi;
    const int xi1 = min(xi + 1, W - 1), yi1 = min(yi + 1, H - 1);
    const float bl = src[(size_t)yi * stride + xi], br = src[(size_t)yi * stride + xi1];
    const float tl = src[(size_t)yi1 * stride + xi], tr = src[(size_t)yi1 * stride + xi1];
    const float b = xf * br + (1.f - xf) * bl;
    const float t = xf * tr + (1.f - xf) * tl;
    return yf * t + (1.f - yf) * b;
}

// q = rescaleBilinear(mean a) * I + rescaleBilinear(mean b) at (y, x) (guidedfilter.cc:225-240)
__device__ __forceinline__ float dh_q(const float *__restrict__ ma, const float *__restrict__ mb, int w, int h, float col_scale, float ymrs, int x, float I)
{
    const float fx = x * col_scale;
    return dh_bilinear(ma, w, w, h, fx, ymrs) * I + dh_bilinear(mb, w, w, h, fx, ymrs);
}

hipError_t launch_dh_max(const DhImage &im, float *partial, int npartial, DhState *st, hipStream_t s);
hipError_t launch_dh_thumb(const DhThumbArgs &a, hipStream_t s);
hipError_t launch_dh_black(const float *thumb, int n, float scaling, DhState *st, hipStream_t s);
hipError_t launch_dh_normalize(const DhImage &im, const DhState *st, int has_black, hipStream_t s);
hipError_t launch_dh_restore(const DhImage &im, const DhState *st, hipStream_t s);
hipError_t launch_dh_gf_subsample(const DhImage &im, const float *src, size_t src_stride, const DhGuided &gf, hipStream_t s);   // src == nullptr: the three self-guided filters
hipError_t launch_dh_gf_ab(const DhGuided &gf, int self3, hipStream_t s);
hipError_t launch_dh_dark(const DhDarkArgs &a, bool from_q, hipStream_t s);
hipError_t launch_dh_expand(const DhExpandArgs &a, hipStream_t s);
hipError_t launch_dh_transmission(const DhTransArgs &a, hipStream_t s);
hipError_t launch_dh_recover(const DhRecoverArgs &a, hipStream_t s);
constexpr int DH_MAX_PARTIALS = 1024;
constexpr int DH_MAX_PATCH = 256;

// host side
void dh_thumb_size(int W, int H, int *ww, int *hh);                                      // L254-257 / L372-375
void dh_strength_lut(const double *pts, int npts, float lut[65536]);                      // L419-424
float dh_estimate_ambient(const float *R, const float *G, const float *B, int ww, int hh, float ambient[3]);   // L385-386

} // namespace artgpu
