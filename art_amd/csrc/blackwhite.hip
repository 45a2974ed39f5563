// art_amd/csrc/blackwhite.hip -- ImProcFunctions::blackAndWhite's pixel loops (rtengine/ipbw.cc:285-315, 346-363), one lane per pixel, in place.
// The reference walks a row in groups of four (x < W - 3) and finishes it one pixel at a time; the two differ in the LUTf lookup they use
// (operator[](vfloat), LUT.h:349-377, against operator[](float), LUT.h:436-459), so columns below W & ~3 take the first and the rest the second.
// The mix is ((bwr * r + bwg * g) + bwb * b) * kcorec in float, unfused (the file is built with -ffp-contract=off), in both.
// The colour cast (L317-364) runs in registers behind the mix: setMode(YUV) (Color::rgb2yuv, color.h:783-788) of a pixel whose three channels
// are the mix, the two lookups on Y with the same body / tail rule, the two additions, and for the stand-alone call Color::yuv2rgb (L791-796).
#include "blackwhite.h"
#include "devmath.h"
#include "devsleef.h"

namespace artgpu {

template <bool GAMMA, bool CAST>
__global__ void __launch_bounds__(256) bw_mix_kernel(BwArgs a)
{
    const int wv = a.w & ~3;
    FOR_IMAGE_XY(y, x, a.w, a.h) {
        const size_t o = (size_t)y * a.stride + x;
        const bool body = x < wv;
        float r = a.img[0][o], g = a.img[1][o], b = a.img[2][o];
        if (GAMMA) {
            if (body) {
                r = lutf_vlookup(a.gamma[0], 65536, r); g = lutf_vlookup(a.gamma[1], 65536, g); b = lutf_vlookup(a.gamma[2], 65536, b);
            } else {
                r = lutf_lookup<true>(a.gamma[0], 65536, r); g = lutf_lookup<true>(a.gamma[1], 65536, g); b = lutf_lookup<true>(a.gamma[2], 65536, b);
            }
        }
        const float bw = (a.bwr * r + a.bwg * g + a.bwb * b) * a.kcorec;
        if (!CAST) {
            a.img[0][o] = bw; a.img[1][o] = bw; a.img[2][o] = bw;
            continue;
        }
        const float Y = bw * a.ws1[0] + bw * a.ws1[1] + bw * a.ws1[2];         // rgbLuminance
        float u = Y - bw, v = bw - Y;
        u = u + (body ? lutf_vlookup(a.ulut, 65536, Y) : lutf_lookup<true>(a.ulut, 65536, Y));
        v = v + (body ? lutf_vlookup(a.vlut, 65536, Y) : lutf_lookup<true>(a.vlut, 65536, Y));
        if (!a.to_rgb) {
            a.img[0][o] = v; a.img[1][o] = Y; a.img[2][o] = u;
            continue;
        }
        const float bo = Y - u, ro = v + Y;
        a.img[0][o] = ro; a.img[1][o] = (Y - ro * a.ws1[0] - bo * a.ws1[2]) / a.ws1[1]; a.img[2][o] = bo;
    }
}

hipError_t launch_bw(const BwArgs &a, hipStream_t s)
{
    const bool gam = a.gamma[0] != nullptr, cast = a.ulut != nullptr;
    const dim3 grid = image_grid(a.w, a.h);
    if (gam && cast) hipLaunchKernelGGL((bw_mix_kernel<true, true>), grid, dim3(256), 0, s, a);
    else if (gam) hipLaunchKernelGGL((bw_mix_kernel<true, false>), grid, dim3(256), 0, s, a);
    else if (cast) hipLaunchKernelGGL((bw_mix_kernel<false, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((bw_mix_kernel<false, false>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace artgpu
