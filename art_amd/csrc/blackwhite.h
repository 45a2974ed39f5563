// art_amd/csrc/blackwhite.h -- ImProcFunctions::blackAndWhite (rtengine/ipbw.cc:214-365): what the kernel file, the table builders
// (hostluts.hip) and the host side (api_blackwhite.hip) share.  The kernel is one pass of 24 B/px: no LDS, no scratch plane.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace artgpu {

constexpr int BW_LDS_BYTES = 0;            // the kernels declare no LDS (tests/test_creative_resources.py)

// BlackWhiteParams::setting and ::filter as numbers, in the order of include/artgpu.h (the eleven presets of ipbw.cc:66-78 first)
constexpr int BW_NPRESETS = 11, BW_RGB_REL = 11, BW_RGB_ABS = 12, BW_ROYGCBPM_REL = 13, BW_ROYGCBPM_ABS = 14, BW_NSETTINGS = 15;
constexpr int BW_NFILTERS = 9;             // None, Red, Orange, Yellow, YellowGreen, Green, Cyan, Blue, Purple (ipbw.cc:164-174)

// what computeBWMixerConstants hands back (the layout of artgpu_bw_mixer)
struct BwMixer { float bwr, bwg, bwb, kcorec, filcor; double rrm, ggm, bbm; };

struct BwArgs {
    float *img[3];             // r, g, b planes, in place
    size_t stride;             // floats
    int w, h;
    float bwr, bwg, bwb, kcorec;
    const float *gamma[3];     // hasgammabw: three 65536-entry tables; else null
    const float *ulut, *vlut;  // the colour cast's tables (65536 entries each); null without a cast
    float ws1[3];              // the cast: row 1 of the working-space matrix as floats (Imagefloat::ws_[1], the Y of setMode(YUV))
    int to_rgb;                // the cast: 1 = the image leaves in RGB mode (the stand-alone call), 0 = in YUV mode as the reference leaves it
};

void bw_mixer_constants(int setting, int filter, float mixerRed, float mixerGreen, float mixerBlue, BwMixer *out);
float bw_gamma_of(int gam);
void build_bw_gamma_table(float gamma, float *lut65536);
hipError_t launch_bw(const BwArgs &a, hipStream_t s);

} // namespace artgpu
