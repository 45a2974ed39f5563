// art_amd/host/artgpu_cli.cc -- command-line counterpart of ART-cli for the hot path
// (reference: rtgui/main-cli.cc:786-903 -> rtengine/simpleprocess.cc:75-420): load a CFA frame,
// run stage_init (demosaic, getImage), stage_denoise (convertColorSpace, denoise), stage_finish
// (process STAGE_1..3) on the GPU through the rtengine-shaped classes of rtengine_gpu.h, write a
// 16-bit PPM.  Input: raw little-endian float32 (values 0..65535) or uint16, W*H samples.
//
//   artgpu-cli --in frame.f32 --width 4000 --height 3000 [--u16] [--filters 0x94949494]
//              [--method amaze|rcd] [--border 4] [--denoise L,C] [--chroma-auto] [--expcomp 0.3] [--out out.ppm]
//              [--dual bilinear|vng4] [--dual-contrast C] [--logenc REG] [--saturation S,V] [--labchroma C]   (SURVEY 8f N4 tools)
//              [--ca auto[,N] | --ca manual,R,B] [--ca-keep-colourshift]   (RawImageSource::CA_correct_RT after the load, before the demosaic)
//              [--local-contrast C[,curve-points]]   (ImProcFunctions::localContrast: one region, contrast C, the default region's curve unless FlatCurve
//                                                      control points follow: kind,x,y,left,right,...)
//              [--dehaze depth[,strength_y[,blackpoint[,luminance]]]]   (ImProcFunctions::dehaze in STAGE_0: strength_y = the y of a flat two-point
//                                                      strength curve, default 0.75)
//              [--sharpen contrast[,radius|auto[,amount[,cornerboost[,latitude]]]]]   (ImProcFunctions::sharpening in STAGE_2, method rld; `auto`
//                                                      (the default) takes the radius from RawImageSource::getDeconvAutoRadius as simpleprocess.cc:274-278 does)
//              [--texture-boost strength,threshold,iterations]   (ImProcFunctions::textureBoost, the first step of STAGE_3: one region, no mask)
//              [--texture-boost-mask lo,hi[,blur[,detail[,threshold[,opacity]]]]]   (a parametric mask on that region, generated on the device by
//                                                      generateMasks: a lightness curve that is 1 between lo and hi and 0 outside, ParametricMask's
//                                                      blur, lightnessDetail, contrastThreshold and Mask::opacity)
//              [--color-correction mode[,key=value...]]   (ImProcFunctions::colorCorrection in STAGE_2 behind the sharpening: one region; mode yuv | rgb |
//                                                      hsl | jzazbz; keys a, b, in_saturation, out_saturation, hueshift, hsl_gamma, rgbluminance and, with one
//                                                      value for all three channels or r:g:b, slope, offset, power, pivot, compression, hue, sat, factor)
//              [--color-correction-mask lo,hi[,blur[,detail[,threshold[,opacity]]]]]   (a parametric mask on that region, in the form of
//                                                      --texture-boost-mask: generateMasks makes its Lmask and abmask on the device)
//              [--smoothing mode,channel,a,b,iterations]   (ImProcFunctions::guidedSmoothing, the last step of STAGE_2: one region; mode guided | nlmeans;
//                                                      channel l | c | lc; a,b = radius,epsilon for guided and nlstrength,nldetail for nlmeans;
//                                                      a value that starts with a digit is the denoiser's --smoothing radius,nlStrength,nlDetail)
//              [--smoothing-mask lo,hi[,blur[,detail[,threshold[,opacity]]]]]   (a parametric mask on that region, in the form of
//                                                      --color-correction-mask: generateMasks makes its Lmask on the device)
//              [--tone-equalizer b0,b1,b2,b3,b4[,regularization[,pivot]]]   (ImProcFunctions::toneEqualizer, the last step of STAGE_1: the five bands
//                                                      -100 .. 100, regularization 0 .. 4 (default 4), pivot in EV (default 0))
//              [--film-simulation file.u16,level[,strength[,after]]]   (ImProcFunctions::filmSimulation in STAGE_3: file.u16 = a HaldCLUT as raw
//                                                      little-endian uint16 RGB triples, level^3 of them with red fastest; level = entries per axis
//                                                      (64 for a level-8 file); strength in percent (default 100); after != 0: behind the tone
//                                                      curve instead of ahead of it.  The CLUT's profile is taken to be the working profile)
//              [--film-grain iso,strength[,color]]   (ImProcFunctions::filmGrain in STAGE_3, behind texture boost: iso 100 .. 6400, strength 0 .. 100,
//                                                      color != 0 adds the chrominance region)
//              [--resize-scale S | --resize-fit WxH]   (the Resize tool behind STAGE_3, simpleprocess.cc:402-414: ImProcFunctions::resizeScale with
//                                                      dataspec 0 (scale S) or 3 (fit the W x H box; never upscales), then ImProcFunctions::resize)
//              [--gradient DEG,FEATHER,STRENGTH,CX,CY] [--vignette STRENGTH,FEATHER,ROUNDNESS,CX,CY]   (ImProcFunctions::creativeGradients, the first step
//                                                      of STAGE_3: the graduated filter's GradientParams and the vignette filter's PCVignetteParams)
//              [--soft-light N]                        (ImProcFunctions::softLight behind the tone curve: strength 0 .. 100)
//              [--bw SETTING[,FILTER[,R,G,B[,GR,GG,GB]]]]   (ImProcFunctions::blackAndWhite, the last step of STAGE_3: SETTING and FILTER by the
//                                                      reference's names (NormalContrast .. InfraRed, RGB-Rel, RGB-Abs, ROYGCBPM-Rel, ROYGCBPM-Abs; None, Red ..
//                                                      Purple), the mixer's and the gamma's red, green and blue)
//   artgpu-cli --batch a.u16,b.u16,... --width W --height H [--lanes N] [--black B] [--method ..] [--denoise L,C] [--expcomp E] [--ca ..] [--dehaze ..] [--sharpen ..]
//              [--tone-equalizer ..] [--film-simulation ..] [--film-grain ..] [--gradient ..] [--vignette ..] [--soft-light ..] [--bw ..] [--resize-scale ..] [--resize-fit ..] [--texture-boost ..] [--texture-boost-mask ..] [--color-correction ..] [--color-correction-mask ..] [--smoothing ..] [--smoothing-mask ..] [--out prefix]
//              the batch queue's loop (simpleprocess.cc:586-612): uint16 sensor frames through scaleColors + the same stages, 16-bit
//              scanlines as the writers take them (getScanline: clip and truncate), written as prefix.K.ppm; artgpu_batch_run_io
#include <cctype>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include "rtengine_gpu.h"

using namespace artgpu_host;

static std::vector<float> default_tone_lut()
{
    // a fixed S-curve (an input of the tone stage; ART builds it from the user's DiagonalCurve, curves.cc:221-231)
    std::vector<float> lut(65536);
    for (int i = 0; i < 65536; ++i) {
        const double x = i / 65535.0;
        lut[i] = (float)((1.0 - std::cos(M_PI * std::pow(x, 0.7))) / 2.0 * 65535.0);
    }
    return lut;
}

int main(int argc, char **argv)
{
    std::string in, out, batch;
    int lanes = 1;
    float black = 0.f;
    int W = 0, H = 0, border = 4, method = ARTGPU_BAYER_AMAZE;
    bool u16 = false;
    uint32_t filters = 0x94949494u;
    double lum = 0, chroma = 0, expcomp = 0;
    bool dn = false, smoothing = false, chroma_auto = false;
    int tone_mode = ARTGPU_TONE_STD;
    int xtrans_passes = 0;   // 0 = Bayer; 1 / 3 = X-Trans ONE_PASS / THREE_PASS with the Fuji colour map
    int gradius = 3, nlstrength = 0, nldetail = 80;
    bool dual = false, dual_auto = true, logenc = false, labcurve = false;
    int dual_second = ARTGPU_DUAL_BILINEAR, logenc_reg = 60, sat = 0, vib = 0, labchroma = 0;
    bool ca_enable = false, ca_auto = true, ca_avoid = true;       // RAWParams: enable_ca, ca_autocorrect, ca_avoidcolourshift
    int ca_iter = 2;                                               // caautoiterations
    double ca_red = 0.0, ca_blue = 0.0;                            // cared, cablue
    double dual_contrast = 20;
    bool lc_enable = false;                                        // LocalContrastParams::enabled, one region
    double lc_contrast = 0;
    std::vector<double> lc_curve;                                  // empty: the default region's curve
    bool dh_enable = false;                                        // DehazeParams::enabled
    int dh_depth = 25, dh_black = 0, dh_lum = 0;
    double dh_y = 0.75;
    bool sh_enable = false, sh_auto = true;                        // SharpeningParams::enabled, deconvAutoRadius
    double sh_contrast = 20.0, sh_radius = 0.75, sh_boost = 0.0;
    int sh_amount = 100, sh_latitude = 25;
    bool tb_enable = false;                                        // TextureBoostParams::enabled, one region
    double tb_strength = 0.0, tb_threshold = 0.2;
    int tb_iterations = 1;
    bool tbm_enable = false;                                       // a parametric Mask on the texture-boost region
    double tbm_lo = 0.0, tbm_hi = 1.0, tbm_blur = 0.0;
    int tbm_detail = 0, tbm_threshold = 0, tbm_opacity = 100;
    bool cc_enable = false;                                        // ColorCorrectionParams::enabled, one region
    ProcParams::ColorCorrectionRegion cc_region;
    bool ccm_enable = false;                                       // a parametric Mask on the colour-correction region
    double ccm_lo = 0.0, ccm_hi = 1.0, ccm_blur = 0.0;
    int ccm_detail = 0, ccm_threshold = 0, ccm_opacity = 100;
    bool sm_enable = false;                                        // SmoothingParams::enabled, one region
    ProcParams::SmoothingRegion sm_region;
    bool smm_enable = false;                                       // a parametric Mask on the smoothing region
    double smm_lo = 0.0, smm_hi = 1.0, smm_blur = 0.0;
    int smm_detail = 0, smm_threshold = 0, smm_opacity = 100;
    bool te_enable = false;                                        // ToneEqualizerParams
    int te_bands[5] = {0, 0, 0, 0, 0}, te_reg = 4;
    double te_pivot = 0.0;
    std::string fs_file;                                           // FilmSimulationParams: the CLUT, strength, after_tone_curve
    int fs_level = 0, fs_strength = 100, fs_after = 0;
    bool fg_enable = false;                                        // GrainParams
    int fg_iso = 400, fg_strength = 50, fg_color = 0;
    bool rs_enable = false;                                        // ResizeParams
    int rs_dataspec = 0, rs_width = 900, rs_height = 900;
    double rs_scale = 1.0;
    bool gr_enable = false, pv_enable = false, sl_enable = false, bw_enable = false;      // GradientParams, PCVignetteParams, SoftLightParams, BlackWhiteParams
    double gr_degree = 0.0, gr_strength = 0.6, pv_strength = 0.6;
    int gr_feather = 25, gr_cx = 0, gr_cy = 0, pv_feather = 50, pv_roundness = 50, pv_cx = 0, pv_cy = 0, sl_strength = 30;
    int bw_setting = ARTGPU_BW_RGB_REL, bw_filter = ARTGPU_BW_FILTER_NONE, bw_mix[3] = {33, 33, 33}, bw_gam[3] = {0, 0, 0};
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char * { if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", a.c_str()); std::exit(2); } return argv[++i]; };
        if (a == "--in") in = next();
        else if (a == "--batch") batch = next();
        else if (a == "--lanes") lanes = std::atoi(next());
        else if (a == "--black") black = (float)std::atof(next());
        else if (a == "--out") out = next();
        else if (a == "--width") W = std::atoi(next());
        else if (a == "--height") H = std::atoi(next());
        else if (a == "--u16") u16 = true;
        else if (a == "--filters") filters = (uint32_t)std::strtoul(next(), nullptr, 0);
        else if (a == "--border") border = std::atoi(next());
        else if (a == "--expcomp") expcomp = std::atof(next());
        else if (a == "--method") { std::string m = next(); method = (m == "rcd") ? ARTGPU_BAYER_RCD : ARTGPU_BAYER_AMAZE; }
        else if (a == "--chroma-auto") { chroma_auto = true; }
        else if (a == "--denoise") { dn = true; if (std::sscanf(next(), "%lf,%lf", &lum, &chroma) != 2) { std::fprintf(stderr, "--denoise L,C\n"); return 2; } }
        else if (a == "--xtrans") { xtrans_passes = std::atoi(next()); border = 7; }
        else if (a == "--tone") { std::string m = next(); tone_mode = (m == "neutral") ? ARTGPU_TONE_NEUTRAL : ARTGPU_TONE_STD; }
        // (a value that starts with a digit is the denoiser's smoothing; one that starts with a mode's name is the Smoothing tool, further down)
        else if (a == "--smoothing" && i + 1 < argc && !std::isalpha((unsigned char)argv[i + 1][0])) { smoothing = true; if (std::sscanf(next(), "%d,%d,%d", &gradius, &nlstrength, &nldetail) != 3) { std::fprintf(stderr, "--smoothing radius,nlStrength,nlDetail\n"); return 2; } }
        else if (a == "--dual") { std::string m = next(); dual = true; dual_second = (m == "vng4") ? ARTGPU_DUAL_VNG4 : ARTGPU_DUAL_BILINEAR; }
        else if (a == "--dual-contrast") { dual_contrast = std::atof(next()); dual_auto = false; }
        else if (a == "--logenc") { logenc = true; logenc_reg = std::atoi(next()); }
        else if (a == "--saturation") { if (std::sscanf(next(), "%d,%d", &sat, &vib) != 2) { std::fprintf(stderr, "--saturation S,V\n"); return 2; } }
        else if (a == "--labchroma") { labchroma = std::atoi(next()); labcurve = true; }
        else if (a == "--ca") {
            const std::string m = next();
            ca_enable = true;
            if (m == "auto" || m.rfind("auto,", 0) == 0) { ca_auto = true; if (m.size() > 5) ca_iter = std::atoi(m.c_str() + 5); }
            else if (std::sscanf(m.c_str(), "manual,%lf,%lf", &ca_red, &ca_blue) == 2) ca_auto = false;
            else { std::fprintf(stderr, "--ca auto[,N] | --ca manual,R,B\n"); return 2; }
        }
        else if (a == "--ca-keep-colourshift") ca_avoid = false;
        else if (a == "--local-contrast") {
            const char *v = next();
            char *end = nullptr;
            lc_contrast = std::strtod(v, &end);
            if (end == v) { std::fprintf(stderr, "--local-contrast C[,curve-points]\n"); return 2; }
            lc_enable = true;
            while (*end == ',') {
                const char *q = end + 1;
                const double x = std::strtod(q, &end);
                if (end == q) { std::fprintf(stderr, "--local-contrast C[,curve-points]\n"); return 2; }
                lc_curve.push_back(x);
            }
        }
        else if (a == "--dehaze") {
            if (std::sscanf(next(), "%d,%lf,%d,%d", &dh_depth, &dh_y, &dh_black, &dh_lum) < 1) { std::fprintf(stderr, "--dehaze depth[,strength_y[,blackpoint[,luminance]]]\n"); return 2; }
            dh_enable = true;
        }
        else if (a == "--sharpen") {
            // contrast[,radius|auto[,amount[,cornerboost[,latitude]]]]
            std::vector<std::string> f;
            const std::string v = next();
            for (size_t pos = 0;;) { const size_t e = v.find(',', pos); f.push_back(v.substr(pos, e == std::string::npos ? std::string::npos : e - pos)); if (e == std::string::npos) break; pos = e + 1; }
            char *end = nullptr;
            sh_contrast = std::strtod(f[0].c_str(), &end);
            if (end == f[0].c_str() || f.size() > 5) { std::fprintf(stderr, "--sharpen contrast[,radius|auto[,amount[,cornerboost[,latitude]]]]\n"); return 2; }
            if (f.size() > 1 && f[1] != "auto") { sh_auto = false; sh_radius = std::atof(f[1].c_str()); }
            if (f.size() > 2) sh_amount = std::atoi(f[2].c_str());
            if (f.size() > 3) sh_boost = std::atof(f[3].c_str());
            if (f.size() > 4) sh_latitude = std::atoi(f[4].c_str());
            sh_enable = true;
        }
        else if (a == "--texture-boost") {
            if (std::sscanf(next(), "%lf,%lf,%d", &tb_strength, &tb_threshold, &tb_iterations) != 3) { std::fprintf(stderr, "--texture-boost strength,threshold,iterations\n"); return 2; }
            tb_enable = true;
        }
        else if (a == "--texture-boost-mask") {
            if (std::sscanf(next(), "%lf,%lf,%lf,%d,%d,%d", &tbm_lo, &tbm_hi, &tbm_blur, &tbm_detail, &tbm_threshold, &tbm_opacity) < 2) {
                std::fprintf(stderr, "--texture-boost-mask lo,hi[,blur[,detail[,threshold[,opacity]]]]\n"); return 2;
            }
            tbm_enable = true;
        }
        else if (a == "--color-correction") {
            std::vector<std::string> f;
            const std::string v = next();
            for (size_t pos = 0; pos <= v.size();) {
                const size_t e = v.find(',', pos);
                f.push_back(v.substr(pos, e == std::string::npos ? std::string::npos : e - pos));
                if (e == std::string::npos) break;
                pos = e + 1;
            }
            const char *usage = "--color-correction yuv|rgb|hsl|jzazbz[,key=value...] (a triple as r:g:b or one value)\n";
            if (f[0] == "yuv") cc_region.mode = ARTGPU_CC_YUV;
            else if (f[0] == "rgb") cc_region.mode = ARTGPU_CC_RGB;
            else if (f[0] == "hsl") cc_region.mode = ARTGPU_CC_HSL;
            else if (f[0] == "jzazbz") cc_region.mode = ARTGPU_CC_JZAZBZ;
            else { std::fprintf(stderr, "%s", usage); return 2; }
            for (size_t k = 1; k < f.size(); ++k) {
                const size_t eq = f[k].find('=');
                if (eq == std::string::npos) { std::fprintf(stderr, "%s", usage); return 2; }
                const std::string key = f[k].substr(0, eq), val = f[k].substr(eq + 1);
                double t[3];
                const int nt = std::sscanf(val.c_str(), "%lf:%lf:%lf", &t[0], &t[1], &t[2]);
                if (nt == 1) t[1] = t[2] = t[0];
                double *scalar = key == "a" ? &cc_region.a : key == "b" ? &cc_region.b : key == "in_saturation" ? &cc_region.inSaturation :
                                 key == "out_saturation" ? &cc_region.outSaturation : key == "hueshift" ? &cc_region.hueshift :
                                 key == "hsl_gamma" ? &cc_region.hsl_gamma : nullptr;
                double *triple = key == "slope" ? cc_region.slope : key == "offset" ? cc_region.offset : key == "power" ? cc_region.power :
                                 key == "pivot" ? cc_region.pivot : key == "compression" ? cc_region.compression : key == "hue" ? cc_region.hue :
                                 key == "sat" ? cc_region.sat : key == "factor" ? cc_region.factor : nullptr;
                if (scalar && nt == 1) *scalar = t[0];
                else if (triple && (nt == 1 || nt == 3)) { triple[0] = t[0]; triple[1] = t[1]; triple[2] = t[2]; }
                else if (key == "rgbluminance" && nt == 1) cc_region.rgbluminance = t[0] != 0;
                else { std::fprintf(stderr, "%s", usage); return 2; }
            }
            cc_enable = true;
        }
        else if (a == "--color-correction-mask") {
            if (std::sscanf(next(), "%lf,%lf,%lf,%d,%d,%d", &ccm_lo, &ccm_hi, &ccm_blur, &ccm_detail, &ccm_threshold, &ccm_opacity) < 2) {
                std::fprintf(stderr, "--color-correction-mask lo,hi[,blur[,detail[,threshold[,opacity]]]]\n"); return 2;
            }
            ccm_enable = true;
        }
        else if (a == "--smoothing") {
            char mode[16] = {0}, channel[8] = {0};
            int va = 0, vb = 0, it = 1;
            const char *usage = "--smoothing guided|nlmeans,l|c|lc,a,b,iterations (a,b: radius,epsilon or nlstrength,nldetail)\n";
            if (std::sscanf(next(), "%15[a-z],%7[a-z],%d,%d,%d", mode, channel, &va, &vb, &it) != 5) { std::fprintf(stderr, "%s", usage); return 2; }
            const std::string m = mode, c = channel;
            if (m == "guided") { sm_region.mode = ARTGPU_SMOOTHING_GUIDED; sm_region.radius = va; sm_region.epsilon = vb; }
            else if (m == "nlmeans") { sm_region.mode = ARTGPU_SMOOTHING_NLMEANS; sm_region.nlstrength = va; sm_region.nldetail = vb; }
            else { std::fprintf(stderr, "%s", usage); return 2; }
            if (c == "l") sm_region.channel = ARTGPU_SMOOTHING_LUMINANCE;
            else if (c == "c") sm_region.channel = ARTGPU_SMOOTHING_CHROMINANCE;
            else if (c == "lc") sm_region.channel = ARTGPU_SMOOTHING_RGB;
            else { std::fprintf(stderr, "%s", usage); return 2; }
            sm_region.iterations = it;
            sm_enable = true;
        }
        else if (a == "--smoothing-mask") {
            if (std::sscanf(next(), "%lf,%lf,%lf,%d,%d,%d", &smm_lo, &smm_hi, &smm_blur, &smm_detail, &smm_threshold, &smm_opacity) < 2) {
                std::fprintf(stderr, "--smoothing-mask lo,hi[,blur[,detail[,threshold[,opacity]]]]\n"); return 2;
            }
            smm_enable = true;
        }
        else if (a == "--tone-equalizer") {
            if (std::sscanf(next(), "%d,%d,%d,%d,%d,%d,%lf", &te_bands[0], &te_bands[1], &te_bands[2], &te_bands[3], &te_bands[4], &te_reg, &te_pivot) < 5) {
                std::fprintf(stderr, "--tone-equalizer b0,b1,b2,b3,b4[,regularization[,pivot]]\n"); return 2;
            }
            te_enable = true;
        }
        else if (a == "--film-simulation") {
            const std::string v = next();
            const size_t c = v.find(',');
            if (c == std::string::npos || std::sscanf(v.c_str() + c + 1, "%d,%d,%d", &fs_level, &fs_strength, &fs_after) < 1) {
                std::fprintf(stderr, "--film-simulation file.u16,level[,strength[,after]]\n"); return 2;
            }
            fs_file = v.substr(0, c);
        }
        else if (a == "--film-grain") {
            if (std::sscanf(next(), "%d,%d,%d", &fg_iso, &fg_strength, &fg_color) < 2) { std::fprintf(stderr, "--film-grain iso,strength[,color]\n"); return 2; }
            fg_enable = true;
        }
        else if (a == "--gradient") {
            if (std::sscanf(next(), "%lf,%d,%lf,%d,%d", &gr_degree, &gr_feather, &gr_strength, &gr_cx, &gr_cy) != 5) { std::fprintf(stderr, "--gradient DEG,FEATHER,STRENGTH,CX,CY\n"); return 2; }
            gr_enable = true;
        }
        else if (a == "--vignette") {
            if (std::sscanf(next(), "%lf,%d,%d,%d,%d", &pv_strength, &pv_feather, &pv_roundness, &pv_cx, &pv_cy) != 5) { std::fprintf(stderr, "--vignette STRENGTH,FEATHER,ROUNDNESS,CX,CY\n"); return 2; }
            pv_enable = true;
        }
        else if (a == "--soft-light") { sl_strength = std::atoi(next()); sl_enable = true; }
        else if (a == "--bw") {
            static const char *const settings[] = {"NormalContrast", "Panchromatic", "HyperPanchromatic", "LowSensitivity", "HighSensitivity", "Orthochromatic", "HighContrast",
                                                   "Luminance", "Landscape", "Portrait", "InfraRed", "RGB-Rel", "RGB-Abs", "ROYGCBPM-Rel", "ROYGCBPM-Abs"};
            static const char *const filters_[] = {"None", "Red", "Orange", "Yellow", "YellowGreen", "Green", "Cyan", "Blue", "Purple"};
            std::vector<std::string> f;
            const std::string v = next();
            for (size_t pos = 0;;) { const size_t e = v.find(',', pos); f.push_back(v.substr(pos, e == std::string::npos ? std::string::npos : e - pos)); if (e == std::string::npos) break; pos = e + 1; }
            bw_setting = bw_filter = -1;
            for (int k = 0; k < ARTGPU_BW_SETTING_COUNT; ++k) if (f[0] == settings[k]) bw_setting = k;
            if (f.size() < 2) bw_filter = ARTGPU_BW_FILTER_NONE;
            else for (int k = 0; k < ARTGPU_BW_FILTER_COUNT; ++k) if (f[1] == filters_[k]) bw_filter = k;
            if (bw_setting < 0 || bw_filter < 0 || (f.size() != 1 && f.size() != 2 && f.size() != 5 && f.size() != 8)) { std::fprintf(stderr, "--bw SETTING[,FILTER[,R,G,B[,GR,GG,GB]]]\n"); return 2; }
            for (size_t k = 2; k < f.size(); ++k) (k < 5 ? bw_mix[k - 2] : bw_gam[k - 5]) = std::atoi(f[k].c_str());
            bw_enable = true;
        }
        else if (a == "--resize-scale") { rs_scale = std::atof(next()); rs_dataspec = 0; rs_enable = true; }
        else if (a == "--resize-fit") {
            if (std::sscanf(next(), "%dx%d", &rs_width, &rs_height) != 2 || rs_width < 1 || rs_height < 1) { std::fprintf(stderr, "--resize-fit WxH\n"); return 2; }
            rs_dataspec = 3; rs_enable = true;
        }
        else { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
    }
    ProcParams::Mask cc_mask;
    cc_mask.parametricMask.enabled = true; cc_mask.parametricMask.blur = ccm_blur; cc_mask.parametricMask.lightnessDetail = ccm_detail;
    cc_mask.parametricMask.contrastThreshold = ccm_threshold; cc_mask.opacity = ccm_opacity;
    cc_mask.parametricMask.lightness = {1 /*FCT_MinMaxCPoints*/, 0.0, 0.0, 0.35, 0.35, ccm_lo, 1.0, 0.35, 0.35, ccm_hi, 1.0, 0.35, 0.35, 1.0, 0.0, 0.35, 0.35};
    ProcParams::Mask sm_mask;
    sm_mask.parametricMask.enabled = true; sm_mask.parametricMask.blur = smm_blur; sm_mask.parametricMask.lightnessDetail = smm_detail;
    sm_mask.parametricMask.contrastThreshold = smm_threshold; sm_mask.opacity = smm_opacity;
    sm_mask.parametricMask.lightness = {1 /*FCT_MinMaxCPoints*/, 0.0, 0.0, 0.35, 0.35, smm_lo, 1.0, 0.35, 0.35, smm_hi, 1.0, 0.35, 0.35, 1.0, 0.0, 0.35, 0.35};
    ProcParams::Mask tb_mask;
    tb_mask.parametricMask.enabled = true; tb_mask.parametricMask.blur = tbm_blur; tb_mask.parametricMask.lightnessDetail = tbm_detail;
    tb_mask.parametricMask.contrastThreshold = tbm_threshold; tb_mask.opacity = tbm_opacity;
    tb_mask.parametricMask.lightness = {1 /*FCT_MinMaxCPoints*/, 0.0, 0.0, 0.35, 0.35, tbm_lo, 1.0, 0.35, 0.35, tbm_hi, 1.0, 0.35, 0.35, 1.0, 0.0, 0.35, 0.35};
    // the CLUT file onto the context's device (what CLUTStore::getHaldClut hands to CLUTApplication); released when `clut` leaves scope
    struct ClutHandle { artgpu_clut *h = nullptr; ~ClutHandle() { artgpu_clut_destroy(h); } } clut;
    const auto film_simulation = [&](Context &ctx, ProcParams &params) {
        if (fs_file.empty()) return;
        const size_t n = fs_level > 0 && fs_level <= 256 ? (size_t)fs_level * fs_level * fs_level * 3 : 0;
        std::vector<uint16_t> table(n);
        std::ifstream f(fs_file, std::ios::binary);
        if (!f) throw std::runtime_error("cannot open " + fs_file);
        f.read(reinterpret_cast<char *>(table.data()), (std::streamsize)n * 2);
        if (!f) throw std::runtime_error("short read on " + fs_file);
        ctx.check(artgpu_clut_create(ctx.get(), table.data(), fs_level, 3, &clut.h));
        params.filmSimulation.enabled = true; params.filmSimulation.clut = clut.h; params.filmSimulation.strength = fs_strength;
        params.filmSimulation.after_tone_curve = fs_after != 0; params.filmSimulation.same_profile = true;
    };
    if ((in.empty() && batch.empty()) || W <= 0 || H <= 0) { std::fprintf(stderr, "usage: artgpu-cli --in frame.f32 | --batch a.u16,b.u16,... --width W --height H [options]\n"); return 2; }
    if (!batch.empty()) {
        try {
            Context ctx(0);
            ProcParams params;
            params.bayersensor.method = method; params.bayersensor.border = border;
            params.denoise.enabled = dn; params.denoise.luminance = lum; params.denoise.chrominance = chroma; params.denoise.luminanceDetail = 50;
            params.exposure.expcomp = expcomp;
            params.toneCurve.lut = default_tone_lut(); params.toneCurve.curveMode = tone_mode;
            params.raw.enable_ca = ca_enable; params.raw.ca_autocorrect = ca_auto; params.raw.caautoiterations = ca_iter;
            params.raw.cared = ca_red; params.raw.cablue = ca_blue; params.raw.ca_avoidcolourshift = ca_avoid;
            params.dehaze.enabled = dh_enable; params.dehaze.depth = dh_depth; params.dehaze.blackpoint = dh_black; params.dehaze.luminance = dh_lum != 0;
            params.dehaze.strength = {1, 0.0, dh_y, 0.0, 0.0, 1.0, dh_y, 0.0, 0.0};
            params.sharpening.enabled = sh_enable; params.sharpening.contrast = sh_contrast; params.sharpening.deconvradius = sh_radius; params.sharpening.deconvAutoRadius = sh_auto;
            params.sharpening.deconvamount = sh_amount; params.sharpening.deconvCornerBoost = sh_boost; params.sharpening.deconvCornerLatitude = sh_latitude;
            params.textureBoost.enabled = tb_enable; params.textureBoost.regions = {{tb_strength, tb_threshold, tb_iterations}};
        if (tbm_enable) params.textureBoost.masks = {ProcParams::TextureBoostMask{true, nullptr, &tb_mask}};
        params.colorcorrection.enabled = cc_enable; params.colorcorrection.regions = {cc_region};
        if (ccm_enable) params.colorcorrection.masks = {ProcParams::ColorCorrectionMask{true, nullptr, nullptr, &cc_mask}};
        params.toneEqualizer.enabled = te_enable; params.toneEqualizer.regularization = te_reg; params.toneEqualizer.pivot = te_pivot;
        for (int k = 0; k < 5; ++k) params.toneEqualizer.bands[k] = te_bands[k];
        film_simulation(ctx, params);
        params.grain.enabled = fg_enable; params.grain.iso = fg_iso; params.grain.strength = fg_strength; params.grain.color = fg_color != 0;
        params.smoothing.enabled = sm_enable; params.smoothing.regions = {sm_region};
        if (smm_enable) params.smoothing.masks = {ProcParams::SmoothingMask{true, nullptr, &sm_mask}};
        params.gradient.enabled = gr_enable; params.gradient.degree = gr_degree; params.gradient.feather = gr_feather; params.gradient.strength = gr_strength;
        params.gradient.centerX = gr_cx; params.gradient.centerY = gr_cy;
        params.pcvignette.enabled = pv_enable; params.pcvignette.strength = pv_strength; params.pcvignette.feather = pv_feather; params.pcvignette.roundness = pv_roundness;
        params.pcvignette.centerX = pv_cx; params.pcvignette.centerY = pv_cy;
        params.softlight.enabled = sl_enable; params.softlight.strength = sl_strength;
        params.blackwhite.enabled = bw_enable; params.blackwhite.setting = bw_setting; params.blackwhite.filter = bw_filter;
        params.blackwhite.mixerRed = bw_mix[0]; params.blackwhite.mixerGreen = bw_mix[1]; params.blackwhite.mixerBlue = bw_mix[2];
        params.blackwhite.gammaRed = bw_gam[0]; params.blackwhite.gammaGreen = bw_gam[1]; params.blackwhite.gammaBlue = bw_gam[2];
        params.resize.enabled = rs_enable; params.resize.dataspec = rs_dataspec; params.resize.scale = rs_scale; params.resize.width = rs_width; params.resize.height = rs_height;
            BatchQueue q(ctx, 16);
            std::vector<std::string> names;
            for (size_t pos = 0; pos <= batch.size();) {
                const size_t e = batch.find(',', pos);
                names.push_back(batch.substr(pos, e == std::string::npos ? std::string::npos : e - pos));
                if (e == std::string::npos) break;
                pos = e + 1;
            }
            for (const std::string &n : names) {
                BatchQueue::Job &j = q.addJob(W, H, border, &params);
                std::ifstream f(n, std::ios::binary);
                if (!f) throw std::runtime_error("cannot open " + n);
                f.read(reinterpret_cast<char *>(j.sensor), (std::streamsize)W * H * 2);
                if (!f) throw std::runtime_error("short read on " + n);
            }
            const float mul[3] = {2.1374f, 1.0f, 1.5918f};
            const double mat[9] = {0.6325, 0.2312, 0.0921, 0.2198, 0.7712, 0.0090, 0.0166, 0.0713, 0.7514};
            const float cblack[4] = {black, black, black, black}, smul[4] = {1.f, 1.f, 1.f, 1.f};
            auto t0 = std::chrono::steady_clock::now();
            q.process(params, filters, mul, mat, lanes, cblack, smul);
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            const int fw = q.jobs[0].outW, fh = q.jobs[0].outH;
            for (size_t k = 0; k < q.jobs.size(); ++k) {
                if (out.empty()) break;
                std::ofstream o(out + "." + std::to_string(k) + ".ppm", std::ios::binary);
                o << "P6\n" << fw << " " << fh << "\n65535\n";
                const uint16_t *sc = reinterpret_cast<const uint16_t *>(q.jobs[k].scanlines);
                std::vector<unsigned char> row((size_t)fw * 6);
                for (int y = 0; y < fh; ++y) {
                    for (size_t e = 0; e < (size_t)fw * 3; ++e) { const uint16_t v = sc[(size_t)y * fw * 3 + e]; row[2 * e] = (unsigned char)(v >> 8); row[2 * e + 1] = (unsigned char)(v & 255); }
                    o.write(reinterpret_cast<char *>(row.data()), (std::streamsize)row.size());
                }
            }
            std::printf("{\"frames\": %zu, \"lanes\": %d, \"width\": %d, \"height\": %d, \"out_width\": %d, \"out_height\": %d, \"batch_ms\": %.3f, \"chmax0\": [%.1f, %.1f, %.1f]}\n",
                        q.jobs.size(), lanes, W, H, fw, fh, ms, q.jobs[0].chmax[0], q.jobs[0].chmax[1], q.jobs[0].chmax[2]);
        } catch (const std::exception &e) {
            std::fprintf(stderr, "artgpu-cli: %s\n", e.what());
            return 1;
        }
        return 0;
    }
    try {
        std::vector<float> cfa((size_t)W * H);
        std::ifstream f(in, std::ios::binary);
        if (!f) throw std::runtime_error("cannot open " + in);
        if (u16) {
            std::vector<uint16_t> t((size_t)W * H);
            f.read(reinterpret_cast<char *>(t.data()), (std::streamsize)t.size() * 2);
            for (size_t k = 0; k < t.size(); ++k) cfa[k] = (float)t[k];
        } else {
            f.read(reinterpret_cast<char *>(cfa.data()), (std::streamsize)cfa.size() * 4);
        }
        if (!f) throw std::runtime_error("short read on " + in);

        Context ctx(0);
        ProcParams params;
        params.bayersensor.method = method;
        params.bayersensor.border = border;
        params.denoise.enabled = dn; params.denoise.luminance = lum; params.denoise.chrominance = chroma; params.denoise.luminanceDetail = 50;
        params.denoise.smoothingEnabled = smoothing; params.denoise.guidedChromaRadius = gradius; params.denoise.nlStrength = nlstrength; params.denoise.nlDetail = nldetail;
        params.exposure.expcomp = expcomp;
        params.toneCurve.lut = default_tone_lut();
        params.toneCurve.curveMode = tone_mode;
        // the default-off tools of SURVEY 8f N4, driven through the same ImProcFunctions mirror
        params.bayersensor.dual = dual; params.bayersensor.dualSecond = dual_second;
        params.bayersensor.dualDemosaicContrast = dual_contrast; params.bayersensor.dualDemosaicAutoContrast = dual_auto;
        params.logenc.enabled = logenc; params.logenc.regularization = logenc_reg;
        params.saturation.enabled = sat != 0 || vib != 0; params.saturation.saturation = sat; params.saturation.vibrance = vib;
        params.labCurve.enabled = labcurve; params.labCurve.chromaticity = labchroma;
        params.dehaze.enabled = dh_enable; params.dehaze.depth = dh_depth; params.dehaze.blackpoint = dh_black; params.dehaze.luminance = dh_lum != 0;
        params.dehaze.strength = {1, 0.0, dh_y, 0.0, 0.0, 1.0, dh_y, 0.0, 0.0};
        params.sharpening.enabled = sh_enable; params.sharpening.contrast = sh_contrast; params.sharpening.deconvradius = sh_radius; params.sharpening.deconvAutoRadius = sh_auto;
        params.sharpening.deconvamount = sh_amount; params.sharpening.deconvCornerBoost = sh_boost; params.sharpening.deconvCornerLatitude = sh_latitude;
        params.textureBoost.enabled = tb_enable; params.textureBoost.regions = {{tb_strength, tb_threshold, tb_iterations}};
        if (tbm_enable) params.textureBoost.masks = {ProcParams::TextureBoostMask{true, nullptr, &tb_mask}};
        params.colorcorrection.enabled = cc_enable; params.colorcorrection.regions = {cc_region};
        if (ccm_enable) params.colorcorrection.masks = {ProcParams::ColorCorrectionMask{true, nullptr, nullptr, &cc_mask}};
        params.toneEqualizer.enabled = te_enable; params.toneEqualizer.regularization = te_reg; params.toneEqualizer.pivot = te_pivot;
        for (int k = 0; k < 5; ++k) params.toneEqualizer.bands[k] = te_bands[k];
        film_simulation(ctx, params);
        params.grain.enabled = fg_enable; params.grain.iso = fg_iso; params.grain.strength = fg_strength; params.grain.color = fg_color != 0;
        params.smoothing.enabled = sm_enable; params.smoothing.regions = {sm_region};
        if (smm_enable) params.smoothing.masks = {ProcParams::SmoothingMask{true, nullptr, &sm_mask}};
        params.gradient.enabled = gr_enable; params.gradient.degree = gr_degree; params.gradient.feather = gr_feather; params.gradient.strength = gr_strength;
        params.gradient.centerX = gr_cx; params.gradient.centerY = gr_cy;
        params.pcvignette.enabled = pv_enable; params.pcvignette.strength = pv_strength; params.pcvignette.feather = pv_feather; params.pcvignette.roundness = pv_roundness;
        params.pcvignette.centerX = pv_cx; params.pcvignette.centerY = pv_cy;
        params.softlight.enabled = sl_enable; params.softlight.strength = sl_strength;
        params.blackwhite.enabled = bw_enable; params.blackwhite.setting = bw_setting; params.blackwhite.filter = bw_filter;
        params.blackwhite.mixerRed = bw_mix[0]; params.blackwhite.mixerGreen = bw_mix[1]; params.blackwhite.mixerBlue = bw_mix[2];
        params.blackwhite.gammaRed = bw_gam[0]; params.blackwhite.gammaGreen = bw_gam[1]; params.blackwhite.gammaBlue = bw_gam[2];
        params.resize.enabled = rs_enable; params.resize.dataspec = rs_dataspec; params.resize.scale = rs_scale; params.resize.width = rs_width; params.resize.height = rs_height;
        params.localContrast.enabled = lc_enable;
        if (lc_enable) {
            ProcParams::LocalContrastRegion region;
            region.contrast = lc_contrast;
            if (!lc_curve.empty()) region.curve = lc_curve;
            params.localContrast.regions.push_back(region);
        }
        params.labCurve.curves = [](const uint32_t *, std::vector<float> &lc, std::vector<float> &ac, std::vector<float> &bc) {
            // stands in for get_L_curve / get_ab_curves (DiagonalCurve, host code of the application): identity curves, so only chromaticity acts
            lc.resize(32770); ac.resize(65536); bc.resize(65536);
            for (int i = 0; i < 32770; ++i) lc[i] = (float)i;
            for (int i = 0; i < 65536; ++i) ac[i] = bc[i] = (float)i;
        };

        auto t0 = std::chrono::steady_clock::now();
        // stage_init (simpleprocess.cc:215-259)
        static const int32_t fuji[36] = {1, 1, 0, 1, 1, 2, 1, 1, 2, 1, 1, 0, 2, 0, 1, 0, 2, 1, 1, 1, 2, 1, 1, 0, 1, 1, 0, 1, 1, 2, 0, 2, 1, 2, 0, 1};
        static const float cam[12] = {1.60f, -0.45f, -0.15f, 0.f, -0.20f, 1.45f, -0.25f, 0.f, 0.02f, -0.50f, 1.48f, 0.f};
        RawImageSource imgsrc = xtrans_passes ? RawImageSource(ctx, W, H, fuji, cam) : RawImageSource(ctx, W, H, filters, 1.0);
        params.xtranssensor.method = xtrans_passes == 1 ? ProcParams::ONE_PASS : ProcParams::THREE_PASS;
        imgsrc.setBorder(border);
        imgsrc.load(cfa.data());
        params.raw.enable_ca = ca_enable; params.raw.ca_autocorrect = ca_auto; params.raw.caautoiterations = ca_iter;
        params.raw.cared = ca_red; params.raw.cablue = ca_blue; params.raw.ca_avoidcolourshift = ca_avoid;
        imgsrc.preprocessCA(params);            // rawimagesource.cc:1827-1840 (the input stands for the scaled CFA)
        imgsrc.demosaic(params);
        int fw, fh;
        imgsrc.getFullSize(fw, fh);
        Imagefloat full(fw, fh);
        Imagefloat &img = full;
        const float mul[3] = {2.1374f, 1.0f, 1.5918f};
        const double mat[9] = {0.6325, 0.2312, 0.0921, 0.2198, 0.7712, 0.0090, 0.0166, 0.0713, 0.7514};
        ImProcFunctions ipf(ctx, &params, 1.0);
        if (dn && chroma_auto) {    // simpleprocess.cc:254-256
            ImProcFunctions::DenoiseInfoStore dnstore;
            params.denoise.chrominanceMethod = 1;
            imgsrc.setColorMatrix(mat);
            ipf.denoiseComputeParams(&imgsrc, mul, true, dnstore, params.denoise);
            std::fprintf(stderr, "auto chrominance: %.6f  red-green %.6f  blue-yellow %.6f\n", params.denoise.chrominance,
                         params.denoise.chrominanceRedGreen, params.denoise.chrominanceBlueYellow);
        }
        if (params.sharpening.enabled && params.sharpening.deconvAutoRadius) {      // simpleprocess.cc:274-278
            float r = 0.f;
            if (imgsrc.getDeconvAutoRadius(&r)) {
                params.sharpening.deconvradius = r;
                std::fprintf(stderr, "auto deconvolution radius: %.6f\n", r);
            }
        }
        imgsrc.getImage(mul, true, &img);
        // stage_denoise (simpleprocess.cc:311-315)
        imgsrc.convertColorSpace(&img, mat);
        ipf.denoise(&imgsrc, &img);
        ipf.process(ImProcFunctions::Pipeline::OUTPUT, ImProcFunctions::Stage::STAGE_0, &img);       // simpleprocess.cc:329
        // stage_finish (simpleprocess.cc:389-396)
        ipf.process(ImProcFunctions::Pipeline::OUTPUT, ImProcFunctions::Stage::STAGE_1, &img);
        ipf.process(ImProcFunctions::Pipeline::OUTPUT, ImProcFunctions::Stage::STAGE_2, &img);
        ipf.process(ImProcFunctions::Pipeline::OUTPUT, ImProcFunctions::Stage::STAGE_3, &img);
        // the Resize tool (simpleprocess.cc:402-414)
        std::unique_ptr<Imagefloat> resized;
        if (params.resize.enabled) {
            int imw, imh;
            const float rscale = ImProcFunctions::resizeScale(&params, fw, fh, imw, imh);
            if (rscale < 1.f || (rscale > 1.f && (params.resize.allowUpscaling || params.resize.dataspec == 0))) {
                resized.reset(new Imagefloat(imw, imh));
                ipf.resize(&full, resized.get(), rscale);
                fw = imw; fh = imh;
            }
        }
        Imagefloat &result = resized ? *resized : full;
        ctx.synchronize();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

        std::vector<float> r((size_t)fw * fh), g(r.size()), b(r.size());
        result.r.download(r.data()); result.g.download(g.data()); result.b.download(b.data());
        double sum = 0;
        for (size_t k = 0; k < r.size(); ++k) sum += r[k] + g[k] + b[k];
        if (!out.empty()) {
            std::ofstream o(out, std::ios::binary);
            o << "P6\n" << fw << " " << fh << "\n65535\n";
            std::vector<unsigned char> row((size_t)fw * 6);
            for (int y = 0; y < fh; ++y) {
                for (int x = 0; x < fw; ++x) {
                    const float v[3] = {r[(size_t)y * fw + x], g[(size_t)y * fw + x], b[(size_t)y * fw + x]};
                    for (int c = 0; c < 3; ++c) {
                        const int q = (int)std::lrint(std::fmin(std::fmax(v[c], 0.f), 65535.f));
                        row[(size_t)x * 6 + 2 * c] = (unsigned char)(q >> 8);
                        row[(size_t)x * 6 + 2 * c + 1] = (unsigned char)(q & 255);
                    }
                }
                o.write(reinterpret_cast<char *>(row.data()), (std::streamsize)row.size());
            }
        }
        std::printf("{\"width\": %d, \"height\": %d, \"out_width\": %d, \"out_height\": %d, \"total_ms_incl_io\": %.3f, \"mean\": %.4f}\n",
                    W, H, fw, fh, ms, sum / (3.0 * r.size()));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "artgpu-cli: %s\n", e.what());
        return 1;
    }
    return 0;
}
