// art_amd/host/rtengine_gpu.h -- C++ host-side mirror of the rtengine classes on the hot path, over the
// C ABI of include/artgpu.h.  Same method names, argument meaning and call order as the reference, so
// that a caller written against rtengine (rtgui/main-cli.cc:786-903, rtengine/simpleprocess.cc:75-420)
// reads the same:
//   RawImageSource::{demosaic, getImage, convertColorSpace, setBorder}   rawimagesource.h:119-136,266-290
//   ImProcFunctions::{process, exposure, toneCurve, denoise}             improcfun.h:95,132-133,147,150
//   Imagefloat (planar fp32 R|G|B, row stride ceil16(W*4))               iimage.h:653-720
// Frames stay resident in HBM between stages (on_device planes).  Error behaviour: the reference
// methods return void; here a failing artgpu_* call throws std::runtime_error with the library's
// message -- an adapter inside ART would instead fall through to the CPU code.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <functional>
#include <memory>
#include <vector>
#include "../../include/artgpu.h"

namespace artgpu_host {

inline void hipcheck(hipError_t e, const char *what)
{
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

class Context {
public:
    explicit Context(int device = 0) { if (artgpu_create(device, &ctx_) != 0) throw std::runtime_error("artgpu_create failed"); }
    ~Context() { if (ctx_) artgpu_destroy(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    artgpu_ctx *get() const { return ctx_; }
    void check(int rc) const { if (rc != 0) throw std::runtime_error(std::string("artgpu: ") + artgpu_last_error(ctx_)); }
    void synchronize() const { check(artgpu_synchronize(ctx_)); }
private:
    artgpu_ctx *ctx_ = nullptr;
};

// One fp32 plane in HBM (array2D<float> counterpart; rows contiguous, stride W*4)
class DevicePlane {
public:
    DevicePlane() = default;
    DevicePlane(int w, int h, int64_t stride_bytes = 0) { alloc(w, h, stride_bytes); }
    ~DevicePlane() { release(); }
    DevicePlane(const DevicePlane &) = delete;
    DevicePlane &operator=(const DevicePlane &) = delete;
    void alloc(int w, int h, int64_t stride_bytes = 0)
    {
        release();
        w_ = w; h_ = h; stride_ = stride_bytes ? stride_bytes : (int64_t)w * 4;
        hipcheck(hipMalloc(reinterpret_cast<void **>(&p_), (size_t)stride_ * h), "hipMalloc(plane)");
    }
    void release() { if (p_) { (void)hipFree(p_); p_ = nullptr; } }
    void upload(const float *host) { hipcheck(hipMemcpy2D(p_, (size_t)stride_, host, (size_t)w_ * 4, (size_t)w_ * 4, h_, hipMemcpyHostToDevice), "upload"); }
    void download(float *host) const { hipcheck(hipMemcpy2D(host, (size_t)w_ * 4, p_, (size_t)stride_, (size_t)w_ * 4, h_, hipMemcpyDeviceToHost), "download"); }
    artgpu_plane view() const { return artgpu_plane{p_, w_, h_, stride_, 1}; }
    int width() const { return w_; }
    int height() const { return h_; }
private:
    float *p_ = nullptr;
    int w_ = 0, h_ = 0;
    int64_t stride_ = 0;
};

// rtengine::Imagefloat counterpart: three planes, row stride ceil16(W*4) bytes (iimage.h:653-720)
class Imagefloat {
public:
    Imagefloat(int w, int h) : r(w, h, ((int64_t)w * 4 + 15) / 16 * 16), g(w, h, ((int64_t)w * 4 + 15) / 16 * 16), b(w, h, ((int64_t)w * 4 + 15) / 16 * 16) {}
    int getWidth() const { return r.width(); }
    int getHeight() const { return r.height(); }
    artgpu_rgb view() const { return artgpu_rgb{r.view(), g.view(), b.view()}; }
    DevicePlane r, g, b;
};

// The fields of ProcParams the path reads (procparams.cc:1528-3335 for the defaults)
struct ProcParams {
    // raw.bayersensor.{method,border,dualDemosaicContrast,dualDemosaicAutoContrast}; dual = the AMAZEBILINEAR / RCDBILINEAR / AMAZEVNG4 / RCDVNG4 methods
    // (first demosaicer `method`, dualSecond in flat regions; rawimagesource.cc:1876-1886 -> dual_demosaic_RT)
    struct { int method = ARTGPU_BAYER_AMAZE; int border = 4; bool dual = false; int dualSecond = ARTGPU_DUAL_BILINEAR; double dualDemosaicContrast = 20; bool dualDemosaicAutoContrast = true; } bayersensor;
    enum XTransMethod { ONE_PASS = 1, THREE_PASS = 3 };
    struct { int method = THREE_PASS; int border = 7; } xtranssensor;          // raw.xtranssensor.{method,border} (procparams.cc:3064)
    // RAWParams' CA correction fields (procparams.cc:3122-3133; the Dynamic profile's Auto-Matched Curve.arp sets enable_ca and ca_autocorrect)
    struct { bool enable_ca = false; bool ca_autocorrect = false; int caautoiterations = 2; double cared = 0, cablue = 0; bool ca_avoidcolourshift = true; } raw;
    // the call site's condition (rawimagesource.cc:1827): Bayer only, auto or a manual shift
    bool caApplies() const { return raw.enable_ca && (raw.ca_autocorrect || std::fabs(raw.cared) > 0.001 || std::fabs(raw.cablue) > 0.001); }
    artgpu_ca_params caParams() const
    {
        return artgpu_ca_params{raw.ca_autocorrect ? 1 : 0, raw.caautoiterations, raw.cared, raw.cablue, raw.ca_avoidcolourshift ? 1 : 0};
    }
    struct { bool enabled = false; double luminance = 0, luminanceDetail = 0; int luminanceDetailThreshold = 0; double chrominance = 15,
             chrominanceRedGreen = 0, chrominanceBlueYellow = 0, gamma = 1.7, chrominanceAutoFactor = 1; bool aggressive = false; int colorSpace = 0, chrominanceMethod = 0;
             bool smoothingEnabled = false; int guidedChromaRadius = 3, nlDetail = 80, nlStrength = 0; } denoise;   // procparams.cc:1900-1918 (chrominanceMethod: 0 MANUAL, 1 AUTOMATIC)
    struct { bool enabled = true; double expcomp = 0, black = 0; } exposure;
    struct { bool enabled = false; int red[3] = {1000, 0, 0}, green[3] = {0, 1000, 0}, blue[3] = {0, 0, 1000}; } chmixer;        // procparams.cc (ChannelMixerParams)
    struct { bool enabled = false; std::vector<double> hCurve, sCurve, lCurve; int smoothing = 0; } hsl;                         // HSLEqualizerParams
    struct { bool enabled = false; double gain = 0, targetGray = 18, blackEv = -13.5, whiteEv = 2.5; int regularization = 60; bool satcontrol = true;
             int highlightCompression = 0; } logenc;                                                                               // LogEncodingParams (procparams.cc:2039-2051)
    // LabCurveParams: brightness / contrast / the three DiagonalCurves stay host code (get_L_curve / get_ab_curves, iplabadjustments.cc:67-191);
    // `curves` is that code: it receives hist16 (nullptr unless contrast != 0) and fills lcurve[32770], acurve[65536], bcurve[65536]
    struct { bool enabled = false; int chromaticity = 0, contrast = 0;
             std::function<void(const uint32_t *hist16, std::vector<float> &lcurve, std::vector<float> &acurve, std::vector<float> &bcurve)> curves; } labCurve;
    struct { bool enabled = false; int saturation = 0, vibrance = 0; } saturation;                                               // SaturationParams
    // DehazeParams (procparams.cc:2694-2711); strength = FlatCurve control points
    struct { bool enabled = false; std::vector<double> strength = {1 /*FCT_MinMaxCPoints*/, 0.0, 0.75, 0.0, 0.0, 1.0, 0.75, 0.0, 0.0}; bool showDepthMap = false;
             int depth = 25; bool luminance = false; int blackpoint = 0; } dehaze;
    artgpu_dehaze_params dehazeParams() const
    {
        return artgpu_dehaze_params{dehaze.enabled ? 1 : 0, dehaze.strength.data(), (int32_t)dehaze.strength.size(), dehaze.showDepthMap ? 1 : 0, dehaze.depth,
                                    dehaze.luminance ? 1 : 0, dehaze.blackpoint};
    }
    // SharpeningParams (procparams.cc:1756-1775), the fields the rld method reads; the Dynamic profile's Sharpening.arp sets enabled, method rld,
    // contrast 20, deconvamount 100 and deconvAutoRadius below ISO 640
    struct { bool enabled = false; double contrast = 20.0; int amount = 200; int method = ARTGPU_SHARPEN_RLD; int deconvamount = 100; double deconvradius = 0.75;
             bool deconvAutoRadius = true; double deconvCornerBoost = 0.0; int deconvCornerLatitude = 25; } sharpening;
    // offset_x / offset_y / full_width / full_height: ImProcFunctions' crop geometry (improcfun.h), 0 = the image itself
    artgpu_sharpening_params sharpeningParams(int offset_x = 0, int offset_y = 0, int full_width = 0, int full_height = 0) const
    {
        return artgpu_sharpening_params{sharpening.enabled ? 1 : 0, sharpening.method, sharpening.amount, sharpening.deconvamount, sharpening.contrast,
                                        sharpening.deconvradius, sharpening.deconvCornerBoost, sharpening.deconvCornerLatitude, offset_x, offset_y,
                                        full_width, full_height, 0};
    }
    // ImpulseDenoiseParams (procparams.h:736-744) and DefringeParams (procparams.h:721-731; defaults procparams.cc:1835-1867)
    struct { bool enabled = false; int thresh = 50; } impulseDenoise;
    struct { bool enabled = false; double radius = 2.0; int threshold = 13;
             std::vector<double> huecurve = {1 /*FCT_MinMaxCPoints*/, 0.166666667, 0., 0.35, 0.35, 0.347, 0., 0.35, 0.35, 0.513667426, 0, 0.35, 0.35, 0.668944571, 0., 0.35, 0.35,
                                             0.8287775246, 0.97835991, 0.35, 0.35, 0.9908883827, 0., 0.35, 0.35}; } defringe;
    artgpu_impulse_denoise_params impulseDenoiseParams() const { return artgpu_impulse_denoise_params{impulseDenoise.enabled ? 1 : 0, impulseDenoise.thresh}; }
    artgpu_defringe_params defringeParams() const
    {
        return artgpu_defringe_params{defringe.enabled ? 1 : 0, defringe.threshold, defringe.radius, defringe.huecurve.empty() ? nullptr : defringe.huecurve.data(),
                                      (int32_t)defringe.huecurve.size(), 0};
    }
    // rtengine::procparams::Mask (procparams.cc:1014-1053, 1122-1137) as generateMasks' parametric path reads it.  `area` is
    // generate_area_mask's finished plane (rasterising the shapes is host code of the application).  deltaE, drawn, external and linked masks,
    // a mask curve other than the identity: flags only, artgpu_generate_masks answers them with ARTGPU_EUNSUPPORTED
    struct Mask {
        bool enabled = true, inverted = false;
        struct {
            bool enabled = false; double blur = 0;
            std::vector<double> hue = {1 /*FCT_MinMaxCPoints*/, 0.166666667, 1., 0.35, 0.35, 0.8287775246, 1., 0.35, 0.35};
            std::vector<double> chromaticity = {1, 0., 1., 0.35, 0.35, 1., 1., 0.35, 0.35}, lightness = {1, 0., 1., 0.35, 0.35, 1., 1., 0.35, 0.35};
            int lightnessDetail = 0, contrastThreshold = 0;
        } parametricMask;
        const DevicePlane *area = nullptr;
        bool deltaEEnabled = false, drawnEnabled = false, externalEnabled = false, linkedEnabled = false, curveIsIdentity = true;
        int posterization = 0, smoothing = 0, opacity = 100;
        // `areaView` keeps the view `area` points to
        artgpu_mask_params params(artgpu_plane &areaView, bool show = false) const
        {
            const auto &pm = parametricMask;
            artgpu_mask_params m = {};
            m.parametric_enabled = pm.enabled ? 1 : 0; m.lightness_detail = pm.lightnessDetail;
            m.hue = pm.hue.data(); m.chromaticity = pm.chromaticity.data(); m.lightness = pm.lightness.data();
            m.nhue = (int32_t)pm.hue.size(); m.nchromaticity = (int32_t)pm.chromaticity.size(); m.nlightness = (int32_t)pm.lightness.size();
            m.contrast_threshold = pm.contrastThreshold; m.blur = pm.blur;
            if (area) { areaView = area->view(); m.area = &areaView; }
            m.posterization = posterization; m.smoothing = smoothing; m.inverted = inverted ? 1 : 0; m.opacity = opacity;
            m.deltae_enabled = deltaEEnabled ? 1 : 0; m.drawn_enabled = drawnEnabled ? 1 : 0; m.external_enabled = externalEnabled ? 1 : 0;
            m.linked_enabled = linkedEnabled ? 1 : 0; m.curve_is_identity = curveIsIdentity ? 1 : 0; m.show_mask = show ? 1 : 0;
            return m;
        }
    };
    // the artgpu_mask_params of a list of Masks; `areas` keeps the views they point to
    static std::vector<artgpu_mask_params> maskParams(const std::vector<const Mask *> &masks, std::vector<artgpu_plane> &areas, int show_mask_idx = -1)
    {
        static const Mask dflt;
        areas.assign(masks.size(), artgpu_plane{});
        std::vector<artgpu_mask_params> out;
        for (size_t k = 0; k < masks.size(); ++k) out.push_back((masks[k] ? masks[k] : &dflt)->params(areas[k], (int)k == show_mask_idx));
        return out;
    }
    // LocalContrastParams (procparams.cc:1700-1760): regions {contrast, curve as FlatCurve control points}; masks[i].enabled and either the
    // blend plane the application's generateMasks made of masks[i] (`blend`; nullptr = all ones) or the Mask itself (`mask`: the plane is
    // generated on the device, ImProcFunctions::generateMasks below), one per region
    struct LocalContrastRegion { double contrast = 0; std::vector<double> curve = {1 /*FCT_MinMaxCPoints*/, 0.0, 0.5, 0.0, 0.0, 1.0, 0.5, 0.0, 0.0}; };
    struct LocalContrastMask { bool enabled = true; const DevicePlane *blend = nullptr; const Mask *mask = nullptr; };
    struct { bool enabled = false; std::vector<LocalContrastRegion> regions; std::vector<LocalContrastMask> masks; } localContrast;
    // TextureBoostParams (procparams.cc:1950-2022): regions {strength, detailThreshold, iterations}; masks[i].enabled and the blend plane
    // generateMasks makes of masks[i] (host code of the application; nullptr = all ones), one per region
    struct TextureBoostRegion { double strength = 0; double detailThreshold = 0.2; int iterations = 1; };
    struct TextureBoostMask { bool enabled = true; const DevicePlane *blend = nullptr; const Mask *mask = nullptr; };
    struct { bool enabled = false; std::vector<TextureBoostRegion> regions = {TextureBoostRegion()}; std::vector<TextureBoostMask> masks; } textureBoost;
    // the enabled regions as the library takes them; `blends` keeps the mask views the regions point to
    std::vector<artgpu_texture_boost_region> textureBoostRegions(std::vector<artgpu_plane> &blends) const
    {
        const auto &p = textureBoost;
        blends.assign(p.regions.size(), artgpu_plane{});
        std::vector<artgpu_texture_boost_region> regions;
        for (size_t k = 0; k < p.regions.size(); ++k) {
            if (k < p.masks.size() && !p.masks[k].enabled) continue;
            artgpu_texture_boost_region reg{p.regions[k].strength, p.regions[k].detailThreshold, p.regions[k].iterations, nullptr};
            if (k < p.masks.size() && p.masks[k].blend) { blends[k] = p.masks[k].blend->view(); reg.mask = &blends[k]; }
            regions.push_back(reg);
        }
        return regions;
    }
    // ColorCorrectionParams (procparams.cc:2834-2855, 2906-2920): regions with the reference's defaults (mode JZAZBZ); masks[i].enabled and either
    // the two blend planes the application's generateMasks made of masks[i] (`lblend` / `abblend`; nullptr = all ones) or the Mask itself
    struct ColorCorrectionRegion {
        int mode = ARTGPU_CC_JZAZBZ;
        bool rgbluminance = false;
        double a = 0, b = 0, inSaturation = 0, outSaturation = 0, hueshift = 0, hsl_gamma = 2.4;
        double slope[3] = {1, 1, 1}, offset[3] = {0, 0, 0}, power[3] = {1, 1, 1}, pivot[3] = {1, 1, 1}, compression[3] = {0, 0, 0};
        double hue[3] = {0, 0, 0}, sat[3] = {0, 0, 0}, factor[3] = {0, 0, 0};
    };
    struct ColorCorrectionMask { bool enabled = true; const DevicePlane *lblend = nullptr, *abblend = nullptr; const Mask *mask = nullptr; };
    struct { bool enabled = false; std::vector<ColorCorrectionRegion> regions = {ColorCorrectionRegion()}; std::vector<ColorCorrectionMask> masks; } colorcorrection;
    // the enabled regions as the library takes them; `blends` keeps the mask views the regions point to (two per region)
    std::vector<artgpu_color_correction_region> colorCorrectionRegions(std::vector<artgpu_plane> &blends) const
    {
        const auto &p = colorcorrection;
        blends.assign(2 * p.regions.size(), artgpu_plane{});
        std::vector<artgpu_color_correction_region> regions;
        for (size_t k = 0; k < p.regions.size(); ++k) {
            if (k < p.masks.size() && !p.masks[k].enabled) continue;
            const ColorCorrectionRegion &r = p.regions[k];
            artgpu_color_correction_region reg = {};
            reg.mode = r.mode; reg.rgbluminance = r.rgbluminance ? 1 : 0;
            reg.a = r.a; reg.b = r.b; reg.in_saturation = r.inSaturation; reg.out_saturation = r.outSaturation; reg.hueshift = r.hueshift; reg.hsl_gamma = r.hsl_gamma;
            for (int c = 0; c < 3; ++c) {
                reg.slope[c] = r.slope[c]; reg.offset[c] = r.offset[c]; reg.power[c] = r.power[c]; reg.pivot[c] = r.pivot[c]; reg.compression[c] = r.compression[c];
                reg.hue[c] = r.hue[c]; reg.sat[c] = r.sat[c]; reg.factor[c] = r.factor[c];
            }
            if (k < p.masks.size() && p.masks[k].lblend) { blends[2 * k] = p.masks[k].lblend->view(); reg.lmask = &blends[2 * k]; }
            if (k < p.masks.size() && p.masks[k].abblend) { blends[2 * k + 1] = p.masks[k].abblend->view(); reg.abmask = &blends[2 * k + 1]; }
            regions.push_back(reg);
        }
        return regions;
    }
    // ToneEqualizerParams (procparams.cc:2097-2104)
    struct { bool enabled = false; int bands[5] = {0, 0, 0, 0, 0}; int regularization = 4; bool show_colormap = false; double pivot = 0; } toneEqualizer;
    artgpu_tone_equalizer_params toneEqualizerParams() const
    {
        const auto &t = toneEqualizer;
        artgpu_tone_equalizer_params q = {};
        q.enabled = t.enabled ? 1 : 0; q.regularization = t.regularization; q.show_colormap = t.show_colormap ? 1 : 0; q.pivot = t.pivot;
        for (int k = 0; k < 5; ++k) q.bands[k] = t.bands[k];
        return q;
    }
    // FilmSimulationParams (procparams.h: enabled, clutFilename, strength, after_tone_curve) as the device path takes them: the CLUT the application's
    // CLUTStore loaded as a handle (artgpu_clut_create), strength in percent, and what CLUTApplication::init derives from the two profile names
    // (clutstore.cc:1090-1097): same_profile, or the four ICCStore matrices
    struct {
        bool enabled = false; int strength = 100; bool after_tone_curve = false;
        const artgpu_clut *clut = nullptr;
        bool same_profile = true;
        double work_to_xyz[9] = {}, xyz_to_clut[9] = {}, clut_to_xyz[9] = {}, xyz_to_work[9] = {};
    } filmSimulation;
    artgpu_film_simulation_params filmSimulationParams() const
    {
        const auto &f = filmSimulation;
        artgpu_film_simulation_params q = {};
        q.strength = float(f.strength) / 100.f;                           // ipfilmsim.cc:46
        q.same_profile = f.same_profile ? 1 : 0;
        for (int k = 0; k < 9; ++k) { q.work_to_xyz[k] = f.work_to_xyz[k]; q.xyz_to_clut[k] = f.xyz_to_clut[k]; q.clut_to_xyz[k] = f.clut_to_xyz[k]; q.xyz_to_work[k] = f.xyz_to_work[k]; }
        return q;
    }
    // GrainParams (procparams.cc:2731-2737)
    struct { bool enabled = false; int iso = 400; int strength = 50; bool color = false; } grain;
    artgpu_film_grain_params grainParams() const { return artgpu_film_grain_params{grain.enabled ? 1 : 0, grain.iso, grain.strength, grain.color ? 1 : 0}; }
    // GradientParams, PCVignetteParams (procparams.cc:2355-2389), CropParams' box, SoftLightParams (L2675-2679), BlackWhiteParams (L2470-2482)
    struct { bool enabled = false; double degree = 0.0; int feather = 25; double strength = 0.60; int centerX = 0, centerY = 0; } gradient;
    struct { bool enabled = false; double strength = 0.60; int feather = 50, roundness = 50, centerX = 0, centerY = 0; } pcvignette;
    struct { bool enabled = false; int x = -1, y = -1, w = 15000, h = 15000; } crop;
    struct { bool enabled = false; int strength = 30; } softlight;
    struct {
        bool enabled = false;
        int filter = ARTGPU_BW_FILTER_NONE, setting = ARTGPU_BW_RGB_REL;
        int mixerRed = 33, mixerGreen = 33, mixerBlue = 33, gammaRed = 0, gammaGreen = 0, gammaBlue = 0;
        int colorCastBottom = 0, colorCastTop = 0;
        std::vector<float> ulut, vlut;             // the colour cast's tables (ipbw.cc:325-341), filled by the application: 65536 entries each
    } blackwhite;
    // offset, full size (-1: the image's own) and scale are ImProcFunctions' (improcfun.h:216-230), which the caller passes
    artgpu_creative_gradients_params creativeGradientsParams(int offset_x, int offset_y, int full_width, int full_height, double scale_) const
    {
        artgpu_creative_gradients_params q = {};
        q.gradient_enabled = gradient.enabled ? 1 : 0; q.gradient_degree = gradient.degree; q.gradient_feather = gradient.feather;
        q.gradient_strength = gradient.strength; q.gradient_center_x = gradient.centerX; q.gradient_center_y = gradient.centerY;
        q.pcvignette_enabled = pcvignette.enabled ? 1 : 0; q.pcvignette_strength = pcvignette.strength; q.pcvignette_feather = pcvignette.feather;
        q.pcvignette_roundness = pcvignette.roundness; q.pcvignette_center_x = pcvignette.centerX; q.pcvignette_center_y = pcvignette.centerY;
        q.crop_enabled = crop.enabled ? 1 : 0; q.crop_x = crop.x; q.crop_y = crop.y; q.crop_w = crop.w; q.crop_h = crop.h;
        q.offset_x = offset_x; q.offset_y = offset_y; q.full_width = full_width; q.full_height = full_height; q.scale = scale_;
        return q;
    }
    artgpu_soft_light_params softLightParams() const { return artgpu_soft_light_params{softlight.enabled ? 1 : 0, softlight.strength}; }
    artgpu_black_and_white_params blackAndWhiteParams() const
    {
        const auto &b = blackwhite;
        const bool cast = b.colorCastBottom > 0 && b.ulut.size() == 65536 && b.vlut.size() == 65536;
        return artgpu_black_and_white_params{b.enabled ? 1 : 0, b.setting, b.filter, b.mixerRed, b.mixerGreen, b.mixerBlue, b.gammaRed, b.gammaGreen, b.gammaBlue,
                                             b.colorCastBottom, b.colorCastTop, cast ? b.ulut.data() : nullptr, cast ? b.vlut.data() : nullptr};
    }
    // SmoothingParams (procparams.cc:2753-2775, procparams.h:1289-1347): regions with the reference's defaults (mode GUIDED, channel RGB);
    // masks[i].enabled and either the blend plane the application's generateMasks made of masks[i] (`blend`; nullptr = all ones) or the Mask itself
    struct SmoothingRegion {
        int mode = ARTGPU_SMOOTHING_GUIDED, channel = ARTGPU_SMOOTHING_RGB;
        int radius = 0;
        double sigma = 0;
        int epsilon = 0, iterations = 1;
        double falloff = 1;
        int nldetail = 50, nlstrength = 0, numblades = 9;
        double angle = 0, curvature = 0, offset = 0;
        int noise_strength = 10, noise_coarseness = 30;
        double halation_size = 1.0, halation_color = 0.0, wav_strength = 0;
        int wav_levels = 5;
        double wav_gamma = 2.2;
    };
    struct SmoothingMask { bool enabled = true; const DevicePlane *blend = nullptr; const Mask *mask = nullptr; };
    struct { bool enabled = false; std::vector<SmoothingRegion> regions = {SmoothingRegion()}; std::vector<SmoothingMask> masks; } smoothing;
    // the enabled regions as the library takes them; `blends` keeps the mask views the regions point to
    std::vector<artgpu_smoothing_region> smoothingRegions(std::vector<artgpu_plane> &blends) const
    {
        const auto &p = smoothing;
        blends.assign(p.regions.size(), artgpu_plane{});
        std::vector<artgpu_smoothing_region> regions;
        for (size_t k = 0; k < p.regions.size(); ++k) {
            if (k < p.masks.size() && !p.masks[k].enabled) continue;
            const SmoothingRegion &r = p.regions[k];
            artgpu_smoothing_region reg = {};
            reg.mode = r.mode; reg.channel = r.channel; reg.radius = r.radius; reg.epsilon = r.epsilon; reg.sigma = r.sigma; reg.iterations = r.iterations;
            reg.nldetail = r.nldetail; reg.falloff = r.falloff; reg.nlstrength = r.nlstrength; reg.numblades = r.numblades; reg.angle = r.angle;
            reg.curvature = r.curvature; reg.offset = r.offset; reg.noise_strength = r.noise_strength; reg.noise_coarseness = r.noise_coarseness;
            reg.halation_size = r.halation_size; reg.halation_color = r.halation_color; reg.wav_strength = r.wav_strength; reg.wav_levels = r.wav_levels;
            reg.wav_gamma = r.wav_gamma;
            if (k < p.masks.size() && p.masks[k].blend) { blends[k] = p.masks[k].blend->view(); reg.mask = &blends[k]; }
            regions.push_back(reg);
        }
        return regions;
    }
    // the Masks of the enabled regions (nullptr: the region carries none), and whether any region carries one
    template <class Tool> static bool regionMasks(const Tool &p, std::vector<const Mask *> &masks)
    {
        bool any = false;
        masks.clear();
        for (size_t k = 0; k < p.regions.size(); ++k) {
            if (k < p.masks.size() && !p.masks[k].enabled) continue;
            masks.push_back(k < p.masks.size() ? p.masks[k].mask : nullptr);
            any = any || masks.back();
        }
        return any;
    }
    // ResizeParams (procparams.h) as ImProcFunctions::resizeScale reads them: dataspec 0 scale, 1 width, 2 height, 3 fit box; width / height are
    // get_width() / get_height(), in pixels.  The mirror has no crop, so appliesTo is not here
    struct { bool enabled = false; int dataspec = 3; double scale = 1.0; int width = 900, height = 900; bool allowUpscaling = false; } resize;
    artgpu_resize_params resizeParams() const
    {
        artgpu_resize_params q = {};
        q.enabled = resize.enabled ? 1 : 0; q.dataspec = resize.dataspec; q.scale = resize.scale; q.width = resize.width; q.height = resize.height;
        q.allow_upscaling = resize.allowUpscaling ? 1 : 0;
        return q;
    }
    struct { bool enabled = false; std::vector<float> rlut, glut, blut; } rgbCurves;                                             // RGBCurvesParams, as outCurve LUTs
    struct { bool enabled = true; int curveMode = ARTGPU_TONE_STD; std::vector<float> lut; float whitePoint = 1.f; bool basecurveLinear = true; } toneCurve;
    // toneCurve.curveMode: ARTGPU_TONE_STD or ARTGPU_TONE_NEUTRAL (ART's default, procparams.cc:1585)
    double workingSpace[9] = {0.6734241, 0.1656411, 0.1251286, 0.2790177, 0.6753402, 0.0456377, -0.0019300, 0.0299784, 0.7973330}; // Rec2020 TMatrix (iccmatrices.h:151-155)
    double workingSpaceInverse[9] = {1.6473376, -0.3935675, -0.2359961, -0.6826036, 1.6475887, 0.0128190, 0.0296524, -0.0628993, 1.2531279};   // iccmatrices.h:157-161
    // NeutralToneCurve::ApplyState::to_out / to_work (curves.cc:870-878): identity unless the output profile has a matrix
    float toOut[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, toWork[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
};

// rtengine::RawImageSource counterpart for a Bayer sensor
class RawImageSource {
public:
    RawImageSource(Context &c, int W, int H, uint32_t filters, double initialGain = 1.0)
        : ctx(c), W(W), H(H), filters(filters), initialGain(initialGain), rawData(W, H), red(W, H), green(W, H), blue(W, H) {}
    // X-Trans sensor: 6x6 colour map (RawImage::getXtransMatrix) and camera matrix (getRgbCam)
    RawImageSource(Context &c, int W, int H, const int32_t xtrans_[36], const float rgb_cam_[12])
        : ctx(c), W(W), H(H), filters(9), initialGain(1.0), rawData(W, H), red(W, H), green(W, H), blue(W, H), isXtrans(true)
    {
        for (int i = 0; i < 36; ++i) xtrans[i] = xtrans_[i];
        for (int i = 0; i < 12; ++i) rgb_cam[i] = rgb_cam_[i];
        border = 7;
    }
    void setBorder(int b) { border = b; }                                   // rawimagesource.h (simpleprocess.cc:138-146)
    void load(const float *cfa_host) { rawData.upload(cfa_host); }          // stands in for load()/preprocess(): CFA 0..65535
    // RawImageSource::CA_correct_RT on rawData (CA_correct_RT.cc:122-1384, one frame), called from preprocess after scaleColors
    // (rawimagesource.cc:1827-1840) when ProcParams::caApplies(); X-Trans frames never get here (the reference skips them)
    void CA_correct_RT(bool autoCA, size_t autoIterations, double cared, double cablue, bool avoidColourshift)
    {
        artgpu_plane raw = rawData.view();
        const artgpu_ca_params cp{autoCA ? 1 : 0, (int32_t)autoIterations, cared, cablue, avoidColourshift ? 1 : 0};
        ctx.check(artgpu_raw_ca_correct(ctx.get(), &raw, filters, &cp, nullptr));
    }
    void preprocessCA(const ProcParams &p)
    {
        if (!isXtrans && p.caApplies())
            CA_correct_RT(p.raw.ca_autocorrect, (size_t)p.raw.caautoiterations, p.raw.cared, p.raw.cablue, p.raw.ca_avoidcolourshift);
    }
    // RawImageSource::demosaic (rawimagesource.cc:1854-1962)
    void demosaic(const ProcParams &p)
    {
        artgpu_plane raw = rawData.view();
        artgpu_rgb out{red.view(), green.view(), blue.view()};
        if (isXtrans) {   // rawimagesource.cc:1915-1925: ONE_PASS -> (1, false), THREE_PASS -> (3, true)
            const int passes = p.xtranssensor.method == ProcParams::ONE_PASS ? 1 : 3;
            ctx.check(artgpu_demosaic_xtrans(ctx.get(), passes, passes > 1 ? 1 : 0, &raw, xtrans, rgb_cam, &out));
            return;
        }
        if (p.bayersensor.dual) {       // `contrast` comes back as the threshold in use (the reference's `double &contrast`)
            dualDemosaicContrastUsed = p.bayersensor.dualDemosaicContrast;
            ctx.check(artgpu_dual_demosaic_bayer(ctx.get(), p.bayersensor.method, p.bayersensor.dualSecond, &raw, filters, initialGain, border, &dualDemosaicContrastUsed,
                                                 p.bayersensor.dualDemosaicAutoContrast ? 1 : 0, &out));
            return;
        }
        ctx.check(artgpu_demosaic_bayer(ctx.get(), p.bayersensor.method, &raw, filters, initialGain, border, &out));
    }
    double dualDemosaicContrastUsed = 0;
    // RawImageSource::getDeconvAutoRadius (deconvautoradius.cc:200-245) on rawData as preprocess left it: Bayer and monochrome (filters 0)
    // sensors; out == nullptr only asks whether the sensor is supported.  clipVal = (ri->get_white(1) - ri->get_cblack(1)) * scale_mul[1].
    bool getDeconvAutoRadius(float *out = nullptr)
    {
        if (isXtrans) return false;                                       // calcRadiusXtrans is not on the device path
        if (!out) return true;
        artgpu_plane raw = rawData.view();
        ctx.check(artgpu_deconv_auto_radius(ctx.get(), &raw, filters, 1000.f, deconvClipVal, out, nullptr));
        return true;
    }
    float deconvClipVal = 65535.f;
    void getFullSize(int &w, int &h) const { w = W - 2 * border; h = H - 2 * border; }   // computeFullSize (L1163-1193), tran = 0
    // RawImageSource::getImage (rawimagesource.cc:781-1104): tran = 0, skip = 1; rm/gm/bm as the caller computed them
    void getImage(const float mul[3], bool doClip, Imagefloat *image, int x = 0, int y = 0, int skip = 1)
    {
        artgpu_rgb planes{red.view(), green.view(), blue.view()};
        artgpu_rgb img = image->view();
        // PreviewProps(x, y, w, h, skip): transformRect adds the border; rm/gm/bm are divided by skip*skip (L922-926)
        const float area = float(skip) * float(skip);
        const float m[3] = {mul[0] / area, mul[1] / area, mul[2] / area};
        ctx.check(artgpu_get_image_skip(ctx.get(), &planes, x + border, y + border, skip, skip > 1 ? m : mul, doClip ? 1 : 0, nullptr, &img));
    }
    // RawImageSource::convertColorSpace, matrix branch (rawimagesource.cc:1128-1143,3184-3213)
    void convertColorSpace(Imagefloat *image, const double mat[9])
    {
        setColorMatrix(mat);
        artgpu_rgb img = image->view();
        ctx.check(artgpu_convert_color_space(ctx.get(), &img, mat));
    }
    // the camera -> working-space matrix convertColorSpace derives from params->icm (rawimagesource.cc:1128-1143); remembered
    // because ImProcFunctions::denoise applies it again to its quarter-size calclum copy (ipdenoise.cc:1131)
    void setColorMatrix(const double mat[9]) { for (int k = 0; k < 9; ++k) colorMatrix[k] = mat[k]; hasColorMatrix = true; }
    double colorMatrix[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    bool hasColorMatrix = false;
    Context &ctx;
    int W, H, border = 4;
    uint32_t filters;
    double initialGain;
    DevicePlane rawData, red, green, blue;
    bool isXtrans = false;
    int32_t xtrans[36] = {};
    float rgb_cam[12] = {};
};

// rtengine::ImProcFunctions counterpart
class ImProcFunctions {
public:
    enum class Stage { STAGE_0, STAGE_1, STAGE_2, STAGE_3 };
    enum class Pipeline { THUMBNAIL, NAVIGATOR, PREVIEW, OUTPUT };
    ImProcFunctions(Context &c, const ProcParams *p, double scale = 1.0) : ctx(c), params(p), scale(scale) {}

    // ImProcFunctions::process (improcfun.cc:567-641): same step order; steps that are disabled / identity in the
    // default ProcParams and not on the device path (DRC, impulse denoise, defringe, the DCP look) are
    // skipped here exactly as their `enabled == false` early-outs skip them.  STAGE_2 holds capture sharpening, its first step.
    bool process(Pipeline pipeline, Stage stage, Imagefloat *img)
    {
        cur_pipeline = pipeline;
        switch (stage) {
        case Stage::STAGE_0: dehaze(img); break;                                              // improcfun.cc:577
        case Stage::STAGE_1: channelMixer(img); exposure(img); hslEqualizer(img); toneEqualizer(img); break;   // improcfun.cc:581-588
        case Stage::STAGE_2: sharpening(img); impulsedenoise(img); defringe(img); colorCorrection(img); guidedSmoothing(img); break;   // improcfun.cc:595-602
        case Stage::STAGE_3:                                                                  // improcfun.cc:605-627 (the steps this library has)
            creativeGradients(img);                                                           // L605
            textureBoost(img); filmGrain(img); logEncoding(img); saturationVibrance(img);       // L606-611
            if (!params->filmSimulation.after_tone_curve) filmSimulation(img);                // L614-616
            toneCurve(img);
            if (params->filmSimulation.after_tone_curve) filmSimulation(img);                 // L618-620
            rgbCurves(img); labAdjustments(img); softLight(img); localContrast(img);          // L621-625
            blackAndWhite(img);                                                               // L627
            break;
        }
        return false;
    }
    Pipeline cur_pipeline = Pipeline::OUTPUT;
    // rtengine::generateMasks (masks.cc:1037-1516) over artgpu_generate_masks: the reference's arguments but the tool name and the linked-mask
    // manager (linked masks are not on the device path), the image's mode as ARTGPU_MASKS_MODE_*, and device planes for the results.  A null
    // entry of `masks` stands for a default Mask.  offset_x / offset_y place the shapes of the area mask, which the caller rasterised.  Returns
    // false where the reference does (a shown mask); what the library does not support throws through Context::check
    bool generateMasks(Imagefloat *rgb, int mode, const std::vector<const ProcParams::Mask *> &masks, int offset_x, int offset_y, int full_width, int full_height,
                       double scale_, int show_mask_idx, std::vector<std::unique_ptr<DevicePlane>> *Lmask, std::vector<std::unique_ptr<DevicePlane>> *abmask)
    {
        (void)offset_x; (void)offset_y;
        std::vector<artgpu_plane> areas;
        const std::vector<artgpu_mask_params> mp = ProcParams::maskParams(masks, areas, show_mask_idx);
        std::vector<artgpu_plane> lv, av;
        for (auto *set : {Lmask, abmask}) {
            if (!set) continue;
            set->clear();
            for (size_t k = 0; k < masks.size(); ++k) {
                set->emplace_back(new DevicePlane(rgb->getWidth(), rgb->getHeight()));
                (set == Lmask ? lv : av).push_back(set->back()->view());
            }
        }
        artgpu_rgb i = rgb->view();
        ctx.check(artgpu_generate_masks(ctx.get(), &i, mode, params->workingSpace, mp.data(), (int)mp.size(), full_width, full_height, scale_,
                                        Lmask ? lv.data() : nullptr, abmask ? av.data() : nullptr, nullptr));
        return true;
    }
    // ImProcFunctions::textureBoost (iptextureboost.cc:183-248): setMode(YUV), every enabled region with strength != 0 through texture_boost and
    // the mask blend on the Y plane; this mirror has no mode tracking and converts back at once (Imagefloat::yuv_to_rgb)
    bool textureBoost(Imagefloat *img)
    {
        if (!params->textureBoost.enabled) return false;
        std::vector<artgpu_plane> blends;
        std::vector<artgpu_texture_boost_region> regions = params->textureBoostRegions(blends);
        std::vector<const ProcParams::Mask *> masks;
        std::vector<std::unique_ptr<DevicePlane>> generated;
        std::vector<artgpu_plane> views(regions.size());
        if (ProcParams::regionMasks(params->textureBoost, masks)) {                      // iptextureboost.cc:210, on the RGB image
            generateMasks(img, ARTGPU_MASKS_MODE_RGB, masks, 0, 0, -1, -1, scale, -1, &generated, nullptr);
            for (size_t k = 0; k < regions.size(); ++k)
                if (masks[k]) { views[k] = generated[k]->view(); regions[k].mask = &views[k]; }
        }
        artgpu_rgb i = img->view();
        ctx.check(artgpu_texture_boost(ctx.get(), &i, regions.data(), (int)regions.size(), params->workingSpace, scale,
                                       (scale == 1 || cur_pipeline == Pipeline::OUTPUT) ? 1 : 0, 1, nullptr));
        return false;
    }
    // ImProcFunctions::colorCorrection (ipcolorcorrection.cc:39-866): generateMasks(rgb, ., &Lmask, &abmask) on the RGB image (L236), setMode(YUV),
    // every enabled region; this mirror has no mode tracking and converts back at once, like textureBoost above
    bool colorCorrection(Imagefloat *img)
    {
        if (!params->colorcorrection.enabled) return false;
        std::vector<artgpu_plane> blends;
        std::vector<artgpu_color_correction_region> regions = params->colorCorrectionRegions(blends);
        std::vector<const ProcParams::Mask *> masks;
        std::vector<std::unique_ptr<DevicePlane>> Lmask, abmask;
        std::vector<artgpu_plane> views(2 * regions.size());
        if (ProcParams::regionMasks(params->colorcorrection, masks)) {
            generateMasks(img, ARTGPU_MASKS_MODE_RGB, masks, 0, 0, -1, -1, scale, -1, &Lmask, &abmask);
            for (size_t k = 0; k < regions.size(); ++k)
                if (masks[k]) {
                    views[2 * k] = Lmask[k]->view(); views[2 * k + 1] = abmask[k]->view();
                    regions[k].lmask = &views[2 * k]; regions[k].abmask = &views[2 * k + 1];
                }
        }
        artgpu_rgb i = img->view();
        ctx.check(artgpu_color_correction(ctx.get(), &i, regions.data(), (int)regions.size(), params->workingSpace, params->workingSpaceInverse, 1, nullptr));
        return false;
    }
    // ImProcFunctions::guidedSmoothing (ipsmoothing.cc:902-1073), modes GUIDED and NLMEANS: generateMasks on the image (L929), setMode(RGB) -- a
    // no-op here, the mirror's tools hand back RGB --, every enabled region
    bool guidedSmoothing(Imagefloat *img)
    {
        if (!params->smoothing.enabled) return false;
        std::vector<artgpu_plane> blends;
        std::vector<artgpu_smoothing_region> regions = params->smoothingRegions(blends);
        std::vector<const ProcParams::Mask *> masks;
        std::vector<std::unique_ptr<DevicePlane>> generated;
        std::vector<artgpu_plane> views(regions.size());
        if (ProcParams::regionMasks(params->smoothing, masks)) {
            generateMasks(img, ARTGPU_MASKS_MODE_RGB, masks, 0, 0, -1, -1, scale, -1, &generated, nullptr);
            for (size_t k = 0; k < regions.size(); ++k)
                if (masks[k]) { views[k] = generated[k]->view(); regions[k].mask = &views[k]; }
        }
        artgpu_rgb i = img->view();
        ctx.check(artgpu_smoothing(ctx.get(), &i, regions.data(), (int)regions.size(), params->workingSpace, scale, nullptr));
        return false;
    }
    // ImProcFunctions::toneEqualizer (iptoneequalizer.cc:345-371).  show_colormap only exists in the PREVIEW pipeline (L365) and is not on the device
    // path: elsewhere the flag is dropped as the reference drops it, there the library refuses it
    bool toneEqualizer(Imagefloat *img)
    {
        if (!params->toneEqualizer.enabled) return false;
        artgpu_tone_equalizer_params tp = params->toneEqualizerParams();
        tp.show_colormap = tp.show_colormap && cur_pipeline == Pipeline::PREVIEW;
        artgpu_rgb i = img->view();
        ctx.check(artgpu_tone_equalizer(ctx.get(), &i, &tp, params->workingSpace, scale, nullptr));
        return false;
    }
    // ImProcFunctions::filmSimulation (ipfilmsim.cc:33-73) with a HaldCLUT; the image is in RGB mode at both of its positions.  A missing handle is the
    // reference's "file could not be read": the step does nothing (its listener message stays with the application)
    void filmSimulation(Imagefloat *img)
    {
        if (!params->filmSimulation.enabled || !params->filmSimulation.clut) return;
        const artgpu_film_simulation_params fp = params->filmSimulationParams();
        artgpu_rgb i = img->view();
        ctx.check(artgpu_film_simulation(ctx.get(), &i, params->filmSimulation.clut, &fp));
    }
    // ImProcFunctions::filmGrain (ipgrain.cc:88-98): guidedSmoothing over the NOISE regions it derives; the reference adds noise in the OUTPUT and
    // PREVIEW pipelines only (ipsmoothing.cc:990), elsewhere the regions' blend and the normalise round trip is all that happens -- not on the device path
    void filmGrain(Imagefloat *img)
    {
        if (!params->grain.enabled || (cur_pipeline != Pipeline::OUTPUT && cur_pipeline != Pipeline::PREVIEW)) return;
        const artgpu_film_grain_params gp = params->grainParams();
        artgpu_rgb i = img->view();
        ctx.check(artgpu_film_grain(ctx.get(), &i, &gp, params->workingSpace, scale, cur_pipeline == Pipeline::OUTPUT ? 1 : 0, nullptr));
    }
    // ImProcFunctions::creativeGradients (iptransform.cc:1390-1408) with the viewport members below (full_width 0 = the image's own size, the
    // reference's -1)
    void creativeGradients(Imagefloat *img)
    {
        const bool own = full_width <= 0 || full_height <= 0;
        const artgpu_creative_gradients_params cp = params->creativeGradientsParams(offset_x, offset_y, own ? -1 : full_width, own ? -1 : full_height, scale);
        artgpu_rgb i = img->view();
        ctx.check(artgpu_creative_gradients(ctx.get(), &i, &cp));
    }
    // ImProcFunctions::softLight (ipsoftlight.cc:46-82)
    void softLight(Imagefloat *img)
    {
        const artgpu_soft_light_params sp = params->softLightParams();
        artgpu_rgb i = img->view();
        ctx.check(artgpu_soft_light(ctx.get(), &i, &sp));
    }
    // ImProcFunctions::blackAndWhite (ipbw.cc:214-365).  The mirror's images are in RGB mode between calls, so a colour cast comes back as RGB
    void blackAndWhite(Imagefloat *img)
    {
        const artgpu_black_and_white_params bp = params->blackAndWhiteParams();
        artgpu_rgb i = img->view();
        ctx.check(artgpu_black_and_white(ctx.get(), &i, &bp, params->workingSpace));
    }
    // ImProcFunctions::resizeScale (ipresize.cc:226-297) without a crop
    static float resizeScale(const ProcParams *params, int fw, int fh, int &imw, int &imh)
    {
        float s = 1.f;
        const artgpu_resize_params rp = params ? params->resizeParams() : artgpu_resize_params{};
        (void)artgpu_resize_scale(params ? &rp : nullptr, fw, fh, &imw, &imh, &s);
        return s;
    }
    // ImProcFunctions::Lanczos (ipresize.cc:53-223).  The mirror's images are in RGB mode between calls (localContrast switches back), so this is
    // always the reference's setMode(LAB) / resample / setMode(RGB); src is left as the reference leaves it, in LAB mode.  The pipe
    // (artgpu_set_pipeline_resize) keeps the reference's lazy mode behind localContrast instead
    void Lanczos(Imagefloat *src, Imagefloat *dst, float scale_)
    {
        artgpu_rgb s = src->view(), d = dst->view();
        ctx.check(artgpu_resize_lanczos(ctx.get(), &s, &d, scale_, ARTGPU_RESIZE_RGB, params->workingSpace, params->workingSpaceInverse));
    }
    void resize(Imagefloat *src, Imagefloat *dst, float dScale) { Lanczos(src, dst, dScale); }
    // ImProcFunctions::dehaze (ipdehaze.cc:306-512)
    void dehaze(Imagefloat *img)
    {
        if (!params->dehaze.enabled) return;
        const artgpu_dehaze_params dp = params->dehazeParams();
        artgpu_rgb i = img->view();
        ctx.check(artgpu_dehaze(ctx.get(), &i, &dp, params->workingSpace, scale, nullptr));
    }
    // ImProcFunctions::sharpening (ipsharpen.cc:791-794 -> doSharpening L712-788), method rld; the radius is params->sharpening.deconvradius, which
    // the caller replaces by RawImageSource::getDeconvAutoRadius's when deconvAutoRadius is set (simpleprocess.cc:274-278)
    bool sharpening(Imagefloat *img)
    {
        if (!params->sharpening.enabled) return false;
        const artgpu_sharpening_params sp = params->sharpeningParams(offset_x, offset_y, full_width, full_height);
        artgpu_rgb i = img->view();
        ctx.check(artgpu_sharpening(ctx.get(), &i, &sp, params->workingSpace, scale, nullptr));
        return false;
    }
    // ImProcFunctions::impulsedenoise (impulse_denoise.cc:179-189) and ::defringe (PF_correct_RT.cc:210-218), the tools behind the sharpening in STAGE_2.  The
    // reference leaves the image in LAB mode for the next tool's setMode; this mirror has no mode tracking and converts back at once (like labAdjustments)
    void impulsedenoise(Imagefloat *img)
    {
        if (!params->impulseDenoise.enabled) return;
        const artgpu_impulse_denoise_params ip = params->impulseDenoiseParams();
        artgpu_rgb i = img->view();
        ctx.check(artgpu_impulse_denoise(ctx.get(), &i, &ip, params->workingSpace, params->workingSpaceInverse, scale, 1, nullptr));
    }
    void defringe(Imagefloat *img)
    {
        if (!params->defringe.enabled) return;
        const artgpu_defringe_params dp = params->defringeParams();
        artgpu_rgb i = img->view();
        ctx.check(artgpu_defringe(ctx.get(), &i, &dp, params->workingSpace, params->workingSpaceInverse, scale, 0, 1, nullptr));
    }
    int offset_x = 0, offset_y = 0;    // with full_width / full_height (logEncoding): where the image lies in the full frame (improcfun.h setViewport)
    // ImProcFunctions::channelMixer (ipchmixer.cc:152-234), RGB_MATRIX mode: the nine percentages / 1000 (L185-199)
    void channelMixer(Imagefloat *img)
    {
        if (!params->chmixer.enabled) return;
        float m[9];
        for (int k = 0; k < 3; ++k) { m[k] = params->chmixer.red[k] / 1000.f; m[3 + k] = params->chmixer.green[k] / 1000.f; m[6 + k] = params->chmixer.blue[k] / 1000.f; }
        artgpu_rgb i = img->view();
        ctx.check(artgpu_channel_mixer(ctx.get(), &i, m));
    }
    // ImProcFunctions::hslEqualizer (iphsl.cc:29-221); leaves the image in YUV mode like the reference unless the caller's Imagefloat
    // has no mode tracking (this mirror's has none: planes are converted back to RGB)
    void hslEqualizer(Imagefloat *img)
    {
        const auto &p = params->hsl;
        if (!p.enabled) return;
        artgpu_rgb i = img->view();
        ctx.check(artgpu_hsl_equalizer(ctx.get(), &i, p.hCurve.empty() ? nullptr : p.hCurve.data(), (int)p.hCurve.size(), p.sCurve.empty() ? nullptr : p.sCurve.data(),
                                       (int)p.sCurve.size(), p.lCurve.empty() ? nullptr : p.lCurve.data(), (int)p.lCurve.size(), p.smoothing, params->workingSpace, scale, 1));
    }
    // ImProcFunctions::logEncoding (iplogenc.cc:395-402); full_width/full_height as set by ImProcFunctions::setViewport (0 = the image itself)
    int full_width = 0, full_height = 0;
    void logEncoding(Imagefloat *img)
    {
        const auto &p = params->logenc;
        if (!p.enabled) return;
        artgpu_logenc_params lp = {1, p.regularization, p.satcontrol ? 1 : 0, p.highlightCompression, p.gain, p.targetGray, p.blackEv, p.whiteEv};
        artgpu_rgb i = img->view();
        ctx.check(artgpu_log_encoding(ctx.get(), &i, &lp, params->workingSpace, full_width, full_height));
    }
    // ImProcFunctions::labAdjustments (iplabadjustments.cc:277-345): setMode(LAB), hist16 when contrast != 0, the caller's curve builders,
    // the curve loop; the reference leaves the image in LAB mode for the next step's setMode -- this mirror has no mode tracking and
    // converts back at once (Imagefloat::lab_to_rgb)
    void labAdjustments(Imagefloat *img)
    {
        const auto &p = params->labCurve;
        if (!p.enabled || !p.curves) return;
        artgpu_rgb i = img->view();
        ctx.check(artgpu_rgb_to_lab(ctx.get(), &i, params->workingSpace));
        std::vector<uint32_t> hist16;
        if (p.contrast != 0) { hist16.resize(65536); ctx.check(artgpu_lab_histogram(ctx.get(), &i, hist16.data())); }
        std::vector<float> lc, ac, bc;
        p.curves(hist16.empty() ? nullptr : hist16.data(), lc, ac, bc);
        if (lc.size() != 32770 || ac.size() != 65536 || bc.size() != 65536) throw std::runtime_error("labAdjustments: curve LUT sizes");
        ctx.check(artgpu_lab_adjustments(ctx.get(), &i, lc.data(), ac.data(), bc.data(), (p.chromaticity + 100.0f) / 100.0f));
        ctx.check(artgpu_lab_to_rgb(ctx.get(), &i, params->workingSpaceInverse));
    }
    // ImProcFunctions::localContrast (iplocalcontrast.cc:425-487): setMode(LAB), every enabled region through local_contrast_wavelets and the
    // mask blend on the L plane (Imagefloat::g); like labAdjustments this mirror converts back at once.  An empty or FCT_Linear curve takes
    // the default region's (L358-363); a curve whose LUT stays unset (identity) reads as 0 (L53-56)
    bool localContrast(Imagefloat *img)
    {
        const auto &p = params->localContrast;
        if (!p.enabled) return false;
        std::vector<std::vector<float>> luts(p.regions.size(), std::vector<float>(501));
        std::vector<artgpu_plane> blends(p.regions.size());
        std::vector<artgpu_local_contrast_region> regions;
        for (size_t k = 0; k < p.regions.size(); ++k) {
            if (k < p.masks.size() && !p.masks[k].enabled) continue;
            const ProcParams::LocalContrastRegion dflt;
            const auto &r = p.regions[k];
            const std::vector<double> &curve = (r.curve.empty() || r.curve[0] == 0 /*FCT_Linear*/) ? dflt.curve : r.curve;
            int is_set = 0;
            ctx.check(artgpu_local_contrast_curve_lut(curve.data(), (int)curve.size(), luts[k].data(), &is_set));
            artgpu_local_contrast_region reg{r.contrast, is_set ? luts[k].data() : nullptr, nullptr};
            if (k < p.masks.size() && p.masks[k].blend) { blends[k] = p.masks[k].blend->view(); reg.mask = &blends[k]; }
            regions.push_back(reg);
        }
        artgpu_rgb i = img->view();
        ctx.check(artgpu_rgb_to_lab(ctx.get(), &i, params->workingSpace));
        std::vector<const ProcParams::Mask *> masks;
        std::vector<std::unique_ptr<DevicePlane>> generated;
        std::vector<artgpu_plane> views(regions.size());
        if (ProcParams::regionMasks(p, masks)) {                                        // iplocalcontrast.cc:454, on the LAB image
            generateMasks(img, ARTGPU_MASKS_MODE_LAB, masks, 0, 0, -1, -1, scale, -1, &generated, nullptr);
            for (size_t k = 0; k < regions.size(); ++k)
                if (masks[k]) { views[k] = generated[k]->view(); regions[k].mask = &views[k]; }
        }
        ctx.check(artgpu_local_contrast(ctx.get(), &i.g, regions.data(), (int)regions.size(), scale, nullptr));
        ctx.check(artgpu_lab_to_rgb(ctx.get(), &i, params->workingSpaceInverse));
        return false;
    }
    // ImProcFunctions::saturationVibrance (ipsaturation.cc:43-83)
    void saturationVibrance(Imagefloat *img)
    {
        if (!params->saturation.enabled) return;
        artgpu_rgb i = img->view();
        ctx.check(artgpu_saturation_vibrance(ctx.get(), &i, params->saturation.saturation, params->saturation.vibrance, params->workingSpace));
    }
    // ImProcFunctions::rgbCurves (iprgbcurves.cc:30-148): the three 65536-entry outCurve LUTs are built by the caller (RGBCurve, L41-53)
    void rgbCurves(Imagefloat *img)
    {
        const auto &p = params->rgbCurves;
        if (!p.enabled) return;
        artgpu_rgb i = img->view();
        ctx.check(artgpu_rgb_curves(ctx.get(), &i, p.rlut.size() == 65536 ? p.rlut.data() : nullptr, p.glut.size() == 65536 ? p.glut.data() : nullptr,
                                    p.blut.size() == 65536 ? p.blut.data() : nullptr));
    }
    // ImProcFunctions::exposure -> expcomp (ipexposure.cc:28-79)
    void exposure(Imagefloat *img) { expcomp(img, params->exposure.expcomp, params->exposure.black, params->exposure.enabled); }
    void expcomp(Imagefloat *img, double ec, double black, bool enabled)
    {
        if (!enabled) return;
        const float exp_scale = (float)std::pow(2.0, ec);          // pow(2.f, double) promotes (ipexposure.cc:40)
        const float blk = (float)(black * 2000.0);
        artgpu_rgb i = img->view();
        ctx.check(artgpu_exposure(ctx.get(), &i, exp_scale, blk));
    }
    // ImProcFunctions::toneCurve (iptonecurve.cc:553-716): single STD curve, LINEAR base curve
    void toneCurve(Imagefloat *img)
    {
        if (!params->toneCurve.enabled) return;
        artgpu_rgb i = img->view();
        const float *lut = params->toneCurve.lut.size() == 65536 ? params->toneCurve.lut.data() : nullptr;
        if (params->toneCurve.curveMode == ARTGPU_TONE_NEUTRAL) {
            // single NEUTRAL curve: no filmlike_clip pre-pass (iptonecurve.cc:586-595), apply_tc(NEUTRAL) with basecurve == nullptr
            artgpu_neutral_state st;
            for (int k = 0; k < 9; ++k) { st.ws[k] = params->workingSpace[k]; st.iws[k] = params->workingSpaceInverse[k]; st.to_out[k] = params->toOut[k]; st.to_work[k] = params->toWork[k]; }
            ctx.check(artgpu_tone_curve_neutral(ctx.get(), &i, lut, params->toneCurve.whitePoint, &st));
            return;
        }
        ctx.check(artgpu_tone_curve(ctx.get(), &i, params->toneCurve.curveMode, lut, params->toneCurve.whitePoint, params->toneCurve.basecurveLinear ? 1 : 0));
    }
    // DenoiseInfoStore (improcfun.h:117-131)
    struct DenoiseInfoStore : artgpu_denoise_info_store {
        DenoiseInfoStore() { reset(); }
        void reset() { *static_cast<artgpu_denoise_info_store *>(this) = artgpu_denoise_info_store{}; }
    };
    // ImProcFunctions::denoiseComputeParams (ipdenoise.cc:800-1093): AUTOMATIC chrominance from nine crops of the sensor planes.
    // The reference pulls rm/gm/bm and the camera matrix out of imgsrc/currWB/params->icm; here the caller hands in the
    // multipliers and must have called imgsrc->setColorMatrix().
    void denoiseComputeParams(RawImageSource *imgsrc, const float mul[3], bool doClip, DenoiseInfoStore &store, decltype(ProcParams::denoise) &dnparams)
    {
        artgpu_denoise_params dn{dnparams.luminance, dnparams.luminanceDetail, dnparams.luminanceDetailThreshold, dnparams.chrominance,
                                 dnparams.chrominanceRedGreen, dnparams.chrominanceBlueYellow, dnparams.gamma, dnparams.aggressive ? 1 : 0,
                                 dnparams.colorSpace, dnparams.chrominanceMethod};
        artgpu_rgb planes{imgsrc->red.view(), imgsrc->green.view(), imgsrc->blue.view()};
        ctx.check(artgpu_denoise_compute_params(ctx.get(), &planes, imgsrc->border, mul, doClip ? 1 : 0, imgsrc->colorMatrix, params->workingSpace,
                                                dnparams.chrominanceAutoFactor, &store, &dn));
        dnparams.chrominance = dn.chrominance; dnparams.chrominanceRedGreen = dn.chrominance_red_green; dnparams.chrominanceBlueYellow = dn.chrominance_blue_yellow;
    }
    // ImProcFunctions::denoise (ipdenoise.cc:1096-1189): calclum/ccalc chroma noise map with the fixed noise curve
    // (L1139-1149), exposure pre-compensation, RGB_denoise, guided smoothing + NL-means, post-compensation.
    void denoise(RawImageSource *imgsrc, Imagefloat *img)
    {
        const auto &d = params->denoise;
        if (!d.enabled) return;
        const double ecomp = params->exposure.enabled ? params->exposure.expcomp : 0.0;
        artgpu_denoise_tool_params tp{{d.luminance, d.luminanceDetail, d.luminanceDetailThreshold, d.chrominance, d.chrominanceRedGreen,
                                       d.chrominanceBlueYellow, d.gamma, d.aggressive ? 1 : 0, d.colorSpace, d.chrominanceMethod},
                                      d.smoothingEnabled ? 1 : 0, d.guidedChromaRadius, d.nlStrength, d.nlDetail};
        static const double curve_points[9] = {1 /*FCT_MinMaxCPoints*/, 0.05, 0.50, 0.35, 0.35, 0.35, 0.05, 0.35, 0.35};
        float curve[501], sum = 0.f;
        ctx.check(artgpu_noise_curve_lut(curve_points, 9, curve, &sum));
        artgpu_rgb i = img->view();
        ctx.check(artgpu_improc_denoise(ctx.get(), &i, &tp, params->workingSpace, params->workingSpaceInverse, ecomp, scale, imgsrc && imgsrc->hasColorMatrix ? imgsrc->colorMatrix : nullptr,
                                        curve, 0u));
    }
    Context &ctx;
    const ProcParams *params;
    double scale;
};

// The batch queue's loop (rtengine/simpleprocess.cc:586-612 batchProcessingThread: one ImageProcessor per job, jobs share nothing) between
// the decoder's and the writers' formats: uint16 sensor data in, the scanlines Imagefloat::getScanline hands the TIFF / PNG writers out
// (artgpu_batch_run_io).  Buffers are pinned (hipHostMalloc) so that a job's upload and download run beside its neighbours' kernels.
class BatchQueue {
public:
    struct Job {
        uint16_t *sensor = nullptr;      // W x H, pinned
        unsigned char *scanlines = nullptr;   // outH x outW x 3 x bps / 8, pinned
        int W = 0, H = 0;
        int outW = 0, outH = 0;               // (W - 2 border) x (H - 2 border), or what the Resize tool makes of it
        float chmax[4] = {0, 0, 0, 0};
        int status = 0;
    };
    BatchQueue(Context &c, int bps = 16) : ctx(c), bps(bps) {}
    ~BatchQueue() { for (Job &j : jobs) { if (j.sensor) (void)hipHostFree(j.sensor); if (j.scanlines) (void)hipHostFree(j.scanlines); } }
    BatchQueue(const BatchQueue &) = delete;
    BatchQueue &operator=(const BatchQueue &) = delete;
    // a job's buffers; the caller fills `sensor` (the decoder's output).  p: the parameters process() will get, for the Resize tool's output size
    // (simpleprocess.cc:402-407)
    Job &addJob(int W, int H, int border, const ProcParams *p = nullptr)
    {
        Job j; j.W = W; j.H = H; j.outW = W - 2 * border; j.outH = H - 2 * border;
        if (p && p->resize.enabled) {
            int imw, imh;
            const float s = ImProcFunctions::resizeScale(p, j.outW, j.outH, imw, imh);
            if (s < 1.f || (s > 1.f && (p->resize.allowUpscaling || p->resize.dataspec == 0))) { j.outW = imw; j.outH = imh; }
        }
        hipcheck(hipHostMalloc(reinterpret_cast<void **>(&j.sensor), (size_t)W * H * 2, hipHostMallocDefault), "hipHostMalloc(sensor)");
        hipcheck(hipHostMalloc(reinterpret_cast<void **>(&j.scanlines), (size_t)j.outW * 3 * (bps / 8) * (size_t)j.outH, hipHostMallocDefault), "hipHostMalloc(scanlines)");
        jobs.push_back(j);
        return jobs.back();
    }
    size_t rowBytes(int W, int border) const { return (size_t)(W - 2 * border) * 3 * (bps / 8); }
    // ImageProcessor::operator() for every job: stage_init (scaleColors + demosaic), stage_denoise, stage_finish up to the tone curve, then the
    // output profile's matrix (identity here: the working space is the output space) and getScanline
    void process(const ProcParams &p, uint32_t filters, const float mul[3], const double cam2work[9], int lanes,
                 const float cblacksom[4], const float scale_mul[4])
    {
        artgpu_pipeline_params pp = {};
        pp.sensor = 0; pp.bayer_method = p.bayersensor.method; pp.filters = filters; pp.initial_gain = 1.0; pp.xtrans_passes = 3; pp.border = p.bayersensor.border;
        for (int k = 0; k < 3; ++k) pp.mul[k] = mul[k];
        pp.do_clip = 1; pp.has_cam_to_work = 1;
        for (int k = 0; k < 9; ++k) { pp.cam_to_work[k] = cam2work[k]; pp.ws[k] = p.workingSpace[k]; pp.iws[k] = p.workingSpaceInverse[k]; pp.to_out[k] = p.toOut[k]; pp.to_work[k] = p.toWork[k]; }
        const auto &d = p.denoise;
        pp.denoise_enabled = d.enabled ? 1 : 0;
        pp.denoise = artgpu_denoise_tool_params{{d.luminance, d.luminanceDetail, d.luminanceDetailThreshold, d.chrominance, d.chrominanceRedGreen, d.chrominanceBlueYellow,
                                                 d.gamma, d.aggressive ? 1 : 0, d.colorSpace, d.chrominanceMethod},
                                                d.smoothingEnabled ? 1 : 0, d.guidedChromaRadius, d.nlStrength, d.nlDetail};
        pp.exposure_enabled = p.exposure.enabled ? 1 : 0; pp.expcomp = p.exposure.expcomp; pp.black = p.exposure.black;
        pp.tone_enabled = p.toneCurve.enabled ? 1 : 0; pp.tone_mode = p.toneCurve.curveMode; pp.tone_lut = p.toneCurve.lut.data(); pp.white_point = p.toneCurve.whitePoint;
        pp.scale = 1.0; pp.chrominance_auto_factor = d.chrominanceAutoFactor;
        pp.ca_enabled = p.raw.enable_ca ? 1 : 0; pp.ca = p.caParams();    // the library applies the call site's condition per frame
        pp.dehaze_enabled = p.dehaze.enabled ? 1 : 0; pp.dehaze = p.dehazeParams();
        pp.sharpening_enabled = p.sharpening.enabled ? 1 : 0; pp.sharpening = p.sharpeningParams();
        pp.sharpening_auto_radius = p.sharpening.deconvAutoRadius ? 1 : 0; pp.sharpening_clip_val = (65535.f - cblacksom[1]) * scale_mul[1];
        std::vector<artgpu_plane> tb_blends;
        const std::vector<artgpu_texture_boost_region> tb_regions = p.textureBoostRegions(tb_blends);
        pp.texture_boost_enabled = p.textureBoost.enabled ? 1 : 0; pp.texture_boost_nregions = (int32_t)tb_regions.size(); pp.texture_boost_regions = tb_regions.data();
        // regions that carry Masks: the pipe generates the tool's planes itself (a region without one gets a default Mask)
        std::vector<const ProcParams::Mask *> tb_masks;
        std::vector<artgpu_plane> tb_areas;
        std::vector<artgpu_mask_params> tb_mp;
        if (ProcParams::regionMasks(p.textureBoost, tb_masks)) tb_mp = ProcParams::maskParams(tb_masks, tb_areas);
        ctx.check(artgpu_set_pipeline_masks(ctx.get(), nullptr, 0, tb_mp.empty() ? nullptr : tb_mp.data(), (int)tb_mp.size()));
        // ImProcFunctions::impulsedenoise and ::defringe behind the sharpening
        const artgpu_impulse_denoise_params imp = p.impulseDenoiseParams();
        const artgpu_defringe_params dfp = p.defringeParams();
        ctx.check(artgpu_set_pipeline_impulse_defringe(ctx.get(), p.impulseDenoise.enabled ? &imp : nullptr, p.defringe.enabled ? &dfp : nullptr));
        // ImProcFunctions::colorCorrection behind them: the regions (and their Masks, generated by the pipe) as a setting of the context
        std::vector<artgpu_plane> cc_blends, cc_areas;
        std::vector<artgpu_color_correction_region> cc_regions;
        std::vector<const ProcParams::Mask *> cc_masks;
        std::vector<artgpu_mask_params> cc_mp;
        if (p.colorcorrection.enabled) {
            cc_regions = p.colorCorrectionRegions(cc_blends);
            if (ProcParams::regionMasks(p.colorcorrection, cc_masks)) cc_mp = ProcParams::maskParams(cc_masks, cc_areas);
        }
        ctx.check(artgpu_set_pipeline_color_correction(ctx.get(), cc_regions.empty() ? nullptr : cc_regions.data(), (int)cc_regions.size(),
                                                       cc_mp.empty() ? nullptr : cc_mp.data()));
        // ImProcFunctions::guidedSmoothing behind it, likewise
        std::vector<artgpu_plane> sm_blends, sm_areas;
        std::vector<artgpu_smoothing_region> sm_regions;
        std::vector<const ProcParams::Mask *> sm_masks;
        std::vector<artgpu_mask_params> sm_mp;
        if (p.smoothing.enabled) {
            sm_regions = p.smoothingRegions(sm_blends);
            if (ProcParams::regionMasks(p.smoothing, sm_masks)) sm_mp = ProcParams::maskParams(sm_masks, sm_areas);
        }
        ctx.check(artgpu_set_pipeline_smoothing(ctx.get(), sm_regions.empty() ? nullptr : sm_regions.data(), (int)sm_regions.size(),
                                                sm_mp.empty() ? nullptr : sm_mp.data()));
        // ImProcFunctions::toneEqualizer behind the exposure (the batch queue is the OUTPUT pipeline: no colour map)
        artgpu_tone_equalizer_params te = p.toneEqualizerParams();
        te.show_colormap = 0;
        ctx.check(artgpu_set_pipeline_tone_equalizer(ctx.get(), p.toneEqualizer.enabled ? &te : nullptr));
        // ImProcFunctions::filmSimulation on either side of the tone curve
        const artgpu_film_simulation_params fs = p.filmSimulationParams();
        const bool fs_on = p.filmSimulation.enabled && p.filmSimulation.clut;
        ctx.check(artgpu_set_pipeline_film_simulation(ctx.get(), fs_on ? p.filmSimulation.clut : nullptr, &fs, p.filmSimulation.after_tone_curve ? 1 : 0));
        // ImProcFunctions::filmGrain behind texture boost
        const artgpu_film_grain_params fg = p.grainParams();
        ctx.check(artgpu_set_pipeline_film_grain(ctx.get(), p.grain.enabled ? &fg : nullptr));
        // ImProcFunctions::creativeGradients ahead of texture boost, softLight behind the tone curve, blackAndWhite behind local contrast
        const artgpu_creative_gradients_params cgp = p.creativeGradientsParams(0, 0, -1, -1, 1.0);
        ctx.check(artgpu_set_pipeline_creative_gradients(ctx.get(), p.gradient.enabled || p.pcvignette.enabled ? &cgp : nullptr));
        const artgpu_soft_light_params slp = p.softLightParams();
        ctx.check(artgpu_set_pipeline_soft_light(ctx.get(), p.softlight.enabled ? &slp : nullptr));
        const artgpu_black_and_white_params bwp = p.blackAndWhiteParams();
        ctx.check(artgpu_set_pipeline_black_and_white(ctx.get(), p.blackwhite.enabled ? &bwp : nullptr));
        // ImProcFunctions::resize behind STAGE_3 (the jobs' scanline buffers have the size addJob derived from the same parameters)
        const artgpu_resize_params rs = p.resizeParams();
        ctx.check(artgpu_set_pipeline_resize(ctx.get(), p.resize.enabled ? &rs : nullptr));
        std::vector<artgpu_sensor_frame> in(jobs.size());
        std::vector<artgpu_scanline_frame> out(jobs.size());
        for (size_t k = 0; k < jobs.size(); ++k) {
            const Job &j = jobs[k];
            in[k] = artgpu_sensor_frame{j.sensor, j.W, j.H, (int64_t)j.W * 2, 1, 0, {cblacksom[0], cblacksom[1], cblacksom[2], cblacksom[3]},
                                        {scale_mul[0], scale_mul[1], scale_mul[2], scale_mul[3]}};
            out[k] = artgpu_scanline_frame{};
            out[k].scanlines = j.scanlines; out[k].row_stride_bytes = (int64_t)j.outW * 3 * (bps / 8); out[k].bps = bps; out[k].is_float = 0;
            out[k].rgb2out_enabled = 0; out[k].trc_linear = 1;
        }
        ctx.check(artgpu_set_batch_lanes(ctx.get(), lanes));
        const int rc = artgpu_batch_run_io(ctx.get(), (int)jobs.size(), in.data(), &pp, out.data());
        (void)artgpu_set_pipeline_masks(ctx.get(), nullptr, 0, nullptr, 0);
        (void)artgpu_set_pipeline_impulse_defringe(ctx.get(), nullptr, nullptr);
        (void)artgpu_set_pipeline_color_correction(ctx.get(), nullptr, 0, nullptr);
        (void)artgpu_set_pipeline_smoothing(ctx.get(), nullptr, 0, nullptr);
        (void)artgpu_set_pipeline_tone_equalizer(ctx.get(), nullptr);
        (void)artgpu_set_pipeline_film_simulation(ctx.get(), nullptr, nullptr, 0);
        (void)artgpu_set_pipeline_film_grain(ctx.get(), nullptr);
        (void)artgpu_set_pipeline_resize(ctx.get(), nullptr);
        (void)artgpu_set_pipeline_creative_gradients(ctx.get(), nullptr);
        (void)artgpu_set_pipeline_soft_light(ctx.get(), nullptr);
        (void)artgpu_set_pipeline_black_and_white(ctx.get(), nullptr);
        for (size_t k = 0; k < jobs.size(); ++k) { jobs[k].status = out[k].status; for (int c = 0; c < 4; ++c) jobs[k].chmax[c] = out[k].chmax[c]; }
        ctx.check(rc);
    }
    std::vector<Job> jobs;
    Context &ctx;
    int bps;
};

} // namespace artgpu_host
