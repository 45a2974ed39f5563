"""ctypes binding of ``libartgpu.so`` (the C ABI in ``include/artgpu.h``).

This is plumbing for the tests and ``bench.py``: device memory comes from torch (ROCm),
pointers and sizes go straight through the C ABI, the same entry points a C++ adapter inside
ART would call.  No CPU fallback: if the library is missing, import fails.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ARTGPU_LIB", os.path.join(_HERE, "libartgpu.so"))  # ARTGPU_LIB: kernel-variant experiments

BAYER_AMAZE = 0
BAYER_RCD = 1
BAYER_VNG4 = 2
DUAL_BILINEAR = 0
DUAL_VNG4 = 1


class Plane(C.Structure):
    _fields_ = [("p", C.c_void_p), ("w", C.c_int32), ("h", C.c_int32),
                ("row_stride_bytes", C.c_int64), ("on_device", C.c_int32)]


class RGB(C.Structure):
    _fields_ = [("r", Plane), ("g", Plane), ("b", Plane)]


class Timings(C.Structure):
    _fields_ = [("demosaic_ms", C.c_float), ("border_ms", C.c_float), ("total_ms", C.c_float)]


class DenoiseParams(C.Structure):
    _fields_ = [("luminance", C.c_double), ("luminance_detail", C.c_double), ("luminance_detail_threshold", C.c_int32),
                ("chrominance", C.c_double), ("chrominance_red_green", C.c_double), ("chrominance_blue_yellow", C.c_double),
                ("gamma", C.c_double), ("aggressive", C.c_int32), ("color_space", C.c_int32), ("chrominance_method", C.c_int32)]


class LogEncParams(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("regularization", C.c_int32), ("satcontrol", C.c_int32), ("highlight_compression", C.c_int32),
                ("gain", C.c_double), ("target_gray", C.c_double), ("black_ev", C.c_double), ("white_ev", C.c_double)]


class DenoiseInfoStore(C.Structure):
    """DenoiseInfoStore (improcfun.h:117-131) + per-crop diagnostics"""
    _fields_ = [("valid", C.c_int32), ("ch_M", C.c_float * 9), ("max_r", C.c_float * 9), ("max_b", C.c_float * 9),
                ("chrominance", C.c_double), ("chrominance_red_green", C.c_double), ("chrominance_blue_yellow", C.c_double),
                ("crop_info", (C.c_float * 16) * 9)]


class NeutralState(C.Structure):
    _fields_ = [("ws", C.c_double * 9), ("iws", C.c_double * 9), ("to_out", C.c_float * 9), ("to_work", C.c_float * 9)]


class CaParams(C.Structure):
    """artgpu_ca_params: RAWParams' CA correction fields"""
    _fields_ = [("autocorrect", C.c_int32), ("iterations", C.c_int32), ("red", C.c_double), ("blue", C.c_double),
                ("avoid_colour_shift", C.c_int32)]


class LocalContrastRegion(C.Structure):
    """artgpu_local_contrast_region: one LocalContrastParams::Region, its curve as the 501-entry LUT, its blend mask"""
    _fields_ = [("contrast", C.c_double), ("curve", C.POINTER(C.c_float)), ("mask", C.POINTER(Plane))]


class LocalContrastInfo(C.Structure):
    _fields_ = [("nlevels", C.c_int32), ("ave", C.c_float), ("min0", C.c_float), ("max0", C.c_float),
                ("mean", C.c_float * 10), ("sigma", C.c_float * 10), ("maxp", C.c_float * 10)]


class DehazeParams(C.Structure):
    """artgpu_dehaze_params: DehazeParams, the strength curve as FlatCurve points"""
    _fields_ = [("enabled", C.c_int32), ("strength", C.POINTER(C.c_double)), ("nstrength", C.c_int32), ("show_depth_map", C.c_int32),
                ("depth", C.c_int32), ("luminance", C.c_int32), ("blackpoint", C.c_int32)]


class DehazeInfo(C.Structure):
    _fields_ = [("haze_detected", C.c_int32), ("patchsize", C.c_int32), ("small_w", C.c_int32), ("small_h", C.c_int32),
                ("maxval", C.c_float), ("black", C.c_float * 3), ("ambient", C.c_float * 3), ("max_t", C.c_float), ("t0", C.c_float)]


class TextureBoostRegion(C.Structure):
    """artgpu_texture_boost_region: one TextureBoostParams::Region and its blend mask"""
    _fields_ = [("strength", C.c_double), ("detail_threshold", C.c_double), ("iterations", C.c_int32), ("mask", C.POINTER(Plane))]


class TextureBoostInfo(C.Structure):
    _fields_ = [("radius", C.c_int32), ("isguided", C.c_int32), ("rescaled", C.c_int32), ("work_w", C.c_int32), ("work_h", C.c_int32),
                ("kernel_size", C.c_int32), ("minval", C.c_float), ("strength", C.c_float), ("strength2", C.c_float)]


class ColorCorrectionRegion(C.Structure):
    """artgpu_color_correction_region: one ColorCorrectionParams::Region and its two blend planes"""
    _fields_ = [("mode", C.c_int32), ("rgbluminance", C.c_int32), ("a", C.c_double), ("b", C.c_double), ("in_saturation", C.c_double),
                ("out_saturation", C.c_double), ("hueshift", C.c_double), ("hsl_gamma", C.c_double), ("slope", C.c_double * 3),
                ("offset", C.c_double * 3), ("power", C.c_double * 3), ("pivot", C.c_double * 3), ("compression", C.c_double * 3),
                ("hue", C.c_double * 3), ("sat", C.c_double * 3), ("factor", C.c_double * 3), ("lmask", C.POINTER(Plane)),
                ("abmask", C.POINTER(Plane))]


class ColorCorrectionInfo(C.Structure):
    """artgpu_color_correction_info, one per region"""
    _fields_ = [("abca", C.c_float), ("abcb", C.c_float), ("enabled", C.c_int32), ("rgbmode", C.c_int32), ("slope", C.c_float * 3),
                ("offset", C.c_float * 3), ("power", C.c_float * 3), ("pivot", C.c_float * 3), ("compression", C.c_float * 6), ("rhs", C.c_float),
                ("oor_pixels", C.c_int64)]


CC_YUV, CC_RGB, CC_HSL, CC_JZAZBZ, CC_LUT = 0, 1, 2, 3, 4
CC_MODES = {"yuv": CC_YUV, "rgb": CC_RGB, "hsl": CC_HSL, "jzazbz": CC_JZAZBZ, "lut": CC_LUT}


def color_correction_regions(regions):
    """[dict, ...] -> (ColorCorrectionRegion array, objects to keep alive with it).  A dict holds Region's fields under the names of
    ColorCorrectionRegion with Region's defaults (procparams.cc:2834-2855) for what it leaves out: mode JZAZBZ (an ARTGPU_CC_* value or its
    name), slope / power / pivot 1, hsl_gamma 2.4, everything else 0; a per-channel field takes one number for all three channels or three;
    lmask / abmask are Planes or None."""
    arr = (ColorCorrectionRegion * max(len(regions), 1))()
    keep = []
    for k, r in enumerate(regions):
        r = dict(r)
        a = arr[k]
        mode = r.pop("mode", CC_JZAZBZ)
        a.mode = CC_MODES[mode.lower()] if isinstance(mode, str) else int(mode)
        a.rgbluminance = 1 if r.pop("rgbluminance", False) else 0
        for name, dflt in (("a", 0.0), ("b", 0.0), ("in_saturation", 0.0), ("out_saturation", 0.0), ("hueshift", 0.0), ("hsl_gamma", 2.4)):
            setattr(a, name, float(r.pop(name, dflt)))
        for name, dflt in (("slope", 1.0), ("offset", 0.0), ("power", 1.0), ("pivot", 1.0), ("compression", 0.0), ("hue", 0.0), ("sat", 0.0),
                           ("factor", 0.0)):
            v = r.pop(name, dflt)
            v = [float(v)] * 3 if np.isscalar(v) else [float(x) for x in v]
            assert len(v) == 3, name
            setattr(a, name, (C.c_double * 3)(*v))
        for name in ("lmask", "abmask"):
            pl = r.pop(name, None)
            if pl is not None:
                keep.append(pl)
                setattr(a, name, C.pointer(pl))
        assert not r, "unknown colour-correction fields: %s" % sorted(r)
    return arr, keep


SMOOTHING_REGION_FIELDS = (("mode", C.c_int32, 0), ("channel", C.c_int32, 2), ("radius", C.c_int32, 0), ("epsilon", C.c_int32, 0), ("sigma", C.c_double, 0.0),
                           ("iterations", C.c_int32, 1), ("nldetail", C.c_int32, 50), ("falloff", C.c_double, 1.0), ("nlstrength", C.c_int32, 0),
                           ("numblades", C.c_int32, 9), ("angle", C.c_double, 0.0), ("curvature", C.c_double, 0.0), ("offset", C.c_double, 0.0),
                           ("noise_strength", C.c_int32, 10), ("noise_coarseness", C.c_int32, 30), ("halation_size", C.c_double, 1.0),
                           ("halation_color", C.c_double, 0.0), ("wav_strength", C.c_double, 0.0), ("wav_levels", C.c_int32, 5), ("pad_", C.c_int32, 0),
                           ("wav_gamma", C.c_double, 2.2))


class SmoothingRegion(C.Structure):
    """artgpu_smoothing_region: one SmoothingParams::Region (defaults procparams.cc:2753-2775) and its blend plane"""
    _fields_ = [(n, t) for n, t, _ in SMOOTHING_REGION_FIELDS] + [("mask", C.POINTER(Plane))]


class SmoothingInfo(C.Structure):
    """artgpu_smoothing_info, one per region"""
    _fields_ = [("r", C.c_int32), ("epsilon", C.c_float), ("min_x", C.c_int32), ("min_y", C.c_int32), ("max_x", C.c_int32), ("max_y", C.c_int32),
                ("cropped", C.c_int32), ("work_w", C.c_int32), ("work_h", C.c_int32), ("subsampling", C.c_int32), ("box_radius", C.c_int32),
                ("skipped", C.c_int32)]


(SMOOTHING_GUIDED, SMOOTHING_GAUSSIAN, SMOOTHING_GAUSSIAN_GLOW, SMOOTHING_NLMEANS, SMOOTHING_MOTION, SMOOTHING_LENS, SMOOTHING_NOISE,
 SMOOTHING_HALATION, SMOOTHING_WAVELETS) = range(9)
SMOOTHING_MODES = {"guided": 0, "gaussian": 1, "gaussian_glow": 2, "nlmeans": 3, "motion": 4, "lens": 5, "noise": 6, "halation": 7, "wavelets": 8}
SMOOTHING_LUMINANCE, SMOOTHING_CHROMINANCE, SMOOTHING_RGB = 0, 1, 2
SMOOTHING_CHANNELS = {"l": 0, "luminance": 0, "c": 1, "chrominance": 1, "lc": 2, "rgb": 2}
SMOOTHING_MIN_SIZE = 5
SMOOTHING_SKIP_RADIUS, SMOOTHING_SKIP_STRENGTH, SMOOTHING_SKIP_EMPTY = 1, 2, 3


def smoothing_regions(regions):
    """[dict, ...] -> (SmoothingRegion array, objects to keep alive with it).  A dict holds Region's fields under SmoothingRegion's names with
    Region's defaults for what it leaves out; mode and channel are ARTGPU_SMOOTHING_* values or their names; mask is a Plane or None."""
    arr = (SmoothingRegion * max(len(regions), 1))()
    keep = []
    for k, r in enumerate(regions):
        r = dict(r)
        a = arr[k]
        mode, channel = r.pop("mode", SMOOTHING_GUIDED), r.pop("channel", SMOOTHING_RGB)
        a.mode = SMOOTHING_MODES[mode.lower()] if isinstance(mode, str) else int(mode)
        a.channel = SMOOTHING_CHANNELS[channel.lower()] if isinstance(channel, str) else int(channel)
        for name, typ, dflt in SMOOTHING_REGION_FIELDS[2:]:
            v = r.pop(name, dflt)
            setattr(a, name, float(v) if typ is C.c_double else int(v))
        pl = r.pop("mask", None)
        if pl is not None:
            keep.append(pl)
            a.mask = C.pointer(pl)
        assert not r, "unknown smoothing fields: %s" % sorted(r)
    return arr, keep


class ToneEqualizerParams(C.Structure):
    """artgpu_tone_equalizer_params: ToneEqualizerParams (defaults procparams.cc:2097-2104)"""
    _fields_ = [("enabled", C.c_int32), ("bands", C.c_int32 * 5), ("regularization", C.c_int32), ("show_colormap", C.c_int32), ("pivot", C.c_double)]


class ToneEqualizerInfo(C.Structure):
    """artgpu_tone_equalizer_info: what the host derived"""
    _fields_ = [("gain", C.c_float), ("w_sum", C.c_float), ("factors", C.c_float * 12), ("filters", C.c_int32), ("radius", C.c_int32 * 3),
                ("subsampling", C.c_int32 * 3), ("box_radius", C.c_int32 * 3), ("epsilon", C.c_float * 3)]


def tone_equalizer_params(bands=(0, 0, 0, 0, 0), regularization=4, pivot=0.0, enabled=True, show_colormap=False) -> ToneEqualizerParams:
    assert len(bands) == 5
    return ToneEqualizerParams(int(bool(enabled)), (C.c_int32 * 5)(*[int(b) for b in bands]), int(regularization), int(bool(show_colormap)), float(pivot))


def tone_equalizer_lut(params: ToneEqualizerParams):
    """the tool's correction table (65536 float32) and a ToneEqualizerInfo with gain, w_sum and factors, built on the host (no context)"""
    lut = np.empty(65536, np.float32)
    info = ToneEqualizerInfo()
    rc = LIB.artgpu_tone_equalizer_lut(C.byref(params), lut.ctypes.data_as(C.POINTER(C.c_float)), C.byref(info))
    if rc:
        raise ArtGpuError(f"artgpu_tone_equalizer_lut: error {rc}")
    return lut, info


class FilmSimulationParams(C.Structure):
    """artgpu_film_simulation_params: strength (already divided by 100), same_profile, the four ICCStore matrices (row-major)"""
    _fields_ = [("strength", C.c_float), ("same_profile", C.c_int32), ("work_to_xyz", C.c_double * 9), ("xyz_to_clut", C.c_double * 9),
                ("clut_to_xyz", C.c_double * 9), ("xyz_to_work", C.c_double * 9)]


def film_simulation_params(strength=1.0, work_to_xyz=None, xyz_to_clut=None, clut_to_xyz=None, xyz_to_work=None) -> FilmSimulationParams:
    """same_profile unless the four matrices are given"""
    mats = (work_to_xyz, xyz_to_clut, clut_to_xyz, xyz_to_work)
    same = all(m is None for m in mats)
    assert same or all(m is not None for m in mats)
    p = FilmSimulationParams()
    p.strength = float(strength); p.same_profile = int(same)
    for name, m in zip(("work_to_xyz", "xyz_to_clut", "clut_to_xyz", "xyz_to_work"), mats):
        if m is not None:
            getattr(p, name)[:] = [float(v) for v in np.asarray(m, np.float64).reshape(9)]
    return p


def film_simulation_tables():
    """the two 65536-entry float32 tables the film simulation reads (Color::gamma2curve, Color::igammatab_srgb), built on the host (no context)"""
    g, ig = np.empty(65536, np.float32), np.empty(65536, np.float32)
    rc = LIB.artgpu_film_simulation_tables(g.ctypes.data_as(C.POINTER(C.c_float)), ig.ctypes.data_as(C.POINTER(C.c_float)))
    if rc:
        raise ArtGpuError(f"artgpu_film_simulation_tables: error {rc}")
    return g, ig


FILM_GRAIN_MAX_REGIONS, GRAIN_TABLE_SIZE = 4, 5233


class FilmGrainParams(C.Structure):
    """artgpu_film_grain_params: GrainParams (enabled 0, iso 400, strength 50, color 0)"""
    _fields_ = [("enabled", C.c_int32), ("iso", C.c_int32), ("strength", C.c_int32), ("color", C.c_int32)]


class FilmGrainRegionInfo(C.Structure):
    _fields_ = [("channel", C.c_int32), ("strength", C.c_int32), ("coarseness", C.c_int32), ("seed", C.c_int32), ("sz", C.c_int32), ("sf", C.c_float)]

    def as_tuple(self):
        return (self.channel, self.strength, self.coarseness, self.seed, self.sz, np.float32(self.sf))


class FilmGrainInfo(C.Structure):
    _fields_ = [("nregions", C.c_int32), ("region", FilmGrainRegionInfo * FILM_GRAIN_MAX_REGIONS)]

    def regions(self):
        return [self.region[i].as_tuple() for i in range(self.nregions)]


def film_grain_params(iso=400, strength=50, color=False, enabled=True) -> FilmGrainParams:
    return FilmGrainParams(int(bool(enabled)), int(iso), int(strength), int(bool(color)))


def grain_table(seed: int, radius: float = None):
    """what add_noise builds before it reads a pixel, on the host (no context): (normd[5233], state) of a generator seeded `seed`, and with
    `radius` also (the sz x sz normalised cone, sz)"""
    normd = np.empty(GRAIN_TABLE_SIZE, np.float32)
    taps = np.zeros(49, np.float32)
    sz, state = C.c_int(0), C.c_uint64(0)
    rc = LIB.artgpu_grain_table(int(seed), normd.ctypes.data_as(C.POINTER(C.c_float)), taps.ctypes.data_as(C.POINTER(C.c_float)) if radius is not None else None,
                                C.byref(sz), C.c_float(0.0 if radius is None else float(radius)), C.byref(state))
    if rc:
        raise ArtGpuError(f"artgpu_grain_table: error {rc}")
    if radius is None:
        return normd, int(state.value)
    return normd, int(state.value), taps[:sz.value * sz.value].reshape(sz.value, sz.value).copy(), sz.value


RESIZE_PLANES, RESIZE_RGB = 0, 1


class ResizeParams(C.Structure):
    """artgpu_resize_params: ResizeParams as ImProcFunctions::resizeScale reads them (dataspec: 0 scale, 1 width, 2 height, 3 fit box)"""
    _fields_ = [("enabled", C.c_int32), ("dataspec", C.c_int32), ("scale", C.c_double), ("width", C.c_int32), ("height", C.c_int32),
                ("allow_upscaling", C.c_int32)]


def resize_params(dataspec=0, scale=1.0, width=900, height=900, allow_upscaling=False, enabled=True) -> ResizeParams:
    return ResizeParams(int(bool(enabled)), int(dataspec), float(scale), int(width), int(height), int(bool(allow_upscaling)))


def resize_scale(params, fw: int, fh: int):
    """ImProcFunctions::resizeScale on the host (no context): (imw, imh, scale)"""
    imw, imh, sc = C.c_int(), C.c_int(), C.c_float()
    rc = LIB.artgpu_resize_scale(C.byref(params) if params is not None else None, int(fw), int(fh), C.byref(imw), C.byref(imh), C.byref(sc))
    if rc:
        raise ArtGpuError(f"artgpu_resize_scale: error {rc}")
    return imw.value, imh.value, np.float32(sc.value)


class CreativeGradientsParams(C.Structure):
    """artgpu_creative_gradients_params: GradientParams, PCVignetteParams, CropParams and ImProcFunctions' offset / full size / scale"""
    _fields_ = [("gradient_enabled", C.c_int32), ("gradient_degree", C.c_double), ("gradient_feather", C.c_int32), ("gradient_strength", C.c_double),
                ("gradient_center_x", C.c_int32), ("gradient_center_y", C.c_int32),
                ("pcvignette_enabled", C.c_int32), ("pcvignette_strength", C.c_double), ("pcvignette_feather", C.c_int32), ("pcvignette_roundness", C.c_int32),
                ("pcvignette_center_x", C.c_int32), ("pcvignette_center_y", C.c_int32),
                ("crop_enabled", C.c_int32), ("crop_x", C.c_int32), ("crop_y", C.c_int32), ("crop_w", C.c_int32), ("crop_h", C.c_int32),
                ("offset_x", C.c_int32), ("offset_y", C.c_int32), ("full_width", C.c_int32), ("full_height", C.c_int32), ("scale", C.c_double)]


class CreativeGradientDerived(C.Structure):
    """artgpu_creative_gradient_derived: grad_params and pcv_params as the kernel takes them"""
    _fields_ = ([(n, C.c_int32) for n in ("apply_gradient", "apply_pcvignette", "cx", "cy", "angle_is_zero", "transpose", "bright_top", "h")] +
                [(n, C.c_float) for n in ("ta", "yc", "xc", "ys", "ys_inv", "scale", "botmul", "topmul", "top_edge_0",
                                          "oe_a", "oe_b", "oe1_a", "oe1_b", "oe2_a", "oe2_b", "ie_mul", "ie1_mul", "ie2_mul", "sepmix", "feather")] +
                [(n, C.c_int32) for n in ("x1", "x2", "y1", "y2", "ex", "ey", "ew", "eh", "sep", "is_super_ellipse_mode", "is_portrait")] +
                [("pcv_scale", C.c_float), ("fadeout_mul", C.c_float)])


def creative_gradients_params(gradient=None, pcvignette=None, crop=None, offset=(0, 0), full=(-1, -1), scale=1.0) -> CreativeGradientsParams:
    """gradient: (degree, feather, strength, center_x, center_y) or None; pcvignette: (strength, feather, roundness, center_x, center_y) or None;
    crop: (x, y, w, h) or None"""
    g = gradient if gradient is not None else (0.0, 25, 0.6, 0, 0)
    v = pcvignette if pcvignette is not None else (0.6, 50, 50, 0, 0)
    c = crop if crop is not None else (0, 0, 0, 0)
    return CreativeGradientsParams(int(gradient is not None), float(g[0]), int(g[1]), float(g[2]), int(g[3]), int(g[4]),
                                   int(pcvignette is not None), float(v[0]), int(v[1]), int(v[2]), int(v[3]), int(v[4]),
                                   int(crop is not None), int(c[0]), int(c[1]), int(c[2]), int(c[3]),
                                   int(offset[0]), int(offset[1]), int(full[0]), int(full[1]), float(scale))


def creative_gradient_params(params: CreativeGradientsParams, w: int, h: int) -> CreativeGradientDerived:
    """calcGradientParams / calcPCVignetteParams on the host (no context) for a w x h image"""
    out = CreativeGradientDerived()
    rc = LIB.artgpu_creative_gradient_params(C.byref(params), int(w), int(h), C.byref(out))
    if rc:
        raise ArtGpuError(f"artgpu_creative_gradient_params: error {rc}")
    return out


class SoftLightParams(C.Structure):
    """artgpu_soft_light_params: SoftLightParams (enabled 0, strength 30)"""
    _fields_ = [("enabled", C.c_int32), ("strength", C.c_int32)]


def soft_light_params(strength=30, enabled=True) -> SoftLightParams:
    return SoftLightParams(int(bool(enabled)), int(strength))


def soft_light_lut(strength: int) -> np.ndarray:
    """ImProcFunctions::softLight's 65536-entry table, built on the host (no context)"""
    lut = np.empty(65536, np.float32)
    rc = LIB.artgpu_soft_light_lut(int(strength), lut.ctypes.data_as(C.POINTER(C.c_float)))
    if rc:
        raise ArtGpuError(f"artgpu_soft_light_lut: error {rc}")
    return lut


BW_SETTINGS = ("NormalContrast", "Panchromatic", "HyperPanchromatic", "LowSensitivity", "HighSensitivity", "Orthochromatic", "HighContrast", "Luminance",
               "Landscape", "Portrait", "InfraRed", "RGB-Rel", "RGB-Abs", "ROYGCBPM-Rel", "ROYGCBPM-Abs")
BW_FILTERS = ("None", "Red", "Orange", "Yellow", "YellowGreen", "Green", "Cyan", "Blue", "Purple")


class BlackAndWhiteParams(C.Structure):
    """artgpu_black_and_white_params: BlackWhiteParams (setting / filter: indices into BW_SETTINGS / BW_FILTERS)"""
    _fields_ = [("enabled", C.c_int32), ("setting", C.c_int32), ("filter", C.c_int32), ("mixer_red", C.c_int32), ("mixer_green", C.c_int32),
                ("mixer_blue", C.c_int32), ("gamma_red", C.c_int32), ("gamma_green", C.c_int32), ("gamma_blue", C.c_int32), ("cast_bottom", C.c_int32),
                ("cast_top", C.c_int32), ("ulut", C.POINTER(C.c_float)), ("vlut", C.POINTER(C.c_float))]


class BwMixer(C.Structure):
    """artgpu_bw_mixer: what computeBWMixerConstants returns"""
    _fields_ = [("bwr", C.c_float), ("bwg", C.c_float), ("bwb", C.c_float), ("kcorec", C.c_float), ("filcor", C.c_float),
                ("rrm", C.c_double), ("ggm", C.c_double), ("bbm", C.c_double)]


def black_and_white_params(setting="RGB-Rel", filter="None", mixer=(33, 33, 33), gamma=(0, 0, 0), cast=(0, 0), ulut=None, vlut=None, enabled=True):
    """-> (BlackAndWhiteParams, keepalive); ulut / vlut: float32 arrays of 65536 entries (the colour cast's tables) or None"""
    keep = [None if t is None else np.ascontiguousarray(t, np.float32) for t in (ulut, vlut)]
    assert all(t is None or t.shape == (65536,) for t in keep)
    ptr = [None if t is None else t.ctypes.data_as(C.POINTER(C.c_float)) for t in keep]
    st = setting if isinstance(setting, int) else BW_SETTINGS.index(setting)
    fl = filter if isinstance(filter, int) else BW_FILTERS.index(filter)
    return BlackAndWhiteParams(int(bool(enabled)), int(st), int(fl), *[int(v) for v in mixer], *[int(v) for v in gamma], int(cast[0]), int(cast[1]), ptr[0], ptr[1]), keep


def bw_mixer_constants(setting, filter, mixer=(33, 33, 33)) -> BwMixer:
    """computeBWMixerConstants on the host (no context)"""
    st = setting if isinstance(setting, int) else BW_SETTINGS.index(setting)
    fl = filter if isinstance(filter, int) else BW_FILTERS.index(filter)
    out = BwMixer()
    rc = LIB.artgpu_bw_mixer_constants(int(st), int(fl), int(mixer[0]), int(mixer[1]), int(mixer[2]), C.byref(out))
    if rc:
        raise ArtGpuError(f"artgpu_bw_mixer_constants: error {rc}")
    return out


class Clut:
    """artgpu_clut: a HaldCLUT on a context's device.  `table`: uint16 array of level^3 entries, red fastest, 3 or 4 values each."""

    def __init__(self, ctx: "Context", table: np.ndarray, level: int):
        table = np.ascontiguousarray(table)
        assert table.dtype == np.uint16 and table.ndim == 2 and table.shape[1] in (3, 4)
        assert int(level) not in [k * k for k in range(2, 17)] or table.shape[0] == int(level) ** 3   # (any other level: the library refuses it unread)
        self._h = C.c_void_p()
        ctx._chk(LIB.artgpu_clut_create(ctx._h, table.ctypes.data_as(C.POINTER(C.c_uint16)), int(level), int(table.shape[1]), C.byref(self._h)))

    def close(self):
        if self._h:
            LIB.artgpu_clut_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MaskParams(C.Structure):
    """artgpu_mask_params: one rtengine::procparams::Mask as the parametric path of generateMasks reads it"""
    _fields_ = [("parametric_enabled", C.c_int32), ("lightness_detail", C.c_int32), ("hue", C.POINTER(C.c_double)),
                ("chromaticity", C.POINTER(C.c_double)), ("lightness", C.POINTER(C.c_double)), ("nhue", C.c_int32), ("nchromaticity", C.c_int32),
                ("nlightness", C.c_int32), ("contrast_threshold", C.c_int32), ("blur", C.c_double), ("area", C.POINTER(Plane)),
                ("posterization", C.c_int32), ("smoothing", C.c_int32), ("inverted", C.c_int32), ("opacity", C.c_int32),
                ("deltae_enabled", C.c_int32), ("drawn_enabled", C.c_int32), ("external_enabled", C.c_int32), ("linked_enabled", C.c_int32),
                ("curve_is_identity", C.c_int32), ("show_mask", C.c_int32)]


class MasksInfo(C.Structure):
    """artgpu_masks_info, one per region"""
    _fields_ = [("has_mask", C.c_int32), ("has_lmask", C.c_int32), ("ll_radius_small", C.c_int32), ("ll_radius", C.c_int32),
                ("blurred", C.c_int32), ("r1", C.c_int32), ("r2", C.c_int32), ("cthr_w", C.c_int32), ("cthr_h", C.c_int32),
                ("smoothing_radius", C.c_int32)]


MASKS_MIN_SIZE = 8
MASKS_MODE_RGB, MASKS_MODE_LAB, MASKS_MODE_YUV, MASKS_MODE_XYZ = 0, 1, 2, 3
# ParametricMask's default curves (procparams.cc:1014-1053)
DEFAULT_MASK_HUE_POINTS = (1.0, 0.166666667, 1.0, 0.35, 0.35, 0.8287775246, 1.0, 0.35, 0.35)
DEFAULT_MASK_CL_POINTS = (1.0, 0.0, 1.0, 0.35, 0.35, 1.0, 1.0, 0.35, 0.35)


def mask_params(masks):
    """[dict, ...] -> (MaskParams array, objects to keep alive with it).  A dict holds Mask's fields under the names of MaskParams with
    Mask's defaults for what it leaves out (parametric_enabled False, the default curves, blur 0, opacity 100, curve_is_identity True);
    curves are sequences of FlatCurve points, `area` a Plane."""
    arr = (MaskParams * max(len(masks), 1))()
    keep = []
    for k, m in enumerate(masks):
        m = dict(m)
        a = arr[k]
        a.parametric_enabled = 1 if m.pop("parametric_enabled", False) else 0
        for name, dflt in (("hue", DEFAULT_MASK_HUE_POINTS), ("chromaticity", DEFAULT_MASK_CL_POINTS), ("lightness", DEFAULT_MASK_CL_POINTS)):
            pts = m.pop(name, dflt)
            buf = (C.c_double * max(len(pts), 1))(*[float(v) for v in pts])
            keep.append(buf)
            setattr(a, name, C.cast(buf, C.POINTER(C.c_double)))
            setattr(a, "n" + name, len(pts))
        a.lightness_detail = int(m.pop("lightness_detail", 0))
        a.contrast_threshold = int(m.pop("contrast_threshold", 0))
        a.blur = float(m.pop("blur", 0.0))
        area = m.pop("area", None)
        if area is not None:
            keep.append(area)
            a.area = C.pointer(area)
        a.posterization = int(m.pop("posterization", 0)); a.smoothing = int(m.pop("smoothing", 0))
        a.inverted = 1 if m.pop("inverted", False) else 0
        a.opacity = int(m.pop("opacity", 100))
        for name in ("deltae_enabled", "drawn_enabled", "external_enabled", "linked_enabled", "show_mask"):
            setattr(a, name, 1 if m.pop(name, False) else 0)
        a.curve_is_identity = 1 if m.pop("curve_is_identity", True) else 0
        assert not m, sorted(m)
    return arr, keep


SHARPEN_RLD, SHARPEN_USM, SHARPEN_PSF = 0, 1, 2
SHARPEN_REGIME_COPY, SHARPEN_REGIME_3X3, SHARPEN_REGIME_5X5, SHARPEN_REGIME_7X7, SHARPEN_REGIME_YVV = 0, 1, 2, 3, 4
GAUSS_STANDARD, GAUSS_MULT, GAUSS_DIV = 0, 1, 2


class SharpeningParams(C.Structure):
    """artgpu_sharpening_params: SharpeningParams' fields of the rld method + ImProcFunctions' crop geometry"""
    _fields_ = [("enabled", C.c_int32), ("method", C.c_int32), ("amount", C.c_int32), ("deconvamount", C.c_int32),
                ("contrast", C.c_double), ("deconvradius", C.c_double), ("deconvCornerBoost", C.c_double),
                ("deconvCornerLatitude", C.c_int32), ("offset_x", C.c_int32), ("offset_y", C.c_int32),
                ("full_width", C.c_int32), ("full_height", C.c_int32), ("pad_", C.c_int32)]


class SharpeningInfo(C.Structure):
    _fields_ = [("sigma", C.c_double), ("regime", C.c_int32), ("early_out", C.c_int32), ("contrast_threshold", C.c_float),
                ("pad_", C.c_int32), ("impulse_pixels", C.c_int64), ("frozen_pixels", C.c_int64)]


def sharpening_params(enabled=True, method=SHARPEN_RLD, amount=200, contrast=20.0, deconvradius=0.75, deconvamount=100, corner_boost=0.0,
                      corner_latitude=25, offset_x=0, offset_y=0, full_width=0, full_height=0):
    """SharpeningParams' defaults (procparams.cc:1756-1775); Sharpening.arp sets Enabled, Method=rld, Contrast=20, DeconvAmount=100"""
    return SharpeningParams(1 if enabled else 0, int(method), int(amount), int(deconvamount), float(contrast), float(deconvradius),
                            float(corner_boost), int(corner_latitude), int(offset_x), int(offset_y), int(full_width), int(full_height), 0)


class ImpulseDenoiseParams(C.Structure):
    """artgpu_impulse_denoise_params: ImpulseDenoiseParams (defaults: off, 50)"""
    _fields_ = [("enabled", C.c_int32), ("thresh", C.c_int32)]


class ImpulseDenoiseInfo(C.Structure):
    _fields_ = [("early_out", C.c_int32), ("thresh", C.c_float), ("sigma", C.c_float), ("impthr", C.c_float), ("impulse_pixels", C.c_int64)]


def impulse_denoise_params(enabled=True, thresh=50):
    return ImpulseDenoiseParams(1 if enabled else 0, int(thresh))


DEFRINGE_MAX_HALFWIN = 11
DEFRINGE_BLUR_COPY, DEFRINGE_BLUR_3X3, DEFRINGE_BLUR_YVV = 0, 1, 2
# DefringeParams' default hue curve (procparams.cc:1839-1865)
DEFRINGE_DEFAULT_HUECURVE = (1.0, 0.166666667, 0., 0.35, 0.35, 0.347, 0., 0.35, 0.35, 0.513667426, 0., 0.35, 0.35, 0.668944571, 0., 0.35, 0.35,
                             0.8287775246, 0.97835991, 0.35, 0.35, 0.9908883827, 0., 0.35, 0.35)


class DefringeParams(C.Structure):
    """artgpu_defringe_params: DefringeParams (defaults: off, 2.0, 13, DEFRINGE_DEFAULT_HUECURVE)"""
    _fields_ = [("enabled", C.c_int32), ("threshold", C.c_int32), ("radius", C.c_double), ("huecurve", C.POINTER(C.c_double)),
                ("nhuecurve", C.c_int32), ("pad_", C.c_int32)]


class DefringeInfo(C.Structure):
    _fields_ = [("early_out", C.c_int32), ("halfwin", C.c_int32), ("blur", C.c_int32), ("curve", C.c_int32), ("radius", C.c_double),
                ("chromave", C.c_double), ("threshfactor", C.c_float), ("pad_", C.c_int32), ("corrected_pixels", C.c_int64)]


def defringe_params(enabled=True, radius=2.0, threshold=13, huecurve=DEFRINGE_DEFAULT_HUECURVE):
    """huecurve: FlatCurve control points, or None / () for no curve.  The structure keeps the array alive."""
    pts = [float(v) for v in (huecurve or ())]
    arr = (C.c_double * len(pts))(*pts) if pts else None
    p = DefringeParams(1 if enabled else 0, int(threshold), float(radius), C.cast(arr, C.POINTER(C.c_double)) if pts else None, len(pts), 0)
    p._keep = arr
    return p


class PipelineParams(C.Structure):
    pass


class DenoiseToolParams(C.Structure):
    _fields_ = [("dn", DenoiseParams), ("smoothing_enabled", C.c_int32), ("guided_chroma_radius", C.c_int32),
                ("nl_strength", C.c_int32), ("nl_detail", C.c_int32)]


class DenoiseFusion(C.Structure):
    _fields_ = [("demosaiced", C.POINTER(RGB)), ("sx1", C.c_int32), ("sy1", C.c_int32), ("mul", C.c_float * 3), ("do_clip", C.c_int32),
                ("cam_to_work", C.POINTER(C.c_double)), ("exposure_enabled", C.c_int32), ("exp_scale", C.c_float), ("black", C.c_float)]


PipelineParams._fields_ = [
    ("sensor", C.c_int32), ("bayer_method", C.c_int32), ("filters", C.c_uint32), ("initial_gain", C.c_double),
    ("xtrans_passes", C.c_int32), ("xtrans", C.c_int32 * 36), ("rgb_cam", C.c_float * 12), ("border", C.c_int32),
    ("mul", C.c_float * 3), ("do_clip", C.c_int32), ("has_cam_to_work", C.c_int32), ("cam_to_work", C.c_double * 9),
    ("ws", C.c_double * 9), ("iws", C.c_double * 9), ("denoise_enabled", C.c_int32), ("denoise", DenoiseToolParams),
    ("exposure_enabled", C.c_int32), ("expcomp", C.c_double), ("black", C.c_double), ("tone_enabled", C.c_int32),
    ("tone_mode", C.c_int32), ("tone_lut", C.POINTER(C.c_float)), ("white_point", C.c_float), ("to_out", C.c_float * 9),
    ("to_work", C.c_float * 9), ("scale", C.c_double), ("chrominance_auto_factor", C.c_double), ("ca_enabled", C.c_int32), ("ca", CaParams),
    ("local_contrast_enabled", C.c_int32), ("local_contrast_nregions", C.c_int32), ("local_contrast_regions", C.POINTER(LocalContrastRegion)),
    ("dehaze_enabled", C.c_int32), ("dehaze", DehazeParams),
    ("sharpening_enabled", C.c_int32), ("sharpening_auto_radius", C.c_int32), ("sharpening_clip_val", C.c_float), ("pad_sharpening_", C.c_int32),
    ("sharpening", SharpeningParams),
    ("texture_boost_enabled", C.c_int32), ("texture_boost_nregions", C.c_int32), ("texture_boost_regions", C.POINTER(TextureBoostRegion))]



class SensorFrame(C.Structure):
    """artgpu_sensor_frame: a frame as the decoder hands it over (uint16 / float sensor data + scaleColors' constants)"""
    _fields_ = [("data", C.c_void_p), ("w", C.c_int32), ("h", C.c_int32), ("row_stride_bytes", C.c_int64), ("is_u16", C.c_int32),
                ("on_device", C.c_int32), ("cblacksom", C.c_float * 4), ("scale_mul", C.c_float * 4)]


class ScanlineFrame(C.Structure):
    """artgpu_scanline_frame: a frame as the writers take it (rgb2out matrix path + getScanline)"""
    _fields_ = [("scanlines", C.c_void_p), ("row_stride_bytes", C.c_int64), ("bps", C.c_int32), ("is_float", C.c_int32),
                ("on_device", C.c_int32), ("rgb2out_enabled", C.c_int32), ("out_matrix", C.c_float * 9), ("trc_linear", C.c_int32),
                ("trc_lut", C.POINTER(C.c_float)), ("trc_lutsz", C.c_int32), ("chmax", C.c_float * 4), ("status", C.c_int32)]


DN_SKIP_DETAIL_RECOVERY = 1
LOCAL_CONTRAST_MIN_SIZE = 8
TEXTURE_BOOST_MIN_SIZE = 5
# LocalContrastParams::Region's default curve (procparams.cc:1700-1714)
DEFAULT_LOCAL_CONTRAST_CURVE_POINTS = (1.0, 0.0, 0.5, 0.0, 0.0, 1.0, 0.5, 0.0, 0.0)
# the chroma noise curve ImProcFunctions::denoise always installs (ipdenoise.cc:1139-1149)
DEFAULT_NOISE_C_CURVE_POINTS = (1.0, 0.05, 0.50, 0.35, 0.35, 0.35, 0.05, 0.35, 0.35)


def noise_curve_lut(points=DEFAULT_NOISE_C_CURVE_POINTS):
    """NoiseCurve::Set -> (501-entry float32 LUT, sum)."""
    pts = (C.c_double * len(points))(*[float(p) for p in points])
    lut = np.zeros(501, np.float32)
    s = C.c_float(0)
    rc = LIB.artgpu_noise_curve_lut(pts, len(points), lut.ctypes.data_as(C.POINTER(C.c_float)), C.byref(s))
    if rc:
        raise ArtGpuError(f"artgpu_noise_curve_lut: error {rc}")
    return lut, float(s.value)


def local_contrast_curve_lut(points=DEFAULT_LOCAL_CONTRAST_CURVE_POINTS):
    """WavOpacityCurveWL::Set -> (501-entry float32 LUT, is_set); an unset LUT (identity, empty or linear curve) comes back zeroed."""
    pts = (C.c_double * max(len(points), 1))(*[float(p) for p in points])
    lut = np.zeros(501, np.float32)
    is_set = C.c_int(0)
    rc = LIB.artgpu_local_contrast_curve_lut(pts, len(points), lut.ctypes.data_as(C.POINTER(C.c_float)), C.byref(is_set))
    if rc:
        raise ArtGpuError(f"artgpu_local_contrast_curve_lut: error {rc}")
    return lut, bool(is_set.value)


# DehazeParams::strength's default (procparams.cc:2694-2711)
DEFAULT_DEHAZE_STRENGTH_POINTS = (1.0, 0.0, 0.75, 0.0, 0.0, 1.0, 0.75, 0.0, 0.0)


def dehaze_strength_lut(points=DEFAULT_DEHAZE_STRENGTH_POINTS):
    """ipdehaze.cc:419-424 -> the 65536-entry float32 strength table"""
    pts = (C.c_double * max(len(points), 1))(*[float(p) for p in points])
    lut = np.zeros(65536, np.float32)
    rc = LIB.artgpu_dehaze_strength_lut(pts, len(points), lut.ctypes.data_as(C.POINTER(C.c_float)))
    if rc:
        raise ArtGpuError(f"artgpu_dehaze_strength_lut: error {rc}")
    return lut


def dehaze_estimate_ambient(R, G, B):
    """get_dark_channel(.., 2, nullptr, false) + estimate_ambient_light on three hh x ww planes -> (ambient float32[3], max_t)"""
    planes = [np.ascontiguousarray(a, dtype=np.float32) for a in (R, G, B)]
    hh, ww = planes[0].shape
    ambient = (C.c_float * 3)()
    max_t = C.c_float(0)
    fp = C.POINTER(C.c_float)
    rc = LIB.artgpu_dehaze_estimate_ambient(*[a.ctypes.data_as(fp) for a in planes], ww, hh, ambient, C.byref(max_t))
    if rc:
        raise ArtGpuError(f"artgpu_dehaze_estimate_ambient: error {rc}")
    return np.array(ambient[:], np.float32), np.float32(max_t.value)


def dehaze_params(strength=DEFAULT_DEHAZE_STRENGTH_POINTS, depth=25, show_depth_map=False, luminance=False, blackpoint=0, enabled=True):
    """-> (DehazeParams, the object to keep alive with it)"""
    pts = (C.c_double * max(len(strength), 1))(*[float(v) for v in strength])
    p = DehazeParams(1 if enabled else 0, C.cast(pts, C.POINTER(C.c_double)), len(strength), 1 if show_depth_map else 0, int(depth),
                     1 if luminance else 0, int(blackpoint))
    return p, pts


def texture_boost_regions(regions):
    """[(strength, detail threshold, iterations, mask Plane or None), ...] -> (TextureBoostRegion array, objects to keep alive with it)"""
    arr = (TextureBoostRegion * max(len(regions), 1))()
    keep = []
    for k, (strength, threshold, iterations, mask) in enumerate(regions):
        arr[k].strength = float(strength)
        arr[k].detail_threshold = float(threshold)
        arr[k].iterations = int(iterations)
        if mask is not None:
            keep.append(mask)
            arr[k].mask = C.pointer(mask)
    return arr, keep


def local_contrast_regions(regions):
    """[(contrast, curve LUT or None, mask Plane or None), ...] -> (LocalContrastRegion array, objects to keep alive with it)"""
    arr = (LocalContrastRegion * max(len(regions), 1))()
    keep = []
    for k, (contrast, curve, mask) in enumerate(regions):
        arr[k].contrast = float(contrast)
        if curve is not None:
            cv = np.ascontiguousarray(curve, dtype=np.float32)
            assert cv.shape == (501,)
            keep.append(cv)
            arr[k].curve = cv.ctypes.data_as(C.POINTER(C.c_float))
        if mask is not None:
            keep.append(mask)
            arr[k].mask = C.pointer(mask)
    return arr, keep


class ArtGpuError(RuntimeError):
    pass


PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p, C.c_double)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback for the device path)")
    # When this process also uses torch (device buffers, torch.distributed), torch must load its bundled HIP/HSA runtime
    # FIRST: loading libartgpu.so (linked against /opt/rocm's libamdhip64) before torch leaves two runtimes in the process
    # and hipGetDeviceCount fails.  Stand-alone users of the library (artgpu-cli, a C++ host) are unaffected.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    lib.artgpu_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.artgpu_destroy.argtypes = [C.c_void_p]
    lib.artgpu_last_error.argtypes = [C.c_void_p]
    lib.artgpu_last_error.restype = C.c_char_p
    lib.artgpu_version.restype = C.c_char_p
    lib.artgpu_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.artgpu_synchronize.argtypes = [C.c_void_p]
    lib.artgpu_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
    lib.artgpu_get_option.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_long)]
    lib.artgpu_set_curve_tail.argtypes = [C.c_void_p, C.c_int, C.c_double]
    lib.artgpu_set_curve_tail_parametric.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
    lib.artgpu_enable_timing.argtypes = [C.c_void_p, C.c_int]
    lib.artgpu_get_timings.argtypes = [C.c_void_p, C.POINTER(Timings)]
    lib.artgpu_scratch_bytes.argtypes = [C.c_void_p]
    lib.artgpu_scratch_bytes.restype = C.c_size_t
    lib.artgpu_trim_scratch.argtypes = [C.c_void_p]
    lib.artgpu_demosaic_bayer.argtypes = [C.c_void_p, C.c_int, C.POINTER(Plane), C.c_uint32, C.c_double, C.c_int, C.POINTER(RGB)]
    lib.artgpu_border_interpolate2.argtypes = [C.c_void_p, C.POINTER(Plane), C.c_uint32, C.c_int, C.POINTER(RGB)]
    lib.artgpu_wavelet_decompose.argtypes = [C.c_void_p, C.POINTER(Plane), C.c_int, C.POINTER(C.c_void_p)]
    lib.artgpu_wavelet_mad.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    lib.artgpu_wavelet_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.artgpu_wavelet_get_band.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.artgpu_wavelet_set_band.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.artgpu_wavelet_reconstruct.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Plane), C.c_float]
    lib.artgpu_wavelet_free.argtypes = [C.c_void_p, C.c_void_p]
    lib.artgpu_rgb_denoise.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(DenoiseParams), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_double,
                                       C.c_double, C.POINTER(Plane), C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.artgpu_denoise_guided_smoothing.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(C.c_double), C.c_int, C.c_double]
    lib.artgpu_gaussian_blur.argtypes = [C.c_void_p, C.POINTER(Plane), C.c_double]
    lib.artgpu_detail_mask.argtypes = [C.c_void_p, C.POINTER(Plane), C.POINTER(Plane), C.c_float, C.c_float, C.c_float, C.c_float, C.c_float]
    lib.artgpu_nlmeans.argtypes = [C.c_void_p, C.POINTER(Plane), C.c_float, C.c_int, C.c_int, C.c_float]
    lib.artgpu_improc_denoise.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(DenoiseToolParams), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double,
                                          C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_float), C.c_uint32]
    lib.artgpu_improc_denoise_fused.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(DenoiseFusion), C.POINTER(DenoiseToolParams), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_float), C.c_uint32]
    lib.artgpu_raw_ca_correct.argtypes = [C.c_void_p, C.POINTER(Plane), C.c_uint32, C.POINTER(CaParams), C.POINTER(C.c_double)]
    lib.artgpu_local_contrast_curve_lut.argtypes = [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    lib.artgpu_dehaze.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(DehazeParams), C.POINTER(C.c_double), C.c_double, C.POINTER(DehazeInfo)]
    lib.artgpu_dehaze_strength_lut.argtypes = [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_float)]
    lib.artgpu_dehaze_estimate_ambient.argtypes = [C.POINTER(C.c_float)] * 3 + [C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.artgpu_dehaze_dark_channel.argtypes = [C.c_void_p, C.POINTER(RGB), C.c_int, C.POINTER(C.c_float), C.c_int, C.POINTER(Plane)]
    lib.artgpu_sharpening.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(SharpeningParams), C.POINTER(C.c_double), C.c_double, C.POINTER(SharpeningInfo)]
    lib.artgpu_rl_deconvolution.argtypes = [C.c_void_p, C.POINTER(Plane), C.POINTER(Plane), C.c_void_p, C.c_double, C.c_float, C.POINTER(SharpeningInfo)]
    lib.artgpu_gaussian_blur_ex.argtypes = [C.c_void_p, C.POINTER(Plane), C.POINTER(Plane), C.POINTER(Plane), C.c_double, C.c_int]
    lib.artgpu_deconv_auto_radius.argtypes = [C.c_void_p, C.POINTER(Plane), C.c_uint32, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.artgpu_impulse_denoise.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(ImpulseDenoiseParams), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_int,
                                           C.POINTER(ImpulseDenoiseInfo)]
    lib.artgpu_defringe.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(DefringeParams), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_int, C.c_int,
                                    C.POINTER(DefringeInfo)]
    lib.artgpu_texture_boost_plane.argtypes = [C.c_void_p, C.POINTER(Plane), C.POINTER(TextureBoostRegion), C.c_double, C.c_int, C.POINTER(TextureBoostInfo)]
    lib.artgpu_texture_boost.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(TextureBoostRegion), C.c_int, C.POINTER(C.c_double), C.c_double, C.c_int, C.c_int,
                                         C.POINTER(TextureBoostInfo)]
    lib.artgpu_generate_masks.argtypes = [C.c_void_p, C.POINTER(RGB), C.c_int, C.POINTER(C.c_double), C.POINTER(MaskParams), C.c_int, C.c_int, C.c_int,
                                          C.c_double, C.POINTER(Plane), C.POINTER(Plane), C.POINTER(MasksInfo)]
    lib.artgpu_set_pipeline_masks.argtypes = [C.c_void_p, C.POINTER(MaskParams), C.c_int, C.POINTER(MaskParams), C.c_int]
    lib.artgpu_color_correction.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(ColorCorrectionRegion), C.c_int, C.POINTER(C.c_double),
                                            C.POINTER(C.c_double), C.c_int, C.POINTER(ColorCorrectionInfo)]
    lib.artgpu_color_correction_yuv.argtypes = lib.artgpu_color_correction.argtypes
    lib.artgpu_set_pipeline_color_correction.argtypes = [C.c_void_p, C.POINTER(ColorCorrectionRegion), C.c_int, C.POINTER(MaskParams)]
    lib.artgpu_smoothing.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(SmoothingRegion), C.c_int, C.POINTER(C.c_double), C.c_double,
                                     C.POINTER(SmoothingInfo)]
    lib.artgpu_set_pipeline_smoothing.argtypes = [C.c_void_p, C.POINTER(SmoothingRegion), C.c_int, C.POINTER(MaskParams)]
    lib.artgpu_tone_equalizer.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(ToneEqualizerParams), C.POINTER(C.c_double), C.c_double,
                                          C.POINTER(ToneEqualizerInfo)]
    lib.artgpu_tone_equalizer_lut.argtypes = [C.POINTER(ToneEqualizerParams), C.POINTER(C.c_float), C.POINTER(ToneEqualizerInfo)]
    lib.artgpu_set_pipeline_tone_equalizer.argtypes = [C.c_void_p, C.POINTER(ToneEqualizerParams)]
    lib.artgpu_clut_create.argtypes = [C.c_void_p, C.POINTER(C.c_uint16), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.artgpu_clut_destroy.argtypes = [C.c_void_p]
    lib.artgpu_clut_destroy.restype = None
    lib.artgpu_film_simulation.argtypes = [C.c_void_p, C.POINTER(RGB), C.c_void_p, C.POINTER(FilmSimulationParams)]
    lib.artgpu_film_simulation_tables.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.artgpu_set_pipeline_film_simulation.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(FilmSimulationParams), C.c_int]
    lib.artgpu_film_grain.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(FilmGrainParams), C.POINTER(C.c_double), C.c_double, C.c_int, C.POINTER(FilmGrainInfo)]
    lib.artgpu_add_noise.argtypes = [C.c_void_p, C.POINTER(RGB), C.c_int, C.c_int, C.c_int, C.POINTER(Plane), C.POINTER(C.c_double), C.c_double, C.c_int, C.c_int]
    lib.artgpu_grain_table.argtypes = [C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int), C.c_float, C.POINTER(C.c_uint64)]
    lib.artgpu_grain_indices.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.c_int64, C.POINTER(C.c_uint32)]
    lib.artgpu_set_pipeline_film_grain.argtypes = [C.c_void_p, C.POINTER(FilmGrainParams)]
    lib.artgpu_creative_gradients.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(CreativeGradientsParams)]
    lib.artgpu_creative_gradient_params.argtypes = [C.POINTER(CreativeGradientsParams), C.c_int, C.c_int, C.POINTER(CreativeGradientDerived)]
    lib.artgpu_set_pipeline_creative_gradients.argtypes = [C.c_void_p, C.POINTER(CreativeGradientsParams)]
    lib.artgpu_soft_light.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(SoftLightParams)]
    lib.artgpu_soft_light_lut.argtypes = [C.c_int, C.POINTER(C.c_float)]
    lib.artgpu_set_pipeline_soft_light.argtypes = [C.c_void_p, C.POINTER(SoftLightParams)]
    lib.artgpu_black_and_white.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(BlackAndWhiteParams), C.POINTER(C.c_double)]
    lib.artgpu_bw_mixer_constants.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(BwMixer)]
    lib.artgpu_set_pipeline_black_and_white.argtypes = [C.c_void_p, C.POINTER(BlackAndWhiteParams)]
    lib.artgpu_set_pipeline_impulse_defringe.argtypes = [C.c_void_p, C.POINTER(ImpulseDenoiseParams), C.POINTER(DefringeParams)]
    lib.artgpu_resize_lanczos.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(RGB), C.c_float, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.artgpu_resize_scale.argtypes = [C.POINTER(ResizeParams), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float)]
    lib.artgpu_set_pipeline_resize.argtypes = [C.c_void_p, C.POINTER(ResizeParams)]
    lib.artgpu_local_contrast.argtypes = [C.c_void_p, C.POINTER(Plane), C.POINTER(LocalContrastRegion), C.c_int, C.c_double, C.POINTER(LocalContrastInfo)]
    lib.artgpu_scale_colors.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_uint32,
                                        C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(Plane), C.POINTER(C.c_float)]
    lib.artgpu_denoise_compute_params.argtypes = [C.c_void_p, C.POINTER(RGB), C.c_int, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_double),
                                                  C.POINTER(C.c_double), C.c_double, C.POINTER(DenoiseInfoStore), C.POINTER(DenoiseParams)]
    lib.artgpu_ordered_sum_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float)]
    lib.artgpu_eval_primitive.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float,
                                          C.POINTER(C.c_float), C.c_int]
    lib.artgpu_saturation_vibrance.argtypes = [C.c_void_p, C.POINTER(RGB), C.c_int, C.c_int, C.POINTER(C.c_double)]
    lib.artgpu_set_batch_lanes.argtypes = [C.c_void_p, C.c_int]
    lib.artgpu_set_progress_callback.argtypes = [C.c_void_p, PROGRESS_FN, C.c_void_p]
    lib.artgpu_batch_complete.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.artgpu_rgb2out_matrix.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(RGB), C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float), C.c_int]
    lib.artgpu_get_scanlines.argtypes = [C.c_void_p, C.POINTER(RGB), C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int]
    lib.artgpu_guided_filter.argtypes = [C.c_void_p, C.POINTER(Plane), C.POINTER(Plane), C.POINTER(Plane), C.c_int, C.c_float, C.c_int]
    lib.artgpu_hsl_equalizer.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_int,
                                         C.c_int, C.POINTER(C.c_double), C.c_double, C.c_int]
    lib.artgpu_log_encoding.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(LogEncParams), C.POINTER(C.c_double), C.c_int, C.c_int]
    lib.artgpu_rgb_to_lab.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(C.c_double)]
    lib.artgpu_lab_to_rgb.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(C.c_double)]
    lib.artgpu_lab_to_yuv.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(C.c_double)]
    lib.artgpu_lab_histogram.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(C.c_uint32)]
    lib.artgpu_lab_adjustments.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float]
    lib.artgpu_dual_demosaic_bayer.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(Plane), C.c_uint32, C.c_double, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(RGB)]
    lib.artgpu_channel_mixer.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(C.c_float)]
    lib.artgpu_rgb_curves.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.artgpu_pipeline_run.argtypes = [C.c_void_p, C.POINTER(Plane), C.POINTER(PipelineParams), C.POINTER(RGB)]
    lib.artgpu_batch_run.argtypes = [C.c_void_p, C.c_int, C.POINTER(Plane), C.POINTER(PipelineParams), C.POINTER(RGB)]
    lib.artgpu_batch_run_io.argtypes = [C.c_void_p, C.c_int, C.POINTER(SensorFrame), C.POINTER(PipelineParams), C.POINTER(ScanlineFrame)]
    lib.artgpu_demosaic_xtrans.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(Plane), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(RGB)]
    lib.artgpu_tone_curve_neutral.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(C.c_float), C.c_float, C.POINTER(NeutralState)]
    lib.artgpu_noise_curve_lut.argtypes = [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.artgpu_denoise_chroma_map.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_float),
                                              C.POINTER(Plane)]
    lib.artgpu_get_image_skip.argtypes = [C.c_void_p, C.POINTER(RGB), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int,
                                          C.POINTER(C.c_double), C.POINTER(RGB)]
    lib.artgpu_get_image.argtypes = [C.c_void_p, C.POINTER(RGB), C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int,
                                     C.POINTER(C.c_double), C.POINTER(RGB)]
    lib.artgpu_convert_color_space.argtypes = [C.c_void_p, C.POINTER(RGB), C.POINTER(C.c_double)]
    lib.artgpu_exposure.argtypes = [C.c_void_p, C.POINTER(RGB), C.c_float, C.c_float]
    lib.artgpu_tone_curve.argtypes = [C.c_void_p, C.POINTER(RGB), C.c_int, C.POINTER(C.c_float), C.c_float, C.c_int]
    return lib


LIB = _load()

# artgpu_eval_primitive ids (include/artgpu.h: ARTGPU_PRIM_*)
PRIM_XEXPF_S = 0
PRIM_XEXPF_V = 1
PRIM_XEXPF_VN = 2
PRIM_XEXPF_V_LDEXP = 3
PRIM_XLOGF_S = 4
PRIM_XLOGF_V = 5
PRIM_XLOGF_VN = 6
PRIM_POW_F = 7
PRIM_XLIN2LOG = 8
PRIM_XLOG2LIN = 9
PRIM_XCBRTF = 10
PRIM_XATAN2F = 11
PRIM_XSINCOSF = 12
PRIM_LUTF_SCALAR = 13
PRIM_LUTF_VECTOR = 14
PRIM_MEDIAN3 = 15
PRIM_VMINF = 16
PRIM_VMAXF = 17
PRIM_VINTPF = 18
PRIM_XDIV2F = 19
PRIM_XDIVF2 = 20
PRIM_XLOG_D = 21
PRIM_XEXP_D = 22
PRIM_FLOAT_TO_HALF = 23     # out: float32-sized words, the half in the low 16 bits (eval_primitive returns them as uint32)
PRIM_XSINF_S = 24           # sleef.h's scalar xsinf
PRIM_XCOSF_S = 25           # sleef.h's scalar xcosf, which under SSE2 is lane 0 of the vector form

EXPORTS = ["artgpu_eval_primitive", "artgpu_set_progress_callback", "artgpu_set_option", "artgpu_get_option", "artgpu_set_curve_tail", "artgpu_set_curve_tail_parametric", "artgpu_create", "artgpu_destroy", "artgpu_last_error", "artgpu_version", "artgpu_set_stream",
           "artgpu_synchronize", "artgpu_enable_timing", "artgpu_get_timings", "artgpu_scratch_bytes", "artgpu_trim_scratch",
           "artgpu_demosaic_bayer", "artgpu_border_interpolate2", "artgpu_get_image",
           "artgpu_convert_color_space", "artgpu_exposure", "artgpu_tone_curve",
           "artgpu_wavelet_decompose", "artgpu_wavelet_mad", "artgpu_wavelet_info", "artgpu_wavelet_get_band", "artgpu_wavelet_set_band",
           "artgpu_wavelet_reconstruct", "artgpu_wavelet_free", "artgpu_rgb_denoise", "artgpu_denoise_guided_smoothing",
           "artgpu_gaussian_blur", "artgpu_detail_mask", "artgpu_nlmeans", "artgpu_improc_denoise", "artgpu_improc_denoise_fused", "artgpu_noise_curve_lut", "artgpu_denoise_chroma_map", "artgpu_tone_curve_neutral", "artgpu_demosaic_xtrans", "artgpu_pipeline_run", "artgpu_batch_run", "artgpu_batch_run_io", "artgpu_scale_colors", "artgpu_channel_mixer", "artgpu_rgb_curves", "artgpu_denoise_compute_params", "artgpu_ordered_sum_f32", "artgpu_get_image_skip", "artgpu_saturation_vibrance", "artgpu_set_batch_lanes", "artgpu_batch_complete", "artgpu_rgb2out_matrix", "artgpu_get_scanlines", "artgpu_guided_filter", "artgpu_hsl_equalizer", "artgpu_log_encoding", "artgpu_rgb_to_lab", "artgpu_lab_to_rgb", "artgpu_lab_to_yuv", "artgpu_lab_histogram", "artgpu_lab_adjustments", "artgpu_dual_demosaic_bayer", "artgpu_raw_ca_correct", "artgpu_local_contrast_curve_lut", "artgpu_local_contrast",
           "artgpu_dehaze", "artgpu_dehaze_strength_lut", "artgpu_dehaze_estimate_ambient", "artgpu_dehaze_dark_channel",
           "artgpu_sharpening", "artgpu_rl_deconvolution", "artgpu_gaussian_blur_ex", "artgpu_deconv_auto_radius", "artgpu_impulse_denoise", "artgpu_defringe", "artgpu_set_pipeline_impulse_defringe",
           "artgpu_texture_boost_plane", "artgpu_texture_boost", "artgpu_generate_masks", "artgpu_set_pipeline_masks",
           "artgpu_color_correction", "artgpu_color_correction_yuv", "artgpu_set_pipeline_color_correction", "artgpu_smoothing", "artgpu_set_pipeline_smoothing",
           "artgpu_tone_equalizer", "artgpu_tone_equalizer_lut", "artgpu_set_pipeline_tone_equalizer",
           "artgpu_clut_create", "artgpu_clut_destroy", "artgpu_film_simulation", "artgpu_film_simulation_tables", "artgpu_set_pipeline_film_simulation",
           "artgpu_resize_lanczos", "artgpu_resize_scale", "artgpu_set_pipeline_resize",
           "artgpu_film_grain", "artgpu_add_noise", "artgpu_grain_table", "artgpu_grain_indices", "artgpu_set_pipeline_film_grain",
           "artgpu_creative_gradients", "artgpu_creative_gradient_params", "artgpu_set_pipeline_creative_gradients",
           "artgpu_soft_light", "artgpu_soft_light_lut", "artgpu_set_pipeline_soft_light",
           "artgpu_black_and_white", "artgpu_bw_mixer_constants", "artgpu_set_pipeline_black_and_white"]


def host_plane(a: np.ndarray) -> Plane:
    assert a.dtype == np.float32 and a.ndim == 2 and a.strides[1] == 4
    return Plane(a.ctypes.data, a.shape[1], a.shape[0], a.strides[0], 0)


def sensor_frame(a: np.ndarray, cblacksom=(0.0, 0.0, 0.0, 0.0), scale_mul=(1.0, 1.0, 1.0, 1.0)) -> SensorFrame:
    assert a.dtype in (np.uint16, np.float32) and a.ndim == 2 and a.strides[1] == a.itemsize
    return SensorFrame(a.ctypes.data, a.shape[1], a.shape[0], a.strides[0], 1 if a.dtype == np.uint16 else 0, 0,
                       (C.c_float * 4)(*[float(v) for v in cblacksom]), (C.c_float * 4)(*[float(v) for v in scale_mul]))


def scanline_frame(a: np.ndarray, matrix=None, trc_lut=None, is_float: bool = False) -> ScanlineFrame:
    """`a`: (h, w, 3) uint8 / uint16 / float32 host array the scanlines land in (uint16 + is_float: half floats).  matrix: rgb2out's
    3 x 3 (None: no rgb2out); trc_lut: float32 array the caller keeps alive until the batch call has returned (None: linear TRC)."""
    assert a.ndim == 3 and a.shape[2] == 3 and a.strides[2] == a.itemsize and a.strides[1] == 3 * a.itemsize
    f = ScanlineFrame()
    f.scanlines = a.ctypes.data; f.row_stride_bytes = a.strides[0]; f.bps = 8 * a.itemsize
    f.is_float = 1 if (is_float or a.dtype == np.float32) else 0
    f.on_device = 0
    f.rgb2out_enabled = 0 if matrix is None else 1
    if matrix is not None:
        f.out_matrix[:] = [float(v) for v in np.asarray(matrix, np.float32).reshape(9)]
    f.trc_linear = 1 if trc_lut is None else 0
    if trc_lut is not None:
        assert trc_lut.dtype == np.float32 and trc_lut.flags.c_contiguous
        f.trc_lut = trc_lut.ctypes.data_as(C.POINTER(C.c_float)); f.trc_lutsz = trc_lut.size
    return f


def host_rgb(planes) -> RGB:
    return RGB(*[host_plane(p) for p in planes])


def device_plane(t) -> Plane:
    """`t`: a 2-D float32 torch tensor on the context's device with unit column stride."""
    assert t.dim() == 2 and t.stride(1) == 1 and t.element_size() == 4
    return Plane(t.data_ptr(), t.shape[1], t.shape[0], t.stride(0) * 4, 1)


class Context:
    """One device context (include/artgpu.h: artgpu_create / artgpu_destroy)."""

    def __init__(self, device: int = 0, stream=None):
        self._h = C.c_void_p()
        rc = LIB.artgpu_create(device, C.byref(self._h))
        if rc != 0:
            raise ArtGpuError(f"artgpu_create(device={device}) failed: {rc}")
        if stream is not None:
            self.set_stream(stream)

    def _chk(self, rc):
        if rc != 0:
            raise ArtGpuError(f"[{rc}] {LIB.artgpu_last_error(self._h).decode()}")

    def set_stream(self, stream_handle: int):
        self._chk(LIB.artgpu_set_stream(self._h, C.c_void_p(stream_handle)))

    def synchronize(self):
        self._chk(LIB.artgpu_synchronize(self._h))

    def set_option(self, name: str, value: int):
        self._chk(LIB.artgpu_set_option(self._h, name.encode(), C.c_long(int(value))))

    def get_option(self, name: str) -> int:
        v = C.c_long(0)
        self._chk(LIB.artgpu_get_option(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    def set_curve_tail(self, kind: int, y_last: float = 1.0):
        """0 LUT clip (no Curve object), 1 constant y_last, 2 identity, 3 host (default): curves::setLutVal above 65535"""
        self._chk(LIB.artgpu_set_curve_tail(self._h, int(kind), float(y_last)))

    def set_curve_tail_parametric(self, p):
        """DiagonalCurve's DCT_Parametric parameter vector (8 or 9 doubles, p[0] = the kind): getVal above 1.0 on the device"""
        arr = (C.c_double * len(p))(*[float(v) for v in p])
        self._chk(LIB.artgpu_set_curve_tail_parametric(self._h, arr, len(p)))

    def enable_timing(self, on: bool = True):
        self._chk(LIB.artgpu_enable_timing(self._h, int(on)))

    def timings(self) -> Timings:
        t = Timings()
        self._chk(LIB.artgpu_get_timings(self._h, C.byref(t)))
        return t

    def scratch_bytes(self) -> int:
        return LIB.artgpu_scratch_bytes(self._h)

    def trim_scratch(self):
        self._chk(LIB.artgpu_trim_scratch(self._h))

    def demosaic_bayer(self, method: int, raw: Plane, filters: int, initial_gain: float, border: int, out: RGB):
        self._chk(LIB.artgpu_demosaic_bayer(self._h, method, C.byref(raw), filters, initial_gain, border, C.byref(out)))

    def border_interpolate2(self, raw: Plane, filters: int, lborders: int, out: RGB):
        self._chk(LIB.artgpu_border_interpolate2(self._h, C.byref(raw), filters, lborders, C.byref(out)))

    def get_image(self, planes: RGB, sx1: int, sy1: int, mul, do_clip: bool, mat, image: RGB, skip: int = 1):
        m = (C.c_float * 3)(*[float(v) for v in mul])
        mp = None if mat is None else (C.c_double * 9)(*[float(v) for v in np.asarray(mat, dtype=np.float64).reshape(9)])
        if skip == 1:
            self._chk(LIB.artgpu_get_image(self._h, C.byref(planes), sx1, sy1, m, int(do_clip), mp, C.byref(image)))
        else:
            self._chk(LIB.artgpu_get_image_skip(self._h, C.byref(planes), sx1, sy1, int(skip), m, int(do_clip), mp, C.byref(image)))

    def convert_color_space(self, image: RGB, mat):
        mp = (C.c_double * 9)(*[float(v) for v in np.asarray(mat, dtype=np.float64).reshape(9)])
        self._chk(LIB.artgpu_convert_color_space(self._h, C.byref(image), mp))

    def exposure(self, image: RGB, exp_scale: float, black: float):
        self._chk(LIB.artgpu_exposure(self._h, C.byref(image), exp_scale, black))

    def tone_curve(self, image: RGB, lut, whitept: float = 1.0, filmlike_clip: bool = True, mode: int = 0):
        lp = None
        if lut is not None:
            lut = np.ascontiguousarray(lut, dtype=np.float32)
            assert lut.shape == (65536,)
            lp = lut.ctypes.data_as(C.POINTER(C.c_float))
        self._chk(LIB.artgpu_tone_curve(self._h, C.byref(image), mode, lp, whitept, int(filmlike_clip)))

    def rgb_denoise(self, image: RGB, params: DenoiseParams, ws, expcomp: float = 0.0, scale: float = 1.0,
                    ccalc: Plane = None, flags: int = DN_SKIP_DETAIL_RECOVERY, want_resid: bool = False, iws=None):
        wsf = (C.c_float * 9)(*[float(v) for v in np.asarray(ws, dtype=np.float32).reshape(9)])
        iwsf = None if iws is None else (C.c_float * 9)(*[float(v) for v in np.asarray(iws, dtype=np.float32).reshape(9)])
        nresi, highresi = C.c_float(0), C.c_float(0)
        self._chk(LIB.artgpu_rgb_denoise(self._h, C.byref(image), C.byref(params), wsf, iwsf, expcomp, scale,
                                         None if ccalc is None else C.byref(ccalc), flags,
                                         C.byref(nresi) if want_resid else None, C.byref(highresi) if want_resid else None))
        if want_resid:
            return float(nresi.value), float(highresi.value)

    def denoise_guided_smoothing(self, image: RGB, ws, radius: int = 3, scale: float = 1.0):
        m = (C.c_double * 9)(*[float(v) for v in np.asarray(ws, dtype=np.float64).reshape(9)])
        self._chk(LIB.artgpu_denoise_guided_smoothing(self._h, C.byref(image), m, radius, scale))

    def gaussian_blur(self, img: Plane, sigma: float):
        self._chk(LIB.artgpu_gaussian_blur(self._h, C.byref(img), sigma))

    def detail_mask(self, src: Plane, mask: Plane, scaling, threshold, ceiling, factor, blur):
        self._chk(LIB.artgpu_detail_mask(self._h, C.byref(src), C.byref(mask), scaling, threshold, ceiling, factor, blur))

    def nlmeans(self, img: Plane, strength: int = 50, detail: int = 80, scale: float = 1.0, normcoeff: float = 65535.0):
        self._chk(LIB.artgpu_nlmeans(self._h, C.byref(img), normcoeff, strength, detail, scale))

    def scale_colors(self, src: np.ndarray, filters: int, xtrans, cblacksom, scale_mul, dst: Plane, device_src=None):
        """host uint16 / float32 sensor data -> scaled float CFA plane; returns chmax[4].  device_src: the sensor data on the device instead
        (`src` is then ignored): a 2-D torch tensor of 16-bit integers (read as uint16) or float32 with unit column stride and any row stride."""
        xt = None if xtrans is None else np.ascontiguousarray(xtrans, dtype=np.int32).reshape(36).ctypes.data_as(C.POINTER(C.c_int32))
        cb = (C.c_float * 4)(*[float(v) for v in cblacksom]); sm = (C.c_float * 4)(*[float(v) for v in scale_mul])
        mx = (C.c_float * 4)()
        if device_src is None:
            assert src.dtype in (np.uint16, np.float32) and src.flags.c_contiguous
            h, w = src.shape
            ptr, row_bytes, is_u16, on_device = src.ctypes.data, src.strides[0], src.dtype == np.uint16, 0
        else:
            t = device_src
            assert t.dim() == 2 and t.stride(1) == 1 and t.element_size() in (2, 4) and (t.element_size() == 2 or t.is_floating_point())
            h, w = t.shape
            ptr, row_bytes, is_u16, on_device = t.data_ptr(), t.stride(0) * t.element_size(), t.element_size() == 2, 1
        self._chk(LIB.artgpu_scale_colors(self._h, ptr, w, h, row_bytes, 1 if is_u16 else 0, on_device, filters, xt, cb, sm, C.byref(dst), mx))
        return [float(v) for v in mx]

    def raw_ca_correct(self, raw: Plane, filters: int, params: "CaParams", want_fit: bool = False):
        """RawImageSource::CA_correct_RT in place on a scaled CFA plane; returns fitparams as a (2, 2, 16) array when want_fit"""
        fit = np.zeros(64, np.float64) if want_fit else None
        self._chk(LIB.artgpu_raw_ca_correct(self._h, C.byref(raw), filters, C.byref(params),
                                            fit.ctypes.data_as(C.POINTER(C.c_double)) if want_fit else None))
        return fit.reshape(2, 2, 16) if want_fit else None

    def local_contrast(self, L: Plane, regions, scale: float = 1.0, want_info: bool = False):
        """ImProcFunctions::localContrast in place on an L plane; `regions`: [(contrast, curve LUT or None, mask Plane or None), ...].
        Returns the LocalContrastInfo of the last region when want_info."""
        arr, keep = local_contrast_regions(regions)
        info = LocalContrastInfo() if want_info else None
        self._chk(LIB.artgpu_local_contrast(self._h, C.byref(L), arr, len(regions), float(scale), C.byref(info) if want_info else None))
        del keep
        return info

    local_contrast_curve_lut = staticmethod(local_contrast_curve_lut)

    def dehaze(self, image: RGB, params: "DehazeParams", ws, scale: float = 1.0, want_info: bool = False):
        """ImProcFunctions::dehaze in place (params from dehaze_params()); returns the DehazeInfo when want_info."""
        wsd = (C.c_double * 9)(*np.asarray(ws, np.float64).ravel())
        info = DehazeInfo() if want_info else None
        self._chk(LIB.artgpu_dehaze(self._h, C.byref(image), C.byref(params), wsd, float(scale), C.byref(info) if want_info else None))
        return info

    def dehaze_dark_channel(self, rgb: RGB, patchsize: int, ambient, clip: bool, dst: Plane):
        amb = None if ambient is None else (C.c_float * 3)(*[float(v) for v in ambient])
        self._chk(LIB.artgpu_dehaze_dark_channel(self._h, C.byref(rgb), int(patchsize), amb, 1 if clip else 0, C.byref(dst)))

    dehaze_strength_lut = staticmethod(dehaze_strength_lut)
    dehaze_estimate_ambient = staticmethod(dehaze_estimate_ambient)

    def texture_boost_plane(self, Y: Plane, strength: float, detail_threshold: float = 0.2, iterations: int = 1, scale: float = 1.0,
                            high_detail: bool = True, want_info: bool = False):
        """one texture_boost call (iptextureboost.cc:37-178) in place on a Y plane; returns the TextureBoostInfo when want_info."""
        arr, _ = texture_boost_regions([(strength, detail_threshold, iterations, None)])
        info = TextureBoostInfo() if want_info else None
        self._chk(LIB.artgpu_texture_boost_plane(self._h, C.byref(Y), arr, float(scale), 1 if high_detail else 0, C.byref(info) if want_info else None))
        return info

    def texture_boost(self, image: RGB, regions, ws, scale: float = 1.0, high_detail: bool = True, to_rgb: bool = True, want_info: bool = False):
        """ImProcFunctions::textureBoost in place on an RGB image.  regions: [(strength, detail threshold, iterations, mask Plane or None), ...];
        returns the TextureBoostInfo of the last region that ran when want_info."""
        arr, keep = texture_boost_regions(regions)
        wsd = (C.c_double * 9)(*np.asarray(ws, np.float64).ravel())
        info = TextureBoostInfo() if want_info else None
        self._chk(LIB.artgpu_texture_boost(self._h, C.byref(image), arr, len(regions), wsd, float(scale), 1 if high_detail else 0, 1 if to_rgb else 0,
                                           C.byref(info) if want_info else None))
        del keep
        return info

    def generate_masks(self, image: RGB, mode: int, ws, masks, full_w: int = -1, full_h: int = -1, scale: float = 1.0, Lmask=None, abmask=None,
                       want_info: bool = False):
        """rtengine::generateMasks' parametric path.  masks: what mask_params() takes; Lmask / abmask: a list of len(masks) Planes each, or
        None.  Returns the list of MasksInfo (one per region) when want_info."""
        arr, keep = mask_params(masks)
        n = len(masks)
        wsd = None if ws is None else (C.c_double * 9)(*np.asarray(ws, np.float64).ravel())
        sets = []
        for planes in (Lmask, abmask):
            assert planes is None or len(planes) == n
            sets.append(None if planes is None else (Plane * max(n, 1))(*planes))
        info = (MasksInfo * max(n, 1))() if want_info else None
        self._chk(LIB.artgpu_generate_masks(self._h, C.byref(image), int(mode), wsd, arr, n, int(full_w), int(full_h), float(scale), sets[0], sets[1], info))
        del keep
        return list(info)[:n] if want_info else None

    def set_pipeline_masks(self, local_contrast_masks=None, texture_boost_masks=None):
        """the region masks pipeline_run / batch_run / batch_run_io generate themselves (what mask_params() takes, one per region of the tool;
        None: that tool's regions use their own planes).  The library copies them."""
        lc, k1 = mask_params(local_contrast_masks or [])
        tb, k2 = mask_params(texture_boost_masks or [])
        self._chk(LIB.artgpu_set_pipeline_masks(self._h, lc if local_contrast_masks else None, len(local_contrast_masks or []),
                                                tb if texture_boost_masks else None, len(texture_boost_masks or [])))
        del k1, k2

    def color_correction(self, image: RGB, regions, ws, iws, to_rgb: bool = False, want_info: bool = False, from_yuv: bool = False):
        """ImProcFunctions::colorCorrection in place on an RGB image, or with from_yuv on one in YUV mode already (left in YUV mode unless to_rgb).
        regions: what color_correction_regions() takes.  Returns the list of ColorCorrectionInfo (one per region) when want_info."""
        arr, keep = color_correction_regions(regions)
        n = len(regions)
        wsd = (C.c_double * 9)(*np.asarray(ws, np.float64).ravel())
        iwsd = (C.c_double * 9)(*np.asarray(iws, np.float64).ravel())
        info = (ColorCorrectionInfo * max(n, 1))() if want_info else None
        self._chk((LIB.artgpu_color_correction_yuv if from_yuv else LIB.artgpu_color_correction)(self._h, C.byref(image), arr, n, wsd, iwsd, 1 if to_rgb else 0, info))
        del keep
        return list(info)[:n] if want_info else None

    def set_pipeline_color_correction(self, regions=None, masks=None):
        """the colour correction pipeline_run / batch_run / batch_run_io run behind the sharpening (what color_correction_regions() takes;
        None: off) and, optionally, the masks they generate its planes from (what mask_params() takes, one per region).  The library copies both."""
        arr, k1 = color_correction_regions(regions or [])
        mk, k2 = mask_params(masks or [])
        assert not masks or len(masks) == len(regions or [])
        self._chk(LIB.artgpu_set_pipeline_color_correction(self._h, arr if regions else None, len(regions or []), mk if masks else None))
        del k1, k2

    def smoothing(self, image: RGB, regions, ws, scale: float = 1.0, want_info: bool = False):
        """ImProcFunctions::guidedSmoothing (modes GUIDED and NLMEANS) in place on an RGB image.  regions: what smoothing_regions() takes.
        Returns the list of SmoothingInfo (one per region) when want_info."""
        arr, keep = smoothing_regions(regions)
        n = len(regions)
        wsd = (C.c_double * 9)(*np.asarray(ws, np.float64).ravel())
        info = (SmoothingInfo * max(n, 1))() if want_info else None
        self._chk(LIB.artgpu_smoothing(self._h, C.byref(image), arr, n, wsd, float(scale), info))
        del keep
        return list(info)[:n] if want_info else None

    def set_pipeline_smoothing(self, regions=None, masks=None):
        """the Smoothing tool pipeline_run / batch_run / batch_run_io run behind colour correction (what smoothing_regions() takes; None: off)
        and, optionally, the masks they generate its planes from (what mask_params() takes, one per region).  The library copies both."""
        arr, k1 = smoothing_regions(regions or [])
        mk, k2 = mask_params(masks or [])
        assert not masks or len(masks) == len(regions or [])
        self._chk(LIB.artgpu_set_pipeline_smoothing(self._h, arr if regions else None, len(regions or []), mk if masks else None))
        del k1, k2

    def tone_equalizer(self, image: RGB, params: ToneEqualizerParams, ws, scale: float = 1.0, want_info: bool = False):
        """ImProcFunctions::toneEqualizer in place on an RGB image (params from tone_equalizer_params()); returns the ToneEqualizerInfo when
        want_info."""
        wsd = (C.c_double * 9)(*np.asarray(ws, np.float64).ravel())
        info = ToneEqualizerInfo() if want_info else None
        self._chk(LIB.artgpu_tone_equalizer(self._h, C.byref(image), C.byref(params), wsd, float(scale), C.byref(info) if want_info else None))
        return info

    tone_equalizer_lut = staticmethod(tone_equalizer_lut)

    def set_pipeline_tone_equalizer(self, params: ToneEqualizerParams = None):
        """the tone equalizer pipeline_run / batch_run / batch_run_io run behind the exposure (None: off).  The library copies it."""
        self._chk(LIB.artgpu_set_pipeline_tone_equalizer(self._h, C.byref(params) if params is not None else None))

    def clut(self, table: np.ndarray, level: int) -> "Clut":
        """a HaldCLUT on this context's device (artgpu_clut_create): level^3 x 3 or x 4 uint16, red fastest; level = entries per axis"""
        return Clut(self, table, level)

    def film_simulation(self, image: RGB, clut: "Clut", params: FilmSimulationParams):
        """ImProcFunctions::filmSimulation with a HaldCLUT in place on an RGB image (params from film_simulation_params())"""
        self._chk(LIB.artgpu_film_simulation(self._h, C.byref(image), clut._h, C.byref(params)))

    film_simulation_tables = staticmethod(film_simulation_tables)

    def set_pipeline_film_simulation(self, clut: "Clut" = None, params: FilmSimulationParams = None, after_tone_curve: bool = False):
        """film simulation in pipeline_run / batch_run / batch_run_io: between texture boost and the tone curve, or right behind the tone curve
        (None: off).  The library copies the parameters and keeps a reference to the CLUT."""
        self._chk(LIB.artgpu_set_pipeline_film_simulation(self._h, clut._h if clut is not None else None, C.byref(params) if params is not None else None,
                                                          int(bool(after_tone_curve))))

    def film_grain(self, image: RGB, params: FilmGrainParams, ws, scale: float = 1.0, output_pipeline: bool = True, want_info: bool = False):
        """ImProcFunctions::filmGrain in place on an RGB image (params from film_grain_params()); returns the FilmGrainInfo when want_info"""
        wsd = (C.c_double * 9)(*np.asarray(ws, np.float64).ravel()) if ws is not None else None
        info = FilmGrainInfo() if want_info else None
        self._chk(LIB.artgpu_film_grain(self._h, C.byref(image), C.byref(params) if params is not None else None, wsd, float(scale), int(bool(output_pipeline)),
                                        C.byref(info) if want_info else None))
        return info

    def add_noise(self, image: RGB, strength: int, coarseness: int, channel: int, ws, scale: float = 1.0, mask: Plane = None, first: bool = True, last: bool = True):
        """one NOISE region of guidedSmoothing in place on an RGB image: add_noise on the mask's working area and the blend; first / last: this
        call normalises the image ahead of the region / scales it back behind it"""
        wsd = (C.c_double * 9)(*np.asarray(ws, np.float64).ravel()) if ws is not None else None
        self._chk(LIB.artgpu_add_noise(self._h, C.byref(image), int(strength), int(coarseness), int(channel), C.byref(mask) if mask is not None else None, wsd,
                                       float(scale), int(bool(first)), int(bool(last))))

    grain_table = staticmethod(grain_table)

    def grain_indices(self, state: int, first: int, n: int) -> np.ndarray:
        """the table indices of draws first .. first + n - 1 counted from `state`, through the device's jump-ahead (a diagnostic)"""
        out = np.zeros(max(int(n), 1), np.uint32)
        self._chk(LIB.artgpu_grain_indices(self._h, int(state), int(first), int(n), out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out[:n]

    def set_pipeline_film_grain(self, params: FilmGrainParams = None):
        """film grain in pipeline_run / batch_run / batch_run_io: behind texture boost, ahead of film simulation (None: off).  The library copies it."""
        self._chk(LIB.artgpu_set_pipeline_film_grain(self._h, C.byref(params) if params is not None else None))

    def resize_lanczos(self, src: RGB, dst: RGB, scale: float, mode: int = RESIZE_PLANES, ws=None, iws=None):
        """ImProcFunctions::Lanczos from src into dst (the caller's size).  RESIZE_RGB: setMode(LAB) on src (whose contents are unspecified
        afterwards), the resampler, setMode(RGB) on dst; needs ws and iws"""
        def mat(m):
            return None if m is None else (C.c_double * 9)(*[float(v) for v in np.asarray(m, dtype=np.float64).reshape(9)])
        self._chk(LIB.artgpu_resize_lanczos(self._h, C.byref(src), C.byref(dst), C.c_float(float(scale)), int(mode), mat(ws), mat(iws)))

    resize_scale = staticmethod(resize_scale)

    def set_pipeline_resize(self, params: ResizeParams = None):
        """the Resize tool behind STAGE_3 of the per-frame pipe (None: off): outputs are then imw x imh of resize_scale on the bordered frame"""
        self._chk(LIB.artgpu_set_pipeline_resize(self._h, C.byref(params) if params is not None else None))

    def creative_gradients(self, image: RGB, params: CreativeGradientsParams):
        """ImProcFunctions::creativeGradients in place on an RGB image (params from creative_gradients_params())"""
        self._chk(LIB.artgpu_creative_gradients(self._h, C.byref(image), C.byref(params) if params is not None else None))

    creative_gradient_params = staticmethod(creative_gradient_params)

    def set_pipeline_creative_gradients(self, params: CreativeGradientsParams = None):
        """the graduated / vignette filters in pipeline_run / batch_run / batch_run_io: the first step of STAGE_3 (None: off).  The library copies it."""
        self._chk(LIB.artgpu_set_pipeline_creative_gradients(self._h, C.byref(params) if params is not None else None))

    def soft_light(self, image: RGB, params: SoftLightParams):
        """ImProcFunctions::softLight in place on an RGB image (params from soft_light_params())"""
        self._chk(LIB.artgpu_soft_light(self._h, C.byref(image), C.byref(params) if params is not None else None))

    soft_light_lut = staticmethod(soft_light_lut)

    def set_pipeline_soft_light(self, params: SoftLightParams = None):
        """soft light in pipeline_run / batch_run / batch_run_io: behind the tone curve, ahead of local contrast (None: off).  The library copies it."""
        self._chk(LIB.artgpu_set_pipeline_soft_light(self._h, C.byref(params) if params is not None else None))

    def black_and_white(self, image: RGB, params: BlackAndWhiteParams, ws=None):
        """ImProcFunctions::blackAndWhite in place on an RGB image (params from black_and_white_params()); ws: the colour cast only"""
        wsd = (C.c_double * 9)(*np.asarray(ws, np.float64).ravel()) if ws is not None else None
        self._chk(LIB.artgpu_black_and_white(self._h, C.byref(image), C.byref(params) if params is not None else None, wsd))

    bw_mixer_constants = staticmethod(bw_mixer_constants)

    def set_pipeline_black_and_white(self, params: BlackAndWhiteParams = None):
        """black-and-white in pipeline_run / batch_run / batch_run_io: behind local contrast (None: off).  The library copies parameters and tables."""
        self._chk(LIB.artgpu_set_pipeline_black_and_white(self._h, C.byref(params) if params is not None else None))

    def set_pipeline_impulse_defringe(self, impulse: "ImpulseDenoiseParams" = None, defringe: "DefringeParams" = None):
        """impulse noise reduction / defringe in pipeline_run / batch_run / batch_run_io: behind the sharpening, ahead of colour correction (None: off).
        The library copies the parameters and the hue curve."""
        self._chk(LIB.artgpu_set_pipeline_impulse_defringe(self._h, C.byref(impulse) if impulse is not None else None,
                                                           C.byref(defringe) if defringe is not None else None))

    def sharpening(self, image: RGB, params: "SharpeningParams", ws, scale: float = 1.0, want_info: bool = False):
        """ImProcFunctions::sharpening (method rld) in place (params from sharpening_params()); returns the SharpeningInfo when want_info."""
        wsd = (C.c_double * 9)(*np.asarray(ws, np.float64).ravel())
        info = SharpeningInfo() if want_info else None
        self._chk(LIB.artgpu_sharpening(self._h, C.byref(image), C.byref(params), wsd, float(scale), C.byref(info) if want_info else None))
        return info

    def rl_deconvolution(self, luminance: Plane, blend: Plane, impulse, sigma: float, amount: float, want_info: bool = False):
        """deconvsharpening in place on `luminance`; impulse: the address of W * H bytes where the luminance plane lives (host or device)"""
        info = SharpeningInfo() if want_info else None
        self._chk(LIB.artgpu_rl_deconvolution(self._h, C.byref(luminance), C.byref(blend), C.c_void_p(int(impulse)), float(sigma), float(amount),
                                              C.byref(info) if want_info else None))
        return info

    def impulse_denoise(self, image: RGB, params: "ImpulseDenoiseParams", ws, iws=None, scale: float = 1.0, to_rgb: bool = True, want_info: bool = False):
        """ImProcFunctions::impulsedenoise in place on an image in RGB mode (params from impulse_denoise_params()); to_rgb False leaves the image in
        LAB mode as the reference does; returns the ImpulseDenoiseInfo when want_info."""
        wsd = (C.c_double * 9)(*np.asarray(ws, np.float64).ravel())
        iwsd = None if iws is None else (C.c_double * 9)(*np.asarray(iws, np.float64).ravel())
        info = ImpulseDenoiseInfo() if want_info else None
        self._chk(LIB.artgpu_impulse_denoise(self._h, C.byref(image), C.byref(params), wsd, iwsd, float(scale), 1 if to_rgb else 0,
                                             C.byref(info) if want_info else None))
        return info

    def defringe(self, image: RGB, params: "DefringeParams", ws, iws=None, scale: float = 1.0, to_rgb: bool = True, want_info: bool = False, from_lab: bool = False):
        """ImProcFunctions::defringe in place on an image in RGB mode, or in LAB mode with from_lab (params from defringe_params()); to_rgb False leaves
        the image in LAB mode as the reference does; returns the DefringeInfo when want_info."""
        wsd = None if ws is None else (C.c_double * 9)(*np.asarray(ws, np.float64).ravel())
        iwsd = None if iws is None else (C.c_double * 9)(*np.asarray(iws, np.float64).ravel())
        info = DefringeInfo() if want_info else None
        self._chk(LIB.artgpu_defringe(self._h, C.byref(image), C.byref(params), wsd, iwsd, float(scale), 1 if from_lab else 0, 1 if to_rgb else 0,
                                      C.byref(info) if want_info else None))
        return info

    def gaussian_blur_ex(self, src: Plane, dst: Plane, div, sigma: float, gausstype: int):
        """gaussianBlur(src, dst, .., gausstype, div) for src != dst, GAUSS_DIV / GAUSS_MULT; above sigma 1.15 GAUSS_MULT overwrites src"""
        self._chk(LIB.artgpu_gaussian_blur_ex(self._h, C.byref(src), C.byref(dst), None if div is None else C.byref(div), float(sigma), int(gausstype)))

    def deconv_auto_radius(self, raw: Plane, filters: int, lower_limit: float = 1000.0, clip_val: float = 65535.0):
        """RawImageSource::getDeconvAutoRadius (Bayer / monochrome) -> (radius, max_ratio) as float32"""
        r, m = C.c_float(0), C.c_float(0)
        self._chk(LIB.artgpu_deconv_auto_radius(self._h, C.byref(raw), int(filters), float(lower_limit), float(clip_val), C.byref(r), C.byref(m)))
        return np.float32(r.value), np.float32(m.value)

    def denoise_compute_params(self, planes: RGB, border: int, mul, do_clip: bool, cam_to_work, ws, dn: DenoiseParams,
                               auto_factor: float = 1.0, store: "DenoiseInfoStore" = None) -> "DenoiseInfoStore":
        """ImProcFunctions::denoiseComputeParams; updates dn.chrominance* in place and returns the store"""
        store = store if store is not None else DenoiseInfoStore()
        d9 = lambda m: (C.c_double * 9)(*[float(v) for v in np.asarray(m, dtype=np.float64).reshape(9)])
        self._chk(LIB.artgpu_denoise_compute_params(self._h, C.byref(planes), int(border), (C.c_float * 3)(*[float(v) for v in mul]),
                                                    1 if do_clip else 0, d9(cam_to_work), d9(ws), float(auto_factor), C.byref(store), C.byref(dn)))
        return store

    def ordered_sum_f32(self, x) -> np.float32:
        """acc = 0; for v in x: acc += v  (fp32), x a numpy array (host) or a CUDA torch tensor"""
        r = C.c_float(0)
        if isinstance(x, np.ndarray):
            a = np.ascontiguousarray(x, dtype=np.float32)
            self._chk(LIB.artgpu_ordered_sum_f32(self._h, a.ctypes.data, a.size, 0, C.byref(r)))
        else:
            assert x.is_contiguous() and x.dtype.itemsize == 4
            self._chk(LIB.artgpu_ordered_sum_f32(self._h, x.data_ptr(), x.numel(), 1, C.byref(r)))
        return np.float32(r.value)

    def eval_primitive(self, prim: int, a, b=None, c=None, param: float = 0.0, table=None):
        """out0[i] = f(a[i] [, b[i] [, c[i]]]) with the device's own math primitive `prim` (PRIM_*); host numpy arrays in and out.
        PRIM_XSINCOSF returns (sin, cos); PRIM_XLOG_D / PRIM_XEXP_D work on float64."""
        dt = np.float64 if prim in (PRIM_XLOG_D, PRIM_XEXP_D) else np.float32
        arrs = [None if x is None else np.ascontiguousarray(x, dtype=dt) for x in (a, b, c)]
        n = arrs[0].size
        out0, out1 = np.empty(n, dt), np.empty(n, dt)
        tab = None if table is None else np.ascontiguousarray(table, dtype=np.float32)
        ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        self._chk(LIB.artgpu_eval_primitive(self._h, int(prim), ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), ptr(out0), ptr(out1), C.c_int64(n),
                                            C.c_float(param), None if tab is None else tab.ctypes.data_as(C.POINTER(C.c_float)),
                                            0 if tab is None else tab.size))
        if prim == PRIM_FLOAT_TO_HALF:
            return out0.view(np.uint32)
        return (out0, out1) if prim == PRIM_XSINCOSF else out0

    def saturation_vibrance(self, image: RGB, saturation: int, vibrance: int, ws):
        self._chk(LIB.artgpu_saturation_vibrance(self._h, C.byref(image), int(saturation), int(vibrance),
                                                 (C.c_double * 9)(*[float(v) for v in np.asarray(ws, dtype=np.float64).reshape(9)])))

    def rgb2out_matrix(self, src: RGB, dst: RGB, matrix, trc_linear: bool, lut=None):
        m = (C.c_float * 9)(*[float(v) for v in np.asarray(matrix, np.float32).reshape(9)])
        la = None if lut is None else np.ascontiguousarray(lut, dtype=np.float32)
        self._chk(LIB.artgpu_rgb2out_matrix(self._h, C.byref(src), C.byref(dst), m, 1 if trc_linear else 0,
                                            None if la is None else la.ctypes.data_as(C.POINTER(C.c_float)), 0 if la is None else la.size))

    def get_scanlines(self, image: RGB, bps: int, is_float: bool = False, device_dst=None):
        """Imagefloat::getScanline for every row -> (h, w, 3) array of uint8 / uint16 / float16-bits (uint16) / float32.  device_dst: the
        scanlines go to the device instead and nothing is returned: a 2-D torch tensor of bytes, one row per scanline (at least
        w * 3 * bps / 8 bytes each, unit column stride, any row stride)."""
        if device_dst is not None:
            t = device_dst
            assert t.dim() == 2 and t.element_size() == 1 and t.stride(1) == 1 and t.shape[0] == image.r.h and t.shape[1] >= image.r.w * 3 * bps // 8
            self._chk(LIB.artgpu_get_scanlines(self._h, C.byref(image), bps, 1 if is_float else 0, t.data_ptr(), t.stride(0), 1))
            return None
        dt = np.float32 if (is_float and bps == 32) else (np.uint8 if bps == 8 else np.uint16)
        out = np.zeros((image.r.h, image.r.w, 3), dt)
        self._chk(LIB.artgpu_get_scanlines(self._h, C.byref(image), bps, 1 if is_float else 0, out.ctypes.data, out.strides[0], 0))
        return out

    def guided_filter(self, guide: Plane, src: Plane, dst: Plane, r: int, epsilon: float, subsampling: int = 0):
        self._chk(LIB.artgpu_guided_filter(self._h, C.byref(guide), C.byref(src), C.byref(dst), int(r), float(epsilon), int(subsampling)))

    def hsl_equalizer(self, image: RGB, hcurve, scurve, lcurve, smoothing: int, ws, scale: float = 1.0, to_rgb: bool = True):
        def arr(c):
            if c is None:
                return None, 0
            a = (C.c_double * len(c))(*[float(v) for v in c])
            return a, len(c)
        (h, nh), (s, ns), (l, nl) = arr(hcurve), arr(scurve), arr(lcurve)
        self._chk(LIB.artgpu_hsl_equalizer(self._h, C.byref(image), h, nh, s, ns, l, nl, int(smoothing),
                                           (C.c_double * 9)(*[float(v) for v in np.asarray(ws, dtype=np.float64).reshape(9)]), float(scale), 1 if to_rgb else 0))

    def log_encoding(self, image: RGB, ws, gain=0.0, target_gray=18.0, black_ev=-13.5, white_ev=2.5, regularization=60, satcontrol=True,
                     highlight_compression=0, full_width=0, full_height=0, enabled=True):
        p = LogEncParams(1 if enabled else 0, int(regularization), 1 if satcontrol else 0, int(highlight_compression),
                         float(gain), float(target_gray), float(black_ev), float(white_ev))
        self._chk(LIB.artgpu_log_encoding(self._h, C.byref(image), C.byref(p), (C.c_double * 9)(*[float(v) for v in np.asarray(ws, dtype=np.float64).reshape(9)]),
                                          int(full_width), int(full_height)))

    def rgb_to_lab(self, image: RGB, ws):
        self._chk(LIB.artgpu_rgb_to_lab(self._h, C.byref(image), (C.c_double * 9)(*[float(v) for v in np.asarray(ws, dtype=np.float64).reshape(9)])))

    def lab_to_rgb(self, image: RGB, iws):
        self._chk(LIB.artgpu_lab_to_rgb(self._h, C.byref(image), (C.c_double * 9)(*[float(v) for v in np.asarray(iws, dtype=np.float64).reshape(9)])))

    def lab_to_yuv(self, image: RGB, iws):
        """Imagefloat::setMode(YUV) on an image in LAB mode (lab_to_yuv), in place"""
        self._chk(LIB.artgpu_lab_to_yuv(self._h, C.byref(image), (C.c_double * 9)(*[float(v) for v in np.asarray(iws, dtype=np.float64).reshape(9)])))

    def lab_histogram(self, image: RGB):
        hist = np.zeros(65536, np.uint32)
        self._chk(LIB.artgpu_lab_histogram(self._h, C.byref(image), hist.ctypes.data_as(C.POINTER(C.c_uint32))))
        return hist

    def lab_adjustments(self, image: RGB, lcurve, acurve, bcurve, chroma: float):
        keep = [np.ascontiguousarray(c, dtype=np.float32) for c in (lcurve, acurve, bcurve)]
        assert keep[0].size == 32770 and keep[1].size == 65536 and keep[2].size == 65536
        self._chk(LIB.artgpu_lab_adjustments(self._h, C.byref(image), *[k.ctypes.data_as(C.POINTER(C.c_float)) for k in keep], float(chroma)))

    def dual_demosaic_bayer(self, method: int, raw: Plane, filters: int, initial_gain: float, border: int, contrast: float, auto_contrast: bool, out: RGB,
                            second: int = DUAL_BILINEAR):
        """returns the contrast threshold in percent (searched when auto_contrast)"""
        c = C.c_double(float(contrast))
        self._chk(LIB.artgpu_dual_demosaic_bayer(self._h, method, second, C.byref(raw), filters, float(initial_gain), border, C.byref(c), 1 if auto_contrast else 0, C.byref(out)))
        return c.value

    def channel_mixer(self, image: RGB, m):
        self._chk(LIB.artgpu_channel_mixer(self._h, C.byref(image), (C.c_float * 9)(*[float(v) for v in np.asarray(m, np.float32).reshape(9)])))

    def rgb_curves(self, image: RGB, rcurve=None, gcurve=None, bcurve=None):
        ptr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))
        keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (rcurve, gcurve, bcurve)]
        self._chk(LIB.artgpu_rgb_curves(self._h, C.byref(image), *[None if k is None else k.ctypes.data_as(C.POINTER(C.c_float)) for k in keep]))

    def set_progress_callback(self, fn):
        """fn(stage: str, fraction: float) or None"""
        self._progress = PROGRESS_FN(lambda user, stage, frac: fn(stage.decode(), frac)) if fn else PROGRESS_FN()
        self._chk(LIB.artgpu_set_progress_callback(self._h, self._progress, None))

    def set_batch_lanes(self, lanes: int):
        self._chk(LIB.artgpu_set_batch_lanes(self._h, int(lanes)))

    def batch_complete(self, record, nranks: int = 1, rccl_comm=None):
        """All-gather of the ranks' 8-word completion records over an RCCL communicator (None: single rank)."""
        rec = (C.c_int64 * 8)(*[int(v) for v in record])
        out = (C.c_int64 * (8 * nranks))()
        self._chk(LIB.artgpu_batch_complete(self._h, rccl_comm, int(nranks), rec, out))
        return [list(out[8 * r:8 * r + 8]) for r in range(nranks)]

    def pipeline_run(self, raw: Plane, params: PipelineParams, out: RGB):
        self._chk(LIB.artgpu_pipeline_run(self._h, C.byref(raw), C.byref(params), C.byref(out)))

    def batch_run(self, raws, params: PipelineParams, outs):
        n = len(raws)
        self._chk(LIB.artgpu_batch_run(self._h, n, (Plane * n)(*raws), C.byref(params), (RGB * n)(*outs)))

    def batch_run_io(self, sensor_frames, params: PipelineParams, scanline_frames, check: bool = True):
        """artgpu_batch_run_io: sensor data in, writers' scanlines out, copies beside the kernels.  `sensor_frames`: numpy arrays (uint16 /
        float32, host) or ready SensorFrame structures; `scanline_frames`: ScanlineFrame structures (scanline_frame() builds one around a
        numpy array).  Returns the array of ScanlineFrame (chmax / status filled in).  check=False: no exception for a non-zero return code;
        returns (code, array) -- a frame whose status is 0 is complete whatever the code (artgpu.h)."""
        n = len(sensor_frames)
        ins = (SensorFrame * n)()
        for k, f in enumerate(sensor_frames):
            ins[k] = f if isinstance(f, SensorFrame) else sensor_frame(f)
        outs = (ScanlineFrame * n)(*scanline_frames)
        rc = LIB.artgpu_batch_run_io(self._h, n, ins, C.byref(params), outs)
        if not check:
            return rc, outs
        self._chk(rc)
        return outs

    def demosaic_xtrans(self, passes: int, use_cielab: bool, raw: Plane, xtrans, rgb_cam, out: RGB):
        xt = np.ascontiguousarray(xtrans, dtype=np.int32).reshape(36)
        cam = np.ascontiguousarray(rgb_cam, dtype=np.float32).reshape(12)
        self._chk(LIB.artgpu_demosaic_xtrans(self._h, passes, 1 if use_cielab else 0, C.byref(raw), xt.ctypes.data_as(C.POINTER(C.c_int32)),
                                             cam.ctypes.data_as(C.POINTER(C.c_float)), C.byref(out)))

    def tone_curve_neutral(self, image: RGB, lut65536, whitecoeff, ws, iws, to_out=None, to_work=None):
        lut = np.ascontiguousarray(lut65536, dtype=np.float32)
        assert lut.shape == (65536,)
        ident = np.eye(3, dtype=np.float32)
        st = NeutralState()
        st.ws[:] = [float(v) for v in np.asarray(ws, np.float64).reshape(9)]
        st.iws[:] = [float(v) for v in np.asarray(iws, np.float64).reshape(9)]
        st.to_out[:] = [float(v) for v in np.asarray(ident if to_out is None else to_out, np.float32).reshape(9)]
        st.to_work[:] = [float(v) for v in np.asarray(ident if to_work is None else to_work, np.float32).reshape(9)]
        self._chk(LIB.artgpu_tone_curve_neutral(self._h, C.byref(image), lut.ctypes.data_as(C.POINTER(C.c_float)), whitecoeff, C.byref(st)))

    def denoise_chroma_map(self, image: RGB, calclum_mat, ws, curve, ccalc: Plane):
        m = None if calclum_mat is None else (C.c_double * 9)(*[float(v) for v in np.asarray(calclum_mat, dtype=np.float64).reshape(9)])
        wsd = (C.c_double * 9)(*[float(v) for v in np.asarray(ws, dtype=np.float64).reshape(9)])
        cv = np.ascontiguousarray(curve, dtype=np.float32)
        assert cv.shape == (501,)
        self._chk(LIB.artgpu_denoise_chroma_map(self._h, C.byref(image), m, wsd, cv.ctypes.data_as(C.POINTER(C.c_float)), C.byref(ccalc)))

    def improc_denoise(self, image: RGB, params: DenoiseToolParams, ws, ecomp: float = 0.0, scale: float = 1.0, calclum_mat=None,
                       noise_c_curve=None, flags: int = 0, iws=None):
        wsd = (C.c_double * 9)(*[float(v) for v in np.asarray(ws, dtype=np.float64).reshape(9)])
        m = None if calclum_mat is None else (C.c_double * 9)(*[float(v) for v in np.asarray(calclum_mat, dtype=np.float64).reshape(9)])
        cv = None
        if noise_c_curve is not None:
            cva = np.ascontiguousarray(noise_c_curve, dtype=np.float32)
            assert cva.shape == (501,)
            cv = cva.ctypes.data_as(C.POINTER(C.c_float))
        iwsd = None if iws is None else (C.c_double * 9)(*[float(v) for v in np.asarray(iws, dtype=np.float64).reshape(9)])
        self._chk(LIB.artgpu_improc_denoise(self._h, C.byref(image), C.byref(params), wsd, iwsd, ecomp, scale, m, cv, flags))

    def improc_denoise_fused(self, image: RGB, params: DenoiseToolParams, ws, demosaiced: RGB = None, sx1: int = 0, sy1: int = 0, mul=(1.0, 1.0, 1.0),
                             do_clip: bool = True, cam_to_work=None, exposure=None, ecomp: float = 0.0, scale: float = 1.0, calclum_mat=None,
                             noise_c_curve=None, flags: int = 0, iws=None):
        """artgpu_improc_denoise_fused: getImage + convertColorSpace in front (demosaiced != None) and ImProcFunctions::exposure behind
        (exposure = (exp_scale, black)) inside the tool's own pixel passes"""
        fu = DenoiseFusion()
        keep = []
        if demosaiced is not None:
            keep.append(demosaiced)
            fu.demosaiced = C.pointer(demosaiced)
            fu.sx1, fu.sy1 = int(sx1), int(sy1)
            fu.mul[:] = [float(v) for v in mul]
            fu.do_clip = 1 if do_clip else 0
            if cam_to_work is not None:
                cm = (C.c_double * 9)(*[float(v) for v in np.asarray(cam_to_work, dtype=np.float64).reshape(9)])
                keep.append(cm)
                fu.cam_to_work = C.cast(cm, C.POINTER(C.c_double))
        if exposure is not None:
            fu.exposure_enabled = 1
            fu.exp_scale, fu.black = float(exposure[0]), float(exposure[1])
        wsd = (C.c_double * 9)(*[float(v) for v in np.asarray(ws, dtype=np.float64).reshape(9)])
        m = None if calclum_mat is None else (C.c_double * 9)(*[float(v) for v in np.asarray(calclum_mat, dtype=np.float64).reshape(9)])
        cv = None
        if noise_c_curve is not None:
            cva = np.ascontiguousarray(noise_c_curve, dtype=np.float32)
            assert cva.shape == (501,)
            cv = cva.ctypes.data_as(C.POINTER(C.c_float))
        iwsd = None if iws is None else (C.c_double * 9)(*[float(v) for v in np.asarray(iws, dtype=np.float64).reshape(9)])
        self._chk(LIB.artgpu_improc_denoise_fused(self._h, C.byref(image), C.byref(fu), C.byref(params), wsd, iwsd, C.c_double(ecomp), C.c_double(scale), m, cv, flags))

    # ---- wavelet_decomposition ----
    def wavelet_decompose(self, src: Plane, maxlvl: int):
        h = C.c_void_p()
        self._chk(LIB.artgpu_wavelet_decompose(self._h, C.byref(src), maxlvl, C.byref(h)))
        return h

    def wavelet_info(self, wv):
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(LIB.artgpu_wavelet_info(wv, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def wavelet_get_band(self, wv, level: int, direction: int) -> np.ndarray:
        w2, h2, _ = self.wavelet_info(wv)
        out = np.empty((h2, w2), np.float32)
        self._chk(LIB.artgpu_wavelet_get_band(self._h, wv, level, direction, out.ctypes.data, 0))
        return out

    def wavelet_set_band(self, wv, level: int, direction: int, data: np.ndarray):
        data = np.ascontiguousarray(data, dtype=np.float32)
        self._chk(LIB.artgpu_wavelet_set_band(self._h, wv, level, direction, data.ctypes.data, 0))

    def wavelet_mad(self, wv) -> np.ndarray:
        """SQR(MadRgb) of every detail band: [3 * level + dir - 1]"""
        _, _, lv = self.wavelet_info(wv)
        out = (C.c_float * (3 * lv))()
        self._chk(LIB.artgpu_wavelet_mad(self._h, wv, out))
        return np.array(out[:], dtype=np.float32)

    def wavelet_reconstruct(self, wv, dst: Plane, blend: float = 1.0):
        self._chk(LIB.artgpu_wavelet_reconstruct(self._h, wv, C.byref(dst), blend))

    def wavelet_free(self, wv):
        LIB.artgpu_wavelet_free(self._h, wv)

    # convenience for tests: host numpy in, host numpy out (staged through the library)
    def demosaic_bayer_host(self, method: int, raw: np.ndarray, filters: int, initial_gain: float = 1.0, border: int = 4):
        raw = np.ascontiguousarray(raw, dtype=np.float32)
        h, w = raw.shape
        planes = [np.full((h, w), np.nan, dtype=np.float32) for _ in range(3)]
        out = RGB(host_plane(planes[0]), host_plane(planes[1]), host_plane(planes[2]))
        self.demosaic_bayer(method, host_plane(raw), filters, initial_gain, border, out)
        return planes

    def close(self):
        if self._h:
            LIB.artgpu_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
