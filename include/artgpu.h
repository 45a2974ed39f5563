/*
 * include/artgpu.h -- C ABI of libartgpu.so: the MI355X (gfx950) implementation of ART's
 * raw-development hot path.  Plain pointers and sizes only; no C++ or torch types.
 *
 * The reference (artpixls/ART) has no FFI or plugin seam: the boundary this ABI replaces is
 * the C++ member/free-function layer of rtengine.  Each entry point names the reference
 * function whose body it stands in for; INTEGRATION.md shows the adapter a maintainer adds.
 *
 * Conventions
 *   - every function returns 0 on success, a negative ARTGPU_E* code otherwise;
 *     artgpu_last_error(ctx) gives the message.  The reference's functions return void and
 *     cannot fail (allocation failures are compiled out, rtengine/FTblockDN.cc:859); an
 *     adapter falls through to the CPU code on a non-zero return.
 *   - images are caller-owned.  artgpu_plane.on_device != 0 means `p` is a device (HBM)
 *     pointer usable on ctx's device; otherwise it is host memory and the call stages it
 *     through the context's device buffers (H2D before, D2H after).
 *   - a context is bound to one HIP device and one stream; calls on one context are
 *     serialised by the caller (the reference runs one pipeline thread per ImageProcessor,
 *     rtengine/improccoordinator.cc:192).  Device-pointer calls are asynchronous on the
 *     context's stream; host-pointer calls return after the D2H copy has completed.
 *   - there is no CPU fallback inside the library.
 */
#ifndef ARTGPU_H
#define ARTGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libartgpu.so is built with hidden visibility: what this header declares is what the library exports */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define ARTGPU_OK            0
#define ARTGPU_EINVAL       -1  /* bad argument */
#define ARTGPU_EHIP         -2  /* HIP runtime error (message has the hipError string) */
#define ARTGPU_ENOMEM       -3  /* device allocation failed */
#define ARTGPU_EUNSUPPORTED -4  /* valid in the reference, not implemented on the device path */

/* RAWParams::BayerSensor::Method values handled here (rtengine/procparams.h; dispatch at
 * rtengine/rawimagesource.cc:1862-1912). */
#define ARTGPU_BAYER_AMAZE 0
#define ARTGPU_BAYER_RCD   1
#define ARTGPU_BAYER_VNG4  2
/* second demosaicer of artgpu_dual_demosaic_bayer */
#define ARTGPU_DUAL_BILINEAR 0
#define ARTGPU_DUAL_VNG4     1

typedef struct artgpu_ctx artgpu_ctx;

/* One fp32 plane.  Mirrors array2D<float> (rtengine/array2D.h:74-296: row pointers into one
 * block, row stride W*4 bytes) and one channel of PlanarRGBData<float>
 * (rtengine/iimage.h:653-720: row stride = ceil16(W*4) bytes). */
typedef struct {
    float   *p;
    int32_t  w, h;
    int64_t  row_stride_bytes;
    int32_t  on_device;
} artgpu_plane;

typedef struct { artgpu_plane r, g, b; } artgpu_rgb;

/* Per-call device timings in milliseconds (hipEvents on the context's stream); filled only
 * when timing is enabled with artgpu_enable_timing(). */
typedef struct {
    float demosaic_ms;
    float border_ms;
    float total_ms;
} artgpu_timings;

int artgpu_create(int hip_device, artgpu_ctx **out);
int artgpu_destroy(artgpu_ctx *ctx);
const char *artgpu_last_error(const artgpu_ctx *ctx);
const char *artgpu_version(void);

/* Launch all work of this context on `hip_stream` (a hipStream_t; NULL = default stream).  Work the context has queued on its previous
 * stream is ordered before whatever it queues on the new one (its scratch memory and cached tables are shared between the two). */
int artgpu_set_stream(artgpu_ctx *ctx, void *hip_stream);
int artgpu_synchronize(artgpu_ctx *ctx);
/* Test / profiling switches of the context (they never change what a call computes, only which of two bit-identical device
 * paths runs or how scratch memory is prepared).  Unknown names return ARTGPU_EINVAL.
 *   "amaze_path"        0 (default): full AMaZE tiles are streamed through LDS (amaze_stream.hip), partial tiles and tiles the
 *                       stream hands back run on the per-tile arena kernel (amaze.hip); 1: arena kernel for every tile
 *   "amaze_split"       1 (with amaze_path 1): one kernel launch per AMaZE phase (per-phase profile)
 *   "amaze_zero_mask" / "amaze_zero_frame" / "amaze_poison"   arena-clearing experiments of tests/test_gpu_demosaic.py
 *   "amaze_overlap"     0: the arena kernel's tiles behind the stream kernel instead of beside it
 *   "amaze_grid"        n > 0: at most n stream workgroups (one per CU); 0 (default): every CU, or 5/8 of them while artgpu_batch_run has several
 *                       frames in flight (the other frames' memory-bound passes get the rest)
 *   "dn_fused"          1 (default): ShrinkAllL / ShrinkAllAB as one pass over the coefficients, one launch for the three channels where nothing has
 *                       to happen between them; 2: one launch per channel; 0: the three-kernel form (factors, row sums, column sums + update)
 *   "dn_detail_plain"   0 (default): the DCT detail recovery's trimmed kernels (blocks inside the image on a path of their own, the gather by rows);
 *                       1: the kernels before them, same bits (what tests/test_gpu_detail_paths.py compares against); 2 / 3: only the block kernel /
 *                       only the gather kernel plain
 *   "dn_mad_fold"       1 (default): MadRgb of the decomposed bands from the low bins the wavelet analysis kernels count while they write the bands
 *                       (DESIGN.md section 28), the full histogram only for a band whose median lies above them; 0: a pass over the bands, as before.
 *                       Same bits.  "dn_mad_fold_grid" n > 0: the counting kernels with at most n workgroups (tests, timing).  artgpu_get_option:
 *                       "dn_mad_fold_settled" / "dn_mad_fold_fallback": bands of the context's last RGB_denoise settled from the counts / left to
 *                       the full histogram; "dn_mad_bitsK": bit pattern of word K (0 .. 95) of its SQR(MadRgb) block
 *   "fg_grid"           n > 0: the film grain region kernel with at most n workgroups, each walking a longer chunk of tiles (tests, timing); 0 (default):
 *                       four per CU.  Same bits.
 *   "dn_streams"        0 (default since round 5): RGB_denoise's kernels one after the other on the context's stream; 1: the DCT detail recovery of L on a
 *                       side stream beside the reconstructions of a and b (the default of rounds 3 and 4); "lut_lds" 0: never the LUT-in-LDS shape
 *                       of the pixel passes; "rcd_rows" 4 | 8; "roctx" 1: roctx ranges named after the reference functions
 *   "io_direct"         artgpu_batch_run_io, scanlines that go to PINNED host memory: n > 0: n persistent workgroups on the download stream write
 *                       them there directly (no staging plane, no copy); 0: staged on the device and copied by the runtime; -1 (default): 8 with
 *                       two lanes, 0 otherwise (measured: DESIGN.md section 17); "cu_reserve" n: the persistent one-workgroup-per-CU pixel passes launch
 *                       n workgroups fewer (experiments with kernels running beside a frame).  The value is the caller's: artgpu_batch_run_io
 *                       reserves CUs for its direct downloads on its own account while it runs, the larger of the two applies, and the
 *                       option reads back as it was set (artgpu_get_option: "cu_reserve", "io_direct") */
int artgpu_set_option(artgpu_ctx *ctx, const char *name, long value);
/* read-only counterparts: "amaze_counter0" .. "amaze_counter7" = bookkeeping of the last AMaZE call (how many tiles were streamed a
 * second time, handed to the arena kernel, ...); synchronises the context's stream */
int artgpu_get_option(artgpu_ctx *ctx, const char *name, long *value);
int artgpu_enable_timing(artgpu_ctx *ctx, int enable);
int artgpu_get_timings(const artgpu_ctx *ctx, artgpu_timings *out);

/* Replaces the Bayer branch of RawImageSource::demosaic (rtengine/rawimagesource.cc:1854-1912):
 *   ARTGPU_BAYER_AMAZE -> amaze_demosaic_RT(0,0,W,H,rawData,red,green,blue)
 *                         (rtengine/amaze_demosaic_RT.cc:41-1595) including its
 *                         border_interpolate2(W,H,3,...) when border < 4 (L1587-1589);
 *   ARTGPU_BAYER_RCD   -> rcd_demosaic() (rtengine/rcd_demosaic.cc:51-347) including its
 *                         border_interpolate2(W,H,9,...) (L342).
 *   ARTGPU_BAYER_VNG4  -> vng4_demosaic(rawData, red, green, blue) (rtengine/vng4_demosaic_RT.cc:62-397) including its
 *                         border_interpolate2(W,H,3,...) (L384).  The four-colour pattern it works on (RawImage::prefilters: the second
 *                         green is colour 3) is derived from `filters` the way dcraw's identify() does.
 * raw      : the CFA plane (RawImageSource::rawData), values 0..65535
 * filters  : RawImage::filters bit pattern (rtengine/rawimage.h:186-189), RGB Bayer only
 * initial_gain : RawImageSource::initialGain (clip_pt = 1/initialGain, amaze L53-54)
 * border   : RawImageSource::border (simpleprocess.cc:138-146)
 * out      : red, green, blue (same w,h as raw), fully overwritten. */
int artgpu_demosaic_bayer(artgpu_ctx *ctx, int method, const artgpu_plane *raw, uint32_t filters,
                          double initial_gain, int border, artgpu_rgb *out);

/* border_interpolate2 alone (rtengine/demosaic_algos.cc:200-353). */
int artgpu_border_interpolate2(artgpu_ctx *ctx, const artgpu_plane *raw, uint32_t filters,
                               int lborders, artgpu_rgb *out);

/* Replaces RawImageSource::xtrans_interpolate(passes, useCieLab) (rtengine/xtrans_demosaic.cc:181-969) including the
 * final xtransborder_interpolate(passes > 1 ? 8 : 11) (L968).  ART calls it as (1, false) for ONE_PASS and (3, true)
 * for THREE_PASS (rawimagesource.cc:1920-1925).
 * xtrans : RawImage::getXtransMatrix, 6x6 row-major, 0 = R, 1 = G, 2 = B.
 * rgb_cam: RawImage::getRgbCam, 3x4 row-major (only used to build xyz_cam for the CIELab path, L219-230). */
int artgpu_demosaic_xtrans(artgpu_ctx *ctx, int passes, int use_cielab, const artgpu_plane *raw, const int32_t xtrans[36],
                           const float rgb_cam[12], artgpu_rgb *out);

/* Replaces RawImageSource::getImage for tran=0, skip=1, no highlight recovery
 * (rtengine/rawimagesource.cc:781-1104; pixel loop L940-1025), optionally fused with the matrix
 * branch of colorSpaceConversion_ (L3184-3213) when `mat` is not NULL:
 *   image(y,x) = CLIP?( planes(sy1+y, sx1+x) * mul[c] ),  then  image = (float)(mat * image)
 * planes : red/green/blue produced by artgpu_demosaic_bayer (full sensor size)
 * sx1,sy1: crop origin = RawImageSource::border (transformRect, L664-700)
 * mul    : rm, gm, bm computed by the caller as in L790-928
 * do_clip: the reference's doClip (L964-973)
 * mat    : 9 doubles row-major = work^-1 * xyz_cam (L3187-3195), or NULL
 * image  : destination Imagefloat planes (w,h = cropped size), may not alias `planes`. */
int artgpu_get_image(artgpu_ctx *ctx, const artgpu_rgb *planes, int sx1, int sy1, const float mul[3],
                     int do_clip, const double *mat, artgpu_rgb *image);
/* The same with PreviewProps::skip > 1 (the editor's zoomed-out crops, dcrop.cc:204-205): every output pixel is the sum of a
 * skip x skip window in row-major order (L944-957) times mul -- the caller divides rm/gm/bm by skip*skip as L922-926 does --
 * with the window origin clamped to (W - skip, H - skip) (L945,949).  image is ceil(crop/skip) in each direction (L745-747). */
int artgpu_get_image_skip(artgpu_ctx *ctx, const artgpu_rgb *planes, int sx1, int sy1, int skip, const float mul[3],
                          int do_clip, const double *mat, artgpu_rgb *image);

/* RawImageSource::convertColorSpace, default-camera-profile (matrix) branch, in place
 * (rtengine/rawimagesource.cc:1128-1143,3184-3213): double accumulation, float store. */
int artgpu_convert_color_space(artgpu_ctx *ctx, artgpu_rgb *image, const double mat[9]);

/* ImProcFunctions::exposure -> expcomp (rtengine/ipexposure.cc:28-79), in place:
 *   v = max(v * exp_scale - black, 0), exp_scale = pow(2.f, expcomp), black = params.black*2000
 * (both computed by the caller, L39-40). */
int artgpu_exposure(artgpu_ctx *ctx, artgpu_rgb *image, float exp_scale, float black);

/* Device part of ImProcFunctions::toneCurve (rtengine/iptonecurve.cc:553-716) for
 * curveMode == STD with a single curve: optional filmlike_clip(img, whitept) (L214-231; taken
 * when basecurve is LINEAR, L593) followed by StandardToneCurve::Apply with the 65536-entry
 * LUT that ToneCurve::Set built on the host (rtengine/curves.cc:221-231; curves.h:224-231,
 * 360-368).  `lut65536` is a HOST pointer (copied to the device), NULL = clip only.
 * whitept > 1 needs the analytic curve beyond the LUT (setLutVal's else branch) and returns
 * ARTGPU_EUNSUPPORTED; other curve modes (NEUTRAL, PERCEPTUAL, ...) likewise. */
#define ARTGPU_TONE_STD 0
#define ARTGPU_TONE_NEUTRAL 1   /* through artgpu_tone_curve_neutral */
int artgpu_tone_curve(artgpu_ctx *ctx, artgpu_rgb *image, int mode, const float *lut65536,
                      float whitept, int filmlike_clip);

/* Host look-up tables.  One lifetime rule for every entry point that takes a LUT (artgpu_tone_curve, artgpu_tone_curve_neutral,
 * artgpu_rgb_curves, artgpu_rgb2out_matrix, artgpu_lab_adjustments, ...): the caller's array is free again when the call returns.
 * The tone and rgb curves are kept in a context-owned copy (the same curve call after call is uploaded once); the others are
 * copied on the context's stream, which is drained before the call returns if the array is pinned host memory (hipHostMalloc /
 * hipHostRegister: the DMA engine reads it when the stream gets there; a pageable array has been staged by then). */

/* curves::setLutVal (rtengine/curves.h:224-231): a value above 65535 does not go through the LUT but through the Curve object,
 * curve->getVal(val / 65535.f) * 65535.f.  The LUT is all that crosses this boundary, so the adapter states what its Curve returns
 * above 1.0 (rtengine/diagonalcurves.cc:443-561); the setting applies to the following artgpu_tone_curve / artgpu_tone_curve_neutral
 * calls of the context:
 *   ARTGPU_CURVE_TAIL_LUT       no Curve object (ToneCurve::curve == nullptr): the LUT's last entry
 *   ARTGPU_CURVE_TAIL_CONSTANT  DCT_Linear / DCT_Spline / DCT_CatmullRom: the last point's y (`y_last`, L476-477, L514-515)
 *   ARTGPU_CURVE_TAIL_IDENTITY  DCT_Empty, DCT_NURBS beyond its hash table: t itself (L529-535, L557-560)
 *   ARTGPU_CURVE_TAIL_PARAMETRIC  DCT_Parametric: the analytic form (L448-470), evaluated per pixel on the device; set with
 *                               artgpu_set_curve_tail_parametric, which takes the curve's parameter vector
 *   ARTGPU_CURVE_TAIL_HOST      (default) the adapter has not said: artgpu_tone_curve then returns ARTGPU_EUNSUPPORTED for
 *                               whitept > 1; values above 65535 that reach the curve because filmlike_clip is off take the LUT's
 *                               last entry (set the tail if the image can hold such values). */
#define ARTGPU_CURVE_TAIL_LUT 0
#define ARTGPU_CURVE_TAIL_CONSTANT 1
#define ARTGPU_CURVE_TAIL_IDENTITY 2
#define ARTGPU_CURVE_TAIL_HOST 3
#define ARTGPU_CURVE_TAIL_PARAMETRIC 4
int artgpu_set_curve_tail(artgpu_ctx *ctx, int kind, double y_last);
/* DiagonalCurve(p) with p[0] == DCT_Parametric (rtengine/diagonalcurves.cc:106-131): `p` is the curve's parameter vector as the
 * reference's constructor receives it -- p[0] the kind, p[1..3] the three zone boundaries, p[4..7] highlights / lights / darks /
 * shadows (-100 .. 100), optionally p[8] -- and `np` its length (8 or 9).  The derived constants (mc, mfc, msc, mhc) are computed here
 * with the reference's double-precision sleef forms; getVal above 1.0 then runs on the device.  ARTGPU_EINVAL for an all-zero
 * slider set: that curve is the identity in the reference and has no Curve object (ARTGPU_CURVE_TAIL_LUT). */
int artgpu_set_curve_tail_parametric(artgpu_ctx *ctx, const double *p, int np);

/* rtengine::ProgressListener (rtengine/rtengine.h:165-181; the demosaicers report through it, amaze_demosaic_RT.cc:1567-1580).
 * `fn(user, stage, fraction)` is called on the calling thread by every stage-level entry point: fraction 0.0 when the stage starts
 * queueing its work, 1.0 when the entry point returns (device-resident outputs may still be in flight on the stream; host-resident
 * ones are complete).  `stage` is the name of the reference function the entry point replaces.  NULL removes the callback.
 * The same names label roctx ranges when artgpu_set_option(ctx, "roctx", 1) is set (rocprofv3 --marker-trace). */
typedef void (*artgpu_progress_fn)(void *user, const char *stage, double fraction);
int artgpu_set_progress_callback(artgpu_ctx *ctx, artgpu_progress_fn fn, void *user);

/* rtengine::wavelet_decomposition with subsampling == 1 and the 6-tap Daub4 filters, the only
 * configuration the denoise path uses (rtengine/cplx_wavelet_dec.h:97-270; constructed at
 * rtengine/FTblockDN.cc:2296,2328,2365).  The object owns its coefficients in HBM.
 *   decompose   == the constructor (level 0 decimated Daub4, levels >= 1 undecimated Haar)
 *   band access == level_coeffs(level)[dir], dir 1..3; dir 0 = coeff0 (final low-pass)
 *   reconstruct == reconstruct(dst, blend); like the reference it consumes the object's
 *                  coefficients (the low-pass is overwritten level by level).
 * Requires min(w2,h2) >= 2^maxlvl (no Haar level wider than half the plane). */
typedef struct artgpu_wavelet artgpu_wavelet;
int artgpu_wavelet_decompose(artgpu_ctx *ctx, const artgpu_plane *src, int maxlvl, artgpu_wavelet **out);
/* SQR(MadRgb(band)) of every detail band (rtengine/FTblockDN.cc:569-603: the median of (int)min(|x|, 65535) found by a histogram
 * walk, / 0.6745): mad_sqr[3 * level + dir - 1], host memory, 3 * nlevels floats.  RGB_denoise calls it on the L and ab
 * decompositions (L2307-2320, L1000-1010); exposed so that the median search can be tested on arbitrary band contents. */
int artgpu_wavelet_mad(artgpu_ctx *ctx, const artgpu_wavelet *wv, float *mad_sqr);
int artgpu_wavelet_info(const artgpu_wavelet *wv, int32_t *w2, int32_t *h2, int32_t *nlevels);
/* copy one subband out of / into the object; `host_or_device` follows `on_device` */
int artgpu_wavelet_get_band(artgpu_ctx *ctx, const artgpu_wavelet *wv, int level, int dir, float *dst, int on_device);
int artgpu_wavelet_set_band(artgpu_ctx *ctx, artgpu_wavelet *wv, int level, int dir, const float *src, int on_device);
int artgpu_wavelet_reconstruct(artgpu_ctx *ctx, artgpu_wavelet *wv, artgpu_plane *dst, float blend);
int artgpu_wavelet_free(artgpu_ctx *ctx, artgpu_wavelet *wv);

/* The fields of procparams::DenoiseParams the path reads (rtengine/procparams.cc:1901-1918). */
typedef struct {
    double  luminance;                 /* 0..100 */
    double  luminance_detail;          /* 0..100 */
    int32_t luminance_detail_threshold;
    double  chrominance;
    double  chrominance_red_green;
    double  chrominance_blue_yellow;
    double  gamma;
    int32_t aggressive;                /* 0 = standard, 1 = QUALITY_HIGH (BiShrinkL / BiShrinkAB, FTblockDN.cc:2406-2449): both on the device */
    int32_t color_space;               /* 0 = RGB, 1 = LAB (needs the inverse working-space matrix `iwpi`): both on the device */
    int32_t chrominance_method;        /* 0 = MANUAL, 1 = AUTOMATIC: artgpu_rgb_denoise only takes `autoch` from it; the estimation itself
                                          (denoiseComputeParams) is artgpu_denoise_compute_params, which artgpu_pipeline_run calls */
} artgpu_denoise_params;

#define ARTGPU_DN_SKIP_DETAIL_RECOVERY 1u  /* leave out detail_recovery (FTblockDN.cc:1479-1635) */

/* Replaces denoise::RGB_denoise(im, kall=0, src=img, dst=img, calclum, ..., isRAW=true, dnparams,
 * expcomp, noiseLCurve(empty), noiseCCurve, nresi, highresi) (rtengine/FTblockDN.cc:1638-2689) for
 * colorSpace RGB or LAB, QUALITY_STANDARD or HIGH (aggressive), one tile (Tile_calc always yields one, L442-480).
 * img      : Imagefloat planes, denoised in place
 * ws       : ICCStore::workingSpaceMatrix(params->icm.workingProfile) as 9 floats, row-major (wpi)
 * iws      : workingSpaceInverseMatrix as 9 floats (wpi_inverse, L1702-1706); only read in LAB mode, may be NULL otherwise
 * expcomp  : RGB_denoise's `expcomp` argument (gain = 2^expcomp; 0 from ImProcFunctions::denoise)
 * scale    : ImProcData::scale (1 for full-resolution export)
 * ccalc    : the quarter-resolution chroma noise-curve map `ccalc` (L1707-1777), ((w+1)/2 x (h+1)/2),
 *            or NULL when the chroma curve is off (noisevarchrom = 1)
 * flags    : ARTGPU_DN_* ; nresi/highresi: nullable, only computed when not NULL. */
int artgpu_rgb_denoise(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_denoise_params *params, const float ws[9], const float *iws,
                       double expcomp, double scale, const artgpu_plane *ccalc, uint32_t flags,
                       float *nresi, float *highresi);

/* Replaces denoise::denoiseGuidedSmoothing (rtengine/ipsmoothing.cc:875-897): normalise to [0,1],
 * guided_smoothing(R,G,B, ws, iws, Channel::C, guidedChromaRadius, 0.001, scale) (L334-409) built on
 * guidedFilterLog / guidedFilter (rtengine/guidedfilter.cc:58-265), back to [0,65535].  In place.
 * ws: ICCStore::workingSpaceMatrix as 9 DOUBLES (TMatrix), row-major. */
int artgpu_denoise_guided_smoothing(artgpu_ctx *ctx, artgpu_rgb *img, const double ws[9], int guided_chroma_radius, double scale);

/* gaussianBlur(src, src, W, H, sigma) in place for 0.6 <= sigma < 25, GAUSS_STANDARD (rtengine/gauss.cc:1387-1574:
 * gaussHorizontalSse + gaussVerticalSse, L554-665,716-856).  Other sigma ranges: ARTGPU_EUNSUPPORTED. */
int artgpu_gaussian_blur(artgpu_ctx *ctx, artgpu_plane *img, double sigma);

/* denoise::detail_mask(src, mask, scaling, threshold, ceiling, factor, BlurType::GAUSS, blur)
 * (rtengine/FTblockDN.cc:1408-1476).  mask: same size as src, written. */
int artgpu_detail_mask(artgpu_ctx *ctx, const artgpu_plane *src, artgpu_plane *mask, float scaling, float threshold,
                       float ceiling, float factor, float blur);

/* denoise::NLMeans(img, normcoeff, strength, detail_thresh, scale) (rtengine/nlmeans.cc:50-280) on one plane
 * (the Y plane after Imagefloat::setMode(YUV), ipdenoise.cc:1174-1177), in place. */
int artgpu_nlmeans(artgpu_ctx *ctx, artgpu_plane *img, float normcoeff, int strength, int detail_thresh, float scale);

/* NEUTRAL tone-curve mode (ToneCurveParams::TcMode::NEUTRAL, ART's default): replaces apply_tc(..., NEUTRAL, ...)
 * = NeutralToneCurve::ApplyState + BatchApply (rtengine/iptonecurve.cc:88-99, rtengine/curves.cc:854-1038) for
 * BcMode::LINEAR (basecurve == nullptr).  lut65536 = ToneCurve::lutToneCurve (host), whitecoeff = ToneCurve::whitecoeff.
 * ws / iws: ICCStore workingSpaceMatrix / workingSpaceInverseMatrix (doubles; cast to float inside, curves.cc:861-868);
 * to_out / to_work: the output-profile gamut matrices inverse(om)*work and iwork*om (curves.cc:870-878; identity when
 * the output profile has no matrix).  Pixels whose Jzazbz LMS response exceeds 1 evaluate powf per pixel (device powf:
 * <= 2 ulp of the host libm's), every other pixel is bit-exact. */
typedef struct {
    double ws[9], iws[9];
    float to_out[9], to_work[9];
} artgpu_neutral_state;
int artgpu_tone_curve_neutral(artgpu_ctx *ctx, artgpu_rgb *img, const float *lut65536, float whitecoeff, const artgpu_neutral_state *state);

/* NoiseCurve::Set(const std::vector<double>&) (rtengine/ipdenoise.cc:684-716): builds the 501-entry noise-curve LUT
 * from FlatCurve control points {kind, x, y, leftTangent, rightTangent, ...} on the host (pure table construction,
 * no context needed).  *sum receives NoiseCurve::getSum(); RGB_denoise uses the chroma curve only when sum > 5
 * (FTblockDN.cc:1672).  The curve ImProcFunctions::denoise always sets is
 * {1, 0.05,0.50,0.35,0.35, 0.35,0.05,0.35,0.35} (ipdenoise.cc:1139-1149). */
int artgpu_noise_curve_lut(const double *points, int npoints, float lut[501], float *sum);

/* The quarter-resolution chroma noise map `ccalc` of RGB_denoise: calclum = every second pixel of img
 * (ipdenoise.cc:1113-1129), converted by calclum_mat like RawImageSource::convertColorSpace does to it (L1131;
 * NULL = no conversion), then Color::rgbxyz(ws)/XYZ2Lab and the curve (FTblockDN.cc:1716-1777).
 * ccalc: (w+1)/2 x (h+1)/2, host or device. */
int artgpu_denoise_chroma_map(artgpu_ctx *ctx, const artgpu_rgb *img, const double *calclum_mat, const double ws[9],
                              const float noise_c_curve[501], artgpu_plane *ccalc);

/* Replaces ImProcFunctions::denoise (rtengine/ipdenoise.cc:1096-1189):
 *   calclum/ccalc map from the un-compensated image (only if noise_c_curve != NULL and its sum > 5);
 *   if (ecomp > 0) expcomp(+ecomp); RGB_denoise(kall 0, isRAW, expcomp 0); if (smoothing_enabled) {
 *   denoiseGuidedSmoothing; if (nl_strength) { setMode(YUV); NLMeans(Y, 65535, nl_strength, nl_detail, scale);
 *   setMode(RGB); } } if (ecomp > 0) expcomp(-ecomp).
 * ecomp = params->exposure.enabled ? params->exposure.expcomp : 0 (L1155).  ws: working-space matrix as doubles
 * (TMatrix); the float casts the reference makes (wpi, Imagefloat::ws_) are made inside.
 * calclum_mat / noise_c_curve as in artgpu_denoise_chroma_map; flags: ARTGPU_DN_* (0 = the reference's behaviour). */
typedef struct {
    artgpu_denoise_params dn;
    int32_t smoothing_enabled;
    int32_t guided_chroma_radius;
    int32_t nl_strength;
    int32_t nl_detail;
} artgpu_denoise_tool_params;
int artgpu_improc_denoise(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_denoise_tool_params *params, const double ws[9], const double *iws /* LAB mode only */,
                          double ecomp, double scale, const double *calclum_mat, const float *noise_c_curve, uint32_t flags);

/* The same tool with its neighbours in the processing order fused into its first and last pixel passes (simpleprocess.cc:259 getImage,
 * :311 convertColorSpace, :315 denoise, :389 process STAGE_1 -> ImProcFunctions::exposure, ipexposure.cc:28-79): per pixel the operations
 * and their order are those of the separate calls -- the image is simply not written and read again between them.
 *   demosaiced != NULL: `img` is an output only; its pixels are RawImageSource::getImage(demosaiced, sx1, sy1, skip 1, mul, do_clip) followed
 *                       by convertColorSpace(cam_to_work; NULL = none), evaluated where the denoise reads them (artgpu_get_image's arguments);
 *                       `img` must not overlap the demosaiced planes (as for artgpu_get_image: the crop shifts the pixels);
 *   exposure_enabled:   ImProcFunctions::exposure(exp_scale, black) (artgpu_exposure's arguments) is applied to the tool's result.
 * A part that cannot be fused for the given parameters (nothing to denoise, the guided smoothing / NL-means stages between the wavelet
 * denoise and the exposure, host planes) runs as the separate call it stands for: same result either way.  fusion == NULL: artgpu_improc_denoise. */
typedef struct {
    const artgpu_rgb *demosaiced;
    int32_t sx1, sy1;
    float mul[3];
    int32_t do_clip;
    const double *cam_to_work;     /* 9 doubles or NULL */
    int32_t exposure_enabled;
    float exp_scale, black;
} artgpu_denoise_fusion;
int artgpu_improc_denoise_fused(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_denoise_fusion *fusion, const artgpu_denoise_tool_params *params,
                                const double ws[9], const double *iws, double ecomp, double scale, const double *calclum_mat,
                                const float *noise_c_curve, uint32_t flags);

/* The step immediately before the path: RawImageSource::copyOriginalPixels without dark frame / flat
 * field (rawimagesource.cc:2325-2428: rawData = (float)src->data) followed by RawImageSource::scaleColors (L2677-2859):
 *   val = max(0, raw - cblacksom[c4]) * scale_mul[c4],  chmax[c] = max over the frame   (c4 = 3 for the second Bayer green).
 * src: the sensor data as uint16 (src_is_u16 != 0, row stride in BYTES as usual) or float; dst: float CFA plane.
 * cfa: Bayer `filters` word when xtrans == NULL, else the 6x6 X-Trans colour map.  The host keeps computing cblacksom /
 * scale_mul (calculate_scale_mul, L753-779: a handful of scalars).  chmax[4]: channel maxima (chmax[3] = chmax[1], L2855). */
int artgpu_scale_colors(artgpu_ctx *ctx, const void *src, int32_t w, int32_t h, int64_t src_row_stride_bytes, int32_t src_is_u16,
                        int32_t src_on_device, uint32_t filters, const int32_t *xtrans, const float cblacksom[4],
                        const float scale_mul[4], artgpu_plane *dst, float chmax[4]);

/* ImProcFunctions::denoiseComputeParams (rtengine/ipdenoise.cc:800-1093): the AUTOMATIC chrominance estimation (the default
 * chrominanceMethod, procparams.cc:1909).  Nine crops of (widIm/2) x (heiIm/2) of the white-balanced sensor planes go through
 * RGB_denoise_info (ipdenoise.cc:227-669): Lab hue/chroma/luminance statistics at half resolution, a 5-level wavelet
 * decomposition of the gamma-encoded chroma planes and the MADs of its 30 subbands (WaveletDenoiseAll_info / ShrinkAll_info,
 * FTblockDN.cc:1227-1362), calcautodn_info (ipdenoise.cc:66-206) per crop and the reduction of L960-1072.  Raw sources only
 * (imgsrc->isRAW()).
 *   planes        : RawImageSource red/green/blue after demosaic (what getImage reads)
 *   border        : RawImageSource::border (getFullSize subtracts it twice, transformRect adds it to every crop origin)
 *   mul, do_clip  : getImage's per-channel multipliers and clip flag, as for artgpu_get_image
 *   cam_to_work   : the convertColorSpace matrix, as for artgpu_convert_color_space
 *   ws            : ICCStore::workingSpaceMatrix(params->icm.workingProfile)
 *   store         : DenoiseInfoStore (improcfun.h:117-131).  valid != 0 on entry: only dn is refreshed from it (L802-809).
 *   dn            : in: gamma, aggressive, chrominance_method; out: chrominance, chrominance_red_green, chrominance_blue_yellow
 *                   = store value x chrominance_auto_factor.  chrominance_method != AUTOMATIC: nothing happens. */
typedef struct {
    int32_t valid;
    float   ch_M[9], max_r[9], max_b[9];
    double  chrominance, chrominance_red_green, chrominance_blue_yellow;
    /* diagnostics, not part of the reference's store: per crop (k = hcr*3 + wcr) {chaut, maxredaut, maxblueaut, minredaut,
     * minblueaut, chromina, lumema, redyel, skinc, nsknc, Nb, 0...} as RGB_denoise_info returns them */
    float   crop_info[9][16];
} artgpu_denoise_info_store;
int artgpu_denoise_compute_params(artgpu_ctx *ctx, const artgpu_rgb *planes, int border, const float mul[3], int do_clip,
                                  const double cam_to_work[9], const double ws[9], double chrominance_auto_factor,
                                  artgpu_denoise_info_store *store, artgpu_denoise_params *dn);

/* rtengine::guidedFilter(guide, src, dst, r, epsilon, multithread, subsampling) (guidedfilter.cc:78-241), the single-channel fast guided
 * filter behind several tools (hslEqualizer, guided smoothing, dehaze, local contrast masks): bilinear subsample by
 * calculate_subsampling (subsampling <= 0: L58-75), four box means, a / b, their means, bilinear upsample.  guide, src and dst are
 * planes of one size; dst may be src or guide.  The denoise tool's three-channel log variant is artgpu_denoise_guided_smoothing. */
int artgpu_guided_filter(artgpu_ctx *ctx, const artgpu_plane *guide, const artgpu_plane *src, artgpu_plane *dst, int r, float epsilon,
                         int subsampling);

/* ImProcFunctions::hslEqualizer (rtengine/iphsl.cc:29-221): hue / saturation / luminance adjustments as FlatCurves
 * over hue.  Each curve is the `std::vector<double>` of ProcParams (hsl.hCurve / sCurve / lCurve: {FCT_MinMaxCPoints, x, y, left
 * tangent, right tangent, ...}; NULL / n <= 4 or an identity curve = not applied), built into its polyline on the host exactly as
 * FlatCurve's constructor does (periodic, CURVES_MIN_POLY_POINTS / scale points) and evaluated per pixel on the device; the masks
 * are smoothed with rtengine::guidedFilter (radius from `smoothing` and scale, L118-123).  img is RGB on entry.  The reference leaves
 * the Imagefloat in YUV mode (g = Y, b = u, r = v); to_rgb != 0 applies Imagefloat::setMode(RGB) on top so that the planes are RGB again. */
int artgpu_hsl_equalizer(artgpu_ctx *ctx, artgpu_rgb *img, const double *hcurve, int nh, const double *scurve, int ns,
                         const double *lcurve, int nl, int smoothing, const double ws[9], double scale, int to_rgb);

/* RawImageSource::dual_demosaic_RT (rtengine/dual_demosaic_RT.cc:39-155), Bayer methods AMAZEBILINEAR / RCDBILINEAR / AMAZEVNG4 / RCDVNG4:
 * the first demosaicer (method = ARTGPU_BAYER_AMAZE or ARTGPU_BAYER_RCD, exactly artgpu_demosaic_bayer), then L* of its output
 * (Color::RGB2L, color.cc:1343-1379), the contrast blend mask (buildBlendMask, rt_algo.cc:315-498: sigmoid of the 8-neighbour contrast
 * against the threshold, 2-pixel frame, gaussian blur sigma 2) and the blend with a bilinear interpolation in flat regions
 * (bayer_bilinear_demosaic.cc:33-77).  *contrast is RAWParams::BayerSensor::dualDemosaicContrast in percent, in/out like the reference's
 * `double &contrast`: with auto_contrast != 0 the threshold is searched (flattest 80 / 40-pixel tile, calcContrastThreshold) and written
 * back.  contrast == 0 without auto_contrast runs only the first demosaicer.  second = ARTGPU_DUAL_VNG4 (AMAZEVNG4 / RCDVNG4): the flat
 * regions come from vng4_demosaic instead (all three channels of every pixel, dual_demosaic_RT.cc:128-148).  DCB as first demosaicer
 * and X-Trans (fast_xtrans_interpolate_blend) are not on the device path. */
int artgpu_dual_demosaic_bayer(artgpu_ctx *ctx, int method, int second, const artgpu_plane *raw, uint32_t filters, double initial_gain, int border,
                               double *contrast, int auto_contrast, artgpu_rgb *out);

/* ImProcFunctions::logEncoding (rtengine/iplogenc.cc:132-316,395-402): brightness-norm log tone mapping.
 * The struct holds the LogEncodingParams fields the function reads (procparams.h; defaults procparams.cc:2039-2051); `enabled == 0`
 * returns at once like the reference.  regularization > 0 smooths the posterised log-norm with rtengine::guidedFilter at radius
 * max(full_width, W, full_height, H) / 30 (full_width/height = ImProcFunctions::full_width/full_height, the uncropped image size).
 * highlight_compression > 0 (L148-170) evaluates std::pow(float, float) twice per pixel above 0.8; the C library's powf is not
 * specified bit for bit, the device uses double-precision pow rounded to float: identical to glibc's result except for a few
 * values per million (at most 1.2e-6 relative; tests/test_gpu_logenc.py holds the bound).  Every other branch is bit-exact. */
typedef struct artgpu_logenc_params {
    int32_t enabled;
    int32_t regularization;          /* 0..100 */
    int32_t satcontrol;
    int32_t highlight_compression;   /* 0..100 */
    double gain, target_gray, black_ev, white_ev;
} artgpu_logenc_params;
int artgpu_log_encoding(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_logenc_params *p, const double ws[9], int full_width, int full_height);

/* ImProcFunctions::labAdjustments (rtengine/iplabadjustments.cc:277-345) as the four device steps the function is
 * made of; the caller keeps building the three curves (get_L_curve / get_ab_curves, DiagonalCurve: host code), exactly where it does now:
 *   artgpu_rgb_to_lab      Imagefloat::setMode(LAB) from RGB = rgb_to_lab (imagefloat.cc:841-876): in place, afterwards g = L, r = a, b = b.
 *                          ws = the working-space TMatrix (narrowed to float like Imagefloat::get_ws).
 *   artgpu_lab_histogram   hist16[(int)L]++ over the L plane (L300-327; 65536 bins, index clamped like LUTu::operator[]) - only needed
 *                          when labCurve.contrast != 0.
 *   artgpu_lab_adjustments lab_adjustments' curve loop (L236-264): L = lcurve[L], a = (acurve[a + 32768] - 32768) * chroma, same for b.
 *                          lcurve has 32770 entries (LUTf(32770, 0)), acurve / bcurve 65536; chroma = (chromaticity + 100) / 100.
 *   artgpu_lab_to_rgb      the next setMode(RGB) = lab_to_rgb (imagefloat.cc:941-970), iws = the inverse working-space matrix.
 * The reference runs all of them four pixels at a time with a scalar tail and the two forms round differently; the device follows the
 * form of each pixel's column (and, for XYZ2Lab, of its group of four). */
int artgpu_rgb_to_lab(artgpu_ctx *ctx, artgpu_rgb *img, const double ws[9]);
int artgpu_lab_to_rgb(artgpu_ctx *ctx, artgpu_rgb *img, const double iws[9]);
/* Imagefloat::setMode(YUV) on an image in LAB mode = lab_to_yuv (imagefloat.cc:988-1022), in place: Lab2XYZ, xyz2rgb with iws, then g = Y,
 * b = Y - B, r = R - Y with the Y of XYZ.  Columns below 4 * (W / 4) take the 4-wide body's Lab2XYZ, the others the scalar one, as in
 * artgpu_lab_to_rgb.  In bits this is NOT artgpu_lab_to_rgb followed by the RGB -> YUV switch (there Y is a row of ws times the rounded RGB). */
int artgpu_lab_to_yuv(artgpu_ctx *ctx, artgpu_rgb *img, const double iws[9]);
int artgpu_lab_histogram(artgpu_ctx *ctx, const artgpu_rgb *img, uint32_t hist[65536]);
int artgpu_lab_adjustments(artgpu_ctx *ctx, artgpu_rgb *img, const float *lcurve, const float *acurve, const float *bcurve, float chroma);

/* SURVEY section 8f N1, the parts of the output stage that are plain arithmetic (everything lcms2 evaluates stays on the host):
 * artgpu_rgb2out_matrix : ARTOutputProfile::operator()(const Imagefloat*, Imagefloat*), the matrix + TRC fast path of
 *                         ImProcFunctions::rgb2out for matrix output profiles (iprgb2out.cc:94-172,452-461).  matrix = the host's
 *                         `matrix_` (inverse profile matrix x working space, L119); trc_linear != 0 for MODE_LINEAR; otherwise
 *                         lut/lutsz = the host's `lut_` (compute_lut, L207-215; preview pipelines use 65536 / 1024 / 256 entries).
 *                         Values > 1 in a non-linear mode need ARTOutputProfile::eval (lcms2 / libm): the call then fails with
 *                         ARTGPU_EUNSUPPORTED after counting them (dst is complete for all other pixels).
 * artgpu_get_scanlines  : Imagefloat::getScanline for all rows (imagefloat.cc:125-170): interleaved RGB as the TIFF/PNG/JPEG
 *                         writers consume it; (bps, is_float) = (8,0), (16,0), (16,1: half, DNG_FloatToHalf), (32,1).  Moves 3-6 B/px
 *                         to the host instead of 12. */
int artgpu_rgb2out_matrix(artgpu_ctx *ctx, const artgpu_rgb *src, artgpu_rgb *dst, const float matrix[9], int trc_linear,
                          const float *lut, int lutsz);
int artgpu_get_scanlines(artgpu_ctx *ctx, const artgpu_rgb *img, int bps, int is_float, void *dst, int64_t dst_row_stride_bytes,
                         int dst_on_device);

/* acc = 0; for (i = 0; i < n; ++i) acc += x[i];  in fp32 -- the order-defined sum the reference uses for its image statistics
 * (ShrinkAll_info, FTblockDN.cc:1237-1290), evaluated on the device by an exact parallel scan (values >= 0 take the fast path;
 * anything else is still exact, one value at a time).  Exported because it is the building block of
 * artgpu_denoise_compute_params that is worth testing on its own. */
int artgpu_ordered_sum_f32(artgpu_ctx *ctx, const float *x, int64_t n, int on_device, float *result);

/* The device-side math primitives of the path (art_amd/csrc/devmath.h, devsleef.h, paramcurve.h -- every kernel is built from them),
 * evaluated one value per lane on host arrays of n values: out0[i] = f(a[i] [, b[i] [, c[i]]]).  Diagnostic entry point: it lets a caller
 * (tests/test_gpu_primitives.py) compare the GPU's results bit for bit with fixtures generated from the reference's own headers
 * compiled in place -- rtengine/sleef.h:938-966,1198-1313 (xexpf, xlogf, pow_F, xlin2log, xlog2lin, xcbrtf, xatan2f, double xlog / xexp),
 * sleefsseavx.h:978-1000,1232-1345 (the 4-lane forms, whose last bits differ), sleefsseavx.h:1435-1442 + helpersse2.h:168-179 (vminf / vmaxf
 * operand order, vintpf), median.h (median3), LUT.h:349-377 / 436-459 (LUTf::operator[] for vfloat / float).  The product path never calls it.
 * XSINCOSF writes sin to out0 and cos to out1; XLIN2LOG / XLOG2LIN take the base in `param`; the LUTF_* forms look a[i] up in
 * table[table_size]; XLOG_D / XEXP_D read and write double arrays; FLOAT_TO_HALF (DNG_FloatToHalf, halffloat.h:9-46: the half-float scanlines)
 * writes 32-bit words with the half in the low 16 bits; XSINF_S / XCOSF_S are sleef.h:993-1046's scalar xsinf and xcosf, the latter being lane 0 of
 * sleefsseavx.h:1024-1049's vector form under SSE2 (tests/test_gpu_creative_primitives.py).  Returns ARTGPU_EINVAL for a missing operand. */
enum {
    ARTGPU_PRIM_XEXPF_S = 0, ARTGPU_PRIM_XEXPF_V, ARTGPU_PRIM_XEXPF_VN, ARTGPU_PRIM_XEXPF_V_LDEXP, ARTGPU_PRIM_XLOGF_S, ARTGPU_PRIM_XLOGF_V,
    ARTGPU_PRIM_XLOGF_VN, ARTGPU_PRIM_POW_F, ARTGPU_PRIM_XLIN2LOG, ARTGPU_PRIM_XLOG2LIN, ARTGPU_PRIM_XCBRTF, ARTGPU_PRIM_XATAN2F,
    ARTGPU_PRIM_XSINCOSF, ARTGPU_PRIM_LUTF_SCALAR, ARTGPU_PRIM_LUTF_VECTOR, ARTGPU_PRIM_MEDIAN3, ARTGPU_PRIM_VMINF, ARTGPU_PRIM_VMAXF,
    ARTGPU_PRIM_VINTPF, ARTGPU_PRIM_XDIV2F, ARTGPU_PRIM_XDIVF2, ARTGPU_PRIM_XLOG_D, ARTGPU_PRIM_XEXP_D, ARTGPU_PRIM_FLOAT_TO_HALF,
    ARTGPU_PRIM_XSINF_S, ARTGPU_PRIM_XCOSF_S,
    ARTGPU_PRIM_COUNT
};
int artgpu_eval_primitive(artgpu_ctx *ctx, int prim, const void *a, const void *b, const void *c, void *out0, void *out1, int64_t n,
                          float param, const float *table, int table_size);

/* Two of the default-off pixelwise steps of ImProcFunctions::process, so that a frame with these
 * common edits stays on the device:
 * artgpu_channel_mixer : the pixel loop of ImProcFunctions::channelMixer (ipchmixer.cc:185-230); m = {RR,RG,RB, GR,GG,GB,
 *                        BR,BG,BB} as the function computes them (params/1000, or get_mixer_matrix for PRIMARIES_CHROMA).
 * artgpu_rgb_curves    : the pixel loop of ImProcFunctions::rgbCurves (iprgbcurves.cc:116-143); each LUT is the 65536-entry
 *                        `outCurve` RGBCurve() builds on the host (L41-53), NULL for an identity curve. */
int artgpu_channel_mixer(artgpu_ctx *ctx, artgpu_rgb *img, const float m[9]);
int artgpu_rgb_curves(artgpu_ctx *ctx, artgpu_rgb *img, const float *rcurve, const float *gcurve, const float *bcurve);
/* ImProcFunctions::saturationVibrance (ipsaturation.cc:43-83): saturation, vibrance = params->saturation.{saturation,vibrance}
 * (integers; both 0 = nothing to do), ws = working-space matrix (row 1 is the luminance). */
int artgpu_saturation_vibrance(artgpu_ctx *ctx, artgpu_rgb *img, int saturation, int vibrance, const double ws[9]);

/* RawImageSource::CA_correct_RT (rtengine/CA_correct_RT.cc:122-1384) for one frame (numFrames == 1, no fitParamsTransfer), called
 * after scaleColors and before the demosaic (rawimagesource.cc:1827-1840).  In place on the scaled CFA plane `raw` (host or device;
 * a host plane is staged and written back).  Auto mode: caautoiterations passes of detection (tiles of 128, step 112), 4th-order
 * (linear under 32 blocks) fit and correction; fewer than 10 usable blocks or a vanishing block denominator end the iterations
 * without pass 2, which is not an error.  Manual mode: one pass with shifts from red / blue (L1040-1046).  avoid_colour_shift:
 * the factors oldraw / raw at R and B sites, blurred by gaussianBlur(sigma 30), multiplied back after every iteration
 * (L168-181,1276-1352).  Block sums are taken in tile raster order (the reference leaves that order to its thread schedule).
 * fit_out (may be NULL): fitparams[2][2][16] ([colour][dir][coefficient]) of the last fit that ran, zeros where none did; a non-NULL
 * fit_out makes the call wait for the stream.  ARTGPU_EUNSUPPORTED, plane untouched: X-Trans (filters == 9), a fourth colour,
 * a frame under 64x64.  Manual shifts are not limited, as in the reference (ART's sliders reach 8, i.e. 8 * H / W px); past
 * 60 px, where the reference's reads would leave its tile's colour planes, they are held at 60.  Manual mode reads the G
 * half plane where its own interpolation does not reach (tile borders); the reference leaves that plane unwritten in manual mode,
 * the device zeroes it. */
typedef struct {
    int32_t autocorrect;          /* RAWParams::ca_autocorrect */
    int32_t iterations;           /* caautoiterations (auto only; < 1 means 1, as the reference) */
    double  red, blue;            /* cared, cablue (manual only) */
    int32_t avoid_colour_shift;   /* ca_avoidcolourshift */
} artgpu_ca_params;
int artgpu_raw_ca_correct(artgpu_ctx *ctx, artgpu_plane *raw, uint32_t filters, const artgpu_ca_params *p, double fit_out[64]);

/* ImProcFunctions::localContrast (rtengine/iplocalcontrast.cc:425-487; called at improcfun.cc:625) on the L plane of an image in LAB mode
 * (artgpu_rgb_to_lab: Imagefloat::g), in place; the plane may be on the host or on the device, with any row stride.  For every region, in
 * order: local_contrast_wavelets (L251-420) -- wavelet_decomposition(L, level, subsamp 1) with the level rule of L256-260, the contrast
 * remap of coeff0 (L271-347), evaluate_params (L97-248: double sums in a fixed order on the device, no atomics), the curve remap of the
 * detail bands (L365-417), reconstruct(L, 1.f) -- then rgb->g = intp(mask, L_new, l) (L474-480; a NULL mask does the same arithmetic with
 * 1.f), and L carries on into the next region.  The caller keeps what is host code in the reference: generateMasks' blend planes and
 * the `masks[i].enabled` test (a disabled region is simply not passed).
 * The constants of L372-380 go through the C library's log, so they are computed on the host: per region the call waits once for the
 * stream, for the statistics block.  A non-NULL `info` receives what the last region computed.
 * ARTGPU_EUNSUPPORTED, plane untouched: scale != 1 (wavelet_decomposition's skip form is not on the device path); a plane narrower or
 * lower than ARTGPU_LOCAL_CONTRAST_MIN_SIZE, the smallest size at which the wavelet kernels take the level count the reference chooses
 * (artgpu_wavelet_decompose: w, h >= 8 and min(w2, h2) >= 2^(levels - 1), which the level rule satisfies from 8 up).
 * Device scratch (context pool, artgpu_trim_scratch returns it): 3 * levels + 2 quarter-size band planes and one full-size plane. */
#define ARTGPU_LOCAL_CONTRAST_MIN_SIZE 8
typedef struct {
    double contrast;              /* LocalContrastParams::Region::contrast */
    const float *curve;           /* 501 entries (host), WavOpacityCurveWL's LUT; NULL = unset curve (operator[] returns 0, L53-56) */
    const artgpu_plane *mask;     /* generateMasks' blend plane for this region (host or device); NULL = all ones */
} artgpu_local_contrast_region;
typedef struct {                  /* what the last region computed; filled only when asked for */
    int32_t nlevels;
    float ave, min0, max0;        /* coeff0 statistics (ave as the float of L317; min0 / max0 before the / 327.68); 0 when contrast == 0 */
    float mean[10], sigma[10], maxp[10];   /* evaluate_params' mean, sigma, MaxP per level */
} artgpu_local_contrast_info;
/* WavOpacityCurveWL::Set(const std::vector<double>&) (L85-94): the 501-entry LUT of a FlatCurve {FCT_MinMaxCPoints, x, y, left tangent,
 * right tangent, ...} with identity value 0, on the host (no context needed).  *is_set = 0 (lut zeroed) for an empty, FCT_Linear or identity
 * curve, whose LUT the reference leaves unset; in the empty / FCT_Linear case the caller passes the default region's curve
 * {1, 0, 0.5, 0, 0, 1, 0.5, 0, 0} instead, as L358-363 do. */
int artgpu_local_contrast_curve_lut(const double *points, int npoints, float lut[501], int *is_set);
int artgpu_local_contrast(artgpu_ctx *ctx, artgpu_plane *L, const artgpu_local_contrast_region *regions, int nregions,
                          double scale, artgpu_local_contrast_info *info /* may be NULL */);

/* ImProcFunctions::dehaze (rtengine/ipdehaze.cc:306-512; the first step of ImProcFunctions::process, improcfun.cc:577, STAGE_0): haze
 * removal by the dark channel prior, in place on an RGB image whose planes are on the host or on the device, with any row stride.
 * The call follows the reference step by step: normalize (L64-80: maxval = max(2 * max(r, g, b), 65535), the image times
 * 1.f / maxval -- a multiplication by a reciprocal, which the final * maxval does not undo in bits), subtract_black when
 * blackpoint != 0 (L249-301), extract_channels (L233-246: three self-guided filters, r = max(int(5 / scale), 2), epsilon 0.1f),
 * rescaleNearest to the ww x hh thumbnail (L372-381; for portrait frames ww = 200 / (W / H) is larger than 200 and hh = 200),
 * the ambient light (L385-386), the dark channel with patchsize = max(max(W, H) / 600, 2), the ambient light and the clip (L396-404),
 * t~ = 1 - |s| * dark with s = strength[rgbLuminance(r, g, b, ws) * maxval] (L419-436), guidedFilter(B, t~, t, 4 * patchsize, 1e-5f)
 * (L438-445), the recovery loop with all of its branches (L453-509) and restore (L511).  When the ambient estimate finds no haze
 * (max_t < 0, L387-393) the image returned is restore() of the normalised, black-subtracted image, not the input, and
 * info->haze_detected = 0.  ws = the working-space matrix (row 1 is the luminance), scale = ImProcFunctions::scale.
 * Every reduction of the tool is a maximum or a minimum, so the result does not depend on the order the device takes them in; the
 * few log / exp (float overloads) and double sums work on the thumbnail and run on the host: the call waits once for the stream, for
 * the three thumbnail planes.  Contract: NaN-free input (normalize's max depends on the order for NaN).
 * ARTGPU_EUNSUPPORTED, image untouched, where the reference itself reads out of bounds or the kernels have a limit:
 *   - blackpoint != 0 with min(ww, hh) < 2 * (max(ww, hh) / 20) + 1: the thumbnail is narrower than the box blur's window
 *     (boxblur.h:318 needs W, H >= 2 * radius + 1), an aspect ratio above about 9.5;
 *   - a side shorter than the guided filters' subsampling (W / s or H / s == 0: rescaleBilinear to an empty grid);
 *   - max(W, H) >= 600 * 257 (a patch wider than the dark-channel kernel's workgroup).
 * Device scratch (context pool, artgpu_trim_scratch returns it): one full-size plane, the guided filters' statistics grids (six planes
 * of W / s x H / s twice), the patch grid, the thumbnails and the strength table. */
typedef struct artgpu_dehaze_params {
    int32_t enabled;                  /* DehazeParams::enabled; 0: the call returns at once (L315-320) */
    const double *strength;           /* DehazeParams::strength, FlatCurve points {FCT_MinMaxCPoints, x, y, lt, rt, ...}; */
    int32_t nstrength;                /*   default procparams.cc:2694-2711: {1, 0, 0.75, 0, 0, 1, 0.75, 0, 0} */
    int32_t show_depth_map, depth, luminance, blackpoint;
} artgpu_dehaze_params;
typedef struct artgpu_dehaze_info {   /* what the call derived; for callers and for locating a mismatch */
    int32_t haze_detected;            /* 0: the "no haze" return; ambient and t0 are then 0 */
    int32_t patchsize;                /* max(max(W, H) / 600, 2) */
    int32_t small_w, small_h;         /* the thumbnail, ww x hh */
    float maxval, black[3], ambient[3], max_t, t0;
} artgpu_dehaze_info;
int artgpu_dehaze(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_dehaze_params *params, const double ws[9], double scale,
                  artgpu_dehaze_info *info /* may be NULL */);
/* L419-424 on the host (no context needed): lut[i] = (FlatCurve(points, false).getVal(Color::gamma2curve[i] / 65535.f) - 0.5f) * 1.3f
 * with identity value 0.5; Color::gamma2curve as color.cc:241-244 build it (gamma2 in double, stored as float, *= 65535.f).  An empty,
 * FCT_Linear or identity curve gives all zeros. */
int artgpu_dehaze_strength_lut(const double *points, int npoints, float lut[65536]);
/* get_dark_channel(RR, GG, BB, D, 2, nullptr, false) and estimate_ambient_light (L128-230, L385-386) on the host, on three contiguous
 * ww x hh planes: the ambient light and max_t; *max_t < 0 (ambient zeroed) when no dark-channel value lies in [0, 1 - 1e-5]. */
int artgpu_dehaze_estimate_ambient(const float *R, const float *G, const float *B, int ww, int hh, float ambient[3], float *max_t);
/* get_dark_channel (L89-125) on the device: dst = per patchsize x patchsize patch (edge patches are partial) the minimum of r, g, b, each
 * divided by its ambient component when `ambient` is not NULL, LIM01 of it when clip != 0.  With positive ambient components the
 * division is taken once per channel and patch (x / a is monotonic in x, the bits are the same); otherwise per pixel, as written.
 * The sign of a zero result is not defined (the minimum of zeros of opposite sign depends on the order).  patchsize 1 .. 256. */
int artgpu_dehaze_dark_channel(artgpu_ctx *ctx, const artgpu_rgb *rgb, int patchsize, const float *ambient /* [3] or NULL */, int clip,
                               artgpu_plane *dst);

/* Capture sharpening: ImProcFunctions::doSharpening(img, params->sharpening, false) for method "rld" (rtengine/ipsharpen.cc:712-788; the
 * first step of STAGE_2, improcfun.cc:595), in place on an RGB image whose planes are on the host or on the device, with any row stride.
 *   early-outs (L717: !enabled, amount < 1, W < 8, H < 8): the image is untouched, the call succeeds;
 *   Y = r * ws[1][0] + g * ws[1][1] + b * ws[1][2] in float (rt_algo.cc:942-956; TMatrix is float here: row 1 of `ws` is rounded once);
 *   the blend mask: buildBlendMask(Y, blend, W, H, pow_F(contrast / 100.f, 1.2f) * sqrt(scale), 1.f, false, 2.f / sqrt(scale)) (L726-729);
 *   markImpulse(W, H, Y, impulse, 2.f) (rt_algo.cc:497-596): gaussian sigma 2, the 25-term sum of |src - lpf| in row-major order, the
 *   sign-bit test in the columns of the reference's 4-wide loop and `>` elsewhere;
 *   deconvsharpening (L144-229) with sigma = deconvradius / scale, amount = deconvamount / 100.f: twenty Richardson-Lucy iterations of
 *   gaussianBlur(GAUSS_DIV) and gaussianBlur(GAUSS_MULT) with check_stop, see artgpu_rl_deconvolution;
 *   the corner boost when deconvCornerBoost / scale > 0.01f: a second run at sigma + delta, blended by CornerBoostMask (L315-340, L758-774);
 *   multiply (rt_algo.cc:958-976): the three planes times YY / Y where Y > 0.
 * Where deconvsharpening returns early (amount <= 0, sigma < 0.2f) the planes are still multiplied by Y / Y, as in the reference.
 * ARTGPU_EUNSUPPORTED, image untouched: another method (usm, psf); a sigma (after the corner-boost delta as well) that is not finite or
 * is >= 25 (the reference's behaviour there is an accident of NaN comparisons); 2 / sqrt(scale) < 0.6 (the mask blur leaves the shared
 * gaussian's range).  Not built: show_sharpening_mask, prsharpening.
 * Device scratch (context pool, artgpu_trim_scratch returns it): eight full-size planes and a byte plane, one plane more with corner boost. */
#define ARTGPU_SHARPEN_RLD 0
#define ARTGPU_SHARPEN_USM 1
#define ARTGPU_SHARPEN_PSF 2
#define ARTGPU_SHARPEN_REGIME_COPY 0   /* sigma in [0.2, 0.25): gaussianBlur copies */
#define ARTGPU_SHARPEN_REGIME_3X3  1   /* [0.25, 0.6) */
#define ARTGPU_SHARPEN_REGIME_5X5  2   /* [0.6, 0.84] */
#define ARTGPU_SHARPEN_REGIME_7X7  3   /* (0.84, 1.15] */
#define ARTGPU_SHARPEN_REGIME_YVV  4   /* (1.15, 25): the recursive gaussian */
typedef struct artgpu_sharpening_params {   /* SharpeningParams (procparams.h:669-693; defaults procparams.cc:1756-1775) */
    int32_t enabled;
    int32_t method;                   /* ARTGPU_SHARPEN_* */
    int32_t amount;                   /* only its `< 1` early-out is read on this path (L717) */
    int32_t deconvamount;
    double contrast;
    double deconvradius;
    double deconvCornerBoost;
    int32_t deconvCornerLatitude;
    int32_t offset_x, offset_y;       /* ImProcFunctions::offset_x / offset_y / full_width / full_height: where the image lies in the */
    int32_t full_width, full_height;  /*   full frame (corner boost only); 0 = W / H (L763-764) */
    int32_t pad_;
} artgpu_sharpening_params;
typedef struct artgpu_sharpening_info {     /* what the call derived; filling it costs a host wait, so it is filled only when asked for */
    double sigma;                     /* of the (first) deconvolution */
    int32_t regime;                   /* ARTGPU_SHARPEN_REGIME_*; -1: no iteration ran */
    int32_t early_out;                /* 0 none; 1 !enabled, 2 amount < 1, 3 W or H < 8 (doSharpening); 4 amount <= 0, 5 sigma < 0.2f (deconvsharpening) */
    float contrast_threshold;         /* pow_F(contrast / 100.f, 1.2f) * sqrt(scale); 0 from artgpu_rl_deconvolution */
    int32_t pad_;
    int64_t impulse_pixels;           /* non-zero bytes of the impulse map */
    int64_t frozen_pixels;            /* pixels check_stop froze before the last iteration (iterations 1 .. 19 of 20) */
} artgpu_sharpening_info;
int artgpu_sharpening(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_sharpening_params *params, const double ws[9], double scale,
                      artgpu_sharpening_info *info /* may be NULL */);
/* deconvsharpening(luminance, blend, impulse, W, H, sigma, amount) (ipsharpen.cc:144-229) in place on `luminance`: + 1000, the estimate
 * max(l, 0), twenty times  tmp = l / blur(estimate) (GAUSS_DIV), estimate *= blur(tmp) (GAUSS_MULT), check_stop (a pixel whose estimate
 * leaves l +- 0.2 l is frozen at get_output the first time that happens and goes on iterating for its neighbours), then get_output and
 * max(l - 1000, 0).  For the stencil regimes an iteration is ONE kernel (the estimate ping-pongs between two planes); above 1.15 the
 * recurrences are the shared recursive gaussian and the DIV / MULT / check_stop steps run behind it.  amount <= 0 or sigma < 0.2f: nothing
 * happens (L146-156).  sigma not finite or >= 25: ARTGPU_EUNSUPPORTED.  W, H >= 8.  impulse: W * H bytes, rows of W, on the host or on
 * the device like `luminance`; blend: a plane of the same size, either residency. */
int artgpu_rl_deconvolution(artgpu_ctx *ctx, artgpu_plane *luminance, const artgpu_plane *blend, const uint8_t *impulse,
                            double sigma, float amount, artgpu_sharpening_info *info /* may be NULL */);
/* gaussianBlur(src, dst, W, H, sigma, nullptr, gausstype, div) for src != dst and the GAUSS_DIV / GAUSS_MULT types (gauss.cc:1437-1523):
 *   sigma < 0.25 a copy (whatever the type); [0.25, 0.6) gauss3x3div / gauss3x3mult with their edge formulas; [0.6, 0.84] and (0.84, 1.15]
 *   the 5x5 / 7x7 forms (DIV writes 1.f into a ring of width 2 / 3 and divides by max(val, 0.00001f); MULT leaves the ring of dst alone;
 *   the 7x7 forms multiply one term of the c21 group by c21 twice, L302 / L404); (1.15, 25) gaussHorizontalSse + gaussVerticalSsediv /
 *   gaussVerticalSsemult (the 8-column groups' last three rows carry no max(.., 0)).
 * DIV: dst = div / blur(src) in the form's rule.  MULT: dst is read and written, dst *= blur(src).  Above 1.15 the reference filters src in
 * place for MULT: `src` IS OVERWRITTEN there (with the blurred plane; its content is not part of the contract).  Planes on the host or on the
 * device, any row stride, W, H >= 8; sigma not finite or >= 25 and GAUSS_STANDARD (artgpu_gaussian_blur): ARTGPU_EUNSUPPORTED. */
#define ARTGPU_GAUSS_STANDARD 0
#define ARTGPU_GAUSS_MULT 1
#define ARTGPU_GAUSS_DIV 2
int artgpu_gaussian_blur_ex(artgpu_ctx *ctx, artgpu_plane *src, artgpu_plane *dst, const artgpu_plane *div /* DIV only */, double sigma,
                            int gausstype);
/* RawImageSource::getDeconvAutoRadius for Bayer and monochrome sensors = calcRadiusBayer(rawData, W, H, lower_limit, clip_val, fc)
 * (deconvautoradius.cc:39-96, 200-245): one pass over the green sites of rows 4 .. H - 5 (columns 5 + (FC(row, 0) & 1), step 2, below
 * W - 4) and their two lower diagonal neighbours.  The reference adopts a pair only if maxVal > maxRatio * minVal, under an OpenMP
 * max-reduction, so its own result depends on the thread schedule in the last place; the contract here is
 *   *max_ratio = max(1, fl(maxVal / minVal)) over ALL eligible pairs (both values positive, maxVal > lower_limit, neither clipped rule
 *   fires), a tree of maxima: deterministic;  *radius = sqrt((1 / (log(1 / max_ratio) / 2)) / -2) in the float overloads, on the host.
 * filters: the Bayer pattern; 0 = monochrome (fc = {0, 0}).  max_ratio == 1 (no eligible pair) makes the radius NaN as in the reference:
 * it is returned and the caller decides (artgpu_sharpening rejects it).  The call waits for the stream.  X-Trans (filters == 9,
 * calcRadiusXtrans): ARTGPU_EUNSUPPORTED. */
int artgpu_deconv_auto_radius(artgpu_ctx *ctx, const artgpu_plane *raw, uint32_t filters, float lower_limit, float clip_val,
                              float *radius, float *max_ratio /* may be NULL */);

/* Impulse noise reduction: ImProcFunctions::impulsedenoise (rtengine/impulse_denoise.cc:179-189; the second tool of STAGE_2,
 * improcfun.cc:589-603) with impulse_nr (L33-174), in place on an image in RGB mode (host or device, any row stride or start offset):
 *   the gates of L182: enabled, W >= 8, H >= 8, scale >= 0.5 -- otherwise nothing happens and the call succeeds (info->early_out says which);
 *   float t = thresh / scale (the quotient in double, narrowed); impulse_nr(img, t / 20.0) hands markImpulse the float of that double;
 *   setMode(LAB) (artgpu_rgb_to_lab with `ws`): afterwards g = L, r = a, b = b;
 *   markImpulse on the L plane (rt_algo.cc:497-596): the low-pass is gaussianBlur at max(2.f, thresh - 1.f), always the recursive gaussian;
 *   impthr = max(1.f, 5.5f - thresh); a pixel is impish when |L - lpf| exceeds impthr / 24 times the sum over the rest of its 5 x 5 window
 *   (the columns the reference's 4-wide loop covers test the sign bit as _mm_movemask_ps does);
 *   for every impish pixel, over its 5 x 5 window clamped at the four edges, row-major, skipping impish neighbours:
 *   dirwt = 1 / (SQR(L[i1][j1] - L[i][j]) + 1.f), norm += dirwt and three sums of dirwt * {L, a, b} (float, unfused, from 0); the three
 *   quotients by norm are written `if (norm)`.  Only impish pixels are written and only other pixels are read, so the result does not
 *   depend on the order of the pixels: the reference's bits.
 * to_rgb != 0 applies setMode(RGB) (artgpu_lab_to_rgb with `iws`) on top; the reference leaves the image in LAB mode (to_rgb == 0, `iws` may
 * then be NULL), as artgpu_texture_boost's to_rgb.  A non-NULL `info` costs the call's one host wait.
 * ARTGPU_EINVAL, image untouched: a bad image, NULL params or ws, to_rgb without iws.
 * Device scratch (context pool, shared with artgpu_sharpening): three full-size planes and a byte plane. */
typedef struct artgpu_impulse_denoise_params {   /* ImpulseDenoiseParams (procparams.h:736-744; defaults: off, 50) */
    int32_t enabled;
    int32_t thresh;
} artgpu_impulse_denoise_params;
typedef struct artgpu_impulse_denoise_info {
    int32_t early_out;                /* 0 none; 1 !enabled, 2 W or H < 8, 3 scale < 0.5 (or not a number) */
    float thresh;                     /* what markImpulse received */
    float sigma;                      /* max(2.f, thresh - 1.f) */
    float impthr;                     /* max(1.f, 5.5f - thresh) */
    int64_t impulse_pixels;           /* non-zero bytes of the impulse map */
} artgpu_impulse_denoise_info;
int artgpu_impulse_denoise(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_impulse_denoise_params *params, const double ws[9],
                           const double *iws /* to_rgb only */, double scale, int to_rgb, artgpu_impulse_denoise_info *info /* may be NULL */);

/* Defringe: ImProcFunctions::defringe (rtengine/PF_correct_RT.cc:210-218; the third tool of STAGE_2) with PF_correct_RT (L44-205), in place
 * on an image in RGB mode (host or device, any row stride or start offset):
 *   the gates of L212: enabled, W >= 8, H >= 8 -- otherwise nothing happens and the call succeeds (info->early_out says which);
 *   radius = params.radius / scale in double, halfwin = ceil(2 * radius) + 1; setMode(LAB) (g = L, r = a, b = b);
 *   tmpa = gaussianBlur(a), tmpb = gaussianBlur(b), src != dst, GAUSS_STANDARD (gauss.cc:1437-1523): a copy below 0.25, the non-separated
 *   gauss3x3 (gauss.cc:129-174, coefficients in double on the host, L1448-1461) in [0.25, 0.6), the recursive gaussian from 0.6;
 *   L73-114: chroma = chromaChfactor * (SQR(a - tmpa) + SQR(b - tmpb)); with a hue curve (huecurve non-empty and huecurve[0] above
 *   FCT_Linear; the tool's default has one) chromaChfactor = SQR(1.f + chparam), chparam = float(curve.getVal(huelab_to_huehsv2(xatan2f(b,
 *   a))) - 0.5f), doubled when negative; the curve is FlatCurve(huecurve) (periodic, 1000 polygon points), evaluated in double;
 *   chromave = the double sum of the float chroma values / (H * W).  DEFINITION 1: the reference's sum is an OpenMP reduction whose last
 *   bits depend on the schedule; here it is taken in a fixed order that depends on W * H alone (pixels in row-major index order form chunks of
 *   4096; within a chunk 256 strided sub-sums of 16, folded pairwise at distances 32 .. 1 within each group of 64 and the four groups in
 *   order; the chunks' sums combined the same way), without atomics: the same bits on every run;
 *   nothing more happens unless chromave > 0.0 (L119); wt = float(1.f / (chroma + chromave)), threshfactor = float(1.f / (SQR(thresh / 33.f)
 *   * chromave * 5.0f + chromave)), both in the reference's float / double mix, on the device;
 *   every pixel with wt < threshfactor becomes a = atot / norm, b = btot / norm, the sums of wt * a, wt * b and wt over its (2 halfwin - 1)^2
 *   window clamped to the image, row-major, float, unfused.  DEFINITION 2: EVERY WINDOW READS THE TOOL'S INPUT a AND b (the values behind
 *   setMode(LAB)).  The reference overwrites a and b while other pixels' windows read them, under schedule(dynamic,16), so its own output
 *   depends on thread timing; one thread gives a raster-order sweep in which each corrected pixel depends on the ones before it.  The SET of
 *   corrected pixels is the reference's (wt is complete before the loop), and so is every corrected pixel whose window holds no other
 *   corrected pixel.
 * from_lab != 0: the image is in LAB mode already (artgpu_impulse_denoise with to_rgb == 0 ran ahead), setMode(LAB) does nothing and `ws` is
 * not read.  to_rgb as in artgpu_impulse_denoise.  A non-NULL `info` costs the call's one host wait; without it the tool never waits for the device.
 * ARTGPU_EUNSUPPORTED, image untouched, decided before any kernel runs:
 *   - radius / scale not finite or >= 25;
 *   - halfwin > ARTGPU_DEFRINGE_MAX_HALFWIN (radius / scale > 5: at the GUI's largest radius, 5, every scale below 1; at the default
 *     radius 2, scales below 0.4), the limit of the averaging kernel's tile in LDS;
 *   - W < 2 * halfwin - 2, where the reference's first column loop (L144-151) reads past the end of the row;
 *   - more than 2^31 - 1 pixels; a hue curve whose polyline exceeds 64 KB.
 * ARTGPU_EINVAL: a bad image, NULL params or ws, to_rgb without iws, scale <= 0, a negative radius, nhuecurve < 0 or without huecurve.
 * Device scratch (context pool): four full-size planes (shared with artgpu_sharpening), 64 KB + 8 bytes per 4096 pixels. */
#define ARTGPU_DEFRINGE_MAX_HALFWIN 11
#define ARTGPU_DEFRINGE_BLUR_COPY 0
#define ARTGPU_DEFRINGE_BLUR_3X3  1
#define ARTGPU_DEFRINGE_BLUR_YVV  2
typedef struct artgpu_defringe_params {   /* DefringeParams (procparams.h:721-731; defaults procparams.cc:1835-1867: off, 2.0, 13, six points) */
    int32_t enabled;
    int32_t threshold;
    double radius;
    const double *huecurve;           /* FlatCurve control points {type, x, y, left tangent, right tangent, ...}; read during the call only */
    int32_t nhuecurve;                /* doubles in huecurve; 0: no curve */
    int32_t pad_;
} artgpu_defringe_params;
typedef struct artgpu_defringe_info {
    int32_t early_out;                /* 0 none; 1 !enabled, 2 W or H < 8 */
    int32_t halfwin;
    int32_t blur;                     /* ARTGPU_DEFRINGE_BLUR_* */
    int32_t curve;                    /* 0: no hue curve; 1: evaluated; -1: a curve FlatCurve's constructor leaves empty (getVal = 0.5) */
    double radius;                    /* params.radius / scale */
    double chromave;
    float threshfactor;               /* 0 unless chromave > 0 */
    int32_t pad_;
    int64_t corrected_pixels;         /* pixels with wt < threshfactor */
} artgpu_defringe_info;
int artgpu_defringe(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_defringe_params *params, const double *ws /* unless from_lab */,
                    const double *iws /* to_rgb only */, double scale, int from_lab, int to_rgb, artgpu_defringe_info *info /* may be NULL */);

/* Texture boost: ImProcFunctions::textureBoost (rtengine/iptextureboost.cc:183-248; the first arithmetic step of STAGE_3, improcfun.cc:606),
 * ART's detail tool.  artgpu_texture_boost_plane is one texture_boost call (L37-178) in place on a Y plane (host or device, any row stride),
 * without a mask blend:
 *   the scalars of L39-50 on the host exactly as written (pow_F in the sleef form): full_radius = detail_threshold * 3.5f, fradius =
 *   full_radius / scale, radius = max(int(fradius + 0.5f), 1), delta = radius / fradius, s, strength, strength2, isguided = full_radius >= 1;
 *   the rescale of L57-63 when fradius > 1 && delta > 1.01: the work happens on rescaleBilinear(Y) at int(W * delta + 0.5f) x
 *   int(H * delta + 0.5f) (up to 1.33x per axis) and L175-177 rescale src * 65535.f back;
 *   L85-101: v = src / 65535.f, mid = clamp(v, 1e-5f, 32.f), minval = min(v); columns below 4 * (w / 4) clamp as the reference's vector body
 *   does (vmaxf(vminf(v, hi), lo)), the others as LIM does, likewise the max of L145 / L154: a NaN pixel lands where the reference puts it;
 *   per iteration i (L114-157): mid = guidedFilter(mid, mid, mid, radius, 0.001f) when isguided, else Convolution(build_gaussian_kernel(
 *   fradius))(mid, mid); base = guidedFilter(mid, mid, ., radius * 4, 0.0001f); src = intp(2^-i, max(base + (src - mid) * strength +
 *   (mid - base) * strength2, minval), src); then src * 65535.f.
 * Convolution (rt_algo.cc:733-899) is an FFTW product in the reference.  Its index arithmetic makes it
 *   dst[y][x] = sum over ky, kx of kernel[ky][kx] * src[clamp(y + K / 2 - ky)][clamp(x + K / 2 - kx)]  (clamp to edge, K = 3, 5, 7 or 9 for
 *   a sigma below 1), and that sum is what runs here: fp32, ky-major, unfused, from 0.f, with build_gaussian_kernel (L902-939) restated on the
 *   host.  This stage is exact against that definition; the reference's own output differs from it by the FFT's rounding (the direct sum is
 *   within (K * K + 1) * 2^-24 relative of the exact convolution of positive input).
 * artgpu_texture_boost is the whole tool on an image in RGB mode: setMode(YUV) (always, also when no region runs: the YUV round trip is not
 * the identity in bits), for every region with strength != 0 in order texture_boost(Y) and Y = intp(mask, Y_new, Y) (L221-241; a NULL mask
 * does the same arithmetic with 1.f), and setMode(RGB) on top when to_rgb != 0 (the reference leaves the image in YUV mode, as
 * artgpu_hsl_equalizer's to_rgb).  The caller keeps what is host code in the reference: generateMasks' blend planes and the
 * `masks[i].enabled` test (a disabled region is simply not passed).  high_detail = (scale == 1 || pipeline == OUTPUT) (L228).
 * A non-NULL `info` receives what the last region that ran derived (zeros when none ran); filling it costs the call's one host wait.
 * Contract: NaN-free input for minval (a minimum's result depends on the order for NaN), and the sign of a zero minval is not defined.
 * ARTGPU_EUNSUPPORTED, image untouched, decided before any kernel runs:
 *   - !isguided && !high_detail (the preview's gaussianBlur at a sub-pixel sigma);
 *   - !isguided with a gaussian larger than 9 x 9 (fradius >= 1 while full_radius < 1: scale < 1);
 *   - iterations < 1;
 *   - a working plane with a side shorter than the guided filters' subsampling (w / s or h / s == 0 at radius or radius * 4, s <= 5 and
 *     s == 1 while max(w, h) <= 600): every plane with both sides >= ARTGPU_TEXTURE_BOOST_MIN_SIZE is accepted;
 *   - a box radius above 900 (detail_threshold above about 320).
 * Device scratch (context pool, artgpu_trim_scratch returns it): two planes of the working size (three on the convolution path), the
 * guided filters' statistics grid twice (two planes of w / s x h / s each), 64 K floats of partial minima; a host mask or Y plane is staged
 * in one plane more each. */
#define ARTGPU_TEXTURE_BOOST_MIN_SIZE 5
typedef struct artgpu_texture_boost_region {
    double strength;                  /* TextureBoostParams::Region::strength (procparams.h:789-793; defaults 0, 0.2, 1) */
    double detail_threshold;          /* ::detailThreshold */
    int32_t iterations;               /* ::iterations */
    const artgpu_plane *mask;         /* generateMasks' blend plane for this region (host or device); NULL = all ones; artgpu_texture_boost only */
} artgpu_texture_boost_region;
typedef struct artgpu_texture_boost_info {
    int32_t radius, isguided, rescaled;
    int32_t work_w, work_h;           /* the size the region worked at */
    int32_t kernel_size;              /* K of the gaussian; 0 when isguided */
    float minval, strength, strength2;
} artgpu_texture_boost_info;
int artgpu_texture_boost_plane(artgpu_ctx *ctx, artgpu_plane *Y, const artgpu_texture_boost_region *region, double scale, int high_detail,
                               artgpu_texture_boost_info *info /* may be NULL */);
int artgpu_texture_boost(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_texture_boost_region *regions, int nregions, const double ws[9],
                         double scale, int high_detail, int to_rgb, artgpu_texture_boost_info *info /* may be NULL */);

/* Region masks: rtengine::generateMasks (rtengine/masks.cc:1037-1516), the parametric path -- the blend planes ImProcFunctions::localContrast,
 * textureBoost, colorCorrection and guidedSmoothing multiply their regions with.  `img` is the image the tool hands over, in RGB mode
 * (Color::rgb2lab with `ws`, L617) or in LAB mode (L = g, a = r, b = b, L626-630; `ws` is not read); YUV and XYZ: ARTGPU_EUNSUPPORTED.
 * `masks` holds one entry per region (the caller passes the regions generateMasks would treat as needed; `Mask::enabled` is the tool's
 * test, as for the tools' region lists).  Lmask / abmask: n planes of the image's size each, host or device, any row stride; NULL = not
 * asked for (localContrast and textureBoost ask for Lmask only).  At least one of the two.  Per pixel and region, in the reference's order:
 *   - a curve counts as present when parametric_enabled and it is not empty, not FCT_Linear and not Mask's default (L1068-1080, defaults of
 *     procparams.cc:1014-1053 below); has_mask = some region has a curve or opacity < 100 (L1059-1084: global over the regions);
 *   - lightness-detail plane (L1113-1137), built only when Lmask is asked for and some region has a lightness curve (the reference builds it
 *     whenever Lmask is asked for and reads it under the same condition only): guide = L / 32768.f, LL = round(l * 40.f) / 40.f,
 *     guidedFilter(guide, guide, guide, int(10.f / scale), 0.01f) when that radius is > 0, guidedFilter(guide, LL, LL,
 *     int(max(max(full_w, W), max(full_h, H)) / 30.f), 0.001f);
 *   - the fused pass (L1171-1241): l /= 32768.f, a /= 42000.f, b /= 42000.f, guide = LIM01(l), c = xlin2log(sqrtf(a * a + b * b) / 327.68f *
 *     c_factor, 50.f), h = xlin2log(wrap(float(huelab_to_huehsv2(xatan2f(b, a))) + 1.f / 6.f), 3.f), blend = float(1.f * hue(h) * chroma(c) *
 *     lightness(Lmask ? intp(LIM01(lightness_detail / 100.f), LL, l) : l)) -- a double product of FlatCurve::getVal values, 1.f for an absent
 *     curve (FlatCurve(points, periodic = hue only), 1000 polygon points).  The 4-wide Color::Lab2Lch the reference's SSE2 build takes below
 *     4 * (W / 4) is the scalar one's arithmetic lane by lane (sleefsseavx.h:1168-1208 selects where sleef.h:1155-1188 branches);
 *   - without has_mask every plane is 1.f (L1296-1308); with it EVERY region, one without curves included, is blurred when blur > -10.f
 *     (blur = blur < 0 ? -1.f / blur : 1.f + blur; blur = 0 while !parametric_enabled): abmask guidedFilter(guide, ., ., r1 = max(int(4 /
 *     scale * blur + 0.5), 1), 0.001), Lmask r2 = max(int(25 / scale * blur + 0.5), 1), 0.0001; then LIM01 (L1244-1295);
 *   - contrast threshold (L1359-1376, L696-734) when parametric_enabled && contrast_threshold != 0: above 1920 px on the longer side
 *     rescaleBilinear(guide) down by s = max(W, H) / 1920.f to int(W / s) x int(H / s) and scale *= s; buildBlendMask(., ., w, h,
 *     |threshold| / 100.f * sqrt(scale), 1.f, false, max(blur, 2.0) / sqrt(scale), 32768.f); rescaleBilinear back; the planes are multiplied
 *     by it, or by 1.f - it for a negative threshold;
 *   - `area`: generate_area_mask's finished plane (the shapes' rasterisation stays with the caller), multiplied in (L1380-1393);
 *   - mask_postprocess (L737-802): posterization p = {30, 20, 10, 5, 3, 2}[LIM(posterization, 0, 6) - 1]: int(m * p + 0.5) / p; with
 *     smoothing also the threshold plane (m > 1e-4f ? 1.f : fillval), guidedFilter(guide, m, m, int(max(full_w, full_h) / (10.f * (101.f -
 *     smoothing))), 0.015f) and their product;
 *   - inverted: 1.f - m; opacity < 100: m * LIM01(opacity / 100.f).
 * full_w / full_h < 0 stand for the image's size, like the reference's (L1310-1315).  Asynchronous on the context's stream for device planes.
 * A non-NULL `info` receives n entries with what the call derived on the host (no extra wait).
 * ARTGPU_EUNSUPPORTED, decided before any kernel runs, outputs untouched:
 *   - deltae_enabled (lcms2's double-precision cmsCIE2000DeltaE), drawn_enabled, external_enabled, linked_enabled;
 *   - !curve_is_identity (Mask::curve, a DiagonalCurve evaluated per pixel); show_mask;
 *   - mode YUV or XYZ;
 *   - a guided filter whose box radius (r / subsampling) is above 900, or a statistics grid without pixels; an image with a side below
 *     ARTGPU_MASKS_MIN_SIZE (what the filters' subsampling of up to 5, buildBlendMask's frame and the gaussian need).
 * Device scratch (context pool, artgpu_trim_scratch returns it): guide, LL, the posterization's threshold plane, one blend plane per region,
 * the contrast threshold's planes (up to four), one plane per output, the guided filter's statistics grid. */
#define ARTGPU_MASKS_MIN_SIZE 8
#define ARTGPU_MASKS_MODE_RGB 0
#define ARTGPU_MASKS_MODE_LAB 1
#define ARTGPU_MASKS_MODE_YUV 2
#define ARTGPU_MASKS_MODE_XYZ 3
typedef struct artgpu_mask_params {
    int32_t parametric_enabled;       /* ParametricMask::enabled (procparams.h; defaults: false, blur 0, lightnessDetail 0, contrastThreshold 0) */
    int32_t lightness_detail;         /* ::lightnessDetail */
    const double *hue;                /* ::hue, ::chromaticity, ::lightness: FlatCurve points as artgpu_hsl_equalizer takes them; the defaults are */
    const double *chromaticity;       /*   hue {1, 0.166666667, 1, 0.35, 0.35, 0.8287775246, 1, 0.35, 0.35}, the others {1, 0, 1, 0.35, 0.35, 1, 1, 0.35, 0.35} */
    const double *lightness;
    int32_t nhue, nchromaticity, nlightness;
    int32_t contrast_threshold;       /* ::contrastThreshold */
    double blur;                      /* ::blur */
    const artgpu_plane *area;         /* generate_area_mask's plane for this region (host or device, the image's size); NULL = none */
    int32_t posterization, smoothing; /* Mask::posterization, ::smoothing (defaults 0, 0) */
    int32_t inverted, opacity;        /* Mask::inverted, ::opacity (defaults false, 100) */
    int32_t deltae_enabled, drawn_enabled, external_enabled, linked_enabled;   /* non-zero: ARTGPU_EUNSUPPORTED */
    int32_t curve_is_identity;        /* Mask::curve is the identity (its default, DCT_Linear); 0: ARTGPU_EUNSUPPORTED */
    int32_t show_mask;                /* this region is the one show_mask_idx names; non-zero: ARTGPU_EUNSUPPORTED */
} artgpu_mask_params;
typedef struct artgpu_masks_info {    /* one per region */
    int32_t has_mask;                 /* (the same in every entry) */
    int32_t has_lmask;                /* the lightness-detail plane was built (the same in every entry) */
    int32_t ll_radius_small, ll_radius;   /* its two guided-filter radii */
    int32_t blurred, r1, r2;          /* the region went through the guided blur; its radii */
    int32_t cthr_w, cthr_h;           /* the size contrast_threshold_mask worked at; 0 x 0 when it did not run */
    int32_t smoothing_radius;         /* mask_postprocess's guided-filter radius; -1 when it did not run */
} artgpu_masks_info;
int artgpu_generate_masks(artgpu_ctx *ctx, const artgpu_rgb *img, int mode, const double ws[9], const artgpu_mask_params *masks, int n,
                          int full_w, int full_h, double scale, artgpu_plane *Lmask /* n planes or NULL */, artgpu_plane *abmask /* n planes or NULL */,
                          artgpu_masks_info *info /* n entries or NULL */);

/* Colour correction: ImProcFunctions::colorCorrection (rtengine/ipcolorcorrection.cc:39-866), ART's colour-grading tool, on an image in RGB
 * mode (host or device, any row stride): setMode(YUV) (L770; always, also without regions), every region in order, setMode(RGB) when `to_rgb`
 * (the reference leaves the image in YUV mode) -- one pass over the image for up to four regions, further passes for a longer list.
 * Per region the host derives what L88-141 and L280-414 derive, in the reference's types: abca / abcb from a / b through abcoord2 and hs2uv
 * (zero in the RGB and HSL modes), rs = 1.f + in_saturation / 100.f, rsout, rhs = hueshift * RT_PI_F_180 (0 in RGB mode), rgbmode 0 (YUV,
 * JZAZBZ: channel 0's slope / offset / power / pivot / compression serve all three), 1 (RGB, HSL) or 2 (with rgbluminance), rpower = 1.0 /
 * power, compression {c * 100, log(1 + y0 * c * 100) / slope} for c > 0; in HSL mode slope / offset / power from hue / sat / factor (satcoeff
 * 2.5, pivot 1); enabled = some channel differs from the identity.  Per pixel the CDL lambda (L416-554): the hue shift (in HSL, plain yuv or
 * Jzazbz terms), then in the RGB modes in-saturation, the per-channel chain v = rgb / 65535 * slope + offset / 2, v > 0 ? pow_F(v / pivot,
 * power) * pivot : 0, xlogf(v * c0 + 1) / c1, with pow_F(., 1 / hsl_gamma) before and pow_F(., hsl_gamma) after it in HSL mode, back through
 * rgb2yuv or, with rgbluminance, Y1 = rgbLuminance(old + (new - old) * max(ws[1]) / ws[1][c]) and u, v *= Y1 / Y; in the YUV and JZAZBZ modes
 * the chain on Y with u, v *= YY / Y, yuv2jzazbz, in-saturation; in all modes u += max(Y, 0) * abcb, v += max(Y, 0) * abca, out-saturation
 * (and jzazbz2yuv); then Y = intp(lmask, Y_new, Y), u, v = intp(abmask, ., .).  Columns below 4 * (W / 4) take the reference's 4-wide CDL_v
 * (a group of four runs when any of its lanes has a blend above 0, vector sleef forms, vmaxf), the others the scalar CDL: see DESIGN.md.
 * The caller keeps `masks[i].enabled` (a disabled region is not passed) and calls artgpu_generate_masks(img in RGB mode, Lmask, abmask)
 * first, as for texture boost.  lmask / abmask: planes of the image's size, host or device; NULL = all ones; one plane may serve as both.
 * A non-NULL `info` receives nregions entries with the derived scalars, each with the call's count of pixels that took a per-pixel powf in
 * PQ / PQ_inv (a Jzazbz argument above 1: the device's powf there, everything else is the reference's bits); the count costs the call's one
 * host wait and is not taken without `info`.  Asynchronous on the context's stream for a device image without `info`.
 * ARTGPU_EUNSUPPORTED, decided before any kernel runs, image untouched: mode LUT (CLUT files); a non-finite derived scalar (power[j] == 0
 * among them); hsl_gamma <= 0 in HSL mode.  Not built: show_mask and the pipette buffers. */
#define ARTGPU_CC_YUV 0                /* ColorCorrectionParams::Mode (procparams.h:1351-1357) */
#define ARTGPU_CC_RGB 1
#define ARTGPU_CC_HSL 2
#define ARTGPU_CC_JZAZBZ 3
#define ARTGPU_CC_LUT 4
typedef struct artgpu_color_correction_region {   /* ColorCorrectionParams::Region, defaults procparams.cc:2834-2855 */
    int32_t mode;                     /* ARTGPU_CC_YUV / RGB / HSL / JZAZBZ / LUT (LUT: unsupported); default JZAZBZ */
    int32_t rgbluminance;             /* ::rgbluminance (false) */
    double a, b, in_saturation, out_saturation, hueshift, hsl_gamma;       /* 0, 0, 0, 0, 0, 2.4 */
    double slope[3], offset[3], power[3], pivot[3], compression[3];        /* 1, 0, 1, 1, 0 */
    double hue[3], sat[3], factor[3];                                      /* 0, 0, 0 */
    const artgpu_plane *lmask, *abmask;   /* generateMasks' planes; NULL = all ones */
} artgpu_color_correction_region;
typedef struct artgpu_color_correction_info {     /* one per region */
    float abca, abcb;
    int32_t enabled, rgbmode;
    float slope[3], offset[3], power[3], pivot[3];
    float compression[3][2];
    float rhs;
    int64_t oor_pixels;               /* of the whole call (the same in every entry) */
} artgpu_color_correction_info;
int artgpu_color_correction(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_color_correction_region *regions, int nregions, const double ws[9],
                            const double iws[9], int to_rgb, artgpu_color_correction_info *info /* nregions entries or NULL */);
/* ... on an image that is in YUV mode already (g = Y, b = u, r = v), where the tool's setMode(YUV) does nothing: behind artgpu_lab_to_yuv on the
 * LAB image artgpu_impulse_denoise / artgpu_defringe leave with to_rgb == 0, which is how the reference reaches colorCorrection from them. */
int artgpu_color_correction_yuv(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_color_correction_region *regions, int nregions, const double ws[9],
                                const double iws[9], int to_rgb, artgpu_color_correction_info *info /* nregions entries or NULL */);

/* ImProcFunctions::guidedSmoothing (rtengine/ipsmoothing.cc:902-1073), ART's "Smoothing" tool, modes GUIDED and NLMEANS: the last step of
 * STAGE_2, behind colorCorrection (improcfun.cc:602).  `img`: RGB mode, 0..65535, host or device, any row stride, in place.  The image is
 * normalised (x * (1.f / 65535.f), imagefloat.cc:396-432); every region in order, each reading what the previous one wrote: find_region
 * (L411-434) gives the box of mask > 0 (max exclusive); with ww * hh < (W * H) / 2 (int, strict) the region works on a copy of the box,
 * otherwise on a copy of the frame (L957-980);
 *   GUIDED  (L1039-1045, L334-409): epsilon = (float)max(0.001f * pow(2, -epsilon), 1e-6); `iterations` times, with r = max(int(round(radius
 *           / scale)), 0) and nothing when r == 0: LC three self-guided guidedFilterLog(10.f, chan, r, epsilon); L and C the guide
 *           xlin2log(max(rgbLuminance, 0), 10) for all three and the YUV recombination of L382-406 (L keeps the input's u, v; C the input's Y
 *           with bump = oY > 1e-5f ? iY / oY : 1.f), ws in double;
 *   NLMEANS (L500-562): denoise::NLMeans(., 1.f, nlstrength, nldetail, scale) `iterations` times -- L on the Y plane, then yuv2rgb(Y, u, v)
 *           with u, v of the untouched channels; LC on R, G, B; C as LC with the input's Y put back;
 * then rgb = intp(mask, working, rgb) over the box (L1050-1064), and after the last region x * 65535.f on every pixel: a pixel no region
 * touches comes out as (x * (1.f / 65535.f)) * 65535.f.  As in the reference a region whose filter does nothing (r == 0, nlstrength == 0)
 * still goes through its blend (and, NLMEANS L / C, the YUV round trip); `skipped` says why the filter did not run.
 * mask: generateMasks' Lmask plane for the region (artgpu_generate_masks on the RGB image), of the image's size, host or device; NULL = all
 * ones.  The caller keeps `masks[i].enabled` and does not pass a disabled region.  The boxes of all regions come from one device pass over
 * the mask planes and one host wait for 4 * nregions ints (neither with NULL masks only); the whole plan is made after that wait and before
 * any kernel writes the image.  A mask with no pixel above zero (undefined in the reference: an inverted box, negative sizes) skips the
 * region: nothing of it runs, skipped = ARTGPU_SMOOTHING_SKIP_EMPTY.  nregions == 0: the normalise round trip.  NaN-free input is the
 * contract.
 * ARTGPU_EUNSUPPORTED, image untouched: the modes GAUSSIAN, GAUSSIAN_GLOW, MOTION, LENS, NOISE, HALATION (Convolution is an FFTW product;
 * inpaint; NOISE regions are not taken here but by artgpu_add_noise / artgpu_film_grain below) and WAVELETS; iterations < 1; a GUIDED region (r > 0) whose statistics grid (working size /
 * subsampling) has a side below ARTGPU_SMOOTHING_MIN_SIZE, or whose box radius is above the blur kernels' 900; an NLMEANS region
 * (nlstrength != 0) with a working plane below 32 x 32, (ww + 14) * (hh + 14) >= 2^30, or scale < 1.  Not built: show_mask, the pipette
 * buffers. */
#define ARTGPU_SMOOTHING_GUIDED 0         /* SmoothingParams::Region::Mode (procparams.h:1296-1306) */
#define ARTGPU_SMOOTHING_GAUSSIAN 1
#define ARTGPU_SMOOTHING_GAUSSIAN_GLOW 2
#define ARTGPU_SMOOTHING_NLMEANS 3
#define ARTGPU_SMOOTHING_MOTION 4
#define ARTGPU_SMOOTHING_LENS 5
#define ARTGPU_SMOOTHING_NOISE 6
#define ARTGPU_SMOOTHING_HALATION 7
#define ARTGPU_SMOOTHING_WAVELETS 8
#define ARTGPU_SMOOTHING_LUMINANCE 0      /* SmoothingParams::Region::Channel (procparams.h:1291-1295) */
#define ARTGPU_SMOOTHING_CHROMINANCE 1
#define ARTGPU_SMOOTHING_RGB 2
/* the smallest side of a GUIDED region's statistics grid (working size / subsampling).  It comes from f_mean's clamp of the box radius,
 * LIM(int(r / subsampling), 0, (min(w, h) - 1) / 2 - 1) (guidedfilter.cc:160-164): a side of 5 is the first at which a radius of 1 survives
 * it, and a radius >= 1 with 2 * radius + 3 <= side is what the shared hblur / vblur_combine kernels take (their first rows and columns sum
 * radius + 1 values without looking at the size).  Below it every radius clamps to 0, no blur would run and the "filter" is the identity
 * through a log / exp round trip: refused, so that a region that small is noticed */
#define ARTGPU_SMOOTHING_MIN_SIZE 5
#define ARTGPU_SMOOTHING_SKIP_RADIUS 1    /* artgpu_smoothing_info::skipped: GUIDED with r == 0 */
#define ARTGPU_SMOOTHING_SKIP_STRENGTH 2  /* NLMEANS with nlstrength == 0 */
#define ARTGPU_SMOOTHING_SKIP_EMPTY 3     /* no mask pixel above zero */
typedef struct artgpu_smoothing_region {  /* SmoothingParams::Region, defaults procparams.cc:2753-2775 */
    int32_t mode;                     /* ARTGPU_SMOOTHING_GUIDED .. WAVELETS; default GUIDED */
    int32_t channel;                  /* ARTGPU_SMOOTHING_LUMINANCE / CHROMINANCE / RGB; default RGB */
    int32_t radius;                   /* 0 */
    int32_t epsilon;                  /* 0 */
    double sigma;                     /* 0 */
    int32_t iterations;               /* 1 */
    int32_t nldetail;                 /* 50 */
    double falloff;                   /* 1 */
    int32_t nlstrength;               /* 0 */
    int32_t numblades;                /* 9 */
    double angle, curvature, offset;  /* 0, 0, 0 */
    int32_t noise_strength;           /* 10 */
    int32_t noise_coarseness;         /* 30 */
    double halation_size;             /* 1.0 */
    double halation_color;            /* 0.0 */
    double wav_strength;              /* 0 */
    int32_t wav_levels;               /* 5 */
    int32_t pad_;
    double wav_gamma;                 /* 2.2 */
    const artgpu_plane *mask;         /* generateMasks' Lmask plane; NULL = all ones */
} artgpu_smoothing_region;
typedef struct artgpu_smoothing_info {    /* one per region: what the host derived */
    int32_t r;                        /* max(int(round(radius / scale)), 0) (GUIDED; 0 otherwise) */
    float epsilon;                    /* GUIDED; 0 otherwise */
    int32_t min_x, min_y, max_x, max_y;   /* the box the region blends over (max exclusive); the frame when not cropped; zeros when skipped for an empty mask */
    int32_t cropped;
    int32_t work_w, work_h;
    int32_t subsampling, box_radius;  /* GUIDED with r > 0: calculate_subsampling, f_mean's radius; 0 otherwise */
    int32_t skipped;                  /* 0 or ARTGPU_SMOOTHING_SKIP_* */
} artgpu_smoothing_info;
int artgpu_smoothing(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_smoothing_region *regions, int nregions, const double ws[9], double scale,
                     artgpu_smoothing_info *info /* nregions entries or NULL */);

/* ImProcFunctions::toneEqualizer (rtengine/iptoneequalizer.cc:345-371) and its tone_eq (L69-340), ART's shadows / midtones / highlights tool:
 * the last step of STAGE_1, behind exposure and hslEqualizer (improcfun.cc:580-588).  `img`: RGB mode, 0..65535, host or device, any row
 * stride or start alignment, in place.  enabled == 0 returns at once.  gain = (float)(1.f / 65535.f * pow(2.f, -pivot)); the image times
 * gain, tone_eq, the image times 1.f / gain -- the two scaled images are never stored, ((R * gain) * corr) * (1.f / gain) has the same roundings.
 *   Y = LIM(rgbLuminance(R, G, B, ws), 1e-5f, 32.f) with the double matrix;
 *   regularization > 0: guidedFilterLog(10.f, Y, radius = int(5.f / scale + 0.5f), 0.014f) when radius > 0 (self-guided, in log form);
 *   regularization > 1: Y2 = Y, Y = exp2(round(LIM(log2(max(Y, 1e-9f)), -16, 6) * 5.f) / 5.f), guidedFilter(Y2, Y, Y, r = int(350.f / scale),
 *     0.004f) and, with reg = 5 - min(regularization, 4) > 1, guidedFilter(Y2, Y, Y, r * (reg - 1), 0.004f / 100);
 *   corr: for the columns below 4 * (W / 4), in groups of four counted from column 0 of the row: vprocess_pixel (the 4-lane xlogf / xexpf)
 *     for all four when any of their Y is above 1.f, else the vector LUTf lookup at Y * 65535.f; for the W % 4 columns behind them
 *     Y > 1.f ? process_pixel(Y) : lut[Y * 65535.f] with the scalar forms (L315-339).  The table is artgpu_tone_equalizer_lut's.
 * NaN-free input is the contract.
 * ARTGPU_EUNSUPPORTED, image untouched, decided before any kernel runs: show_colormap (lcms2, PREVIEW pipeline only); regularization outside
 * 0..4; scale < 1; a regularising guided filter that would run with radius 0 (scale above 350); a box radius (r / subsampling) above the blur
 * kernels' 900; a filter whose statistics grid (size / subsampling) has a side below ARTGPU_SMOOTHING_MIN_SIZE -- the same reasoning as there:
 * below 5 every box radius clamps to 0 and the shared blur kernels take no such grid.  With regularization == 0 no filter runs and every size
 * from 1 x 1 is accepted.  (A detail filter whose radius comes out 0, scale >= 10, does not run, as in the reference.) */
typedef struct artgpu_tone_equalizer_params {   /* ToneEqualizerParams, defaults procparams.cc:2097-2104 */
    int32_t enabled;
    int32_t bands[5];          /* -100 .. 100 */
    int32_t regularization;    /* 0 .. 4, default 4 */
    int32_t show_colormap;     /* != 0: ARTGPU_EUNSUPPORTED */
    double pivot;              /* -12 .. 12 */
} artgpu_tone_equalizer_params;
typedef struct artgpu_tone_equalizer_info {     /* what the host derived */
    float gain, w_sum, factors[12];
    int32_t filters;                        /* 0 .. 3 guided filters that ran */
    int32_t radius[3], subsampling[3], box_radius[3];   /* detail, regularise 1, regularise 2; zeros when not run */
    float epsilon[3];
} artgpu_tone_equalizer_info;
int artgpu_tone_equalizer(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_tone_equalizer_params *params, const double ws[9], double scale,
                          artgpu_tone_equalizer_info *info /* or NULL */);
/* Host only, no context: gain, w_sum, factors (info; may be NULL) and the 65536-entry table lut[i] = process_pixel(i / 65535.f) (L305-310) with
 * the host's scalar sleef forms.  This is the one table the device path reads. */
int artgpu_tone_equalizer_lut(const artgpu_tone_equalizer_params *params, float *lut /* 65536, host */, artgpu_tone_equalizer_info *info);

/* ImProcFunctions::filmSimulation (rtengine/ipfilmsim.cc:33-73) with a HaldCLUT: CLUTApplication (clutstore.cc:1063-1112, 1464-1484,
 * 1502-1615) over HaldCLUT::getRGB in its SSE2 form (clutstore.cc:178-288).  In STAGE_3 between texture boost and the tone curve, or, with
 * filmSimulation.after_tone_curve, right behind the tone curve (improcfun.cc:614-620).
 *
 * A CLUT handle: `table` is the HaldCLUT as HaldCLUT::loadFile leaves it (clutstore.cc:83-96), level^3 entries with red fastest, each 3
 * (channels == 3) or 4 (channels == 4, the fourth ignored) uint16 values, on the host.  `level` is the reference's clut_level after
 * squaring (clutstore.cc:154), entries per axis: 64 for a level-8 file (512 x 512), 144 for a level-12 file (1728 x 1728).  Accepted: the
 * squares of 2 .. 16; anything else is ARTGPU_EINVAL.  The device copy (RGBX, one padding entry behind the last as in the reference, and
 * the two sRGB gamma tables beside it) is uploaded once to ctx's device and never changes; every context on that device may use the
 * handle, from any thread.  Decoding the PNG / TIFF, the file cache and the profile name in the file name (StdImageSource, CLUTStore,
 * CLUTStore::splitClutFilename) stay with the caller.  artgpu_clut_destroy releases the caller's reference; a pipe setting (below) holds
 * one of its own, so destroying a handle that is still set is safe.  NULL is accepted. */
typedef struct artgpu_clut artgpu_clut;
int artgpu_clut_create(artgpu_ctx *ctx, const uint16_t *table, int level, int channels, artgpu_clut **out);
void artgpu_clut_destroy(artgpu_clut *clut);

/* `img`: RGB mode, 0..65535, host or device, any row stride or start alignment, in place; every size from 1 x 1.  Per pixel:
 *   same_profile == 0: working -> CLUT space, Color::rgbxyz(work_to_xyz) then Color::xyz2rgb(xyz_to_clut): for the columns below
 *     4 * (W / 4), in groups of four counted from column 0 of the row, the vfloat overloads with the matrices rounded to float
 *     (L1518-1532), for the W % 4 columns behind them the scalar overloads with the double matrices (L1536-1544);
 *   Color::gamma_srgbclipped: gamma2curve[x], clipped on both sides (L1557-1559);
 *   HaldCLUT::getRGB: cell = unsigned(min(float(level - 2), x * (float(level - 1) / 65535.0f))) per channel, the position inside it
 *     x * flevel_minus_one - float(cell) (exactly 1 at 65535), seven vintpf(a, b, c) = a * b + (1 - a) * c per channel over the eight
 *     corners in the reference's order (red, green, red, green, blue), then vintpf(strength, out, gamma-encoded input);
 *   Color::igamma_srgb: igammatab_srgb[x], a table without clipping: it extrapolates past either end (L1570-1572);
 *   same_profile == 0: CLUT -> working space with clut_to_xyz and xyz_to_work, body and tail as above (L1581-1607).
 * No product is contracted into an FMA.  NaN-free input is the contract.  ARTGPU_EINVAL: a bad handle, a handle of another device, a
 * strength that is not finite. */
typedef struct artgpu_film_simulation_params {
    float strength;            /* float(params->filmSimulation.strength) / 100.f: the caller divides */
    int32_t same_profile;      /* != 0: the CLUT's profile is the working profile; the matrices are not read */
    double work_to_xyz[9];     /* ICCStore::workingSpaceMatrix(working profile), row-major (clutstore.cc:1093) */
    double xyz_to_clut[9];     /* ICCStore::workingSpaceInverseMatrix(CLUT profile) (L1096) */
    double clut_to_xyz[9];     /* ICCStore::workingSpaceMatrix(CLUT profile) (L1097) */
    double xyz_to_work[9];     /* ICCStore::workingSpaceInverseMatrix(working profile) (L1094) */
} artgpu_film_simulation_params;
int artgpu_film_simulation(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_clut *clut, const artgpu_film_simulation_params *params);
/* Host only, no context: the two 65536-entry tables the device path reads, as Color::init builds them (color.cc:239-255): gamma2curve
 * (gammatab_srgb: float(gamma2(i / 65535.0)) * 65535.f) and igammatab_srgb.  Either may be NULL. */
int artgpu_film_simulation_tables(float *gamma2curve /* 65536, host */, float *igammatab_srgb /* 65536, host */);

/* The whole hot path for one frame in one call -- what ART's batch loop does per image between load and rgb2out
 * (simpleprocess.cc stage_init L215-259, stage_denoise L311-315, stage_finish L389-396):
 *   demosaic -> getImage (crop `border`, x mul, clip) + convertColorSpace matrix -> ImProcFunctions::denoise ->
 *   [ImProcFunctions::dehaze ->] ImProcFunctions::exposure [-> ImProcFunctions::sharpening] [-> ImProcFunctions::textureBoost] ->
 *   ImProcFunctions::toneCurve [-> ImProcFunctions::localContrast].
 * raw: CFA plane (host or device).  out: (W - 2*border) x (H - 2*border) planes (host or device; the frame stays on the device
 * between the stages either way).  Disabled stages are skipped exactly like their `enabled == false` early-outs. */
typedef struct {
    int32_t sensor;                 /* 0 = Bayer, 1 = X-Trans */
    int32_t bayer_method;           /* ARTGPU_BAYER_*; what artgpu_demosaic_bayer does not support (a method off the device path, initial_gain <= 0, a
                                     * four-colour CFA, a frame under 64x64) fails the frame before any stage has run */
    uint32_t filters;
    double initial_gain;
    int32_t xtrans_passes;          /* 1 (ONE_PASS) or 3 (THREE_PASS, CIELab); what artgpu_demosaic_xtrans does not support (passes, the colour map, a
                                     * frame under 64x64, a row beyond the reference's short offsets) fails the frame before any stage has run */
    int32_t xtrans[36];
    float rgb_cam[12];
    int32_t border;                 /* raw.bayersensor.border / raw.xtranssensor.border */
    float mul[3];                   /* rm, gm, bm of getImage */
    int32_t do_clip;
    int32_t has_cam_to_work;
    double cam_to_work[9];          /* matrix branch of convertColorSpace */
    double ws[9], iws[9];           /* working space <-> XYZ (TMatrix) */
    int32_t denoise_enabled;
    artgpu_denoise_tool_params denoise;   /* what artgpu_improc_denoise does not support (color_space, chrominance_method, scale < 1, a side above 32767, and
                                     * with smoothing_enabled the limits of artgpu_denoise_guided_smoothing and artgpu_nlmeans) fails the frame before
                                     * any stage has run; so does AUTOMATIC chroma on an image under 100x100 (artgpu_denoise_compute_params) */
    int32_t exposure_enabled;
    double expcomp, black;
    int32_t tone_enabled;
    int32_t tone_mode;              /* ARTGPU_TONE_STD / ARTGPU_TONE_NEUTRAL; what artgpu_tone_curve / artgpu_tone_curve_neutral do not support (another mode,
                                     * white_point <= 0, white_point > 1 with the default curve tail, NEUTRAL without tone_lut) fails the frame before
                                     * any stage has run */
    const float *tone_lut;          /* 65536 entries (host) */
    float white_point;
    float to_out[9], to_work[9];    /* NEUTRAL only */
    double scale;
    double chrominance_auto_factor; /* DenoiseParams::chrominanceAutoFactor; 0 means 1 (only read when denoise.dn.chrominance_method is AUTOMATIC:
                                     * artgpu_denoise_compute_params then runs on the demosaiced planes, as simpleprocess.cc:254-256 does) */
    int32_t ca_enabled;             /* RAWParams::enable_ca: artgpu_raw_ca_correct ahead of the demosaic when
                                     * ca_enabled && (ca.autocorrect || |ca.red| > 0.001 || |ca.blue| > 0.001) && sensor == Bayer
                                     * (rawimagesource.cc:1827); on a device copy of `raw` (artgpu_batch_run_io: on its staged plane) */
    artgpu_ca_params ca;
    int32_t local_contrast_enabled; /* LocalContrastParams::enabled: after the tone curve (improcfun.cc:617-625 with the steps in between off) the image goes
                                     * through artgpu_rgb_to_lab(ws), artgpu_local_contrast on its L plane with these regions and `scale`, artgpu_lab_to_rgb(iws);
                                     * what artgpu_local_contrast does not support fails the frame before any stage has run.  0 = off */
    int32_t local_contrast_nregions;
    const artgpu_local_contrast_region *local_contrast_regions;   /* masks: planes of the output size */
    int32_t dehaze_enabled;         /* DehazeParams::enabled: artgpu_dehaze with `dehaze`, ws and `scale` between the denoise tool and the exposure
                                     * (simpleprocess.cc:329 before :389; the exposure then runs as its own artgpu_exposure call instead of inside the
                                     * tool's last pass, the tool's ecomp is unchanged); what artgpu_dehaze does not support fails the frame before
                                     * any stage has run.  0 = off (dehaze.enabled is not looked at) */
    artgpu_dehaze_params dehaze;
    int32_t sharpening_enabled;     /* artgpu_sharpening with `sharpening`, ws and `scale` after the exposure and before the tone curve (the first step of
                                     * STAGE_2: simpleprocess.cc:395 between :389 and :396); method, scale and an X-Trans frame with the automatic radius
                                     * fail the frame before any stage has run.  0 = off (nothing below is looked at) */
    int32_t sharpening_auto_radius; /* SharpeningParams::deconvAutoRadius: when sharpening.enabled, artgpu_deconv_auto_radius(raw as the demosaic reads it,
                                     * after CA correction; filters; 1000.f; sharpening_clip_val) replaces sharpening.deconvradius (simpleprocess.cc:274-278).
                                     * The pass is launched ahead of the demosaic; the host waits for its number where the sharpening starts.  A frame
                                     * without an eligible pair (radius NaN) fails there with ARTGPU_EUNSUPPORTED */
    float sharpening_clip_val;      /* (ri->get_white(1) - ri->get_cblack(1)) * scale_mul[1] (deconvautoradius.cc:202) */
    int32_t pad_sharpening_;
    artgpu_sharpening_params sharpening;
    int32_t texture_boost_enabled;  /* TextureBoostParams::enabled: artgpu_texture_boost with these regions, ws, `scale`, high_detail = 1 (the batch pipe is the
                                     * OUTPUT pipeline) and to_rgb = 1 after the sharpening and before the tone curve (the first arithmetic step of STAGE_3,
                                     * improcfun.cc:606); what artgpu_texture_boost does not support fails the frame before any stage has run.  0 = off */
    int32_t texture_boost_nregions;
    const artgpu_texture_boost_region *texture_boost_regions;   /* masks: planes of the output size */
} artgpu_pipeline_params;
int artgpu_pipeline_run(artgpu_ctx *ctx, const artgpu_plane *raw, const artgpu_pipeline_params *params, artgpu_rgb *out);
/* Region masks the per-frame pipe generates itself, a setting of the context like artgpu_set_curve_tail (artgpu_pipeline_params keeps its
 * layout; its last fields stay the texture-boost ones).  local_contrast_masks: nlc entries,
 * one per region of params->local_contrast_regions; texture_boost_masks: ntb entries, one per region of params->texture_boost_regions; NULL / 0
 * = that tool's regions use their own `mask` planes (or all ones), the default.  The entries, their curves and the area planes' descriptors
 * are copied (the area planes' memory stays the caller's).  While set, artgpu_pipeline_run, artgpu_batch_run and artgpu_batch_run_io generate
 * that tool's L planes with artgpu_generate_masks' code where the reference calls generateMasks -- texture boost on the RGB image ahead of
 * setMode(YUV) (iptextureboost.cc:210), local contrast on the LAB image (iplocalcontrast.cc:454) -- with the output's size as the full size and
 * params->scale, and feed them to the regions without leaving the device; the regions' own `mask` pointers are not read.  A count that differs
 * from the frame's region count is ARTGPU_EINVAL, what artgpu_generate_masks does not support ARTGPU_EUNSUPPORTED, both before any stage runs. */
int artgpu_set_pipeline_masks(artgpu_ctx *ctx, const artgpu_mask_params *local_contrast_masks, int nlc,
                              const artgpu_mask_params *texture_boost_masks, int ntb);
/* Impulse noise reduction and defringe in the per-frame pipe, a setting of the context for the same reason.  Either pointer may be NULL = that
 * tool off; both off is the default, and the pipe then launches exactly what it launched before.  The parameters (and the hue curve) are
 * copied; batch lanes inherit them.  While set, the three pipe entries run artgpu_impulse_denoise's / artgpu_defringe's code with
 * params->scale behind the sharpening and ahead of colour correction, in the reference's order (improcfun.cc:597-599).  The first of the
 * two whose gates pass does setMode(LAB), and the image stays in LAB mode until the next tool's setMode, as in the reference:
 *   colour correction next, or texture boost with no tool in between: pipe-generated masks are generated on the LAB image
 *   (ARTGPU_MASKS_MODE_LAB), then artgpu_lab_to_yuv and the tool's existing YUV input;
 *   smoothing next: its pipe-generated masks on the LAB image, then its setMode(RGB) = artgpu_lab_to_rgb;
 *   otherwise (a gradient filter, film grain, the tone curve, the end of the pipe): artgpu_lab_to_rgb at the end of STAGE_2.
 * What artgpu_defringe refuses fails the frame before any stage runs. */
int artgpu_set_pipeline_impulse_defringe(artgpu_ctx *ctx, const artgpu_impulse_denoise_params *impulse /* or NULL */,
                                         const artgpu_defringe_params *defringe /* or NULL */);
/* Colour correction in the per-frame pipe, a setting of the context for the same reason.  regions: n entries (deep-copied; batch lanes share
 * the copy); NULL / 0 = off, the default.  masks: n entries or NULL, copied as artgpu_set_pipeline_masks copies them.  While set, the three
 * pipe entries run artgpu_color_correction's code after the sharpening and before texture boost (STAGE_2, improcfun.cc:601).  With `masks`
 * both planes of every region are generated on the RGB image (ipcolorcorrection.cc:236), the output's size as the full size, params->scale,
 * and never leave the device; the regions' own lmask / abmask are then not read.  When texture boost follows, the image stays in YUV mode
 * between the two (in the reference textureBoost's setMode(YUV) is then a no-op); otherwise the tool ends with setMode(RGB).  Colour
 * correction ahead of pipe-generated texture-boost masks is ARTGPU_EUNSUPPORTED (the mask engine has no YUV mode), like everything
 * artgpu_color_correction and artgpu_generate_masks do not support: before any stage runs.  n < 0 or a NULL list with n > 0: ARTGPU_EINVAL. */
int artgpu_set_pipeline_color_correction(artgpu_ctx *ctx, const artgpu_color_correction_region *regions, int n,
                                         const artgpu_mask_params *masks /* n entries or NULL */);
/* The Smoothing tool in the per-frame pipe, a setting of the context for the same reason.  regions: n entries (deep-copied; batch lanes share
 * the copy); NULL / 0 = off, the default.  masks: n entries or NULL, copied as artgpu_set_pipeline_masks copies them.  While set, the three
 * pipe entries run artgpu_smoothing's code with params->scale after colour correction and before texture boost (the last step of STAGE_2,
 * improcfun.cc:602).  The tool works in RGB mode (its setMode(RGB), ipsmoothing.cc:937): colour correction ahead of it then ends with the
 * switch back to RGB even when texture boost follows, and texture boost does its own setMode(YUV) again; with smoothing unset the image
 * stays in YUV between those two as before.  With `masks` the Lmask planes are generated on the RGB image, the output's size as the full
 * size, params->scale, and never leave the device; the regions' own `mask` pointers are then not read.  Colour correction ahead of
 * pipe-generated smoothing masks is ARTGPU_EUNSUPPORTED (the reference generates them on the YUV image, ipsmoothing.cc:929, and the mask
 * engine has no YUV mode).  Modes, iterations, scale, what artgpu_generate_masks does not support, and the size limits of a region without a
 * mask fail the frame before any stage runs; a limit that depends on a mask's box fails at the tool, before the tool writes. */
int artgpu_set_pipeline_smoothing(artgpu_ctx *ctx, const artgpu_smoothing_region *regions, int n,
                                  const artgpu_mask_params *masks /* n entries or NULL */);
/* The tone equalizer in the per-frame pipe, a setting of the context for the same reason (copied; batch lanes inherit it).  NULL = off, the
 * default.  While set, the three pipe entries run artgpu_tone_equalizer's code with params->ws and params->scale after the exposure -- fused
 * into the denoise tool's last pass or run on its own behind dehaze -- and before the sharpening (the last step of STAGE_1, improcfun.cc:588).
 * What artgpu_tone_equalizer does not support fails the frame before any stage has run. */
int artgpu_set_pipeline_tone_equalizer(artgpu_ctx *ctx, const artgpu_tone_equalizer_params *params);
/* Film simulation in the per-frame pipe, a setting of the context for the same reason (params copied, a reference to the handle kept;
 * batch lanes inherit it).  clut == NULL = off, the default.  While set, the three pipe entries run artgpu_film_simulation's code after
 * texture boost and before the tone curve (improcfun.cc:614-616) or, with after_tone_curve != 0, right behind the tone curve (L618-620);
 * the image is in RGB mode at both points, ahead of local contrast.  A bad handle or a handle of another device fails the frame before
 * any stage has run.  With the setting off the pipe launches exactly what it launched without it. */
int artgpu_set_pipeline_film_simulation(artgpu_ctx *ctx, const artgpu_clut *clut, const artgpu_film_simulation_params *params, int after_tone_curve);

/* ImProcFunctions::filmGrain (rtengine/ipgrain.cc:33-98), ART's "Film grain" tool: the second step of STAGE_3, behind textureBoost and ahead of
 * logEncoding / filmSimulation (improcfun.cc:606-616).  `img`: RGB mode, 0..65535, host or device, any row stride or start offset, in place.
 * enabled == 0 returns at once.  The tool is guidedSmoothing (ipsmoothing.cc:933-1067) over NOISE regions it derives itself (ipgrain.cc:40-69):
 *   coarseness = int(LIM01(float(iso - 19) / 6380.f) * 100.f + 0.5f); nlevels = 3 in the OUTPUT pipeline, int(ceil(3 / scale)) otherwise;
 *   with `color` first one CHROMINANCE region (strength / 2, coarseness / 2); then LUMINANCE regions i = 0 .. nlevels - 1 with
 *   strength / (nlevels - i) and coarseness / (i + 1), all int divisions.  Their masks are default-constructed: generateMasks finds nothing
 *   that makes a mask (masks.cc:1053-1084) and fills the planes with 1.f (L1296-1308), which is what mask == NULL means here.
 * Around the regions: setMode(RGB), x * (1.f / 65535.f) (normalizeFloatTo1), per region the working area (the crop rule of artgpu_smoothing,
 * L948-980), add_noise on the working copy, rgb = intp(mask, working, rgb) over the area (L1050-1064: with an all-ones mask still
 * 1.f * w + (1.f - 1.f) * r), and x * 65535.f behind the last region.
 * add_noise (L565-695) of (strength, coarseness, channel) at `scale`:
 *   sf = LIM01(float(strength) / (L ? 200.f : 100.f)) / scale; radius = (0.5f + 1.75f * float(coarseness) / 100.f) / scale (both double
 *   quotients narrowed to float); the kernel is the sz x sz cone, sz = 2 * ceil(radius) + 1: k = d < 0 ? 1 : max(1 - d, 0) with
 *   d = float(sqrt(di^2 + dj^2)) - radius, its total summed in double, every tap divided by float(total);
 *   the generator (rng.h:31-57) is seeded 42 + int(channel) + coarseness and first fills normd[5233] through NormalDistribution (rng.h:61-90:
 *   Marsaglia's polar method, u, v, s double, xlogf of s narrowed to float, sqrtf, the spare value kept as float);
 *   per plane a, in raster order: mu = max(a, 0.f) * c, r = normd[randint(5233)] * sd, m = mu + sqrtf(mu) * r, noise = m / c - a with
 *   c = 655.35f / (20.f + powf(coarseness / 100.f, 0.5f) * 80.f) and sd = 1 for Y, 0.7 / 1 / 1.3 for R / G / B; the noise plane convolved
 *   with the kernel (replicate padding); a = max(a + sf * conv, 0.f).
 *   LUMINANCE runs on Y of rgb2yuv and keeps u, v; RGB on R, G, B; CHROMINANCE as RGB, then the input's Y under the noisy u, v.
 * Two things the reference leaves open are defined here:
 *   draw order -- the reference draws from one generator inside an OpenMP loop, a race; the single-threaded raster order is the definition:
 *     pixel (y, x) of plane p of a ww x hh working area reads draw number p * ww * hh + y * ww + x, counted from the state the table left;
 *   convolution -- rt_algo.cc:733-775 multiplies FFTs; the definition is the direct sum acc = 0.f; for i, for j: acc = acc + k[i][j] *
 *     noise[clamp(y + i - c)][clamp(x + j - c)] in fp32, unfused.
 * Every consumer of the generator reads bits 16..47 of its state, and bit k of an LCG's next state depends on bits <= k only, so the
 * stream is a 48-bit LCG (a = 25214903917, c = 11) and any draw is reached by jump-ahead: one launch per region, no noise plane.
 * `info` (or NULL): the regions that were derived, in the order they ran.
 * ARTGPU_EUNSUPPORTED, image untouched: scale < 1 (sz would exceed 7); a working area with 3 * ww * hh >= 2^32; iso outside 100 .. 6400 or
 * strength outside 0 .. 100 (rtgui/grain.cc:47,51); for artgpu_add_noise strength or coarseness outside 0 .. 100 (rtgui/smoothing.cc:348,351).
 * ARTGPU_EINVAL: bad pointers, a channel other than ARTGPU_SMOOTHING_LUMINANCE / CHROMINANCE / RGB, scale not finite.  NaN-free input is the
 * contract.  Not built: show_mask, the pipette buffers, the NAVIGATOR pipeline (where the reference adds no noise). */
#define ARTGPU_FILM_GRAIN_MAX_REGIONS 4
#define ARTGPU_GRAIN_TABLE_SIZE 5233
typedef struct artgpu_film_grain_params {   /* GrainParams, defaults procparams.cc:2731-2737 */
    int32_t enabled;           /* 0 */
    int32_t iso;               /* 400 */
    int32_t strength;          /* 50 */
    int32_t color;             /* 0 */
} artgpu_film_grain_params;
typedef struct artgpu_film_grain_region_info {     /* what filmGrain and add_noise derived for one region */
    int32_t channel, strength, coarseness, seed, sz;
    float sf;
} artgpu_film_grain_region_info;
typedef struct artgpu_film_grain_info {
    int32_t nregions;          /* 0 when the tool is disabled */
    artgpu_film_grain_region_info region[ARTGPU_FILM_GRAIN_MAX_REGIONS];
} artgpu_film_grain_info;
int artgpu_film_grain(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_film_grain_params *params, const double ws[9], double scale, int output_pipeline,
                      artgpu_film_grain_info *info /* or NULL */);
/* One NOISE region of guidedSmoothing: the working area from `mask` (the crop rule; NULL = all ones, the frame), add_noise on it, the blend.
 * first != 0: this call normalises the image (x * (1.f / 65535.f)) ahead of the region; last != 0: it stores x * 65535.f behind it.
 * artgpu_film_grain is a loop over this call with first / last set at either end; a region in between finds and leaves the image
 * normalised.  A mask with no pixel above zero skips the region (only the normalise passes asked for run). */
int artgpu_add_noise(artgpu_ctx *ctx, artgpu_rgb *img, int strength, int coarseness, int channel, const artgpu_plane *mask, const double ws[9],
                     double scale, int first, int last);
/* Host only, no context: what add_noise builds before it reads a pixel.  normd: the 5233 NormalDistribution draws of a generator seeded
 * `seed`; *state: the generator's low 48 bits after them; kernel / *sz: the normalised cone of `radius` (49 floats of room; pass NULL to skip).
 * ARTGPU_EINVAL: seed == 0 (the reference asserts), a radius that is not finite, <= 0 or gives sz > 7. */
int artgpu_grain_table(int seed, float normd[ARTGPU_GRAIN_TABLE_SIZE], float *kernel /* 49 or NULL */, int *sz, float radius, uint64_t *state);
/* Diagnostic: the table indices randint(5233) of draws first .. first + n - 1 counted from `state` (artgpu_grain_table's), computed on the
 * device by the jump-ahead the region kernel uses.  `out`: n host words.  ARTGPU_EINVAL unless first >= 0, 1 <= n <= 2^24, first + n <= 2^32 and state < 2^48. */
int artgpu_grain_indices(artgpu_ctx *ctx, uint64_t state, int64_t first, int64_t n, uint32_t *out);
/* Film grain in the per-frame pipe, a setting of the context (copied; batch lanes inherit it).  NULL = off, the default.  While set (and
 * enabled) the three pipe entries run artgpu_film_grain's code as the OUTPUT pipeline with params->ws and params->scale behind texture boost
 * and ahead of the first film simulation position (improcfun.cc:606-616); the image is in RGB mode there.  What artgpu_film_grain does not
 * support fails the frame before any stage has run.  With the setting off the pipe launches exactly what it launched without it. */
int artgpu_set_pipeline_film_grain(artgpu_ctx *ctx, const artgpu_film_grain_params *params);

/* ImProcFunctions::Lanczos (rtengine/ipresize.cc:53-223), the Resize tool's resampler: Lanczos-3 from `src` into `dst`, whose size is the
 * caller's (imw x imh of artgpu_resize_scale; as in the reference it is not derived from `scale`).  src and dst are different images,
 * each on the host or on the device, with any row stride.
 *   weights: per destination column and row, on the host with the reference's float expressions: x0 = (j + 0.5f) * delta - 0.5f with
 *     delta = 1.0f / scale, sc = min(scale, 1.0f), support = int(2.0f * 3.0f / sc) + 1, taps max(0, int(floorf(x0 - 3.0f / sc)) + 1) ..
 *     min(sW, int(floorf(x0 + 3.0f / sc)) + 1) - 1, Lanc(sc * (x0 - jj), 3.0f) with the scalar xsinf (sleef.h:993-1016), divided by their
 *     float sum.  The tables are uploaded once per (source size, destination size, scale) and kept by the context;
 *   arithmetic: the vertical pass over ascending source rows (L181-195; its 4-wide body is the same arithmetic), then the horizontal pass
 *     over ascending source columns (L198-215), acc += w * value with the product rounded before the sum.  A row or column without taps --
 *     a dst larger than scale implies -- is 0.0f.  The vertically interpolated rows live on chip; one kernel, all three planes.
 *   mode: the reference resamples the image's LAB representation (src->setMode(LAB), L56; dst->setMode(mode), L222).
 *     ARTGPU_RESIZE_PLANES  the three planes as they are: Lanczos() on an image that is already in LAB mode (or any three planes);
 *     ARTGPU_RESIZE_RGB     Lanczos() on an image in RGB mode: artgpu_rgb_to_lab(ws) on src, the resampler, artgpu_lab_to_rgb(iws) on dst.
 *                           What src holds afterwards is unspecified (the reference leaves it in LAB mode and deletes it).
 * ARTGPU_EINVAL: scale == 1 (the caller's artgpu_resize_scale returns 1 for "no resize"), not finite or <= 0; an unknown mode; RGB mode
 * without ws / iws.  ARTGPU_EUNSUPPORTED: a scale so small that the horizontal taps of eight neighbouring destination columns do not lie
 * within 256 source columns (about scale < 1/17; every 1/16 <= scale is supported, upscales of any factor).  Neither writes dst. */
#define ARTGPU_RESIZE_PLANES 0
#define ARTGPU_RESIZE_RGB    1
int artgpu_resize_lanczos(artgpu_ctx *ctx, artgpu_rgb *src, artgpu_rgb *dst, float scale, int mode,
                          const double ws[9], const double iws[9] /* RGB mode only */);
/* ResizeParams as ImProcFunctions::resizeScale reads them (ipresize.cc:226-297).  The pipe has no crop, so the crop branches of resizeScale
 * (crop.enabled with appliesTo "Cropped area" / "Full image") are not restated: the values apply to the full image. */
typedef struct artgpu_resize_params {
    int32_t enabled;
    int32_t dataspec;          /* 0 scale, 1 width, 2 height, 3 fit box */
    double scale;
    int32_t width, height;     /* ResizeParams::get_width() / get_height(): pixels */
    int32_t allow_upscaling;
} artgpu_resize_params;
/* Host only, no context: ImProcFunctions::resizeScale(params, fw, fh, imw, imh).  *scale is what it returns: 1.0f with *imw = fw, *imh = fh
 * for a NULL or disabled tool and for |dScale - 1| <= 1e-5; otherwise float(dScale) with *imw = int(fw * dScale + 0.5), likewise *imh. */
int artgpu_resize_scale(const artgpu_resize_params *params, int fw, int fh, int *imw, int *imh, float *scale);
/* The Resize tool in the per-frame pipe, a setting of the context for the same reason (copied; batch lanes inherit it).  NULL = off, the
 * default.  While set, the three pipe entries call artgpu_resize_scale on the frame's size behind the border, and where the reference
 * resizes (simpleprocess.cc:406-407: scale < 1, or scale > 1 with allow_upscaling or dataspec 0) the output is imw x imh: artgpu_pipeline_run
 * and artgpu_batch_run take `out` of that size, artgpu_batch_run_io writes imh rows of imw pixels.  Every stage in front sees the full size
 * (the working image then lives in the context's scratch); ImProcFunctions::resize follows STAGE_3.  With local contrast on, the image is
 * still in LAB mode there (iplocalcontrast.cc:441), so the LAB planes are resampled as they are and the switch to RGB happens on the small
 * image; otherwise it is the ARTGPU_RESIZE_RGB path.  Where the reference does not resize, the frame goes through at full size with the same
 * bits as with the setting off.  An unsupported scale, a result smaller than one pixel or an `out` of another size fail the frame before any
 * stage has run.  With the setting off the pipe allocates and launches exactly what it did without it. */
int artgpu_set_pipeline_resize(artgpu_ctx *ctx, const artgpu_resize_params *params);

/* ImProcFunctions::creativeGradients (rtengine/iptransform.cc:1390-1408): the graduated filter and the vignette filter, i.e.
 * transformLuminanceOnly(img, img, ..., creative = true) (L987-1048), in place on an image in RGB mode.  One kernel, one pixel per lane,
 * 12 bytes in and 12 bytes out per pixel, no scratch plane.
 *   what runs: needsGradient / needsPCVignetting (L1354-1362): enabled and fabs(strength) > 1e-15.  With neither, ARTGPU_OK without a launch;
 *   geometry: the pixel (x, y) of the image is (offset_x + x, offset_y + y) of a picture of cw x ch = full_width x full_height (the image's
 *     own size when full_width < 0, L1397-1403), and fw = int(cw * scale), fh = int(ch * scale) is what the crop's numbers refer to;
 *   derived parameters: calcGradientParams (L677-758) and calcPCVignetteParams (L828-895) run once per call on the host, statement by
 *     statement in the reference's double / float mixture, with the host's libm (fmod, cos, tan, pow, powf) as in the reference.
 *     artgpu_creative_gradient_params (host only, no context) hands the result out; the kernel takes that struct by value;
 *   per pixel: calcGradientFactor (L761-812) and calcPCVignetteFactor (L898-983) with normn / pow3 / pow4 (L36-89) and sleef's scalar xsinf /
 *     xcosf / xcbrtf.  Each returns a float; `factor` is the double 1.0 times each of them, and a channel is float(double(pixel) * factor).
 *     With one tool on that equals the float product (the double product of two floats is exact), with both on the channel product is
 *     rounded twice; the kernel has one form for each.  Only normn's cases 2, 4, 6 and 8 can occur (sep = int(sepf) & ~1 with sepf in 2 .. 6).
 * ARTGPU_EINVAL: bad pointers, values that are not finite, full_width >= 0 with full_height < 1, scale <= 0.  ARTGPU_EUNSUPPORTED, image
 * untouched: a roundness outside 0 .. 100 (sep would leave 2 .. 6), a feather outside 0 .. 100, a negative offset, and a size, offset + size or
 * crop beyond 32767 (the reference squares distances and sizes in int).  Not built: the lens-correction vignetting
 * branch of transformLuminanceOnly (creative = false). */
typedef struct artgpu_creative_gradients_params {
    int32_t gradient_enabled;                  /* GradientParams, defaults procparams.cc: false, 0, 25, 0.60, 0, 0 */
    double gradient_degree;
    int32_t gradient_feather;
    double gradient_strength;
    int32_t gradient_center_x, gradient_center_y;
    int32_t pcvignette_enabled;                /* PCVignetteParams: false, 0.60, 50, 50, 0, 0 */
    double pcvignette_strength;
    int32_t pcvignette_feather, pcvignette_roundness, pcvignette_center_x, pcvignette_center_y;
    int32_t crop_enabled, crop_x, crop_y, crop_w, crop_h;      /* CropParams: only the vignette filter reads them */
    int32_t offset_x, offset_y, full_width, full_height;       /* ImProcFunctions::offset_x .. full_height: 0, 0, -1, -1 */
    double scale;                              /* ImProcFunctions::scale: 1 */
} artgpu_creative_gradients_params;
typedef struct artgpu_creative_gradient_derived {   /* grad_params and pcv_params (iptransform.cc:668-675, 815-825), bools as int32 */
    int32_t apply_gradient, apply_pcvignette;
    int32_t cx, cy;                            /* offset_x, offset_y */
    int32_t angle_is_zero, transpose, bright_top, h;
    float ta, yc, xc, ys, ys_inv, scale, botmul, topmul, top_edge_0;
    float oe_a, oe_b, oe1_a, oe1_b, oe2_a, oe2_b, ie_mul, ie1_mul, ie2_mul, sepmix, feather;
    int32_t x1, x2, y1, y2, ex, ey, ew, eh, sep, is_super_ellipse_mode, is_portrait;
    float pcv_scale, fadeout_mul;
} artgpu_creative_gradient_derived;
int artgpu_creative_gradients(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_creative_gradients_params *params);
/* w x h: the image's size (what full_width < 0 stands for).  Fields of a tool that does not run are zero. */
int artgpu_creative_gradient_params(const artgpu_creative_gradients_params *params, int w, int h, artgpu_creative_gradient_derived *out);
/* The two filters in the per-frame pipe, a setting of the context (copied; batch lanes inherit it).  NULL = off, the default.  While set the
 * three pipe entries run artgpu_creative_gradients' code as the first step of STAGE_3, ahead of texture boost and its masks
 * (improcfun.cc:605), with offset 0, the frame's size behind the border as the full size and scale 1, whatever the struct holds there.
 * The step starts with setMode(RGB): behind colour correction (which leaves YUV) that is the switch colour correction ends with, and texture
 * boost then finds RGB.  What the call refuses fails the frame before any stage has run.  With the setting off, or with neither filter
 * running, the pipe launches exactly what it launched without it. */
int artgpu_set_pipeline_creative_gradients(artgpu_ctx *ctx, const artgpu_creative_gradients_params *params);

/* ImProcFunctions::softLight (rtengine/ipsoftlight.cc:31-82) in place on an image in RGB mode: one table, applied to the three channels.
 *   table: artgpu_soft_light_lut builds it on the host (no context) as the reference does per call: for i in 0 .. 65535
 *     v = Color::gamma_srgb(float(i)) / 65535.f; v2 = v * v; v22 = v2 * 2.f; v = v2 + v22 - v22 * v (Pegtop's formula);
 *     lut[i] = intp(strength / 100.f, Color::igamma_srgb(v * 65535.f), float(i)) with rt_math.h's intp, a * b + (1 - a) * c.  The two colour
 *     functions are float-indexed LUTf lookups in tables that do not clip (color.cc:183-185), restated on the host.  The context keeps the
 *     table of the last strength on the device;
 *   pixels: x <= 65535.f takes LUTf::operator[](float) with both clip flags (a value below 0 takes entry 0); a value above 65535 and a NaN,
 *     which fails the comparison, stay as they are.  The kernel is the tone curve's (the same table shape) with that rule switched on,
 *     and takes the same LUT-in-LDS shape on large frames.
 * Not enabled or strength <= 0: ARTGPU_OK without a launch, as the reference returns.  ARTGPU_EUNSUPPORTED: strength above 100 (the GUI's
 * range, rtgui/softlight.cc).  ARTGPU_EINVAL: bad pointers. */
typedef struct artgpu_soft_light_params {   /* SoftLightParams, defaults procparams.cc:2675-2679 */
    int32_t enabled;           /* 0 */
    int32_t strength;          /* 30 */
} artgpu_soft_light_params;
int artgpu_soft_light(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_soft_light_params *params);
int artgpu_soft_light_lut(int strength, float lut[65536]);
/* Soft light in the per-frame pipe, a setting of the context (copied; batch lanes inherit it).  NULL = off, the default.  While set (and
 * enabled with strength > 0) the three pipe entries run artgpu_soft_light's code behind the tone curve and the second film simulation
 * position, ahead of local contrast (improcfun.cc:623); the image is in RGB mode there.  What artgpu_soft_light refuses fails the frame
 * before any stage has run.  With the setting off the pipe launches exactly what it launched without it. */
int artgpu_set_pipeline_soft_light(artgpu_ctx *ctx, const artgpu_soft_light_params *params);

/* ImProcFunctions::blackAndWhite (rtengine/ipbw.cc:214-365) in place on an image in RGB mode.
 *   mixer: computeBWMixerConstants (L50-211) runs on the host exactly as written, from float(mixer_red / _green / _blue), the setting and the
 *     filter, with kcorec starting at 1.  L192-194 are part of the definition: each of the three statements reads the mixer values the
 *     statement before it has already overwritten.  artgpu_bw_mixer_constants (host only, no context) hands the result out;
 *   gamma: gamma = 1.f - float(g) / (g < 0 ? 100.f : 125.f) per channel; if any is not 1, three tables pow_F(float(i) / 65535.f, gamma) *
 *     65535.f (sleef's scalar pow_F restated on the host) and a lookup per channel in front of the mix;
 *   pixels: columns below W & ~3 are the reference's 4-wide body (LUTf::operator[](vfloat), LUT.h:349-377), the remaining columns its scalar
 *     tail (operator[](float), L436-459); (bwr * r + bwg * g + bwb * b) * kcorec in float, left to right, written to all three channels;
 *   colour cast (cast_bottom > 0): ulut / vlut, 65536 floats each, come from the caller as tone, RGB and Lab curves do, because filling
 *     them takes DiagonalCurve's spline, which is host code of the application.  ART fills them like this (L319-341): s = pow_F(bottom /
 *     100.f, 3.f), h = top / 180.f * pi; for i: x = Color::gamma_srgbclipped(i) / 65535.f, y = DiagonalCurve(curves::filmcurve_def)
 *     .getVal(x) * 65535.f, c = FlatCurve{FCT_MinMaxCPoints, 0, 0, 0.35, 0, 0.5, 1, 0.35, 0.35, 1, 0, 0, 0.35}.getVal(x), hsl2yuv(h, s * c, u, v),
 *     ulut[i] = y * u, vlut[i] = y * v.  Behind the mix, in registers: setMode(YUV) with row 1 of `ws` as floats, u += ulut[Y], v += vlut[Y]
 *     with the same body / tail rule.  The reference leaves the image in YUV mode; the stand-alone call hands back RGB (Color::yuv2rgb), as
 *     artgpu_texture_boost and artgpu_color_correction do.  cast_top is not read by the device path (it only shapes the caller's tables).
 * Not enabled: ARTGPU_OK without a launch.  ARTGPU_EINVAL: bad pointers, a setting or filter outside the enums, a cast without ulut / vlut
 * or without ws.  ARTGPU_EUNSUPPORTED: a gamma outside -100 .. 100 or a mixer value outside -100 .. 200 (the GUI's ranges). */
enum {   /* BlackWhiteParams::setting */
    ARTGPU_BW_NORMAL_CONTRAST = 0, ARTGPU_BW_PANCHROMATIC, ARTGPU_BW_HYPER_PANCHROMATIC, ARTGPU_BW_LOW_SENSITIVITY, ARTGPU_BW_HIGH_SENSITIVITY,
    ARTGPU_BW_ORTHOCHROMATIC, ARTGPU_BW_HIGH_CONTRAST, ARTGPU_BW_LUMINANCE, ARTGPU_BW_LANDSCAPE, ARTGPU_BW_PORTRAIT, ARTGPU_BW_INFRARED,
    ARTGPU_BW_RGB_REL, ARTGPU_BW_RGB_ABS, ARTGPU_BW_ROYGCBPM_REL, ARTGPU_BW_ROYGCBPM_ABS, ARTGPU_BW_SETTING_COUNT
};
enum {   /* BlackWhiteParams::filter */
    ARTGPU_BW_FILTER_NONE = 0, ARTGPU_BW_FILTER_RED, ARTGPU_BW_FILTER_ORANGE, ARTGPU_BW_FILTER_YELLOW, ARTGPU_BW_FILTER_YELLOW_GREEN,
    ARTGPU_BW_FILTER_GREEN, ARTGPU_BW_FILTER_CYAN, ARTGPU_BW_FILTER_BLUE, ARTGPU_BW_FILTER_PURPLE, ARTGPU_BW_FILTER_COUNT
};
typedef struct artgpu_black_and_white_params {   /* BlackWhiteParams, defaults procparams.cc:2470-2482 */
    int32_t enabled;           /* 0 */
    int32_t setting;           /* ARTGPU_BW_RGB_REL */
    int32_t filter;            /* ARTGPU_BW_FILTER_NONE */
    int32_t mixer_red, mixer_green, mixer_blue;   /* 33, 33, 33 */
    int32_t gamma_red, gamma_green, gamma_blue;   /* 0, 0, 0 */
    int32_t cast_bottom, cast_top;                /* colorCast.getBottom() / getTop(): 0, 0 */
    const float *ulut, *vlut;  /* the cast's tables, 65536 floats each (host; the call keeps its own copy); NULL without a cast */
} artgpu_black_and_white_params;
typedef struct artgpu_bw_mixer {   /* computeBWMixerConstants' results */
    float bwr, bwg, bwb, kcorec, filcor;
    double rrm, ggm, bbm;
} artgpu_bw_mixer;
int artgpu_black_and_white(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_black_and_white_params *params, const double ws[9] /* the cast only */);
int artgpu_bw_mixer_constants(int setting, int filter, int mixer_red, int mixer_green, int mixer_blue, artgpu_bw_mixer *out);
/* Black-and-white in the per-frame pipe, a setting of the context (parameters and tables copied; batch lanes inherit it).  NULL = off, the
 * default.  While set (and enabled) the three pipe entries run artgpu_black_and_white's code behind local contrast (improcfun.cc:627).  The
 * tool needs RGB, so with it on the image goes back from LAB to RGB behind local contrast even when the Resize tool follows, and the
 * resampler then takes its ARTGPU_RESIZE_RGB path; with a cast the image is in YUV mode behind the tool and is switched to RGB as the
 * reference's next setMode(RGB) would (rgb2out's); a cast together with the Resize tool is ARTGPU_EUNSUPPORTED, because Lanczos' setMode(LAB)
 * then starts from YUV (Imagefloat::yuv_to_lab), which the device path has not.  What artgpu_black_and_white refuses fails the frame before
 * any stage has run.  With the setting off the pipe launches exactly what it launched without it. */
int artgpu_set_pipeline_black_and_white(artgpu_ctx *ctx, const artgpu_black_and_white_params *params);

/* This rank's share of a batch: frames are independent (batchProcessingThread handles them one after another,
 * simpleprocess.cc:586-612), so a multi-GPU batch is one context per GPU each running its own frames; the completion
 * barrier / gather lives in the host driver (bench.py, art_amd/batch.py), not in the data path. */
int artgpu_batch_run(artgpu_ctx *ctx, int nframes, const artgpu_plane *raws, const artgpu_pipeline_params *params, artgpu_rgb *outs);
/* Frames in flight per GPU for artgpu_batch_run (default 1 = one after another on the context's stream).  With lanes > 1 the
 * context keeps lanes-1 sibling contexts (own stream, work arenas and host thread); frame f runs on lane f % lanes, the results are
 * the same bits.  On return the secondary lanes have completed; lane 0 stays ordered on the context's stream as before. */
int artgpu_set_batch_lanes(artgpu_ctx *ctx, int lanes);

/* A batch whose frames arrive as the decoder delivers them and leave as the writers take them -- the data formats either side of the
 * path, so that 2 + 6 (or 2 + 3) bytes per pixel cross PCIe instead of 4 + 12:
 *   in : uint16 (or float) sensor data + the black levels / multipliers of RawImageSource::scaleColors (rawimagesource.cc:2677-2859,
 *        artgpu_scale_colors); the frame's channel maxima come back in `chmax`;
 *   out: ARTOutputProfile's matrix + TRC fast path of ImProcFunctions::rgb2out (iprgb2out.cc:94-172,452-461, artgpu_rgb2out_matrix;
 *        rgb2out_enabled = 0: the working-space image as it is) followed by Imagefloat::getScanline for every row
 *        (imagefloat.cc:125-170, artgpu_get_scanlines: (bps, is_float) = (8,0), (16,0), (16,1), (32,1)).
 * Between the two: artgpu_pipeline_run's stages with `params` (params->border trims the scanlines like getImage does).
 * The call is built for host buffers: every lane (artgpu_set_batch_lanes) keeps a frame's upload, its kernels and its download on three
 * streams with two staging slots each, so the upload of frame f + 1 and the download of frame f - 1 run beside the kernels of frame f and
 * the host thread never waits for a copy before the batch ends.  Pinned host memory (hipHostMalloc / hipHostRegister) is what makes the
 * copies asynchronous; pageable memory works and is staged by the runtime, one blocking copy at a time.  Device pointers (on_device != 0)
 * skip the corresponding copy; frames of different residency may share a batch.  Same bits as artgpu_scale_colors -> artgpu_pipeline_run ->
 * artgpu_rgb2out_matrix -> artgpu_get_scanlines.
 * `status` of a frame, when the call returns -- WHATEVER it returns:
 *   ARTGPU_OK            the frame's scanlines are complete and its `chmax` is valid;
 *   ARTGPU_EUNSUPPORTED  with valid `chmax`: rgb2out met values above 1 with a non-linear TRC (artgpu_rgb2out_matrix's rule; the scanlines
 *                        are complete for every other pixel);
 *   any code, `chmax` 0  the frame was not run, or its lane cannot vouch for it.  A lane (frames k, k + lanes, ...) stops at the first of
 *                        its frames that is refused (arguments, something the path does not support, memory): that frame and the lane's
 *                        later ones carry the code and their buffers are not written, the frames before it run to their end and
 *                        report as usual.  After a HIP error or a kernel that gave up a bounded wait on the lane, every frame of the
 *                        lane carries the code.  Other lanes are not affected.
 * The call returns non-zero if any frame's status is: a lane's own error before a frame's rgb2out report, the lowest lane first.  So: look
 * at the return code to learn that something went wrong, at `status` to learn which frames can be written. */
typedef struct {
    const void *data;               /* sensor values, row-major */
    int32_t w, h;
    int64_t row_stride_bytes;
    int32_t is_u16;                 /* 1: uint16_t, 0: float */
    int32_t on_device;
    float cblacksom[4], scale_mul[4];
} artgpu_sensor_frame;
typedef struct {
    void *scanlines;                /* (h - 2 border) rows of (w - 2 border) interleaved RGB pixels */
    int64_t row_stride_bytes;
    int32_t bps, is_float;
    int32_t on_device;
    int32_t rgb2out_enabled;
    float out_matrix[9];
    int32_t trc_linear;
    const float *trc_lut;           /* host, trc_lutsz entries (NULL with trc_linear) */
    int32_t trc_lutsz;
    float chmax[4];                 /* out: scaleColors' channel maxima (chmax[3] = chmax[1]) */
    int32_t status;                 /* out: ARTGPU_OK = scanlines complete and chmax valid, whatever the call returned (the contract above) */
} artgpu_scanline_frame;
int artgpu_batch_run_io(artgpu_ctx *ctx, int nframes, const artgpu_sensor_frame *in, const artgpu_pipeline_params *params,
                        artgpu_scanline_frame *out);

/* The completion step of a multi-GPU batch -- the only collective of the path (frames are independent; the reference's loop
 * simply finishes, simpleprocess.cc:591-611): every rank contributes one 64-byte record (by convention of art_amd/batch.py: rank,
 * frames done, status, checksum of the outputs, elapsed microseconds, 3 spare words) and receives all of them, rank-major, in
 * `all_records` (host memory, nranks * 8 words).  `rccl_comm` is the caller's ncclComm_t (RCCL) whose ranks each hold one
 * artgpu context on their own GPU; the all-gather runs on the context's stream after the frames queued there, and doubles as
 * the batch barrier.  NULL with nranks == 1 copies the record.  RCCL is loaded at run time (no link-time dependency). */
#define ARTGPU_BATCH_RECORD_WORDS 8
int artgpu_batch_complete(artgpu_ctx *ctx, void *rccl_comm, int nranks, const int64_t record[ARTGPU_BATCH_RECORD_WORDS], int64_t *all_records);

/* Bytes of device scratch the context currently holds (arena + staging + the denoise pool: for a 45 MP frame through
 * artgpu_improc_denoise about 5.0 GB -- two L band sets, the chroma band sets of both channels, the DCT block buffer; the hand-over ring of the
 * fused shrink pass is 24 MB -- per context and per batch lane; grown on demand, kept between frames, artgpu_trim_scratch gives it back). */
size_t artgpu_scratch_bytes(const artgpu_ctx *ctx);

/* Gives the context's device scratch back to the driver (work arenas, staging planes, the denoise pool, of the context and of its batch
 * lanes): waits for the context's queued work first, keeps settings, curves and streams; the next call grows what it needs again and rebuilds
 * the tables that lived in the pool.  The reference frees its scratch when each tool returns (FTblockDN.cc:2655-2689, amaze_demosaic_RT.cc:1583);
 * the device path keeps it between frames because allocation is what a steady-state batch must not pay for -- this is the call for the moment
 * a batch is over, a much smaller frame size follows, or several contexts / ranks have to share one GPU's memory. */
int artgpu_trim_scratch(artgpu_ctx *ctx);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* ARTGPU_H */
