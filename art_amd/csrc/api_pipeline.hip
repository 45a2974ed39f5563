// art_amd/csrc/api_pipeline.hip -- one frame through the whole path: the plan, the five stages, and the settings of the context the pipe
// reads (artgpu_set_pipeline_*).  What it may take from a stage is what api_internal.h declares.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

// ---------------------------------------------------------------------------------------------
// the pipe's settings: deep copies owned by the context
// ---------------------------------------------------------------------------------------------

namespace {

// a deep copy of n mask entries (their curves and the area planes' descriptors) for a setting of the context
const artgpu_mask_params *own_pipe_masks(artgpu_ctx::PipeMasks &o, const artgpu_mask_params *src, int n)
{
    o.m.assign(src, src + n);
    o.curves.assign((size_t)3 * n, std::vector<double>());
    o.areas.assign(n, artgpu_plane{});
    for (int i = 0; i < n; ++i) {
        artgpu_mask_params &m = o.m[i];
        const double **pts[3] = {&m.hue, &m.chromaticity, &m.lightness};
        int32_t *cnt[3] = {&m.nhue, &m.nchromaticity, &m.nlightness};
        for (int k = 0; k < 3; ++k) {
            if (*cnt[k] < 0) *cnt[k] = 0;
            if (*pts[k] && *cnt[k] > 0) o.curves[3 * i + k].assign(*pts[k], *pts[k] + *cnt[k]);
            *pts[k] = o.curves[3 * i + k].empty() ? nullptr : o.curves[3 * i + k].data();
            if (!*pts[k]) *cnt[k] = 0;
        }
        if (m.area) { o.areas[i] = *m.area; m.area = &o.areas[i]; }
    }
    return n > 0 ? o.m.data() : nullptr;
}

// what artgpu_set_pipeline_color_correction and artgpu_set_pipeline_smoothing share: the regions are copied, the descriptors of their mask
// planes (the members `fields` names) too -- the planes' memory stays the caller's --, the mask entries are owned or reset, and the pipe's
// view of the setting (regions, entries, count) is written
template <typename Region>
void own_pipe_regions(artgpu_ctx::PipeRegions<Region> &o, const Region *regions, int n, std::initializer_list<const artgpu_plane *Region::*> fields,
                      const artgpu_mask_params *masks, const Region **regs, const artgpu_mask_params **entries, int *count)
{
    o.regs.assign(regions, regions + n);
    o.planes.assign(fields.size() * n, artgpu_plane{});
    artgpu_plane *next = o.planes.data();
    for (Region &r : o.regs)
        for (const auto f : fields) {
            if (r.*f) { *next = *(r.*f); r.*f = next; }
            ++next;
        }
    *entries = masks ? own_pipe_masks(o.masks, masks, n) : nullptr;
    if (!masks) o.masks = artgpu_ctx::PipeMasks{};
    *regs = n > 0 ? o.regs.data() : nullptr;
    *count = n;
}

} // namespace

// ---------------------------------------------------------------------------------------------
// one frame / one batch share through the whole path
// ---------------------------------------------------------------------------------------------

namespace artgpu { namespace api {

// the call site's condition (rawimagesource.cc:1827): CA correction enabled, auto or a manual shift, Bayer only (X-Trans skips it)
bool pipeline_ca(const artgpu_pipeline_params *p)
{
    return p->ca_enabled && (p->ca.autocorrect || fabs(p->ca.red) > 0.001 || fabs(p->ca.blue) > 0.001) && p->sensor == 0;
}
// what the CA correction of a frame refuses (cfa: the pattern as ca_correct_dev takes it)
static int pipeline_ca_check(artgpu_ctx *ctx, int W, int H, const artgpu_pipeline_params *p, unsigned *cfa)
{
    if (!ca_cfa(p->filters, cfa)) return fail(ctx, ARTGPU_EUNSUPPORTED, "pipeline: CA correction on RGB Bayer patterns only (filters 0x%08x)", p->filters);
    if (W < 64 || H < 64) return fail(ctx, ARTGPU_EUNSUPPORTED, "pipeline: CA correction on a frame smaller than 64x64");
    return ARTGPU_OK;
}
// CA correction of the CFA plane `raw` (device, rows of `stride` floats) in place, ahead of the demosaic
int pipeline_ca_dev(artgpu_ctx *ctx, float *raw, size_t stride, int W, int H, const artgpu_pipeline_params *p)
{
    unsigned cfa;
    const int rc = pipeline_ca_check(ctx, W, H, p, &cfa);
    return rc ? rc : ca_correct_dev(ctx, raw, stride, W, H, cfa, &p->ca, nullptr);
}

} } // namespace artgpu::api

namespace {

enum PipeMode { PIPE_RGB, PIPE_YUV, PIPE_LAB };
// Everything a frame decides before its first launch (pipeline_plan).  The stages only read it, but for the `mask` pointers of lc_regs / tb_regs,
// which pipe_stage3 aims at the planes it generates.
struct PipePlan {
    int W, H, b, w, h;             // the raw frame, its border, the image behind the demosaic (W - 2b x H - 2b)
    double scale;
    bool lc_on, lc_gen, tb_on, tb_gen, cc_on, cc_gen, sm_on, sm_gen;   // the local tools: on, and the pipe generates their masks (artgpu_set_pipeline_*)
    bool cc_to_rgb, tb_in_yuv;     // the mode walk: colour correction ends with the switch back to RGB; texture boost finds the image in YUV mode
    bool imp_on, df_on, id_lab;    // impulse noise reduction / defringe run (artgpu_set_pipeline_impulse_defringe, the gates passed); either leaves LAB mode
    bool sm_from_lab, tb_from_lab, lab_to_rgb_end;   // ... which smoothing / texture boost find (masks on the LAB image, then their switch), or STAGE_2 ends with the switch to RGB
    ImpPlan imp;
    DfPlan df;
    std::vector<artgpu_local_contrast_region> lc_regs;             // copies of the regions whose masks the pipe generates ...
    std::vector<artgpu_texture_boost_region> tb_regs;
    const artgpu_local_contrast_region *lc_regions;                // ... or the caller's
    const artgpu_texture_boost_region *tb_regions;
    MkPlan lc_mk, tb_mk, cc_mk, sm_mk;
    CcPlan cc;
    DehazePlan dehaze;
    bool te_on;                                                    // the tone equalizer (artgpu_set_pipeline_tone_equalizer, enabled)
    artgpu_tone_equalizer_info te;
    bool fs_on;                                                    // film simulation (artgpu_set_pipeline_film_simulation)
    FgPlan fg;                                                     // film grain (artgpu_set_pipeline_film_grain): the derived regions, none when off
    CgDerived cg;                                                  // the graduated / vignette filters (artgpu_set_pipeline_creative_gradients): both apply_* 0 when off
    SlPlan sl;                                                     // soft light (artgpu_set_pipeline_soft_light), black-and-white (artgpu_set_pipeline_black_and_white):
    BwPlan bw;                                                     // `on` is 0 when off
    bool rs_on;                                                    // the Resize tool (artgpu_set_pipeline_resize) changes this frame's size: to imw x imh
    int imw, imh;
    float rs_scale;
    bool sh_on, sh_auto, sh_radius_pending;
    artgpu_sharpening_params shpar;                                // (deconvradius: 0.75 stands in while the automatic radius is pending)
    SharpenPlan sharpen;
    std::vector<TbPlan> tb;
};
// What the stages hand on: the CFA plane the demosaic reads (the caller's, or its CA-corrected copy in the pool), the demosaiced W x H planes in the
// pool, the w x h image the later stages work on (the caller's planes if they are on the device, else a staged copy; with the Resize tool: planes of
// the pool, and `small` is the caller's imw x imh image the resampler writes)
struct PipeFrame { artgpu_plane raw; DevRGB dem; DevRGB d; DevRGB small; };

// the MkPlan of n regions whose masks the pipe generates on its own image (mode: ARTGPU_MASKS_MODE_LAB or _RGB; full size, no crop)
static int pipe_plan_masks(artgpu_ctx *ctx, const artgpu_pipeline_params *p, const PipePlan &pl, int mode, const artgpu_mask_params *masks, int n, bool want_ab, const char *who, MkPlan *mk)
{
    return mk_plan(ctx, pl.w, pl.h, mode, mode == ARTGPU_MASKS_MODE_LAB ? nullptr : p->ws, masks, n, pl.w, pl.h, pl.scale, true, want_ab, who, mk, nullptr);
}

// generateMasks(rgb, ., masks, 0, 0, full size, scale, ., -1, &Lmask, [&abmask]) on the device image: the planes go to pool slot `slot` and never
// leave the device.  *planes: their descriptors, n L planes, then n ab planes when asked for
static int pipe_gen_masks(artgpu_ctx *ctx, const artgpu_pipeline_params *p, const DevRGB &d, int slot, const artgpu_mask_params *masks, const MkPlan &mk, int n, bool want_ab,
                          std::vector<artgpu_plane> *planes)
{
    const size_t np = (size_t)d.w * d.h, count = (size_t)n * (want_ab ? 2 : 1);
    float *mo;
    int rc;
    if ((rc = pool_get(ctx, slot, count * np * 4, &mo)) || (rc = masks_dev(ctx, d.p, d.stride, p->ws, masks, mk, mo, want_ab ? mo + n * np : nullptr))) return rc;
    planes->resize(count);
    for (size_t i = 0; i < count; ++i) (*planes)[i] = mk_dev_plane(mo + i * np, d.w, d.h);
    return ARTGPU_OK;
}

// Checks and derives everything; launches nothing and takes no pool slot, so a refused frame leaves the output planes alone.  The checks, in the
// order they report (a frame that is wrong in two ways names the first):
//   1. ctx, raw / p / out, the border, the Resize tool's result, the output's size (then hipSetDevice, the one HIP call here; then rs_check; then cg_check,
//   whose result the mode walk needs; before it df_plan: defringe's radius, window and curve)   2. artgpu_set_pipeline_masks' counts against the frame's
//   3. local contrast masks: region list, mk_plan   4. texture boost masks: region list, mk_plan   5. colour correction: texture boost's masks from a YUV image,
//   cc_check, mk_plan   6. smoothing: its masks from a YUV image, sm_check, sm_plan_region of the mask-less regions, mk_plan   7. local_contrast_check
//   8. dehaze_check, te_check, fs_check, fg_check, sl_check, bw_check (and a colour cast in front of the Resize tool)   9. sharpening: X-Trans with the automatic radius, sharpen_check   10. tb_check
//   then the oldest stages in the order they run:   11. the CA correction's pattern and size (do_ca), demosaic_bayer_check / demosaic_xtrans_check
//   12. dn_compute_params_check (AUTOMATIC chroma)   13. denoise_tool_check   14. tone_curve_check / tone_neutral_check
// What is left to the stages is a refusal that depends on a number computed on the device: the automatic sharpening radius (pipe_stage2).  RGB_denoise's
// "too small for n wavelet levels" is not one: dn_plan caps the levels by the smaller side (maxlev2), and for every cap the side already holds them
// (levels 8 / 7 / 6 / 5 / 4 / 3 need a side of 255 / 127 / 63 / 31 / 15 / 7), so it fires for w or h under 8 alone, which check 1 has refused.
static int pipeline_plan(artgpu_ctx *ctx, const artgpu_plane *raw_in, const artgpu_pipeline_params *p, const artgpu_rgb *out, bool do_ca, PipePlan *pl)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(raw_in) || !p || !out) return fail(ctx, ARTGPU_EINVAL, "pipeline_run: null/bad argument");
    const int b = p->border, w = raw_in->w - 2 * b, h = raw_in->h - 2 * b, nlc = p->local_contrast_nregions, ntb = p->texture_boost_nregions;
    const double scale = p->scale > 0 ? p->scale : 1.0;
    pl->W = raw_in->w; pl->H = raw_in->h; pl->b = b; pl->w = w; pl->h = h; pl->scale = scale;
    if (b < 0 || w < 8 || h < 8) return fail(ctx, ARTGPU_EINVAL, "pipeline_run: border %d leaves no image", b);
    // ImProcFunctions::resizeScale on the image behind the border, and simpleprocess.cc:406-407's decision
    pl->rs_on = pipeline_resize(ctx, w, h, &pl->imw, &pl->imh, &pl->rs_scale);
    if (pl->imw < 1 || pl->imh < 1) return fail(ctx, ARTGPU_EINVAL, "pipeline_run: the Resize tool leaves no image (%dx%d)", pl->imw, pl->imh);
    if (out->r.w != pl->imw || out->r.h != pl->imh) return fail(ctx, ARTGPU_EINVAL, "pipeline_run: output must be %dx%d", pl->imw, pl->imh);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    if (pl->rs_on && (rc = rs_check(ctx, w, h, pl->imw, pl->imh, pl->rs_scale, "pipeline_run(resize)"))) return rc;
    const artgpu_ctx::Shared &s = ctx->shared;
    pl->lc_on = p->local_contrast_enabled && nlc > 0; pl->lc_gen = pl->lc_on && s.pipe_lc;
    pl->tb_on = p->texture_boost_enabled != 0;        pl->tb_gen = pl->tb_on && ntb > 0 && s.pipe_tb;
    pl->cc_on = s.pipe_ncc > 0 && s.pipe_cc;          pl->cc_gen = pl->cc_on && s.pipe_cc_masks;
    pl->sm_on = s.pipe_nsm > 0 && s.pipe_sm;          pl->sm_gen = pl->sm_on && s.pipe_sm_masks;
    // The image's colour mode in front of each tool, in pipe order, as the reference has it: sharpening works on RGB; colorCorrection generates its masks
    // on RGB and leaves YUV; guidedSmoothing generates its masks on what it finds, then setMode(RGB); textureBoost likewise, then setMode(YUV), and ends in
    // RGB for the tone curve and localContrast (whose LAB, masks included, is its own switch).  The mask engine reads RGB only: masks to be generated
    // on a YUV image fail the frame.  Colour correction ends with the next tool's setMode(RGB) (to_rgb) unless that tool is texture boost, which then skips
    // its own switch (in_yuv).  '-': not read; the mask columns say what happens where the pipe generates that tool's masks
    //   cc sm | in front of sm | in front of tb | cc to_rgb (tb off / on) | tb in_yuv | sm's masks | tb's masks
    //    0  0 |       -        |      RGB       |           -             |     0     |     -      |    ok
    //    0  1 |      RGB       |      RGB       |           -             |     0     |     ok     |    ok
    //    1  0 |       -        |      YUV       |         1 / 0           |     1     |     -      |  refused
    //    1  1 |      YUV       |      RGB       |         1 / 1           |     0     |  refused   |    ok
    // Impulse noise reduction and defringe sit between the sharpening and colour correction; the first of them that runs does setMode(LAB), and the image
    // stays LAB until the next tool's setMode (id: either runs).  The mask engine reads LAB, so whatever finds the LAB image generates its masks on it:
    //   id cc sm | in front of cc | in front of sm | in front of tb | hand-over
    //    1  1  . |      LAB       |   as above     |   as above     | cc's masks on LAB, lab_to_yuv, cc from_yuv; then the rows above
    //    1  0  1 |       -        |      LAB       |      RGB       | sm's masks on LAB, lab_to_rgb (sm's setMode(RGB))
    //    1  0  0 |       -        |       -        |      LAB       | tb's masks on LAB, lab_to_yuv, tb in_yuv; without tb (or with a gradient filter ahead of
    //            |                |                |                | it: creativeGradients' setMode(RGB)) STAGE_2 ends with lab_to_rgb
    if (s.pipe_imp_on) pl->imp = imp_plan(w, h, &s.pipe_imp, scale);
    pl->imp_on = s.pipe_imp_on && !pl->imp.early;
    if (s.pipe_df_on && (rc = df_plan(ctx, w, h, &s.pipe_df, scale, "pipeline_run(defringe)", &pl->df))) return rc;
    pl->df_on = s.pipe_df_on && !pl->df.early;
    pl->id_lab = pl->imp_on || pl->df_on;
    PipeMode mode = pl->cc_on ? PIPE_YUV : (pl->id_lab ? PIPE_LAB : PIPE_RGB);           // (sharpening: RGB in, RGB out)
    const bool sm_masks_from_yuv = pl->sm_gen && mode == PIPE_YUV;
    pl->sm_from_lab = pl->sm_on && mode == PIPE_LAB;
    if (pl->sm_on) mode = PIPE_RGB;
    // creativeGradients, the first step of STAGE_3, starts with setMode(RGB): behind colour correction that is the switch colour correction ends with
    if (s.pipe_cg_on) {
        artgpu_creative_gradients_params cgp = s.pipe_cg;
        cgp.offset_x = cgp.offset_y = 0; cgp.full_width = w; cgp.full_height = h; cgp.scale = 1.0;
        if ((rc = cg_check(ctx, w, h, &cgp, "pipeline_run(creative gradients)", &pl->cg))) return rc;
        if (pl->cg.apply_gradient || pl->cg.apply_pcvignette) { pl->lab_to_rgb_end = mode == PIPE_LAB; mode = PIPE_RGB; }
    }
    const bool tb_masks_from_yuv = pl->tb_gen && mode == PIPE_YUV;
    pl->tb_from_lab = pl->tb_on && mode == PIPE_LAB;
    pl->tb_in_yuv = pl->tb_on && mode != PIPE_RGB;
    pl->cc_to_rgb = !pl->tb_in_yuv;
    if (mode == PIPE_LAB && !pl->tb_on) pl->lab_to_rgb_end = true;     // film grain, the tone curve, the end of the pipe: setMode(RGB)
    // regions whose blend planes the pipe generates itself (artgpu_set_pipeline_masks): the regions' own `mask` pointers are
    // not read, the planes of artgpu_generate_masks take their place; what it does not support fails the frame here
    if ((pl->lc_gen && s.pipe_nlc != nlc) || (pl->tb_gen && s.pipe_ntb != ntb))
        return fail(ctx, ARTGPU_EINVAL, "pipeline_run: artgpu_set_pipeline_masks holds %d / %d entries, the frame has %d / %d regions", s.pipe_nlc, s.pipe_ntb, nlc, ntb);
    const auto own = [](auto &regs, const auto *src, int n) { regs.assign(src, src + n); for (auto &r : regs) r.mask = nullptr; };
    if (pl->lc_gen) {
        if (!p->local_contrast_regions) return fail(ctx, ARTGPU_EINVAL, "pipeline_run(local contrast): bad region list");
        own(pl->lc_regs, p->local_contrast_regions, nlc);
        if ((rc = pipe_plan_masks(ctx, p, *pl, ARTGPU_MASKS_MODE_LAB, s.pipe_lc, nlc, false, "pipeline_run(local contrast masks)", &pl->lc_mk))) return rc;
    }
    if (pl->tb_gen) {
        if (!p->texture_boost_regions) return fail(ctx, ARTGPU_EINVAL, "pipeline_run(texture boost): bad region list");
        own(pl->tb_regs, p->texture_boost_regions, ntb);
        if ((rc = pipe_plan_masks(ctx, p, *pl, pl->tb_from_lab ? ARTGPU_MASKS_MODE_LAB : ARTGPU_MASKS_MODE_RGB, s.pipe_tb, ntb, false, "pipeline_run(texture boost masks)", &pl->tb_mk))) return rc;
    }
    pl->lc_regions = pl->lc_gen ? pl->lc_regs.data() : p->local_contrast_regions;
    pl->tb_regions = pl->tb_gen ? pl->tb_regs.data() : p->texture_boost_regions;
    if (pl->cc_on) {      // ImProcFunctions::colorCorrection (artgpu_set_pipeline_color_correction)
        if (tb_masks_from_yuv)
            return fail(ctx, ARTGPU_EUNSUPPORTED, "pipeline_run: colour correction leaves the image in YUV mode, which the mask engine cannot generate texture boost's masks from");
        if ((rc = cc_check(ctx, w, h, s.pipe_cc, s.pipe_ncc, p->ws, p->iws, !pl->cc_gen, "pipeline_run(colour correction)", &pl->cc))) return rc;
        if (pl->cc_gen && (rc = pipe_plan_masks(ctx, p, *pl, pl->id_lab ? ARTGPU_MASKS_MODE_LAB : ARTGPU_MASKS_MODE_RGB, s.pipe_cc_masks, s.pipe_ncc, true, "pipeline_run(colour correction masks)", &pl->cc_mk))) return rc;
    }
    if (pl->sm_on) {      // ImProcFunctions::guidedSmoothing (artgpu_set_pipeline_smoothing): what does not depend on a mask's box is checked here
        if (sm_masks_from_yuv)
            return fail(ctx, ARTGPU_EUNSUPPORTED, "pipeline_run: colour correction leaves the image in YUV mode, which the mask engine cannot generate smoothing's masks from");
        if ((rc = sm_check(ctx, w, h, s.pipe_sm, s.pipe_nsm, p->ws, scale, !pl->sm_gen, "pipeline_run(smoothing)"))) return rc;
        for (int i = 0; i < s.pipe_nsm && !pl->sm_gen; ++i) {       // a region without a mask is the frame: its limits are known now
            SmRegionPlan sp;
            if (!s.pipe_sm[i].mask && (rc = sm_plan_region(ctx, w, h, s.pipe_sm[i], nullptr, scale, "pipeline_run(smoothing)", i, &sp))) return rc;
        }
        if (pl->sm_gen && (rc = pipe_plan_masks(ctx, p, *pl, pl->sm_from_lab ? ARTGPU_MASKS_MODE_LAB : ARTGPU_MASKS_MODE_RGB, s.pipe_sm_masks, s.pipe_nsm, false, "pipeline_run(smoothing masks)", &pl->sm_mk))) return rc;
    }
    if (pl->lc_on && (rc = local_contrast_check(ctx, w, h, pl->lc_regions, nlc, scale, "pipeline_run(local contrast)"))) return rc;
    if (p->dehaze_enabled && (rc = dehaze_check(ctx, w, h, &p->dehaze, p->ws, scale, "pipeline_run(dehaze)", &pl->dehaze))) return rc;
    pl->te_on = s.pipe_te_on && s.pipe_te.enabled;
    if (pl->te_on && (rc = te_check(ctx, w, h, &s.pipe_te, p->ws, scale, "pipeline_run(tone equalizer)", &pl->te))) return rc;
    pl->fs_on = s.pipe_fs != nullptr;
    if (pl->fs_on && (rc = fs_check(ctx, s.pipe_fs, &s.pipe_fs_par, "pipeline_run(film simulation)"))) return rc;
    if (s.pipe_fg_on && (rc = fg_check(ctx, w, h, &s.pipe_fg, p->ws, scale, 1, "pipeline_run(film grain)", &pl->fg))) return rc;      // (the batch pipe is the OUTPUT pipeline)
    if (s.pipe_sl_on && (rc = sl_check(ctx, &s.pipe_sl, "pipeline_run(soft light)", &pl->sl))) return rc;
    if (s.pipe_bw_on && (rc = bw_check(ctx, &s.pipe_bw, p->ws, "pipeline_run(black and white)", &pl->bw))) return rc;
    if (pl->bw.on && pl->bw.ulut && pl->rs_on)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "pipeline_run(black and white): the colour cast leaves the image in YUV mode, which the Resize tool's switch to LAB does not start from");
    // sharpening (STAGE_2): method, scale and, with the automatic radius, the sensor are checked before any stage runs
    pl->shpar = p->sharpening;
    pl->sh_on = p->sharpening_enabled != 0;
    pl->sh_auto = pl->sh_on && pl->shpar.enabled && p->sharpening_auto_radius;      // simpleprocess.cc:274
    if (pl->sh_on) {
        if (pl->sh_auto && p->sensor != 0) return fail(ctx, ARTGPU_EUNSUPPORTED, "pipeline_run(sharpening): the automatic radius of X-Trans frames is not on the device path");
        if (pl->sh_auto) pl->shpar.deconvradius = 0.75;                             // (replaced in pipe_stage2; the check is about everything else)
        if ((rc = sharpen_check(ctx, w, h, &pl->shpar, scale, "pipeline_run(sharpening)", &pl->sharpen))) return rc;
    }
    pl->sh_radius_pending = pl->sh_auto && !pl->sharpen.early;
    if (pl->tb_on && (rc = tb_check(ctx, w, h, pl->tb_regions, ntb, p->ws, scale, 1, "pipeline_run(texture boost)", &pl->tb))) return rc;
    unsigned cfa;
    if (do_ca && pipeline_ca(p) && (rc = pipeline_ca_check(ctx, pl->W, pl->H, p, &cfa))) return rc;
    // (X-Trans: no CA correction, so the demosaic reads the caller's plane: a device plane's own rows, a staged host plane's dense ones)
    if (p->sensor == 0) rc = demosaic_bayer_check(ctx, p->bayer_method, p->filters, p->initial_gain, pl->W, pl->H);
    else rc = demosaic_xtrans_check(ctx, p->xtrans_passes, p->xtrans, pl->W, pl->H, raw_in->on_device ? (size_t)(raw_in->row_stride_bytes / 4) : (size_t)pl->W);
    if (rc) return rc;
    if (p->denoise_enabled) {
        if (p->denoise.dn.chrominance_method == 1 && (rc = dn_compute_params_check(ctx, pl->W, pl->H, b))) return rc;
        if ((rc = denoise_tool_check(ctx, w, h, &p->denoise, p->iws, scale))) return rc;
    }
    if (p->tone_enabled && p->tone_mode == ARTGPU_TONE_NEUTRAL) return tone_neutral_check(ctx, p->tone_lut, p->white_point);
    return p->tone_enabled ? tone_curve_check(ctx, p->tone_mode, p->white_point) : ARTGPU_OK;
}

// The raw side: RawImageSource::CA_correct_RT between scaleColors and the demosaic, on a device copy (the caller's raw is never written), and
// RawImageSource::getDeconvAutoRadius on the plane the demosaic reads (simpleprocess.cc:274-278 after preprocess): launched here, its one
// number is waited for where the sharpening needs it
static int pipe_raw_side(artgpu_ctx *ctx, const artgpu_pipeline_params *p, const PipePlan &pl, const artgpu_plane *raw_in, bool do_ca, PipeFrame *fr)
{
    const int W = pl.W, H = pl.H;
    int rc;
    float *cp, *res;
    fr->raw = *raw_in;
    if (do_ca && pipeline_ca(p)) {
        if ((rc = plane_to_pool(ctx, raw_in, P_CA_RAW, &cp)) || (rc = pipeline_ca_dev(ctx, cp, W, W, H, p))) return rc;
        fr->raw = mk_dev_plane(cp, W, H);
    }
    if (!pl.sh_radius_pending) return ARTGPU_OK;
    const float *rp = fr->raw.p;
    size_t rstride = (size_t)(fr->raw.row_stride_bytes / 4);
    if (!fr->raw.on_device) {
        const size_t need = std::max((size_t)W * H, (size_t)SHP_NPLANES * pl.w * pl.h) * 4;
        if ((rc = pool_get(ctx, P_SH_PLANES, need, &cp)) || (rc = plane_into(ctx, &fr->raw, cp))) return rc;
        rp = cp; rstride = W;
    }
    if ((rc = auto_radius_dev(ctx, rp, rstride, W, H, p->filters, 1000.f, p->sharpening_clip_val, &res))) return rc;
    if (!ctx->sh_host) {
        if (hipHostMalloc(reinterpret_cast<void **>(&ctx->sh_host), 64, hipHostMallocDefault) != hipSuccess) { ctx->sh_host = nullptr; return fail(ctx, ARTGPU_ENOMEM, "pipeline_run(sharpening): pinned word"); }
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->sh_ev, hipEventDisableTiming));
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->sh_host, res, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->sh_ev, ctx->stream));
    return ARTGPU_OK;
}

// The demosaic into planes of the context pool (they never leave the device), and the image the remaining stages work on
static int pipe_demosaic(artgpu_ctx *ctx, const artgpu_pipeline_params *p, const PipePlan &pl, artgpu_rgb *out, PipeFrame *fr)
{
    float *dp[3];
    int rc;
    for (int k = 0; k < 3; ++k)
        if ((rc = pool_get(ctx, P_PIPE_R + k, (size_t)pl.W * pl.H * 4, &dp[k]))) return rc;
    fr->dem = DevRGB{{dp[0], dp[1], dp[2]}, (size_t)pl.W, pl.W, pl.H, false};
    const artgpu_rgb dem = mk_dev_rgb(dp, pl.W, pl.H, pl.W);
    DevImage di;                   // (a host CFA plane is staged here)
    if ((rc = bind_images(ctx, &fr->raw, &dem, &di))) return rc;
    if (p->sensor == 0) {
        StageScope scope_(ctx, "RawImageSource::demosaic (Bayer)");
        rc = demosaic_bayer_dev(ctx, di, pl.W, pl.H, p->bayer_method, p->filters, p->initial_gain, pl.b);
    } else {
        StageScope scope_(ctx, "RawImageSource::xtrans_interpolate");
        rc = demosaic_xtrans_dev(ctx, di, pl.W, pl.H, p->xtrans_passes, p->xtrans_passes > 1 ? 1 : 0, p->xtrans, p->rgb_cam);
    }
    if (rc) return rc;
    if (pl.rs_on) {
        // the full-size working image cannot be the caller's planes: they have the size the resampler writes
        if ((rc = bind_rgb(ctx, out, 4, false, &fr->small, "pipeline_run(out)"))) return rc;
        for (int k = 0; k < 3; ++k)
            if ((rc = pool_get(ctx, P_RS_IMG0 + k, (size_t)pl.w * pl.h * 4, &fr->d.p[k]))) return rc;
        fr->d.stride = pl.w; fr->d.w = pl.w; fr->d.h = pl.h; fr->d.staged = false;
    } else if ((rc = bind_rgb(ctx, out, 4, false, &fr->d, "pipeline_run(out)"))) return rc;
    return ARTGPU_OK;
}

// From the demosaiced planes to the exposed image: denoiseComputeParams, getImage + convertColorSpace + the denoise tool, dehaze (STAGE_0), the exposure and
// the tone equalizer (STAGE_1)
static int pipe_input(artgpu_ctx *ctx, const artgpu_pipeline_params *p, const PipePlan &pl, PipeFrame *fr)
{
    const double *cam_to_work = p->has_cam_to_work ? p->cam_to_work : nullptr;
    const DevRGB &d = fr->d;
    int rc;
    artgpu_denoise_tool_params dnp = p->denoise;
    if (p->denoise_enabled && dnp.dn.chrominance_method == 1) {
        // ipf.denoiseComputeParams(imgsrc, currWB, dnstore, params.denoise) before getImage (simpleprocess.cc:254-256); a fresh store per frame
        static const double ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        artgpu_denoise_info_store store = {};
        if ((rc = dn_compute_params_dev(ctx, fr->dem, pl.b, p->mul, p->do_clip, cam_to_work ? cam_to_work : ident, p->ws,
                                        p->chrominance_auto_factor != 0.0 ? p->chrominance_auto_factor : 1.0, &store, &dnp.dn)))
            return rc;
    }
    if (p->denoise_enabled) {
        // getImage + convertColorSpace in front of the tool and the STAGE_1 exposure behind it live in the tool's own pixel passes where
        // its parameters allow (improc_denoise_dev: otherwise they run as the separate passes)
        static const double curve_points[9] = {1 /*FCT_MinMaxCPoints*/, 0.05, 0.50, 0.35, 0.35, 0.35, 0.05, 0.35, 0.35};   // ipdenoise.cc:1139-1149
        float curve[501];
        (void)noise_curve_lut(curve_points, 9, curve);
        const double ecomp = p->exposure_enabled ? p->expcomp : 0.0;       // ipdenoise.cc:1155
        artgpu_denoise_fusion fu = {};
        fu.sx1 = pl.b; fu.sy1 = pl.b;                       // (the demosaiced planes travel as fr->dem)
        for (int k = 0; k < 3; ++k) fu.mul[k] = p->mul[k];
        fu.do_clip = p->do_clip; fu.cam_to_work = cam_to_work;
        fu.exposure_enabled = p->exposure_enabled && !p->dehaze_enabled ? 1 : 0;      // (dehaze sits between the tool and the exposure)
        fu.exp_scale = (float)std::pow(2.0, p->expcomp); fu.black = (float)(p->black * 2000.0);
        StageScope scope_(ctx, "ImProcFunctions::denoise");
        if ((rc = improc_denoise_dev(ctx, d, &fr->dem, &fu, true, &dnp, p->ws, p->iws, ecomp, pl.scale, cam_to_work, curve, 0u))) return rc;
    } else {
        StageScope scope_(ctx, "RawImageSource::getImage");
        if ((rc = get_image_dev(ctx, fr->dem, d, pl.b, pl.b, 1, p->mul, p->do_clip, cam_to_work))) return rc;
    }
    // ImProcFunctions::dehaze, STAGE_0 of ImProcFunctions::process (improcfun.cc:577), ahead of the exposure (STAGE_1)
    if (p->dehaze_enabled && (rc = dehaze_dev(ctx, d.p, d.stride, d.w, d.h, &p->dehaze, p->ws, pl.dehaze, nullptr))) return rc;
    if (p->exposure_enabled && (!p->denoise_enabled || p->dehaze_enabled)) {
        StageScope scope_(ctx, "ImProcFunctions::expcomp");
        if ((rc = exposure_dev(ctx, d, (float)std::pow(2.0, p->expcomp), (float)(p->black * 2000.0)))) return rc;
    }
    // ImProcFunctions::toneEqualizer, the last step of STAGE_1 (improcfun.cc:588), behind the exposure wherever that ran
    if (pl.te_on) return tone_equalizer_dev(ctx, d.p, d.stride, d.w, d.h, &ctx->shared.pipe_te, p->ws, pl.te, "pipeline_run(tone equalizer)");
    return ARTGPU_OK;
}

// STAGE_2 of ImProcFunctions::process: sharpening, impulsedenoise, defringe, colorCorrection, guidedSmoothing
static int pipe_stage2(artgpu_ctx *ctx, const artgpu_pipeline_params *p, const PipePlan &pl, PipeFrame *fr)
{
    const DevRGB &d = fr->d;
    const artgpu_ctx::Shared &s = ctx->shared;
    std::vector<artgpu_plane> gen;
    int rc;
    // ImProcFunctions::sharpening, the first step of STAGE_2 (improcfun.cc:595; simpleprocess.cc:395 between the exposure and the tone curve)
    if (pl.sh_on) {
        artgpu_sharpening_params shpar = pl.shpar;
        SharpenPlan shp = pl.sharpen;
        if (pl.sh_radius_pending) {
            HIPCHK(ctx, hipEventSynchronize(ctx->sh_ev));
            shpar.deconvradius = auto_radius_of(ctx->sh_host[0]);                    // params.sharpening.deconvradius = r
            if ((rc = sharpen_check(ctx, d.w, d.h, &shpar, pl.scale, "pipeline_run(sharpening, automatic radius)", &shp))) return rc;
        }
        if ((rc = sharpen_dev(ctx, d.p, d.stride, d.w, d.h, &shpar, p->ws, shp, nullptr))) return rc;
    }
    // ImProcFunctions::impulsedenoise and ::defringe (improcfun.cc:597-599): the first that runs switches to LAB mode, which the image keeps
    if (pl.imp_on && (rc = impulse_denoise_dev(ctx, d, pl.imp, p->ws, nullptr, 0, 0, nullptr))) return rc;
    if (pl.df_on && (rc = defringe_dev(ctx, d, pl.df, p->ws, nullptr, pl.imp_on, 0, nullptr))) return rc;
    // ImProcFunctions::colorCorrection, STAGE_2 behind them (improcfun.cc:601): generateMasks(rgb, ., &Lmask, &abmask) on the image as it is, RGB or LAB
    // (ipcolorcorrection.cc:236), then the tool, whose setMode(YUV) on a LAB image is lab_to_yuv.  It leaves the image in YUV mode for textureBoost,
    // whose setMode(YUV) is then a no-op
    if (pl.cc_on) {
        const int n = s.pipe_ncc;
        std::vector<artgpu_color_correction_region> regs(s.pipe_cc, s.pipe_cc + n);
        if (pl.cc_gen && (rc = pipe_gen_masks(ctx, p, d, P_CC_GEN, s.pipe_cc_masks, pl.cc_mk, n, true, &gen))) return rc;
        for (int i = 0; i < n && pl.cc_gen; ++i) { regs[i].lmask = &gen[i]; regs[i].abmask = &gen[n + i]; }
        if (pl.id_lab && (rc = lab_to_yuv_dev(ctx, d, p->iws))) return rc;
        if ((rc = color_correction_dev(ctx, d.p, d.stride, d.w, d.h, regs.data(), pl.cc, pl.id_lab, pl.cc_to_rgb, nullptr))) return rc;
    }
    // ImProcFunctions::guidedSmoothing, the last step of STAGE_2 (improcfun.cc:602): generateMasks on the image (ipsmoothing.cc:929), setMode(RGB)
    // (colour correction ahead of it ends with that switch), the tool
    if (pl.sm_on) {
        const int n = s.pipe_nsm;
        std::vector<artgpu_smoothing_region> regs(s.pipe_sm, s.pipe_sm + n);
        if (pl.sm_gen && (rc = pipe_gen_masks(ctx, p, d, P_SM_GEN, s.pipe_sm_masks, pl.sm_mk, n, false, &gen))) return rc;
        for (int i = 0; i < n && pl.sm_gen; ++i) regs[i].mask = &gen[i];
        if (pl.sm_from_lab && (rc = lab_switch_dev(ctx, d, p->iws, false))) return rc;
        if ((rc = smoothing_dev(ctx, d.p, d.stride, d.w, d.h, regs.data(), n, p->ws, pl.scale, nullptr, "pipeline_run(smoothing)"))) return rc;
    }
    if (pl.lab_to_rgb_end) return lab_switch_dev(ctx, d, p->iws, false);
    return ARTGPU_OK;
}

// STAGE_3 of ImProcFunctions::process and what follows: creativeGradients, textureBoost, filmGrain, filmSimulation on either side of the tone curve, softLight, localContrast,
// blackAndWhite, [the Resize tool]; then the image goes back to the caller's planes
static int pipe_stage3(artgpu_ctx *ctx, const artgpu_pipeline_params *p, PipePlan &pl, artgpu_rgb *out, PipeFrame *fr)
{
    const DevRGB &d = fr->d;
    const int ntb = p->texture_boost_nregions, nlc = p->local_contrast_nregions;
    const artgpu_ctx::Shared &s = ctx->shared;
    std::vector<artgpu_plane> gen;
    int rc;
    // ImProcFunctions::creativeGradients, the first step of STAGE_3 (improcfun.cc:605)
    if ((rc = creative_gradients_dev(ctx, d.p, d.stride, d.w, d.h, pl.cg))) return rc;
    // ImProcFunctions::textureBoost, the next step of STAGE_3 (improcfun.cc:606); the batch pipe is the OUTPUT pipeline: high_detail
    if (pl.tb_gen && (rc = pipe_gen_masks(ctx, p, d, P_MK_OUT, ctx->shared.pipe_tb, pl.tb_mk, ntb, false, &gen))) return rc;   // iptextureboost.cc:210, ahead of setMode(YUV)
    for (int i = 0; i < ntb && pl.tb_gen; ++i) pl.tb_regs[i].mask = &gen[i];
    if (pl.tb_from_lab && (rc = lab_to_yuv_dev(ctx, d, p->iws))) return rc;          // textureBoost's setMode(YUV) on the LAB image impulsedenoise / defringe left
    if (pl.tb_on && (rc = texture_boost_dev(ctx, d.p, d.stride, d.w, d.h, pl.tb_regions, ntb, p->ws, pl.tb, 1, nullptr, pl.tb_in_yuv))) return rc;
    // ImProcFunctions::filmGrain, right behind texture boost (improcfun.cc:608): its guidedSmoothing starts with setMode(RGB), which texture boost ended with
    if (pl.fg.info.nregions > 0 && (rc = film_grain_dev(ctx, d.p, d.stride, d.w, d.h, p->ws, pl.fg))) return rc;
    // ImProcFunctions::filmSimulation ahead of the tone curve (improcfun.cc:614-616; the image is in RGB mode: texture boost ends with that switch)
    if (pl.fs_on && !s.pipe_fs_after && (rc = film_simulation_dev(ctx, d.p, d.stride, d.w, d.h, s.pipe_fs, &s.pipe_fs_par))) return rc;
    if (p->tone_enabled && p->tone_mode == ARTGPU_TONE_NEUTRAL) {
        artgpu_neutral_state st;
        for (int k = 0; k < 9; ++k) { st.ws[k] = p->ws[k]; st.iws[k] = p->iws[k]; st.to_out[k] = p->to_out[k]; st.to_work[k] = p->to_work[k]; }
        StageScope scope_(ctx, "ImProcFunctions::toneCurve (NEUTRAL)");
        if ((rc = tone_neutral_dev(ctx, d, p->tone_lut, p->white_point, &st))) return rc;
    } else if (p->tone_enabled) {
        StageScope scope_(ctx, "ImProcFunctions::toneCurve");
        if ((rc = tone_curve_dev(ctx, d, p->tone_lut, p->white_point, 1))) return rc;
    }
    // ... or right behind it (filmSimulation.after_tone_curve, L618-620)
    if (pl.fs_on && s.pipe_fs_after && (rc = film_simulation_dev(ctx, d.p, d.stride, d.w, d.h, s.pipe_fs, &s.pipe_fs_par))) return rc;
    // ImProcFunctions::softLight (improcfun.cc:623): setMode(RGB) is a no-op here
    if (pl.sl.on && (rc = soft_light_dev(ctx, d, pl.sl))) return rc;
    // ImProcFunctions::localContrast (improcfun.cc:625): setMode(LAB), [generateMasks on the LAB image, iplocalcontrast.cc:454,] the regions on the
    // L plane (Imagefloat::g), back to RGB
    if (pl.lc_on) {
        if ((rc = lab_switch_dev(ctx, d, p->ws, true)) || (pl.lc_gen && (rc = pipe_gen_masks(ctx, p, d, P_MK_OUT, ctx->shared.pipe_lc, pl.lc_mk, nlc, false, &gen)))) return rc;
        for (int i = 0; i < nlc && pl.lc_gen; ++i) pl.lc_regs[i].mask = &gen[i];
        if ((rc = local_contrast_dev(ctx, d.p[1], d.stride, d.w, d.h, pl.lc_regions, nlc, nullptr))) return rc;
        // (with the Resize tool the image stays in LAB mode, as in the reference: iplocalcontrast.cc:441 does not switch back; blackAndWhite's
        // setMode(RGB) is that switch when the tool is on)
        if ((!pl.rs_on || pl.bw.on) && (rc = lab_switch_dev(ctx, d, p->iws, false))) return rc;
    }
    // ImProcFunctions::blackAndWhite (improcfun.cc:627).  With a colour cast the reference leaves YUV; the next setMode(RGB) (rgb2out's) happens here
    if (pl.bw.on && (rc = black_and_white_dev(ctx, d.p, d.stride, d.w, d.h, p->ws, pl.bw, 1))) return rc;
    if (!pl.rs_on) return unbind_rgb(ctx, out, &d);
    // ImProcFunctions::resize (simpleprocess.cc:402-414): Lanczos' setMode(LAB) is a no-op behind localContrast; the switch to RGB happens on the
    // small image (iprgb2out.cc:455); behind blackAndWhite the image is in RGB mode, whatever ran before
    if ((rc = resize_dev(ctx, d, fr->small, pl.rs_scale, pl.lc_on && !pl.bw.on ? nullptr : p->ws, p->iws))) return rc;
    return unbind_rgb(ctx, out, &fr->small);
}

} // namespace

namespace artgpu { namespace api {

// One frame: the plan, then the stages (do_ca: artgpu_pipeline_run; io_frame has corrected its staged CFA plane itself).  The stages call *_dev
// functions only, so a stage that reports to the progress listener / roctx does it through a StageScope opened here or in improc_denoise_dev, under
// the name its entry point reports.  Which report: the frame itself, the demosaic, ImProcFunctions::denoise (inside it denoise::RGB_denoise,
// denoiseGuidedSmoothing, NLMeans, and getImage or expcomp where the tool could not fuse them), getImage without the tool, the exposure on its own,
// the two tone curves.  Silent inside a frame: CA correction, denoiseComputeParams, the Lab switches and every tool that has a *_check in the plan's
// items 1 - 10 (whether those should report is a question of behaviour, not of structure).
int pipeline_run_impl(artgpu_ctx *ctx, const artgpu_plane *raw_in, const artgpu_pipeline_params *p, artgpu_rgb *out, bool do_ca)
{
    StageScope scope_(ctx, "ImageProcessor (stage_init .. stage_finish)");
    PipePlan pl{};
    PipeFrame fr;
    int rc;
    if ((rc = pipeline_plan(ctx, raw_in, p, out, do_ca, &pl)) || (rc = pipe_raw_side(ctx, p, pl, raw_in, do_ca, &fr)) || (rc = pipe_demosaic(ctx, p, pl, out, &fr)) ||
        (rc = pipe_input(ctx, p, pl, &fr)) || (rc = pipe_stage2(ctx, p, pl, &fr)))
        return rc;
    return pipe_stage3(ctx, p, pl, out, &fr);
}

} } // namespace artgpu::api

extern "C" {

int artgpu_set_pipeline_masks(artgpu_ctx *ctx, const artgpu_mask_params *lc, int nlc, const artgpu_mask_params *tb, int ntb)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (nlc < 0 || ntb < 0 || (nlc > 0 && !lc) || (ntb > 0 && !tb)) return fail(ctx, ARTGPU_EINVAL, "set_pipeline_masks: bad arguments");
    ctx->shared.pipe_lc = own_pipe_masks(ctx->pipe_lc_own, lc, nlc); ctx->shared.pipe_nlc = nlc;
    ctx->shared.pipe_tb = own_pipe_masks(ctx->pipe_tb_own, tb, ntb); ctx->shared.pipe_ntb = ntb;
    return ARTGPU_OK;
}

int artgpu_pipeline_run(artgpu_ctx *ctx, const artgpu_plane *raw, const artgpu_pipeline_params *p, artgpu_rgb *out)
{
    return pipeline_run_impl(ctx, raw, p, out, true);
}

int artgpu_set_pipeline_color_correction(artgpu_ctx *ctx, const artgpu_color_correction_region *regions, int n, const artgpu_mask_params *masks)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (n < 0 || (n > 0 && !regions) || (n == 0 && masks)) return fail(ctx, ARTGPU_EINVAL, "set_pipeline_color_correction: bad arguments");
    own_pipe_regions(ctx->pipe_cc_own, regions, n, {&artgpu_color_correction_region::lmask, &artgpu_color_correction_region::abmask}, masks,
                     &ctx->shared.pipe_cc, &ctx->shared.pipe_cc_masks, &ctx->shared.pipe_ncc);
    return ARTGPU_OK;
}

int artgpu_set_pipeline_impulse_defringe(artgpu_ctx *ctx, const artgpu_impulse_denoise_params *impulse, const artgpu_defringe_params *defringe)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (defringe && (defringe->nhuecurve < 0 || (defringe->nhuecurve > 0 && !defringe->huecurve))) return fail(ctx, ARTGPU_EINVAL, "set_pipeline_impulse_defringe: bad hue curve");
    artgpu_ctx::Shared &s = ctx->shared;
    s.pipe_imp_on = impulse != nullptr;
    s.pipe_imp = impulse ? *impulse : artgpu_impulse_denoise_params{};
    s.pipe_df_on = defringe != nullptr;
    s.pipe_df = defringe ? *defringe : artgpu_defringe_params{};
    ctx->pipe_df_curve.assign(s.pipe_df.huecurve, s.pipe_df.huecurve + s.pipe_df.nhuecurve);
    s.pipe_df.huecurve = ctx->pipe_df_curve.empty() ? nullptr : ctx->pipe_df_curve.data();
    return ARTGPU_OK;
}

int artgpu_set_pipeline_smoothing(artgpu_ctx *ctx, const artgpu_smoothing_region *regions, int n, const artgpu_mask_params *masks)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (n < 0 || (n > 0 && !regions) || (n == 0 && masks)) return fail(ctx, ARTGPU_EINVAL, "set_pipeline_smoothing: bad arguments");
    own_pipe_regions(ctx->pipe_sm_own, regions, n, {&artgpu_smoothing_region::mask}, masks, &ctx->shared.pipe_sm, &ctx->shared.pipe_sm_masks, &ctx->shared.pipe_nsm);
    return ARTGPU_OK;
}

} // extern "C"
