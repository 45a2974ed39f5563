// art_amd/csrc/api_internal.h -- what the host files of the C ABI share: the context, the staging and pool helpers, and per stage
// exactly the plan structs and *_dev / *_check / *_plan functions that ANOTHER file calls: the frame driver (api_pipeline.hip), io_frame
// (api_batch.hip) or a sibling stage.  This header is the list of what a stage exposes; everything a stage uses only itself stays
// static or in an anonymous namespace in its own file.  The shared functions live in artgpu::api.  None of them is in the library's
// dynamic symbol table, and no namespace opening has to say so: every translation unit is compiled with hidden visibility, and
// nothing is exported unless include/artgpu.h declares it.  Each is defined once (the helpers in artgpu_api.hip; every stage in the
// api_<stage>.hip named after its kernel file, the demosaicers in api_demosaic.hip, the shared filters in api_filters.hip, the pixel passes
// in api_pixelops.hip); none is inline.
#pragma once
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <cmath>
#include <cstdio>
#include <cstdarg>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>
#include <algorithm>

#include "../../include/artgpu.h"
#include "kernels.h"
#include "dehaze.h"
#include "textureboost.h"
#include "colorcorrection.h"
#include "smoothing.h"
#include "toneequalizer.h"
#include "filmsim.h"
#include "filmgrain.h"
#include "resize.h"
#include "masks.h"
#include "sharpen.h"
#include "blackwhite.h"
#include "creativegradients.h"
#include "impulse.h"
#include "defringe.h"

struct artgpu_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t aux = nullptr;      // second stream (serial statistics of the AUTOMATIC chroma estimation run beside the decompositions)
    hipEvent_t aux_ev[2] = {nullptr, nullptr};
    // RGB_denoise: the DCT detail recovery of L runs on a side stream beside the chroma blurs / reconstructions
    hipStream_t dn_stream[1] = {nullptr};
    hipEvent_t dn_ev[2] = {nullptr, nullptr};
    const float *gam_tab = nullptr; float gam_key[6] = {};   // RGB_denoise's gamma / inverse-gamma tables in pool[P_GAM]: what they were built from
    // What a batch lane inherits from its parent context (batch_prepare_lanes copies the block as one value on every batch call).  A field
    // belongs here exactly if a frame's result or its reporting must not depend on which lane ran it.  (io_cu_reserve is not one: io_frame sets it
    // per lane; the *_own storage the pipe_* pointers point into stays with the parent.)
    struct Shared {
        // options (artgpu_set_option): test / profiling switches that used to be environment variables
        int opt_sharpen_fused = 1;     // RL deconvolution, stencil regimes -- 1: one kernel per iteration (rl_iter_kernel); 0: DIV, MULT and check_stop as three launches (timing)
        int opt_te_group_thread = 0;   // tone equalizer, the group-of-four rule -- 0: one pixel per lane, the decision from a ballot; 1: one thread per group (tests, timing)
        int opt_te_fuse_upsample = 1;  // tone equalizer -- 1: the last regularising filter's up-sample happens in te_apply; 0: it writes Y, te_apply reads it (tests, timing)
        int opt_lut_lds = 1;           // 0: never the LUT-in-LDS shapes of the pixel passes (tests compare the two)
        int opt_dn_streams = 0;        // 1: the DCT detail recovery of L on a side stream beside the reconstructions of a and b.  The default until round 5, when the
                                       // stage waited on LDS round trips and left the chip half idle; since detail_blocks_kernel lost a fifth of its time (detail.hip) the
                                       // two chains only get in each other's way: one kernel after the other is 0.1 - 0.15 ms per 45 MP frame faster (scripts/r5_ab9.sh)
        int opt_dn_fused = 1;          // ShrinkAllL / ShrinkAllAB -- 0: three kernels per channel (factors, row sums, column sums + update); 2: one kernel per
                                       // channel; 1: one kernel, and one launch for all three channels where nothing has to happen between them
        int opt_dn_detail_plain = 0;   // DCT detail recovery -- 0: trimmed kernels; 1: the kernels before them (what the tests compare against);
                                       // 2: only detail_blocks_kernel plain; 3: only detail_gather_kernel plain (timing of the two halves)
        int opt_dn_mad_fold = 1;       // MadRgb -- 1: from the bins the analysis kernels count while they write the bands; 0: launch_mad's pass over the bands
        int opt_dn_mad_fold_grid = 0;  // > 0: the counting analysis kernels with at most this many workgroups (tests: many steps per workgroup; timing of the grid cap)
        int opt_fg_grid = 0;           // film grain: > 0: the region kernel with at most this many workgroups (tests: a workgroup walks many tiles; timing)
        int opt_dn_debug_stall = -1;   // test hook: band << 16 | strip of the fused shrink pass that never publishes its progress (-1: none)
        long opt_dn_wait_ms = 0;       // how long a strip of the fused shrink pass waits for the strip above before it gives up (0: five seconds)
        int opt_io_direct = -1;        // artgpu_batch_run_io, scanlines into pinned host memory: n > 0: written there by n persistent workgroups (no staging, no copy); 0: staged +
                                       // hipMemcpy; -1 (default): 8 with two lanes, 0 otherwise (io_frame has the measurements)
        int opt_cu_reserve = 0;        // the caller's "cu_reserve": the persistent one-workgroup-per-CU pixel passes launch this many workgroups fewer.  Only
                                       // artgpu_set_option writes it (a batch keeps its own figure in io_cu_reserve; the launchers take cu_reserve_of())
        int opt_amaze_path = 0;        // 0: LDS streaming kernel for full tiles + arena kernel for the rest; 1: arena kernel for every tile
        int opt_amaze_split = 0;       // 1 (with path 1): one launch per phase
        long opt_amaze_zero_mask = 0x81f0;
        int opt_amaze_zero_frame = 16;
        int opt_amaze_poison = -1;     // >= 0: byte pattern the arenas are filled with before the launch
        int opt_roctx = 0;             // 1: roctx ranges named after the reference functions around the entry points (rocprofv3 --marker-trace)
        int opt_amaze_overlap = 1;     // 0: the arena kernel's static tiles behind the stream kernel instead of beside it
        int opt_amaze_grid = 0;        // > 0: at most this many stream workgroups (each owns a CU): with several frames in flight the CUs left over
                                       // take the other frames' bandwidth-bound passes while this frame's issue-bound demosaic runs
        int opt_rcd_rows = 8;          // rows per iteration of the streaming kernel (4 or 8)
        int curve_tail_kind = ARTGPU_CURVE_TAIL_HOST;   // artgpu_set_curve_tail
        double curve_tail_y = 1.0;
        artgpu::ParamCurve curve_tail_pc = {};
        artgpu_progress_fn progress_fn = nullptr;   // artgpu_set_progress_callback
        void *progress_user = nullptr;
        // artgpu_set_pipeline_masks / _color_correction / _smoothing: what the pipe reads (the parent's pipe_*_own hold the memory)
        const artgpu_mask_params *pipe_lc = nullptr, *pipe_tb = nullptr;
        int pipe_nlc = 0, pipe_ntb = 0;
        const artgpu_color_correction_region *pipe_cc = nullptr;
        const artgpu_mask_params *pipe_cc_masks = nullptr;
        int pipe_ncc = 0;
        const artgpu_smoothing_region *pipe_sm = nullptr;
        const artgpu_mask_params *pipe_sm_masks = nullptr;
        int pipe_nsm = 0;
        int pipe_te_on = 0;            // artgpu_set_pipeline_tone_equalizer: a copy by value
        artgpu_tone_equalizer_params pipe_te = {};
        const artgpu_clut *pipe_fs = nullptr;      // artgpu_set_pipeline_film_simulation: the handle (the parent's pipe_fs_own holds the reference),
        artgpu_film_simulation_params pipe_fs_par = {};   // a copy of the parameters, and the position
        int pipe_fs_after = 0;
        int pipe_fg_on = 0;            // artgpu_set_pipeline_film_grain: a copy by value
        artgpu_film_grain_params pipe_fg = {};
        int pipe_rs_on = 0;            // artgpu_set_pipeline_resize: a copy by value
        artgpu_resize_params pipe_rs = {};
        int pipe_cg_on = 0;            // artgpu_set_pipeline_creative_gradients: a copy by value
        artgpu_creative_gradients_params pipe_cg = {};
        int pipe_sl_on = 0;            // artgpu_set_pipeline_soft_light: a copy by value
        artgpu_soft_light_params pipe_sl = {};
        int pipe_bw_on = 0;            // artgpu_set_pipeline_black_and_white: a copy by value; its ulut / vlut point into the parent's pipe_bw_tabs
        artgpu_black_and_white_params pipe_bw = {};
        int pipe_imp_on = 0, pipe_df_on = 0;   // artgpu_set_pipeline_impulse_defringe: copies by value; the hue curve points into the parent's pipe_df_curve
        artgpu_impulse_denoise_params pipe_imp = {};
        artgpu_defringe_params pipe_df = {};
    } shared;
    float *sh_host = nullptr;      // pinned: the auto radius' maximum ratio on its way to the host (pipeline: launched early, waited for where it is used)
    hipEvent_t sh_ev = nullptr;
    // artgpu_set_pipeline_masks: deep copies (entries, curves, area descriptors); batch lanes point at their parent's
    struct PipeMasks { std::vector<artgpu_mask_params> m; std::vector<std::vector<double>> curves; std::vector<artgpu_plane> areas; } pipe_lc_own, pipe_tb_own;
    // artgpu_set_pipeline_color_correction / artgpu_set_pipeline_smoothing: the regions, their mask planes' descriptors and the mask parameters
    template <typename Region> struct PipeRegions { std::vector<Region> regs; std::vector<artgpu_plane> planes; PipeMasks masks; };
    PipeRegions<artgpu_color_correction_region> pipe_cc_own;
    PipeRegions<artgpu_smoothing_region> pipe_sm_own;
    std::vector<double> pipe_df_curve;     // artgpu_set_pipeline_impulse_defringe: defringe's hue curve (batch lanes point at their parent's)
    std::vector<float> pipe_bw_tabs;       // artgpu_set_pipeline_black_and_white: the cast's two tables (batch lanes point at their parent's)
    artgpu_clut *pipe_fs_own = nullptr;    // artgpu_set_pipeline_film_simulation: the reference this context holds (batch lanes hold none)
    std::string err;
    int *fs_diag = nullptr;        // pinned host words the fused shrink pass writes before it traps (which strip waited for which): see fail()
    long long batch_px = 0;       // artgpu_batch_run: pixels of the largest frame this context's scratch was grown for since the last trim
    // RGB_denoise's last call: the fold's flag block (96 words in the P_MAD slot behind the 96 medians) and which of its words the call's launch_mad_fold launches wrote (first, count)
    const int *dn_fold_flags = nullptr; int dn_fold_ranges[8][2] = {}; int dn_fold_nranges = 0;
    int dn_form = -1, dn_form_streak = 0;   // RGB_denoise: the shrink passes' form of the last call (1 fused / 0 three kernels) and how many calls in a row used it
    // per-workgroup work arenas (demosaic)
    float *arena = nullptr;
    size_t arena_bytes = 0;
    // staging for host-pointer calls: one CFA plane + three output planes
    static constexpr int NSTAGE = 8;
    float *stage[NSTAGE] = {};
    size_t stage_bytes[NSTAGE] = {};
    // grow-only scratch pool for the denoise path (planes, decompositions, shrink buffers)
    static constexpr int NPOOL = 104;
    float *pool[NPOOL] = {};
    size_t pool_bytes[NPOOL] = {};
    // artgpu_batch_run lanes: sibling contexts (own stream, arena, pools) that take every lanes-th frame on their own host thread
    std::vector<artgpu_ctx *> lanes;
    int batch_lanes = 1;
    int frames_in_flight = 1;      // set by artgpu_batch_run on itself and its lanes while a batch with L > 1 lanes runs: the demosaic then takes 5/8 of the CUs (option amaze_grid)
    bool owns_stream = false;
    // artgpu_batch_run_io: a frame's upload and download run on streams of their own beside the kernels on `stream`.  Events, by staging slot
    // (the parity of the frame's turn on this lane): [0,1] uploaded, [2,3] the upload slot has been read, [4,5] scanlines written, [6,7] downloaded
    hipStream_t io_up = nullptr, io_down = nullptr;
    hipEvent_t io_ev[8] = {};
    int *io_host = nullptr;        // pinned, 8 words per frame of the lane: channel maxima (bit patterns) x 3, -, rgb2out's count of unsupported values
    int io_host_cap = 0;
    int io_cu_reserve = 0;         // set by io_frame while a batch's downloads run as a kernel of a few workgroups: the persistent one-workgroup-per-CU pixel passes leave those CUs alone
    // (what artgpu_improc_denoise_fused fuses into the denoise tool's pixel passes is not state of the context: it travels as a DnFusion argument)
    float *bbox = nullptr; // AMaZE: per-tile nyquist bounding boxes
    size_t bbox_bytes = 0;
    // AMaZE v2: tile lists on the device (ints).  [stream tiles | arena-tile template: count, tiles | working copy: count, tiles + room
    // for every streamed tile the stream kernel hands back]
    float *amz_lists = nullptr;
    size_t amz_lists_bytes = 0;
    int amz_w = 0, amz_h = 0, amz_nstream = 0, amz_narena = 0, amz_mode = -1;
    int num_cus = 0;
    hipStream_t amz_side = nullptr;
    hipEvent_t amz_ev[2] = {nullptr, nullptr};
    int *rcd_counter = nullptr;    // RCD streaming kernel: tile counter
    float *lut = nullptr; // 65536-entry tone LUT on the device
    size_t lut_bytes = 0;
    std::vector<float> lut_host;           // what ctx->lut holds (a curve that comes back unchanged is not uploaded again)
    std::vector<float> ncurve_host;        // likewise the 501-entry chroma noise curve behind the cachef table
    char *tab_ring = nullptr;              // pinned staging ring of h2d_table (caller look-up tables)
    size_t tab_ring_bytes = 0, tab_ring_off = 0;
    bool tab_ring_busy = false;
    hipEvent_t tab_ev = nullptr;
    std::vector<float> rgbcurve_host[3];   // likewise the three rgbCurves tables (P_RGBCURVES: a slot nothing else writes)
    std::vector<float> te_lut_host;        // the tone equalizer's correction table (65536 entries), the bands it was built from, and where in
    int te_lut_bands[5] = {};              // P_TE_LUT (a slot nothing else writes) it was uploaded to: rebuilt when the bands change, uploaded
    const float *te_lut_dev = nullptr;     // again when the slot moved (artgpu_trim_scratch)
    // the resampler's tables (api_resize.hip): what the host copy was built for, the copy, and where in P_RS_TAB (a slot nothing else writes) it
    // was uploaded to: rebuilt when the key changes, uploaded again when the slot moved
    int rs_key[4] = {}; float rs_key_scale = 0.f;
    int rs_support = 0, rs_tile_w = 0;
    std::vector<int> rs_host;
    const float *rs_dev = nullptr;
    // soft light's table (api_softlight.hip): the strength the host copy was built for, the copy, and where in P_SL_LUT (a slot nothing else
    // writes) it was uploaded to: rebuilt when the strength changes, uploaded again when the slot moved
    int sl_lut_strength = -1;
    std::vector<float> sl_lut_host;
    const float *sl_lut_dev = nullptr;
    // black-and-white's tables (api_blackwhite.hip) in P_BW_TAB (a slot nothing else writes): [gamma r | g | b | ulut | vlut], 65536 floats each.
    // The host copy of each, what the gamma tables were built for, and where they were uploaded to
    std::vector<float> bw_tab_host[5];
    float bw_gam_key[3] = {};
    const float *bw_tab_dev = nullptr;
    // timing
    bool timing = false;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    artgpu_timings last = {0.f, 0.f, 0.f};
};

namespace artgpu { namespace api {

// ---------------------------------------------------------------------------------------------
// context: errors, staging of host planes, the scratch pool
// ---------------------------------------------------------------------------------------------
int fail(artgpu_ctx *ctx, int code, const char *fmt, ...);

#define HIPCHK(ctx, call)                                                                        \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail(ctx, ARTGPU_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// A call that puts work on a side stream has to leave with the context's stream behind that work on EVERY path: an error return in between
// would otherwise leave the side stream running on pool buffers the next call hands out again.  Armed when the fork happens, disarmed by the
// regular join (an event wait, no host blocking); on any other exit the destructor drains the side stream.
struct SideStreamJoin {
    hipStream_t side = nullptr;
    void arm(hipStream_t s) { side = s; }
    void disarm() { side = nullptr; }
    ~SideStreamJoin() { if (side) (void)hipStreamSynchronize(side); }
};

int ensure(artgpu_ctx *ctx, float **buf, size_t *cur, size_t need);
int h2d_table(artgpu_ctx *ctx, void *dst, const void *src, size_t bytes);
bool plane_ok(const artgpu_plane *p);

struct DevImage {
    const float *raw; size_t raw_stride;
    float *r, *g, *b; size_t out_stride;
    bool staged;
};
int bind_images(artgpu_ctx *ctx, const artgpu_plane *raw, const artgpu_rgb *out, DevImage *d);
int unbind_images(artgpu_ctx *ctx, artgpu_rgb *out, const DevImage *d);

// Generic RGB image binding: device planes are used in place, host planes are staged through
// ctx->stage[slot..slot+2] (copy_in: H2D now; the D2H happens in unbind_rgb).
struct DevRGB {
    float *p[3];
    size_t stride; // floats
    int w, h;
    bool staged;
};
artgpu_plane mk_dev_plane(float *p, int w, int h);
artgpu_rgb mk_dev_rgb(float *const p[3], int w, int h, size_t stride);
int bind_rgb(artgpu_ctx *ctx, const artgpu_rgb *img, int slot, bool copy_in, DevRGB *d, const char *what);
int unbind_rgb(artgpu_ctx *ctx, artgpu_rgb *img, const DevRGB *d);

enum { P_L = 0, P_A, P_B, P_LBANDS, P_LLOW0, P_LLOW1, P_CBANDS, P_CLOW0, P_CLOW1, P_SF, P_TMP, P_HISTO, P_MAD, P_GAM, P_CCALC, P_LIN, P_BLOCKS, P_DTAB, P_CCMAP, P_CACHEF, P_PQ, P_XCBRT, P_GAUSS64, P_DMASK, P_LABTABS, P_PIPE_R, P_PIPE_G, P_PIPE_B, P_DNINFO, P_BATCH, P_DCTTAB, P_CBANDS2, P_CLOW0_2, P_CLOW1_2, P_SF_A, P_SF_B, P_HISTO_A, P_HISTO_B, P_RGBCURVES, P_FUSED, P_LBANDS2,
       P_IO_IN0, P_IO_IN1, P_IO_CFA, P_IO_IMG0, P_IO_IMG1, P_IO_IMG2, P_IO_IMG3, P_IO_IMG4, P_IO_IMG5, P_IO_OUT0, P_IO_OUT1, P_IO_FLAGS,      // artgpu_batch_run_io: staging slots, the CFA plane, the working image, the frames' flag words
       P_CA_HALF, P_CA_BLK, P_CA_GUARD, P_CA_RAW,                                                                       // artgpu_raw_ca_correct
       P_LC_BANDS, P_LC_LOW0, P_LC_LOW1, P_LC_NEW, P_LC_STATS, P_LC_MASK, P_LC_L,                                       // artgpu_local_contrast
       P_DH_STATE, P_DH_THUMB, P_DH_LOW, P_DH_TMP, P_DH_T, P_DH_DARK,                                                   // artgpu_dehaze
       P_SH_PLANES, P_SH_BYTES, P_SH_STATE,                                                                             // artgpu_sharpening
       P_TB_PLANES, P_TB_LOW, P_TB_TMP, P_TB_STATE, P_TB_MASK, P_TB_Y,                                                  // artgpu_texture_boost
       P_MK_WORK, P_MK_TAB, P_MK_CTHR, P_MK_AREA, P_MK_OUT,                                                             // artgpu_generate_masks
       P_CC_MASK, P_CC_OOR, P_CC_GEN,                                                                                   // artgpu_color_correction
       P_SM_PLANES, P_SM_MASK, P_SM_BOX, P_SM_GEN,                                                                      // artgpu_smoothing
       P_TE_PLANES, P_TE_LUT,                                                                                           // artgpu_tone_equalizer
       P_RS_TAB, P_RS_IMG0, P_RS_IMG1, P_RS_IMG2,                                                                       // artgpu_resize_lanczos: the tables; the pipe's full-size working image
       P_FG_WORK, P_FG_TAB, P_FG_IDX,                                                                                   // artgpu_film_grain: the planes a region writes, its tables; artgpu_grain_indices
       P_SL_LUT, P_BW_TAB,                                                                                              // artgpu_soft_light's table; artgpu_black_and_white's gamma and cast tables
       P_MADPART,                                                                                                       // RGB_denoise: the counting analysis kernels' bins (launch_mad_fold)
       P_DF_STATE,                                                                                                      // artgpu_defringe: state, hue curve, the sum's partials (its planes: P_SH_PLANES)
       P_NSLOTS };
static_assert(P_NSLOTS <= artgpu_ctx::NPOOL, "grow artgpu_ctx::pool");
int pool_get(artgpu_ctx *ctx, int slot, size_t bytes, float **out);
int plane_to_pool(artgpu_ctx *ctx, const artgpu_plane *pl, int slot, float **out);
int pool_to_plane(artgpu_ctx *ctx, const float *src, artgpu_plane *pl);
// read-only planes (masks, area planes) as (pointer, row stride in floats): device planes in place, each distinct host plane staged once into `slot`
int bind_plane(artgpu_ctx *ctx, const artgpu_plane *pl, int slot, const float **p, size_t *stride);
int bind_planes(artgpu_ctx *ctx, int W, int H, const artgpu_plane *const *planes, int n, int slot, const float **p, size_t *stride);

#ifndef ARTGPU_MAX_TILE_WG
#define ARTGPU_MAX_TILE_WG 8192
#endif
constexpr int MAX_TILE_WORKGROUPS = ARTGPU_MAX_TILE_WG;

int check_async_faults(artgpu_ctx *ctx);
// CUs the persistent one-workgroup-per-CU passes of this context leave alone: the caller's option or what the batch in flight needs, whichever is more
inline int cu_reserve_of(const artgpu_ctx *ctx) { return ctx->shared.opt_cu_reserve > ctx->io_cu_reserve ? ctx->shared.opt_cu_reserve : ctx->io_cu_reserve; }

// Host-side milestones of an entry point: the reference's ProgressListener (rtengine.h:165; amaze_demosaic_RT.cc:1567-1580 reports
// per-tile fractions, the device path reports 0 when the stage's work starts being queued and 1 when the entry point returns) and,
// with the "roctx" option, a roctx range named after the reference function so that profiles read like the reference's call tree.
struct StageScope {
    artgpu_ctx *ctx;
    const char *name;
    bool range;
    typedef int (*push_fn)(const char *);
    typedef int (*pop_fn)();
    static push_fn &push();
    static pop_fn &pop();
    StageScope(artgpu_ctx *c, const char *n);
    ~StageScope();
};

// ---------------------------------------------------------------------------------------------
// raw CA correction
// ---------------------------------------------------------------------------------------------
bool ca_cfa(uint32_t filters, unsigned *cfa);
int ca_correct_dev(artgpu_ctx *ctx, float *raw, size_t stride, int W, int H, unsigned cfa, const artgpu_ca_params *p, double *fit_out);

// ---------------------------------------------------------------------------------------------
// local contrast
// ---------------------------------------------------------------------------------------------
int local_contrast_check(artgpu_ctx *ctx, int w, int h, const artgpu_local_contrast_region *regions, int nregions, double scale, const char *who);
int local_contrast_dev(artgpu_ctx *ctx, float *L, size_t stride, int w, int h, const artgpu_local_contrast_region *regions, int nregions,
                       artgpu_local_contrast_info *info);

// ---------------------------------------------------------------------------------------------
// dehaze
// ---------------------------------------------------------------------------------------------
// the sizes the call derives from W, H and scale before it touches anything
struct DehazePlan {
    int ww, hh, brad;              // thumbnail, subtract_black's blur radius (L254-257, L268)
    int w1, h1, rad1;              // extract_channels' statistics grid and box radius
    int patch, npx, npy;           // L396
    int w2, h2, rad2;              // the transmission map's guided filter (L438-445)
};
int dehaze_check(artgpu_ctx *ctx, int W, int H, const artgpu_dehaze_params *p, const double *ws, double scale, const char *who, DehazePlan *pl);
int dehaze_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const artgpu_dehaze_params *p, const double ws[9],
               const DehazePlan &pl, artgpu_dehaze_info *info);

// ---------------------------------------------------------------------------------------------
// texture boost
// ---------------------------------------------------------------------------------------------
// what one texture_boost call derives from its region, the plane's size and scale before it touches anything (iptextureboost.cc:39-63)
struct TbPlan {
    int radius, isguided, rescaled, w, h, K;       // w x h: the size the call works at; K: the gaussian's size (0 when guided)
    float strength, strength2;
    float coef[TB_MAX_K * TB_MAX_K];
    int w1, h1, rad1;                              // guidedFilter(mid, mid, mid, radius, 0.001f)'s statistics grid and box radius (guided only)
    int w2, h2, rad2;                              // guidedFilter(mid, mid, base, radius * 4, 0.0001f)'s
};
int tb_check(artgpu_ctx *ctx, int W, int H, const artgpu_texture_boost_region *regions, int nregions, const double *ws, double scale, int high_detail,
             const char *who, std::vector<TbPlan> *plans);
int texture_boost_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const artgpu_texture_boost_region *regions, int nregions,
                      const double ws[9], const std::vector<TbPlan> &plans, int to_rgb, artgpu_texture_boost_info *info, int already_yuv = 0);

// ---------------------------------------------------------------------------------------------
// region masks
// ---------------------------------------------------------------------------------------------
struct MkRegionPlan {
    MkCurve curve[3];                 // offsets inside the region's own table
    std::vector<double> tab;
    float ldetail;
    int blurred, r1, r2;
    int cthr, cthr_neg, cw, ch; float cthr_thresh, cthr_blur;
    float post_p; int smooth, smooth_r; float fillval;
    int inverted, has_opacity; float opacity;
};
struct MkPlan {
    int W, H, lab, want_L, want_ab, has_mask, need_ll, need_guide, ll_r_small, ll_r;
    std::vector<MkRegionPlan> reg;
};
int mk_plan(artgpu_ctx *ctx, int W, int H, int mode, const double *ws, const artgpu_mask_params *masks, int n, int full_w, int full_h, double scale,
            bool want_L, bool want_ab, const char *who, MkPlan *pl, artgpu_masks_info *info);
int masks_dev(artgpu_ctx *ctx, float *const img[3], size_t stride, const double *ws, const artgpu_mask_params *masks, const MkPlan &pl,
              float *Lout, float *about);

// ---------------------------------------------------------------------------------------------
// colour correction
// ---------------------------------------------------------------------------------------------
// what a call derives on the host before it touches anything (L88-141, L280-414), and every reason not to run
struct CcPlan { std::vector<CcRegion> regs; float ws[9], iws[9], fR, fG, fB; bool any_jz; };
int cc_check(artgpu_ctx *ctx, int W, int H, const artgpu_color_correction_region *regions, int nregions, const double *ws, const double *iws, bool read_masks,
             const char *who, CcPlan *pl);
int color_correction_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const artgpu_color_correction_region *regions,
                         const CcPlan &pl, int from_yuv, int to_rgb, artgpu_color_correction_info *info);

// ---------------------------------------------------------------------------------------------
// smoothing
// ---------------------------------------------------------------------------------------------
// what a call derives per region on the host before any kernel writes the image (ipsmoothing.cc:943-980, L348, L1040)
struct SmRegionPlan {
    int mode, channel, iterations, r, nlstrength, nldetail;
    float epsilon;
    int x0, y0, x1, y1, cropped, ww, hh;       // the box (max exclusive) and the working size
    int sub, w, h, rad;                        // GUIDED: subsampling, statistics grid, f_mean's radius
    int skipped;
};
int sm_check(artgpu_ctx *ctx, int W, int H, const artgpu_smoothing_region *regions, int nregions, const double *ws, double scale, bool read_masks, const char *who);
bool sm_working_area(int W, int H, const int *box, SmRegionPlan *pl);       // the crop rule alone (what film grain's NOISE regions share with the modes above)
int sm_plan_region(artgpu_ctx *ctx, int W, int H, const artgpu_smoothing_region &r, const int *box, double scale, const char *who, int i, SmRegionPlan *pl);
// the regions' blend planes on the device and the box of each (find_region): see the definition
int sm_mask_boxes(artgpu_ctx *ctx, int W, int H, const artgpu_plane *const *masks, int n, std::vector<const float *> *mp, std::vector<size_t> *ms, std::vector<int> *boxes);
int smoothing_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const artgpu_smoothing_region *regions, int n, const double *ws, double scale,
                  artgpu_smoothing_info *info, const char *who);

// ---------------------------------------------------------------------------------------------
// guided filter (shared by the tools that call rtengine::guidedFilter)
// ---------------------------------------------------------------------------------------------
int gf_subsampling(int w, int h, int r);
// one call's statistics grid: subsampling (calculate_subsampling unless the caller names one), size, f_mean's box radius (0 for an empty grid)
struct GfGrid { int sub, w, h, rad; };
GfGrid gf_grid(int W, int H, int r, int subsampling = 0);
// the plain box blur f_mean runs (boxblur.h:318), `count` planes n floats apart, in place through `tmp`; nothing for rad == 0
int box_blur_planes(artgpu_ctx *ctx, float *planes, float *tmp, int count, size_t n, int w, int h, int rad);
int guided_filter_stats(artgpu_ctx *ctx, const float *guide, const float *src, int W, int H, int r, float epsilon, int subsampling, const char *who, GuidedArgs *g);
int guided_filter_dev(artgpu_ctx *ctx, const float *guide, const float *src, float *q, size_t q_stride, int W, int H, int r, float epsilon, int subsampling,
                      const char *who);

// ---------------------------------------------------------------------------------------------
// what a stage exposes to its sibling stages, by the file that defines it
// ---------------------------------------------------------------------------------------------
// artgpu_api.hip
// A table of constants in a pool slot of its own, built on the host by `fill` (which gets `nfloats` zeroed floats) and uploaded once per context
int const_table_dev(artgpu_ctx *ctx, int slot, size_t nfloats, void (*fill)(float *), const char *what, float **out);
// Color::cachef / cachefy / denoiseGammaTab / denoiseIGammaTab, built on the host like the reference's (color.cc:202-292), in P_LABTABS
int lab_tabs_dev(artgpu_ctx *ctx, float **tabs_out);

// api_pixelops.hip: each *_dev is one launch on ctx->stream; the *_check beside it is every reason not to run, and launches nothing
// RawImageSource::getImage + the matrix branch of convertColorSpace: `dst` from the window of `src` at (sx1, sy1), every skip-th pixel
int get_image_dev(artgpu_ctx *ctx, const DevRGB &src, const DevRGB &dst, int sx1, int sy1, int skip, const float mul[3], int do_clip, const double *mat);
int exposure_dev(artgpu_ctx *ctx, const DevRGB &d, float exp_scale, float black);
int tone_curve_check(artgpu_ctx *ctx, int mode, float whitept);
int tone_curve_dev(artgpu_ctx *ctx, const DevRGB &d, const float *lut65536, float whitept, int filmlike_clip);
int tone_neutral_check(artgpu_ctx *ctx, const float *lut65536, float whitecoeff);
int tone_neutral_dev(artgpu_ctx *ctx, const DevRGB &d, const float *lut65536, float whitecoeff, const artgpu_neutral_state *st);
// Imagefloat::setMode(LAB) / (RGB) on device planes
int lab_switch_dev(artgpu_ctx *ctx, const DevRGB &d, const double m[9], bool to_lab);
// Imagefloat::setMode(YUV) on device planes in LAB mode (lab_to_yuv)
int lab_to_yuv_dev(artgpu_ctx *ctx, const DevRGB &d, const double iws[9]);
// scaleColors' ScaleArgs but for the buffers: the size, the 6x6 colour map (xtrans, or the Bayer word `filters` when it is null; a fourth
// colour is refused under `who`), black levels and multipliers
int scale_args_fill(artgpu_ctx *ctx, int w, int h, int src_is_u16, uint32_t filters, const int32_t *xtrans, const float cblacksom[4], const float scale_mul[4],
                    const char *who, ScaleArgs *a);

// api_demosaic.hip: the checks are what the entry points refuse about method, gain, colour map and size (raw_stride: the CFA plane's row in
// floats as bind_images will produce it); the *_dev run on a bound image and keep the timing events beside the launches they time
int demosaic_bayer_check(artgpu_ctx *ctx, int method, uint32_t filters, double initial_gain, int W, int H);
int demosaic_bayer_dev(artgpu_ctx *ctx, const DevImage &d, int W, int H, int method, uint32_t filters, double initial_gain, int border);
int demosaic_xtrans_check(artgpu_ctx *ctx, int passes, const int32_t xtrans[36], int W, int H, size_t raw_stride);
int demosaic_xtrans_dev(artgpu_ctx *ctx, const DevImage &d, int W, int H, int passes, int use_cielab, const int32_t xtrans[36], const float rgb_cam[12]);

// api_denoise.hip
// denoiseComputeParams' nine-crop layout on W x H planes behind `border` (the 100 px rule); the estimate itself, which ends in the host wait its result needs
int dn_compute_params_check(artgpu_ctx *ctx, int W, int H, int border);
int dn_compute_params_dev(artgpu_ctx *ctx, const DevRGB &src, int border, const float mul[3], int do_clip, const double cam_to_work[9], const double ws[9],
                          double chrominance_auto_factor, artgpu_denoise_info_store *store, artgpu_denoise_params *dn);
// every reason ImProcFunctions::denoise has not to run on a w x h image: RGB_denoise's parameters and size, and with smoothing_enabled the
// limits of the guided chroma smoothing and of NL-means behind it
int denoise_tool_check(artgpu_ctx *ctx, int w, int h, const artgpu_denoise_tool_params *p, const double *iws, double scale);
// the tool on the device image `d`, after denoise_tool_check.  fu: what artgpu_improc_denoise_fused may fuse of the stages around it (null: nothing;
// its `demosaiced` is not read: `dem` is those planes, bound, or null); fuse_ok: the caller's planes were on the device (a staged copy keeps the
// separate passes it always had)
int improc_denoise_dev(artgpu_ctx *ctx, const DevRGB &d, const DevRGB *dem, const artgpu_denoise_fusion *fu, bool fuse_ok, const artgpu_denoise_tool_params *p,
                       const double ws[9], const double *iws, double ecomp, double scale, const double *calclum_mat, const float *noise_c_curve, uint32_t flags);

// api_wavelet.hip
int wavelet_skip(int level);
// one plane's decomposition in pool buffers the caller has fetched (RGB_denoise, local contrast); st: the context's stream unless named
struct DevDecomp {
    float *bands, *low[2];
    int cur, nlevels, w, h, w2, h2;
    size_t n;
    int *cnt;                   // non-null: decompose with the counting kernels -- MadRgb's low bins of this channel's bands, [3 * nlevels][MAD_FOLD_NB]
    int g0, g1;                 // ... their grids
    float *band(int l, int dir) const { return bands + ((size_t)l * 3 + (dir - 1)) * n; }
};
int decompose_dev(artgpu_ctx *ctx, DevDecomp &d, const float *src, hipStream_t st = nullptr, size_t src_stride = 0);
int reconstruct_dev(artgpu_ctx *ctx, DevDecomp &d, float *dst, hipStream_t st = nullptr);

// api_filters.hip (with the guided filter above)
int gaussian_dev(artgpu_ctx *ctx, float *img, float *tmp, int W, int H, double sigma);
int detail_mask_dev(artgpu_ctx *ctx, const float *src, size_t src_stride, float *mask, int W, int H,
                    float scaling, float threshold, float ceiling, float factor, float blur, float *scratch /* >= W*H + 2*(W/4)*(H/4) */);
// denoise::NLMeans (nlmeans.cc:44-320) on a contiguous device plane (rows of W floats), in place; enqueued on ctx->stream.  The caller has checked
// strength != 0, nlm_check and scale >= 1.  Scratch: P_TMP, P_LIN, P_BLOCKS
int nlm_check(artgpu_ctx *ctx, int W, int H);                 // W, H >= 32, (W + 14) * (H + 14) < 2^30
int nlm_plane_dev(artgpu_ctx *ctx, float *work, int W, int H, float normcoeff, int strength, int detail_thresh, float scale);
// ... on any plane (host, or device rows with padding: through a contiguous working copy in P_SF)
int nlm_dev(artgpu_ctx *ctx, artgpu_plane *img, float normcoeff, int strength, int detail_thresh, float scale);
// denoise::denoiseGuidedSmoothing (ipsmoothing.cc:875) for a radius that is not 0 and scale >= 1: the radius / scale combinations the device path has
// not, and the filter on the device image.  Scratch: P_SF, P_TMP, P_LIN
int denoise_guided_smoothing_check(artgpu_ctx *ctx, int W, int H, int guided_chroma_radius, double scale);
int denoise_guided_smoothing_dev(artgpu_ctx *ctx, const DevRGB &d, const double ws[9], int guided_chroma_radius, double scale);

// api_colorcorrection.hip
// the PQ tables of Color::init (P_PQ: forward, inverse, then the NEUTRAL curve's four hue anchors, which belong to the tables' lifetime)
int pq_tables_dev(artgpu_ctx *ctx, float **out);

// ---------------------------------------------------------------------------------------------
// tone equalizer
// ---------------------------------------------------------------------------------------------
// what a call derives on the host before any kernel runs: artgpu_tone_equalizer_info is the plan (filters, radii, grids' subsampling, box radii)
int te_check(artgpu_ctx *ctx, int W, int H, const artgpu_tone_equalizer_params *p, const double *ws, double scale, const char *who, artgpu_tone_equalizer_info *pl);
int tone_equalizer_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const artgpu_tone_equalizer_params *p, const double ws[9],
                       const artgpu_tone_equalizer_info &pl, const char *who);

// ---------------------------------------------------------------------------------------------
// film simulation
// ---------------------------------------------------------------------------------------------
// every reason not to run (a bad handle, another device's, a strength that is not finite): nothing is launched
int fs_check(artgpu_ctx *ctx, const artgpu_clut *clut, const artgpu_film_simulation_params *p, const char *who);
// the tool on device planes (rows of `stride` floats) in RGB mode, after fs_check; enqueued on ctx->stream
int film_simulation_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const artgpu_clut *clut, const artgpu_film_simulation_params *p);
void clut_release(artgpu_clut *clut);      // drops one reference; the last one frees the device copy

// ---------------------------------------------------------------------------------------------
// film grain
// ---------------------------------------------------------------------------------------------
// what filmGrain derives from its parameters (ipgrain.cc:40-69) and add_noise from each region (ipsmoothing.cc:572-597), before anything runs
struct FgPlan { artgpu_film_grain_info info; double scale; };
// every reason not to run; nothing is uploaded or launched
int fg_check(artgpu_ctx *ctx, int W, int H, const artgpu_film_grain_params *p, const double *ws, double scale, int output_pipeline, const char *who, FgPlan *pl);
// the tool on device planes (rows of `stride` floats) in RGB mode, after fg_check; enqueued on ctx->stream
int film_grain_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const double ws[9], const FgPlan &pl);

// ---------------------------------------------------------------------------------------------
// creative gradients, soft light, black-and-white
// ---------------------------------------------------------------------------------------------
// every reason not to run, and the derived parameters of the filters that do (apply_gradient / apply_pcvignette; both 0: nothing runs)
int cg_check(artgpu_ctx *ctx, int W, int H, const artgpu_creative_gradients_params *p, const char *who, CgDerived *d);
// the tool on device planes in RGB mode, after cg_check; one launch on ctx->stream
int creative_gradients_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const CgDerived &d);
// every reason not to run, and what the call derives on the host; nothing is uploaded or launched.  on == 0: the tool returns at once
struct SlPlan { int on, strength; };
int sl_check(artgpu_ctx *ctx, const artgpu_soft_light_params *p, const char *who, SlPlan *pl);
// the tool on a device image in RGB mode, after sl_check; one launch on ctx->stream
int soft_light_dev(artgpu_ctx *ctx, const DevRGB &d, const SlPlan &pl);
struct BwPlan { int on, hasgamma; BwMixer mix; float gam[3]; const float *ulut, *vlut; };
int bw_check(artgpu_ctx *ctx, const artgpu_black_and_white_params *p, const double *ws, const char *who, BwPlan *pl);
// the tool on device planes in RGB mode, after bw_check; one launch on ctx->stream.  to_rgb: with a cast, leave in RGB mode (else YUV)
int black_and_white_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const double *ws, const BwPlan &pl, int to_rgb);

// ---------------------------------------------------------------------------------------------
// resize
// ---------------------------------------------------------------------------------------------
// every reason not to run, and the tables (built on the host and kept by the context; nothing is uploaded or launched)
int rs_check(artgpu_ctx *ctx, int sW, int sH, int dW, int dH, float scale, const char *who);
// ImProcFunctions::Lanczos on device planes, after rs_check with the same sizes and scale; enqueued on ctx->stream.  m_in / m_out: ws / iws of the
// mode switches in front (on src, in place) and behind (on dst), or null for none
int resize_dev(artgpu_ctx *ctx, const DevRGB &src, const DevRGB &dst, float scale, const double *m_in, const double *m_out);
// the pipe's decision (simpleprocess.cc:402-407): does a frame of w x h leave at another size, and which
bool pipeline_resize(const artgpu_ctx *ctx, int w, int h, int *imw, int *imh, float *scale);

// ---------------------------------------------------------------------------------------------
// capture sharpening
// ---------------------------------------------------------------------------------------------
// the stage's full-size planes in pool slot P_SH_PLANES; SHP_EST_A .. SHP_GTMP are what one deconvolution works in
enum { SHP_Y = 0, SHP_BLEND, SHP_YY, SHP_EST_A, SHP_EST_B, SHP_RATIO, SHP_OUT, SHP_GTMP, SHP_YY2, SHP_NPLANES };
// what the call derives from its parameters before it touches anything
struct SharpenPlan {
    int early;                     // artgpu_sharpening_info::early_out of doSharpening's own tests (L717)
    float contrast, blur_radius, amount, delta;
    double sigma;
    int boost;
};
int sharpen_check(artgpu_ctx *ctx, int W, int H, const artgpu_sharpening_params *p, double scale, const char *who, SharpenPlan *pl);
int sharpen_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const artgpu_sharpening_params *p, const double ws[9],
                const SharpenPlan &pl, artgpu_sharpening_info *info);
int plane_into(artgpu_ctx *ctx, const artgpu_plane *pl, float *dst);
int auto_radius_dev(artgpu_ctx *ctx, const float *raw, size_t stride, int W, int H, uint32_t filters, float lower, float upper, float **result);
float auto_radius_of(float maxRatio);

// ---------------------------------------------------------------------------------------------
// impulse noise reduction, defringe
// ---------------------------------------------------------------------------------------------
// what impulsedenoise derives from its parameters (impulse_denoise.cc:182-187, rt_algo.cc:511-517); early: artgpu_impulse_denoise_info::early_out
struct ImpPlan { int early; float thresh, sigma, impthr; };
ImpPlan imp_plan(int W, int H, const artgpu_impulse_denoise_params *p, double scale);
// the tool on a device image, enqueued on ctx->stream; already_lab: the tool ahead left the image in LAB mode (setMode(LAB) does nothing);
// to_rgb: setMode(RGB) with iws on top.  The host waits only to fill `info`
int impulse_denoise_dev(artgpu_ctx *ctx, const DevRGB &d, const ImpPlan &pl, const double ws[9], const double *iws, int already_lab, int to_rgb,
                        artgpu_impulse_denoise_info *info);
// what defringe derives before it touches anything (PF_correct_RT.cc:47-50, 130, 212-216; gauss.cc:1437-1461), and every reason not to run
struct DfPlan {
    int early, halfwin, blur, curve_n, thresh;     // curve_n: points of the polyline; 0: no curve; -1: FCT_Empty
    double radius;
    float c0, c1, c2, b0, b1;                      // DF_BLUR_3X3
    std::vector<double> tab;                       // poly_x, poly_y, dyByDx
};
int df_plan(artgpu_ctx *ctx, int W, int H, const artgpu_defringe_params *p, double scale, const char *who, DfPlan *pl);
int defringe_dev(artgpu_ctx *ctx, const DevRGB &d, const DfPlan &pl, const double ws[9], const double *iws, int already_lab, int to_rgb,
                 artgpu_defringe_info *info);

// ---------------------------------------------------------------------------------------------
// api_pipeline.hip: what io_frame (api_batch.hip) takes from the frame driver
// ---------------------------------------------------------------------------------------------
bool pipeline_ca(const artgpu_pipeline_params *p);
int pipeline_ca_dev(artgpu_ctx *ctx, float *raw, size_t stride, int W, int H, const artgpu_pipeline_params *p);
int pipeline_run_impl(artgpu_ctx *ctx, const artgpu_plane *raw_in, const artgpu_pipeline_params *p, artgpu_rgb *out, bool do_ca);

} } // namespace artgpu::api
