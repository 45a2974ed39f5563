// art_amd/csrc/api_denoise.hip -- the denoiser behind the C ABI: denoise::RGB_denoise (FTblockDN.cc; the plan, the pool buffers, the chroma
// and luma chains, the DCT detail recovery) and around it the tool, ImProcFunctions::denoise (ipdenoise.cc; the chroma noise map, the
// automatic chroma parameters, guided smoothing / NL-means behind the wavelets, what the frame driver fuses into its pixel passes).  The
// kernels are denoise.hip's, shrinkblur.hip's and detail.hip's; the decompositions are api_wavelet.hip's.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace {

// What of the neighbouring stages rides inside the denoise tool's pixel passes.  artgpu_improc_denoise_fused decides it and hands
// it down as an argument; the public entry points pass an empty one.  A zero-initialised value means "nothing fused".
struct DnFusion {
    float pre_scale, post_scale;      // != 0: the tool's expcomp(+ecomp) in front of rgb2yuv / expcomp(-ecomp) behind yuv2rgb
    GetImageFuse gi;                  // getImage + matrix read from the demosaiced planes by the chroma map and rgb2yuv
    int exp_on;                       // ImProcFunctions::exposure (process STAGE_1) behind yuv2rgb
    float exp_scale, exp_black;
    int tail_on;                      // ... or on the tool's LAST pixel pass when that is not yuv2rgb (guided smoothing / NL-means behind it)
    float tail_scale, tail_black;
    int ccalc_nonneg;                 // the chroma noise map is the one chroma_map_kernel has just written (squares: no negative value)
};

// detail_recovery's tile masks and the 64-point cosine table with its transpose (L1479-1635), exactly as the reference builds them:
// [tilemask_in | tilemask_out | C | C^T], 64 x 64 each
void build_dct_tabs(float *host)
{
    float *tm_in = host, *tm_out = tm_in + 4096, *ct = tm_out + 4096, *ctt = ct + 4096;
    const float epsilon = 0.001f / (64 * 64);
    const int border = 4; // MAX(2, TS/16)
    for (int i = 0; i < 64; ++i) {
        const float i1 = std::abs((i > 32 ? i - 64 + 1 : i));
        const float vmask = (i1 < border ? (float)0 + (std::sin((M_PI * i1) / (2 * border)) * std::sin((M_PI * i1) / (2 * border))) : 1.0f);
        const float vmask2 = (i1 < 2 * border ? (std::sin((M_PI * i1) / (2 * border)) * std::sin((M_PI * i1) / (2 * border))) : 1.0f);
        for (int j = 0; j < 64; ++j) {
            const float j1 = std::abs((j > 32 ? j - 64 + 1 : j));
            const double sj = std::sin((M_PI * j1) / (2 * border));
            tm_in[i * 64 + j] = (vmask * (j1 < border ? sj * sj : 1.0f)) + epsilon;
            tm_out[i * 64 + j] = (vmask2 * (j1 < 2 * border ? sj * sj : 1.0f)) + epsilon;
            ct[i * 64 + j] = (float)std::cos(M_PI * (j + 0.5) * i / 64.0);
            ctt[j * 64 + i] = ct[i * 64 + j];
        }
    }
}

// Everything RGB_denoise decides on the host before it touches the device: the reference's scalars and the form the shrink passes take.
struct DnPlan {
    int w, h, w2, h2;
    size_t n, n2;                  // pixels of a full-size / a half-size plane
    bool lab_mode, do_detail, useNoiseCCurve;
    float noisevarL;
    bool denoiseLuminance;
    float gam, gamthresh, gamslope, igam, igamthresh, igamslope, gain;
    float realred, realblue, noisevarab_r, noisevarab_b, maxNoiseVarab;
    bool aggressive, autoch;
    int levwav, nsub;
    bool too_small;                // the planes do not hold `levwav` levels on the device path: nothing below is filled
    int rad[10], maxrad;           // box radius of the shrink factors per level
    bool fork;                     // the DCT detail recovery of L on the side stream
    bool mad_fold;                 // MadRgb of the decomposed bands from the analysis kernels' counts (launch_mad_fold)
    int fold_g0, fold_g1;          // ... the grids of the counting level-0 / Haar analysis kernels
    bool fused, merged, merged_mad;   // ShrinkAll: one kernel per channel / one launch for all three / with one MadRgb launch set
    bool two_chroma;               // a and b keep their own decomposition (otherwise b reuses a's)
    int detail_plain;              // DetailArgs::plain
    long long wait_ticks;          // FusedShrinkArgs: bounded wait, test stall
    int stall_band, stall_strip;
};

// Pure: no context, no HIP call.
DnPlan dn_plan(int w, int h, const artgpu_denoise_params *p, double scale, double expcomp, uint32_t flags, bool want_resid, bool has_ccalc,
               int opt_dn_streams, int opt_dn_fused, int opt_dn_detail_plain, long opt_dn_wait_ms, int opt_dn_debug_stall, int opt_dn_mad_fold, int opt_dn_mad_fold_grid)
{
    DnPlan pl = {};
    const int w2 = (w + 1) / 2, h2 = (h + 1) / 2;
    pl.w = w; pl.h = h; pl.w2 = w2; pl.h2 = h2; pl.n = (size_t)w * h; pl.n2 = (size_t)w2 * h2;
    pl.lab_mode = p->color_space == 1;
    pl.do_detail = !(flags & ARTGPU_DN_SKIP_DETAIL_RECOVERY);
    pl.useNoiseCCurve = has_ccalc;
    pl.detail_plain = opt_dn_detail_plain == 1 ? 3 : opt_dn_detail_plain == 2 ? 1 : opt_dn_detail_plain == 3 ? 2 : 0;
    pl.wait_ticks = (long long)opt_dn_wait_ms * 100000LL;
    pl.stall_band = opt_dn_debug_stall < 0 ? -1 : opt_dn_debug_stall >> 16;
    pl.stall_strip = opt_dn_debug_stall < 0 ? -1 : opt_dn_debug_stall & 0xffff;

    // ---- scalar set-up, as the reference computes it on the host (L1687-1688,1795-1825,2032-2082,2246-2293)
    const float noiseluma = (float)p->luminance;
    const double nl_t = (noiseluma / 125.0) * (1.0 + noiseluma / 25.0);
    const float noisevarL = (float)(nl_t * nl_t);
    const bool denoiseLuminance = noisevarL > 0.00001f;
    const float gam = (float)p->gamma;
    const float gamthresh = 0.001f;
    const float gamslope = (float)(std::exp(std::log((double)gamthresh) / gam) / gamthresh);
    pl.noisevarL = noisevarL; pl.denoiseLuminance = denoiseLuminance;
    pl.gam = gam; pl.gamthresh = gamthresh; pl.gamslope = gamslope;
    pl.igam = 1.f / gam; pl.igamthresh = gamthresh * gamslope; pl.igamslope = 1.f / gamslope;
    pl.gain = std::pow(2.0f, float(expcomp));
    const float interm_med = (float)p->chrominance / 10.0;
    float intermred = p->chrominance_red_green > 0. ? (p->chrominance_red_green / 10.) : (float)p->chrominance_red_green / 7.0;
    float intermblue = p->chrominance_blue_yellow > 0. ? (p->chrominance_blue_yellow / 10.) : (float)p->chrominance_blue_yellow / 7.0;
    float realred = interm_med + intermred;
    if (realred <= 0.f) realred = 0.001f;
    float realblue = interm_med + intermblue;
    if (realblue <= 0.f) realblue = 0.001f;
    const float noisevarab_r = realred * realred, noisevarab_b = realblue * realblue;
    pl.realred = realred; pl.realblue = realblue; pl.noisevarab_r = noisevarab_r; pl.noisevarab_b = noisevarab_b;
    pl.maxNoiseVarab = noisevarab_b > noisevarab_r ? noisevarab_b : noisevarab_r;
    int levwav = 5;
    const float maxreal = realred > realblue ? realred : realblue;
    if (maxreal < 8.f) levwav = 5; else if (maxreal < 10.f) levwav = 6; else if (maxreal < 15.f) levwav = 7; else levwav = 8;
    const bool aggressive = p->aggressive != 0;          // QUALITY_HIGH (L1671)
    if (aggressive) levwav += 2;                         // L2260-2262
    if (levwav > 8) levwav = 8;
    { const int t = int(levwav - std::ceil(std::log(scale))); levwav = t > 5 ? t : 5; }
    const int minsizetile = w < h ? w : h;
    int maxlev2 = 8;
    if (minsizetile < 256) maxlev2 = 7;
    if (minsizetile < 128) maxlev2 = 6;
    if (minsizetile < 64) maxlev2 = 5;
    if (minsizetile < 32) maxlev2 = 4;
    if (minsizetile < 16) maxlev2 = 3;
    levwav = levwav < maxlev2 ? levwav : maxlev2;
    const int nsub = 3 * levwav;
    const bool autoch = p->chrominance_method == 1;
    pl.aggressive = aggressive; pl.autoch = autoch; pl.levwav = levwav; pl.nsub = nsub;
    pl.too_small = (w2 < h2 ? w2 : h2) < 2 * wavelet_skip(levwav - 1) || w < 8 || h < 8;
    if (pl.too_small) return pl;

    // ---- streams.  The reference runs a, then b, then L (L2328-2438).  The chains only meet in the untouched L coefficients and their MADs
    // (read by the chroma shrink factors) and in yuv2rgb, so their order is free.  With option "dn_streams" 1 the DCT detail recovery of L -- bound by
    // instruction issue, it leaves HBM idle -- runs on a side stream beside the box blurs and reconstructions of a and b, which are bound by
    // HBM: L goes first for that, after the chroma shrink factors have read its coefficients.  Same kernels on the same data: the same bits.
    // (Rounds 3 and 4: -0.3 ms per frame, the default.  Round 5: off by default -- see opt_dn_streams.)
    // (Running all three chains side by side was measured too: 9.7 ms against 9.2 -- three HBM-bound chains only get in each other's way.)
    pl.fork = opt_dn_streams != 0 && pl.do_detail && denoiseLuminance;

    pl.maxrad = 1;
    for (int l = 0; l < levwav; ++l) { const int r = int((l + 2) / scale); pl.rad[l] = r > 1 ? r : 1; pl.maxrad = pl.rad[l] > pl.maxrad ? pl.rad[l] : pl.maxrad; }
    // ShrinkAllL / ShrinkAllAB as one kernel per channel (shrinkblur.hip: factors, both running sums and the coefficient update in one pass
    // over the coefficients) instead of three with the factor and the row-blurred planes in between: no `sf` / `tmp` planes at all
    pl.fused = opt_dn_fused != 0 && shrink_blur_supported(w2, h2, pl.rad, 0, nsub);
    // ... and for all three channels in ONE launch where nothing has to happen between them (no residuals to read back, no BiShrink
    // passes, every level of L shrunk, both chroma channels denoised): the strips of a band can only follow each other a few blocks apart, so
    // it takes the bands of all channels to keep every CU busy, and one launch instead of three has one ragged end instead of three
    pl.merged = pl.fused && opt_dn_fused != 2 && !aggressive && !want_resid && denoiseLuminance && levwav <= 5 &&
                (autoch || (noisevarab_r > 0.001f && noisevarab_b > 0.001f));
    pl.merged_mad = pl.merged && opt_dn_fused != 3;      // (3: test switch, MadRgb per channel)
    pl.two_chroma = pl.fork || pl.merged;
    // (a frame whose workgroups would count more than their threads' 8-bit counters hold keeps launch_mad: 195 MP and up with the default grids)
    pl.fold_g0 = mad_fold_grid_a0(w2, h2, opt_dn_mad_fold_grid); pl.fold_g1 = mad_fold_grid_haar(pl.n2, opt_dn_mad_fold_grid);
    pl.mad_fold = opt_dn_mad_fold != 0 && mad_fold_a0_fits(w2, h2, pl.fold_g0) && mad_fold_haar_fits(pl.n2, pl.fold_g1);
    return pl;
}

// The planes, decompositions and scratch of one RGB_denoise call, all of them pool slots
struct DnBuffers {
    float *L, *A, *B, *gamlut, *mad, *ccalc_dev;
    float *sfc[3], *tmpc[3], *histo_fc[3];          // 0: L, 1: a, 2: b
    DevDecomp Ld, Cdd[2];
    float *fused_scratch, *Lbands2;
    int *fold_cnt;                                  // mad_fold: the counting kernels' bins, [channel][band of the channel][MAD_FOLD_NB]
    int *fold_flags;
};

// a context that changes between the two forms of the passes gives back what only the other form uses (everything else is shared)
int pool_drop(artgpu_ctx *ctx, int slot)
{
    if (!ctx->pool[slot]) return ARTGPU_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->dn_stream[0]) HIPCHK(ctx, hipStreamSynchronize(ctx->dn_stream[0]));
    HIPCHK(ctx, hipFree(ctx->pool[slot]));
    ctx->pool[slot] = nullptr; ctx->pool_bytes[slot] = 0;
    return ARTGPU_OK;
}

// ---- device buffers; nothing is allocated in steady state.  Scratch planes are shared wherever the order of the kernels allows it:
// one `tmp` (horizontally blurred factors) serves all three channels -- its producer and its consumer are neighbours on the context's
// stream --; in the reference's order one `sf` plane set and one chroma decomposition do too, with the side stream a and b keep theirs
// across the L chain.
int dn_buffers(artgpu_ctx *ctx, const DnPlan &pl, const artgpu_plane *ccalc, DnBuffers *out)
{
    const int w2 = pl.w2, h2 = pl.h2, nsub = pl.nsub;
    const size_t n = pl.n, n2 = pl.n2;
    const bool fused = pl.fused, merged = pl.merged, merged_mad = pl.merged_mad;
    DnBuffers &b = *out;
    b = DnBuffers{};
    float *tmp1 = nullptr;
    DevDecomp &Ld = b.Ld, *Cdd = b.Cdd;
    Ld.w = pl.w; Ld.h = pl.h; Ld.w2 = w2; Ld.h2 = h2; Ld.n = n2; Ld.nlevels = pl.levwav;
    Cdd[0] = Cdd[1] = Ld;
    int rc;
    const size_t histo_bytes = (size_t)nsub * (65536 + MAD_SCRATCH_INTS_PER_BAND) * 4, band_bytes = (size_t)nsub * n2 * 4;
    if ((rc = pool_get(ctx, P_L, n * 4, &b.L)) || (rc = pool_get(ctx, P_A, n * 4, &b.A)) || (rc = pool_get(ctx, P_B, n * 4, &b.B)) ||
        (rc = pool_get(ctx, P_LBANDS, (merged_mad ? 3 : 1) * band_bytes, &Ld.bands)) || (rc = pool_get(ctx, P_LLOW0, n2 * 4, &Ld.low[0])) || (rc = pool_get(ctx, P_LLOW1, n2 * 4, &Ld.low[1])) ||
        (rc = merged_mad ? ARTGPU_OK : pool_get(ctx, P_CBANDS, (merged ? 2 : 1) * band_bytes, &Cdd[0].bands)) || (rc = pool_get(ctx, P_CLOW0, n2 * 4, &Cdd[0].low[0])) || (rc = pool_get(ctx, P_CLOW1, n2 * 4, &Cdd[0].low[1])) ||
        (rc = pool_get(ctx, P_HISTO, (merged_mad ? 3 : 1) * histo_bytes, &b.histo_fc[0])) ||
        (rc = pool_get(ctx, P_MAD, 2 * 3 * 32 * 4, &b.mad)) || (rc = pool_get(ctx, P_GAM, 2 * 65536 * 4, &b.gamlut)))
        return rc;
    b.fold_flags = reinterpret_cast<int *>(b.mad) + 96;
    if (pl.mad_fold) {
        // the channels of one launch_mad_fold call lie behind each other (merged_mad: L, a, b); every other plan takes its MADs channel by
        // channel, each right behind its decomposition on the one stream, so all channels share the first channel's words
        float *pf;
        if ((rc = pool_get(ctx, P_MADPART, (size_t)(merged_mad ? 3 : 1) * nsub * MAD_FOLD_NB * sizeof(int), &pf))) return rc;
        b.fold_cnt = reinterpret_cast<int *>(pf);
    }
    // What only the OTHER form of the shrink passes uses (band-sized slots) is given back, but not on every switch: `fused` depends on the
    // frame (w2, h2 >= 64, radii <= 15), so a context or a batch that alternates small and large frames would pay a stream drain and a band-sized
    // hipFree / hipMalloc per frame -- the allocation the pool exists to avoid.  The slots go after FOUR calls in a row in the same form
    // (artgpu_trim_scratch returns everything at once).
    if (ctx->dn_form == (fused ? 1 : 0)) ++ctx->dn_form_streak; else { ctx->dn_form = fused ? 1 : 0; ctx->dn_form_streak = 1; }
    const bool settle = ctx->dn_form_streak >= 4;
    if (fused) {
        if (settle && ((rc = pool_drop(ctx, P_SF_A)) || (rc = pool_drop(ctx, P_SF_B)) || (merged && (rc = pool_drop(ctx, P_CBANDS2))))) return rc;
        if (!ctx->fs_diag) {      // (optional: without it a timed-out wait still traps, merely unattributed)
            if (hipHostMalloc(reinterpret_cast<void **>(&ctx->fs_diag), 64, hipHostMallocDefault) == hipSuccess) std::memset(ctx->fs_diag, 0, 64);
            else { ctx->fs_diag = nullptr; (void)hipGetLastError(); }
        }
        if ((rc = pool_get(ctx, P_FUSED, shrink_blur_scratch_floats(w2, h2, merged ? 3 * nsub : nsub, pl.maxrad) * 4, &b.fused_scratch))) return rc;
        // the chroma factors need the L coefficients as the decomposition left them: whenever they are evaluated beside or after the L pass
        // (one launch for all channels; the side stream's order) the L pass writes a second band set instead of updating the first
        if ((pl.fork || merged) && (rc = pool_get(ctx, P_LBANDS2, band_bytes, &b.Lbands2))) return rc;
    } else if ((settle && ((rc = pool_drop(ctx, P_FUSED)) || (rc = pool_drop(ctx, P_LBANDS2)))) || (rc = pool_get(ctx, P_SF, band_bytes, &b.sfc[0])) || (rc = pool_get(ctx, P_TMP, band_bytes, &tmp1))) return rc;
    b.tmpc[0] = b.tmpc[1] = b.tmpc[2] = tmp1;
    if (pl.two_chroma) {
        if (merged_mad) Cdd[0].bands = Ld.bands + (size_t)nsub * n2;       // (one MadRgb launch set walks the bands of all three channels)
        if (merged) Cdd[1].bands = Cdd[0].bands + (size_t)nsub * n2;       // (one launch walks both channels' bands: back to back)
        else if ((rc = pool_get(ctx, P_CBANDS2, band_bytes, &Cdd[1].bands))) return rc;
        if ((rc = pool_get(ctx, P_CLOW0_2, n2 * 4, &Cdd[1].low[0])) || (rc = pool_get(ctx, P_CLOW1_2, n2 * 4, &Cdd[1].low[1])) ||
            (rc = pool_get(ctx, P_HISTO_A, (merged ? 2 : 1) * histo_bytes, &b.histo_fc[1])) || (rc = pool_get(ctx, P_HISTO_B, histo_bytes, &b.histo_fc[2])))
            return rc;
        if (!fused && ((rc = pool_get(ctx, P_SF_A, band_bytes, &b.sfc[1])) || (rc = pool_get(ctx, P_SF_B, band_bytes, &b.sfc[2])))) return rc;
    } else {
        b.sfc[1] = b.sfc[2] = b.sfc[0];
        b.histo_fc[1] = b.histo_fc[2] = b.histo_fc[0];
        Cdd[1] = Cdd[0];
    }
    if (pl.mad_fold)
        for (int c = 0; c < 3; ++c) {        // 0: L, 1: a, 2: b
            DevDecomp &d = c == 0 ? Ld : Cdd[c - 1];
            d.g0 = pl.fold_g0; d.g1 = pl.fold_g1;
            d.cnt = b.fold_cnt + (merged_mad ? (size_t)c * nsub * MAD_FOLD_NB : 0);
        }
    if (pl.useNoiseCCurve) {
        if (!plane_ok(ccalc) || ccalc->w != w2 || ccalc->h != h2) return fail(ctx, ARTGPU_EINVAL, "rgb_denoise: ccalc must be %dx%d", w2, h2);
        if (ccalc->on_device && (size_t)ccalc->row_stride_bytes == (size_t)w2 * 4) {
            b.ccalc_dev = ccalc->p;            // dense and on the device already (the map artgpu_improc_denoise has just computed): read in place
        } else {
            if ((rc = pool_get(ctx, P_CCALC, n2 * 4, &b.ccalc_dev))) return rc;
            HIPCHK(ctx, hipMemcpy2DAsync(b.ccalc_dev, (size_t)w2 * 4, ccalc->p, (size_t)ccalc->row_stride_bytes, (size_t)w2 * 4, h2,
                                         ccalc->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
        }
    }
    return ARTGPU_OK;
}

// The steps of one RGB_denoise call on the device: each queues its kernels on the context's stream `sL` (the detail recovery on `sd`)
struct DnRun {
    artgpu_ctx *ctx;
    const DnPlan &pl;
    DnBuffers &b;
    const DnFusion &fu;
    const artgpu_denoise_params *p;
    double scale;
    float *nresi, *highresi;
    hipStream_t sL;
    float noisevar_abc[2];
    float chresidtemp, chmaxresidtemp;
    float *Lout;                     // where the denoised L ends up: yuv2rgb reads it

    BlurArgs blur0() const
    {
        BlurArgs bl0 = {};
        bl0.n = pl.n2; bl0.w = pl.w2; bl0.h = pl.h2;
        for (int l = 0; l < 10; ++l) bl0.rad[l] = pl.rad[l];
        return bl0;
    }
    // what every launch of the fused ShrinkAll pass has in common
    FusedShrinkArgs fused_args(float nv_const) const
    {
        FusedShrinkArgs fa = {};
        fa.n = pl.n2; fa.w = pl.w2; fa.h = pl.h2;
        fa.noisevar = b.ccalc_dev; fa.noisevar_nonneg = fu.ccalc_nonneg; fa.noisevar_const = nv_const; fa.noisevar_scale = pl.maxNoiseVarab;
        fa.useNoiseCCurve = pl.useNoiseCCurve ? 1 : 0;
        for (int l = 0; l < 10; ++l) fa.rad[l] = pl.rad[l];
        fa.diag = ctx->fs_diag; fa.wait_ticks = pl.wait_ticks; fa.stall_band = pl.stall_band; fa.stall_strip = pl.stall_strip;
        return fa;
    }
    int fused_pass(bool ab, const float *cin, float *cout, const float *cL, const float *mL, const float *mab, int lev0, int nb, float nv_const, float noisevar_ab);
    // SQR(MadRgb) of bands that decompose_dev has just written and nothing has touched since (`nb` = one channel's bands, or all three channels')
    int mad_decomposed(const float *bands, int nb, int *histo, float *out)
    {
        if (!pl.mad_fold) { HIPCHK(ctx, launch_mad(bands, pl.n2, nb, histo, out, sL)); return ARTGPU_OK; }
        int *flags = b.fold_flags + (out - b.mad);
        HIPCHK(ctx, launch_mad_fold(bands, pl.n2, nb, pl.nsub, b.fold_cnt, histo, out, flags, sL));
        if (ctx->dn_fold_nranges < 8) { ctx->dn_fold_ranges[ctx->dn_fold_nranges][0] = (int)(out - b.mad); ctx->dn_fold_ranges[ctx->dn_fold_nranges][1] = nb; ++ctx->dn_fold_nranges; }
        return ARTGPU_OK;
    }
    int chroma_front(int ch);
    int chroma_back(int ch);
    int luma(hipStream_t sd);
    int detail_recovery(hipStream_t sd);
    int merged_pass();
};

// one fused ShrinkAll pass over `nb` bands starting at level `lev0` (pointers already offset to the first band)
int DnRun::fused_pass(bool ab, const float *cin, float *cout, const float *cL, const float *mL, const float *mab, int lev0, int nb,
                      float nv_const, float noisevar_ab)
{
    FusedShrinkArgs fa = fused_args(nv_const);
    if (ab) { fa.coefC = cout; fa.nL = 0; fa.nsub_ch = nb; }           // (chroma bands are updated in place: cin == cout)
    else { fa.coef = cin; fa.coef_out = cout; fa.nL = nb; }
    fa.coefL = cL;
    fa.madL = mL; fa.madab = mab;
    fa.noisevar_ab[0] = fa.noisevar_ab[1] = noisevar_ab;
    fa.level0 = lev0; fa.nsub = nb;
    HIPCHK(ctx, launch_shrink_blur(fa, b.fused_scratch, sL));
    return ARTGPU_OK;
}

// ---- a and b (L2328-2402), first half: decompose, MADs, shrink factors against the untouched L coefficients
int DnRun::chroma_front(int ch)
{
    const int nsub = pl.nsub;
    const size_t n2 = pl.n2;
    const DevDecomp &Ld = b.Ld;
    DevDecomp &Cd = b.Cdd[ch];
    float *sf = b.sfc[1 + ch], *tmp = b.tmpc[1 + ch], *madL = b.mad, *madab = b.mad + 32 * (1 + ch);
    int *histo = reinterpret_cast<int *>(b.histo_fc[1 + ch]);
    float noisevar_ab = ch == 0 ? pl.noisevarab_r : pl.noisevarab_b;
    if (pl.autoch && noisevar_ab <= 0.001f) noisevar_ab = 0.02f;
    noisevar_abc[ch] = noisevar_ab;
    int rc2;
    if ((rc2 = decompose_dev(ctx, Cd, ch == 0 ? b.A : b.B, sL))) return rc2;
    if (pl.aggressive && noisevar_ab > 0.001f) {
        // WaveletDenoiseAll_BiShrinkAB (L976-1108): MAD of all untouched bands, ShrinkAllAB on the top level (same MAD),
        // point-wise shrink of the levels below
        if ((rc2 = mad_decomposed(Cd.bands, nsub, histo, madab))) return rc2;
        ShrinkArgs sa = {};
        sa.n = n2; sa.noisevar = b.ccalc_dev; sa.noisevar_scale = pl.maxNoiseVarab; sa.noisevar_ab = noisevar_ab; sa.useNoiseCCurve = pl.useNoiseCCurve ? 1 : 0;
        const size_t top = (size_t)(nsub - 3) * n2;
        sa.coef = Cd.bands + top; sa.coefL = Ld.bands + top; sa.sfave = sf; sa.madL = madL + (nsub - 3); sa.madab = madab + (nsub - 3);
        if (pl.fused) {
            if ((rc2 = fused_pass(true, Cd.bands + top, Cd.bands + top, Ld.bands + top, madL + (nsub - 3), madab + (nsub - 3), pl.levwav - 1, 3, 0.f, noisevar_ab))) return rc2;
        } else {
            HIPCHK(ctx, launch_shrink_sf(sa, 3, true, sL));
            BlurArgs bt = blur0();
            bt.level0 = pl.levwav - 1;
            bt.src = sf; bt.dst = tmp;
            HIPCHK(ctx, launch_hblur(bt, 3, sL));
            bt.src = tmp; bt.sfave = sf; bt.coef = Cd.bands + top;
            HIPCHK(ctx, launch_vblur_combine(bt, 3, sL));
        }
        if (nsub > 3) {
            sa.coef = Cd.bands; sa.coefL = Ld.bands; sa.madL = madL; sa.madab = madab;
            HIPCHK(ctx, launch_bishrink_AB(sa, nsub - 3, sL));
        }
    }
    if (noisevar_ab > 0.001f && !pl.merged_mad) {
        float *out = ch == 1 && pl.merged ? b.mad + 32 + nsub : madab;
        // (the BiShrink branch above has shrunk these bands: they are no longer what the decomposition counted)
        if (pl.aggressive) HIPCHK(ctx, launch_mad(Cd.bands, n2, nsub, histo, out, sL));
        else if ((rc2 = mad_decomposed(Cd.bands, nsub, histo, out))) return rc2;
        if (!pl.fused) {
            ShrinkArgs sa = {};
            sa.coef = Cd.bands; sa.coefL = Ld.bands; sa.sfave = sf; sa.n = n2; sa.madL = madL; sa.madab = madab;
            sa.noisevar = b.ccalc_dev; sa.noisevar_scale = pl.maxNoiseVarab; sa.noisevar_ab = noisevar_ab; sa.useNoiseCCurve = pl.useNoiseCCurve ? 1 : 0;
            HIPCHK(ctx, launch_shrink_sf(sa, nsub, true, sL));
        }
    }
    return ARTGPU_OK;
}

// second half: box blur of the shrink factors, coefficient update, residuals, reconstruction
int DnRun::chroma_back(int ch)
{
    const int nsub = pl.nsub;
    DevDecomp &Cd = b.Cdd[ch];
    float *sf = b.sfc[1 + ch], *tmp = b.tmpc[1 + ch], *madab = b.mad + 32 * (1 + ch);
    int *histo = reinterpret_cast<int *>(b.histo_fc[1 + ch]);
    if (noisevar_abc[ch] > 0.001f && !pl.merged) {
        if (pl.fused) {
            // (the factors read the L coefficients as the decomposition left them: in the reference's order L comes last, with the side
            // stream the L pass has written a second band set)
            int rc2 = fused_pass(true, Cd.bands, Cd.bands, b.Ld.bands, b.mad, madab, 0, nsub, 0.f, noisevar_abc[ch]);
            if (rc2) return rc2;
        } else {
            BlurArgs bl = blur0();
            bl.src = sf; bl.dst = tmp;
            HIPCHK(ctx, launch_hblur(bl, nsub, sL));
            bl.src = tmp; bl.sfave = sf; bl.coef = Cd.bands;
            HIPCHK(ctx, launch_vblur_combine(bl, nsub, sL));
        }
    }
    if (nresi || highresi) {
        // Noise_residualAB (FTblockDN.cc:605-635, kall == 0): SQR(MadRgb) of the shrunk chroma bands, summed in level/dir order
        float host[32];
        HIPCHK(ctx, launch_mad(Cd.bands, pl.n2, nsub, histo, madab, sL));
        HIPCHK(ctx, hipMemcpyAsync(host, madab, (size_t)nsub * sizeof(float), hipMemcpyDeviceToHost, sL));
        HIPCHK(ctx, hipStreamSynchronize(sL));
        float resid = 0.f, maxresid = 0.f;
        for (int k = 0; k < nsub; ++k) {
            resid += host[k];
            if (host[k] > maxresid) maxresid = host[k];
        }
        if (ch == 0) { chresidtemp = resid; chmaxresidtemp = maxresid; }
        else {
            float chresid = resid + chresidtemp, chmaxresid = maxresid + chmaxresidtemp;      // L2389-2396
            chresid = std::sqrt(chresid / (6 * (pl.levwav)));
            if (highresi) *highresi = chresid + 0.66f * (std::sqrt(chmaxresid) - chresid);
            if (nresi) *nresi = chresid;
        }
    }
    return reconstruct_dev(ctx, Cd, ch == 0 ? b.A : b.B, sL);
}

// ---- L: shrink the first min(levels,5) levels, reconstruct (L2405-2438); detail recovery on stream `sd`
int DnRun::luma(hipStream_t sd)
{
    if (!pl.denoiseLuminance) return ARTGPU_OK;
    int rc2;
    const int nsub = pl.nsub, nsubL = 3 * (pl.levwav < 5 ? pl.levwav : 5);
    const size_t n2 = pl.n2;
    const DevDecomp &Ld = b.Ld;
    float *sf = b.sfc[0], *tmp = b.tmpc[0];
    BlurArgs bl = blur0();
    ShrinkArgs sa = {};
    sa.coef = Ld.bands; sa.sfave = sf; sa.n = n2; sa.madL = b.mad; sa.noisevar = nullptr; sa.noisevar_const = pl.noisevarL;
    // QUALITY_HIGH runs WaveletDenoiseAll_BiShrinkL first (L842-973); its per-band body is ShrinkAllL's (top level included),
    // and madL is not recomputed in between (L2408-2421): the standard pass simply runs twice
    DevDecomp Lrec = Ld;                   // what the reconstruction reads
    if (pl.merged) Lrec.bands = b.Lbands2;
    for (int rep = pl.aggressive ? 0 : 1; rep < 2 && !pl.merged; ++rep) {
        if (pl.fused) {
            // the first pass reads the decomposition; with a second band set it writes there, and a second pass (QUALITY_HIGH) works on that
            float *dstb = b.Lbands2 ? b.Lbands2 : Ld.bands;
            if ((rc2 = fused_pass(false, Lrec.bands, dstb, nullptr, b.mad, nullptr, 0, nsubL, pl.noisevarL, 0.f))) return rc2;
            Lrec.bands = dstb;
        } else {
            HIPCHK(ctx, launch_shrink_sf(sa, nsubL, false, sL));
            bl.src = sf; bl.dst = tmp;
            HIPCHK(ctx, launch_hblur(bl, nsubL, sL));
            bl.src = tmp; bl.sfave = sf; bl.coef = Ld.bands;
            HIPCHK(ctx, launch_vblur_combine(bl, nsubL, sL));
        }
    }
    if (Lrec.bands != Ld.bands && nsubL < nsub)          // levels beyond the fifth are reconstructed as they are
        HIPCHK(ctx, hipMemcpyAsync(Lrec.bands + (size_t)nsubL * n2, Ld.bands + (size_t)nsubL * n2, (size_t)(nsub - nsubL) * n2 * 4, hipMemcpyDeviceToDevice, sL));
    if (pl.do_detail) {
        // labdn->L is kept as Lin before the reconstruction modifies it (L2423-2432): here the reconstruction writes a second plane
        // instead of the first being copied
        if ((rc2 = pool_get(ctx, P_LIN, pl.n * 4, &Lout))) return rc2;
    }
    Lrec.cur = Ld.cur;
    if ((rc2 = reconstruct_dev(ctx, Lrec, Lout, sL))) return rc2;
    return pl.do_detail ? detail_recovery(sd) : ARTGPU_OK;
}

// ---- detail_recovery (L1479-1635) of the reconstructed L in `Lout` against the L the decomposition read; host-side scalars exactly as
// the reference computes them.  The detail mask is built on `sL`, the two DCT kernels run on `sd`.
int DnRun::detail_recovery(hipStream_t sd)
{
    const int w = pl.w, h = pl.h;
    int rc2;
    DetailArgs da = {};
    da.w = w; da.h = h;
    da.numblox_W = (int)std::ceil(((float)w) / 25) + 2;
    da.numblox_H = (int)std::ceil(((float)h) / 25) + 2;
    const float params_Ldetail = std::min(float(p->luminance_detail), 99.9f);
    auto compute_detail = [](float dd) -> float { const float t = static_cast<float>((100. - dd) * (100. - dd) + 50. * (100. - dd)) * 64 * 0.5f; return t * t; };
    da.detail_hi = compute_detail(params_Ldetail);
    da.detail_lo = compute_detail(0.f);
    { const int br = int(3 / scale); da.blur_rad = br > 1 ? br : 1; }
    float *dtab;
    // the tables are constants: built and uploaded once per context (a slot of their own: the upload needs a stream
    // synchronisation, i.e. a bubble in the middle of every frame)
    if ((rc2 = const_table_dev(ctx, P_DCTTAB, 4 * 4096, build_dct_tabs, "DCT tables", &dtab))) return rc2;
    if ((rc2 = pool_get(ctx, P_BLOCKS, (size_t)da.numblox_W * da.numblox_H * 4096 * 4, &da.blocks))) return rc2;
    da.tm_in = dtab; da.tm_out = dtab + 4096; da.costab = dtab + 2 * 4096; da.costab_t = dtab + 3 * 4096;
    da.L = Lout; da.Lin = b.L;
    da.plain = pl.detail_plain;
    if (p->luminance_detail_threshold > 0) {
        // detail_mask(LL, mask, 65535, 25, 10000, amount, GAUSS, 25 / scale) on the denoised L (FTblockDN.cc:1502-1507)
        float *dmask;
        if ((rc2 = pool_get(ctx, P_DMASK, pl.n * 4, &dmask))) return rc2;
        const float amount = std::max(0.f, std::min(float(p->luminance_detail_threshold) / 100.f, 1.f));
        float *dm_scratch = b.tmpc[0];
        if (!dm_scratch && (rc2 = pool_get(ctx, P_TMP, ((size_t)w * h + 2 * (size_t)(w / 4) * (h / 4)) * 4, &dm_scratch))) return rc2;   // (fused: no `tmp` plane set)
        if ((rc2 = detail_mask_dev(ctx, Lout, (size_t)w, dmask, w, h, 65535.f, 25.f, 10000.f, amount, (float)(25.f / scale), dm_scratch))) return rc2;
        da.mask = dmask; da.params_Ldetail = params_Ldetail;
    }
    if (sd != sL) {
        HIPCHK(ctx, hipEventRecord(ctx->dn_ev[0], sL));
        HIPCHK(ctx, hipStreamWaitEvent(sd, ctx->dn_ev[0], 0));
    }
    HIPCHK(ctx, launch_detail_blocks(da, sd));
    HIPCHK(ctx, launch_detail_gather(da, sd));
    if (sd != sL) HIPCHK(ctx, hipEventRecord(ctx->dn_ev[1], sd));
    return ARTGPU_OK;
}

// the ShrinkAll passes of L, a and b as one launch (DnPlan::merged)
int DnRun::merged_pass()
{
    const int nsub = pl.nsub;
    FusedShrinkArgs fa = fused_args(pl.noisevarL);
    fa.coef = b.Ld.bands; fa.coef_out = b.Lbands2; fa.coefC = b.Cdd[0].bands; fa.coefL = b.Ld.bands;
    fa.madL = b.mad; fa.madab = pl.merged_mad ? b.mad + nsub : b.mad + 32; fa.mad_ch_stride = nsub;
    fa.noisevar_ab[0] = noisevar_abc[0]; fa.noisevar_ab[1] = noisevar_abc[1];
    fa.level0 = 0; fa.nsub = 3 * nsub; fa.nL = nsub; fa.nsub_ch = nsub;
    HIPCHK(ctx, launch_shrink_blur(fa, b.fused_scratch, sL));
    return ARTGPU_OK;
}

// the checks of RGB_denoise's parameters that the public entry point and the tool share
int rgb_denoise_args_ok(artgpu_ctx *ctx, const artgpu_denoise_params *p, bool has_iws, double scale)
{
    if (p->color_space != 0 && p->color_space != 1) return fail(ctx, ARTGPU_EINVAL, "rgb_denoise: color_space must be 0 (RGB) or 1 (LAB)");
    if (p->color_space == 1 && !has_iws) return fail(ctx, ARTGPU_EINVAL, "rgb_denoise: LAB mode needs the inverse working-space matrix");
    if (p->chrominance_method != 0 && p->chrominance_method != 1) return fail(ctx, ARTGPU_EINVAL, "rgb_denoise: chrominance_method must be 0 (MANUAL) or 1 (AUTOMATIC)");
    if (!(scale >= 1.0)) return fail(ctx, ARTGPU_EINVAL, "rgb_denoise: scale must be >= 1");
    return ARTGPU_OK;
}

int rgb_denoise_size_ok(artgpu_ctx *ctx, int w, int h)
{
    if (w > 32767 || h > 32767) return fail(ctx, ARTGPU_EUNSUPPORTED, "rgb_denoise: the reference holds the size in short (FTblockDN.cc:1779)");
    return ARTGPU_OK;
}

// RGB_denoise on device planes (the caller has checked the parameters and bound the image); `fu`: what the tool around it has fused into
// the first and the last pixel pass
int rgb_denoise_dev(artgpu_ctx *ctx, const DevRGB &d, const artgpu_denoise_params *p, const float ws[9], const float *iws,
                    double expcomp, double scale, const artgpu_plane *ccalc, uint32_t flags, float *nresi, float *highresi, const DnFusion &fu)
{
    const int w = d.w, h = d.h;
    int rc = rgb_denoise_size_ok(ctx, w, h);
    if (rc) return rc;
    if (p->luminance == 0 && p->chrominance == 0 && !ccalc) return ARTGPU_OK; // L1655-1668: nothing to do
    const DnPlan pl = dn_plan(w, h, p, scale, expcomp, flags, nresi || highresi, ccalc != nullptr,
                              ctx->shared.opt_dn_streams, ctx->shared.opt_dn_fused, ctx->shared.opt_dn_detail_plain, ctx->shared.opt_dn_wait_ms, ctx->shared.opt_dn_debug_stall, ctx->shared.opt_dn_mad_fold, ctx->shared.opt_dn_mad_fold_grid);
    if (pl.too_small) return fail(ctx, ARTGPU_EUNSUPPORTED, "rgb_denoise: %dx%d too small for %d wavelet levels on the device path", w, h, pl.levwav);
    DnBuffers b;
    if ((rc = dn_buffers(ctx, pl, ccalc, &b))) return rc;
    if (pl.fork && !ctx->dn_stream[0]) {
        HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->dn_stream[0], hipStreamNonBlocking));
        for (int k = 0; k < 2; ++k) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->dn_ev[k], hipEventDisableTiming));
    }
    hipStream_t sL = ctx->stream;

    // ---- gamma LUTs (built on the device with the SSE-form sleef, color.cc:1128-1161)
    //      -- once per set of parameters: the pair built by the previous call on this context is still there when they have not changed
    {
        const float key[6] = {pl.gam, pl.gamthresh, pl.gamslope, pl.igam, pl.igamthresh, pl.igamslope};
        if (ctx->gam_tab != b.gamlut || std::memcmp(ctx->gam_key, key, sizeof key) != 0) {
            ctx->gam_tab = nullptr;
            HIPCHK(ctx, launch_gamma_lut(b.gamlut, pl.gam, pl.gamthresh, pl.gamslope, 65535.f, 65535.f, sL));
            HIPCHK(ctx, launch_gamma_lut(b.gamlut + 65536, pl.igam, pl.igamthresh, pl.igamslope, 65535.f, 65535.f, sL));
            std::memcpy(ctx->gam_key, key, sizeof key);
            ctx->gam_tab = b.gamlut;
        }
    }

    DnPixArgs px = {};
    for (int k = 0; k < 3; ++k) { px.rgb[k] = d.p[k]; px.ws1[k] = ws[3 + k]; }
    px.stride = d.stride; px.L = b.L; px.A = b.A; px.B = b.B; px.w = w; px.h = h;
    px.gain = pl.gain; px.newGain = 1.f / pl.gain;
    px.gam = pl.gam; px.gamthresh = pl.gamthresh; px.gamslope = pl.gamslope; px.igam = pl.igam; px.igamthresh = pl.igamthresh; px.igamslope = pl.igamslope;
    px.gamcurve = b.gamlut; px.igamcurve = b.gamlut + 65536;
    px.pre_scale = fu.pre_scale; px.post_scale = fu.post_scale; px.no_lds_lut = !ctx->shared.opt_lut_lds; px.cu_reserve = cu_reserve_of(ctx);
    px.gi = fu.gi; px.exp_on = fu.exp_on; px.exp_scale = fu.exp_scale; px.exp_black = fu.exp_black;
    // the inverse-gamma pass looks up gamma-encoded values: the mid-tones sit in the middle of the table, so the 40704 entries kept in LDS
    // start at 8000 (gamma 1.7: linear 0.03 .. 0.60 of white); the forward pass and the tone curve index with linear data and keep [0, 40704)
    px.igam_lds_lo = 8000;
    if (pl.lab_mode) {
        float *tabs;
        if ((rc = lab_tabs_dev(ctx, &tabs))) return rc;
        px.lab_mode = 1;
        px.cachef = tabs; px.cachefy = tabs + 65536; px.dn_gamma = tabs + 2 * 65536; px.dn_igamma = tabs + 3 * 65536;
        for (int k = 0; k < 9; ++k) { px.wpi[k] = ws[k]; px.iws[k] = iws[k]; }
    }
    px.realred = pl.realred; px.realblue = pl.realblue; px.qhighFactor = pl.aggressive ? 1.f / static_cast<float>(0.9) : 1.0f;   // L1672
    HIPCHK(ctx, launch_rgb2yuv(px, sL));

    // ---- L decomposition and its MADs (L2296-2320)
    ctx->dn_fold_nranges = 0; ctx->dn_fold_flags = b.fold_flags;
    if ((rc = decompose_dev(ctx, b.Ld, b.L, sL))) return rc;
    DnRun run = {ctx, pl, b, fu, p, scale, nresi, highresi, sL, {0.f, 0.f}, 0.f, 0.f, b.L};
    if (!pl.merged_mad && (rc = run.mad_decomposed(b.Ld.bands, pl.nsub, reinterpret_cast<int *>(b.histo_fc[0]), b.mad))) return rc;

    if (pl.merged) {
        // decompositions and MADs of a and b, the three channels' ShrinkAll passes as one launch, then the reconstructions -- L first, so that
        // its DCT detail recovery (side stream) runs beside those of a and b
        if ((rc = run.chroma_front(0)) || (rc = run.chroma_front(1))) return rc;
        // MadRgb of all three channels' bands as one launch set (the bands are back to back: L, a, b; the medians land at mad + band)
        if (pl.merged_mad && (rc = run.mad_decomposed(b.Ld.bands, 3 * pl.nsub, reinterpret_cast<int *>(b.histo_fc[0]), b.mad))) return rc;
        if ((rc = run.merged_pass())) return rc;
        SideStreamJoin dn_join;
        if (pl.fork) dn_join.arm(ctx->dn_stream[0]);
        if ((rc = run.luma(pl.fork ? ctx->dn_stream[0] : sL))) return rc;
        if ((rc = run.chroma_back(0)) || (rc = run.chroma_back(1))) return rc;
        if (pl.fork) {
            HIPCHK(ctx, hipStreamWaitEvent(sL, ctx->dn_ev[1], 0));
            dn_join.disarm();
        }
    } else if (!pl.fork) {
        // the reference's order
        for (int ch = 0; ch < 2; ++ch)
            if ((rc = run.chroma_front(ch)) || (rc = run.chroma_back(ch))) return rc;
        if ((rc = run.luma(sL))) return rc;
    } else {
        if ((rc = run.chroma_front(0)) || (rc = run.chroma_front(1))) return rc;      // the last readers of the untouched L coefficients
        SideStreamJoin dn_join;
        dn_join.arm(ctx->dn_stream[0]);                                       // any return below leaves with the side stream drained
        if ((rc = run.luma(ctx->dn_stream[0]))) return rc;
        if ((rc = run.chroma_back(0)) || (rc = run.chroma_back(1))) return rc;
        HIPCHK(ctx, hipStreamWaitEvent(sL, ctx->dn_ev[1], 0));                // join: the context's stream is behind all the work of the call
        dn_join.disarm();
    }
    px.L = run.Lout;

    // ---- back to RGB (L2502-2550)
    HIPCHK(ctx, launch_yuv2rgb(px, ctx->stream));
    return ARTGPU_OK;
}

// fills P_CCMAP ((w+1)/2 x (h+1)/2, contiguous) from device planes, or, with `gi` on, from the demosaiced planes getImage would have read
int chroma_map_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int w, int h, const double *mat, const double ws[9],
                          const float *curve, const GetImageFuse &gi, float **out)
{
    const int wid = (w + 1) / 2, hei = (h + 1) / 2;
    float *map, *tab;
    int rc;
    // P_CACHEF: [cachef, 65536 | the caller's noise curve, 512]; a slot that has just been made holds no curve
    if (!ctx->pool[P_CACHEF]) ctx->ncurve_host.clear();
    if ((rc = pool_get(ctx, P_CCMAP, (size_t)wid * hei * 4, &map)) || (rc = const_table_dev(ctx, P_CACHEF, 65536 + 512, build_cachef, "cachef table", &tab))) return rc;
    // the same curve frame after frame is uploaded once: the copy needs a stream synchronisation (the caller's curve may be a
    // temporary), i.e. a bubble in the middle of every frame
    if (ctx->ncurve_host.size() != 501 || std::memcmp(ctx->ncurve_host.data(), curve, 501 * 4) != 0) {
        ctx->ncurve_host.assign(curve, curve + 501);
        hipError_t e = hipMemcpyAsync(tab + 65536, ctx->ncurve_host.data(), 501 * 4, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            ctx->ncurve_host.clear();
            return fail(ctx, ARTGPU_EHIP, "chroma map: upload of the noise curve failed: %s", hipGetErrorString(e));
        }
    }
    ChromaMapArgs a = {};
    a.gi = gi;
    for (int k = 0; k < 3; ++k) a.src[k] = planes[k];
    a.stride = stride; a.wid = wid; a.hei = hei;
    a.has_mat = mat ? 1 : 0;
    for (int k = 0; k < 9; ++k) { a.mat[k] = mat ? mat[k] : 0.0; a.wpi[k] = (float)ws[k]; }
    a.cachef = tab; a.curve = tab + 65536; a.out = map; a.no_lds_lut = !ctx->shared.opt_lut_lds; a.cu_reserve = cu_reserve_of(ctx);
    HIPCHK(ctx, launch_chroma_map(a, ctx->stream));
    *out = map;
    return ARTGPU_OK;
}

// useNoiseCCurve (FTblockDN.cc:1672): the chroma noise curve counts when NoiseCurve::getSum (ipdenoise.cc:698) of its 501 entries is above 5
bool noise_curve_on(const float *curve)
{
    if (!curve) return false;
    float sum = 0.f;
    for (int i = 0; i < 501; ++i) sum += curve[i];
    return sum > 5.f;
}

// ImProcFunctions::denoise on the device image, after denoise_tool_check; `fu0`: what improc_denoise_dev has decided to fuse of the stages around
// the tool (the tool's own expcomp passes and `ccalc_nonneg` are decided here)
int denoise_tool_dev(artgpu_ctx *ctx, const DevRGB &d, const artgpu_denoise_tool_params *p, const double ws[9], const double *iws,
                     double ecomp, double scale, const double *calclum_mat, const float *noise_c_curve, uint32_t flags, const DnFusion &fu0)
{
    float wsf[9];
    for (int k = 0; k < 9; ++k) wsf[k] = (float)ws[k];
    int rc;
    // adjust_params (ipdenoise.cc:35-63): a preview at scale > 1 sees averaged-down noise, so the strengths shrink with it
    artgpu_denoise_tool_params adj = *p;
    if (scale > 1.0) {
        const auto c = [](double x, double f) -> double {
            const int sgn = (0.0 < x) - (x < 0.0);
            const double y = std::max(0.0, std::min(std::abs(x) / 100.0, 1.0));
            return sgn * (y * (y * f) + (1.0 - y) * y) * 100.0;      // intp(y, y*f, y)
        };
        const double scale_factor = 1.0 / scale;
        const double noise_factor_c = std::pow(scale_factor, 0.46);
        const double noise_factor_l = std::pow(scale_factor, 0.62) * scale_factor;
        adj.dn.luminance = c(adj.dn.luminance, noise_factor_l);
        adj.dn.luminance_detail *= (1.0 + std::pow(1.0 - scale_factor, 2.2));
        adj.dn.chrominance = c(adj.dn.chrominance, noise_factor_c);
        adj.dn.chrominance_red_green = c(adj.dn.chrominance_red_green, noise_factor_c);
        adj.dn.chrominance_blue_yellow = c(adj.dn.chrominance_blue_yellow, noise_factor_c);
    }
    p = &adj;
    artgpu_plane ccalc = {}, *ccalc_p = nullptr;
    if (noise_curve_on(noise_c_curve)) {
        float *map;
        if ((rc = chroma_map_dev(ctx, d.p, d.stride, d.w, d.h, calclum_mat, ws, noise_c_curve, fu0.gi, &map))) return rc;
        ccalc = mk_dev_plane(map, (d.w + 1) / 2, (d.h + 1) / 2);
        ccalc_p = &ccalc;
    }
    // expcomp(+ecomp) / expcomp(-ecomp) (ipdenoise.cc:1161-1163,1181-1184) are fused into RGB_denoise's first and last pixel
    // passes when RGB_denoise will actually run them (same operations on the same values, two fewer passes over the image).
    // (Whether it runs is asked of the ADJUSTED strengths here and of the caller's in improc_denoise_dev: both are kept, see there.)
    const bool dn_runs = !(p->dn.luminance == 0 && p->dn.chrominance == 0 && !ccalc_p);
    const bool fuse_pre = ecomp > 0 && dn_runs, fuse_post = fuse_pre && !p->smoothing_enabled;
    if (ecomp > 0 && !fuse_pre) {
        StageScope scope_(ctx, "ImProcFunctions::expcomp");
        if ((rc = exposure_dev(ctx, d, (float)std::pow(2.0, ecomp), 0.f))) return rc;
    }
    DnFusion fu = fu0;
    fu.pre_scale = fuse_pre ? (float)std::pow(2.0, ecomp) : 0.f;
    fu.post_scale = fuse_post ? (float)std::pow(2.0, -ecomp) : 0.f;
    fu.ccalc_nonneg = ccalc_p ? 1 : 0;
    float iwsf[9];
    if (iws) for (int k = 0; k < 9; ++k) iwsf[k] = (float)iws[k];
    {
        StageScope scope_(ctx, "denoise::RGB_denoise");
        if ((rc = rgb_denoise_dev(ctx, d, &p->dn, wsf, iws ? iwsf : nullptr, 0.0, scale, ccalc_p, flags, nullptr, nullptr, fu))) return rc;
    }
    // the exposure steps behind the tool's last stage -- its own expcomp(-ecomp) (L1181-1184) where yuv2rgb could not take it, and the STAGE_1
    // exposure of artgpu_improc_denoise_fused -- ride on the last pixel pass there is: setMode(RGB) behind NL-means, or one exposure pass
    int chain_n = 0;
    float chain_scale[2], chain_black[2];
    if (ecomp > 0 && !fuse_post) { chain_scale[chain_n] = (float)std::pow(2.0, -ecomp); chain_black[chain_n] = 0.f; ++chain_n; }
    if (fu.tail_on) { chain_scale[chain_n] = fu.tail_scale; chain_black[chain_n] = fu.tail_black; ++chain_n; }
    bool chained = false;
    PixArgs a = {};
    for (int k = 0; k < 3; ++k) a.dst[k] = d.p[k];
    a.dst_stride = d.stride; a.w = d.w; a.h = d.h;
    if (p->smoothing_enabled) {
        {
            StageScope scope_(ctx, "denoise::denoiseGuidedSmoothing");
            if (p->guided_chroma_radius != 0 && (rc = denoise_guided_smoothing_dev(ctx, d, ws, p->guided_chroma_radius, scale))) return rc;   // ipsmoothing.cc:877-879
        }
        if (p->nl_strength) {
            for (int k = 0; k < 3; ++k) a.mul[k] = wsf[3 + k];
            a.do_clip = 0;
            HIPCHK(ctx, launch_yuv_mode(a, ctx->stream));
            {
                StageScope scope_(ctx, "denoise::NLMeans");
                artgpu_plane y = {d.p[1], d.w, d.h, (int64_t)d.stride * 4, 1};
                if ((rc = nlm_dev(ctx, &y, 65535.f, p->nl_strength, p->nl_detail, (float)scale))) return rc;
            }
            a.do_clip = 1;
            a.chain_n = chain_n;
            for (int k = 0; k < chain_n; ++k) { a.chain_scale[k] = chain_scale[k]; a.chain_black[k] = chain_black[k]; }
            HIPCHK(ctx, launch_yuv_mode(a, ctx->stream));
            chained = true;
        }
    }
    if (chain_n && !chained) {
        a.exp_scale = chain_scale[0]; a.black = chain_black[0];
        a.chain_n = chain_n - 1;
        if (chain_n > 1) { a.chain_scale[0] = chain_scale[1]; a.chain_black[0] = chain_black[1]; }
        HIPCHK(ctx, launch_exposure(a, ctx->stream));
    }
    return ARTGPU_OK;
}

} // namespace

extern "C" {

int artgpu_rgb_denoise(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_denoise_params *p, const float ws[9], const float *iws,
                       double expcomp, double scale, const artgpu_plane *ccalc, uint32_t flags,
                       float *nresi, float *highresi)
{
    StageScope scope_(ctx, "denoise::RGB_denoise");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !p || !ws) return fail(ctx, ARTGPU_EINVAL, "rgb_denoise: null argument");
    int rc = rgb_denoise_args_ok(ctx, p, iws != nullptr, scale);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "rgb_denoise"))) return rc;
    if ((rc = rgb_denoise_dev(ctx, d, p, ws, iws, expcomp, scale, ccalc, flags, nresi, highresi, DnFusion{}))) return rc;
    return unbind_rgb(ctx, img, &d);
}

// ---------------------------------------------------------------------------------------------
// chroma noise-curve map + ImProcFunctions::denoise
// ---------------------------------------------------------------------------------------------
int artgpu_noise_curve_lut(const double *points, int npoints, float lut[501], float *sum)
{
    if (!points || npoints < 0 || !lut) return ARTGPU_EINVAL;
    const float s = noise_curve_lut(points, npoints, lut);
    if (sum) *sum = s;
    return ARTGPU_OK;
}

int artgpu_denoise_compute_params(artgpu_ctx *ctx, const artgpu_rgb *planes, int border, const float mul[3], int do_clip,
                                  const double cam_to_work[9], const double ws[9], double chrominance_auto_factor,
                                  artgpu_denoise_info_store *store, artgpu_denoise_params *dn)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!planes || !mul || !cam_to_work || !ws || !store || !dn) return fail(ctx, ARTGPU_EINVAL, "denoise_compute_params: null argument");
    const bool automatic = dn->chrominance_method == 1;
    if (store->valid || !automatic) {                       // ipdenoise.cc:802-809
        if (automatic) {
            dn->chrominance = store->chrominance * chrominance_auto_factor;
            dn->chrominance_red_green = store->chrominance_red_green * chrominance_auto_factor;
            dn->chrominance_blue_yellow = store->chrominance_blue_yellow * chrominance_auto_factor;
        }
        return ARTGPU_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB src;
    int rc;
    if ((rc = bind_rgb(ctx, planes, 1, true, &src, "denoise_compute_params(planes)")) || (rc = dn_compute_params_check(ctx, src.w, src.h, border))) return rc;
    return dn_compute_params_dev(ctx, src, border, mul, do_clip, cam_to_work, ws, chrominance_auto_factor, store, dn);
}

} // extern "C"

namespace artgpu { namespace api {

int dn_compute_params_check(artgpu_ctx *ctx, int W, int H, int border)
{
    if (border < 0) return fail(ctx, ARTGPU_EINVAL, "denoise_compute_params: border %d", border);
    const int widIm = W - 2 * border, heiIm = H - 2 * border;       // getFullSize
    if (widIm < 100 || heiIm < 100)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "denoise_compute_params: %dx%d is too small for the nine-crop layout (crops start 50 px in)", widIm, heiIm);
    return ARTGPU_OK;
}

// denoiseComputeParams with an empty store and AUTOMATIC chroma (ipdenoise.cc:810-1010), after dn_compute_params_check
int dn_compute_params_dev(artgpu_ctx *ctx, const DevRGB &src, int border, const float mul[3], int do_clip, const double cam_to_work[9], const double ws[9],
                          double chrominance_auto_factor, artgpu_denoise_info_store *store, artgpu_denoise_params *dn)
{
    int rc;
    const int widIm = src.w - 2 * border, heiIm = src.h - 2 * border;       // getFullSize
    const int crW = widIm / 2, crH = heiIm / 2;                              // Tile_calc returns one tile: tileWskip = widIm (L836,875-876)
    const int coordW[3] = {50, widIm / 2 - crW / 2, widIm - crW - 50}, coordH[3] = {50, heiIm / 2 - crH / 2, heiIm - crH - 50};
    const int wid = (crW + 1) / 2, hei = (crH + 1) / 2, levwav = 5, nsub = 3 * levwav;   // levwav = max(2, 5 - ceil(log(1)))
    const size_t n = (size_t)crW * crH, n2 = (size_t)wid * hei;
    if (!ctx->aux) {
        HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking));
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->aux_ev[0], hipEventDisableTiming));
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->aux_ev[1], hipEventDisableTiming));
    }

    DnInfoArgs a = {};
    float *tabs, *gamlut, *histo_f, *res;
    DevDecomp Cd = {};
    Cd.w = crW; Cd.h = crH; Cd.w2 = wid; Cd.h2 = hei; Cd.n = n2; Cd.nlevels = levwav;
    if ((rc = lab_tabs_dev(ctx, &tabs)) || (rc = pool_get(ctx, P_A, n * 4, &a.A)) || (rc = pool_get(ctx, P_B, n * 4, &a.B)) ||
        (rc = pool_get(ctx, P_CBANDS, (size_t)nsub * n2 * 4, &Cd.bands)) || (rc = pool_get(ctx, P_CLOW0, n2 * 4, &Cd.low[0])) ||
        (rc = pool_get(ctx, P_CLOW1, n2 * 4, &Cd.low[1])) || (rc = pool_get(ctx, P_SF, (size_t)27 * n2 * 4, &a.maps)) ||
        (rc = pool_get(ctx, P_HISTO, (size_t)nsub * (65536 + MAD_SCRATCH_INTS_PER_BAND) * 4, &histo_f)) || (rc = pool_get(ctx, P_GAM, 2 * 65536 * 4, &gamlut)) ||
        (rc = pool_get(ctx, P_DNINFO, (9 * 32 + 9 * 8) * 4, &res)))
        return rc;
    for (int k = 0; k < 3; ++k) { a.src[k] = src.p[k]; a.mul[k] = mul[k]; }
    a.stride = src.stride; a.do_clip = do_clip ? 1 : 0;
    for (int wcr = 0; wcr < 3; ++wcr)
        for (int hcr = 0; hcr < 3; ++hcr) { a.sx[hcr * 3 + wcr] = coordW[wcr] + border; a.sy[hcr * 3 + wcr] = coordH[hcr] + border; }   // transformRect adds the border
    a.crW = crW; a.crH = crH; a.wid = wid; a.hei = hei;
    for (int k = 0; k < 9; ++k) { a.mat[k] = cam_to_work[k]; a.wp[k] = (float)ws[k]; }
    a.cachef = tabs; a.cachefy = tabs + 65536; a.gamcurve = gamlut;
    // RGB_denoise_infoGamCurve (ipdenoise.cc:209-224), raw: gamma as given
    a.gam = (float)dn->gamma; a.gamthresh = 0.001f;
    a.gamslope = (float)(std::exp(std::log(static_cast<double>(a.gamthresh)) / a.gam) / a.gamthresh);
    { const double expcomp = std::log(5.f) / std::log(2.f); a.gain = std::pow(2.0f, float(expcomp)); }     // L936, L291
    a.stats = res + 9 * 32;
    ctx->gam_tab = nullptr;                    // (the slot RGB_denoise keeps its gamma pair in)
    HIPCHK(ctx, launch_gamma_lut(gamlut, a.gam, a.gamthresh, a.gamslope, 65535.f, 32768.f, ctx->stream));

    // maps of all nine crops, then their serial statistics on the second stream while this one decomposes
    HIPCHK(ctx, launch_dninfo_maps(a, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->aux_ev[0], ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->aux, ctx->aux_ev[0], 0));
    HIPCHK(ctx, launch_dninfo_stats(a, ctx->aux));
    HIPCHK(ctx, hipEventRecord(ctx->aux_ev[1], ctx->aux));
    int *histo = reinterpret_cast<int *>(histo_f);
    for (int k = 0; k < 9; ++k) {
        a.crop = k;
        HIPCHK(ctx, launch_dninfo_ab(a, ctx->stream));
        if ((rc = decompose_dev(ctx, Cd, a.A))) return rc;
        HIPCHK(ctx, launch_mad(Cd.bands, n2, nsub, histo, res + k * 32, ctx->stream));
        if ((rc = decompose_dev(ctx, Cd, a.B))) return rc;
        HIPCHK(ctx, launch_mad(Cd.bands, n2, nsub, histo, res + k * 32 + 16, ctx->stream));
    }
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->aux_ev[1], 0));
    float host[9 * 32 + 9 * 8];
    HIPCHK(ctx, hipMemcpyAsync(host, res, sizeof host, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));

    const bool aggressive = dn->aggressive != 0;
    float info[9][16] = {};
    for (int k = 0; k < 9; ++k) {
        float bs[6];
        dninfo_band_stats(host + k * 32, host + k * 32 + 16, nsub, aggressive, bs);
        const float *st = host + 9 * 32 + k * 8;
        int nry, nsk;
        memcpy(&nry, st + 4, 4); memcpy(&nsk, st + 5, 4);
        const int nc = (int)n2;                              // ShrinkAll_info, lvl == 1 (FTblockDN.cc:1266-1288)
        for (int j = 0; j < 5; ++j) info[k][j] = bs[j];
        info[k][5] = st[0] / nc;                             // chromina
        info[k][6] = st[1] / nc;                             // lumema
        info[k][7] = nry > 0 ? st[2] / nry : 0.f;            // redyel
        info[k][8] = nsk > 0 ? st[3] / nsk : 0.f;            // skinc
        info[k][9] = static_cast<float>(nsk) / static_cast<float>(nc);
        info[k][10] = bs[5];
    }
    float out3[3];
    dninfo_reduce(info, aggressive, store->ch_M, store->max_r, store->max_b, out3);
    store->chrominance = out3[0]; store->chrominance_red_green = out3[1]; store->chrominance_blue_yellow = out3[2];
    dn->chrominance = store->chrominance * chrominance_auto_factor;
    dn->chrominance_red_green = store->chrominance_red_green * chrominance_auto_factor;
    dn->chrominance_blue_yellow = store->chrominance_blue_yellow * chrominance_auto_factor;
    store->valid = 1;
    for (int k = 0; k < 9; ++k) memcpy(store->crop_info[k], info[k], sizeof info[k]);
    return ARTGPU_OK;
}

int denoise_tool_check(artgpu_ctx *ctx, int w, int h, const artgpu_denoise_tool_params *p, const double *iws, double scale)
{
    int rc;
    if ((rc = rgb_denoise_args_ok(ctx, &p->dn, iws != nullptr, scale))) return rc;
    if ((rc = rgb_denoise_size_ok(ctx, w, h))) return rc;
    if (!p->smoothing_enabled) return ARTGPU_OK;
    if (p->guided_chroma_radius != 0 && (rc = denoise_guided_smoothing_check(ctx, w, h, p->guided_chroma_radius, scale))) return rc;
    return p->nl_strength ? nlm_check(ctx, w, h) : ARTGPU_OK;
}

int improc_denoise_dev(artgpu_ctx *ctx, const DevRGB &d, const DevRGB *dem, const artgpu_denoise_fusion *fu, bool fuse_ok, const artgpu_denoise_tool_params *p,
                       const double ws[9], const double *iws, double ecomp, double scale, const double *calclum_mat, const float *noise_c_curve, uint32_t flags)
{
    // what of the neighbouring stages can really live inside the tool's pixel passes: the wavelet denoise has to run (its first pass reads the
    // image, its last one writes it), on device planes; the exposure only when nothing stands between RGB_denoise and it.
    // `dn_runs0` asks the caller's strengths, denoise_tool_dev's `dn_runs` the ones adjust_params has scaled.  adjust_params maps 0 to 0 and
    // any other strength to another one of the same sign, so the two agree for every strength and scale a caller can mean; they part only
    // where the arithmetic underflows (a denormal strength, an infinite scale).  Both are kept as they were.
    const bool dn_runs0 = !(p->dn.luminance == 0 && p->dn.chrominance == 0 && !noise_curve_on(noise_c_curve));
    const bool fuse_gi = dem && dn_runs0 && fuse_ok;
    const bool fuse_exp = fu && fu->exposure_enabled && dn_runs0 && fuse_ok && !p->smoothing_enabled;
    // with guided smoothing / NL-means behind the wavelet denoise the tool's last pixel pass is setMode(RGB) or its own expcomp(-ecomp):
    // the exposure rides on that one
    const bool tail_exp = fu && fu->exposure_enabled && dn_runs0 && fuse_ok && p->smoothing_enabled && (p->nl_strength || ecomp > 0);
    int rc;
    DnFusion f = {};
    if (fuse_gi) {
        GetImageFuse &g = f.gi;
        g.on = 1;
        for (int k = 0; k < 3; ++k) { g.src[k] = dem->p[k]; g.mul[k] = fu->mul[k]; }
        g.stride = dem->stride;
        g.sx1 = fu->sx1; g.sy1 = fu->sy1;
        g.do_clip = fu->do_clip ? 1 : 0; g.has_mat = fu->cam_to_work ? 1 : 0;
        for (int k = 0; k < 9; ++k) g.mat[k] = fu->cam_to_work ? fu->cam_to_work[k] : 0.0;
    } else if (dem) {                                          // the separate pass it stands for
        StageScope scope_(ctx, "RawImageSource::getImage");
        if ((rc = get_image_dev(ctx, *dem, d, fu->sx1, fu->sy1, 1, fu->mul, fu->do_clip, fu->cam_to_work))) return rc;
    }
    if (fuse_exp) { f.exp_on = 1; f.exp_scale = fu->exp_scale; f.exp_black = fu->black; }
    if (tail_exp) { f.tail_on = 1; f.tail_scale = fu->exp_scale; f.tail_black = fu->black; }
    if ((rc = denoise_tool_dev(ctx, d, p, ws, iws, ecomp, scale, calclum_mat, noise_c_curve, flags, f))) return rc;
    // the exposure that could not be fused follows as its own pass
    if (fu && fu->exposure_enabled && !fuse_exp && !tail_exp) {
        StageScope scope_(ctx, "ImProcFunctions::expcomp");
        return exposure_dev(ctx, d, fu->exp_scale, fu->black);
    }
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_denoise_chroma_map(artgpu_ctx *ctx, const artgpu_rgb *img, const double *calclum_mat, const double ws[9],
                              const float noise_c_curve[501], artgpu_plane *ccalc)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !ws || !noise_c_curve || !ccalc) return fail(ctx, ARTGPU_EINVAL, "denoise_chroma_map: null argument");
    DevRGB d;
    int rc = bind_rgb(ctx, img, 4, true, &d, "denoise_chroma_map");
    if (rc) return rc;
    const int wid = (d.w + 1) / 2, hei = (d.h + 1) / 2;
    if (!plane_ok(ccalc) || ccalc->w != wid || ccalc->h != hei) return fail(ctx, ARTGPU_EINVAL, "denoise_chroma_map: ccalc must be %dx%d", wid, hei);
    float *map;
    if ((rc = chroma_map_dev(ctx, d.p, d.stride, d.w, d.h, calclum_mat, ws, noise_c_curve, GetImageFuse{}, &map))) return rc;
    HIPCHK(ctx, hipMemcpy2DAsync(ccalc->p, (size_t)ccalc->row_stride_bytes, map, (size_t)wid * 4, (size_t)wid * 4, hei,
                                 ccalc->on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    if (!ccalc->on_device) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ARTGPU_OK;
}

int artgpu_improc_denoise(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_denoise_tool_params *p, const double ws[9], const double *iws,
                          double ecomp, double scale, const double *calclum_mat, const float *noise_c_curve, uint32_t flags)
{
    return artgpu_improc_denoise_fused(ctx, img, nullptr, p, ws, iws, ecomp, scale, calclum_mat, noise_c_curve, flags);
}

int artgpu_improc_denoise_fused(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_denoise_fusion *fu, const artgpu_denoise_tool_params *p,
                                const double ws[9], const double *iws, double ecomp, double scale, const double *calclum_mat,
                                const float *noise_c_curve, uint32_t flags)
{
    StageScope scope_(ctx, "ImProcFunctions::denoise");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !p || !ws) return fail(ctx, ARTGPU_EINVAL, "improc_denoise: null argument");
    const artgpu_rgb *dm = fu ? fu->demosaiced : nullptr;
    if (dm && (!plane_ok(&dm->r) || !plane_ok(&dm->g) || !plane_ok(&dm->b) || dm->g.row_stride_bytes != dm->r.row_stride_bytes || dm->b.row_stride_bytes != dm->r.row_stride_bytes ||
               fu->sx1 < 0 || fu->sy1 < 0 || fu->sx1 + img->r.w > dm->r.w || fu->sy1 + img->r.h > dm->r.h))
        return fail(ctx, ARTGPU_EINVAL, "improc_denoise_fused: crop %dx%d+%d+%d outside the demosaiced planes", img->r.w, img->r.h, fu->sx1, fu->sy1);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // host planes: stage once (the image itself unless getImage is about to write it), run the whole tool on the staged copy, copy back; device
    // planes are used in place
    const bool fuse_ok = img->r.on_device && (!dm || (dm->r.on_device && dm->g.on_device && dm->b.on_device));
    DevRGB d, dem;
    int rc;
    if ((dm && (rc = bind_rgb(ctx, dm, 1, true, &dem, "get_image(planes)"))) || (rc = bind_rgb(ctx, img, 4, !dm, &d, "improc_denoise")) ||
        (rc = denoise_tool_check(ctx, d.w, d.h, p, iws, scale)) ||
        (rc = improc_denoise_dev(ctx, d, dm ? &dem : nullptr, fu, fuse_ok, p, ws, iws, ecomp, scale, calclum_mat, noise_c_curve, flags)))
        return rc;
    return unbind_rgb(ctx, img, &d);
}

} // extern "C"
