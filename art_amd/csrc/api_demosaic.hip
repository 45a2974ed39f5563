// art_amd/csrc/api_demosaic.hip -- the demosaicers behind the C ABI: RawImageSource::demosaic for Bayer sensors (AMaZE, RCD, VNG4, the
// dual demosaic's second pass and blend), border_interpolate2, and xtrans_interpolate.  The kernels are amaze*.hip's, rcd_stream.hip's,
// vng4.hip's, dualdemosaic.hip's, border.hip's and xtrans.hip's.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace {

int launch_border(artgpu_ctx *ctx, const DevImage &d, int W, int H, unsigned filters, int bord)
{
    if (bord <= 0) return ARTGPU_OK;
    if (W <= 2 * bord || H <= 2 * bord) return fail(ctx, ARTGPU_EUNSUPPORTED, "border_interpolate2: image %dx%d too small for border %d", W, H, bord);
    BorderArgs b;
    b.raw = d.raw; b.raw_stride = d.raw_stride;
    b.red = d.r; b.green = d.g; b.blue = d.b; b.out_stride = d.out_stride;
    b.W = W; b.H = H; b.bord = bord; b.filters = filters;
    const long long total = 2LL * bord * H + 2LL * bord * (W - 2 * bord);
    const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    HIPCHK(ctx, launch_border_interpolate2(b, grid, ctx->stream));
    return ARTGPU_OK;
}

struct DualReq { double *contrast; int auto_contrast; int second; };

// RawImageSource::vng4_demosaic on device planes (vng4_demosaic_RT.cc:62-397)
static int vng4_dev(artgpu_ctx *ctx, const float *raw, size_t raw_stride, float *r, float *g, float *b, size_t out_stride, int W, int H, uint32_t filters)
{
    if (W < 16 || H < 16) return fail(ctx, ARTGPU_EUNSUPPORTED, "vng4: image %dx%d smaller than 16x16", W, H);
    float *image, *codef;
    int rc;
    if ((rc = pool_get(ctx, P_BLOCKS, (size_t)W * H * 16, &image)) || (rc = pool_get(ctx, P_DTAB, 16 * VNG4_CODE_INTS * 4, &codef))) return rc;
    Vng4Args a = {};
    a.raw = raw; a.raw_stride = raw_stride; a.red = r; a.green = g; a.blue = b; a.out_stride = out_stride;
    a.image = image; a.code = reinterpret_cast<const int *>(codef); a.w = W; a.h = H; a.filters = filters; a.prefilters = vng4_prefilters(filters);
    std::vector<int> codes(16 * VNG4_CODE_INTS, 0);
    vng4_build_code(a.prefilters, W, codes.data());
    HIPCHK(ctx, hipMemcpyAsync(codef, codes.data(), codes.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));     // `codes` goes out of scope
    HIPCHK(ctx, launch_vng4(a, ctx->stream));
    return ARTGPU_OK;
}
// dual_demosaic_RT.cc:99-152 after the first demosaicer: L, buildBlendMask (rt_algo.cc:315-498), bilinear blend
static int dual_blend_dev(artgpu_ctx *ctx, const DevImage &d, int W, int H, uint32_t filters, DualReq *req)
{
    const size_t n = (size_t)W * H;
    float *tabs, *L, *blend, *var;
    int rc;
    if ((rc = lab_tabs_dev(ctx, &tabs)) || (rc = pool_get(ctx, P_DMASK, n * 4, &L)) || (rc = pool_get(ctx, P_CCMAP, n * 4, &blend))) return rc;
    DualArgs a = {};
    a.rgb[0] = d.r; a.rgb[1] = d.g; a.rgb[2] = d.b; a.stride = d.out_stride;
    a.raw = d.raw; a.raw_stride = d.raw_stride; a.w = W; a.h = H; a.filters = filters;
    a.cachefy = tabs + 65536; a.L = L; a.blend = blend;
    HIPCHK(ctx, launch_rgb2l(a, ctx->stream));
    float thr = (float)(*req->contrast / 100.0);
    if (req->auto_contrast) {
        // the reference's two-pass search for the flattest tile (rt_algo.cc:317-432): tile statistics on the device, the serial
        // first-minimum scan over them on the host
        std::vector<float> host;
        float *res;
        auto stats = [&](int nH, int nW, int y0, int x0, int step, int ts, int *mi, int *mj, float *minvar) -> int {
            *mi = *mj = 0; *minvar = INFINITY;
            if (nH <= 0 || nW <= 0) return ARTGPU_OK;
            const size_t cnt = (size_t)nH * nW;
            int rc2 = pool_get(ctx, P_TMP, cnt * 4, &var);
            if (rc2) return rc2;
            HIPCHK(ctx, launch_tile_stats(a, nH, nW, y0, x0, step, ts, var, ctx->stream));
            host.resize(cnt);
            HIPCHK(ctx, hipMemcpyAsync(host.data(), var, cnt * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            for (int i = 0; i < nH; ++i)
                for (int j = 0; j < nW; ++j)
                    if (host[(size_t)i * nW + j] < *minvar) { *minvar = host[(size_t)i * nW + j]; *mi = i; *mj = j; }
            return ARTGPU_OK;
        };
        auto threshold_of = [&](int ty, int tx, int ts, float *out_thr) -> int {
            int rc2 = pool_get(ctx, P_MAD, 64, &res);
            if (rc2) return rc2;
            HIPCHK(ctx, launch_contrast_threshold(a, ty, tx, ts, res, ctx->stream));
            HIPCHK(ctx, hipMemcpyAsync(out_thr, res, 4, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            return ARTGPU_OK;
        };
        for (int pass = 0; pass < 2; ++pass) {
            const int ts = 80 / (pass + 1), skip = pass == 0 ? ts : ts / 4;
            const int nW = W / skip - 3 * pass, nH = H / skip - 3 * pass;
            int mi, mj; float minvar;
            if ((rc = stats(nH, nW, 0, 0, skip, ts, &mi, &mj, &minvar))) return rc;
            if (minvar <= 1.f || pass == 1) {
                const int minY = skip * mi, minX = skip * mj;
                if (pass == 0) {
                    if ((rc = threshold_of(minY, minX, ts, &thr))) return rc;
                    break;
                }
                const int y0 = std::max(minY - skip, 0), x0 = std::max(minX - skip, 0);
                const int y1 = std::min(minY + skip, H - ts), x1 = std::min(minX + skip, W - ts);
                int mi2, mj2; float minvar2;
                if ((rc = stats(y1 - y0 + 1, x1 - x0 + 1, y0, x0, 1, ts, &mi2, &mj2, &minvar2))) return rc;
                if (minvar2 <= 8.f) { if ((rc = threshold_of(y0 + mi2, x0 + mj2, ts, &thr))) return rc; }
                else thr = 0.f;
            }
        }
    }
    *req->contrast = thr * 100.f;
    a.threshold = thr;
    HIPCHK(ctx, launch_blend_mask(a, ctx->stream));
    if (thr != 0.f) {
        artgpu_plane bp = {blend, W, H, (int64_t)W * 4, 1};
        if ((rc = artgpu_gaussian_blur(ctx, &bp, 2.0))) return rc;      // rt_algo.cc:492
    }
    if (req->second == ARTGPU_DUAL_VNG4) {
        // vng4_demosaic into temporaries, then all three channels of every pixel (dual_demosaic_RT.cc:128-148)
        float *t;
        if ((rc = pool_get(ctx, P_SF, 3 * n * 4, &t))) return rc;
        if ((rc = vng4_dev(ctx, d.raw, d.raw_stride, t, t + n, t + 2 * n, (size_t)W, W, H, filters))) return rc;
        DevImage tmp = {d.raw, d.raw_stride, t, t + n, t + 2 * n, (size_t)W, false};
        if ((rc = launch_border(ctx, tmp, W, H, filters, 3))) return rc;
        HIPCHK(ctx, launch_dual_blend_planes(a, t, t + n, t + 2 * n, (size_t)W, ctx->stream));
        return ARTGPU_OK;
    }
    HIPCHK(ctx, launch_bilinear_blend(a, ctx->stream));
    return ARTGPU_OK;
}

// the events of artgpu_get_timings, recorded beside the launches (ev[0] .. ev[2]): waited for and read when the stage has been queued
int demosaic_read_timings(artgpu_ctx *ctx, bool has_border)
{
    HIPCHK(ctx, hipEventSynchronize(ctx->ev[2]));
    HIPCHK(ctx, hipEventElapsedTime(&ctx->last.demosaic_ms, ctx->ev[0], ctx->ev[1]));
    if (!has_border) { ctx->last.border_ms = 0.f; ctx->last.total_ms = ctx->last.demosaic_ms; return ARTGPU_OK; }
    HIPCHK(ctx, hipEventElapsedTime(&ctx->last.border_ms, ctx->ev[1], ctx->ev[2]));
    HIPCHK(ctx, hipEventElapsedTime(&ctx->last.total_ms, ctx->ev[0], ctx->ev[2]));
    return ARTGPU_OK;
}

// RawImageSource::demosaic for a Bayer sensor on a bound image, after demosaic_bayer_check; dual: the dual demosaic's second pass and blend behind it
static int demosaic_bayer_run(artgpu_ctx *ctx, const DevImage &d, int W, int H, int method, uint32_t filters, double initial_gain, int border, DualReq *dual)
{
    int rc;
    if (ctx->timing) HIPCHK(ctx, hipEventRecord(ctx->ev[0], ctx->stream));

    int bord = 0;
    if (method == ARTGPU_BAYER_AMAZE) {
        const int nty = (H + 16 + AMAZE_STEP - 1) / AMAZE_STEP, ntx = (W + 16 + AMAZE_STEP - 1) / AMAZE_STEP;
        const int ntiles = nty * ntx;
        // Tile classes (amaze_demosaic_RT.cc:182-334).  Tiles that write no pixel (the clipped tile is at most 32 wide / high) are
        // skipped.  Tiles that are 160 columns wide go to the LDS streaming kernel (amaze_stream.hip) unless their mirrored bottom /
        // right border fill over-runs the tile row or the cfa plane in the reference (it always writes 16 rows / columns from the
        // frame edge: exact only when a full-size tile ends 16 pixels past the frame); everything else -- narrower tiles, those
        // over-run tiles and streamed tiles whose Nyquist sites do not fit the stream's assumption -- is done by the arena kernel
        // (amaze.hip), which reproduces the reference's buffer layout literally.
        const int mode = ctx->shared.opt_amaze_path;
        if (ctx->amz_w != W || ctx->amz_h != H || ctx->amz_mode != mode) {
            std::vector<int> st, ar;
            for (int ty = 0; ty < nty; ++ty)
                for (int tx = 0; tx < ntx; ++tx) {
                    const int top = -16 + ty * AMAZE_STEP, left = -16 + tx * AMAZE_STEP;
                    const int rr1 = std::min(top + AMAZE_TS, H + 16) - top, cc1 = std::min(left + AMAZE_TS, W + 16) - left;
                    if (rr1 <= 32 || cc1 <= 32) continue;
                    // streamable: 160 columns wide (any height), and the 16 mirrored rows / columns the reference appends at the
                    // bottom / right frame edge end exactly at the tile's edge
                    const bool wide = cc1 == AMAZE_TS && (left + AMAZE_TS <= W || left + AMAZE_TS == W + 16);
                    const bool rows_ok = rr1 < AMAZE_TS || top + AMAZE_TS <= H || top + AMAZE_TS == H + 16;
                    (mode == 0 && wide && rows_ok ? st : ar).push_back(ty * ntx + tx);
                }
            // ... + the redo queue: 4 header ints (reserved, taken, pad) and one 64-bit word per streamed tile, 16-byte aligned
            const size_t nfixed = ((st.size() + (1 + ar.size()) + (1 + ar.size() + st.size()) + 3) / 4) * 4;
            const size_t nints = nfixed + 4 + 2 * st.size() + 8;
            if ((rc = ensure(ctx, &ctx->amz_lists, &ctx->amz_lists_bytes, nints * sizeof(int)))) return rc;
            std::vector<int> hostbuf;
            hostbuf.insert(hostbuf.end(), st.begin(), st.end());
            hostbuf.push_back((int)ar.size());
            hostbuf.insert(hostbuf.end(), ar.begin(), ar.end());
            HIPCHK(ctx, hipMemcpyAsync(ctx->amz_lists, hostbuf.data(), hostbuf.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // hostbuf goes out of scope
            ctx->amz_w = W; ctx->amz_h = H; ctx->amz_mode = mode;
            ctx->amz_nstream = (int)st.size(); ctx->amz_narena = (int)ar.size();
        }
        int *const d_stream = reinterpret_cast<int *>(ctx->amz_lists);
        int *const d_templ = d_stream + ctx->amz_nstream;
        int *const d_work = d_templ + 1 + ctx->amz_narena;
        const size_t nfixed = (((size_t)ctx->amz_nstream + (1 + ctx->amz_narena) + (1 + ctx->amz_narena + ctx->amz_nstream) + 3) / 4) * 4;
        int *const d_queue = d_stream + nfixed;                                          // header (4 ints), then the 64-bit entries
        unsigned long long *const d_qwords = reinterpret_cast<unsigned long long *>(d_queue + 4);
        const float clip_pt = (float)(1.0 / initial_gain);   // amaze_demosaic_RT.cc:53-54
        const float clip_pt8 = (float)(0.8 / initial_gain);
        // The arena kernel runs twice.  EARLY, beside the stream kernel on a stream of its own: the tiles the stream cannot take (for a
        // frame width that is not 32 + a multiple of 128 that is a whole column of narrow tiles: 43 of 2860 at 8256 x 5504) -- they are
        // one workgroup each and a chain of twenty HBM round trips, 0.45 ms that used to follow the stream kernel; now they hold a few CUs
        // back for that long while the stream workgroups on the other CUs take tiles from the shared counter.  LATE, behind both: whatever
        // the stream handed back (tiles whose Nyquist sites did not fit its assumption and found no taker in the redo queue), normally nothing.
        const bool split = mode == 1 && ctx->shared.opt_amaze_split;
        const bool early = ctx->amz_nstream > 0 && ctx->amz_narena > 0 && ctx->shared.opt_amaze_overlap;
        const int nlist_max = ctx->amz_narena + ctx->amz_nstream;
        const int cap = split ? MAX_TILE_WORKGROUPS : 768;
        // (the per-phase profiling path runs one arena per tile of the grid, the tiles that write nothing included)
        const int grid = split ? std::min(ntiles, cap) : std::max(1, std::min(nlist_max, cap));
        rc = ensure(ctx, &ctx->arena, &ctx->arena_bytes, (size_t)grid * AMAZE_ARENA_FLOATS * sizeof(float));
        if (rc) return rc;
        if ((rc = ensure(ctx, &ctx->bbox, &ctx->bbox_bytes, (size_t)grid * 4 * sizeof(int)))) return rc;
        AmazeArgs a;
        a.raw = d.raw; a.raw_stride = d.raw_stride;
        a.red = d.r; a.green = d.g; a.blue = d.b; a.out_stride = d.out_stride;
        a.arena = ctx->arena;
        a.W = W; a.H = H; a.ntx = ntx; a.ntiles = ntiles;
        a.filters = filters;
        a.clip_pt = clip_pt;
        a.clip_pt8 = clip_pt8;
        a.bbox = reinterpret_cast<int *>(ctx->bbox);
        // Arena regions that have read-before-write positions on full tiles and therefore must be cleared per tile: vcd, hcd,
        // vcdalt, hcdalt, cddiffsq, nyquist (bits 4-8, 15): on a full tile every other position is written before it is read, for
        // every CFA phase, because the phase loops cover fixed index ranges (derivation: DESIGN.md section 10).
        // tests/test_gpu_demosaic.py re-checks it with poisoned arenas (artgpu_set_option "amaze_poison").  Partial tiles clear everything.
        a.zero_mask = (unsigned)ctx->shared.opt_amaze_zero_mask;
        // ... and of the five full-size planes among them only positions within a few pixels of the tile edge (plus the gap behind each
        // plane): a frame of 4 already passes the poison test, 16 (the discarded tile border) is used.  0: whole planes.
        a.zero_frame = ctx->shared.opt_amaze_zero_frame;
        a.split = split ? 1 : 0;
        a.queue_words = d_qwords;
        a.queue_counters = reinterpret_cast<int *>(d_qwords + ctx->amz_nstream);
        if (ctx->shared.opt_amaze_poison >= 0)   // test hook: fill the arenas with a byte pattern first
            HIPCHK(ctx, hipMemsetAsync(ctx->arena, ctx->shared.opt_amaze_poison, (size_t)grid * AMAZE_ARENA_FLOATS * sizeof(float), ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(d_queue, 0, (4 + 2 * (size_t)ctx->amz_nstream + 8) * sizeof(int), ctx->stream));   // + the 8 counters behind it
        SideStreamJoin amz_join;
        if (early) {
            // the working list starts empty (the stream appends to it), the static tiles are taken from the template
            HIPCHK(ctx, hipMemsetAsync(d_work, 0, sizeof(int), ctx->stream));
            if (!ctx->amz_side) {
                HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->amz_side, hipStreamNonBlocking));
                for (int k = 0; k < 2; ++k) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->amz_ev[k], hipEventDisableTiming));
            }
            // the STREAM kernel goes to the side stream, behind an event: the arena kernel is then the one the hardware starts first (the
            // other way round the persistent stream workgroups took every CU and the arena tiles waited for them to finish)
            HIPCHK(ctx, hipEventRecord(ctx->amz_ev[0], ctx->stream));          // the CFA plane, the cleared queue
            HIPCHK(ctx, hipStreamWaitEvent(ctx->amz_side, ctx->amz_ev[0], 0));
            amz_join.arm(ctx->amz_side);
            a.tile_list = d_templ + 1; a.tile_count = d_templ;
            a.queue_hdr = nullptr;
            HIPCHK(ctx, launch_amaze(a, std::min(ctx->amz_narena, cap), ctx->stream));
        } else {
            HIPCHK(ctx, hipMemcpyAsync(d_work, d_templ, (size_t)(1 + ctx->amz_narena) * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
        }
        if (ctx->amz_nstream > 0) {
            AmazeStreamArgs sa;
            sa.raw = d.raw; sa.raw_stride = d.raw_stride;
            sa.red = d.r; sa.green = d.g; sa.blue = d.b; sa.out_stride = d.out_stride;
            sa.W = W; sa.H = H; sa.ntx = ntx;
            sa.filters = filters;
            sa.clip_pt = clip_pt; sa.clip_pt8 = clip_pt8;
            const unsigned f00 = (filters >> 0) & 3, f01 = (filters >> 2) & 3;   // FC(0,0), FC(0,1)
            sa.g00 = (int)(f00 & 1);
            sa.ey = f00 == 1 ? (f01 == 0 ? 0 : 1) : (f00 == 0 ? 0 : 1);        // row of the red sites (L1381-1386: ey)
            sa.tiles = d_stream; sa.ntiles = ctx->amz_nstream;
            sa.fallback = d_work;
            sa.queue_hdr = d_queue; sa.queue_words = d_qwords;
            // persistent workgroups, one per CU (the kernel needs almost all of a CU's LDS): each streams tiles back to back
            if (ctx->num_cus <= 0) {
                hipDeviceProp_t prop;
                HIPCHK(ctx, hipGetDeviceProperties(&prop, ctx->device));
                ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
            }
            // One stream workgroup owns a CU (156 KB of LDS, sixteen waves at 122 registers) and the kernel is bound by instruction issue; the
            // FTblockDN passes of ANOTHER frame in flight are bound by memory and can do nothing with a CU the demosaic holds.  With frames in
            // flight (artgpu_batch_run lanes) the stream kernel therefore leaves 3/8 of the CUs to them: measured 3881 -> 4006 .. 4056 MP/s with two
            // frames in flight at 45 MP (scripts/r5_lanes.sh: 240 / 224 / 192 / 160 / 144 / 128 workgroups; one frame at a time: all CUs).
            // Option "amaze_grid" overrides.
            const int cu_auto = ctx->frames_in_flight > 1 ? std::max(1, ctx->num_cus * 5 / 8) : ctx->num_cus;
            const int cu_cap = ctx->shared.opt_amaze_grid > 0 ? std::min(ctx->shared.opt_amaze_grid, ctx->num_cus) : cu_auto;
            HIPCHK(ctx, launch_amaze_stream(sa, std::min(ctx->amz_nstream, cu_cap), early ? ctx->amz_side : ctx->stream));
        }
        if (early) {
            HIPCHK(ctx, hipEventRecord(ctx->amz_ev[1], ctx->amz_side));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->amz_ev[1], 0));    // the streamed tiles are written, the hand-back list is final
            amz_join.disarm();
        }
        // arena kernel over the listed tiles (the static ones unless they went early, plus whatever the stream handed back; the count is
        // read on the device)
        if (split) {               // one arena per tile, tiles 0..ntiles-1 (the empty ones write nothing)
            a.tile_list = nullptr; a.tile_count = nullptr;
            if (grid < ntiles) return fail(ctx, ARTGPU_EUNSUPPORTED, "amaze_split needs one arena per tile (%d tiles)", ntiles);
        } else {
            a.tile_list = d_work + 1; a.tile_count = d_work;
        }
        a.queue_hdr = (!split && ctx->amz_nstream > 0) ? d_queue : nullptr;
        HIPCHK(ctx, launch_amaze(a, split ? ntiles : grid, ctx->stream));
        bord = border < 4 ? 3 : 0; // amaze_demosaic_RT.cc:1587-1589
    } else if (method == ARTGPU_BAYER_VNG4) {
        if ((rc = vng4_dev(ctx, d.raw, d.raw_stride, d.r, d.g, d.b, d.out_stride, W, H, filters))) return rc;
        bord = 3; // vng4_demosaic_RT.cc:384
    } else {
        const int tileSizeN = RCD_TS - 2 * RCD_BORDER;      // the reference's tile grid (rcd_demosaic.cc:82-87)
        const int numTh = H / tileSizeN + ((H % tileSizeN) ? 1 : 0), numTw = W / tileSizeN + ((W % tileSizeN) ? 1 : 0);
        const int ntiles = numTh * numTw;
        {
            // persistent workgroups take tiles from a counter; as many as the CUs hold at once
            if (ctx->num_cus <= 0) {
                hipDeviceProp_t prop;
                HIPCHK(ctx, hipGetDeviceProperties(&prop, ctx->device));
                ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
            }
            if (!ctx->rcd_counter) HIPCHK(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->rcd_counter), 64));
            HIPCHK(ctx, hipMemsetAsync(ctx->rcd_counter, 0, sizeof(int), ctx->stream));
            RcdStreamArgs a;
            a.raw = d.raw; a.raw_stride = d.raw_stride;
            a.red = d.r; a.green = d.g; a.blue = d.b; a.out_stride = d.out_stride;
            a.W = W; a.H = H; a.numTw = numTw; a.ntiles = ntiles;
            a.filters = filters;
            a.vec2 = d.out_stride % 2 == 0 && (reinterpret_cast<uintptr_t>(d.r) | reinterpret_cast<uintptr_t>(d.g) | reinterpret_cast<uintptr_t>(d.b)) % 8 == 0;
            a.counter = ctx->rcd_counter;
            const int R = ctx->shared.opt_rcd_rows;
            HIPCHK(ctx, launch_rcd_stream(a, R, std::min(ntiles, ctx->num_cus * rcd_stream_workgroups_per_cu(R)), ctx->stream));
        }
        bord = RCD_BORDER; // rcd_demosaic.cc:342
    }
    if (ctx->timing) HIPCHK(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    rc = launch_border(ctx, d, W, H, filters, bord);
    if (rc) return rc;
    if (dual && (rc = dual_blend_dev(ctx, d, W, H, filters, dual))) return rc;
    if (ctx->timing) HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
    return ctx->timing ? demosaic_read_timings(ctx, true) : ARTGPU_OK;
}

// artgpu_demosaic_bayer and artgpu_dual_demosaic_bayer
static int demosaic_bayer_entry(artgpu_ctx *ctx, int method, const artgpu_plane *raw, uint32_t filters, double initial_gain, int border, artgpu_rgb *out, DualReq *dual)
{
    StageScope scope_(ctx, "RawImageSource::demosaic (Bayer)");
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(raw) || !out) return fail(ctx, ARTGPU_EINVAL, "demosaic_bayer: bad raw plane or null output");
    int rc;
    if ((rc = demosaic_bayer_check(ctx, method, filters, initial_gain, raw->w, raw->h))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevImage d;
    if ((rc = bind_images(ctx, raw, out, &d)) || (rc = demosaic_bayer_run(ctx, d, raw->w, raw->h, method, filters, initial_gain, border, dual))) return rc;
    return unbind_images(ctx, out, &d);
}

} // namespace

extern "C" {

int artgpu_demosaic_bayer(artgpu_ctx *ctx, int method, const artgpu_plane *raw, uint32_t filters,
                          double initial_gain, int border, artgpu_rgb *out)
{
    return demosaic_bayer_entry(ctx, method, raw, filters, initial_gain, border, out, nullptr);
}
int artgpu_dual_demosaic_bayer(artgpu_ctx *ctx, int method, int second, const artgpu_plane *raw, uint32_t filters, double initial_gain, int border,
                               double *contrast, int auto_contrast, artgpu_rgb *out)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (method == ARTGPU_BAYER_VNG4 || (second != ARTGPU_DUAL_BILINEAR && second != ARTGPU_DUAL_VNG4))
        return fail(ctx, ARTGPU_EUNSUPPORTED, "dual_demosaic_bayer: first demosaicer AMAZE or RCD, second BILINEAR or VNG4");
    if (!contrast || !(*contrast >= 0.0)) return fail(ctx, ARTGPU_EINVAL, "dual_demosaic_bayer: contrast must be >= 0");
    if (raw && (raw->w < 96 || raw->h < 96)) return fail(ctx, ARTGPU_EUNSUPPORTED, "dual_demosaic_bayer: image smaller than 96x96");
    DualReq req = {contrast, auto_contrast, second};
    // contrast == 0 without the automatic threshold: only the first demosaicer runs (dual_demosaic_RT.cc:43-71)
    return demosaic_bayer_entry(ctx, method, raw, filters, initial_gain, border, out, (*contrast == 0.0 && !auto_contrast) ? nullptr : &req);
}

int artgpu_border_interpolate2(artgpu_ctx *ctx, const artgpu_plane *raw, uint32_t filters, int lborders, artgpu_rgb *out)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(raw) || !out || lborders < 0) return fail(ctx, ARTGPU_EINVAL, "border_interpolate2: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevImage d;
    int rc = bind_images(ctx, raw, out, &d);
    if (rc) return rc;
    if (d.staged) {
        // host outputs: start from the caller's current contents so that only the frame changes
        const int W = raw->w, H = raw->h;
        artgpu_plane *op[3] = {&out->r, &out->g, &out->b};
        float *dst[3] = {d.r, d.g, d.b};
        for (int k = 0; k < 3; ++k)
            HIPCHK(ctx, hipMemcpy2DAsync(dst[k], (size_t)W * 4, op[k]->p, (size_t)op[k]->row_stride_bytes, (size_t)W * 4, H, hipMemcpyHostToDevice, ctx->stream));
    }
    rc = launch_border(ctx, d, raw->w, raw->h, filters, lborders);
    if (rc) return rc;
    return unbind_images(ctx, out, &d);
}

// ---------------------------------------------------------------------------------------------
// X-Trans demosaic
// ---------------------------------------------------------------------------------------------
int artgpu_demosaic_xtrans(artgpu_ctx *ctx, int passes, int use_cielab, const artgpu_plane *raw, const int32_t xtrans[36],
                           const float rgb_cam[12], artgpu_rgb *out)
{
    StageScope scope_(ctx, "RawImageSource::xtrans_interpolate");
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(raw) || !out || !xtrans || !rgb_cam) return fail(ctx, ARTGPU_EINVAL, "demosaic_xtrans: bad raw plane or null argument");
    int rc;
    // (the row bind_images gives the CFA plane: a device plane's own, a staged host plane's width)
    if ((rc = demosaic_xtrans_check(ctx, passes, xtrans, raw->w, raw->h, raw->on_device ? (size_t)(raw->row_stride_bytes / 4) : (size_t)raw->w))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevImage d;
    if ((rc = bind_images(ctx, raw, out, &d)) || (rc = demosaic_xtrans_dev(ctx, d, raw->w, raw->h, passes, use_cielab, xtrans, rgb_cam))) return rc;
    return unbind_images(ctx, out, &d);
}

} // extern "C"

namespace artgpu { namespace api {

int demosaic_bayer_check(artgpu_ctx *ctx, int method, uint32_t filters, double initial_gain, int W, int H)
{
    if (method != ARTGPU_BAYER_AMAZE && method != ARTGPU_BAYER_RCD && method != ARTGPU_BAYER_VNG4) return fail(ctx, ARTGPU_EUNSUPPORTED, "demosaic_bayer: method %d is not on the device path", method);
    if (!(initial_gain > 0.0)) return fail(ctx, ARTGPU_EINVAL, "demosaic_bayer: initial_gain must be > 0");
    // RGB Bayer only: the reference falls back to igv_interpolate for 4-colour CFAs (rcd_demosaic.cc:57-66)
    for (unsigned r = 0; r < 2; ++r)
        for (unsigned c = 0; c < 2; ++c)
            if (((filters >> ((((r << 1) & 14) + (c & 1)) << 1)) & 3) == 3) return fail(ctx, ARTGPU_EUNSUPPORTED, "demosaic_bayer: 4-colour CFA");
    if (W < 64 || H < 64) return fail(ctx, ARTGPU_EUNSUPPORTED, "demosaic_bayer: image %dx%d smaller than 64x64", W, H);
    return ARTGPU_OK;
}

int demosaic_bayer_dev(artgpu_ctx *ctx, const DevImage &d, int W, int H, int method, uint32_t filters, double initial_gain, int border)
{
    return demosaic_bayer_run(ctx, d, W, H, method, filters, initial_gain, border, nullptr);
}

int demosaic_xtrans_check(artgpu_ctx *ctx, int passes, const int32_t xtrans[36], int W, int H, size_t raw_stride)
{
    if (passes < 1 || passes > 4) return fail(ctx, ARTGPU_EINVAL, "demosaic_xtrans: passes must be 1..4");
    if (W < 64 || H < 64) return fail(ctx, ARTGPU_EUNSUPPORTED, "demosaic_xtrans: image %dx%d smaller than 64x64", W, H);
    int ngreen = 0;
    for (int i = 0; i < 36; ++i) {
        if (xtrans[i] < 0 || xtrans[i] > 2) return fail(ctx, ARTGPU_EINVAL, "demosaic_xtrans: colour map entries must be 0..2");
        ngreen += xtrans[i] == 1;
    }
    if (ngreen != 20) return fail(ctx, ARTGPU_EUNSUPPORTED, "demosaic_xtrans: not an X-Trans colour map (%d green of 36)", ngreen);
    // the reference keeps the hexagon offsets in `short` (xtrans_demosaic.cc:233): same range limit here
    if (2 * (long long)raw_stride + 2 > 32767) return fail(ctx, ARTGPU_EUNSUPPORTED, "demosaic_xtrans: row stride %zu exceeds the reference's short offsets", raw_stride);
    return ARTGPU_OK;
}

// RawImageSource::xtrans_interpolate on a bound image, after demosaic_xtrans_check
int demosaic_xtrans_dev(artgpu_ctx *ctx, const DevImage &d, int W, int H, int passes, int use_cielab, const int32_t xtrans[36], const float rgb_cam[12])
{
    int rc;
    XtransArgs a = {};
    a.raw = d.raw; a.raw_stride = d.raw_stride;
    a.red = d.r; a.green = d.g; a.blue = d.b; a.out_stride = d.out_stride;
    a.W = W; a.H = H; a.passes = passes; a.ndir = 4 << (passes > 1); a.use_cielab = use_cielab ? 1 : 0;
    for (int i = 0; i < 36; ++i) a.xtrans[i] = xtrans[i];
    auto isgreen = [&](int row, int col) { return a.xtrans[(row % 3) * 6 + col % 3] & 1; };
    {   // xyz_cam (L219-230)
        static const float xyz_rgb[3][3] = {{0.412453, 0.357580, 0.180423}, {0.212671, 0.715160, 0.072169}, {0.019334, 0.119193, 0.950227}};
        static const float d65_white[3] = {0.950456, 1, 1.088754};
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                float acc = 0;
                for (int k = 0; k < 3; k++) acc += xyz_rgb[i][k] * rgb_cam[k * 4 + j] / d65_white[i];
                a.xyz_cam[i * 3 + j] = acc;
            }
    }
    {   // green hexagons around each site class and the solitary-green phase (L232-267)
        static const int orth[12] = {1, 0, 0, 1, -1, 0, 0, -1, 1, 0, 0, 1};
        static const int patt[2][16] = {{0, 1, 0, -1, 2, 0, -1, 0, 1, 1, 1, -1, 0, 0, 0, 0}, {0, 1, 0, -2, 1, 0, -2, 0, 1, 1, -2, -2, 1, -1, -1, 1}};
        for (int row = 0; row < 3; row++)
            for (int col = 0; col < 3; col++) {
                const int gint = isgreen(row, col);
                for (int ng = 0, dd = 0; dd < 10; dd += 2) {
                    if (isgreen(row + orth[dd] + 6, col + orth[dd + 2] + 6)) ng = 0; else ng++;
                    if (ng == 4) { a.sgrow = row; a.sgcol = col; }
                    if (ng == gint + 1)
                        for (int c = 0; c < 8; c++) {
                            const int v = orth[dd] * patt[gint][c * 2] + orth[dd + 1] * patt[gint][c * 2 + 1];
                            const int h = orth[dd + 2] * patt[gint][c * 2] + orth[dd + 3] * patt[gint][c * 2 + 1];
                            a.allhex0[row][col][c ^ (gint * 2 & dd)] = h + v * (int)d.raw_stride;
                            a.allhex1[row][col][c ^ (gint * 2 & dd)] = h + v * XTRANS_TS;
                        }
                }
            }
        for (int row = 0; row < 3; row++) {
            int greencount = 0;
            for (int col = 0; col < 3; col++) greencount += isgreen(row, col);
            a.right_shift[row] = greencount == 2;
        }
    }
    float *lut;
    const bool fresh = ctx->pool[P_XCBRT] == nullptr;
    if ((rc = pool_get(ctx, P_XCBRT, 0x14000 * 4, &lut))) return rc;
    if (fresh) {   // cielab's LUT (L43-57), built on the host like the reference's
        std::vector<float> host(0x14000);
        const double eps = 216.0 / 24389.0, kappa = 24389.0 / 27.0;
        for (int i = 0; i < 0x14000; i++) {
            const double r = i / 65535.0;
            host[i] = (float)(r > eps ? std::cbrt(r) : (kappa * r + 16.0) / 116.0);
        }
        HIPCHK(ctx, hipMemcpyAsync(lut, host.data(), host.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    a.cbrt_lut = lut;
    a.ntx = (W - 22 + (XTRANS_TS - 16) - 1) / (XTRANS_TS - 16);
    const int nty = (H - 22 + (XTRANS_TS - 16) - 1) / (XTRANS_TS - 16);
    a.ntiles = a.ntx * nty;
    // one 1024-thread workgroup is resident per CU: one persistent workgroup per CU, tiles from a shared counter (the arena is 0.45 GB)
    if (ctx->num_cus <= 0) {
        hipDeviceProp_t prop;
        HIPCHK(ctx, hipGetDeviceProperties(&prop, ctx->device));
        ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    const int grid = a.ntiles < ctx->num_cus ? a.ntiles : ctx->num_cus;
    if (!ctx->rcd_counter) HIPCHK(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->rcd_counter), 64));
    a.counter = ctx->rcd_counter + 4;           // (the RCD kernel's counter is word 0 of the same 64 bytes)
    HIPCHK(ctx, hipMemsetAsync(a.counter, 0, sizeof(int), ctx->stream));
    a.arena_floats = (size_t)XTRANS_TS * XTRANS_TS * (a.ndir * 4 + 3) + 128;
    rc = ensure(ctx, &ctx->arena, &ctx->arena_bytes, (size_t)grid * a.arena_floats * sizeof(float));
    if (rc) return rc;
    a.arena = ctx->arena;
    if (ctx->timing) HIPCHK(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    HIPCHK(ctx, launch_xtrans(a, grid, ctx->stream));
    if (ctx->timing) { HIPCHK(ctx, hipEventRecord(ctx->ev[1], ctx->stream)); HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream)); }
    return ctx->timing ? demosaic_read_timings(ctx, false) : ARTGPU_OK;
}

} } // namespace artgpu::api
