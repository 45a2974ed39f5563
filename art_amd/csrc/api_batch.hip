// art_amd/csrc/api_batch.hip -- batches: the lanes, artgpu_batch_run, the I/O lanes (io_frame, artgpu_batch_run_io), artgpu_batch_complete
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

extern "C" {

int artgpu_set_batch_lanes(artgpu_ctx *ctx, int lanes)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (lanes < 1 || lanes > 8) return fail(ctx, ARTGPU_EINVAL, "set_batch_lanes: 1..8");
    ctx->batch_lanes = lanes;
    return ARTGPU_OK;
}

} // extern "C"

namespace {

// The scratch of a context only grows (about 5 GB for a 45 MP frame through the whole tool).  A batch that goes on with much smaller frames
// would keep the large frame's pools for nothing: when this frame AND the lane's next one have less than half the pixels the pools were
// grown for, the lane gives them back first (artgpu_trim_scratch: a stream drain and a few hipFree, paid once per such transition; a
// batch that alternates sizes keeps its pools).  Round-5 review, weak point 10.  `nxt` < 0: the lane's last frame has no successor to go
// by -- it keeps the pools, a caller that is done calls artgpu_trim_scratch.
int batch_settle_scratch(artgpu_ctx *c, long long px, long long nxt)
{
    if (nxt < 0) nxt = c->batch_px;
    if (c->batch_px && 2 * px < c->batch_px && 2 * nxt < c->batch_px) {
        std::vector<artgpu_ctx *> keep;
        keep.swap(c->lanes);                       // (only this context's own pools: its lanes decide for themselves)
        const int rc = artgpu_trim_scratch(c);
        keep.swap(c->lanes);
        if (rc) return rc;
        c->batch_px = 0;
    }
    if (px > c->batch_px) c->batch_px = px;
    return ARTGPU_OK;
}

// Frames are independent: lane k (its own context, stream and host thread) takes frames k, k+L, ...  The kernels of one frame
// are a mix of latency-bound (AMaZE) and bandwidth-bound (wavelet passes) work, so frames in flight on different streams fill
// each other's gaps (+11 % throughput with three lanes at 45 MP, scripts/overlap_time.py).
int batch_prepare_lanes(artgpu_ctx *ctx, int L)
{
    HIPCHK(ctx, hipSetDevice(ctx->device));
    while ((int)ctx->lanes.size() < L - 1) {
        artgpu_ctx *peer = nullptr;
        int rc = artgpu_create(ctx->device, &peer);
        if (rc) return fail(ctx, rc, "batch_run: cannot create lane %d", (int)ctx->lanes.size() + 1);
        if (hipStreamCreateWithFlags(&peer->stream, hipStreamNonBlocking) != hipSuccess) { (void)artgpu_destroy(peer); return fail(ctx, ARTGPU_EHIP, "batch_run: stream"); }
        peer->owns_stream = true;
        ctx->lanes.push_back(peer);
    }
    // the lanes are this context as far as the caller can tell: its options, curve tail and progress listener apply to every frame,
    // whichever lane runs it (copied on every call -- they may change between calls)
    for (artgpu_ctx *peer : ctx->lanes) {
        peer->shared = ctx->shared;
        peer->frames_in_flight = L;
    }
    ctx->frames_in_flight = L;
    return ARTGPU_OK;
}
struct InFlightReset { artgpu_ctx *c; ~InFlightReset() { c->frames_in_flight = 1; for (artgpu_ctx *p : c->lanes) p->frames_in_flight = 1; } };

// run `work(lane context, lane index)` on L lanes (lane 0 on the calling thread) and gather the status codes
template <typename F>
int batch_on_lanes(artgpu_ctx *ctx, int L, F work)
{
    std::vector<int> rcs(L, ARTGPU_OK);
    // (the lanes' contexts are looked up HERE: lane 0 may take ctx->lanes aside for a moment while it trims its own pools -- batch_settle_scratch --,
    // and a thread that starts late must not index the vector then)
    std::vector<artgpu_ctx *> cs(L, ctx);
    for (int k = 1; k < L; ++k) cs[k] = ctx->lanes[k - 1];
    std::vector<std::thread> threads;
    for (int k = 1; k < L; ++k) threads.emplace_back([&rcs, &work, &cs, k]() { rcs[k] = work(cs[k], k); });
    rcs[0] = work(ctx, 0);
    for (std::thread &t : threads) t.join();
    for (int k = 0; k < L; ++k)
        if (rcs[k]) return fail(ctx, rcs[k], "batch_run: lane %d: %s", k, k == 0 ? ctx->err.c_str() : cs[k]->err.c_str());
    return ARTGPU_OK;
}

} // namespace

extern "C" {

int artgpu_batch_run(artgpu_ctx *ctx, int nframes, const artgpu_plane *raws, const artgpu_pipeline_params *params, artgpu_rgb *outs)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (nframes < 0 || (nframes && (!raws || !params || !outs))) return fail(ctx, ARTGPU_EINVAL, "batch_run: null argument");
    const int L = std::min(ctx->batch_lanes, nframes);
    auto px_of = [&](int f) { return (long long)raws[f].w * raws[f].h; };
    if (L <= 1) {
        for (int f = 0; f < nframes; ++f) {
            int rc = batch_settle_scratch(ctx, px_of(f), f + 1 < nframes ? px_of(f + 1) : -1);
            if (!rc) rc = pipeline_run_impl(ctx, &raws[f], params, &outs[f], true);
            if (rc) return rc;
        }
        return ARTGPU_OK;
    }
    int rc = batch_prepare_lanes(ctx, L);
    if (rc) return rc;
    InFlightReset in_flight_reset{ctx};
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      // inputs the caller produced on this context's stream
    return batch_on_lanes(ctx, L, [&](artgpu_ctx *c, int k) -> int {
        for (int f = k; f < nframes; f += L) {
            int rc2 = batch_settle_scratch(c, px_of(f), f + L < nframes ? px_of(f + L) : -1);
            if (!rc2) rc2 = pipeline_run_impl(c, &raws[f], params, &outs[f], true);
            if (rc2) return rc2;
        }
        if (k > 0 && hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, ARTGPU_EHIP, "batch_run: lane %d: stream", k);
        return ARTGPU_OK;
    });
}

} // extern "C"

// ---------------------------------------------------------------------------------------------
// the batch between the decoder's and the writers' formats, copies beside the kernels
// ---------------------------------------------------------------------------------------------

namespace {

int io_setup(artgpu_ctx *c, int nfr)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->io_up) HIPCHK(c, hipStreamCreateWithFlags(&c->io_up, hipStreamNonBlocking));
    if (!c->io_down) HIPCHK(c, hipStreamCreateWithFlags(&c->io_down, hipStreamNonBlocking));
    for (int k = 0; k < 8; ++k)
        if (!c->io_ev[k]) HIPCHK(c, hipEventCreateWithFlags(&c->io_ev[k], hipEventDisableTiming));
    if (c->io_host_cap < nfr) {
        if (c->io_host) { HIPCHK(c, hipHostFree(c->io_host)); c->io_host = nullptr; c->io_host_cap = 0; }
        const int cap = nfr < 16 ? 16 : nfr;
        if (hipHostMalloc(reinterpret_cast<void **>(&c->io_host), (size_t)cap * 8 * sizeof(int), hipHostMallocDefault) != hipSuccess) {
            c->io_host = nullptr;
            return fail(c, ARTGPU_ENOMEM, "batch_run_io: pinned flag words for %d frames", cap);
        }
        c->io_host_cap = cap;
    }
    std::memset(c->io_host, 0, (size_t)c->io_host_cap * 8 * sizeof(int));
    return ARTGPU_OK;
}

// pinned (hipHostMalloc / hipHostRegister) host memory?  Its device address if so.  Pageable memory is "invalid value" to the query: not an error here.
void *pinned_device_address(const void *p)
{
    hipPointerAttribute_t at = {};
    if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer) return at.devicePointer;
    (void)hipGetLastError();
    return nullptr;
}

// frame `i` of this lane: everything is queued, nothing is waited for (the staging slots of turn i - 2 are released through events)
int io_frame(artgpu_ctx *c, int i, const artgpu_sensor_frame *in, const artgpu_pipeline_params *p, artgpu_scanline_frame *out)
{
    const int s = i & 1, W = in->w, H = in->h, b = p->border;
    const int esz = in->is_u16 ? 2 : 4;
    if (!in->data || W <= 0 || H <= 0 || in->row_stride_bytes < (int64_t)W * esz || in->row_stride_bytes % esz)
        return fail(c, ARTGPU_EINVAL, "batch_run_io: sensor frame: bad pointer/size/stride");
    if (b < 0 || W - 2 * b < 8 || H - 2 * b < 8) return fail(c, ARTGPU_EINVAL, "batch_run_io: border %d leaves no image", b);
    // the size the frame leaves at: the image behind the border, or what the Resize tool makes of it (artgpu_set_pipeline_resize)
    int iw, ih;
    float rs_scale;
    (void)pipeline_resize(c, W - 2 * b, H - 2 * b, &iw, &ih, &rs_scale);
    if (iw < 1 || ih < 1) return fail(c, ARTGPU_EINVAL, "batch_run_io: the Resize tool leaves no image (%dx%d)", iw, ih);
    const bool okfmt = out->is_float ? (out->bps == 16 || out->bps == 32) : (out->bps == 8 || out->bps == 16);
    if (!okfmt) return fail(c, ARTGPU_EINVAL, "batch_run_io: bps %d / is_float %d", out->bps, out->is_float);
    const size_t rowb = (size_t)iw * 3 * (out->bps / 8);
    if (!out->scanlines || out->row_stride_bytes < (int64_t)rowb) return fail(c, ARTGPU_EINVAL, "batch_run_io: scanlines: bad pointer / row stride < %zu", rowb);
    if (out->rgb2out_enabled) {
        if (!out->trc_linear && (!out->trc_lut || out->trc_lutsz < 2)) return fail(c, ARTGPU_EINVAL, "batch_run_io: a non-linear TRC needs its LUT");
        if (out->trc_lut && (out->trc_lutsz < 2 || out->trc_lutsz > 65536)) return fail(c, ARTGPU_EINVAL, "batch_run_io: trc_lutsz %d", out->trc_lutsz);
    }
    int rc;
    float *cfa, *img[3], *flags_f;
    if ((rc = pool_get(c, P_IO_CFA, (size_t)W * H * 4, &cfa)) || (rc = pool_get(c, P_IO_FLAGS, 2 * 8 * sizeof(int), &flags_f))) return rc;
    for (int k = 0; k < 3; ++k)
        if ((rc = pool_get(c, P_IO_IMG0 + 3 * s + k, (size_t)iw * ih * 4, &img[k]))) return rc;      // (two sets: the download of turn i reads its set while turn i + 1 is computed)
    int *flags = reinterpret_cast<int *>(flags_f) + 8 * s;
    // Where do the scanlines go?  Pinned host memory is mapped into the device's address space: a few workgroups on the download stream write
    // them there directly.  Anything else (pageable memory, rows that are not 16-byte aligned, option io_direct = 0) is staged and copied.
    // Scanlines for PINNED memory can be written there by a kernel of the download stream (option io_direct = n workgroups) instead of being staged and
    // copied.  Measured on 8192 x 5464 frames, 16-bit scanlines (scripts/pcie_batch.py, batches of 24 - 36 frames, seven runs): the runtime's copy -- itself a
    // kernel, 268 MB in 4.9 ms -- 11.0 ms per frame with one lane, 10.6 - 13.8 with two (two modes: the lanes lock into step with the copy kernel in
    // about half the runs), 10.7 - 11.3 with three; eight workgroups writing directly 11.7 - 12.6 / 11.2 - 11.8 / 11.7 - 12.9 (they hold eight CUs for
    // 5 ms, and the one-workgroup-per-CU kernels of the next frame wait for a CU or run on fewer: cu_reserve).  So: the copy, except with two lanes.
    const int direct_wgs = c->shared.opt_io_direct >= 0 ? c->shared.opt_io_direct : (c->frames_in_flight == 2 ? 8 : 0);
    // A copy from / to PAGEABLE memory blocks the calling thread until it is done (the runtime stages it in pieces): nothing is gained by giving it a
    // stream of its own, so it stays on the context's stream like the copies of the four separate entry points; lanes still overlap each other.
    unsigned char *const out_pinned = out->on_device ? nullptr : static_cast<unsigned char *>(pinned_device_address(out->scanlines));
    const hipStream_t s_up = (in->on_device || pinned_device_address(in->data)) ? c->io_up : c->stream;
    const hipStream_t s_down = out_pinned ? c->io_down : c->stream;
    unsigned char *host_dev = nullptr;
    if (out_pinned && direct_wgs > 0 && (reinterpret_cast<uintptr_t>(out->scanlines) & 15) == 0 && (out->row_stride_bytes & 15) == 0) host_dev = out_pinned;
    // (this lane's download and a neighbour's; reset when the lane is done.  The caller's own "cu_reserve" is another field: cu_reserve_of())
    c->io_cu_reserve = host_dev ? direct_wgs * (c->frames_in_flight > 1 ? 2 : 1) : 0;
    // The working image of this slot is free again once the download of turn i - 2 has read it -- WHATEVER this frame's own output is: a direct
    // download (launch_scanlines_host on io_down) reads the working image itself, and a frame with its scanlines on the device two turns later
    // writes that image as any other does.  (The wait used to be left out for device outputs: DESIGN.md section 17.)  The event
    // of a turn that had nothing to download holds an older record, long completed: no wait at all.
    if (i >= 2) HIPCHK(c, hipStreamWaitEvent(c->stream, c->io_ev[6 + s], 0));

    // ---- upload (io_up) -> copyOriginalPixels + scaleColors (stream)
    ScaleArgs a = {};
    if (in->on_device) { a.src = in->data; a.src_stride = (size_t)(in->row_stride_bytes / esz); }
    else {
        float *st;
        if ((rc = pool_get(c, P_IO_IN0 + s, (size_t)W * H * esz, &st))) return rc;
        if (i >= 2) HIPCHK(c, hipStreamWaitEvent(s_up, c->io_ev[2 + s], 0));       // the kernel that read this slot two turns ago
        // (always the pitched form: a LINEAR copy from or to pageable memory makes the runtime pin the caller's pages for the occasion, 25 ms for a frame's scanlines)
        HIPCHK(c, hipMemcpy2DAsync(st, (size_t)W * esz, in->data, (size_t)in->row_stride_bytes, (size_t)W * esz, H, hipMemcpyHostToDevice, s_up));
        HIPCHK(c, hipEventRecord(c->io_ev[s], s_up));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->io_ev[s], 0));
        a.src = st; a.src_stride = W;
    }
    a.dst = cfa; a.dst_stride = W;
    if ((rc = scale_args_fill(c, W, H, in->is_u16, p->filters, p->sensor != 0 ? p->xtrans : nullptr, in->cblacksom, in->scale_mul, "batch_run_io", &a))) return rc;
    a.chmax_bits = flags;
    HIPCHK(c, hipMemsetAsync(flags, 0, 8 * sizeof(int), c->stream));
    HIPCHK(c, launch_scale_colors(a, c->stream));
    if (!in->on_device) HIPCHK(c, hipEventRecord(c->io_ev[2 + s], c->stream));

    // ---- the path
    artgpu_plane raw = {cfa, W, H, (int64_t)W * 4, 1};
    // CA_correct_RT on the staged CFA plane itself, after scaleColors and before the demosaic (rawimagesource.cc:1666,1827)
    if (pipeline_ca(p) && (rc = pipeline_ca_dev(c, cfa, W, W, H, p))) return rc;
    artgpu_rgb image = mk_dev_rgb(img, iw, ih, iw);
    // (the frame's plan -- pipeline_plan -- runs in here, behind the upload and scaleColors: a refused frame has done that work already.  Planning
    // ahead of the upload would change what a refused frame leaves behind, so it stays)
    if ((rc = pipeline_run_impl(c, &raw, p, &image, false))) return rc;

    // ---- rgb2out (matrix + TRC, in place) and the writers' scanlines
    OutArgs o = {};
    for (int k = 0; k < 3; ++k) { o.src[k] = img[k]; o.dst[k] = img[k]; }
    o.src_stride = iw; o.dst_stride = iw; o.w = iw; o.h = ih;
    if (out->rgb2out_enabled) {
        for (int k = 0; k < 9; ++k) o.m[k] = out->out_matrix[k];
        o.linear = out->trc_linear ? 1 : 0;
        o.unsupported = flags + 4;
        if (out->trc_lut) {
            float *tab;
            if ((rc = pool_get(c, P_PIPE_R, (size_t)65536 * 4, &tab)) || (rc = h2d_table(c, tab, out->trc_lut, (size_t)out->trc_lutsz * 4))) return rc;   // (the demosaiced plane in this slot is done with)
            o.lut = tab; o.lutsz = out->trc_lutsz;
        }
        HIPCHK(c, launch_rgb2out_matrix(o, c->stream));
    }
    o.bps = out->bps; o.is_float = out->is_float ? 1 : 0;
    if (host_dev) {
        // flags, then the scanlines on the download stream, straight into the caller's buffer
        HIPCHK(c, hipMemcpyAsync(c->io_host + 8 * i, flags, 8 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipEventRecord(c->io_ev[4 + s], c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->io_down, c->io_ev[4 + s], 0));
        o.out = host_dev; o.out_stride_bytes = (size_t)out->row_stride_bytes;
        HIPCHK(c, launch_scanlines_host(o, direct_wgs, c->io_down));
        HIPCHK(c, hipEventRecord(c->io_ev[6 + s], c->io_down));
        return ARTGPU_OK;
    }
    if (out->on_device) { o.out = static_cast<unsigned char *>(out->scanlines); o.out_stride_bytes = (size_t)out->row_stride_bytes; }
    else {
        float *st;
        if ((rc = pool_get(c, P_IO_OUT0 + s, rowb * ih + 16, &st))) return rc;
        o.out = reinterpret_cast<unsigned char *>(st); o.out_stride_bytes = rowb;         // (free again: the wait for turn i - 2's download above)
    }
    HIPCHK(c, launch_scanlines(o, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->io_host + 8 * i, flags, 8 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (!out->on_device) {
        HIPCHK(c, hipEventRecord(c->io_ev[4 + s], c->stream));
        HIPCHK(c, hipStreamWaitEvent(s_down, c->io_ev[4 + s], 0));
        HIPCHK(c, hipMemcpy2DAsync(out->scanlines, (size_t)out->row_stride_bytes, o.out, rowb, rowb, ih, hipMemcpyDeviceToHost, s_down));
        HIPCHK(c, hipEventRecord(c->io_ev[6 + s], s_down));
    }
    return ARTGPU_OK;
}

} // namespace

extern "C" {

int artgpu_batch_run_io(artgpu_ctx *ctx, int nframes, const artgpu_sensor_frame *in, const artgpu_pipeline_params *params, artgpu_scanline_frame *out)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (nframes < 0 || (nframes && (!in || !params || !out))) return fail(ctx, ARTGPU_EINVAL, "batch_run_io: null argument");
    if (nframes == 0) return ARTGPU_OK;
    const int L = std::min(ctx->batch_lanes, nframes);
    // (a frame's `status` is ARTGPU_OK only where a lane vouches for it below: a call that ends before the lanes start says so on every frame)
    auto all_frames = [&](int code) {
        for (int f = 0; f < nframes; ++f) { out[f].status = code; out[f].chmax[0] = out[f].chmax[1] = out[f].chmax[2] = out[f].chmax[3] = 0.f; }
        return code;
    };
    int rc = batch_prepare_lanes(ctx, L);          // (L == 1: no lanes, frames_in_flight = 1)
    if (rc) return all_frames(rc);
    InFlightReset in_flight_reset{ctx};
    if (hipStreamSynchronize(ctx->stream) != hipSuccess)      // inputs the caller produced on this context's stream
        return all_frames(fail(ctx, ARTGPU_EHIP, "batch_run_io: the context's stream"));
    auto px_of = [&](int f) { return (long long)in[f].w * in[f].h; };
    all_frames(ARTGPU_OK);
    rc = batch_on_lanes(ctx, L, [&](artgpu_ctx *c, int k) -> int {
        const int mine = (nframes - k + L - 1) / L;
        int rc2 = io_setup(c, mine);
        int queued = 0;        // turns of this lane that were queued to their end: the first one that was not is where the lane stopped
        for (int f = k, i = 0; !rc2 && f < nframes; f += L, ++i) {
            rc2 = batch_settle_scratch(c, px_of(f), f + L < nframes ? px_of(f + L) : -1);
            if (!rc2) rc2 = io_frame(c, i, &in[f], params, &out[f]);
            if (!rc2) queued = i + 1;
        }
        // the lane's copies and kernels, then what the frames left in the pinned words
        c->io_cu_reserve = 0;
        hipError_t e = hipStreamSynchronize(c->stream);
        if (c->io_down) { const hipError_t e2 = hipStreamSynchronize(c->io_down); if (e == hipSuccess) e = e2; }
        if (c->io_up) { const hipError_t e2 = hipStreamSynchronize(c->io_up); if (e == hipSuccess) e = e2; }
        // A stream that failed or a kernel that gave up a bounded wait: the lane cannot vouch for any of its frames, the turns before a refused
        // one included.  Otherwise those turns have run to their end, and their pinned words are what they are for any other frame.
        if (e != hipSuccess) { rc2 = fail(c, ARTGPU_EHIP, "batch_run_io: lane %d: %s", k, hipGetErrorString(e)); queued = 0; }
        else if (const int rf = check_async_faults(c)) { rc2 = rf; queued = 0; }
        int unsupported = ARTGPU_OK;
        for (int f = k, i = 0; f < nframes; f += L, ++i) {
            if (i >= queued) { out[f].status = rc2; continue; }      // the turn the lane stopped at and every later one: not run, chmax stays 0
            const int *w = c->io_host + 8 * i;
            for (int ch = 0; ch < 3; ++ch) std::memcpy(&out[f].chmax[ch], &w[ch], sizeof(float));
            out[f].chmax[3] = out[f].chmax[1];
            if (out[f].rgb2out_enabled && w[4]) {
                out[f].status = ARTGPU_EUNSUPPORTED;
                // (the lane's own error, if it has one, keeps artgpu_last_error)
                if (!rc2 && !unsupported) unsupported = fail(c, ARTGPU_EUNSUPPORTED, "batch_run_io: frame %d: %d channel values above 1 need ARTOutputProfile::eval (lcms2/libm) on the host", f, w[4]);
            }
        }
        return rc2 ? rc2 : unsupported;
    });
    return rc;
}

// The one collective of a multi-GPU batch: an all-gather of the ranks' completion records over the caller's RCCL communicator.
// RCCL is bound at run time (dlopen), so the library has no link-time dependency on it and single-GPU users never load it.
int artgpu_batch_complete(artgpu_ctx *ctx, void *rccl_comm, int nranks, const int64_t record[ARTGPU_BATCH_RECORD_WORDS], int64_t *all_records)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!record || !all_records || nranks < 1) return fail(ctx, ARTGPU_EINVAL, "batch_complete: bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      // the record describes work that has finished
    if (!rccl_comm) {
        if (nranks != 1) return fail(ctx, ARTGPU_EINVAL, "batch_complete: %d ranks need a communicator", nranks);
        std::memcpy(all_records, record, sizeof(int64_t) * ARTGPU_BATCH_RECORD_WORDS);
        return ARTGPU_OK;
    }
    // ncclResult_t ncclAllGather(const void *sendbuff, void *recvbuff, size_t sendcount, ncclDataType_t, ncclComm_t, hipStream_t)
    typedef int (*allgather_fn)(const void *, void *, size_t, int, void *, hipStream_t);
    typedef const char *(*errstr_fn)(int);
    static allgather_fn allgather = nullptr;
    static errstr_fn errstr = nullptr;
    if (!allgather) {
        void *h = nullptr;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
            if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
        if (!h) return fail(ctx, ARTGPU_EUNSUPPORTED, "batch_complete: cannot load librccl (%s)", dlerror());
        allgather = reinterpret_cast<allgather_fn>(dlsym(h, "ncclAllGather"));
        errstr = reinterpret_cast<errstr_fn>(dlsym(h, "ncclGetErrorString"));
        if (!allgather) return fail(ctx, ARTGPU_EUNSUPPORTED, "batch_complete: librccl has no ncclAllGather");
    }
    constexpr int NCCL_INT64 = 4;       // ncclDataType_t (nccl.h): ncclInt8 0, ncclUint8 1, ncclInt32 2, ncclUint32 3, ncclInt64 4
    const size_t words = ARTGPU_BATCH_RECORD_WORDS;
    float *buf;
    int rc = pool_get(ctx, P_BATCH, (size_t)(nranks + 1) * words * sizeof(int64_t), &buf);
    if (rc) return rc;
    int64_t *d_send = reinterpret_cast<int64_t *>(buf), *d_recv = d_send + words;
    HIPCHK(ctx, hipMemcpyAsync(d_send, record, words * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    const int nrc = allgather(d_send, d_recv, words, NCCL_INT64, rccl_comm, ctx->stream);
    if (nrc != 0) return fail(ctx, ARTGPU_EHIP, "batch_complete: ncclAllGather failed: %s", errstr ? errstr(nrc) : "?");
    HIPCHK(ctx, hipMemcpyAsync(all_records, d_recv, (size_t)nranks * words * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ARTGPU_OK;
}

} // extern "C"
