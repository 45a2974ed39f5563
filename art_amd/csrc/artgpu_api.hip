// art_amd/csrc/artgpu_api.hip -- the C ABI of libartgpu.so (include/artgpu.h) but for the frame driver, the batch lanes, the demosaicers,
// the shared filters and colour correction: context, device buffers, staging for host-pointer calls, kernel launches, error reporting.
// There is no CPU fallback here: every entry point either runs the HIP kernels or fails.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace {

// A table of constants in a pool slot of its own, built on the host by `fill` (which gets `nfloats` zeroed floats) and uploaded once per
// context.  The slot doubles as the "uploaded" flag.  The host waits for the copy because the host vector dies with this call -- a bubble in
// the stream, which is why these tables have slots that nothing else grows -- and on a failed upload the slot is given back, or the next call
// would skip the upload and read an empty table.
int const_table_dev(artgpu_ctx *ctx, int slot, size_t nfloats, void (*fill)(float *), const char *what, float **out)
{
    const bool fresh = ctx->pool[slot] == nullptr;
    const int rc = pool_get(ctx, slot, nfloats * 4, out);
    if (rc || !fresh) return rc;
    std::vector<float> host(nfloats);
    fill(host.data());
    hipError_t e = hipMemcpyAsync(*out, host.data(), nfloats * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(ctx->pool[slot]); ctx->pool[slot] = nullptr; ctx->pool_bytes[slot] = 0;
        *out = nullptr;
        return fail(ctx, ARTGPU_EHIP, "upload of the %s failed: %s", what, hipGetErrorString(e));
    }
    return ARTGPU_OK;
}

// Color::cachef / cachefy / denoiseGammaTab / denoiseIGammaTab, built on the host like the reference's (color.cc:202-292)
void build_lab_tabs(float *host)
{
    build_cachef(host); build_cachefy(host + 65536);
    build_denoise_gamma_tabs(host + 2 * 65536, host + 3 * 65536);
}

} // namespace

namespace artgpu { namespace api {

int fail(artgpu_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) {
        ctx->err = buf;
        // a fault raised by the fused shrink pass's bounded wait (shrinkblur.hip) is attributed: the kernel left these words in pinned host
        // memory when it gave up (check_async_faults finds them at the next synchronisation point)
        if (code == ARTGPU_EHIP && ctx->fs_diag && (unsigned)ctx->fs_diag[0] == 0xF5D1A600u) {
            char more[192];
            snprintf(more, sizeof more, " [shrink_blur_kernel: band %d strip %d gave up waiting for the strip above to hand down block %d (its counter: %d)]",
                     ctx->fs_diag[1], ctx->fs_diag[2], ctx->fs_diag[3], ctx->fs_diag[4]);
            ctx->err += more;
            ctx->fs_diag[0] = 0;      // reported once: a later, unrelated failure is not attributed to it
        }
    }
    return code;
}

int ensure(artgpu_ctx *ctx, float **buf, size_t *cur, size_t need)
{
    if (*cur >= need) return ARTGPU_OK;
    if (*buf) { HIPCHK(ctx, hipFree(*buf)); *buf = nullptr; *cur = 0; }
    hipError_t e = hipMalloc(reinterpret_cast<void **>(buf), need);
    if (e != hipSuccess) {
        *buf = nullptr;
        return fail(ctx, ARTGPU_ENOMEM, "hipMalloc(%zu bytes) failed: %s", need, hipGetErrorString(e));
    }
    *cur = need;
    return ARTGPU_OK;
}

// A caller's look-up table -> device memory, one lifetime rule for all of them (artgpu.h "Host look-up tables"): the array is free when
// the entry point returns, whatever kind of memory it is (pageable, pinned, registered, managed).  The table is copied into a pinned ring the
// context owns and travels from there on the context's stream, so the call neither depends on how HIP treats the caller's memory type nor
// drains the stream; the host only waits (for the ring's last copy) when the ring wraps, every dozen calls.
int h2d_table(artgpu_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (need > ctx->tab_ring_bytes) {
        if (ctx->tab_ring) {
            if (ctx->tab_ring_busy) HIPCHK(ctx, hipEventSynchronize(ctx->tab_ev));
            HIPCHK(ctx, hipHostFree(ctx->tab_ring));
            ctx->tab_ring = nullptr; ctx->tab_ring_bytes = 0; ctx->tab_ring_busy = false;
        }
        const size_t cap = need * 2 > ((size_t)8 << 20) ? need * 2 : ((size_t)8 << 20);
        if (hipHostMalloc(reinterpret_cast<void **>(&ctx->tab_ring), cap, hipHostMallocDefault) != hipSuccess) {
            ctx->tab_ring = nullptr;
            return fail(ctx, ARTGPU_ENOMEM, "pinned staging ring for look-up tables (%zu bytes)", cap);
        }
        ctx->tab_ring_bytes = cap; ctx->tab_ring_off = 0;
        if (!ctx->tab_ev) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->tab_ev, hipEventDisableTiming));
    }
    if (ctx->tab_ring_off + need > ctx->tab_ring_bytes) {        // wrap: what was staged before has to have left the ring
        if (ctx->tab_ring_busy) HIPCHK(ctx, hipEventSynchronize(ctx->tab_ev));
        ctx->tab_ring_busy = false;
        ctx->tab_ring_off = 0;
    }
    char *slot = ctx->tab_ring + ctx->tab_ring_off;
    std::memcpy(slot, src, bytes);
    HIPCHK(ctx, hipMemcpyAsync(dst, slot, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->tab_ev, ctx->stream));
    ctx->tab_ring_busy = true;
    ctx->tab_ring_off += need;
    return ARTGPU_OK;
}

bool plane_ok(const artgpu_plane *p)
{
    return p && p->p && p->w > 0 && p->h > 0 && p->row_stride_bytes >= (int64_t)p->w * 4 && (p->row_stride_bytes % 4) == 0;
}

// Resolve device pointers for (raw, out); host planes are staged through ctx buffers.
int bind_images(artgpu_ctx *ctx, const artgpu_plane *raw, artgpu_rgb *out, DevImage *d)
{
    const int W = raw->w, H = raw->h;
    const artgpu_plane *op[3] = {&out->r, &out->g, &out->b};
    for (int k = 0; k < 3; ++k) {
        if (!plane_ok(op[k]) || op[k]->w != W || op[k]->h != H) return fail(ctx, ARTGPU_EINVAL, "output plane %d: bad pointer/size/stride", k);
        if ((op[k]->on_device != 0) != (out->r.on_device != 0) || op[k]->row_stride_bytes != out->r.row_stride_bytes)
            return fail(ctx, ARTGPU_EINVAL, "output planes must share residency and row stride");
    }
    d->staged = false;
    if (raw->on_device) {
        d->raw = raw->p;
        d->raw_stride = (size_t)(raw->row_stride_bytes / 4);
    } else {
        int rc = ensure(ctx, &ctx->stage[0], &ctx->stage_bytes[0], (size_t)W * H * 4);
        if (rc) return rc;
        HIPCHK(ctx, hipMemcpy2DAsync(ctx->stage[0], (size_t)W * 4, raw->p, (size_t)raw->row_stride_bytes, (size_t)W * 4, H, hipMemcpyHostToDevice, ctx->stream));
        d->raw = ctx->stage[0];
        d->raw_stride = W;
    }
    if (out->r.on_device) {
        d->r = out->r.p; d->g = out->g.p; d->b = out->b.p;
        d->out_stride = (size_t)(out->r.row_stride_bytes / 4);
    } else {
        for (int k = 0; k < 3; ++k) {
            int rc = ensure(ctx, &ctx->stage[1 + k], &ctx->stage_bytes[1 + k], (size_t)W * H * 4);
            if (rc) return rc;
        }
        d->r = ctx->stage[1]; d->g = ctx->stage[2]; d->b = ctx->stage[3];
        d->out_stride = W;
        d->staged = true;
    }
    return ARTGPU_OK;
}

int unbind_images(artgpu_ctx *ctx, artgpu_rgb *out, const DevImage *d)
{
    if (!d->staged) return ARTGPU_OK;
    const int W = out->r.w, H = out->r.h;
    artgpu_plane *op[3] = {&out->r, &out->g, &out->b};
    const float *src[3] = {d->r, d->g, d->b};
    for (int k = 0; k < 3; ++k)
        HIPCHK(ctx, hipMemcpy2DAsync(op[k]->p, (size_t)op[k]->row_stride_bytes, src[k], (size_t)W * 4, (size_t)W * 4, H, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ARTGPU_OK;
}

// descriptors of device memory: one dense w x h plane; three planes with rows of `stride` floats
artgpu_plane mk_dev_plane(float *p, int w, int h) { return artgpu_plane{p, w, h, (int64_t)w * 4, 1}; }
artgpu_rgb mk_dev_rgb(float *const p[3], int w, int h, size_t stride)
{
    const auto plane = [&](int k) { return artgpu_plane{p[k], w, h, (int64_t)stride * 4, 1}; };
    return artgpu_rgb{plane(0), plane(1), plane(2)};
}

int bind_rgb(artgpu_ctx *ctx, const artgpu_rgb *img, int slot, bool copy_in, DevRGB *d, const char *what)
{
    const artgpu_plane *pl[3] = {&img->r, &img->g, &img->b};
    for (int k = 0; k < 3; ++k) {
        if (!plane_ok(pl[k]) || pl[k]->w != img->r.w || pl[k]->h != img->r.h)
            return fail(ctx, ARTGPU_EINVAL, "%s: plane %d has a bad pointer/size/stride", what, k);
        if ((pl[k]->on_device != 0) != (img->r.on_device != 0) || pl[k]->row_stride_bytes != img->r.row_stride_bytes)
            return fail(ctx, ARTGPU_EINVAL, "%s: planes must share residency and row stride", what);
    }
    d->w = img->r.w; d->h = img->r.h;
    if (img->r.on_device) {
        for (int k = 0; k < 3; ++k) d->p[k] = pl[k]->p;
        d->stride = (size_t)(img->r.row_stride_bytes / 4);
        d->staged = false;
        return ARTGPU_OK;
    }
    const size_t rowb = (size_t)d->w * 4;
    for (int k = 0; k < 3; ++k) {
        int rc = ensure(ctx, &ctx->stage[slot + k], &ctx->stage_bytes[slot + k], rowb * d->h);
        if (rc) return rc;
        d->p[k] = ctx->stage[slot + k];
        if (copy_in)
            HIPCHK(ctx, hipMemcpy2DAsync(d->p[k], rowb, pl[k]->p, (size_t)pl[k]->row_stride_bytes, rowb, d->h, hipMemcpyHostToDevice, ctx->stream));
    }
    d->stride = d->w;
    d->staged = true;
    return ARTGPU_OK;
}

int unbind_rgb(artgpu_ctx *ctx, artgpu_rgb *img, const DevRGB *d)
{
    if (!d->staged) return ARTGPU_OK;
    artgpu_plane *pl[3] = {&img->r, &img->g, &img->b};
    const size_t rowb = (size_t)d->w * 4;
    for (int k = 0; k < 3; ++k)
        HIPCHK(ctx, hipMemcpy2DAsync(pl[k]->p, (size_t)pl[k]->row_stride_bytes, d->p[k], rowb, rowb, d->h, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ARTGPU_OK;
}

int pool_get(artgpu_ctx *ctx, int slot, size_t bytes, float **out)
{
    int rc = ensure(ctx, &ctx->pool[slot], &ctx->pool_bytes[slot], bytes);
    *out = ctx->pool[slot];
    return rc;
}

// contiguous device working copy of one plane (host planes are staged, strided device planes copied)
int plane_to_pool(artgpu_ctx *ctx, const artgpu_plane *pl, int slot, float **out)
{
    const size_t rowb = (size_t)pl->w * 4;
    int rc = pool_get(ctx, slot, rowb * pl->h, out);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpy2DAsync(*out, rowb, pl->p, (size_t)pl->row_stride_bytes, rowb, pl->h,
                                 pl->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    return ARTGPU_OK;
}
int pool_to_plane(artgpu_ctx *ctx, const float *src, artgpu_plane *pl)
{
    const size_t rowb = (size_t)pl->w * 4;
    HIPCHK(ctx, hipMemcpy2DAsync(pl->p, (size_t)pl->row_stride_bytes, src, rowb, rowb, pl->h,
                                 pl->on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    if (!pl->on_device) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ARTGPU_OK;
}

// A kernel that gave up a bounded wait (the fused shrink pass: a strip whose predecessor did not hand down a block within five seconds) says so in
// pinned host words and runs to its end with wrong coefficients instead of trapping -- a trap aborts the host process inside the runtime.  The
// library reads the words wherever it has just waited for the stream and turns them into ARTGPU_EHIP with the band / strip / block in
// artgpu_last_error (fail() appends them); the frame in flight is invalid, the context stays usable.
int check_async_faults(artgpu_ctx *ctx)
{
    if (ctx->fs_diag && (unsigned)ctx->fs_diag[0] == 0xF5D1A600u) return fail(ctx, ARTGPU_EHIP, "a kernel gave up a bounded wait: the results of the calls since the last synchronisation are invalid");
    return ARTGPU_OK;
}

StageScope::push_fn &StageScope::push() { static push_fn f = nullptr; return f; }
StageScope::pop_fn &StageScope::pop() { static pop_fn f = nullptr; return f; }
StageScope::StageScope(artgpu_ctx *c, const char *n) : ctx(c), name(n), range(false)
{
    if (!ctx) return;
    if (ctx->shared.opt_roctx) {
        static bool tried = false;
        if (!tried) {
            tried = true;
            void *h = nullptr;
            for (const char *lib : {"libroctx64.so.4", "libroctx64.so", "/opt/rocm/lib/libroctx64.so"})
                if ((h = dlopen(lib, RTLD_NOW | RTLD_GLOBAL))) break;
            if (h) {
                push() = reinterpret_cast<push_fn>(dlsym(h, "roctxRangePushA"));
                pop() = reinterpret_cast<pop_fn>(dlsym(h, "roctxRangePop"));
            }
        }
        if (push() && pop()) { push()(name); range = true; }
    }
    if (ctx->shared.progress_fn) ctx->shared.progress_fn(ctx->shared.progress_user, name, 0.0);
}
StageScope::~StageScope()
{
    if (!ctx) return;
    if (ctx->shared.progress_fn) ctx->shared.progress_fn(ctx->shared.progress_user, name, 1.0);
    if (range) pop()();
}

int lab_tabs_dev(artgpu_ctx *ctx, float **tabs_out)
{
    return const_table_dev(ctx, P_LABTABS, 4 * 65536, build_lab_tabs, "Lab tables", tabs_out);
}

} } // namespace artgpu::api

extern "C" {

const char *artgpu_version(void) { return "artgpu 0.1 (gfx950)"; }

int artgpu_create(int hip_device, artgpu_ctx **out)
{
    if (!out) return ARTGPU_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || hip_device < 0 || hip_device >= n) return ARTGPU_EHIP;
    artgpu_ctx *ctx = new (std::nothrow) artgpu_ctx;
    if (!ctx) return ARTGPU_ENOMEM;
    ctx->device = hip_device;
    if (hipSetDevice(hip_device) != hipSuccess) { delete ctx; return ARTGPU_EHIP; }
    for (int k = 0; k < 3; ++k)
        if (hipEventCreate(&ctx->ev[k]) != hipSuccess) {
            for (int j = 0; j < k; ++j) (void)hipEventDestroy(ctx->ev[j]);     // the events created so far
            delete ctx;
            return ARTGPU_EHIP;
        }
    *out = ctx;
    return ARTGPU_OK;
}

int artgpu_destroy(artgpu_ctx *ctx)
{
    if (!ctx) return ARTGPU_EINVAL;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->arena) (void)hipFree(ctx->arena);
    for (int k = 0; k < artgpu_ctx::NSTAGE; ++k)
        if (ctx->stage[k]) (void)hipFree(ctx->stage[k]);
    if (ctx->lut) (void)hipFree(ctx->lut);
    if (ctx->tab_ring) (void)hipHostFree(ctx->tab_ring);
    if (ctx->fs_diag) (void)hipHostFree(ctx->fs_diag);
    if (ctx->sh_host) (void)hipHostFree(ctx->sh_host);
    if (ctx->sh_ev) (void)hipEventDestroy(ctx->sh_ev);
    if (ctx->tab_ev) (void)hipEventDestroy(ctx->tab_ev);
    if (ctx->bbox) (void)hipFree(ctx->bbox);
    if (ctx->amz_lists) (void)hipFree(ctx->amz_lists);
    if (ctx->rcd_counter) (void)hipFree(ctx->rcd_counter);
    for (int k = 0; k < artgpu_ctx::NPOOL; ++k)
        if (ctx->pool[k]) (void)hipFree(ctx->pool[k]);
    for (int k = 0; k < 3; ++k)
        if (ctx->ev[k]) (void)hipEventDestroy(ctx->ev[k]);
    for (artgpu_ctx *l : ctx->lanes) (void)artgpu_destroy(l);
    ctx->lanes.clear();
    clut_release(ctx->pipe_fs_own);
    if (ctx->io_up) { (void)hipStreamSynchronize(ctx->io_up); (void)hipStreamDestroy(ctx->io_up); }
    if (ctx->io_down) { (void)hipStreamSynchronize(ctx->io_down); (void)hipStreamDestroy(ctx->io_down); }
    for (int k = 0; k < 8; ++k)
        if (ctx->io_ev[k]) (void)hipEventDestroy(ctx->io_ev[k]);
    if (ctx->io_host) (void)hipHostFree(ctx->io_host);
    if (ctx->owns_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    for (int k = 0; k < 2; ++k)
        if (ctx->aux_ev[k]) (void)hipEventDestroy(ctx->aux_ev[k]);
    if (ctx->aux) { (void)hipStreamSynchronize(ctx->aux); (void)hipStreamDestroy(ctx->aux); }
    for (int k = 0; k < 2; ++k)
        if (ctx->dn_ev[k]) (void)hipEventDestroy(ctx->dn_ev[k]);
    if (ctx->dn_stream[0]) { (void)hipStreamSynchronize(ctx->dn_stream[0]); (void)hipStreamDestroy(ctx->dn_stream[0]); }
    for (int k = 0; k < 2; ++k)
        if (ctx->amz_ev[k]) (void)hipEventDestroy(ctx->amz_ev[k]);
    if (ctx->amz_side) { (void)hipStreamSynchronize(ctx->amz_side); (void)hipStreamDestroy(ctx->amz_side); }
    delete ctx;
    return ARTGPU_OK;
}

const char *artgpu_last_error(const artgpu_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int artgpu_set_stream(artgpu_ctx *ctx, void *hip_stream)
{
    if (!ctx) return ARTGPU_EINVAL;
    hipStream_t next = static_cast<hipStream_t>(hip_stream);
    if (next == ctx->stream) return ARTGPU_OK;
    // The context's scratch planes and the tables it keeps between calls (curves, gamma / Lab / DCT tables) were last written on the
    // stream it is leaving: the new stream's work is ordered behind that.  (A previous stream that no longer exists cannot be waited
    // for -- its work is done by definition -- so a failure here is not an error.)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) {
        if (hipEventRecord(ev, ctx->stream) == hipSuccess) (void)hipStreamWaitEvent(next, ev, 0);
        (void)hipEventDestroy(ev);
    }
    (void)hipGetLastError();
    ctx->stream = next;
    return ARTGPU_OK;
}

int artgpu_synchronize(artgpu_ctx *ctx)
{
    if (!ctx) return ARTGPU_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return check_async_faults(ctx);
}

int artgpu_set_curve_tail(artgpu_ctx *ctx, int kind, double y_last)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (kind < ARTGPU_CURVE_TAIL_LUT || kind > ARTGPU_CURVE_TAIL_HOST) return fail(ctx, ARTGPU_EINVAL, "set_curve_tail: kind %d (a parametric curve: artgpu_set_curve_tail_parametric)", kind);
    ctx->shared.curve_tail_kind = kind;
    ctx->shared.curve_tail_y = y_last;
    return ARTGPU_OK;
}

int artgpu_set_curve_tail_parametric(artgpu_ctx *ctx, const double *p, int np)
{
    if (!ctx) return ARTGPU_EINVAL;
    // DiagonalCurve's constructor (diagonalcurves.cc:106-131): eight or nine parameters behind the kind; a curve whose four slider values
    // are all zero is the identity there (and `identity` curves never reach setLutVal with a Curve object: ARTGPU_CURVE_TAIL_LUT)
    if (!p || (np != 8 && np != 9)) return fail(ctx, ARTGPU_EINVAL, "set_curve_tail_parametric: 8 or 9 parameters (p[0] = DCT_Parametric)");
    if (p[4] == 0.0 && p[5] == 0.0 && p[6] == 0.0 && p[7] == 0.0) return fail(ctx, ARTGPU_EINVAL, "set_curve_tail_parametric: an identity curve has no Curve object (ARTGPU_CURVE_TAIL_LUT)");
    pc_init(ctx->shared.curve_tail_pc, p, np);
    ctx->shared.curve_tail_kind = ARTGPU_CURVE_TAIL_PARAMETRIC;
    return ARTGPU_OK;
}

int artgpu_get_option(artgpu_ctx *ctx, const char *name, long *value)
{
    if (!ctx || !name || !value) return ARTGPU_EINVAL;
    const std::string n(name);
    if (n.rfind("amaze_counter", 0) == 0 && n.size() == 14 && n[13] >= '0' && n[13] <= '7') {
        // counters of the last AMaZE call (0 entries pulled by stream workgroups, 1 pulls that found nothing, 2 entries published,
        // 3 tiles handed to the arena list, 4-6 what the arena kernel saw: listed tiles, queue taken, queue reserved)
        if (!ctx->amz_lists || ctx->amz_nstream <= 0) { *value = 0; return ARTGPU_OK; }
        HIPCHK(ctx, hipSetDevice(ctx->device));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        const size_t nfixed = (((size_t)ctx->amz_nstream + (1 + ctx->amz_narena) + (1 + ctx->amz_narena + ctx->amz_nstream) + 3) / 4) * 4;
        int v = 0;
        HIPCHK(ctx, hipMemcpy(&v, reinterpret_cast<int *>(ctx->amz_lists) + nfixed + 4 + 2 * (size_t)ctx->amz_nstream + (n[13] - '0'), sizeof(int), hipMemcpyDeviceToHost));
        *value = v;
        return ARTGPU_OK;
    }
    if (n == "dn_mad_fold") { *value = ctx->shared.opt_dn_mad_fold; return ARTGPU_OK; }
    if (n == "cu_reserve") { *value = ctx->shared.opt_cu_reserve; return ARTGPU_OK; }     // (the caller's value: a batch never writes it)
    if (n == "io_direct") { *value = ctx->shared.opt_io_direct; return ARTGPU_OK; }
    if (n == "te_group_thread") { *value = ctx->shared.opt_te_group_thread; return ARTGPU_OK; }
    if (n == "te_fuse_upsample") { *value = ctx->shared.opt_te_fuse_upsample; return ARTGPU_OK; }
    if (n.rfind("dn_mad_bits", 0) == 0 && n.size() > 11) {
        // the bit pattern of word k (0 .. 95) of the last RGB_denoise call's SQR(MadRgb) block: L at 0, a at 32, b at 64 -- or, with one MadRgb
        // launch set for the three channels, all bands back to back from 0 (DESIGN 28 lists a frame's median bins from these)
        const int k = std::atoi(n.c_str() + 11);
        if (k < 0 || k > 95 || !ctx->dn_fold_flags) return fail(ctx, ARTGPU_EINVAL, "get_option: %s: word 0 .. 95 of a context that has denoised", name);
        HIPCHK(ctx, hipSetDevice(ctx->device));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        int v = 0;
        HIPCHK(ctx, hipMemcpy(&v, ctx->dn_fold_flags - 96 + k, sizeof v, hipMemcpyDeviceToHost));
        *value = v;
        return ARTGPU_OK;
    }
    if (n == "dn_mad_fold_settled" || n == "dn_mad_fold_fallback") {
        // the last RGB_denoise call on this context: bands whose median came from the analysis kernels' counts / bands the counts could not
        // settle, which took the full histogram (both 0 when the call did not fold)
        HIPCHK(ctx, hipSetDevice(ctx->device));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        int flags[96] = {};
        if (ctx->dn_fold_nranges) HIPCHK(ctx, hipMemcpy(flags, ctx->dn_fold_flags, sizeof flags, hipMemcpyDeviceToHost));
        const int want = n == "dn_mad_fold_settled" ? 1 : 2;
        long cnt = 0;
        for (int r = 0; r < ctx->dn_fold_nranges; ++r)
            for (int k = 0; k < ctx->dn_fold_ranges[r][1]; ++k) cnt += flags[ctx->dn_fold_ranges[r][0] + k] == want;
        *value = cnt;
        return ARTGPU_OK;
    }
    return fail(ctx, ARTGPU_EINVAL, "get_option: unknown option '%s'", name);
}

int artgpu_set_option(artgpu_ctx *ctx, const char *name, long value)
{
    if (!ctx || !name) return ARTGPU_EINVAL;
    const std::string n(name);
    if (n == "amaze_path") { if (value < 0 || value > 1) return fail(ctx, ARTGPU_EINVAL, "amaze_path: 0 or 1"); ctx->shared.opt_amaze_path = (int)value; }
    else if (n == "amaze_split") ctx->shared.opt_amaze_split = value != 0;
    else if (n == "amaze_overlap") ctx->shared.opt_amaze_overlap = value != 0;
    else if (n == "amaze_grid") { if (value < 0) return fail(ctx, ARTGPU_EINVAL, "amaze_grid: >= 0"); ctx->shared.opt_amaze_grid = (int)value; }
    else if (n == "amaze_zero_mask") ctx->shared.opt_amaze_zero_mask = value;
    else if (n == "amaze_zero_frame") ctx->shared.opt_amaze_zero_frame = (int)value;
    else if (n == "amaze_poison") ctx->shared.opt_amaze_poison = (int)value;
    else if (n == "roctx") ctx->shared.opt_roctx = value != 0;
    else if (n == "dn_streams") ctx->shared.opt_dn_streams = value != 0;
    else if (n == "dn_fused") ctx->shared.opt_dn_fused = (int)value;
    else if (n == "dn_mad_fold") ctx->shared.opt_dn_mad_fold = value != 0;
    else if (n == "dn_mad_fold_grid") { if (value < 0 || value > 65536) return fail(ctx, ARTGPU_EINVAL, "dn_mad_fold_grid: 0 (default) .. 65536 workgroups"); ctx->shared.opt_dn_mad_fold_grid = (int)value; }
    else if (n == "dn_detail_plain") { if (value < 0 || value > 3) return fail(ctx, ARTGPU_EINVAL, "dn_detail_plain: 0 .. 3"); ctx->shared.opt_dn_detail_plain = (int)value; }
    else if (n == "dn_debug_stall") ctx->shared.opt_dn_debug_stall = (int)value;
    else if (n == "dn_wait_ms") ctx->shared.opt_dn_wait_ms = value < 0 ? 0 : value;
    else if (n == "lut_lds") ctx->shared.opt_lut_lds = value != 0;
    else if (n == "te_group_thread") ctx->shared.opt_te_group_thread = value != 0;
    else if (n == "te_fuse_upsample") ctx->shared.opt_te_fuse_upsample = value != 0;
    else if (n == "sharpen_fused") ctx->shared.opt_sharpen_fused = value != 0;
    else if (n == "cu_reserve") { if (value < 0 || value > 4096) return fail(ctx, ARTGPU_EINVAL, "cu_reserve: 0 .. 4096"); ctx->shared.opt_cu_reserve = (int)value; }
    else if (n == "io_direct") { if (value < -1 || value > 4096) return fail(ctx, ARTGPU_EINVAL, "io_direct: -1 (automatic), 0 .. 4096 workgroups"); ctx->shared.opt_io_direct = (int)value; }
    else if (n == "rcd_rows") { if (value != 4 && value != 8) return fail(ctx, ARTGPU_EINVAL, "rcd_rows: 4 or 8"); ctx->shared.opt_rcd_rows = (int)value; }
    else return fail(ctx, ARTGPU_EINVAL, "set_option: unknown option '%s'", name);
    return ARTGPU_OK;
}

int artgpu_set_progress_callback(artgpu_ctx *ctx, artgpu_progress_fn fn, void *user)
{
    if (!ctx) return ARTGPU_EINVAL;
    ctx->shared.progress_fn = fn;
    ctx->shared.progress_user = user;
    return ARTGPU_OK;
}

int artgpu_enable_timing(artgpu_ctx *ctx, int enable)
{
    if (!ctx) return ARTGPU_EINVAL;
    ctx->timing = enable != 0;
    return ARTGPU_OK;
}

int artgpu_get_timings(const artgpu_ctx *ctx, artgpu_timings *out)
{
    if (!ctx || !out) return ARTGPU_EINVAL;
    *out = ctx->last;
    return ARTGPU_OK;
}

size_t artgpu_scratch_bytes(const artgpu_ctx *ctx)
{
    if (!ctx) return 0;
    size_t s = ctx->arena_bytes;
    for (int k = 0; k < artgpu_ctx::NSTAGE; ++k) s += ctx->stage_bytes[k];
    s += ctx->lut_bytes;
    for (int k = 0; k < artgpu_ctx::NPOOL; ++k) s += ctx->pool_bytes[k];
    return s;
}

int artgpu_trim_scratch(artgpu_ctx *ctx)
{
    if (!ctx) return ARTGPU_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // nothing may still be running on what is about to be freed: the context's stream and the side streams it forks to
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->aux) HIPCHK(ctx, hipStreamSynchronize(ctx->aux));
    if (ctx->dn_stream[0]) HIPCHK(ctx, hipStreamSynchronize(ctx->dn_stream[0]));
    if (ctx->amz_side) HIPCHK(ctx, hipStreamSynchronize(ctx->amz_side));
    if (ctx->io_up) HIPCHK(ctx, hipStreamSynchronize(ctx->io_up));
    if (ctx->io_down) HIPCHK(ctx, hipStreamSynchronize(ctx->io_down));
    auto drop = [](float **p, size_t *b) { if (*p) (void)hipFree(*p); *p = nullptr; *b = 0; };
    drop(&ctx->arena, &ctx->arena_bytes);
    for (int k = 0; k < artgpu_ctx::NSTAGE; ++k) drop(&ctx->stage[k], &ctx->stage_bytes[k]);
    for (int k = 0; k < artgpu_ctx::NPOOL; ++k) drop(&ctx->pool[k], &ctx->pool_bytes[k]);
    ctx->batch_px = 0;
    // host-side records of what pool slots held: the tables are gone with them
    ctx->gam_tab = nullptr;
    ctx->dn_fold_flags = nullptr; ctx->dn_fold_nranges = 0;
    ctx->ncurve_host.clear();
    for (int k = 0; k < 3; ++k) ctx->rgbcurve_host[k].clear();
    ctx->te_lut_dev = nullptr;
    ctx->rs_dev = nullptr;
    int rc = ARTGPU_OK;
    for (artgpu_ctx *l : ctx->lanes) { const int r = artgpu_trim_scratch(l); if (r && !rc) rc = r; }
    return rc;
}

int artgpu_get_image(artgpu_ctx *ctx, const artgpu_rgb *planes, int sx1, int sy1, const float mul[3],
                     int do_clip, const double *mat, artgpu_rgb *image)
{
    StageScope scope_(ctx, "RawImageSource::getImage");
    return artgpu_get_image_skip(ctx, planes, sx1, sy1, 1, mul, do_clip, mat, image);
}

int artgpu_get_image_skip(artgpu_ctx *ctx, const artgpu_rgb *planes, int sx1, int sy1, int skip, const float mul[3],
                          int do_clip, const double *mat, artgpu_rgb *image)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!planes || !image || !mul) return fail(ctx, ARTGPU_EINVAL, "get_image: null argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB src, dst;
    int rc = bind_rgb(ctx, planes, 1, true, &src, "get_image(planes)");
    if (rc) return rc;
    rc = bind_rgb(ctx, image, 4, false, &dst, "get_image(image)");
    if (rc) return rc;
    if (skip < 1 || skip > src.w || skip > src.h) return fail(ctx, ARTGPU_EINVAL, "get_image: skip %d", skip);
    // transformRect (rawimagesource.cc:745-747): the caller's image is ceil(crop / skip); the last window may be pulled back inside
    if (sx1 < 0 || sy1 < 0 || sx1 + (dst.w - 1) * skip >= src.w || sy1 + (dst.h - 1) * skip >= src.h)
        return fail(ctx, ARTGPU_EINVAL, "get_image: crop %dx%d+%d+%d (skip %d) outside the %dx%d planes", dst.w, dst.h, sx1, sy1, skip, src.w, src.h);
    PixArgs a = {};
    for (int k = 0; k < 3; ++k) { a.src[k] = src.p[k]; a.dst[k] = dst.p[k]; a.mul[k] = mul[k]; }
    a.src_stride = src.stride; a.dst_stride = dst.stride;
    a.sx1 = sx1; a.sy1 = sy1; a.w = dst.w; a.h = dst.h;
    a.skip = skip; a.src_w = src.w; a.src_h = src.h;
    a.has_mul = 1; a.do_clip = do_clip ? 1 : 0;
    a.has_mat = mat ? 1 : 0;
    if (mat) for (int k = 0; k < 9; ++k) a.mat[k] = mat[k];
    HIPCHK(ctx, launch_get_image_convert(a, ctx->stream));
    return unbind_rgb(ctx, image, &dst);
}

int artgpu_convert_color_space(artgpu_ctx *ctx, artgpu_rgb *image, const double mat[9])
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!image || !mat) return fail(ctx, ARTGPU_EINVAL, "convert_color_space: null argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    int rc = bind_rgb(ctx, image, 4, true, &d, "convert_color_space");
    if (rc) return rc;
    PixArgs a = {};
    for (int k = 0; k < 3; ++k) { a.src[k] = d.p[k]; a.dst[k] = d.p[k]; }
    a.src_stride = d.stride; a.dst_stride = d.stride; a.w = d.w; a.h = d.h;
    a.has_mul = 0; a.has_mat = 1;
    for (int k = 0; k < 9; ++k) a.mat[k] = mat[k];
    HIPCHK(ctx, launch_get_image_convert(a, ctx->stream));
    return unbind_rgb(ctx, image, &d);
}

int artgpu_exposure(artgpu_ctx *ctx, artgpu_rgb *image, float exp_scale, float black)
{
    StageScope scope_(ctx, "ImProcFunctions::expcomp");
    if (!ctx) return ARTGPU_EINVAL;
    if (!image) return fail(ctx, ARTGPU_EINVAL, "exposure: null image");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    int rc = bind_rgb(ctx, image, 4, true, &d, "exposure");
    if (rc) return rc;
    PixArgs a = {};
    for (int k = 0; k < 3; ++k) a.dst[k] = d.p[k];
    a.dst_stride = d.stride; a.w = d.w; a.h = d.h;
    a.exp_scale = exp_scale; a.black = black;
    HIPCHK(ctx, launch_exposure(a, ctx->stream));
    return unbind_rgb(ctx, image, &d);
}

// the 65536-entry curve of a tone-curve call -> ctx->lut.  The same curve frame after frame (a batch) is uploaded once: a copy from
// pageable host memory stalls the stream and the enqueueing thread for ~60 us each time.
static int upload_curve(artgpu_ctx *ctx, const float *lut65536)
{
    int rc = ensure(ctx, &ctx->lut, &ctx->lut_bytes, 65536 * sizeof(float));
    if (rc) return rc;
    if (ctx->lut_host.size() == 65536 && std::memcmp(ctx->lut_host.data(), lut65536, 65536 * sizeof(float)) == 0) return ARTGPU_OK;
    ctx->lut_host.assign(lut65536, lut65536 + 65536);
    // from the context's own copy: the caller's array may change as soon as this call returns
    hipError_t e = hipMemcpyAsync(ctx->lut, ctx->lut_host.data(), 65536 * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        ctx->lut_host.clear();      // the cache only describes ctx->lut after a copy that succeeded
        return fail(ctx, ARTGPU_EHIP, "tone curve upload failed: %s", hipGetErrorString(e));
    }
    return ARTGPU_OK;
}

int artgpu_tone_curve(artgpu_ctx *ctx, artgpu_rgb *image, int mode, const float *lut65536, float whitept, int filmlike_clip)
{
    StageScope scope_(ctx, "ImProcFunctions::toneCurve");
    if (!ctx) return ARTGPU_EINVAL;
    if (!image) return fail(ctx, ARTGPU_EINVAL, "tone_curve: null image");
    if (mode != ARTGPU_TONE_STD) return fail(ctx, ARTGPU_EUNSUPPORTED, "tone_curve: curve mode %d is not on the device path", mode);
    if (!(whitept > 0.f)) return fail(ctx, ARTGPU_EINVAL, "tone_curve: whitept %g", (double)whitept);
    if (whitept > 1.f && ctx->shared.curve_tail_kind == ARTGPU_CURVE_TAIL_HOST)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "tone_curve: whitept %g needs the curve beyond the LUT (artgpu_set_curve_tail)", (double)whitept);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    int rc = bind_rgb(ctx, image, 4, true, &d, "tone_curve");
    if (rc) return rc;
    PixArgs a = {};
    for (int k = 0; k < 3; ++k) a.dst[k] = d.p[k];
    a.dst_stride = d.stride; a.w = d.w; a.h = d.h;
    a.do_clip = filmlike_clip ? 1 : 0; a.whitept = whitept;
    a.tail_kind = ctx->shared.curve_tail_kind == ARTGPU_CURVE_TAIL_HOST ? 0 : ctx->shared.curve_tail_kind; a.tail_y = ctx->shared.curve_tail_y; a.tail_pc = ctx->shared.curve_tail_pc;
    if (lut65536) {
        if ((rc = upload_curve(ctx, lut65536))) return rc;
        a.lut = ctx->lut;
    }
    a.no_lds_lut = !ctx->shared.opt_lut_lds; a.cu_reserve = cu_reserve_of(ctx);
    HIPCHK(ctx, launch_tone_std(a, ctx->stream));
    return unbind_rgb(ctx, image, &d);
}

// ---------------------------------------------------------------------------------------------
// wavelet_decomposition
// ---------------------------------------------------------------------------------------------
} // extern "C"

struct artgpu_wavelet {
    int w = 0, h = 0, w2 = 0, h2 = 0, nlevels = 0;
    float *bands = nullptr;   // nlevels * 3 * n floats
    float *lowpass[2] = {nullptr, nullptr};
    int cur = 0;              // lowpass[cur] is coeff0
    size_t n = 0;
    float *band(int l, int dir) const { return bands + ((size_t)l * 3 + (dir - 1)) * n; }
};

namespace {
int wavelet_skip(int level) { return level <= 1 ? 1 : 1 << (level - 1); }
}

extern "C" {

int artgpu_wavelet_decompose(artgpu_ctx *ctx, const artgpu_plane *src, int maxlvl, artgpu_wavelet **out)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(src) || !out || maxlvl < 1 || maxlvl > 9) return fail(ctx, ARTGPU_EINVAL, "wavelet_decompose: bad arguments");
    *out = nullptr;
    const int w = src->w, h = src->h, w2 = (w + 1) / 2, h2 = (h + 1) / 2;
    if ((w2 < h2 ? w2 : h2) < 2 * wavelet_skip(maxlvl - 1) || w < 8 || h < 8)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "wavelet_decompose: %dx%d too small for %d levels", w, h, maxlvl);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const float *dsrc = src->p;
    size_t sstride = (size_t)(src->row_stride_bytes / 4);
    if (!src->on_device) {
        int rc = ensure(ctx, &ctx->stage[0], &ctx->stage_bytes[0], (size_t)w * h * 4);
        if (rc) return rc;
        HIPCHK(ctx, hipMemcpy2DAsync(ctx->stage[0], (size_t)w * 4, src->p, (size_t)src->row_stride_bytes, (size_t)w * 4, h, hipMemcpyHostToDevice, ctx->stream));
        dsrc = ctx->stage[0];
        sstride = w;
    }
    artgpu_wavelet *wv = new (std::nothrow) artgpu_wavelet;
    if (!wv) return fail(ctx, ARTGPU_ENOMEM, "wavelet_decompose: out of host memory");
    wv->w = w; wv->h = h; wv->w2 = w2; wv->h2 = h2; wv->nlevels = maxlvl; wv->n = (size_t)w2 * h2;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&wv->bands), (size_t)maxlvl * 3 * wv->n * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&wv->lowpass[0]), wv->n * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&wv->lowpass[1]), wv->n * sizeof(float));
    if (e != hipSuccess) {
        artgpu_wavelet_free(ctx, wv);
        return fail(ctx, ARTGPU_ENOMEM, "wavelet_decompose: hipMalloc failed: %s", hipGetErrorString(e));
    }
    WaveArgs a = {};
    a.w = w; a.h = h; a.w2 = w2; a.h2 = h2;
    for (int l = 0; l < maxlvl; ++l) {
        a.b1 = wv->band(l, 1); a.b2 = wv->band(l, 2); a.b3 = wv->band(l, 3);
        hipError_t le;
        if (l == 0) {
            a.src = dsrc; a.src_stride = sstride; a.lo = wv->lowpass[0];
            wv->cur = 0;
            le = launch_wavelet_analysis0(a, ctx->stream);
        } else {
            a.src = wv->lowpass[wv->cur]; a.lo = wv->lowpass[wv->cur ^ 1]; a.skip = wavelet_skip(l);
            le = launch_wavelet_haar_analysis(a, ctx->stream);
            wv->cur ^= 1;
        }
        if (le != hipSuccess) {
            artgpu_wavelet_free(ctx, wv);
            return fail(ctx, ARTGPU_EHIP, "wavelet_decompose: launch failed: %s", hipGetErrorString(le));
        }
    }
    if (!src->on_device) {
        const hipError_t se = hipStreamSynchronize(ctx->stream);
        if (se != hipSuccess) {
            artgpu_wavelet_free(ctx, wv);
            return fail(ctx, ARTGPU_EHIP, "wavelet_decompose: %s", hipGetErrorString(se));
        }
    }
    *out = wv;
    return ARTGPU_OK;
}

int artgpu_wavelet_info(const artgpu_wavelet *wv, int32_t *w2, int32_t *h2, int32_t *nlevels)
{
    if (!wv) return ARTGPU_EINVAL;
    if (w2) *w2 = wv->w2;
    if (h2) *h2 = wv->h2;
    if (nlevels) *nlevels = wv->nlevels;
    return ARTGPU_OK;
}

int artgpu_wavelet_get_band(artgpu_ctx *ctx, const artgpu_wavelet *wv, int level, int dir, float *dst, int on_device)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!wv || !dst || dir < 0 || dir > 3 || (dir > 0 && (level < 0 || level >= wv->nlevels))) return fail(ctx, ARTGPU_EINVAL, "wavelet_get_band: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const float *p = dir == 0 ? wv->lowpass[wv->cur] : wv->band(level, dir);
    HIPCHK(ctx, hipMemcpyAsync(dst, p, wv->n * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    if (!on_device) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ARTGPU_OK;
}

int artgpu_wavelet_set_band(artgpu_ctx *ctx, artgpu_wavelet *wv, int level, int dir, const float *src, int on_device)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!wv || !src || dir < 0 || dir > 3 || (dir > 0 && (level < 0 || level >= wv->nlevels))) return fail(ctx, ARTGPU_EINVAL, "wavelet_set_band: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    float *p = dir == 0 ? wv->lowpass[wv->cur] : wv->band(level, dir);
    HIPCHK(ctx, hipMemcpyAsync(p, src, wv->n * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    if (!on_device) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ARTGPU_OK;
}

int artgpu_wavelet_reconstruct(artgpu_ctx *ctx, artgpu_wavelet *wv, artgpu_plane *dst, float blend)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!wv || !plane_ok(dst) || dst->w != wv->w || dst->h != wv->h) return fail(ctx, ARTGPU_EINVAL, "wavelet_reconstruct: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    float *ddst = dst->p;
    size_t dstride = (size_t)(dst->row_stride_bytes / 4);
    if (!dst->on_device) {
        int rc = ensure(ctx, &ctx->stage[0], &ctx->stage_bytes[0], (size_t)wv->w * wv->h * 4);
        if (rc) return rc;
        // dst participates in the blend (dst*(1-blend) + blend*4*tot): bring the host contents over
        HIPCHK(ctx, hipMemcpy2DAsync(ctx->stage[0], (size_t)wv->w * 4, dst->p, (size_t)dst->row_stride_bytes, (size_t)wv->w * 4, wv->h, hipMemcpyHostToDevice, ctx->stream));
        ddst = ctx->stage[0];
        dstride = wv->w;
    }
    WaveArgs a = {};
    a.w = wv->w; a.h = wv->h; a.w2 = wv->w2; a.h2 = wv->h2; a.blend = blend;
    for (int l = wv->nlevels - 1; l > 0; --l) {
        a.src = wv->lowpass[wv->cur]; a.lo = wv->lowpass[wv->cur ^ 1];
        a.b1 = wv->band(l, 1); a.b2 = wv->band(l, 2); a.b3 = wv->band(l, 3); a.skip = wavelet_skip(l);
        HIPCHK(ctx, launch_wavelet_haar_synthesis(a, ctx->stream));
        wv->cur ^= 1;
    }
    a.src = wv->lowpass[wv->cur];
    a.b1 = wv->band(0, 1); a.b2 = wv->band(0, 2); a.b3 = wv->band(0, 3);
    a.dst = ddst; a.dst_stride = dstride;
    HIPCHK(ctx, launch_wavelet_synthesis0(a, ctx->stream));
    if (!dst->on_device) {
        HIPCHK(ctx, hipMemcpy2DAsync(dst->p, (size_t)dst->row_stride_bytes, ddst, (size_t)wv->w * 4, (size_t)wv->w * 4, wv->h, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return ARTGPU_OK;
}

int artgpu_wavelet_free(artgpu_ctx *ctx, artgpu_wavelet *wv)
{
    if (!wv) return ARTGPU_EINVAL;
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
    if (wv->bands) (void)hipFree(wv->bands);
    if (wv->lowpass[0]) (void)hipFree(wv->lowpass[0]);
    if (wv->lowpass[1]) (void)hipFree(wv->lowpass[1]);
    delete wv;
    return ARTGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// RGB_denoise (wavelet part)
// ---------------------------------------------------------------------------------------------
} // extern "C"

namespace {

struct DevDecomp {
    float *bands, *low[2];
    int cur, nlevels, w, h, w2, h2;
    size_t n;
    int *cnt;                   // non-null: decompose with the counting kernels -- MadRgb's low bins of this channel's bands, [3 * nlevels][MAD_FOLD_NB]
    int g0, g1;                 // ... their grids
    float *band(int l, int dir) const { return bands + ((size_t)l * 3 + (dir - 1)) * n; }
};

int decompose_dev(artgpu_ctx *ctx, DevDecomp &d, const float *src, hipStream_t st = nullptr, size_t src_stride = 0)
{
    if (!st) st = ctx->stream;
    WaveArgs a = {};
    a.w = d.w; a.h = d.h; a.w2 = d.w2; a.h2 = d.h2;
    if (d.cnt) HIPCHK(ctx, hipMemsetAsync(d.cnt, 0, (size_t)3 * d.nlevels * MAD_FOLD_NB * sizeof(int), st));
    for (int l = 0; l < d.nlevels; ++l) {
        a.cnt = d.cnt ? d.cnt + (size_t)l * 3 * MAD_FOLD_NB : nullptr;
        a.b1 = d.band(l, 1); a.b2 = d.band(l, 2); a.b3 = d.band(l, 3);
        if (l == 0) {
            a.src = src; a.src_stride = src_stride ? src_stride : (size_t)d.w; a.lo = d.low[0]; d.cur = 0;
            a.cnt_grid = d.g0;
            HIPCHK(ctx, d.cnt ? launch_wavelet_analysis0_count(a, st) : launch_wavelet_analysis0(a, st));
        } else {
            a.src = d.low[d.cur]; a.lo = d.low[d.cur ^ 1]; a.skip = wavelet_skip(l);
            a.cnt_grid = d.g1;
            HIPCHK(ctx, d.cnt ? launch_wavelet_haar_analysis_count(a, st) : launch_wavelet_haar_analysis(a, st));
            d.cur ^= 1;
        }
    }
    return ARTGPU_OK;
}

int reconstruct_dev(artgpu_ctx *ctx, DevDecomp &d, float *dst, hipStream_t st = nullptr)
{
    if (!st) st = ctx->stream;
    WaveArgs a = {};
    a.w = d.w; a.h = d.h; a.w2 = d.w2; a.h2 = d.h2; a.blend = 1.f;
    for (int l = d.nlevels - 1; l > 0; --l) {
        a.src = d.low[d.cur]; a.lo = d.low[d.cur ^ 1];
        a.b1 = d.band(l, 1); a.b2 = d.band(l, 2); a.b3 = d.band(l, 3); a.skip = wavelet_skip(l);
        HIPCHK(ctx, launch_wavelet_haar_synthesis(a, st));
        d.cur ^= 1;
    }
    a.src = d.low[d.cur];
    a.b1 = d.band(0, 1); a.b2 = d.band(0, 2); a.b3 = d.band(0, 3);
    a.dst = dst; a.dst_stride = d.w;
    HIPCHK(ctx, launch_wavelet_synthesis0(a, st));
    return ARTGPU_OK;
}

} // namespace

extern "C" {

int artgpu_wavelet_mad(artgpu_ctx *ctx, const artgpu_wavelet *wv, float *mad_sqr)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!wv || !mad_sqr) return fail(ctx, ARTGPU_EINVAL, "wavelet_mad: null argument");
    if (wv->n > 0x7fffffff) return fail(ctx, ARTGPU_EUNSUPPORTED, "wavelet_mad: band larger than an int holds (MadRgb's datalen is an int)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int nsub = 3 * wv->nlevels;
    float *histo_f, *mad;
    int rc;
    if ((rc = pool_get(ctx, P_HISTO, (size_t)nsub * (65536 + MAD_SCRATCH_INTS_PER_BAND) * 4, &histo_f)) || (rc = pool_get(ctx, P_MAD, 3 * 32 * 4, &mad))) return rc;
    HIPCHK(ctx, launch_mad(wv->bands, wv->n, nsub, reinterpret_cast<int *>(histo_f), mad, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(mad_sqr, mad, (size_t)nsub * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ARTGPU_OK;
}

} // extern "C"

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
int rgb_denoise_args_ok(artgpu_ctx *ctx, const artgpu_denoise_params *p, const float *iws, double scale)
{
    if (p->color_space != 0 && p->color_space != 1) return fail(ctx, ARTGPU_EINVAL, "rgb_denoise: color_space must be 0 (RGB) or 1 (LAB)");
    if (p->color_space == 1 && !iws) return fail(ctx, ARTGPU_EINVAL, "rgb_denoise: LAB mode needs the inverse working-space matrix");
    if (p->chrominance_method != 0 && p->chrominance_method != 1) return fail(ctx, ARTGPU_EINVAL, "rgb_denoise: chrominance_method must be 0 (MANUAL) or 1 (AUTOMATIC)");
    if (!(scale >= 1.0)) return fail(ctx, ARTGPU_EINVAL, "rgb_denoise: scale must be >= 1");
    return ARTGPU_OK;
}

// RGB_denoise on device planes (the caller has checked the parameters and bound the image); `fu`: what the tool around it has fused into
// the first and the last pixel pass
int rgb_denoise_dev(artgpu_ctx *ctx, const DevRGB &d, const artgpu_denoise_params *p, const float ws[9], const float *iws,
                    double expcomp, double scale, const artgpu_plane *ccalc, uint32_t flags, float *nresi, float *highresi, const DnFusion &fu)
{
    const int w = d.w, h = d.h;
    if (w > 32767 || h > 32767) return fail(ctx, ARTGPU_EUNSUPPORTED, "rgb_denoise: the reference holds the size in short (FTblockDN.cc:1779)");
    if (p->luminance == 0 && p->chrominance == 0 && !ccalc) return ARTGPU_OK; // L1655-1668: nothing to do
    const DnPlan pl = dn_plan(w, h, p, scale, expcomp, flags, nresi || highresi, ccalc != nullptr,
                              ctx->shared.opt_dn_streams, ctx->shared.opt_dn_fused, ctx->shared.opt_dn_detail_plain, ctx->shared.opt_dn_wait_ms, ctx->shared.opt_dn_debug_stall, ctx->shared.opt_dn_mad_fold, ctx->shared.opt_dn_mad_fold_grid);
    if (pl.too_small) return fail(ctx, ARTGPU_EUNSUPPORTED, "rgb_denoise: %dx%d too small for %d wavelet levels on the device path", w, h, pl.levwav);
    DnBuffers b;
    int rc = dn_buffers(ctx, pl, ccalc, &b);
    if (rc) return rc;
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

} // namespace

extern "C" {

int artgpu_rgb_denoise(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_denoise_params *p, const float ws[9], const float *iws,
                       double expcomp, double scale, const artgpu_plane *ccalc, uint32_t flags,
                       float *nresi, float *highresi)
{
    StageScope scope_(ctx, "denoise::RGB_denoise");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !p || !ws) return fail(ctx, ARTGPU_EINVAL, "rgb_denoise: null argument");
    int rc = rgb_denoise_args_ok(ctx, p, iws, scale);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "rgb_denoise"))) return rc;
    if ((rc = rgb_denoise_dev(ctx, d, p, ws, iws, expcomp, scale, ccalc, flags, nresi, highresi, DnFusion{}))) return rc;
    return unbind_rgb(ctx, img, &d);
}

static int lab_mode_switch(artgpu_ctx *ctx, artgpu_rgb *img, const double m[9], bool to_lab, const char *who)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !m) return fail(ctx, ARTGPU_EINVAL, "%s: null argument", who);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    float *tabs;
    int rc = lab_tabs_dev(ctx, &tabs);
    if (rc) return rc;
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, who))) return rc;
    LabArgs a = {};
    for (int k = 0; k < 3; ++k) a.img[k] = d.p[k];
    a.stride = d.stride; a.w = d.w; a.h = d.h;
    for (int k = 0; k < 9; ++k) { a.ws[k] = (float)m[k]; a.iws[k] = (float)m[k]; }
    a.cachef = tabs; a.cachefy = tabs + 65536;
    HIPCHK(ctx, to_lab ? launch_rgb_to_lab(a, ctx->stream) : launch_lab_to_rgb(a, ctx->stream));
    return unbind_rgb(ctx, img, &d);
}
int artgpu_rgb_to_lab(artgpu_ctx *ctx, artgpu_rgb *img, const double ws[9]) { return lab_mode_switch(ctx, img, ws, true, "rgb_to_lab"); }
int artgpu_lab_to_rgb(artgpu_ctx *ctx, artgpu_rgb *img, const double iws[9]) { return lab_mode_switch(ctx, img, iws, false, "lab_to_rgb"); }

int artgpu_lab_histogram(artgpu_ctx *ctx, const artgpu_rgb *img, uint32_t hist[65536])
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !hist) return fail(ctx, ARTGPU_EINVAL, "lab_histogram: null argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    artgpu_rgb tmp = *img;
    int rc = bind_rgb(ctx, &tmp, 4, true, &d, "lab_histogram");
    if (rc) return rc;
    float *h;
    if ((rc = pool_get(ctx, P_HISTO, 65536 * 4, &h))) return rc;
    LabArgs a = {};
    for (int k = 0; k < 3; ++k) a.img[k] = d.p[k];
    a.stride = d.stride; a.w = d.w; a.h = d.h; a.hist = reinterpret_cast<unsigned *>(h);
    HIPCHK(ctx, hipMemsetAsync(h, 0, 65536 * 4, ctx->stream));
    HIPCHK(ctx, launch_lab_hist(a, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(hist, h, 65536 * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ARTGPU_OK;
}

int artgpu_lab_adjustments(artgpu_ctx *ctx, artgpu_rgb *img, const float *lcurve, const float *acurve, const float *bcurve, float chroma)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !lcurve || !acurve || !bcurve) return fail(ctx, ARTGPU_EINVAL, "lab_adjustments: null argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    int rc = bind_rgb(ctx, img, 4, true, &d, "lab_adjustments");
    if (rc) return rc;
    float *luts;
    constexpr size_t NL = 32772;       // lcurve padded to a multiple of four floats
    if ((rc = pool_get(ctx, P_PIPE_R, (NL + 2 * 65536) * 4, &luts))) return rc;
    if ((rc = h2d_table(ctx, luts, lcurve, 32770 * 4)) || (rc = h2d_table(ctx, luts + NL, acurve, 65536 * 4)) || (rc = h2d_table(ctx, luts + NL + 65536, bcurve, 65536 * 4))) return rc;
    LabArgs a = {};
    for (int k = 0; k < 3; ++k) a.img[k] = d.p[k];
    a.stride = d.stride; a.w = d.w; a.h = d.h;
    a.lcurve = luts; a.acurve = luts + NL; a.bcurve = luts + NL + 65536; a.chroma = chroma;
    HIPCHK(ctx, launch_lab_adjust(a, ctx->stream));
    rc = unbind_rgb(ctx, img, &d);
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));     // the caller's LUTs may go out of scope
    return ARTGPU_OK;
}

int artgpu_log_encoding(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_logenc_params *p, const double ws[9], int full_width, int full_height)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !p || !ws) return fail(ctx, ARTGPU_EINVAL, "log_encoding: null argument");
    if (!p->enabled) return ARTGPU_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LogEncArgs a = {};
    a.gray = std::pow(2.f, -(float)p->gain + std::log2(0.18f));                                   // ev2gray (L119-122)
    a.shadows_range = (float)p->black_ev;
    a.dynamic_range = (float)std::max(p->white_ev - p->black_ev, 0.5);
    const float b = p->target_gray > 1 && p->target_gray < 100 && a.dynamic_range > 0
        ? logenc_find_gray((float)(std::abs(p->black_ev) / a.dynamic_range), (float)(p->target_gray / 100.f)) : 0.f;
    a.linbase = b < 0.f ? 0.f : b;
    a.satcontrol = p->satcontrol ? 1 : 0;
    {   // highlight compression (L148-156): the constants with the host's libm like the reference, the per-pixel curve on the device
        a.hlcompr = p->highlight_compression > 0 ? 1 : 0;
        const float hf = float(p->highlight_compression) / 100.f;
        a.hlcompr_factor = hf < 0.f ? 0.f : (hf > 1.f ? 1.f : hf);
        constexpr float compr_l = 1.01f, compr_t = 0.8f;
        a.compr_p = std::max(a.hlcompr_factor, 0.1f);
        a.compr_s = (compr_l - compr_t) / std::pow(std::pow((1.f - compr_t) / (compr_l - compr_t), -a.compr_p) - 1.f, 1.f / a.compr_p);
    }
    { const float bl = float(p->regularization) / 100.f; a.blend = bl < 0.f ? 0.f : (bl > 1.f ? 1.f : bl); }
    for (int k = 0; k < 3; ++k) a.ws1[k] = ws[3 + k];
    DevRGB d;
    int rc = bind_rgb(ctx, img, 4, true, &d, "log_encoding");
    if (rc) return rc;
    for (int k = 0; k < 3; ++k) a.img[k] = d.p[k];
    a.stride = d.stride; a.w = d.w; a.h = d.h;
    if (p->regularization == 0) {
        HIPCHK(ctx, launch_logenc_direct(a, ctx->stream));
    } else {
        const size_t n = (size_t)d.w * d.h;
        float *Y, *Y2;
        if ((rc = pool_get(ctx, P_DMASK, n * 4, &Y)) || (rc = pool_get(ctx, P_CCMAP, n * 4, &Y2))) return rc;
        a.Y = Y; a.Y2 = Y2;
        HIPCHK(ctx, launch_logenc_prepare(a, ctx->stream));
        const int m1 = full_width > d.w ? full_width : d.w, m2 = full_height > d.h ? full_height : d.h;
        const float radius = (m1 > m2 ? m1 : m2) / 30.f;
        artgpu_plane guide = {Y2, d.w, d.h, (int64_t)d.w * 4, 1}, ypl = {Y, d.w, d.h, (int64_t)d.w * 4, 1};
        if ((rc = artgpu_guided_filter(ctx, &guide, &ypl, &ypl, (int)radius, 0.005f, 0))) return rc;
        HIPCHK(ctx, launch_logenc_blend(a, ctx->stream));
    }
    return unbind_rgb(ctx, img, &d);
}

int artgpu_hsl_equalizer(artgpu_ctx *ctx, artgpu_rgb *img, const double *hcurve, int nh, const double *scurve, int ns,
                         const double *lcurve, int nl, int smoothing, const double ws[9], double scale, int to_rgb)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !ws || !(scale >= 1.0)) return fail(ctx, ARTGPU_EINVAL, "hsl_equalizer: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the four polylines: saturation, luminance, hue (periodic, 1000 / scale points) and the fixed coefficient curve of L125-129
    static const double coeff_pts[9] = {1 /* FCT_MinMaxCPoints */, 0.25, 0.0, 0.5, 0.18, 1, 1, 0, 0.35};
    const double *pts[4] = {scurve, lcurve, hcurve, coeff_pts};
    const int npts[4] = {ns, nl, nh, 9};
    std::vector<double> px[4], py[4], ps[4];
    bool active[4];
    const int ppn = (int)(1000 / scale);
    for (int k = 0; k < 4; ++k) active[k] = pts[k] && flat_curve_polyline(pts[k], npts[k], true, k == 3 ? 1000 : ppn, 0.5, px[k], py[k], ps[k]);
    if (!active[3]) return fail(ctx, ARTGPU_EHIP, "hsl_equalizer: internal curve");
    DevRGB d;
    int rc = bind_rgb(ctx, img, 4, true, &d, "hsl_equalizer");
    if (rc) return rc;
    size_t total = 0;
    for (int k = 0; k < 4; ++k) if (active[k]) total += px[k].size() * 2 + ps[k].size();
    float *tabf, *mask;
    if ((rc = pool_get(ctx, P_PIPE_G, total * 8 + 64, &tabf)) || (rc = pool_get(ctx, P_DMASK, (size_t)d.w * d.h * 4, &mask))) return rc;
    std::vector<double> host(total);
    HslArgs a = {};
    {
        size_t off = 0;
        double *dev = reinterpret_cast<double *>(tabf);
        for (int k = 0; k < 4; ++k) {
            if (!active[k]) continue;
            const size_t n = px[k].size();
            std::copy(px[k].begin(), px[k].end(), host.begin() + off); a.curve[k].x = dev + off; off += n;
            std::copy(py[k].begin(), py[k].end(), host.begin() + off); a.curve[k].y = dev + off; off += n;
            std::copy(ps[k].begin(), ps[k].end(), host.begin() + off); a.curve[k].slope = dev + off; off += ps[k].size();
            a.curve[k].n = (int)n;
        }
        HIPCHK(ctx, hipMemcpyAsync(dev, host.data(), total * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    for (int k = 0; k < 3; ++k) { a.img[k] = d.p[k]; a.ws1[k] = (float)ws[3 + k]; }
    a.stride = d.stride; a.w = d.w; a.h = d.h; a.mask = mask; a.to_rgb = to_rgb ? 1 : 0;
    HIPCHK(ctx, launch_hsl_prepare(a, ctx->stream));
    const float sm = smoothing / 10.f;
    const float smooth = std::pow(10.f, sm < 0.f ? 0.f : (sm > 1.f ? 1.f : sm)) - 1.f;            // L93
    const int radius_small = (int)(4 / scale * smooth + 0.5), radius_large = (int)(25 / scale * smooth + 0.5);
    artgpu_plane guide = {d.p[1], d.w, d.h, (int64_t)d.stride * 4, 1};                             // Y
    artgpu_plane mpl = {mask, d.w, d.h, (int64_t)d.w * 4, 1};
    const int order[3] = {0, 1, 2};                 // saturation, luminance, hue: the reference's order
    for (int k : order) {
        if (!active[k]) continue;
        a.which = k;
        HIPCHK(ctx, launch_hsl_mask(a, ctx->stream));
        const int radius = k == 1 ? radius_large : radius_small;
        const float eps = k == 1 ? 0.0001f : 0.001f;
        if (radius > 0 && (rc = artgpu_guided_filter(ctx, &guide, &mpl, &mpl, radius, eps, 0))) return rc;
        HIPCHK(ctx, launch_hsl_apply(a, ctx->stream));
    }
    HIPCHK(ctx, launch_hsl_finish(a, ctx->stream));
    rc = unbind_rgb(ctx, img, &d);
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // host vector with the polylines goes out of scope
    return ARTGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// NEUTRAL tone curve
// ---------------------------------------------------------------------------------------------
} // extern "C"
extern "C" {
int artgpu_tone_curve_neutral(artgpu_ctx *ctx, artgpu_rgb *image, const float *lut65536, float whitecoeff, const artgpu_neutral_state *st)
{
    StageScope scope_(ctx, "ImProcFunctions::toneCurve (NEUTRAL)");
    if (!ctx) return ARTGPU_EINVAL;
    if (!image || !lut65536 || !st || !(whitecoeff > 0.f)) return fail(ctx, ARTGPU_EINVAL, "tone_curve_neutral: null/invalid argument");
    DevRGB d;
    int rc = bind_rgb(ctx, image, 4, true, &d, "tone_curve_neutral");
    if (rc) return rc;
    float *pq;
    if ((rc = pq_tables_dev(ctx, &pq))) return rc;
    if ((rc = upload_curve(ctx, lut65536))) return rc;
    NeutralArgs a = {};
    for (int k = 0; k < 3; ++k) a.img[k] = d.p[k];
    a.stride = d.stride; a.w = d.w; a.h = d.h;
    a.lut = ctx->lut; a.pq = pq; a.pq_inv = pq + 65536; a.hues = pq + 2 * 65536;
    for (int k = 0; k < 9; ++k) { a.ws[k] = (float)st->ws[k]; a.iws[k] = (float)st->iws[k]; a.to_out[k] = st->to_out[k]; a.to_work[k] = st->to_work[k]; }
    a.whitecoeff = whitecoeff;
    a.tail_kind = ctx->shared.curve_tail_kind == ARTGPU_CURVE_TAIL_HOST ? 0 : ctx->shared.curve_tail_kind; a.tail_y = ctx->shared.curve_tail_y; a.tail_pc = ctx->shared.curve_tail_pc;
    a.no_lds_lut = !ctx->shared.opt_lut_lds; a.cu_reserve = cu_reserve_of(ctx);
    HIPCHK(ctx, launch_tone_neutral(a, ctx->stream));
    return unbind_rgb(ctx, image, &d);
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

// fills P_CCMAP ((w+1)/2 x (h+1)/2, contiguous) from device planes, or, with `gi` on, from the demosaiced planes getImage would have read
static int chroma_map_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int w, int h, const double *mat, const double ws[9],
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
    int rc = bind_rgb(ctx, planes, 1, true, &src, "denoise_compute_params(planes)");
    if (rc) return rc;
    if (border < 0) return fail(ctx, ARTGPU_EINVAL, "denoise_compute_params: border %d", border);
    const int widIm = src.w - 2 * border, heiIm = src.h - 2 * border;       // getFullSize
    const int crW = widIm / 2, crH = heiIm / 2;                              // Tile_calc returns one tile: tileWskip = widIm (L836,875-876)
    if (widIm < 100 || heiIm < 100)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "denoise_compute_params: %dx%d is too small for the nine-crop layout (crops start 50 px in)", widIm, heiIm);
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

int artgpu_ordered_sum_f32(artgpu_ctx *ctx, const float *x, int64_t n, int on_device, float *result)
{
    if (!ctx) return ARTGPU_EINVAL;
    if ((!x && n > 0) || n < 0 || !result) return fail(ctx, ARTGPU_EINVAL, "ordered_sum_f32: bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    float *res, *dev = nullptr;
    int rc = pool_get(ctx, P_DNINFO, (9 * 32 + 9 * 8) * 4, &res);
    if (rc) return rc;
    const float *src = x;
    if (!on_device && n > 0) {
        if ((rc = pool_get(ctx, P_TMP, (size_t)n * 4, &dev))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(dev, x, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        src = dev;
    }
    HIPCHK(ctx, launch_ordered_sum(src, (long long)n, res, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(result, res, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ARTGPU_OK;
}

int artgpu_eval_primitive(artgpu_ctx *ctx, int prim, const void *a, const void *b, const void *c, void *out0, void *out1, int64_t n,
                          float param, const float *table, int table_size)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (prim < 0 || prim >= PRIM_COUNT || n < 0 || (n > 0 && (!a || !out0))) return fail(ctx, ARTGPU_EINVAL, "eval_primitive: bad argument");
    const bool dbl = prim == PRIM_XLOG_D || prim == PRIM_XEXP_D;
    const bool need_b = prim == PRIM_POW_F || prim == PRIM_XATAN2F || prim == PRIM_MEDIAN3 || prim == PRIM_VMINF || prim == PRIM_VMAXF || prim == PRIM_VINTPF;
    const bool need_c = prim == PRIM_MEDIAN3 || prim == PRIM_VINTPF;
    const bool lut = prim == PRIM_LUTF_SCALAR || prim == PRIM_LUTF_VECTOR;
    if ((need_b && !b) || (need_c && !c) || (prim == PRIM_XSINCOSF && !out1) || (lut && (!table || table_size < 2)))
        return fail(ctx, ARTGPU_EINVAL, "eval_primitive: primitive %d lacks an operand", prim);
    if (n == 0) return ARTGPU_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t esz = dbl ? 8 : 4, bytes = (size_t)n * esz, tbytes = lut ? (size_t)table_size * 4 : 0;
    float *buf;
    int rc = pool_get(ctx, P_TMP, 5 * bytes + tbytes + 64, &buf);
    if (rc) return rc;
    char *base = reinterpret_cast<char *>(buf);
    PrimArgs p{};
    p.prim = prim; p.n = n; p.param = param; p.table_size = table_size;
    p.a = base; p.b = base + bytes; p.c = base + 2 * bytes; p.out0 = base + 3 * bytes; p.out1 = base + 4 * bytes;
    p.table = reinterpret_cast<const float *>(base + 5 * bytes);
    HIPCHK(ctx, hipMemcpyAsync(base, a, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (need_b) HIPCHK(ctx, hipMemcpyAsync(base + bytes, b, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (need_c) HIPCHK(ctx, hipMemcpyAsync(base + 2 * bytes, c, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (lut) HIPCHK(ctx, hipMemcpyAsync(base + 5 * bytes, table, tbytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, launch_prim_eval(p, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(out0, p.out0, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (prim == PRIM_XSINCOSF) HIPCHK(ctx, hipMemcpyAsync(out1, p.out1, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ARTGPU_OK;
}

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

// useNoiseCCurve (FTblockDN.cc:1672): the chroma noise curve counts when NoiseCurve::getSum (ipdenoise.cc:698) of its 501 entries is above 5
static bool noise_curve_on(const float *curve)
{
    if (!curve) return false;
    float sum = 0.f;
    for (int i = 0; i < 501; ++i) sum += curve[i];
    return sum > 5.f;
}

// ImProcFunctions::denoise on device planes; `fu0`: what artgpu_improc_denoise_fused has decided to fuse of the stages around the tool (the
// tool's own expcomp passes and `ccalc_nonneg` are decided here)
static int improc_denoise_dev(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_denoise_tool_params *p, const double ws[9], const double *iws,
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
        float *pl[3] = {img->r.p, img->g.p, img->b.p}, *map;
        if (img->g.row_stride_bytes != img->r.row_stride_bytes || img->b.row_stride_bytes != img->r.row_stride_bytes)
            return fail(ctx, ARTGPU_EINVAL, "improc_denoise: planes must share one row stride");
        if ((rc = chroma_map_dev(ctx, pl, (size_t)(img->r.row_stride_bytes / 4), img->r.w, img->r.h, calclum_mat, ws, noise_c_curve, fu0.gi, &map))) return rc;
        ccalc.p = map; ccalc.w = (img->r.w + 1) / 2; ccalc.h = (img->r.h + 1) / 2; ccalc.row_stride_bytes = (int64_t)ccalc.w * 4; ccalc.on_device = 1;
        ccalc_p = &ccalc;
    }
    // expcomp(+ecomp) / expcomp(-ecomp) (ipdenoise.cc:1161-1163,1181-1184) are fused into RGB_denoise's first and last pixel
    // passes when RGB_denoise will actually run them (same operations on the same values, two fewer passes over the image).
    // (Whether it runs is asked of the ADJUSTED strengths here and of the caller's in artgpu_improc_denoise_fused: both are kept, see there.)
    const bool dn_runs = !(p->dn.luminance == 0 && p->dn.chrominance == 0 && !ccalc_p);
    const bool fuse_pre = ecomp > 0 && dn_runs, fuse_post = fuse_pre && !p->smoothing_enabled;
    if (ecomp > 0 && !fuse_pre) { if ((rc = artgpu_exposure(ctx, img, (float)std::pow(2.0, ecomp), 0.f))) return rc; }
    DnFusion fu = fu0;
    fu.pre_scale = fuse_pre ? (float)std::pow(2.0, ecomp) : 0.f;
    fu.post_scale = fuse_post ? (float)std::pow(2.0, -ecomp) : 0.f;
    fu.ccalc_nonneg = ccalc_p ? 1 : 0;
    float iwsf[9];
    if (iws) for (int k = 0; k < 9; ++k) iwsf[k] = (float)iws[k];
    {
        StageScope scope_(ctx, "denoise::RGB_denoise");
        if ((rc = rgb_denoise_args_ok(ctx, &p->dn, iws ? iwsf : nullptr, scale))) return rc;
        HIPCHK(ctx, hipSetDevice(ctx->device));
        DevRGB d;
        if ((rc = bind_rgb(ctx, img, 4, true, &d, "rgb_denoise"))) return rc;       // (device planes: nothing is staged)
        if ((rc = rgb_denoise_dev(ctx, d, &p->dn, wsf, iws ? iwsf : nullptr, 0.0, scale, ccalc_p, flags, nullptr, nullptr, fu))) return rc;
    }
    // the exposure steps behind the tool's last stage -- its own expcomp(-ecomp) (L1181-1184) where yuv2rgb could not take it, and the STAGE_1
    // exposure of artgpu_improc_denoise_fused -- ride on the last pixel pass there is: setMode(RGB) behind NL-means, or one exposure pass
    int chain_n = 0;
    float chain_scale[2], chain_black[2];
    if (ecomp > 0 && !fuse_post) { chain_scale[chain_n] = (float)std::pow(2.0, -ecomp); chain_black[chain_n] = 0.f; ++chain_n; }
    if (fu.tail_on) { chain_scale[chain_n] = fu.tail_scale; chain_black[chain_n] = fu.tail_black; ++chain_n; }
    bool chained = false;
    if (p->smoothing_enabled) {
        if ((rc = artgpu_denoise_guided_smoothing(ctx, img, ws, p->guided_chroma_radius, scale))) return rc;
        if (p->nl_strength) {
            PixArgs a = {};
            float *pl[3] = {img->r.p, img->g.p, img->b.p};
            for (int k = 0; k < 3; ++k) { a.dst[k] = pl[k]; a.mul[k] = wsf[3 + k]; }
            a.dst_stride = (size_t)(img->r.row_stride_bytes / 4); a.w = img->r.w; a.h = img->r.h;
            a.do_clip = 0;
            HIPCHK(ctx, launch_yuv_mode(a, ctx->stream));
            if ((rc = artgpu_nlmeans(ctx, &img->g, 65535.f, p->nl_strength, p->nl_detail, (float)scale))) return rc;
            a.do_clip = 1;
            a.chain_n = chain_n;
            for (int k = 0; k < chain_n; ++k) { a.chain_scale[k] = chain_scale[k]; a.chain_black[k] = chain_black[k]; }
            HIPCHK(ctx, launch_yuv_mode(a, ctx->stream));
            chained = true;
        }
    }
    if (chain_n && !chained) {
        PixArgs a = {};
        float *pl[3] = {img->r.p, img->g.p, img->b.p};
        for (int k = 0; k < 3; ++k) a.dst[k] = pl[k];
        a.dst_stride = (size_t)(img->r.row_stride_bytes / 4); a.w = img->r.w; a.h = img->r.h;
        a.exp_scale = chain_scale[0]; a.black = chain_black[0];
        a.chain_n = chain_n - 1;
        if (chain_n > 1) { a.chain_scale[0] = chain_scale[1]; a.chain_black[0] = chain_black[1]; }
        HIPCHK(ctx, launch_exposure(a, ctx->stream));
    }
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
    // what of the neighbouring stages can really live inside the tool's pixel passes: the wavelet denoise has to run (its first pass reads the
    // image, its last one writes it), on device planes; the exposure only when nothing stands between RGB_denoise and it.
    // `dn_runs0` asks the caller's strengths, improc_denoise_dev's `dn_runs` the ones adjust_params has scaled.  adjust_params maps 0 to 0 and
    // any other strength to another one of the same sign, so the two agree for every strength and scale a caller can mean; they part only
    // where the arithmetic underflows (a denormal strength, an infinite scale).  Both are kept as they were.
    const bool dn_runs0 = !(p->dn.luminance == 0 && p->dn.chrominance == 0 && !noise_curve_on(noise_c_curve));
    const bool dev_planes = img->r.on_device && (!fu || !fu->demosaiced || (fu->demosaiced->r.on_device && fu->demosaiced->g.on_device && fu->demosaiced->b.on_device));
    const bool fuse_gi = fu && fu->demosaiced && dn_runs0 && dev_planes;
    const bool fuse_exp = fu && fu->exposure_enabled && dn_runs0 && dev_planes && !p->smoothing_enabled;
    // with guided smoothing / NL-means behind the wavelet denoise the tool's last pixel pass is setMode(RGB) or its own expcomp(-ecomp):
    // the exposure rides on that one
    const bool tail_exp = fu && fu->exposure_enabled && dn_runs0 && dev_planes && p->smoothing_enabled && (p->nl_strength || ecomp > 0);
    int rc;
    DnFusion f = {};
    if (fu && fu->demosaiced) {
        const artgpu_rgb *dm = fu->demosaiced;
        if (!plane_ok(&dm->r) || !plane_ok(&dm->g) || !plane_ok(&dm->b) || dm->g.row_stride_bytes != dm->r.row_stride_bytes || dm->b.row_stride_bytes != dm->r.row_stride_bytes ||
            fu->sx1 < 0 || fu->sy1 < 0 || fu->sx1 + img->r.w > dm->r.w || fu->sy1 + img->r.h > dm->r.h)
            return fail(ctx, ARTGPU_EINVAL, "improc_denoise_fused: crop %dx%d+%d+%d outside the demosaiced planes", img->r.w, img->r.h, fu->sx1, fu->sy1);
        if (fuse_gi) {
            GetImageFuse &g = f.gi;
            g.on = 1;
            g.src[0] = dm->r.p; g.src[1] = dm->g.p; g.src[2] = dm->b.p;
            g.stride = (size_t)(dm->r.row_stride_bytes / 4);
            g.sx1 = fu->sx1; g.sy1 = fu->sy1;
            for (int k = 0; k < 3; ++k) g.mul[k] = fu->mul[k];
            g.do_clip = fu->do_clip ? 1 : 0; g.has_mat = fu->cam_to_work ? 1 : 0;
            for (int k = 0; k < 9; ++k) g.mat[k] = fu->cam_to_work ? fu->cam_to_work[k] : 0.0;
        } else if ((rc = artgpu_get_image(ctx, dm, fu->sx1, fu->sy1, fu->mul, fu->do_clip, fu->cam_to_work, img))) {     // the separate call it stands for
            return rc;
        }
    }
    if (fuse_exp) { f.exp_on = 1; f.exp_scale = fu->exp_scale; f.exp_black = fu->black; }
    if (tail_exp) { f.tail_on = 1; f.tail_scale = fu->exp_scale; f.tail_black = fu->black; }
    // host planes: stage once, run the whole tool on the staged copy, copy back (device planes are used in place)
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "improc_denoise"))) return rc;
    artgpu_rgb dv = mk_dev_rgb(d.p, d.w, d.h, d.stride);
    if ((rc = improc_denoise_dev(ctx, &dv, p, ws, iws, ecomp, scale, calclum_mat, noise_c_curve, flags, f))) return rc;
    // the exposure that could not be fused follows as its own call
    if (fu && fu->exposure_enabled && !fuse_exp && !tail_exp && (rc = artgpu_exposure(ctx, &dv, fu->exp_scale, fu->black))) return rc;
    return unbind_rgb(ctx, img, &d);
}

// ---------------------------------------------------------------------------------------------
// N4: channel mixer, RGB curves
// ---------------------------------------------------------------------------------------------
int artgpu_channel_mixer(artgpu_ctx *ctx, artgpu_rgb *image, const float m[9])
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!image || !m) return fail(ctx, ARTGPU_EINVAL, "channel_mixer: null argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    int rc = bind_rgb(ctx, image, 4, true, &d, "channel_mixer");
    if (rc) return rc;
    MixArgs a = {};
    for (int k = 0; k < 3; ++k) a.dst[k] = d.p[k];
    a.stride = d.stride; a.w = d.w; a.h = d.h;
    for (int k = 0; k < 9; ++k) a.m[k] = m[k];
    HIPCHK(ctx, launch_channel_mixer(a, ctx->stream));
    return unbind_rgb(ctx, image, &d);
}

int artgpu_rgb2out_matrix(artgpu_ctx *ctx, const artgpu_rgb *src, artgpu_rgb *dst, const float matrix[9], int trc_linear,
                          const float *lut, int lutsz)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!src || !dst || !matrix) return fail(ctx, ARTGPU_EINVAL, "rgb2out_matrix: null argument");
    if (!trc_linear && (!lut || lutsz < 2)) return fail(ctx, ARTGPU_EINVAL, "rgb2out_matrix: a non-linear TRC needs its LUT");
    if (lut && (lutsz < 2 || lutsz > 65536)) return fail(ctx, ARTGPU_EINVAL, "rgb2out_matrix: lutsz %d", lutsz);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB s, d;
    int rc = bind_rgb(ctx, src, 1, true, &s, "rgb2out_matrix(src)");
    if (rc) return rc;
    if ((rc = bind_rgb(ctx, dst, 4, false, &d, "rgb2out_matrix(dst)"))) return rc;
    if (s.w != d.w || s.h != d.h) return fail(ctx, ARTGPU_EINVAL, "rgb2out_matrix: size mismatch");
    float *tab;
    if ((rc = pool_get(ctx, P_PIPE_R, (65536 + 16) * 4, &tab))) return rc;
    OutArgs a = {};
    for (int k = 0; k < 3; ++k) { a.src[k] = s.p[k]; a.dst[k] = d.p[k]; }
    a.src_stride = s.stride; a.dst_stride = d.stride; a.w = s.w; a.h = s.h;
    for (int k = 0; k < 9; ++k) a.m[k] = matrix[k];
    a.linear = trc_linear ? 1 : 0;
    a.unsupported = reinterpret_cast<int *>(tab + 65536);
    HIPCHK(ctx, hipMemsetAsync(a.unsupported, 0, 4, ctx->stream));
    if (lut) {
        if ((rc = h2d_table(ctx, tab, lut, (size_t)lutsz * 4))) return rc;
        a.lut = tab; a.lutsz = lutsz;
    }
    HIPCHK(ctx, launch_rgb2out_matrix(a, ctx->stream));
    int bad = 0;
    HIPCHK(ctx, hipMemcpyAsync(&bad, a.unsupported, 4, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = unbind_rgb(ctx, dst, &d))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (bad) return fail(ctx, ARTGPU_EUNSUPPORTED, "rgb2out_matrix: %d channel values above 1 need ARTOutputProfile::eval (lcms2/libm) on the host", bad);
    return ARTGPU_OK;
}

int artgpu_get_scanlines(artgpu_ctx *ctx, const artgpu_rgb *img, int bps, int is_float, void *dst, int64_t dst_row_stride_bytes, int dst_on_device)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !dst) return fail(ctx, ARTGPU_EINVAL, "get_scanlines: null argument");
    const bool okfmt = is_float ? (bps == 16 || bps == 32) : (bps == 8 || bps == 16);
    if (!okfmt) return fail(ctx, ARTGPU_EINVAL, "get_scanlines: bps %d / is_float %d", bps, is_float);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB s;
    int rc = bind_rgb(ctx, img, 4, true, &s, "get_scanlines");
    if (rc) return rc;
    const size_t rowb = (size_t)s.w * 3 * (bps / 8);
    if (dst_row_stride_bytes < (int64_t)rowb) return fail(ctx, ARTGPU_EINVAL, "get_scanlines: row stride %lld < %zu", (long long)dst_row_stride_bytes, rowb);
    OutArgs a = {};
    for (int k = 0; k < 3; ++k) a.src[k] = s.p[k];
    a.src_stride = s.stride; a.w = s.w; a.h = s.h; a.bps = bps; a.is_float = is_float ? 1 : 0;
    float *stage = nullptr;
    if (dst_on_device) { a.out = static_cast<unsigned char *>(dst); a.out_stride_bytes = (size_t)dst_row_stride_bytes; }
    else {
        if ((rc = pool_get(ctx, P_TMP, rowb * s.h + 16, &stage))) return rc;
        a.out = reinterpret_cast<unsigned char *>(stage); a.out_stride_bytes = rowb;
    }
    HIPCHK(ctx, launch_scanlines(a, ctx->stream));
    if (!dst_on_device) {
        HIPCHK(ctx, hipMemcpy2DAsync(dst, (size_t)dst_row_stride_bytes, stage, rowb, rowb, s.h, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return ARTGPU_OK;
}

int artgpu_saturation_vibrance(artgpu_ctx *ctx, artgpu_rgb *image, int saturation, int vibrance, const double ws[9])
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!image || !ws) return fail(ctx, ARTGPU_EINVAL, "saturation_vibrance: null argument");
    if (!saturation && !vibrance) return ARTGPU_OK;            // ipsaturation.cc:45-46
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    int rc = bind_rgb(ctx, image, 4, true, &d, "saturation_vibrance");
    if (rc) return rc;
    SatArgs a = {};
    for (int k = 0; k < 3; ++k) { a.dst[k] = d.p[k]; a.ws1[k] = ws[3 + k]; }
    a.stride = d.stride; a.w = d.w; a.h = d.h;
    a.saturation = 1.f + saturation / 100.f;
    a.vibrance = 1.f - vibrance / 1000.f;
    a.vib = vibrance ? 1 : 0;
    HIPCHK(ctx, launch_saturation_vibrance(a, ctx->stream));
    return unbind_rgb(ctx, image, &d);
}

int artgpu_rgb_curves(artgpu_ctx *ctx, artgpu_rgb *image, const float *rcurve, const float *gcurve, const float *bcurve)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!image) return fail(ctx, ARTGPU_EINVAL, "rgb_curves: null argument");
    if (!rcurve && !gcurve && !bcurve) return ARTGPU_OK;    // all identity: the reference skips the loop (iprgbcurves.cc:110)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    int rc = bind_rgb(ctx, image, 4, true, &d, "rgb_curves");
    if (rc) return rc;
    // The tables live in a pool slot of their own: the host-side cache below describes what the slot holds, so nothing else may write it
    // (P_PIPE_R, where they used to be, is also labAdjustments' curves, rgb2out's TRC table and the pipeline's red plane).
    float *tabs;
    if (ctx->pool_bytes[P_RGBCURVES] < (size_t)3 * 65536 * 4)
        for (int k = 0; k < 3; ++k) ctx->rgbcurve_host[k].clear();           // a fresh allocation holds nothing
    if ((rc = pool_get(ctx, P_RGBCURVES, 3 * 65536 * 4, &tabs))) return rc;
    const float *host[3] = {rcurve, gcurve, bcurve};
    MixArgs a = {};
    for (int k = 0; k < 3; ++k) {
        a.dst[k] = d.p[k];
        if (host[k]) {
            // one rule for every look-up table that crosses the boundary (artgpu.h "Host look-up tables"): the call keeps its own copy and
            // the caller's array is free when the call returns; the same table call after call is uploaded once
            std::vector<float> &own = ctx->rgbcurve_host[k];
            if (own.size() != 65536 || std::memcmp(own.data(), host[k], 65536 * 4) != 0) {
                own.assign(host[k], host[k] + 65536);
                hipError_t e = hipMemcpyAsync(tabs + (size_t)k * 65536, own.data(), 65536 * 4, hipMemcpyHostToDevice, ctx->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
                if (e != hipSuccess) { own.clear(); return fail(ctx, ARTGPU_EHIP, "rgb_curves: curve upload failed: %s", hipGetErrorString(e)); }
            }
            a.lut[k] = tabs + (size_t)k * 65536;
        }
    }
    a.stride = d.stride; a.w = d.w; a.h = d.h;
    HIPCHK(ctx, launch_rgb_curves(a, ctx->stream));
    rc = unbind_rgb(ctx, image, &d);
    if (rc) return rc;
    return ARTGPU_OK;      // (host LUT lifetime: see "Host look-up tables" in artgpu.h)
}

// ---------------------------------------------------------------------------------------------
// raw pre-stage (N2): copyOriginalPixels + scaleColors
// ---------------------------------------------------------------------------------------------
int artgpu_scale_colors(artgpu_ctx *ctx, const void *src, int32_t w, int32_t h, int64_t src_row_stride_bytes, int32_t src_is_u16,
                        int32_t src_on_device, uint32_t filters, const int32_t *xtrans, const float cblacksom[4],
                        const float scale_mul[4], artgpu_plane *dst, float chmax[4])
{
    if (!ctx) return ARTGPU_EINVAL;
    const int esz = src_is_u16 ? 2 : 4;
    if (!src || !dst || !plane_ok(dst) || !cblacksom || !scale_mul || w <= 0 || h <= 0 || dst->w != w || dst->h != h ||
        src_row_stride_bytes < (int64_t)w * esz || src_row_stride_bytes % esz)
        return fail(ctx, ARTGPU_EINVAL, "scale_colors: bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    ScaleArgs a = {};
    a.w = w; a.h = h; a.src_u16 = src_is_u16 ? 1 : 0;
    // source: device pointer as is, host buffer staged (2 or 4 bytes per pixel over PCIe)
    if (src_on_device) { a.src = src; a.src_stride = (size_t)(src_row_stride_bytes / esz); }
    else {
        float *st;
        if ((rc = pool_get(ctx, P_PIPE_B, (size_t)w * h * esz, &st))) return rc;
        HIPCHK(ctx, hipMemcpy2DAsync(st, (size_t)w * esz, src, (size_t)src_row_stride_bytes, (size_t)w * esz, h, hipMemcpyHostToDevice, ctx->stream));
        a.src = st; a.src_stride = w;
    }
    float *out;
    if (dst->on_device) { out = dst->p; a.dst_stride = (size_t)(dst->row_stride_bytes / 4); }
    else { if ((rc = pool_get(ctx, P_PIPE_G, (size_t)w * h * 4, &out))) return rc; a.dst_stride = w; }
    a.dst = out;
    a.bayer = xtrans ? 0 : 1;
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) {
            int v;
            if (xtrans) v = xtrans[r * 6 + c];
            else v = (filters >> ((((r << 1) & 14) + (c & 1)) << 1)) & 3;      // RawImage::FC, period 2 tiles the 6x6 map
            if (v < 0 || v > 2) return fail(ctx, ARTGPU_EUNSUPPORTED, "scale_colors: three-colour CFAs only");
            a.cfa[r * 6 + c] = v;
        }
    for (int k = 0; k < 4; ++k) { a.cblacksom[k] = cblacksom[k]; a.scale_mul[k] = scale_mul[k]; }
    float *mx;
    if ((rc = pool_get(ctx, P_MAD, 3 * 32 * 4, &mx))) return rc;
    a.chmax_bits = reinterpret_cast<int *>(mx);
    HIPCHK(ctx, hipMemsetAsync(mx, 0, 4 * sizeof(int), ctx->stream));
    HIPCHK(ctx, launch_scale_colors(a, ctx->stream));
    if (!dst->on_device)
        HIPCHK(ctx, hipMemcpy2DAsync(dst->p, (size_t)dst->row_stride_bytes, out, (size_t)w * 4, (size_t)w * 4, h, hipMemcpyDeviceToHost, ctx->stream));
    if (chmax) {
        float host[4];
        HIPCHK(ctx, hipMemcpyAsync(host, mx, 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        chmax[0] = host[0]; chmax[1] = host[1]; chmax[2] = host[2]; chmax[3] = host[1];
    } else if (!dst->on_device) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return ARTGPU_OK;
}

} // extern "C"

namespace artgpu { namespace api {

// Bayer 2x2 colour map of `filters` for the CA correction: FC packed as CaArgs::cfa; false for X-Trans, a fourth colour or a
// pattern without one green per row and column
bool ca_cfa(uint32_t filters, unsigned *cfa)
{
    if (filters == 9) return false;
    unsigned f[2][2], packed = 0;
    for (int r = 0; r < 2; ++r)
        for (int c = 0; c < 2; ++c) {
            f[r][c] = (filters >> ((((r << 1) & 14) + (c & 1)) << 1)) & 3;
            if (f[r][c] == 3) return false;
            packed |= f[r][c] << ((r * 2 + c) * 2);
        }
    for (int k = 0; k < 2; ++k)
        if ((f[k][0] == 1) == (f[k][1] == 1) || (f[0][k] == 1) == (f[1][k] == 1)) return false;
    *cfa = packed;
    return true;
}

// CA_correct_RT on a contiguous-or-strided device CFA plane, enqueued on ctx->stream (no synchronisation unless fit_out)
int ca_correct_dev(artgpu_ctx *ctx, float *raw, size_t stride, int W, int H, unsigned cfa, const artgpu_ca_params *p, double *fit_out)
{
    constexpr int ts = 128, border2 = 16, cb = 2;
    CaArgs a = {};
    a.raw = raw; a.stride = stride; a.W = W; a.H = H; a.width = W + (W & 1); a.cfa = cfa;
    const int vz1 = (H + border2) % (ts - border2) == 0 ? 1 : 0;
    const int hz1 = (a.width + border2) % (ts - border2) == 0 ? 1 : 0;
    a.vblsz = (int)ceil((float)(H + border2) / (ts - border2) + 2 + vz1);
    a.hblsz = (int)ceil((float)(a.width + border2) / (ts - border2) + 2 + hz1);
    a.ntv = (H + 8 + (ts - border2) - 1) / (ts - border2);
    a.nth = (W + 8 + (ts - border2) - 1) / (ts - border2);
    a.fw = (W + 1 - 2 * cb) / 2; a.fh = (H + 1 - 2 * cb) / 2;
    a.autoCA = p->autocorrect ? 1 : 0;
    a.cared = p->red; a.cablue = p->blue;
    const int iterations = a.autoCA ? (p->iterations > 1 ? p->iterations : 1) : 1;
    const bool guard = p->avoid_colour_shift != 0;
    const size_t half = (size_t)H * a.width / 2, nb = (size_t)a.vblsz * a.hblsz, ninner = (size_t)(a.vblsz - 2) * (a.hblsz - 2);
    const size_t fplane = (size_t)a.fw * a.fh;
    float *halfp, *blk, *grd = nullptr;
    int rc;
    if ((rc = pool_get(ctx, P_CA_HALF, 2 * half * 4, &halfp)) || (rc = pool_get(ctx, P_CA_BLK, (144 + nb * 5 + ninner * 8 + 4) * 4, &blk)))
        return rc;
    if (guard && (rc = pool_get(ctx, P_CA_GUARD, ((size_t)a.fw * (H - 2 * cb) + 3 * fplane) * 4, &grd))) return rc;
    a.Gtmp = halfp; a.RawDataTmp = halfp + half;
    a.fit = reinterpret_cast<double *>(blk);                       // 64 doubles first: 8-byte aligned
    a.words = reinterpret_cast<int *>(blk + 128);
    a.blockwt = blk + 144; a.blockshifts = a.blockwt + ((nb + 3) & ~(size_t)3); a.blockfit = a.blockshifts + 4 * nb;
    if (guard) { a.oldraw = grd; a.red = grd + (size_t)a.fw * (H - 2 * cb); a.blue = a.red + fplane; }
    // the reference zeroes blockwt / blockshifts once per call (L208); Gtmp (never written in manual mode) and fitparams (only
    // partly written by a linear fit) are zeroed here so that every value the device reads is defined
    HIPCHK(ctx, hipMemsetAsync(halfp, 0, half * 4, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(blk, 0, (144 + ((nb + 3) & ~(size_t)3) + 4 * nb) * 4, ctx->stream));
    HIPCHK(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a.words), 1, 2, ctx->stream));       // run, processpasstwo
    HIPCHK(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a.words + 2), 4, 1, ctx->stream));   // polyord
    if (guard) HIPCHK(ctx, launch_ca_capture(a, ctx->stream));
    for (int it = 0; it < iterations; ++it) {
        HIPCHK(ctx, launch_ca_iteration(a, ctx->stream));
        if (guard) {
            HIPCHK(ctx, launch_ca_factors(a, ctx->stream));
            if ((rc = gaussian_dev(ctx, a.red, a.blue + fplane, a.fw, a.fh, 30.0)) || (rc = gaussian_dev(ctx, a.blue, a.blue + fplane, a.fw, a.fh, 30.0)))
                return rc;
            HIPCHK(ctx, launch_ca_apply(a, ctx->stream));
        }
        HIPCHK(ctx, launch_ca_step(a, ctx->stream));
    }
    if (fit_out) {
        HIPCHK(ctx, hipMemcpyAsync(fit_out, a.fit, 64 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_raw_ca_correct(artgpu_ctx *ctx, artgpu_plane *raw, uint32_t filters, const artgpu_ca_params *p, double fit_out[64])
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(raw) || !p) return fail(ctx, ARTGPU_EINVAL, "raw_ca_correct: bad argument");
    unsigned cfa;
    if (!ca_cfa(filters, &cfa)) return fail(ctx, ARTGPU_EUNSUPPORTED, "raw_ca_correct: RGB Bayer patterns only (filters 0x%08x)", filters);
    if (raw->w < 64 || raw->h < 64) return fail(ctx, ARTGPU_EUNSUPPORTED, "raw_ca_correct: frame smaller than 64x64");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    if (raw->on_device) return ca_correct_dev(ctx, raw->p, (size_t)(raw->row_stride_bytes / 4), raw->w, raw->h, cfa, p, fit_out);
    float *work;
    if ((rc = pool_get(ctx, P_CA_RAW, (size_t)raw->w * raw->h * 4, &work))) return rc;
    HIPCHK(ctx, hipMemcpy2DAsync(work, (size_t)raw->w * 4, raw->p, (size_t)raw->row_stride_bytes, (size_t)raw->w * 4, raw->h, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = ca_correct_dev(ctx, work, raw->w, raw->w, raw->h, cfa, p, fit_out))) return rc;
    return pool_to_plane(ctx, work, raw);
}

} // extern "C"

// ---------------------------------------------------------------------------------------------
// ImProcFunctions::localContrast
// ---------------------------------------------------------------------------------------------

extern "C" {

int artgpu_local_contrast_curve_lut(const double *points, int npoints, float lut[501], int *is_set)
{
    if (!lut || !is_set || npoints < 0 || (npoints > 0 && !points)) return ARTGPU_EINVAL;
    *is_set = lc_curve_lut(points, npoints, lut) ? 1 : 0;
    return ARTGPU_OK;
}

} // extern "C"

namespace artgpu { namespace api {

// what the call cannot do, before anything is touched: 0, or the code with the message set
int local_contrast_check(artgpu_ctx *ctx, int w, int h, const artgpu_local_contrast_region *regions, int nregions, double scale, const char *who)
{
    if (nregions < 0 || (nregions > 0 && !regions)) return fail(ctx, ARTGPU_EINVAL, "%s: bad region list", who);
    for (int r = 0; r < nregions; ++r) {
        const artgpu_plane *m = regions[r].mask;
        if (m && (!plane_ok(m) || m->w != w || m->h != h)) return fail(ctx, ARTGPU_EINVAL, "%s: the mask of region %d must be a %dx%d plane", who, r, w, h);
    }
    if (scale != 1.0) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: scale %g (the skip form of the wavelet is not on the device path)", who, scale);
    if (w < ARTGPU_LOCAL_CONTRAST_MIN_SIZE || h < ARTGPU_LOCAL_CONTRAST_MIN_SIZE)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: %dx%d is below %dx%d", who, w, h, ARTGPU_LOCAL_CONTRAST_MIN_SIZE, ARTGPU_LOCAL_CONTRAST_MIN_SIZE);
    const int nl = lc_wavelet_levels(w, h), w2 = (w + 1) / 2, h2 = (h + 1) / 2;
    if ((w2 < h2 ? w2 : h2) < 2 * wavelet_skip(nl - 1))       // the wavelet kernels' own limit: never reached by the level rule from 8x8 up
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: %dx%d too small for %d wavelet levels on the device path", who, w, h, nl);
    return ARTGPU_OK;
}

// the regions of ImProcFunctions::localContrast (L463-481) on a device L plane (rows of `stride` floats), enqueued on ctx->stream; per
// region the host waits once, for the statistics block it computes the constants of L372-380 from
int local_contrast_dev(artgpu_ctx *ctx, float *L, size_t stride, int w, int h, const artgpu_local_contrast_region *regions, int nregions,
                              artgpu_local_contrast_info *info)
{
    DevDecomp d = {};
    d.w = w; d.h = h; d.w2 = (w + 1) / 2; d.h2 = (h + 1) / 2; d.nlevels = lc_wavelet_levels(w, h);
    d.n = (size_t)d.w2 * d.h2;
    if (d.n > 0x7fffffff) return fail(ctx, ARTGPU_EUNSUPPORTED, "local_contrast: band larger than an int holds (the reference's W_L * H_L is an int)");
    const int nbands = 3 * d.nlevels, nchunk = (int)((d.n + LC_CHUNK - 1) / LC_CHUNK);
    // statistics block: results | curve | partial sums | counts | maxima | minima
    const size_t res_bytes = 32 * sizeof(LcSegStats), curve_bytes = 512 * 4, np = (size_t)(nbands + 1) * nchunk;
    float *Lnew, *stats;
    int rc;
    if ((rc = pool_get(ctx, P_LC_BANDS, (size_t)nbands * d.n * 4, &d.bands)) || (rc = pool_get(ctx, P_LC_LOW0, d.n * 4, &d.low[0])) ||
        (rc = pool_get(ctx, P_LC_LOW1, d.n * 4, &d.low[1])) || (rc = pool_get(ctx, P_LC_NEW, (size_t)w * h * 4, &Lnew)) ||
        (rc = pool_get(ctx, P_LC_STATS, res_bytes + curve_bytes + np * (8 + 4 + 4 + 4), &stats)))
        return rc;
    char *sb = reinterpret_cast<char *>(stats);
    LcStatArgs sa = {};
    sa.bands = d.bands; sa.n = d.n; sa.nbands = nbands; sa.nchunk = nchunk;
    sa.res = reinterpret_cast<LcSegStats *>(sb);
    float *curve_dev = reinterpret_cast<float *>(sb + res_bytes);
    sa.psum = reinterpret_cast<double *>(sb + res_bytes + curve_bytes);
    sa.pcnt = reinterpret_cast<int *>(sa.psum + np);
    sa.pmax = reinterpret_cast<float *>(sa.pcnt + np);
    sa.pmin = sa.pmax + np;
    for (int r = 0; r < nregions; ++r) {
        const artgpu_local_contrast_region &reg = regions[r];
        const bool contrast_on = (float)reg.contrast != 0;
        if ((rc = decompose_dev(ctx, d, L, nullptr, stride))) return rc;
        if (reg.curve && (rc = h2d_table(ctx, curve_dev, reg.curve, 501 * 4))) return rc;
        sa.coeff0 = contrast_on ? d.low[d.cur] : nullptr;
        HIPCHK(ctx, launch_lc_stats(sa, ctx->stream));
        LcSegStats res[32];
        const int nseg = nbands + (contrast_on ? 1 : 0);
        HIPCHK(ctx, hipMemcpyAsync(res, sa.res, (size_t)nseg * sizeof(LcSegStats), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));             // the region's one host wait
        LcRemapArgs ra = {};
        LcHostInfo hi;
        lc_host_constants(res, d.nlevels, d.n, reg.contrast, &ra, &hi);
        ra.bands = d.bands; ra.coeff0 = d.low[d.cur]; ra.n = d.n; ra.nlevels = d.nlevels; ra.curve = reg.curve ? curve_dev : nullptr;
        HIPCHK(ctx, launch_lc_remap(ra, ctx->stream));
        if ((rc = reconstruct_dev(ctx, d, Lnew))) return rc;
        LcBlendArgs ba = {};
        ba.L = L; ba.l_stride = stride; ba.Lnew = Lnew; ba.w = w; ba.h = h;
        if (reg.mask) {
            if (reg.mask->on_device) { ba.mask = reg.mask->p; ba.m_stride = (size_t)(reg.mask->row_stride_bytes / 4); }
            else {
                float *m;
                if ((rc = plane_to_pool(ctx, reg.mask, P_LC_MASK, &m))) return rc;
                ba.mask = m; ba.m_stride = w;
            }
        }
        HIPCHK(ctx, launch_lc_blend(ba, ctx->stream));
        if (info && r == nregions - 1) {
            info->nlevels = d.nlevels;
            info->ave = hi.ave; info->min0 = hi.min0; info->max0 = hi.max0;
            for (int k = 0; k < 10; ++k) { info->mean[k] = hi.mean[k]; info->sigma[k] = hi.sigma[k]; info->maxp[k] = hi.maxp[k]; }
        }
    }
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_local_contrast(artgpu_ctx *ctx, artgpu_plane *L, const artgpu_local_contrast_region *regions, int nregions, double scale,
                          artgpu_local_contrast_info *info)
{
    StageScope scope_(ctx, "ImProcFunctions::localContrast");
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(L)) return fail(ctx, ARTGPU_EINVAL, "local_contrast: bad plane");
    int rc;
    if ((rc = local_contrast_check(ctx, L->w, L->h, regions, nregions, scale, "local_contrast"))) return rc;
    if (info) *info = artgpu_local_contrast_info{};
    if (nregions == 0) return ARTGPU_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (L->on_device) return local_contrast_dev(ctx, L->p, (size_t)(L->row_stride_bytes / 4), L->w, L->h, regions, nregions, info);
    float *work;
    if ((rc = plane_to_pool(ctx, L, P_LC_L, &work)) || (rc = local_contrast_dev(ctx, work, L->w, L->w, L->h, regions, nregions, info))) return rc;
    return pool_to_plane(ctx, work, L);
}

} // extern "C"

// ---------------------------------------------------------------------------------------------
// ImProcFunctions::dehaze
// ---------------------------------------------------------------------------------------------

extern "C" {

int artgpu_dehaze_strength_lut(const double *points, int npoints, float lut[65536])
{
    if (!lut || npoints < 0 || (npoints > 0 && !points)) return ARTGPU_EINVAL;
    dh_strength_lut(points, npoints, lut);
    return ARTGPU_OK;
}

int artgpu_dehaze_estimate_ambient(const float *R, const float *G, const float *B, int ww, int hh, float ambient[3], float *max_t)
{
    if (!R || !G || !B || ww < 1 || hh < 1 || !ambient || !max_t) return ARTGPU_EINVAL;
    *max_t = dh_estimate_ambient(R, G, B, ww, hh, ambient);
    return ARTGPU_OK;
}

} // extern "C"

namespace {

// the strength table of the last curve seen: a batch passes the same curve for every frame, and 65536 curve evaluations on the host
// would otherwise be the longest step of the call
static const float *dehaze_strength_cached(const artgpu_dehaze_params *p, std::vector<float> &out)
{
    static std::mutex m;
    static std::vector<double> pts;
    static std::vector<float> lut;
    std::lock_guard<std::mutex> lk(m);
    const std::vector<double> now(p->strength, p->strength + p->nstrength);
    if (lut.empty() || now != pts) {
        lut.resize(65536);
        dh_strength_lut(p->strength, p->nstrength, lut.data());
        pts = now;
    }
    out = lut;
    return out.data();
}

} // namespace

namespace artgpu { namespace api {

// what the call cannot do, before anything is touched: 0, or the code with the message set
int dehaze_check(artgpu_ctx *ctx, int W, int H, const artgpu_dehaze_params *p, const double *ws, double scale, const char *who, DehazePlan *pl)
{
    if (!p || !ws || !(scale > 0.0) || p->nstrength < 0 || (p->nstrength > 0 && !p->strength)) return fail(ctx, ARTGPU_EINVAL, "%s: bad arguments", who);
    dh_thumb_size(W, H, &pl->ww, &pl->hh);
    const int lo = pl->ww < pl->hh ? pl->ww : pl->hh, hi = pl->ww < pl->hh ? pl->hh : pl->ww;
    pl->brad = hi / 20 > 1 ? hi / 20 : 1;
    if (p->blackpoint && lo < 2 * pl->brad + 1)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: black point on a %dx%d frame: the %dx%d thumbnail is narrower than its box blur (radius %d)", who, W, H, pl->ww, pl->hh, pl->brad);
    const int r1 = std::max((int)(5 / scale), 2);
    { const GfGrid g = gf_grid(W, H, r1); pl->w1 = g.w; pl->h1 = g.h; pl->rad1 = g.rad; }
    pl->patch = std::max(std::max(W, H) / 600, 2);
    { const GfGrid g = gf_grid(W, H, pl->patch * 4); pl->w2 = g.w; pl->h2 = g.h; pl->rad2 = g.rad; }
    if (pl->w1 < 1 || pl->h1 < 1 || pl->w2 < 1 || pl->h2 < 1)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: a %dx%d frame has a side shorter than the guided filter's subsampling", who, W, H);
    if (pl->patch > DH_MAX_PATCH || pl->rad1 > HBLUR_MAX_RADIUS || pl->rad2 > HBLUR_MAX_RADIUS || pl->brad > HBLUR_MAX_RADIUS)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: a %dx%d frame is beyond the patch / box radius the kernels hold in LDS", who, W, H);
    pl->npx = (W + pl->patch - 1) / pl->patch; pl->npy = (H + pl->patch - 1) / pl->patch;
    return ARTGPU_OK;
}

// ImProcFunctions::dehaze on device planes (rows of `stride` floats), enqueued on ctx->stream; the host waits once, for the thumbnail
int dehaze_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const artgpu_dehaze_params *p, const double ws[9],
               const DehazePlan &pl, artgpu_dehaze_info *info)
{
    DhImage im = {{planes[0], planes[1], planes[2]}, stride, W, H};
    const size_t n = (size_t)W * H, nl1 = (size_t)pl.w1 * pl.h1, nl2 = (size_t)pl.w2 * pl.h2, nt = (size_t)pl.ww * pl.hh;
    const size_t nlow = std::max(6 * nl1, 4 * nl2);
    const int npartial = H < DH_MAX_PARTIALS ? H : DH_MAX_PARTIALS;
    float *stf, *thumb, *low, *tmp, *T, *grid;
    int rc;
    if ((rc = pool_get(ctx, P_DH_STATE, (64 + DH_MAX_PARTIALS + 65536) * 4, &stf)) || (rc = pool_get(ctx, P_DH_THUMB, (6 * nt + 16) * 4, &thumb)) ||
        (rc = pool_get(ctx, P_DH_LOW, nlow * 4, &low)) || (rc = pool_get(ctx, P_DH_TMP, nlow * 4, &tmp)) || (rc = pool_get(ctx, P_DH_T, n * 4, &T)) ||
        (rc = pool_get(ctx, P_DH_DARK, (size_t)pl.npx * pl.npy * 4, &grid)))
        return rc;
    DhState *st = reinterpret_cast<DhState *>(stf);
    float *partial = stf + 64, *lut_dev = stf + 64 + DH_MAX_PARTIALS;
    // normalize, subtract_black (L325, L346-348)
    HIPCHK(ctx, launch_dh_max(im, partial, npartial, st, ctx->stream));
    DhThumbArgs ta = {};
    ta.im = im; ta.st = st; ta.thumb = thumb; ta.ww = pl.ww; ta.hh = pl.hh;
    if (p->blackpoint) {
        HIPCHK(ctx, launch_dh_thumb(ta, ctx->stream));
        if ((rc = box_blur_planes(ctx, thumb, thumb + 3 * nt, 3, nt, pl.ww, pl.hh, pl.brad))) return rc;
        HIPCHK(ctx, launch_dh_black(thumb, (int)nt, float(p->blackpoint) / 100.f, st, ctx->stream));
    }
    HIPCHK(ctx, launch_dh_normalize(im, st, p->blackpoint ? 1 : 0, ctx->stream));
    // extract_channels (L369): the statistics of the three self-guided filters; their outputs are evaluated where they are read
    DhGuided g1 = {low, nl1, pl.w1, pl.h1, 1e-1f};
    HIPCHK(ctx, launch_dh_gf_subsample(im, nullptr, 0, g1, ctx->stream));
    if ((rc = box_blur_planes(ctx, low, tmp, 6, nl1, pl.w1, pl.h1, pl.rad1))) return rc;
    HIPCHK(ctx, launch_dh_gf_ab(g1, 1, ctx->stream));
    if ((rc = box_blur_planes(ctx, low, tmp, 6, nl1, pl.w1, pl.h1, pl.rad1))) return rc;
    // the thumbnail (L372-381) and the state block come to the host: the call's one wait
    std::vector<float> host(3 * nt + 8);
    if (nt) {
        ta.gf = g1; ta.from_q = 1;
        HIPCHK(ctx, launch_dh_thumb(ta, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(host.data(), thumb, 3 * nt * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipMemcpyAsync(host.data() + 3 * nt, st, sizeof(DhState), hipMemcpyDeviceToHost, ctx->stream));
    std::vector<float> lut_store;
    const float *lut = dehaze_strength_cached(p, lut_store);         // (while the device works)
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const DhState hs = *reinterpret_cast<const DhState *>(host.data() + 3 * nt);
    float ambient[3];
    const float max_t = dh_estimate_ambient(host.data(), host.data() + nt, host.data() + 2 * nt, pl.ww, pl.hh, ambient);
    const float depth = -float(p->depth) / 100.f;
    const float teps = 1e-6f;
    const float t0 = max_t < 0.f ? 0.f : std::max(teps, std::exp(depth * max_t));           // L453-455, the float overload
    if (info) {
        info->haze_detected = max_t < 0.f ? 0 : 1;
        info->patchsize = pl.patch; info->small_w = pl.ww; info->small_h = pl.hh;
        info->maxval = hs.maxval; info->max_t = max_t; info->t0 = t0;
        for (int k = 0; k < 3; ++k) { info->black[k] = hs.black[k]; info->ambient[k] = ambient[k]; }
    }
    if (max_t < 0.f) {                                                // L387-393: probably no haze at all
        HIPCHK(ctx, launch_dh_restore(im, st, ctx->stream));
        return ARTGPU_OK;
    }
    if ((rc = h2d_table(ctx, lut_dev, lut, 65536 * 4))) return rc;
    // the dark channel (L404) and the transmission estimate (L429-436)
    DhDarkArgs da = {};
    da.im = im; da.gf = g1; da.grid = grid; da.patch = pl.patch; da.npx = pl.npx; da.npy = pl.npy;
    da.has_ambient = 1; da.clip = 1;
    da.per_pixel = (ambient[0] > 0.f && ambient[1] > 0.f && ambient[2] > 0.f) ? 0 : 1;
    for (int k = 0; k < 3; ++k) da.ambient[k] = ambient[k];
    HIPCHK(ctx, launch_dh_dark(da, true, ctx->stream));
    DhTransArgs tr = {};
    tr.im = im; tr.st = st; tr.grid = grid; tr.patch = pl.patch; tr.npx = pl.npx; tr.lut = lut_dev; tr.t = T;
    for (int k = 0; k < 3; ++k) tr.ws1[k] = ws[3 + k];
    HIPCHK(ctx, launch_dh_transmission(tr, ctx->stream));
    // guidedFilter(B, t~, t, 4 * patchsize, 1e-5f) (L438-445): its last step is the first of the recovery pass
    DhGuided g2 = {low, nl2, pl.w2, pl.h2, 1e-5f};
    HIPCHK(ctx, launch_dh_gf_subsample(im, T, (size_t)W, g2, ctx->stream));
    if ((rc = box_blur_planes(ctx, low, tmp, 4, nl2, pl.w2, pl.h2, pl.rad2))) return rc;
    HIPCHK(ctx, launch_dh_gf_ab(g2, 0, ctx->stream));
    if ((rc = box_blur_planes(ctx, low + 2 * nl2, tmp, 2, nl2, pl.w2, pl.h2, pl.rad2))) return rc;
    DhRecoverArgs ra = {};
    ra.im = im; ra.st = st; ra.gf = g2; ra.lut = lut_dev; ra.t0 = t0;
    for (int k = 0; k < 3; ++k) { ra.ws1[k] = ws[3 + k]; ra.ambient[k] = ambient[k]; }
    ra.ambientY = (float)(ambient[0] * ws[3] + ambient[1] * ws[4] + ambient[2] * ws[5]);
    ra.show_depth_map = p->show_depth_map ? 1 : 0; ra.luminance = p->luminance ? 1 : 0;
    HIPCHK(ctx, launch_dh_recover(ra, ctx->stream));
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_dehaze(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_dehaze_params *params, const double ws[9], double scale, artgpu_dehaze_info *info)
{
    StageScope scope_(ctx, "ImProcFunctions::dehaze");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !params) return fail(ctx, ARTGPU_EINVAL, "dehaze: null argument");
    if (info) *info = artgpu_dehaze_info{};
    if (!params->enabled) return ARTGPU_OK;                           // L315-320
    if (!plane_ok(&img->r)) return fail(ctx, ARTGPU_EINVAL, "dehaze: bad plane");
    DehazePlan pl;
    int rc;
    if ((rc = dehaze_check(ctx, img->r.w, img->r.h, params, ws, scale, "dehaze", &pl))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "dehaze"))) return rc;
    if ((rc = dehaze_dev(ctx, d.p, d.stride, d.w, d.h, params, ws, pl, info))) return rc;
    return unbind_rgb(ctx, img, &d);
}

int artgpu_dehaze_dark_channel(artgpu_ctx *ctx, const artgpu_rgb *rgb, int patchsize, const float *ambient, int clip, artgpu_plane *dst)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!rgb || !plane_ok(dst) || !plane_ok(&rgb->r) || dst->w != rgb->r.w || dst->h != rgb->r.h) return fail(ctx, ARTGPU_EINVAL, "dehaze_dark_channel: bad plane");
    if (patchsize < 1 || patchsize > DH_MAX_PATCH) return fail(ctx, ARTGPU_EINVAL, "dehaze_dark_channel: patch size 1..%d", DH_MAX_PATCH);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    int rc;
    if ((rc = bind_rgb(ctx, rgb, 4, true, &d, "dehaze_dark_channel"))) return rc;
    DhDarkArgs da = {};
    da.im = DhImage{{d.p[0], d.p[1], d.p[2]}, d.stride, d.w, d.h};
    da.patch = patchsize; da.npx = (d.w + patchsize - 1) / patchsize; da.npy = (d.h + patchsize - 1) / patchsize;
    da.has_ambient = ambient ? 1 : 0; da.clip = clip ? 1 : 0;
    if (ambient) {
        for (int k = 0; k < 3; ++k) da.ambient[k] = ambient[k];
        da.per_pixel = (ambient[0] > 0.f && ambient[1] > 0.f && ambient[2] > 0.f) ? 0 : 1;
    }
    float *out = dst->p;
    size_t out_stride = (size_t)(dst->row_stride_bytes / 4);
    if ((rc = pool_get(ctx, P_DH_DARK, (size_t)da.npx * da.npy * 4, &da.grid))) return rc;
    if (!dst->on_device) {
        if ((rc = pool_get(ctx, P_DH_T, (size_t)d.w * d.h * 4, &out))) return rc;
        out_stride = d.w;
    }
    HIPCHK(ctx, launch_dh_dark(da, false, ctx->stream));
    DhExpandArgs ea = {da.grid, patchsize, da.npx, out, out_stride, d.w, d.h};
    HIPCHK(ctx, launch_dh_expand(ea, ctx->stream));
    return dst->on_device ? ARTGPU_OK : pool_to_plane(ctx, out, dst);
}

} // extern "C"

// ---------------------------------------------------------------------------------------------
// ImProcFunctions::textureBoost
// ---------------------------------------------------------------------------------------------

namespace {

// 0, or the code with the message set
static int tb_plan(artgpu_ctx *ctx, int W, int H, const artgpu_texture_boost_region *r, double scale, int high_detail, const char *who, TbPlan *pl)
{
    if (!std::isfinite(r->strength) || !std::isfinite(r->detail_threshold) || !(r->detail_threshold > 0.0))
        return fail(ctx, ARTGPU_EINVAL, "%s: strength %g / detail threshold %g", who, r->strength, r->detail_threshold);
    if (r->iterations < 1) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: %d iterations (the reference then only divides and multiplies by 65535)", who, r->iterations);
    *pl = TbPlan{};
    const float full_radius = r->detail_threshold * 3.5f;
    const float fradius = full_radius / scale;
    const int radius = std::max(int(fradius + 0.5f), 1);
    const float delta = radius / fradius;
    const float s = r->strength >= 0 ? sh_pow_F(r->strength / 2.f, 0.3f) * 2.f : r->strength;
    pl->strength = s >= 0 ? 1.f + s : 1.f / (1.f - s);
    pl->strength2 = s >= 0 ? 1.f + s / 4.f : 1.f / (1.f - s / 2.f);
    pl->radius = radius;
    pl->isguided = full_radius >= 1.f ? 1 : 0;
    pl->w = W; pl->h = H;
    if (fradius > 1.f && delta > 1.01f) {
        pl->rescaled = 1;
        pl->w = int(W * delta + 0.5f);
        pl->h = int(H * delta + 0.5f);
    }
    if (!pl->isguided) {
        if (!high_detail) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: detail threshold %g without high_detail (gaussianBlur at a sub-pixel sigma is not on the device path)", who, r->detail_threshold);
        pl->K = tb_gaussian_kernel(fradius, pl->coef);
        if (pl->K > TB_MAX_K) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: sigma %g needs a %dx%d gaussian, the kernels hold %dx%d", who, fradius, pl->K, pl->K, TB_MAX_K, TB_MAX_K);
    } else {
        { const GfGrid g = gf_grid(pl->w, pl->h, radius); pl->w1 = g.w; pl->h1 = g.h; pl->rad1 = g.rad; }
    }
    { const GfGrid g = gf_grid(pl->w, pl->h, radius * 4); pl->w2 = g.w; pl->h2 = g.h; pl->rad2 = g.rad; }
    if ((pl->isguided && (pl->w1 < 1 || pl->h1 < 1)) || pl->w2 < 1 || pl->h2 < 1)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: a %dx%d plane has a side shorter than the guided filter's subsampling", who, pl->w, pl->h);
    if (pl->rad1 > HBLUR_MAX_RADIUS || pl->rad2 > HBLUR_MAX_RADIUS)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: box radius %d is above the %d the blur kernels hold in LDS", who, std::max(pl->rad1, pl->rad2), HBLUR_MAX_RADIUS);
    return ARTGPU_OK;
}

// one self-guided filter's statistics on `mid`: the grid ends as mean a / mean b
static int tb_guided_stats(artgpu_ctx *ctx, const float *mid, int w, int h, const DhGuided &gf, int rad, float *tmp)
{
    int rc;
    HIPCHK(ctx, launch_tb_gf_subsample(mid, w, h, gf, ctx->stream));
    if ((rc = box_blur_planes(ctx, gf.low, tmp, 2, gf.nl, gf.w, gf.h, rad))) return rc;
    HIPCHK(ctx, launch_tb_gf_ab(gf, ctx->stream));
    return box_blur_planes(ctx, gf.low, tmp, 2, gf.nl, gf.w, gf.h, rad);
}

// texture_boost (iptextureboost.cc:37-178) on a device Y plane (rows of `stride` floats), enqueued on ctx->stream without a host wait;
// do_blend: the region loop's intp(mask, Y, YY) (L234-240) is part of the last store
static int texture_boost_region_dev(artgpu_ctx *ctx, float *Y, size_t stride, int W, int H, const TbPlan &pl, int iterations, int do_blend,
                                    const artgpu_plane *mask, TbState **state)
{
    const size_t nw = (size_t)pl.w * pl.h, nl1 = pl.isguided ? (size_t)pl.w1 * pl.h1 : 0, nl2 = (size_t)pl.w2 * pl.h2;
    const size_t nlow = 2 * std::max(nl1, nl2);
    float *planes, *low, *tmp, *stf;
    int rc;
    if ((rc = pool_get(ctx, P_TB_PLANES, (pl.isguided ? 2 : 3) * nw * 4, &planes)) || (rc = pool_get(ctx, P_TB_LOW, nlow * 4, &low)) ||
        (rc = pool_get(ctx, P_TB_TMP, nlow * 4, &tmp)) || (rc = pool_get(ctx, P_TB_STATE, (sizeof(TbState) / 4 + TB_MAX_PARTIALS) * 4, &stf)))
        return rc;
    TbState *st = reinterpret_cast<TbState *>(stf);
    *state = st;
    float *src = planes, *mid = planes + nw, *spare = planes + 2 * nw;      // (spare: the convolution's other plane)
    const float *mk = nullptr;
    size_t m_stride = 0;
    if (do_blend && mask) {
        if (mask->on_device) { mk = mask->p; m_stride = (size_t)(mask->row_stride_bytes / 4); }
        else {
            float *m;
            if ((rc = plane_to_pool(ctx, mask, P_TB_MASK, &m))) return rc;
            mk = m; m_stride = W;
        }
    }
    TbPrepareArgs pa = {Y, stride, W, H, src, mid, pl.w, pl.h, stf + sizeof(TbState) / 4};
    HIPCHK(ctx, launch_tb_prepare(pa, st, ctx->stream));
    for (int i = 0; i < iterations; ++i) {
        if (pl.isguided) {
            const DhGuided g1 = {low, nl1, pl.w1, pl.h1, 0.001f};
            if ((rc = tb_guided_stats(ctx, mid, pl.w, pl.h, g1, pl.rad1, tmp))) return rc;
            HIPCHK(ctx, launch_tb_gf_finish(mid, pl.w, pl.h, g1, ctx->stream));
        } else {
            TbConvArgs ca = {};
            ca.src = mid; ca.dst = spare; ca.w = pl.w; ca.h = pl.h; ca.K = pl.K;
            std::copy(pl.coef, pl.coef + pl.K * pl.K, ca.coef);
            HIPCHK(ctx, launch_tb_conv(ca, ctx->stream));
            std::swap(mid, spare);
        }
        const DhGuided g2 = {low, nl2, pl.w2, pl.h2, 0.001f / 10.f};
        if ((rc = tb_guided_stats(ctx, mid, pl.w, pl.h, g2, pl.rad2, tmp))) return rc;
        TbCombineArgs cb = {};
        cb.src = src; cb.mid = mid; cb.w = pl.w; cb.h = pl.h; cb.gf = g2; cb.st = st;
        cb.strength = pl.strength; cb.strength2 = pl.strength2; cb.blend = std::ldexp(1.f, -i);      // 1.f / std::pow(2.f, i)
        cb.last = (i == iterations - 1 && !pl.rescaled) ? 1 : 0;
        cb.Y = Y; cb.stride = stride; cb.do_blend = do_blend; cb.mask = mk; cb.m_stride = m_stride;
        HIPCHK(ctx, launch_tb_combine(cb, ctx->stream));
    }
    if (pl.rescaled) {
        const TbDownArgs da = {src, pl.w, pl.h, Y, stride, W, H, do_blend, mk, m_stride};
        HIPCHK(ctx, launch_tb_downscale(da, ctx->stream));
    }
    return ARTGPU_OK;
}

// what `info` reports of a region that ran; the minimum costs the call's one host wait
static int tb_fill_info(artgpu_ctx *ctx, const TbPlan &pl, const TbState *st, artgpu_texture_boost_info *info)
{
    float minval;
    HIPCHK(ctx, hipMemcpyAsync(&minval, &st->minval, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    info->radius = pl.radius; info->isguided = pl.isguided; info->rescaled = pl.rescaled; info->work_w = pl.w; info->work_h = pl.h;
    info->kernel_size = pl.K; info->minval = minval; info->strength = pl.strength; info->strength2 = pl.strength2;
    return ARTGPU_OK;
}

} // namespace

namespace artgpu { namespace api {

// the region list of the whole tool: a plan per region that runs (strength != 0, L227), in order
int tb_check(artgpu_ctx *ctx, int W, int H, const artgpu_texture_boost_region *regions, int nregions, const double *ws, double scale, int high_detail,
                    const char *who, std::vector<TbPlan> *plans)
{
    if (nregions < 0 || (nregions > 0 && !regions) || !ws || !(scale > 0.0)) return fail(ctx, ARTGPU_EINVAL, "%s: bad arguments", who);
    plans->clear();
    for (int r = 0; r < nregions; ++r) {
        const artgpu_plane *m = regions[r].mask;
        if (m && (!plane_ok(m) || m->w != W || m->h != H)) return fail(ctx, ARTGPU_EINVAL, "%s: the mask of region %d must be a %dx%d plane", who, r, W, H);
        if (regions[r].strength == 0) continue;
        TbPlan pl;
        int rc;
        if ((rc = tb_plan(ctx, W, H, &regions[r], scale, high_detail, who, &pl))) return rc;
        plans->push_back(pl);
    }
    return ARTGPU_OK;
}

// ImProcFunctions::textureBoost (L198-242) on device planes in RGB mode: setMode(YUV), the regions that run, setMode(RGB) when asked for.
// already_yuv: the tool ahead (colorCorrection) left the image in YUV mode, where the reference's setMode(YUV) does nothing
int texture_boost_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const artgpu_texture_boost_region *regions, int nregions,
                             const double ws[9], const std::vector<TbPlan> &plans, int to_rgb, artgpu_texture_boost_info *info, int already_yuv)
{
    PixArgs ya = {};                                                   // Imagefloat::setMode (yuv_mode_kernel: do_clip 0 = to YUV, 1 = to RGB)
    for (int k = 0; k < 3; ++k) { ya.dst[k] = planes[k]; ya.mul[k] = (float)ws[3 + k]; }
    ya.dst_stride = stride; ya.w = W; ya.h = H;
    if (!already_yuv) HIPCHK(ctx, launch_yuv_mode(ya, ctx->stream));
    int rc;
    size_t k = 0;
    TbState *st = nullptr;
    for (int r = 0; r < nregions; ++r) {
        if (regions[r].strength == 0) continue;
        if ((rc = texture_boost_region_dev(ctx, planes[1], stride, W, H, plans[k], regions[r].iterations, 1, regions[r].mask, &st))) return rc;
        ++k;
    }
    if (info && k > 0 && (rc = tb_fill_info(ctx, plans[k - 1], st, info))) return rc;
    if (to_rgb) {
        ya.do_clip = 1;
        HIPCHK(ctx, launch_yuv_mode(ya, ctx->stream));
    }
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_texture_boost_plane(artgpu_ctx *ctx, artgpu_plane *Y, const artgpu_texture_boost_region *region, double scale, int high_detail,
                               artgpu_texture_boost_info *info)
{
    StageScope scope_(ctx, "texture_boost");
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(Y) || !region || !(scale > 0.0)) return fail(ctx, ARTGPU_EINVAL, "texture_boost_plane: bad arguments");
    if (info) *info = artgpu_texture_boost_info{};
    TbPlan pl;
    int rc;
    if ((rc = tb_plan(ctx, Y->w, Y->h, region, scale, high_detail, "texture_boost_plane", &pl))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    float *work = Y->p;
    size_t stride = (size_t)(Y->row_stride_bytes / 4);
    if (!Y->on_device) {
        if ((rc = plane_to_pool(ctx, Y, P_TB_Y, &work))) return rc;
        stride = Y->w;
    }
    TbState *st = nullptr;
    if ((rc = texture_boost_region_dev(ctx, work, stride, Y->w, Y->h, pl, region->iterations, 0, nullptr, &st))) return rc;
    if (info && (rc = tb_fill_info(ctx, pl, st, info))) return rc;
    return Y->on_device ? ARTGPU_OK : pool_to_plane(ctx, work, Y);
}

int artgpu_texture_boost(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_texture_boost_region *regions, int nregions, const double ws[9], double scale,
                         int high_detail, int to_rgb, artgpu_texture_boost_info *info)
{
    StageScope scope_(ctx, "ImProcFunctions::textureBoost");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !plane_ok(&img->r)) return fail(ctx, ARTGPU_EINVAL, "texture_boost: bad image");
    if (info) *info = artgpu_texture_boost_info{};
    std::vector<TbPlan> plans;
    int rc;
    if ((rc = tb_check(ctx, img->r.w, img->r.h, regions, nregions, ws, scale, high_detail, "texture_boost", &plans))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "texture_boost"))) return rc;
    if ((rc = texture_boost_dev(ctx, d.p, d.stride, d.w, d.h, regions, nregions, ws, plans, to_rgb, info))) return rc;
    return unbind_rgb(ctx, img, &d);
}

} // extern "C"

// ---------------------------------------------------------------------------------------------
// region masks: rtengine::generateMasks, parametric path (masks.cc:1037-1516)
// ---------------------------------------------------------------------------------------------

namespace {

// one rtengine::guidedFilter call as artgpu_guided_filter will run it: decided in the plan, so that nothing starts before everything fits
struct MkFilter { int on, r; };

// ParametricMask's default curves (procparams.cc:1014-1053)
const double MK_DEFAULT_HUE[9] = {1 /* FCT_MinMaxCPoints */, 0.166666667, 1., 0.35, 0.35, 0.8287775246, 1., 0.35, 0.35};
const double MK_DEFAULT_CL[9] = {1, 0., 1., 0.35, 0.35, 1., 1., 0.35, 0.35};

// L1068-1080: enabled, not empty, not FCT_Linear, not the default
bool mk_curve_present(const artgpu_mask_params &m, const double *pts, int n, const double *dflt)
{
    if (!m.parametric_enabled || !pts || n <= 0 || pts[0] == 0 /* FCT_Linear */) return false;
    return !(n == 9 && std::equal(pts, pts + 9, dflt));
}
int mk_filter_check(artgpu_ctx *ctx, int W, int H, int r, const char *who, const char *what)
{
    const GfGrid grid = gf_grid(W, H, r);
    const int sub = grid.sub, w = grid.w, h = grid.h, rad = grid.rad;
    if (w < 1 || h < 1) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: %s: a %dx%d image has a side shorter than the guided filter's subsampling %d", who, what, W, H, sub);
    if (rad > HBLUR_MAX_RADIUS) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: %s: box radius %d (radius %d / subsampling %d) is above the %d the blur kernels hold in LDS", who, what, rad, r, sub, HBLUR_MAX_RADIUS);
    return ARTGPU_OK;
}

} // namespace

namespace artgpu { namespace api {

// everything generateMasks decides before its first pixel loop, and every reason not to run
int mk_plan(artgpu_ctx *ctx, int W, int H, int mode, const double *ws, const artgpu_mask_params *masks, int n, int full_w, int full_h, double scale,
            bool want_L, bool want_ab, const char *who, MkPlan *pl, artgpu_masks_info *info)
{
    if (!masks || n <= 0 || !(scale > 0.0) || (!want_L && !want_ab)) return fail(ctx, ARTGPU_EINVAL, "%s: bad arguments", who);
    if (mode != ARTGPU_MASKS_MODE_RGB && mode != ARTGPU_MASKS_MODE_LAB) {
        if (mode == ARTGPU_MASKS_MODE_YUV || mode == ARTGPU_MASKS_MODE_XYZ) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: image mode %d (RGB and LAB are on the device path)", who, mode);
        return fail(ctx, ARTGPU_EINVAL, "%s: image mode %d", who, mode);
    }
    if (mode == ARTGPU_MASKS_MODE_RGB && !ws) return fail(ctx, ARTGPU_EINVAL, "%s: RGB mode needs the working-space matrix", who);
    if (W < ARTGPU_MASKS_MIN_SIZE || H < ARTGPU_MASKS_MIN_SIZE)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: %dx%d is below %dx%d", who, W, H, ARTGPU_MASKS_MIN_SIZE, ARTGPU_MASKS_MIN_SIZE);
    *pl = MkPlan{};
    pl->W = W; pl->H = H; pl->lab = mode == ARTGPU_MASKS_MODE_LAB; pl->want_L = want_L; pl->want_ab = want_ab;
    pl->reg.resize(n);
    bool any_light = false;
    int rc;
    for (int i = 0; i < n; ++i) {
        const artgpu_mask_params &m = masks[i];
        MkRegionPlan &r = pl->reg[i];
        if (m.deltae_enabled) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: the deltaE mask (cmsCIE2000DeltaE) is not on the device path", who, i);
        if (m.drawn_enabled || m.external_enabled || m.linked_enabled) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: drawn, external and linked masks are not on the device path", who, i);
        if (!m.curve_is_identity) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: a mask curve other than the identity is not on the device path", who, i);
        if (m.show_mask) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: show_mask is not on the device path", who, i);
        if (m.nhue < 0 || m.nchromaticity < 0 || m.nlightness < 0 || m.posterization < 0) return fail(ctx, ARTGPU_EINVAL, "%s: region %d: negative curve length or posterization", who, i);
        if (m.area && (!plane_ok(m.area) || m.area->w != W || m.area->h != H)) return fail(ctx, ARTGPU_EINVAL, "%s: the area plane of region %d must be a %dx%d plane", who, i, W, H);
        const double *pts[3] = {m.hue, m.chromaticity, m.lightness};
        const int npts[3] = {m.nhue, m.nchromaticity, m.nlightness};
        for (int k = 0; k < 3; ++k) {
            r.curve[k] = MkCurve{0, 0};
            if (!mk_curve_present(m, pts[k], npts[k], k == MK_HUE ? MK_DEFAULT_HUE : MK_DEFAULT_CL)) continue;
            pl->has_mask = 1;
            std::vector<double> x, y, sl;
            if (flat_curve_polyline(pts[k], npts[k], k == MK_HUE, 1000 /* CURVES_MIN_POLY_POINTS */, 0.5, x, y, sl)) {
                r.curve[k] = MkCurve{(int)r.tab.size(), (int)x.size()};
                r.tab.insert(r.tab.end(), x.begin(), x.end());
                r.tab.insert(r.tab.end(), y.begin(), y.end());
                r.tab.insert(r.tab.end(), sl.begin(), sl.end());
            } else {
                r.curve[k] = MkCurve{0, -1};        // FCT_Empty: getVal returns identityValue
            }
            if (k == MK_LIGHT) {
                any_light = true;
                const float d = float(m.lightness_detail) / 100.f;
                r.ldetail = d < 0.f ? 0.f : (d > 1.f ? 1.f : d);
            }
        }
        if (r.tab.size() * sizeof(double) > (size_t)MK_LDS_BYTES) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: the curves' polylines (%zu bytes) do not fit LDS", who, i, r.tab.size() * 8);
        if (m.opacity < 100) pl->has_mask = 1;
    }
    pl->need_ll = want_L && any_light;
    if (pl->need_ll) {
        const int m1 = full_w > W ? full_w : W, m2 = full_h > H ? full_h : H;
        const float radius = (m1 > m2 ? m1 : m2) / 30.f;
        pl->ll_r = (int)radius;
        pl->ll_r_small = (int)(10.f / scale);
        if (pl->ll_r_small > 0 && (rc = mk_filter_check(ctx, W, H, pl->ll_r_small, who, "lightness detail"))) return rc;
        if ((rc = mk_filter_check(ctx, W, H, pl->ll_r, who, "lightness detail"))) return rc;
    }
    if (full_w < 0) full_w = W;
    if (full_h < 0) full_h = H;
    pl->need_guide = pl->has_mask;
    for (int i = 0; i < n; ++i) {
        const artgpu_mask_params &m = masks[i];
        MkRegionPlan &r = pl->reg[i];
        float blur = m.parametric_enabled ? (float)m.blur : 0.f;
        if (pl->has_mask && blur > -10.f) {
            blur = blur < 0.f ? -1.f / blur : 1.f + blur;
            r.blurred = 1;
            r.r1 = std::max(int(4 / scale * blur + 0.5), 1);
            r.r2 = std::max(int(25 / scale * blur + 0.5), 1);
            if (want_ab && (rc = mk_filter_check(ctx, W, H, r.r1, who, "ab mask blur"))) return rc;
            if (want_L && (rc = mk_filter_check(ctx, W, H, r.r2, who, "L mask blur"))) return rc;
        }
        if (m.parametric_enabled && m.contrast_threshold != 0) {        // contrast_threshold_mask (L696-734)
            float fscale = (float)scale;
            const int d = std::max(W, H);
            const float s = float(d) / 1920.f;
            r.cthr = 1; r.cthr_neg = m.contrast_threshold < 0; r.cw = W; r.ch = H;
            if (s > 1.f) { fscale *= s; r.cw = W / s; r.ch = H / s; }
            const float s_scale = std::sqrt(fscale);
            r.cthr_thresh = float(std::abs(m.contrast_threshold)) / 100.f * s_scale;
            r.cthr_blur = std::max(m.blur, 2.0) / s_scale;
            if (r.cw < 8 || r.ch < 8) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: the contrast threshold's %dx%d plane is below 8x8", who, i, r.cw, r.ch);
            pl->need_guide = 1;
        }
        if (m.posterization) {                                          // mask_postprocess (L737-802)
            static const float pp[] = {30.f, 20.f, 10.f, 5.f, 3.f, 2.f};
            r.post_p = pp[std::min(std::max(m.posterization, 0), 6) - 1];
            if (m.smoothing) {
                const float radius_coeff = 10.f * (101.f - float(std::min(std::max(m.smoothing, 0), 100)));
                const float radius = std::max(full_w, full_h) / radius_coeff;
                r.smooth = 1; r.smooth_r = (int)radius;
                const float l = 0.0f, h = 0.25f;
                const float f0 = float(m.smoothing) / 100.f, f = f0 < 0.f ? 0.f : (f0 > 1.f ? 1.f : f0);
                const float f2 = std::max(f - l, 0.f) / (h - l);
                const float v = f < l ? 0.f : (f > h ? 1.f : (f2 < 0.5f ? 2.f * (f2 * f2) : 1.f - 2.f * ((1.f - f2) * (1.f - f2))));
                r.fillval = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
                if ((rc = mk_filter_check(ctx, W, H, r.smooth_r, who, "mask smoothing"))) return rc;
                pl->need_guide = 1;
            }
        }
        r.inverted = m.inverted ? 1 : 0;
        if (m.opacity < 100) {
            const float b = float(m.opacity) / 100.f;
            r.has_opacity = 1; r.opacity = b < 0.f ? 0.f : (b > 1.f ? 1.f : b);
        }
    }
    if (info)
        for (int i = 0; i < n; ++i) {
            const MkRegionPlan &r = pl->reg[i];
            info[i] = artgpu_masks_info{pl->has_mask, pl->need_ll, pl->need_ll ? pl->ll_r_small : 0, pl->need_ll ? pl->ll_r : 0, r.blurred, r.r1, r.r2,
                                        r.cthr ? r.cw : 0, r.cthr ? r.ch : 0, r.smooth ? r.smooth_r : -1};
        }
    return ARTGPU_OK;
}

// generateMasks on a device image (rows of `stride` floats), enqueued on ctx->stream.  Lout / about: n contiguous W x H device planes each,
// or nullptr.  `masks` is read for the area planes only.
int masks_dev(artgpu_ctx *ctx, float *const img[3], size_t stride, const double *ws, const artgpu_mask_params *masks, const MkPlan &pl,
              float *Lout, float *about)
{
    const int W = pl.W, H = pl.H, n = (int)pl.reg.size();
    const size_t np = (size_t)W * H;
    float *work, *cplanes = nullptr, *tabs = nullptr;
    int rc;
    // guide | LL | thr | one blend plane per region
    if ((rc = pool_get(ctx, P_MK_WORK, (size_t)(3 + (pl.has_mask ? n : 0)) * np * 4, &work))) return rc;
    float *guide = work, *LL = work + np, *thr = work + 2 * np, *blend = work + 3 * np;
    MkImage im = {{img[0], img[1], img[2]}, stride, W, H, pl.lab};
    float wp[9] = {};
    if (!pl.lab) {
        for (int k = 0; k < 9; ++k) wp[k] = (float)ws[k];
        if ((rc = lab_tabs_dev(ctx, &tabs))) return rc;
    }
    if (pl.need_ll) {                                                   // L1113-1137
        MkLLArgs a = {};
        a.im = im; std::copy(wp, wp + 9, a.wp); a.cachef = tabs; a.cachefy = tabs ? tabs + 65536 : nullptr; a.guide = guide; a.LL = LL;
        HIPCHK(ctx, launch_mk_ll(a, ctx->stream));
        if (pl.ll_r_small > 0 && (rc = guided_filter_dev(ctx, guide, guide, guide, W, W, H, pl.ll_r_small, 0.01f, 0, "generate_masks"))) return rc;
        if ((rc = guided_filter_dev(ctx, guide, LL, LL, W, W, H, pl.ll_r, 0.001f, 0, "generate_masks"))) return rc;
    }
    if (pl.need_guide) {                                                // L1171-1241, MK_GROUP regions (and MK_LDS_BYTES of polylines) per launch
        MkFusedArgs a = {};
        a.im = im; std::copy(wp, wp + 9, a.wp); a.cachef = tabs; a.cachefy = tabs ? tabs + 65536 : nullptr; a.guide = guide;
        a.LL = pl.need_ll ? LL : nullptr;
        if (!pl.has_mask) {
            HIPCHK(ctx, launch_mk_fused(a, ctx->stream));
        } else {
            size_t total = 0;
            for (const MkRegionPlan &r : pl.reg) total += r.tab.size();
            float *tabf;
            if ((rc = pool_get(ctx, P_MK_TAB, total * 8 + 64, &tabf))) return rc;
            double *dtab = reinterpret_cast<double *>(tabf);
            std::vector<double> host;
            host.reserve(total);
            for (const MkRegionPlan &r : pl.reg) host.insert(host.end(), r.tab.begin(), r.tab.end());
            if (total && (rc = h2d_table(ctx, dtab, host.data(), total * 8))) return rc;
            size_t base = 0;
            for (int i0 = 0; i0 < n;) {
                a.nreg = 0; a.tab = dtab + base; a.tab_len = 0;
                while (i0 + a.nreg < n && a.nreg < MK_GROUP) {
                    const MkRegionPlan &r = pl.reg[i0 + a.nreg];
                    if (a.nreg && ((size_t)a.tab_len + r.tab.size()) * 8 > (size_t)MK_LDS_BYTES) break;
                    for (int k = 0; k < 3; ++k) a.curve[a.nreg][k] = MkCurve{r.curve[k].off + a.tab_len, r.curve[k].n};
                    a.ldetail[a.nreg] = r.ldetail;
                    a.out[a.nreg] = blend + (size_t)(i0 + a.nreg) * np;
                    a.tab_len += (int)r.tab.size();
                    ++a.nreg;
                }
                HIPCHK(ctx, launch_mk_fused(a, ctx->stream));
                base += a.tab_len; i0 += a.nreg;
            }
        }
    }
    for (int i = 0; i < n; ++i) {
        const MkRegionPlan &r = pl.reg[i];
        const float *cthr = nullptr;
        if (r.cthr) {                                                   // contrast_threshold_mask (L696-734)
            const size_t ns = (size_t)r.cw * r.ch;
            if ((rc = pool_get(ctx, P_MK_CTHR, (np + 3 * ns) * 4, &cplanes))) return rc;
            float *full = cplanes, *src = cplanes + np, *dst = src + ns, *gtmp = dst + ns;
            const bool rescaled = r.cw != W || r.ch != H;
            if (rescaled) HIPCHK(ctx, launch_mk_rescale(guide, W, H, src, r.cw, r.ch, ctx->stream));
            DualArgs da = {};
            da.L = rescaled ? src : guide; da.blend = rescaled ? dst : full; da.w = r.cw; da.h = r.ch; da.threshold = r.cthr_thresh;
            HIPCHK(ctx, launch_blend_mask_lum(da, 32768.f, ctx->stream));
            if ((rc = gaussian_dev(ctx, da.blend, gtmp, r.cw, r.ch, (double)r.cthr_blur))) return rc;
            if (rescaled) HIPCHK(ctx, launch_mk_rescale(dst, r.cw, r.ch, full, W, H, ctx->stream));
            cthr = full;
        }
        const float *area = nullptr; size_t area_stride = 0;
        if (masks[i].area) {
            if (masks[i].area->on_device) { area = masks[i].area->p; area_stride = (size_t)(masks[i].area->row_stride_bytes / 4); }
            else { float *ap; if ((rc = plane_to_pool(ctx, masks[i].area, P_MK_AREA, &ap))) return rc; area = ap; area_stride = W; }
        }
        for (int which = 0; which < 2; ++which) {                       // abmask first, like L1264-1269
            float *out = which == 0 ? about : Lout;
            if (!out) continue;
            out += (size_t)i * np;
            if (pl.has_mask) {
                float *b = blend + (size_t)i * np;
                if (r.blurred) {
                    if ((rc = guided_filter_dev(ctx, guide, b, out, W, W, H, which == 0 ? r.r1 : r.r2, which == 0 ? 0.001f : 0.0001f, 0, "generate_masks"))) return rc;
                } else {
                    HIPCHK(ctx, hipMemcpyAsync(out, b, np * 4, hipMemcpyDeviceToDevice, ctx->stream));
                }
            }
            MkTailArgs t = {};
            t.m = out; t.w = W; t.h = H; t.fill_one = !pl.has_mask; t.clamp = pl.has_mask;
            t.cthr = cthr; t.cthr_neg = r.cthr_neg; t.area = area; t.area_stride = area_stride; t.post_p = r.post_p;
            if (r.smooth) { t.thr_out = thr; t.fillval = r.fillval; }
            else { t.inverted = r.inverted; t.has_opacity = r.has_opacity; t.opacity = r.opacity; }
            HIPCHK(ctx, launch_mk_tail(t, ctx->stream));
            if (r.smooth) {                                             // L772-799, then L1438-1467
                if ((rc = guided_filter_dev(ctx, guide, out, out, W, W, H, r.smooth_r, 0.015f, 0, "generate_masks"))) return rc;
                MkTailArgs t2 = {};
                t2.m = out; t2.w = W; t2.h = H; t2.thr_in = thr; t2.inverted = r.inverted; t2.has_opacity = r.has_opacity; t2.opacity = r.opacity;
                HIPCHK(ctx, launch_mk_tail(t2, ctx->stream));
            }
        }
    }
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_generate_masks(artgpu_ctx *ctx, const artgpu_rgb *img, int mode, const double ws[9], const artgpu_mask_params *masks, int n,
                          int full_w, int full_h, double scale, artgpu_plane *Lmask, artgpu_plane *abmask, artgpu_masks_info *info)
{
    StageScope scope_(ctx, "generateMasks");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !plane_ok(&img->r)) return fail(ctx, ARTGPU_EINVAL, "generate_masks: bad image");
    const int W = img->r.w, H = img->r.h;
    MkPlan pl;
    int rc;
    if ((rc = mk_plan(ctx, W, H, mode, ws, masks, n, full_w, full_h, scale, Lmask != nullptr, abmask != nullptr, "generate_masks", &pl, info))) return rc;
    for (artgpu_plane *set : {Lmask, abmask})
        for (int i = 0; set && i < n; ++i)
            if (!plane_ok(&set[i]) || set[i].w != W || set[i].h != H) return fail(ctx, ARTGPU_EINVAL, "generate_masks: output plane %d must be a %dx%d plane", i, W, H);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "generate_masks"))) return rc;
    const size_t np = (size_t)W * H;
    float *outs;
    if ((rc = pool_get(ctx, P_MK_OUT, (size_t)n * np * 4 * ((Lmask ? 1 : 0) + (abmask ? 1 : 0)), &outs))) return rc;
    float *Lout = Lmask ? outs : nullptr, *about = abmask ? outs + (Lmask ? (size_t)n * np : 0) : nullptr;
    if ((rc = masks_dev(ctx, d.p, d.stride, ws, masks, pl, Lout, about))) return rc;
    for (int i = 0; i < n; ++i) {
        if (Lmask && (rc = pool_to_plane(ctx, Lout + (size_t)i * np, &Lmask[i]))) return rc;
        if (abmask && (rc = pool_to_plane(ctx, about + (size_t)i * np, &abmask[i]))) return rc;
    }
    return ARTGPU_OK;
}

} // extern "C"

// ---------------------------------------------------------------------------------------------
// smoothing: ImProcFunctions::guidedSmoothing, modes GUIDED and NLMEANS
// ---------------------------------------------------------------------------------------------

namespace {

// floats of P_SM_PLANES a region needs
size_t sm_region_floats(const SmRegionPlan &p)
{
    const size_t nw = (size_t)p.ww * p.hh;
    if (p.skipped == ARTGPU_SMOOTHING_SKIP_EMPTY || p.skipped == ARTGPU_SMOOTHING_SKIP_RADIUS) return 0;
    if (p.mode == ARTGPU_SMOOTHING_GUIDED) return ((p.channel == SM_CH_LC ? 3 : 7) + (p.iterations > 1 ? 3 : 0)) * nw;
    return (p.channel == SM_CH_L ? 1 : p.channel == SM_CH_LC ? (p.skipped ? 0 : 3) : 4) * nw;
}

// one region on the normalised device image; `mask`: the region's blend plane on the device (rows of mstride floats) or nullptr
// norm_in: the image is not normalised yet and this (full-frame) region does it; denorm_out: this (full-frame) region stores * 65535.f
int sm_region_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, const SmRegionPlan &p, const float *mask, size_t mstride, const double *ws, double scale, float *big,
                  bool norm_in, bool denorm_out)
{
    int rc;
    const size_t nw = (size_t)p.ww * p.hh, off = (size_t)p.y0 * stride + p.x0;
    SmArgs a = {};
    for (int k = 0; k < 3; ++k) { a.img[k] = planes[k] + off; a.ws1[k] = ws[3 + k]; }
    a.stride = stride;
    a.mask = mask ? mask + (size_t)p.y0 * mstride + p.x0 : nullptr; a.mask_stride = mstride;
    a.ww = p.ww; a.hh = p.hh; a.channel = p.channel;
    a.img_norm = norm_in ? 1 : 0; a.out_denorm = denorm_out ? 1 : 0;
    if (p.mode == ARTGPU_SMOOTHING_GUIDED) {
        if (p.skipped) {                                              // r == 0: working == rgb, blended all the same (L1050-1064)
            a.channel = SM_CH_LC;
            HIPCHK(ctx, launch_sm_nlm_merge(a, ctx->stream));
            return ARTGPU_OK;
        }
        const bool self = p.channel == SM_CH_LC;
        const size_t nl = (size_t)p.w * p.h;
        float *low, *tmp, *q = big;
        if ((rc = pool_get(ctx, P_TMP, 8 * nl * 4, &low)) || (rc = pool_get(ctx, P_LIN, 8 * nl * 4, &tmp))) return rc;
        if (!self) { for (int k = 0; k < 3; ++k) { a.in[k] = q; q += nw; } a.guide = q; q += nw; }
        for (int k = 0; k < 3; ++k) { a.chan[k] = q; q += nw; }
        if (p.iterations > 1) for (int k = 0; k < 3; ++k) { a.work[k] = q; q += nw; }
        a.w = p.w; a.h = p.h; a.epsilon = p.epsilon; a.low = low;
        for (int k = 0; k < 3; ++k) { a.a[k] = self ? low + (2 * k) * nl : low + (2 + k) * nl; a.b[k] = self ? low + (2 * k + 1) * nl : low + (5 + k) * nl; }
        GuidedArgs g = {};
        g.W = p.ww; g.H = p.hh; g.w = p.w; g.h = p.h; g.epsilon = p.epsilon; g.guide = a.guide;
        for (int k = 0; k < 3; ++k) g.chan[k] = a.chan[k];
        for (int k = 0; k < 8; ++k) g.low[k] = low + k * nl;
        for (int it = 0; it < p.iterations; ++it) {
            for (int k = 0; k < 3; ++k) a.src[k] = it == 0 ? a.img[k] : a.work[k];
            a.src_stride = it == 0 ? stride : (size_t)p.ww;
            a.src_norm = it == 0 && norm_in ? 1 : 0;
            a.last = it == p.iterations - 1;
            HIPCHK(ctx, launch_sm_prepare(a, ctx->stream));
            if (self) {
                HIPCHK(ctx, launch_sm_subsample_self(a, ctx->stream));
                if ((rc = box_blur_planes(ctx, low, tmp, 6, nl, p.w, p.h, p.rad))) return rc;        // mean I, corr I per channel
                HIPCHK(ctx, launch_sm_ab_self(a, ctx->stream));
                if ((rc = box_blur_planes(ctx, low, tmp, 6, nl, p.w, p.h, p.rad))) return rc;        // mean a, mean b per channel
            } else {
                HIPCHK(ctx, launch_gf_subsample(g, ctx->stream));
                if ((rc = box_blur_planes(ctx, low, tmp, 8, nl, p.w, p.h, p.rad))) return rc;        // meanI, corrI, meanp[3], corrIp[3]
                HIPCHK(ctx, launch_gf_ab(g, ctx->stream));
                if ((rc = box_blur_planes(ctx, low + 2 * nl, tmp, 6, nl, p.w, p.h, p.rad))) return rc;   // mean a[3], mean b[3]
            }
            HIPCHK(ctx, launch_sm_finish(a, ctx->stream));
        }
        return ARTGPU_OK;
    }
    // NLMEANS
    float *q = big;
    const int nplanes = p.channel == SM_CH_L ? 1 : 3;
    if (!(p.skipped && p.channel == SM_CH_LC)) {
        for (int k = 0; k < nplanes; ++k) { a.work[k] = q; q += nw; }
        if (p.channel == SM_CH_C) a.in[0] = q;
        HIPCHK(ctx, launch_sm_nlm_split(a, ctx->stream));
        if (!p.skipped)
            for (int it = 0; it < p.iterations; ++it)
                for (int k = 0; k < nplanes; ++k)
                    if ((rc = nlm_plane_dev(ctx, a.work[k], p.ww, p.hh, 1.f, p.nlstrength, p.nldetail, (float)scale))) return rc;
    }
    HIPCHK(ctx, launch_sm_nlm_merge(a, ctx->stream));
    return ARTGPU_OK;
}

} // namespace

namespace artgpu { namespace api {

// everything that does not depend on a mask's box: what the pipe checks before any stage runs
int sm_check(artgpu_ctx *ctx, int W, int H, const artgpu_smoothing_region *regions, int nregions, const double *ws, double scale, bool read_masks, const char *who)
{
    if (nregions < 0 || (nregions > 0 && !regions) || !ws || !(scale > 0.0) || std::isinf(scale)) return fail(ctx, ARTGPU_EINVAL, "%s: bad arguments", who);
    for (int i = 0; i < nregions; ++i) {
        const artgpu_smoothing_region &r = regions[i];
        if (r.mode < ARTGPU_SMOOTHING_GUIDED || r.mode > ARTGPU_SMOOTHING_WAVELETS) return fail(ctx, ARTGPU_EINVAL, "%s: region %d: mode %d", who, i, r.mode);
        if (r.channel < ARTGPU_SMOOTHING_LUMINANCE || r.channel > ARTGPU_SMOOTHING_RGB) return fail(ctx, ARTGPU_EINVAL, "%s: region %d: channel %d", who, i, r.channel);
        if (r.mode != ARTGPU_SMOOTHING_GUIDED && r.mode != ARTGPU_SMOOTHING_NLMEANS)
            return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: mode %d is not on the device path (only GUIDED and NLMEANS are)", who, i, r.mode);
        if (r.iterations < 1) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: iterations %d", who, i, r.iterations);
        if (r.mode == ARTGPU_SMOOTHING_NLMEANS && r.nlstrength != 0 && !(scale >= 1.0))
            return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: NL-means at scale %g (below 1) is not on the device path", who, i, scale);
        if (read_masks && r.mask && (!plane_ok(r.mask) || r.mask->w != W || r.mask->h != H)) return fail(ctx, ARTGPU_EINVAL, "%s: region %d: the mask must be a %dx%d plane", who, i, W, H);
    }
    return ARTGPU_OK;
}

// one region's plan from its box (inclusive maxima as the reduction leaves them; nullptr: a NULL mask, the frame)
int sm_plan_region(artgpu_ctx *ctx, int W, int H, const artgpu_smoothing_region &r, const int *box, double scale, const char *who, int i, SmRegionPlan *pl)
{
    *pl = SmRegionPlan{};
    pl->mode = r.mode; pl->channel = r.channel; pl->iterations = r.iterations; pl->nlstrength = r.nlstrength; pl->nldetail = r.nldetail;
    if (box && box[2] < box[0]) { pl->skipped = ARTGPU_SMOOTHING_SKIP_EMPTY; return ARTGPU_OK; }
    int min_x = box ? box[0] : 0, min_y = box ? box[1] : 0, max_x = box ? box[2] + 1 : W, max_y = box ? box[3] + 1 : H;
    int ww = max_x - min_x, hh = max_y - min_y;
    if (ww * hh < (W * H) / 2) pl->cropped = 1;                    // L957 (int arithmetic, as there)
    else { min_x = 0; min_y = 0; max_x = W; max_y = H; ww = W; hh = H; }
    pl->x0 = min_x; pl->y0 = min_y; pl->x1 = max_x; pl->y1 = max_y; pl->ww = ww; pl->hh = hh;
    if (r.mode == ARTGPU_SMOOTHING_GUIDED) {
        pl->epsilon = (float)std::max(0.001f * std::pow(2.0, (double)-r.epsilon), 1e-6);        // L1040: a double narrowed at the call
        const int rr = (int)std::round(r.radius / scale);             // L348
        pl->r = rr > 0 ? rr : 0;
        if (pl->r == 0) { pl->skipped = ARTGPU_SMOOTHING_SKIP_RADIUS; return ARTGPU_OK; }
        const GfGrid grid = gf_grid(ww, hh, pl->r);                   // calculate_subsampling, f_mean (guidedfilter.cc:58-75, 160-167)
        pl->sub = grid.sub; pl->w = grid.w; pl->h = grid.h;
        if (pl->w < ARTGPU_SMOOTHING_MIN_SIZE || pl->h < ARTGPU_SMOOTHING_MIN_SIZE)
            return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: a %dx%d working plane leaves a %dx%d statistics grid, below %d", who, i, ww, hh, pl->w, pl->h, ARTGPU_SMOOTHING_MIN_SIZE);
        pl->rad = grid.rad;
        if (pl->rad > HBLUR_MAX_RADIUS)
            return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: box radius %d (r / subsampling) is above the %d the blur kernels hold in LDS", who, i, pl->rad, HBLUR_MAX_RADIUS);
    } else {
        if (r.nlstrength == 0) { pl->skipped = ARTGPU_SMOOTHING_SKIP_STRENGTH; return ARTGPU_OK; }
        if (ww < 32 || hh < 32) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: NL-means on a %dx%d working plane, smaller than 32x32", who, i, ww, hh);
        if ((unsigned long long)(ww + 14) * (unsigned long long)(hh + 14) >= (1ull << 30))
            return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: region %d: NL-means on a %dx%d working plane exceeds 2^30 pixels", who, i, ww, hh);
    }
    return ARTGPU_OK;
}

// the tool on device planes (rows of `stride` floats) in RGB mode; enqueued on ctx->stream, one host wait when a region has a mask
int smoothing_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const artgpu_smoothing_region *regions, int n, const double *ws, double scale,
                  artgpu_smoothing_info *info, const char *who)
{
    int rc;
    const size_t np = (size_t)W * H;
    // host planes are staged once each (several regions may share one)
    std::vector<const artgpu_plane *> host;
    for (int i = 0; i < n; ++i) {
        const artgpu_plane *m = regions[i].mask;
        if (m && !m->on_device && std::find_if(host.begin(), host.end(), [m](const artgpu_plane *q) { return q->p == m->p; }) == host.end()) host.push_back(m);
    }
    float *staged = nullptr;
    if (!host.empty()) {
        if ((rc = pool_get(ctx, P_SM_MASK, host.size() * np * 4, &staged))) return rc;
        for (size_t k = 0; k < host.size(); ++k)
            HIPCHK(ctx, hipMemcpy2DAsync(staged + k * np, (size_t)W * 4, host[k]->p, (size_t)host[k]->row_stride_bytes, (size_t)W * 4, H, hipMemcpyHostToDevice, ctx->stream));
    }
    std::vector<const float *> mp(n, nullptr);
    std::vector<size_t> ms(n, 0);
    std::vector<int> masked;
    for (int i = 0; i < n; ++i) {
        const artgpu_plane *m = regions[i].mask;
        if (!m) continue;
        if (m->on_device) { mp[i] = m->p; ms[i] = (size_t)(m->row_stride_bytes / 4); }
        else { mp[i] = staged + (std::find_if(host.begin(), host.end(), [m](const artgpu_plane *q) { return q->p == m->p; }) - host.begin()) * np; ms[i] = W; }
        masked.push_back(i);
    }
    // find_region of every mask: one pass (SM_MAX_BOX_REGIONS planes per launch), one wait for 4 ints per mask
    std::vector<int> boxes(4 * masked.size());
    if (!masked.empty()) {
        for (size_t k = 0; k < masked.size(); ++k) { boxes[4 * k] = W; boxes[4 * k + 1] = H; boxes[4 * k + 2] = -1; boxes[4 * k + 3] = -1; }
        float *bx;
        if ((rc = pool_get(ctx, P_SM_BOX, boxes.size() * 4, &bx))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(bx, boxes.data(), boxes.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        for (size_t k0 = 0; k0 < masked.size(); k0 += SM_MAX_BOX_REGIONS) {
            SmBoxArgs b = {};
            b.n = (int)std::min(masked.size() - k0, (size_t)SM_MAX_BOX_REGIONS); b.W = W; b.H = H; b.box = reinterpret_cast<int *>(bx) + 4 * k0;
            for (int k = 0; k < b.n; ++k) { b.mask[k] = mp[masked[k0 + k]]; b.stride[k] = ms[masked[k0 + k]]; }
            HIPCHK(ctx, launch_sm_box(b, ctx->stream));
        }
        HIPCHK(ctx, hipMemcpyAsync(boxes.data(), bx, boxes.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    // the whole plan, before any kernel writes the image
    std::vector<SmRegionPlan> plans(n);
    size_t need = 0;
    for (int i = 0, k = 0; i < n; ++i) {
        if ((rc = sm_plan_region(ctx, W, H, regions[i], regions[i].mask ? &boxes[4 * k++] : nullptr, scale, who, i, &plans[i]))) return rc;
        need = std::max(need, sm_region_floats(plans[i]));
    }
    float *big = nullptr;
    if (need && (rc = pool_get(ctx, P_SM_PLANES, need * 4, &big))) return rc;
    int first = -1, last = -1;
    for (int i = 0; i < n; ++i)
        if (plans[i].skipped != ARTGPU_SMOOTHING_SKIP_EMPTY) { if (first < 0) first = i; last = i; }
    if (first < 0) {
        HIPCHK(ctx, launch_sm_scale(planes, stride, W, H, 2, ctx->stream));        // normalizeFloatTo1, normalizeFloatTo65535 (L938, L1067)
    } else {
        // a full-frame region at either end takes that end's normalise pass into its own passes (every pixel still sees exactly one of each)
        const bool fuse_in = !plans[first].cropped, fuse_out = !plans[last].cropped;
        if (!fuse_in) HIPCHK(ctx, launch_sm_scale(planes, stride, W, H, 0, ctx->stream));
        for (int i = 0; i < n; ++i)
            if (plans[i].skipped != ARTGPU_SMOOTHING_SKIP_EMPTY &&
                (rc = sm_region_dev(ctx, planes, stride, plans[i], mp[i], ms[i], ws, scale, big, fuse_in && i == first, fuse_out && i == last)))
                return rc;
        if (!fuse_out) HIPCHK(ctx, launch_sm_scale(planes, stride, W, H, 1, ctx->stream));
    }
    if (info)
        for (int i = 0; i < n; ++i) {
            const SmRegionPlan &p = plans[i];
            artgpu_smoothing_info &o = info[i];
            o = artgpu_smoothing_info{};
            o.r = p.r; o.epsilon = p.epsilon; o.min_x = p.x0; o.min_y = p.y0; o.max_x = p.x1; o.max_y = p.y1; o.cropped = p.cropped; o.work_w = p.ww; o.work_h = p.hh;
            o.subsampling = p.sub; o.box_radius = p.rad; o.skipped = p.skipped;
        }
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_smoothing(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_smoothing_region *regions, int nregions, const double ws[9], double scale,
                     artgpu_smoothing_info *info)
{
    StageScope scope_(ctx, "ImProcFunctions::guidedSmoothing");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !plane_ok(&img->r)) return fail(ctx, ARTGPU_EINVAL, "smoothing: bad image");
    int rc;
    if ((rc = sm_check(ctx, img->r.w, img->r.h, regions, nregions, ws, scale, true, "smoothing"))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "smoothing"))) return rc;
    if ((rc = smoothing_dev(ctx, d.p, d.stride, d.w, d.h, regions, nregions, ws, scale, info, "smoothing"))) return rc;
    return unbind_rgb(ctx, img, &d);
}

} // extern "C"

// ---------------------------------------------------------------------------------------------
// capture sharpening: ImProcFunctions::doSharpening, method "rld"
// ---------------------------------------------------------------------------------------------

namespace {

constexpr size_t SH_COUNTER_BYTES = 64;      // P_SH_BYTES: two 64-bit counters, then the impulse map

static bool sharpen_sigma_ok(double sigma) { return sigma == sigma && !std::isinf(sigma) && sigma < 25.0; }

// deconvsharpening on a contiguous device plane; `work`: five planes (estimate x 2, ratio, out, the gaussian's forward buffer).
// counters (device, zeroed; may be null): [1] += the pixels frozen before the last iteration.  *early / *regime for artgpu_sharpening_info.
static int rl_dev(artgpu_ctx *ctx, float *lum, const float *blend, const unsigned char *impulse, int W, int H, double sigma, float amount, float *work,
                  unsigned long long *counters, int *early, int *regime)
{
    *regime = -1; *early = 0;
    if (amount <= 0) { *early = 4; return ARTGPU_OK; }                               // L146-148
    if (sigma < 0.2f) { *early = 5; return ARTGPU_OK; }                              // L154-156
    const size_t n = (size_t)W * H;
    ShRlArgs a = {};
    const int rg = sh_regime(sigma, &a.k);
    *regime = rg;
    float *est = work, *other = work + n, *ratio = work + 2 * n, *out = work + 3 * n, *gtmp = work + 4 * n;
    a.ratio = ratio; a.lum = lum; a.blend = blend; a.impulse = impulse; a.out = out; a.W = W; a.H = H; a.amount = amount;
    int rc;
    HIPCHK(ctx, launch_rl_init(lum, est, out, W, H, ctx->stream));
    for (int it = 0; it < 20; ++it) {
        if (rg == SH_COPY) {
            // gaussianBlur copies whatever the type: the estimate never changes, and neither does check_stop's verdict after the first iteration
            if (it == 0) { a.est_in = est; a.est_out = est; HIPCHK(ctx, launch_rl_point(a, 0, ctx->stream)); }
        } else if (rg == SH_YVV) {
            HIPCHK(ctx, hipMemcpyAsync(ratio, est, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
            if ((rc = gaussian_dev(ctx, ratio, gtmp, W, H, sigma))) return rc;
            HIPCHK(ctx, launch_yvv_div(ratio, lum, W, H, ctx->stream));
            if ((rc = gaussian_dev(ctx, ratio, gtmp, W, H, sigma))) return rc;
            a.est_in = est; a.est_out = est;
            HIPCHK(ctx, launch_rl_point(a, 1, ctx->stream));
        } else if (ctx->shared.opt_sharpen_fused) {
            a.est_in = est; a.est_out = other;
            HIPCHK(ctx, launch_rl_iter(a, rg, ctx->stream));
            std::swap(est, other);
        } else {
            HIPCHK(ctx, launch_gauss_div(est, ratio, lum, W, H, rg, a.k, ctx->stream));
            HIPCHK(ctx, launch_gauss_mult(ratio, est, W, H, rg, a.k, ctx->stream));
            a.est_in = est; a.est_out = est;
            HIPCHK(ctx, launch_rl_point(a, 0, ctx->stream));
        }
        if (it == 18 && counters) HIPCHK(ctx, launch_sh_count(nullptr, out, n, counters, ctx->stream));
    }
    HIPCHK(ctx, launch_rl_final(lum, est, out, blend, impulse, amount, W, H, ctx->stream));
    return ARTGPU_OK;
}

static int sharpen_scratch(artgpu_ctx *ctx, size_t n, int nplanes, float **planes, unsigned long long **counters, unsigned char **impulse)
{
    float *bytes;
    int rc;
    if ((rc = pool_get(ctx, P_SH_PLANES, (size_t)nplanes * n * 4, planes)) || (rc = pool_get(ctx, P_SH_BYTES, SH_COUNTER_BYTES + n, &bytes))) return rc;
    *counters = reinterpret_cast<unsigned long long *>(bytes);
    *impulse = reinterpret_cast<unsigned char *>(bytes) + SH_COUNTER_BYTES;
    return ARTGPU_OK;
}

static int sharpen_read_counters(artgpu_ctx *ctx, const unsigned long long *counters, artgpu_sharpening_info *info)
{
    unsigned long long host[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(host, counters, sizeof host, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    info->impulse_pixels = (int64_t)host[0];
    info->frozen_pixels = (int64_t)host[1];
    return ARTGPU_OK;
}

} // namespace

namespace artgpu { namespace api {

int sharpen_check(artgpu_ctx *ctx, int W, int H, const artgpu_sharpening_params *p, double scale, const char *who, SharpenPlan *pl)
{
    *pl = SharpenPlan{};
    if (!p->enabled) { pl->early = 1; return ARTGPU_OK; }
    if (p->amount < 1) { pl->early = 2; return ARTGPU_OK; }
    if (W < 8 || H < 8) { pl->early = 3; return ARTGPU_OK; }
    if (p->method != ARTGPU_SHARPEN_RLD) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: only the rld method is on the device path (method %d)", who, p->method);
    if (!(scale > 0.0) || std::isinf(scale)) return fail(ctx, ARTGPU_EINVAL, "%s: scale must be positive", who);
    const float s_scale = std::sqrt(scale);                                          // L726-729
    pl->contrast = sh_pow_F(p->contrast / 100.f, 1.2f) * s_scale;
    pl->blur_radius = 2.f / s_scale;
    if (!(pl->blur_radius >= 0.6)) return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: mask blur radius %g (scale %g) below the shared gaussian's range", who, (double)pl->blur_radius, scale);
    pl->sigma = p->deconvradius / scale;                                             // L756-759
    pl->amount = p->deconvamount / 100.f;
    pl->delta = p->deconvCornerBoost / scale;
    pl->boost = pl->delta > 0.01f ? 1 : 0;
    if (!sharpen_sigma_ok(pl->sigma) || (pl->boost && !sharpen_sigma_ok(pl->sigma + pl->delta)))
        return fail(ctx, ARTGPU_EUNSUPPORTED, "%s: deconvolution radius %g (corner boost %g) is not finite or not below 25", who, pl->sigma, (double)pl->delta);
    return ARTGPU_OK;
}

// doSharpening on device planes (rows of `stride` floats), enqueued on ctx->stream; the host waits only to fill `info`
int sharpen_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const artgpu_sharpening_params *p, const double ws[9],
                       const SharpenPlan &pl, artgpu_sharpening_info *info)
{
    if (info) { info->early_out = pl.early; info->regime = -1; }
    if (pl.early) return ARTGPU_OK;
    const size_t n = (size_t)W * H;
    float *sp;
    unsigned long long *counters;
    unsigned char *impulse;
    int rc;
    if ((rc = sharpen_scratch(ctx, n, pl.boost ? SHP_NPLANES : SHP_NPLANES - 1, &sp, &counters, &impulse))) return rc;
    float *Y = sp + SHP_Y * n, *blend = sp + SHP_BLEND * n, *YY = sp + SHP_YY * n, *lpf = sp + SHP_RATIO * n, *gtmp = sp + SHP_GTMP * n;
    ShImage im = {{planes[0], planes[1], planes[2]}, stride, W, H};
    const float ws1[3] = {(float)ws[3], (float)ws[4], (float)ws[5]};                 // TMatrix is float (iccstore.h:38)
    HIPCHK(ctx, launch_sh_luminance(im, ws1, Y, ctx->stream));
    // buildBlendMask(Y, blend, W, H, contrast, 1.f, false, 2.f / s_scale) (rt_algo.cc:416-494)
    DualArgs da = {};
    da.L = Y; da.blend = blend; da.w = W; da.h = H; da.threshold = pl.contrast;
    HIPCHK(ctx, launch_blend_mask(da, ctx->stream));
    if (pl.contrast != 0.f && (rc = gaussian_dev(ctx, blend, gtmp, W, H, pl.blur_radius))) return rc;
    // markImpulse(W, H, Y, impulse, 2.f): the low-pass is gaussianBlur(src, lpf, max(2.f, thresh - 1.f))
    HIPCHK(ctx, hipMemcpyAsync(lpf, Y, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if ((rc = gaussian_dev(ctx, lpf, gtmp, W, H, std::max(2.f, 2.f - 1.f)))) return rc;
    HIPCHK(ctx, launch_sh_impulse(Y, lpf, impulse, W, H, 2.f, ctx->stream));
    if (info) {
        HIPCHK(ctx, hipMemsetAsync(counters, 0, SH_COUNTER_BYTES, ctx->stream));
        HIPCHK(ctx, launch_sh_count(impulse, nullptr, n, counters, ctx->stream));
    }
    HIPCHK(ctx, hipMemcpyAsync(YY, Y, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    int early = 0, regime = -1;
    if ((rc = rl_dev(ctx, YY, blend, impulse, W, H, pl.sigma, pl.amount, sp + SHP_EST_A * n, info ? counters : nullptr, &early, &regime))) return rc;
    if (pl.boost) {
        float *YY2 = sp + SHP_YY2 * n;
        int e2, r2;
        HIPCHK(ctx, hipMemcpyAsync(YY2, Y, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
        if ((rc = rl_dev(ctx, YY2, blend, impulse, W, H, pl.sigma + pl.delta, pl.amount, sp + SHP_EST_A * n, nullptr, &e2, &r2))) return rc;
        const int fw = p->full_width > 0 ? p->full_width : W, fh = p->full_height > 0 ? p->full_height : H;
        ShCornerArgs ca = {};
        ca.YY = YY; ca.YY2 = YY2; ca.W = W; ca.H = H; ca.ox = p->offset_x; ca.oy = p->offset_y; ca.w2 = fw / 2; ca.h2 = fh / 2;
        const float radius = std::max(ca.w2, ca.h2);                                 // CornerBoostMask (L317-323)
        const float lat = float(p->deconvCornerLatitude) / 150.f;
        ca.r2 = (radius - radius * std::max(0.f, std::min(lat, 1.f))) / 2.f;
        ca.sigma = 2.f * ((radius * 0.3f) * (radius * 0.3f));
        HIPCHK(ctx, launch_sh_corner(ca, ctx->stream));
    }
    HIPCHK(ctx, launch_sh_multiply(im, YY, Y, ctx->stream));
    if (info) {
        info->sigma = pl.sigma; info->regime = regime; info->early_out = early; info->contrast_threshold = pl.contrast;
        if ((rc = sharpen_read_counters(ctx, counters, info))) return rc;
    }
    return ARTGPU_OK;
}

int plane_into(artgpu_ctx *ctx, const artgpu_plane *pl, float *dst)
{
    const size_t rowb = (size_t)pl->w * 4;
    HIPCHK(ctx, hipMemcpy2DAsync(dst, rowb, pl->p, (size_t)pl->row_stride_bytes, rowb, pl->h, pl->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    return ARTGPU_OK;
}

// calcRadiusBayer's maximum of a device CFA plane into result[0] (P_SH_STATE), enqueued; no wait
int auto_radius_dev(artgpu_ctx *ctx, const float *raw, size_t stride, int W, int H, uint32_t filters, float lower, float upper, float **result)
{
    float *st;
    int rc;
    if ((rc = pool_get(ctx, P_SH_STATE, (SH_RADIUS_PARTIALS + 16) * 4, &st))) return rc;
    const auto FC = [&](unsigned row, unsigned col) { return (filters >> ((((row << 1) & 14u) + (col & 1u)) << 1)) & 3u; };
    const unsigned fc0 = filters ? FC(0, 0) : 0u, fc1 = filters ? FC(1, 0) : 0u;     // deconvautoradius.cc:207, 240
    HIPCHK(ctx, launch_sh_radius(raw, stride, W, H, fc0, fc1, lower, upper, st + 16, st, ctx->stream));
    *result = st;
    return ARTGPU_OK;
}

float auto_radius_of(float maxRatio) { return std::sqrt((1.f / (std::log(1.f / maxRatio) / 2.f)) / -2.f); }   // L90

} } // namespace artgpu::api

extern "C" {

int artgpu_sharpening(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_sharpening_params *params, const double ws[9], double scale, artgpu_sharpening_info *info)
{
    StageScope scope_(ctx, "ImProcFunctions::sharpening");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !params || !ws) return fail(ctx, ARTGPU_EINVAL, "sharpening: null argument");
    if (info) { *info = artgpu_sharpening_info{}; info->regime = -1; }
    if (!plane_ok(&img->r)) return fail(ctx, ARTGPU_EINVAL, "sharpening: bad plane");
    SharpenPlan pl;
    int rc;
    if ((rc = sharpen_check(ctx, img->r.w, img->r.h, params, scale, "sharpening", &pl))) return rc;
    if (pl.early) { if (info) info->early_out = pl.early; return ARTGPU_OK; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "sharpening"))) return rc;
    if ((rc = sharpen_dev(ctx, d.p, d.stride, d.w, d.h, params, ws, pl, info))) return rc;
    return unbind_rgb(ctx, img, &d);
}

int artgpu_rl_deconvolution(artgpu_ctx *ctx, artgpu_plane *luminance, const artgpu_plane *blend, const uint8_t *impulse, double sigma, float amount,
                            artgpu_sharpening_info *info)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(luminance) || !plane_ok(blend) || !impulse || blend->w != luminance->w || blend->h != luminance->h)
        return fail(ctx, ARTGPU_EINVAL, "rl_deconvolution: bad planes");
    if (info) { *info = artgpu_sharpening_info{}; info->regime = -1; info->sigma = sigma; }
    if (amount <= 0) { if (info) info->early_out = 4; return ARTGPU_OK; }
    if (sigma < 0.2f) { if (info) info->early_out = 5; return ARTGPU_OK; }
    if (!sharpen_sigma_ok(sigma)) return fail(ctx, ARTGPU_EUNSUPPORTED, "rl_deconvolution: sigma %g is not finite or not below 25", sigma);
    const int W = luminance->w, H = luminance->h;
    if (W < 8 || H < 8) return fail(ctx, ARTGPU_EUNSUPPORTED, "rl_deconvolution: plane smaller than 8x8");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H;
    float *sp;
    unsigned long long *counters;
    unsigned char *imp;
    int rc;
    if ((rc = sharpen_scratch(ctx, n, SHP_NPLANES - 1, &sp, &counters, &imp))) return rc;
    float *lum = sp + SHP_YY * n, *bl = sp + SHP_BLEND * n;
    if ((rc = plane_into(ctx, luminance, lum)) || (rc = plane_into(ctx, blend, bl))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(imp, impulse, n, luminance->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    if (info) {
        HIPCHK(ctx, hipMemsetAsync(counters, 0, SH_COUNTER_BYTES, ctx->stream));
        HIPCHK(ctx, launch_sh_count(imp, nullptr, n, counters, ctx->stream));
    }
    int early, regime;
    if ((rc = rl_dev(ctx, lum, bl, imp, W, H, sigma, amount, sp + SHP_EST_A * n, info ? counters : nullptr, &early, &regime))) return rc;
    if (info) {
        info->regime = regime; info->early_out = early;
        if ((rc = sharpen_read_counters(ctx, counters, info))) return rc;
    }
    return pool_to_plane(ctx, lum, luminance);
}

int artgpu_gaussian_blur_ex(artgpu_ctx *ctx, artgpu_plane *src, artgpu_plane *dst, const artgpu_plane *div, double sigma, int gausstype)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(src) || !plane_ok(dst) || dst->w != src->w || dst->h != src->h || src->p == dst->p) return fail(ctx, ARTGPU_EINVAL, "gaussian_blur_ex: bad planes (src != dst)");
    if (gausstype != ARTGPU_GAUSS_MULT && gausstype != ARTGPU_GAUSS_DIV)
        return fail(ctx, ARTGPU_EUNSUPPORTED, "gaussian_blur_ex: GAUSS_MULT or GAUSS_DIV (GAUSS_STANDARD: artgpu_gaussian_blur)");
    const bool is_div = gausstype == ARTGPU_GAUSS_DIV;
    if (is_div && (!plane_ok(div) || div->w != src->w || div->h != src->h)) return fail(ctx, ARTGPU_EINVAL, "gaussian_blur_ex: GAUSS_DIV needs the divisor plane");
    if (!sharpen_sigma_ok(sigma)) return fail(ctx, ARTGPU_EUNSUPPORTED, "gaussian_blur_ex: sigma %g is not finite or not below 25", sigma);
    const int W = src->w, H = src->h;
    if (W < 8 || H < 8) return fail(ctx, ARTGPU_EUNSUPPORTED, "gaussian_blur_ex: plane smaller than 8x8");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H;
    float *sp;
    int rc;
    if ((rc = pool_get(ctx, P_SH_PLANES, 4 * n * 4, &sp))) return rc;
    float *s = sp, *d = sp + n, *v = sp + 2 * n, *gtmp = sp + 3 * n;
    if ((rc = plane_into(ctx, src, s))) return rc;
    ShCoef k;
    const int rg = sh_regime(sigma, &k);
    if (rg == SH_COPY) return pool_to_plane(ctx, s, dst);                            // GAUSS_SKIP ignores the type (gauss.cc:1437-1443)
    if (is_div) { if ((rc = plane_into(ctx, div, v))) return rc; }
    else if ((rc = plane_into(ctx, dst, d))) return rc;
    if (rg == SH_YVV) {
        if ((rc = gaussian_dev(ctx, s, gtmp, W, H, sigma))) return rc;
        if (is_div) { HIPCHK(ctx, launch_yvv_div(s, v, W, H, ctx->stream)); return pool_to_plane(ctx, s, dst); }
        HIPCHK(ctx, launch_yvv_mult(s, d, W, H, ctx->stream));
        if ((rc = pool_to_plane(ctx, s, src))) return rc;                            // the reference filters src in place here
        return pool_to_plane(ctx, d, dst);
    }
    if (is_div) HIPCHK(ctx, launch_gauss_div(s, d, v, W, H, rg, k, ctx->stream));
    else HIPCHK(ctx, launch_gauss_mult(s, d, W, H, rg, k, ctx->stream));
    return pool_to_plane(ctx, d, dst);
}

int artgpu_deconv_auto_radius(artgpu_ctx *ctx, const artgpu_plane *raw, uint32_t filters, float lower_limit, float clip_val, float *radius, float *max_ratio)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (!plane_ok(raw) || !radius) return fail(ctx, ARTGPU_EINVAL, "deconv_auto_radius: bad argument");
    if (filters == 9) return fail(ctx, ARTGPU_EUNSUPPORTED, "deconv_auto_radius: X-Trans (calcRadiusXtrans) is not on the device path");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const float *dev = raw->p;
    size_t stride = (size_t)(raw->row_stride_bytes / 4);
    int rc;
    if (!raw->on_device) {
        float *cp;
        if ((rc = plane_to_pool(ctx, raw, P_SH_PLANES, &cp))) return rc;
        dev = cp; stride = raw->w;
    }
    float *res;
    if ((rc = auto_radius_dev(ctx, dev, stride, raw->w, raw->h, filters, lower_limit, clip_val, &res))) return rc;
    float mr = 1.f;
    HIPCHK(ctx, hipMemcpyAsync(&mr, res, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (max_ratio) *max_ratio = mr;
    *radius = auto_radius_of(mr);
    return ARTGPU_OK;
}

} // extern "C"
