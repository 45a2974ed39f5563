// art_amd/csrc/artgpu_api.hip -- the C ABI of libartgpu.so (include/artgpu.h): the context and what every stage's host file takes from it
// (errors, device buffers, staging for host-pointer calls, the scratch pool, constant tables), the test hooks for device primitives, and the
// seven tools that have no file of their own yet: raw CA correction, local contrast, dehaze, texture boost, masks, smoothing, capture
// sharpening.  The other stages are one api_<stage>.hip each (api_internal.h lists them).
// There is no CPU fallback here: every entry point either runs the HIP kernels or fails.
#include "api_internal.h"

using namespace artgpu;
using namespace artgpu::api;

namespace {

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
    else if (n == "fg_grid") { if (value < 0 || value > 65536) return fail(ctx, ARTGPU_EINVAL, "fg_grid: 0 (default) .. 65536 workgroups"); ctx->shared.opt_fg_grid = (int)value; }
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

// the working area of a region from its box (inclusive maxima as the reduction leaves them; nullptr: a NULL mask, the frame), L948-980: the
// box, or the frame unless the box is under half of it.  false: no mask pixel above zero, skipped = ARTGPU_SMOOTHING_SKIP_EMPTY
bool sm_working_area(int W, int H, const int *box, SmRegionPlan *pl)
{
    if (box && box[2] < box[0]) { pl->skipped = ARTGPU_SMOOTHING_SKIP_EMPTY; return false; }
    int min_x = box ? box[0] : 0, min_y = box ? box[1] : 0, max_x = box ? box[2] + 1 : W, max_y = box ? box[3] + 1 : H;
    int ww = max_x - min_x, hh = max_y - min_y;
    if (ww * hh < (W * H) / 2) pl->cropped = 1;                    // L957 (int arithmetic, as there)
    else { min_x = 0; min_y = 0; max_x = W; max_y = H; ww = W; hh = H; }
    pl->x0 = min_x; pl->y0 = min_y; pl->x1 = max_x; pl->y1 = max_y; pl->ww = ww; pl->hh = hh;
    return true;
}

// one region's plan from its box
int sm_plan_region(artgpu_ctx *ctx, int W, int H, const artgpu_smoothing_region &r, const int *box, double scale, const char *who, int i, SmRegionPlan *pl)
{
    *pl = SmRegionPlan{};
    pl->mode = r.mode; pl->channel = r.channel; pl->iterations = r.iterations; pl->nlstrength = r.nlstrength; pl->nldetail = r.nldetail;
    if (!sm_working_area(W, H, box, pl)) return ARTGPU_OK;
    const int ww = pl->ww, hh = pl->hh;
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

// The blend planes of a call's regions on the device and find_region (L411-434) of each: host planes are staged (P_SM_MASK), every mask's box
// comes from one pass (SM_MAX_BOX_REGIONS planes per launch) and one host wait for 4 ints per mask.  mp / ms: per region the plane and its row
// stride in floats (nullptr: all ones); boxes: 4 ints per region that has a mask, in region order
int sm_mask_boxes(artgpu_ctx *ctx, int W, int H, const artgpu_plane *const *masks, int n, std::vector<const float *> *mp_out, std::vector<size_t> *ms_out,
                  std::vector<int> *boxes_out)
{
    int rc;
    const size_t np = (size_t)W * H;
    // host planes are staged once each (several regions may share one)
    std::vector<const artgpu_plane *> host;
    for (int i = 0; i < n; ++i) {
        const artgpu_plane *m = masks[i];
        if (m && !m->on_device && std::find_if(host.begin(), host.end(), [m](const artgpu_plane *q) { return q->p == m->p; }) == host.end()) host.push_back(m);
    }
    float *staged = nullptr;
    if (!host.empty()) {
        if ((rc = pool_get(ctx, P_SM_MASK, host.size() * np * 4, &staged))) return rc;
        for (size_t k = 0; k < host.size(); ++k)
            HIPCHK(ctx, hipMemcpy2DAsync(staged + k * np, (size_t)W * 4, host[k]->p, (size_t)host[k]->row_stride_bytes, (size_t)W * 4, H, hipMemcpyHostToDevice, ctx->stream));
    }
    std::vector<const float *> &mp = *mp_out;
    std::vector<size_t> &ms = *ms_out;
    std::vector<int> &boxes = *boxes_out;
    mp.assign(n, nullptr); ms.assign(n, 0);
    std::vector<int> masked;
    for (int i = 0; i < n; ++i) {
        const artgpu_plane *m = masks[i];
        if (!m) continue;
        if (m->on_device) { mp[i] = m->p; ms[i] = (size_t)(m->row_stride_bytes / 4); }
        else { mp[i] = staged + (std::find_if(host.begin(), host.end(), [m](const artgpu_plane *q) { return q->p == m->p; }) - host.begin()) * np; ms[i] = W; }
        masked.push_back(i);
    }
    // find_region of every mask: one pass (SM_MAX_BOX_REGIONS planes per launch), one wait for 4 ints per mask
    boxes.assign(4 * masked.size(), 0);
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
    return ARTGPU_OK;
}

// the tool on device planes (rows of `stride` floats) in RGB mode; enqueued on ctx->stream, one host wait when a region has a mask
int smoothing_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const artgpu_smoothing_region *regions, int n, const double *ws, double scale,
                  artgpu_smoothing_info *info, const char *who)
{
    int rc;
    std::vector<const artgpu_plane *> masks(n);
    for (int i = 0; i < n; ++i) masks[i] = regions[i].mask;
    std::vector<const float *> mp;
    std::vector<size_t> ms;
    std::vector<int> boxes;
    if ((rc = sm_mask_boxes(ctx, W, H, masks.data(), n, &mp, &ms, &boxes))) return rc;
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
