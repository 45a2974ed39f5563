// art_amd/csrc/artgpu_api.hip -- the C ABI of libartgpu.so (include/artgpu.h): the context and what every stage's host file takes from it
// (errors, device buffers, staging for host-pointer calls, the scratch pool, constant tables) and the test hooks for device primitives.
// Every stage is one api_<stage>.hip (api_internal.h lists them).
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
int bind_images(artgpu_ctx *ctx, const artgpu_plane *raw, const artgpu_rgb *out, DevImage *d)
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

// A plane a tool only reads (a mask, an area plane) as the device sees it.  One plane: a device plane in place, whatever its row stride; a host plane
// as a working copy in `slot`; no plane: nullptr and 0, nothing touched.  n planes of W x H, null entries allowed: likewise, `slot` holding every
// distinct host plane once (one plane may serve several entries: the host address is the key), staged in the order they are first seen
int bind_plane(artgpu_ctx *ctx, const artgpu_plane *pl, int slot, const float **p, size_t *stride)
{
    *p = nullptr; *stride = 0;
    if (!pl) return ARTGPU_OK;
    if (pl->on_device) { *p = pl->p; *stride = (size_t)(pl->row_stride_bytes / 4); return ARTGPU_OK; }
    float *copy;
    const int rc = plane_to_pool(ctx, pl, slot, &copy);
    *p = copy; *stride = pl->w;
    return rc;
}
int bind_planes(artgpu_ctx *ctx, int W, int H, const artgpu_plane *const *planes, int n, int slot, const float **p, size_t *stride)
{
    const size_t np = (size_t)W * H;
    std::vector<const artgpu_plane *> host;
    std::vector<size_t> at(n, 0);                  // per entry that is a host plane: which of `host`
    for (int i = 0; i < n; ++i) {
        const artgpu_plane *m = planes[i];
        if (!m || m->on_device) { p[i] = m ? m->p : nullptr; stride[i] = m ? (size_t)(m->row_stride_bytes / 4) : 0; continue; }
        at[i] = std::find_if(host.begin(), host.end(), [m](const artgpu_plane *q) { return q->p == m->p; }) - host.begin();
        if (at[i] == host.size()) host.push_back(m);
    }
    float *staged = nullptr;
    int rc;
    if (!host.empty() && (rc = pool_get(ctx, slot, host.size() * np * 4, &staged))) return rc;
    for (size_t k = 0; k < host.size(); ++k)
        HIPCHK(ctx, hipMemcpy2DAsync(staged + k * np, (size_t)W * 4, host[k]->p, (size_t)host[k]->row_stride_bytes, (size_t)W * 4, H, hipMemcpyHostToDevice, ctx->stream));
    for (int i = 0; i < n; ++i)
        if (planes[i] && !planes[i]->on_device) { p[i] = staged + at[i] * np; stride[i] = W; }
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
    ctx->sl_lut_dev = nullptr;
    ctx->bw_tab_dev = nullptr;
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
