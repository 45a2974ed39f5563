// art_amd/csrc/api_filmsim.hip -- ImProcFunctions::filmSimulation (rtengine/ipfilmsim.cc:33-73) with a HaldCLUT behind the C ABI: the CLUT
// handle, the checks, the launch.  The kernel is filmsim.hip's; the two sRGB tables are hostluts.hip's.
#include "api_internal.h"
#include <atomic>

using namespace artgpu;
using namespace artgpu::api;

// The device copy of one HaldCLUT and of the two tables every lookup goes through, in one allocation:
// [gamma2curve 65536 floats | igammatab_srgb 65536 floats | level^3 + 1 RGBX entries].  Immutable after artgpu_clut_create, so every
// context of the device reads it without any ordering of its own; counted because a pipe setting outlives the caller's handle.
struct artgpu_clut {
    unsigned magic;
    int device, level;
    float *dev;
    std::atomic<int> refs;
};

namespace {

constexpr unsigned CLUT_MAGIC = 0x48414c44u;       // "HALD"; cleared when the handle dies

bool clut_level_ok(int level)
{
    for (int k = 2; k <= 16; ++k)
        if (level == k * k) return true;
    return false;
}

} // namespace

namespace artgpu { namespace api {

void clut_release(artgpu_clut *clut)
{
    if (!clut || clut->magic != CLUT_MAGIC || clut->refs.fetch_sub(1) != 1) return;
    clut->magic = 0;
    int cur = -1;
    const bool moved = hipGetDevice(&cur) == hipSuccess && cur != clut->device && hipSetDevice(clut->device) == hipSuccess;
    (void)hipFree(clut->dev);                      // (waits for the device: no kernel still reads the tables)
    if (moved) (void)hipSetDevice(cur);
    delete clut;
}

int fs_check(artgpu_ctx *ctx, const artgpu_clut *clut, const artgpu_film_simulation_params *p, const char *who)
{
    if (!clut || !p) return fail(ctx, ARTGPU_EINVAL, "%s: bad arguments", who);
    if (clut->magic != CLUT_MAGIC || !clut->dev) return fail(ctx, ARTGPU_EINVAL, "%s: not a CLUT handle", who);
    if (clut->device != ctx->device) return fail(ctx, ARTGPU_EINVAL, "%s: the CLUT lives on device %d, the context on device %d", who, clut->device, ctx->device);
    if (!std::isfinite(p->strength)) return fail(ctx, ARTGPU_EINVAL, "%s: strength is not finite", who);
    return ARTGPU_OK;
}

int film_simulation_dev(artgpu_ctx *ctx, float *const planes[3], size_t stride, int W, int H, const artgpu_clut *clut, const artgpu_film_simulation_params *p)
{
    FsArgs a = {};
    for (int k = 0; k < 3; ++k) a.img[k] = planes[k];
    a.stride = stride; a.W = W; a.H = H;
    a.gam = clut->dev; a.igam = clut->dev + 65536;
    a.clut = reinterpret_cast<const unsigned short *>(clut->dev + 2 * 65536);
    a.level = (unsigned)clut->level;
    a.flm1 = static_cast<float>(clut->level - 1) / 65535.0f;            // clutstore.cc:155-156
    a.flm2 = static_cast<float>(clut->level - 2);
    a.strength = p->strength;
    if (!p->same_profile) {
        const double *m[4] = {p->work_to_xyz, p->xyz_to_clut, p->clut_to_xyz, p->xyz_to_work};
        for (int k = 0; k < 4; ++k)
            for (int i = 0; i < 9; ++i) { a.md[k][i] = m[k][i]; a.mf[k][i] = (float)m[k][i]; }       // F2V(wprof_[i][j]) (L1100-1107)
    }
    HIPCHK(ctx, launch_filmsim(a, p->same_profile != 0, ctx->stream));
    return ARTGPU_OK;
}

} } // namespace artgpu::api

extern "C" {

int artgpu_clut_create(artgpu_ctx *ctx, const uint16_t *table, int level, int channels, artgpu_clut **out)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (out) *out = nullptr;
    if (!table || !out || (channels != 3 && channels != 4)) return fail(ctx, ARTGPU_EINVAL, "clut_create: bad arguments");
    if (!clut_level_ok(level)) return fail(ctx, ARTGPU_EINVAL, "clut_create: level %d is not the square of 2 .. 16", level);
    const size_t n = (size_t)level * level * level;
    const size_t floats = 2 * 65536 + (n + 1) * 2;                      // an RGBX entry is 8 bytes
    std::vector<float> host(floats, 0.f);
    build_gamma2curve(host.data());
    build_igammatab_srgb(host.data() + 65536);
    uint16_t *e = reinterpret_cast<uint16_t *>(host.data() + 2 * 65536);
    for (size_t i = 0; i < n; ++i, e += 4) { e[0] = table[i * channels]; e[1] = table[i * channels + 1]; e[2] = table[i * channels + 2]; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    artgpu_clut *c = new (std::nothrow) artgpu_clut;
    if (!c) return fail(ctx, ARTGPU_ENOMEM, "clut_create: handle");
    c->magic = CLUT_MAGIC; c->device = ctx->device; c->level = level; c->dev = nullptr; c->refs = 1;
    if (hipMalloc(reinterpret_cast<void **>(&c->dev), floats * 4) != hipSuccess) { delete c; return fail(ctx, ARTGPU_ENOMEM, "clut_create: %zu bytes on the device", floats * 4); }
    if (hipMemcpy(c->dev, host.data(), floats * 4, hipMemcpyHostToDevice) != hipSuccess) { clut_release(c); return fail(ctx, ARTGPU_EHIP, "clut_create: upload failed"); }
    *out = c;
    return ARTGPU_OK;
}

void artgpu_clut_destroy(artgpu_clut *clut) { clut_release(clut); }

int artgpu_film_simulation_tables(float *gamma2curve, float *igammatab_srgb)
{
    if (gamma2curve) build_gamma2curve(gamma2curve);
    if (igammatab_srgb) build_igammatab_srgb(igammatab_srgb);
    return ARTGPU_OK;
}

int artgpu_film_simulation(artgpu_ctx *ctx, artgpu_rgb *img, const artgpu_clut *clut, const artgpu_film_simulation_params *p)
{
    StageScope scope_(ctx, "ImProcFunctions::filmSimulation");
    if (!ctx) return ARTGPU_EINVAL;
    if (!img || !plane_ok(&img->r)) return fail(ctx, ARTGPU_EINVAL, "film_simulation: bad arguments");
    int rc;
    if ((rc = fs_check(ctx, clut, p, "film_simulation"))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevRGB d;
    if ((rc = bind_rgb(ctx, img, 4, true, &d, "film_simulation"))) return rc;
    if ((rc = film_simulation_dev(ctx, d.p, d.stride, d.w, d.h, clut, p))) return rc;
    return unbind_rgb(ctx, img, &d);
}

int artgpu_set_pipeline_film_simulation(artgpu_ctx *ctx, const artgpu_clut *clut, const artgpu_film_simulation_params *p, int after_tone_curve)
{
    if (!ctx) return ARTGPU_EINVAL;
    if (clut && (!p || clut->magic != CLUT_MAGIC)) return fail(ctx, ARTGPU_EINVAL, "set_pipeline_film_simulation: bad arguments");
    artgpu_clut *keep = const_cast<artgpu_clut *>(clut);
    if (keep) keep->refs.fetch_add(1);
    clut_release(ctx->pipe_fs_own);
    ctx->pipe_fs_own = keep;
    ctx->shared.pipe_fs = keep;
    ctx->shared.pipe_fs_par = keep ? *p : artgpu_film_simulation_params{};
    ctx->shared.pipe_fs_after = keep && after_tone_curve ? 1 : 0;
    return ARTGPU_OK;
}

} // extern "C"
