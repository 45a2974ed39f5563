// art_amd/csrc/filmgrain.hip -- film grain on gfx950: one NOISE region of the Smoothing tool per launch
// (reference: rtengine/ipgrain.cc:33-98 filmGrain; rtengine/ipsmoothing.cc:565-695 add_noise, :943-980 the working copy, :1050-1064 the blend;
//  rtengine/rng.h:31-57 the generator; rtengine/rt_algo.cc:733-775 Convolution; Color::rgb2yuv / yuv2rgb color.h:783-796).
//
// No noise plane exists.  The value add_noise puts into noisebuf[y][x] is a pure function of the pixel and of its draw number, and draw
// number d is reached from the state the table's construction left by d + 1 steps of the generator's low 48 bits -- one affine map, composed
// from the maps of 2^j steps the host passes (DESIGN 35 has the argument why bits 48.. never reach an index).  So a workgroup that owns
// FG_TILE_W x FG_TILE_H pixels recomputes the noise of its (FG_TILE_W + 2r) x (FG_TILE_H + 2r) neighbourhood at clamped coordinates into LDS
// (once for channel L, once per plane for LC and C), runs the sz x sz direct sum from there in the fixed order that is its definition
// (acc = acc + k[i][j] * nb[y + i - c][x + j - c], i outer, j inner, fp32, unfused), and carries on in registers: the update, the channel's
// YUV step, the blend, the store.  A region reads 12 B/px and writes 12 B/px; source and destination are different planes because the
// neighbourhood is read from pixels other workgroups own.
// A workgroup walks a chunk of neighbouring tiles, so the 5233-entry table, the taps and the jump maps are fetched into LDS once per workgroup
// and most runs reach their first draw with one multiply-add from the previous tile's.  Per tile a lane issues its
// loads first (its own pixels and mask, then a run's source values), then computes.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "devmath.h"
#include "smoothing.h"
#include "filmgrain.h"

namespace artgpu {

namespace {

constexpr float FG_F1 = 1.f / 65535.f;     // normalizeFloatTo1's factor (imagefloat.cc:396-432)

// Color::rgb2yuv / yuv2rgb with the double matrix (color.h:783-796): the products are double, the results float
__device__ __forceinline__ float fg_lum(float r, float g, float b, const double *ws1) { return (float)(r * ws1[0] + g * ws1[1] + b * ws1[2]); }
__device__ __forceinline__ void fg_yuv2rgb(float Y, float u, float v, float &R, float &G, float &B, const double *ws1)
{
    B = Y - u;
    R = v + Y;
    G = (float)((Y - R * ws1[0] - B * ws1[2]) / ws1[1]);
}

// RandomNumberGenerator::next on the bits that matter (rng.h:48-51): the state's low 48 bits
__device__ __forceinline__ uint64_t fg_step(uint64_t s) { return (s * FG_LCG_A + FG_LCG_C) & FG_MASK48; }
// n steps at once: the maps of the set bits of n, lowest first (they commute: all are powers of one map).  A, C: the workgroup's LDS copy of
// the table; the loop is not unrolled so that the table stays there instead of being held in a hundred registers
__device__ __forceinline__ uint64_t fg_jump(uint64_t s, uint64_t n, const uint64_t *A, const uint64_t *C)
{
#pragma unroll 1
    for (int b = 0; b < FG_JUMP_USED && (n >> b) != 0; ++b) {
        const uint64_t t = (A[b] * s + C[b]) & FG_MASK48;
        s = ((n >> b) & 1) ? t : s;
    }
    return s;
}
// the state draw number `draw` reads (counted from `state`, the first draw is number 0), and randint(5233) of a state (rng.h:35-39)
__device__ __forceinline__ uint64_t fg_draw_state(uint64_t state, uint64_t draw, const uint64_t *A, const uint64_t *C) { return fg_jump(state, draw + 1, A, C); }
// the table's jump maps (FgJump behind the floats of a region's device table) into LDS
__device__ __forceinline__ void fg_load_jump(const float *tab, uint64_t *A, uint64_t *C, int tid)
{
    const FgJump *j = reinterpret_cast<const FgJump *>(tab + FG_TAB_FLOATS);
    if (tid < FG_JUMP_USED) { A[tid] = j->A[tid]; C[tid] = j->C[tid]; }
}
__device__ __forceinline__ uint32_t fg_index(uint64_t s) { return (uint32_t)(s >> 16) % (uint32_t)FG_NORMD; }

// the lambda's first loop (ipsmoothing.cc:620-629)
__device__ __forceinline__ float fg_noise(float v, float nd, float sd, float c)
{
    const float mu = std_max(v, 0.f) * c;
    const float r = nd * sd;
    const float m = mu + sqrtf(mu) * r;
    return m / c - v;
}

} // namespace

template <int CH, int R>
__global__ void __launch_bounds__(256) fg_region_kernel(FgArgs a)
{
    constexpr int SZ = 2 * R + 1, TW = FG_TILE_W + 2 * R, TH = FG_TILE_H + 2 * R, RUNS = (TW + FG_RUN - 1) / FG_RUN;
    constexpr int NPLANES = CH == SM_CH_L ? 1 : 3;
    __shared__ float s_tab[FG_NORMD];
    __shared__ float s_k[FG_MAX_TAPS];
    __shared__ float s_n[(FG_TILE_H + 2 * FG_MAX_R) * FG_LDS_STRIDE];
    __shared__ uint64_t s_ja[FG_JUMP_USED], s_jc[FG_JUMP_USED];
    const int tid = threadIdx.x;
    fg_load_jump(a.tab, s_ja, s_jc, tid);
    for (int i = tid; i < FG_NORMD; i += 256) s_tab[i] = a.tab[i];
    if (tid < SZ * SZ) s_k[tid] = a.tab[FG_NORMD + tid];
    const int tiles_x = (a.ww + FG_TILE_W - 1) / FG_TILE_W, tiles_y = (a.hh + FG_TILE_H - 1) / FG_TILE_H;
    const int ntiles = tiles_x * tiles_y;
    const int tx = tid & (FG_TILE_W / FG_PX - 1), ty = tid / (FG_TILE_W / FG_PX);
    const uint64_t plane_px = (uint64_t)a.ww * (uint64_t)a.hh;

    // A workgroup takes a contiguous chunk of the tiles in raster order.  Between neighbouring tiles of one tile row a run's first draw number
    // moves on by exactly FG_TILE_W (unless a clamp at the frame's edge is involved), so a lane keeps the state its run started from and
    // reaches the next tile's with the one map of 2^6 steps; everything else (a chunk's first tile, a new tile row, the edges) is the full jump
    static_assert(FG_TILE_W == 64, "the map of 2^6 steps carries a run's state from tile to tile");
    static_assert(RUNS * TH <= 256, "a lane fills at most one run per plane");
    const int chunk = (ntiles + (int)gridDim.x - 1) / (int)gridDim.x;
    const int tile_begin = min((int)blockIdx.x * chunk, ntiles), tile_end = min(tile_begin + chunk, ntiles);
    uint64_t run_state[NPLANES], run_draw[NPLANES];
#pragma unroll
    for (int c = 0; c < NPLANES; ++c) { run_state[c] = 0; run_draw[c] = 1ULL << 40; }      // (no draw number is that large)

    for (int tile = tile_begin; tile < tile_end; ++tile) {
        const int x0 = (tile % tiles_x) * FG_TILE_W, y0 = (tile / tiles_x) * FG_TILE_H;
        const int py = y0 + ty, cy = min(py, a.hh - 1);
        // the lane's own pixels (clamped addresses: a lane past the edge reads the edge and stores nothing)
        float v[3][FG_PX], m[FG_PX];
#pragma unroll
        for (int q = 0; q < FG_PX; ++q) {
            const int cx = min(x0 + tx * FG_PX + q, a.ww - 1);
            const size_t si = (size_t)cy * a.src_stride + cx;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][q] = a.src[c][si];
            m[q] = a.mask ? a.mask[(size_t)cy * a.mask_stride + cx] : 1.f;
        }
        if (a.norm_in) {
#pragma unroll
            for (int q = 0; q < FG_PX; ++q) { v[0][q] *= FG_F1; v[1][q] *= FG_F1; v[2][q] *= FG_F1; }
        }
        float w[3][FG_PX];      // the working copy's pixels
#pragma unroll
        for (int q = 0; q < FG_PX; ++q) {
            if (CH == SM_CH_L) {            // rgb2yuv into G / R / B (L656): w[0] = Y, w[1] = u, w[2] = v
                const float Y = fg_lum(v[0][q], v[1][q], v[2][q], a.ws1);
                w[0][q] = Y; w[1][q] = Y - v[2][q]; w[2][q] = v[0][q] - Y;
            } else { w[0][q] = v[0][q]; w[1][q] = v[1][q]; w[2][q] = v[2][q]; }
        }

#pragma unroll 1
        for (int p = 0; p < NPLANES; ++p) {
            const float sd = CH == SM_CH_L ? 1.f : p == 0 ? 0.7f : p == 1 ? 1.f : 1.3f;      // chan_sd (L610): Y; R, G, B
            const float *sp = p == 0 ? a.src[0] : p == 1 ? a.src[1] : a.src[2];
            __syncthreads();        // the tables are in LDS (first tile); the previous direct sum has read s_n
            if (tid < RUNS * TH) {
                const int ry = tid / RUNS, rx0 = (tid - ry * RUNS) * FG_RUN;
                const int gy = min(max(y0 + ry - R, 0), a.hh - 1);
                int gx[FG_RUN];
                float val[FG_RUN];
#pragma unroll
                for (int k = 0; k < FG_RUN; ++k) {
                    gx[k] = min(max(x0 + rx0 + k - R, 0), a.ww - 1);
                    const size_t si = (size_t)gy * a.src_stride + gx[k];
                    if (CH == SM_CH_L) {
                        float r = a.src[0][si], g = a.src[1][si], b = a.src[2][si];
                        if (a.norm_in) { r *= FG_F1; g *= FG_F1; b *= FG_F1; }
                        val[k] = fg_lum(r, g, b, a.ws1);
                    } else {
                        val[k] = sp[si];
                        if (a.norm_in) val[k] *= FG_F1;
                    }
                }
                // pixel (gy, gx) of plane p draws number p * ww * hh + gy * ww + gx: the run's first by jump-ahead, then a step per new pixel
                const uint64_t draw = (uint64_t)p * plane_px + (uint64_t)gy * (uint64_t)a.ww + (uint64_t)gx[0];
                uint64_t prev_state = 0, prev_draw = 0;
#pragma unroll
                for (int c = 0; c < NPLANES; ++c)
                    if (c == p) { prev_state = run_state[c]; prev_draw = run_draw[c]; }
                uint64_t s = draw == prev_draw + FG_TILE_W ? (s_ja[6] * prev_state + s_jc[6]) & FG_MASK48 : fg_draw_state(a.state, draw, s_ja, s_jc);
#pragma unroll
                for (int c = 0; c < NPLANES; ++c)
                    if (c == p) { run_state[c] = s; run_draw[c] = draw; }
#pragma unroll
                for (int k = 0; k < FG_RUN; ++k) {
                    if (k > 0 && gx[k] != gx[k - 1]) s = fg_step(s);
                    const float nv = fg_noise(val[k], s_tab[fg_index(s)], sd, a.c);
                    if (rx0 + k < TW) s_n[ry * FG_LDS_STRIDE + rx0 + k] = nv;
                }
            }
            __syncthreads();
            // Convolution as the direct sum (rt_algo.cc:733-775): i outer, j inner, one unfused multiply-add per tap
            float acc[FG_PX];
#pragma unroll
            for (int q = 0; q < FG_PX; ++q) acc[q] = 0.f;
            // (the rows one after the other: unrolled, the compiler fetches all sz rows and taps ahead of the sum -- 206 registers at sz 7, two
            // workgroups per CU; this way at most 118, four per CU)
#pragma unroll 1
            for (int i = 0; i < SZ; ++i) {
                float seg[FG_PX + 2 * R];
#pragma unroll
                for (int k = 0; k < FG_PX + 2 * R; ++k) seg[k] = s_n[(ty + i) * FG_LDS_STRIDE + tx * FG_PX + k];
#pragma unroll
                for (int j = 0; j < SZ; ++j) {
                    const float kij = s_k[i * SZ + j];
#pragma unroll
                    for (int q = 0; q < FG_PX; ++q) acc[q] = acc[q] + kij * seg[q + j];
                }
            }
            // a = max(a + sf * n, 0.f) (L640); `p` selects the plane without indexing registers dynamically
#pragma unroll
            for (int q = 0; q < FG_PX; ++q) {
#pragma unroll
                for (int c = 0; c < NPLANES; ++c)
                    if (c == p) w[c][q] = std_max(w[c][q] + a.sf * acc[q], 0.f);
            }
        }

#pragma unroll
        for (int q = 0; q < FG_PX; ++q) {
            float o0, o1, o2;
            if (CH == SM_CH_L) {                    // yuv2rgb(G, R, B) (L667)
                fg_yuv2rgb(w[0][q], w[1][q], w[2][q], o0, o1, o2, a.ws1);
            } else if (CH == SM_CH_C) {             // the input's Y under the noisy u, v (L671-693)
                const float Y0 = fg_lum(v[0][q], v[1][q], v[2][q], a.ws1);
                const float l = fg_lum(w[0][q], w[1][q], w[2][q], a.ws1);
                fg_yuv2rgb(Y0, l - w[2][q], w[0][q] - l, o0, o1, o2, a.ws1);
            } else { o0 = w[0][q]; o1 = w[1][q]; o2 = w[2][q]; }
            o0 = intp(m[q], o0, v[0][q]); o1 = intp(m[q], o1, v[1][q]); o2 = intp(m[q], o2, v[2][q]);     // L1060-1062
            if (a.denorm_out) { o0 *= 65535.f; o1 *= 65535.f; o2 *= 65535.f; }
            const int px = x0 + tx * FG_PX + q;
            if (px < a.ww && py < a.hh) {
                const size_t di = (size_t)py * a.dst_stride + px;
                a.dst[0][di] = o0; a.dst[1][di] = o1; a.dst[2][di] = o2;
            }
        }
    }
}

// artgpu_grain_indices: the table indices of draws first .. first + n - 1, a lane per run of FG_RUN draws as in the region kernel
__global__ void __launch_bounds__(256) fg_indices_kernel(const float *tab, uint64_t state, uint64_t first, int n, uint32_t *out)
{
    __shared__ uint64_t s_ja[FG_JUMP_USED], s_jc[FG_JUMP_USED];
    fg_load_jump(tab, s_ja, s_jc, threadIdx.x);
    __syncthreads();
    const int k0 = (blockIdx.x * 256 + threadIdx.x) * FG_RUN;
    if (k0 >= n) return;
    uint64_t s = fg_draw_state(state, first + (uint64_t)k0, s_ja, s_jc);
    for (int k = 0; k < FG_RUN && k0 + k < n; ++k) {
        if (k > 0) s = fg_step(s);
        out[k0 + k] = fg_index(s);
    }
}

hipError_t launch_fg_region(const FgArgs &a, int max_workgroups, hipStream_t s)
{
    const long long ntiles = (long long)((a.ww + FG_TILE_W - 1) / FG_TILE_W) * ((a.hh + FG_TILE_H - 1) / FG_TILE_H);
    const dim3 g((unsigned)std::max(1LL, std::min(ntiles, (long long)max_workgroups)));
#define FG_BY_R(CH)                                                                                   \
    do {                                                                                              \
        if (a.r == 1) hipLaunchKernelGGL((fg_region_kernel<CH, 1>), g, dim3(256), 0, s, a);           \
        else if (a.r == 2) hipLaunchKernelGGL((fg_region_kernel<CH, 2>), g, dim3(256), 0, s, a);      \
        else hipLaunchKernelGGL((fg_region_kernel<CH, 3>), g, dim3(256), 0, s, a);                    \
    } while (0)
    if (a.r < 1 || a.r > FG_MAX_R) return hipErrorInvalidValue;
    if (a.channel == SM_CH_L) FG_BY_R(SM_CH_L);
    else if (a.channel == SM_CH_C) FG_BY_R(SM_CH_C);
    else FG_BY_R(SM_CH_LC);
#undef FG_BY_R
    return hipGetLastError();
}

hipError_t launch_fg_indices(const float *tab, uint64_t state, uint64_t first, int n, uint32_t *out, hipStream_t s)
{
    const int runs = (n + FG_RUN - 1) / FG_RUN;
    hipLaunchKernelGGL(fg_indices_kernel, dim3((runs + 255) / 256), dim3(256), 0, s, tab, state, first, n, out);
    return hipGetLastError();
}

} // namespace artgpu
