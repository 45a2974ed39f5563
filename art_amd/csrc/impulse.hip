// art_amd/csrc/impulse.hip -- impulse noise reduction: impulse_nr's correction loop behind markImpulse (rtengine/impulse_denoise.cc:84-168).
//
// For every pixel markImpulse flagged, the reference sums dirwt, dirwt * L, dirwt * a and dirwt * b over the 5 x 5 window (clamped at the four
// edges), skipping neighbours that are flagged themselves, dirwt = 1 / (SQR(L[i1][j1] - L[i][j]) + 1.f), and writes the three quotients by norm
// `if (norm)`.  Only flagged pixels are written and only unflagged pixels are read (apart from the pixel's own L), so the loop runs in place
// without a race and gives the reference's bits in any order of the pixels.  A pixel's four sums stay on one lane, row-major, float, unfused
// from 0: their order is the contract.
//
// Kernel shape: one launch, one 256-thread workgroup per IMP_TILE_W x IMP_TILE_H tile.  Flagged pixels are sparse (a per cent or two) and
// clustered, so a lane per pixel would leave a wave waiting behind its one flagged lane through 25 dependent taps.  The workgroup instead
//   1. copies the tile's part of the impulse map plus a halo of 2 into LDS (1 B/px; what lies outside the image counts as flagged, which is
//      the reference's clamping: a skipped tap adds nothing);
//   2. compacts the tile's flagged pixels into a list in LDS: a ballot per wave and pass, the waves' counts in LDS, an exclusive prefix over
//      them (the list is in raster order of 256-pixel passes, whatever the waves' timing);
//   3. gives lane k the k-th flagged pixel (then k + 256, ...), so that the waves that work are full.
// The L, a, b values are read from memory, not staged: a tile's 12 B/px would be fetched for every tile, while the taps of 2 % flagged pixels
// touch a fraction of the lines (and neighbours in a cluster share them in the L1).  Traffic per pixel: 1 B of map, plus per flagged pixel up
// to 25 * 12 B of taps from cache and 12 B written.
#include "impulse.h"

namespace artgpu {

namespace {
constexpr int FW = IMP_TILE_W + 2 * IMP_HALO, FH = IMP_TILE_H + 2 * IMP_HALO;
constexpr int PASSES = IMP_TILE_W * IMP_TILE_H / 256, SLOTS = PASSES * 4;       // a slot: one wave's share of one pass
static_assert(IMP_TILE_W * IMP_TILE_H % 256 == 0 && SLOTS <= 16, "the counts' block holds 16 slots");
}

__global__ void __launch_bounds__(256) imp_correct_kernel(ImpArgs a)
{
    __shared__ unsigned char flag[FH][FW];
    __shared__ unsigned short list[IMP_TILE_W * IMP_TILE_H];
    __shared__ int count[17];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * IMP_TILE_W, y0 = blockIdx.y * IMP_TILE_H;
    for (int k = tid; k < FW * FH; k += 256) {
        const int r = k / FW, c = k - r * FW;
        const int gy = y0 - IMP_HALO + r, gx = x0 - IMP_HALO + c;
        flag[r][c] = (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) ? a.impish[(size_t)gy * a.W + gx] : (unsigned char)1;
    }
    __syncthreads();
    int rank[PASSES];
    bool mine[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const int q = p * 256 + tid, ly = q / IMP_TILE_W, lx = q - ly * IMP_TILE_W;
        mine[p] = y0 + ly < a.H && x0 + lx < a.W && flag[ly + IMP_HALO][lx + IMP_HALO] != 0;
        const unsigned long long m = __ballot(mine[p]);
        rank[p] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) count[p * 4 + wave] = __popcll(m);
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        int base = 0;
        for (int k = 0; k < SLOTS; ++k) {
            const int c = count[k];
            if (k < p * 4 + wave) base += c;
            if (p == 0) total += c;
        }
        if (mine[p]) list[base + rank[p]] = (unsigned short)(p * 256 + tid);
    }
    __syncthreads();
    for (int k = tid; k < total; k += 256) {
        const int q = list[k], ly = q / IMP_TILE_W, lx = q - ly * IMP_TILE_W;
        const int i = y0 + ly, j = x0 + lx;
        const size_t own = (size_t)i * a.stride + j;
        const float Lc = a.L[own];
        float norm = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int di = 0; di < 5; ++di)
            for (int dj = 0; dj < 5; ++dj) {
                if (flag[ly + di][lx + dj]) continue;       // flagged, or outside the image
                const size_t n = (size_t)(i + di - IMP_HALO) * a.stride + (j + dj - IMP_HALO);
                const float Ln = a.L[n];
                const float d = Ln - Lc;
                const float dirwt = 1.f / (d * d + 1.f);
                s0 += dirwt * Ln;
                s1 += dirwt * a.a[n];
                s2 += dirwt * a.b[n];
                norm += dirwt;
            }
        if (norm != 0.f) {                                  // `if (norm)`: a NaN norm writes too
            a.L[own] = s0 / norm;
            a.a[own] = s1 / norm;
            a.b[own] = s2 / norm;
        }
    }
}

hipError_t launch_imp_correct(const ImpArgs &a, hipStream_t s)
{
    const dim3 grid((unsigned)((a.W + IMP_TILE_W - 1) / IMP_TILE_W), (unsigned)((a.H + IMP_TILE_H - 1) / IMP_TILE_H));
    hipLaunchKernelGGL(imp_correct_kernel, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace artgpu
