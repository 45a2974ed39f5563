// art_amd/csrc/resize.hip -- ImProcFunctions::Lanczos on gfx950 (reference: rtengine/ipresize.cc:53-223): the vertical and the horizontal pass
// in one kernel, all three planes in one launch.
//
// A workgroup of 256 lanes produces RS_ROWS destination rows of tile_w destination columns.
//
//   vertical stage    Lane c owns source column jj0[first column of the tile] + c.  It walks down the strip's source rows once, from
//                     ii0[first row] to ii1[last row] - 1, and keeps the RS_ROWS destination rows' accumulators of its column in registers
//                     (3 x RS_ROWS, indexed statically).  Source row ii is added to destination row r exactly if ii0[r] <= ii < ii1[r]: both are
//                     the same for every lane, so the test is a scalar branch, and each destination row sums its taps in ascending source rows
//                     as lL / la / lb of the reference do (ipresize.cc:181-195; the 4-wide body above it is the same arithmetic).  For a
//                     downscale at most seven of the RS_ROWS tests hold for one source row, for an upscale up to all of them.  The weights of
//                     the RS_ROWS rows for one source row are one load: lane r of a wave fetches row r's, the branch reads it with readlane.
//                     Source rows are fetched four at a time, ahead of the arithmetic of the four.
//   LDS               The RS_ROWS x RS_SPAN interpolated values of each plane: what the reference keeps in lL, la, lb, for RS_ROWS rows at once.
//                     3 x 16 x 257 floats = 49 344 bytes, three workgroups per CU.  They never go to memory.
//   horizontal stage  One destination pixel per lane and step: the taps jj0[j] .. jj1[j] - 1 from LDS in ascending order (L198-215).  For a
//                     downscale neighbouring columns start `delta` floats apart in LDS, so the lanes of a wave run down the RS_ROWS rows first
//                     (rows are RS_PITCH = 257 floats apart: 16 different banks) and cover four columns; for an upscale neighbouring columns
//                     start less than one float apart and the lanes run along the row, which also makes the many stores of an upscale contiguous.
//
// w * s is rounded before it is added (-ffp-contract=off); a destination row or column without taps is 0.0f (L182, L202).
#include <hip/hip_runtime.h>
#include "resize.h"

namespace artgpu {

namespace {

template <bool ROWS_FAST>
__global__ void __launch_bounds__(256) resize_lanczos_kernel(RsArgs a)
{
    __shared__ float v[3][RS_ROWS][RS_PITCH];
    const int tid = threadIdx.x, lane = tid & 63;
    const int c0 = blockIdx.x * a.tile_w, c1 = min(c0 + a.tile_w, a.dW);
    const int i0 = blockIdx.y * RS_ROWS, nrows = min(RS_ROWS, a.dH - i0);
    // the tile's source columns [clo, chi): jj0 and jj1 do not decrease with j
    const int clo = min(a.jj0[c0], a.sW);
    const int chi = max(min(a.jj1[c1 - 1], a.sW), clo);

    // ---- vertical stage -----------------------------------------------------------------------------------------------------------
    // lane r of every wave holds the tap range of the tile's row r (rows behind the image's last: empty)
    const int rr = lane & (RS_ROWS - 1);
    const bool row_in = rr < nrows;
    const int my_row = i0 + (row_in ? rr : 0);
    const int my_lo = row_in ? a.ii0[my_row] : 0;
    const int my_hi = row_in ? min(a.ii1[my_row], a.sH) : 0;
    int lo[RS_ROWS], hi[RS_ROWS];
#pragma unroll
    for (int r = 0; r < RS_ROWS; ++r) {
        lo[r] = __builtin_amdgcn_readlane(my_lo, r);
        hi[r] = __builtin_amdgcn_readlane(my_hi, r);
    }
    const int rlo = lo[0];
    const int rhi = __builtin_amdgcn_readlane(my_hi, nrows - 1);       // ii1 does not decrease with i
    float accL[RS_ROWS], accA[RS_ROWS], accB[RS_ROWS];
#pragma unroll
    for (int r = 0; r < RS_ROWS; ++r) accL[r] = accA[r] = accB[r] = 0.f;

    if (clo < chi && rlo < rhi) {
        const int col = min(clo + tid, chi - 1);                       // lanes past the span repeat its last column; nobody reads their values
        const float *wrow = a.wv + (size_t)my_row * a.support;
        const float *pL = a.src[1] + col, *pA = a.src[0] + col, *pB = a.src[2] + col;       // L = g, a = r, b = b (Imagefloat in LAB mode)
        for (int ii = rlo; ii < rhi; ii += 4) {
            float sL[4], sA[4], sB[4], wq[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int row = min(ii + u, rhi - 1);                  // a repeated last row passes no test below
                const size_t o = (size_t)row * a.sstride;
                sL[u] = pL[o]; sA[u] = pA[o]; sB[u] = pB[o];
                wq[u] = wrow[min(max(row - my_lo, 0), a.support - 1)];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int row = ii + u;
#pragma unroll
                for (int r = 0; r < RS_ROWS; ++r) {
                    if (row >= lo[r] && row < hi[r]) {
                        const float w = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wq[u]), r));
                        accL[r] += w * sL[u];
                        accA[r] += w * sA[u];
                        accB[r] += w * sB[u];
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RS_ROWS; ++r) {
        v[0][r][tid] = accL[r];
        v[1][r][tid] = accA[r];
        v[2][r][tid] = accB[r];
    }
    __syncthreads();

    // ---- horizontal stage ---------------------------------------------------------------------------------------------------------
    const int ncols = c1 - c0;
    const auto pixel = [&](int r, int jl) {
        const int j = c0 + jl;
        const int j0 = a.jj0[j], j1 = min(a.jj1[j], a.sW);
        const float *w = a.wh + (size_t)j * a.support;
        const float *xL = &v[0][r][0] + (j0 - clo), *xA = &v[1][r][0] + (j0 - clo), *xB = &v[2][r][0] + (j0 - clo);
        float L = 0.f, A = 0.f, B = 0.f;
        for (int k = 0; k < j1 - j0; ++k) {
            const float wk = w[k];
            L += wk * xL[k];
            A += wk * xA[k];
            B += wk * xB[k];
        }
        const size_t o = (size_t)(i0 + r) * a.dstride + j;
        a.dst[1][o] = L; a.dst[0][o] = A; a.dst[2][o] = B;
    };
    if (ROWS_FAST) {
        const int r = tid & (RS_ROWS - 1);
        for (int jl = tid / RS_ROWS; jl < ncols; jl += 256 / RS_ROWS)
            if (r < nrows) pixel(r, jl);
    } else {
        for (int r = 0; r < nrows; ++r)
            for (int jl = tid; jl < ncols; jl += 256) pixel(r, jl);
    }
}

} // namespace

hipError_t launch_resize_lanczos(const RsArgs &a, bool rows_fast, hipStream_t s)
{
    const dim3 grid((a.dW + a.tile_w - 1) / a.tile_w, (a.dH + RS_ROWS - 1) / RS_ROWS);
    if (rows_fast) hipLaunchKernelGGL(resize_lanczos_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(resize_lanczos_kernel<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace artgpu
