// CPU checker for the raw CA correction (RawImageSource::CA_correct_RT, rtengine/CA_correct_RT.cc:122-1384), one frame.
// TEST INFRASTRUCTURE ONLY: a restatement written from the reference's structure (per-tile buffers, memset per tile, the
// stored filter planes), kept independent of the device code (art_amd/csrc/cacorrect.hip recomputes what this file stores).
//
// The SSE2 build is the one restated: where the reference has a 4-lane body and a scalar tail with different expressions or a
// different summation order, both are kept (lane arrays below).  The places that change bits:
//   - the pass-1 loader stores all 8 samples of a vector step into the G plane (non-green ones included, L338-345), the scalar
//     tail only the green ones; the un-interpolated border rows / columns of the G plane read those values;
//   - rbhpfv / rbhpfh: the vector body associates the second and third differences differently (L500-508 vs L523-528);
//   - the coefficient sums: 4 lane accumulators per row, vhadd ((l0 + l2) + (l1 + l3)), then the scalar tail with the other
//     gdiff form (L561-623).
// Block sums (blockave / blocksqave / blockdenom) run in tile raster order, the reference's single-thread order (the only
// order it leaves to its scheduler).  The tile buffer has the reference's layout (CA_correct_RT.cc:260-287, 64-byte pads between
// the planes): the pass-1 border fills of frames with H % 112 or W % 112 in 1..7 write past a plane's rows into the next row / pad /
// plane, and large manual shifts make pass 2 read G outside rgb[1]; both happen here as in the reference.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

constexpr int ts = 128, tsh = 64, border = 8, border2 = 16, cb = 2;
constexpr int v1 = ts, v2 = 2 * ts, v3 = 3 * ts, v4 = 4 * ts;
constexpr float eps = 1e-5f, eps2 = 1e-10f;

struct Cfa {
    unsigned c[2][2];
    unsigned operator()(int r, int col) const { return c[r & 1][col & 1]; }
};
Cfa make_cfa(unsigned filters)
{
    Cfa f;
    for (int r = 0; r < 2; ++r)
        for (int c = 0; c < 2; ++c) f.c[r][c] = (filters >> ((((r << 1) & 14) + (c & 1)) << 1)) & 3;
    return f;
}
inline float SQR(float x) { return x * x; }
inline float intp(float a, float b, float c) { return a * b + (1.f - a) * c; }
inline float fmin_(float a, float b) { return b < a ? b : a; }
inline float fmax_(float a, float b) { return a < b ? b : a; }

float median9(std::array<float, 9> a)
{
    float tmp;
#define MN(x, y) fmin_(x, y)
#define MX(x, y) fmax_(x, y)
    tmp = MN(a[1], a[2]); a[2] = MX(a[1], a[2]); a[1] = tmp;
    tmp = MN(a[4], a[5]); a[5] = MX(a[4], a[5]); a[4] = tmp;
    tmp = MN(a[7], a[8]); a[8] = MX(a[7], a[8]); a[7] = tmp;
    tmp = MN(a[0], a[1]); a[1] = MX(a[0], a[1]); a[0] = tmp;
    tmp = MN(a[3], a[4]); a[4] = MX(a[3], a[4]); a[3] = tmp;
    tmp = MN(a[6], a[7]); a[7] = MX(a[6], a[7]); a[6] = tmp;
    tmp = MN(a[1], a[2]); a[2] = MX(a[1], a[2]); a[1] = tmp;
    tmp = MN(a[4], a[5]); a[5] = MX(a[4], a[5]); a[4] = tmp;
    tmp = MN(a[7], a[8]); a[8] = MX(a[7], a[8]);
    a[3] = MX(a[0], a[3]);
    a[5] = MN(a[5], a[8]);
    a[7] = MX(a[4], tmp);
    tmp = MN(a[4], tmp);
    a[6] = MX(a[3], a[6]);
    a[4] = MX(a[1], tmp);
    a[2] = MN(a[2], a[5]);
    a[4] = MN(a[4], a[7]);
    tmp = MN(a[4], a[2]);
    a[2] = MX(a[4], a[2]);
    a[4] = MX(a[6], tmp);
    return MN(a[4], a[2]);
#undef MN
#undef MX
}

bool lin_eq_solve(int n, double *m, double *v, double *x)
{
    for (int k = 0; k < n - 1; k++) {
        double mx = std::fabs(m[k * n + k]);
        int p = k;
        for (int i = k + 1; i < n; i++)
            if (mx < std::fabs(m[i * n + k])) { mx = m[i * n + k]; p = i; }   // the reference keeps the signed value here
        if (p != k) {
            for (int i = k; i < n; i++) std::swap(m[k * n + i], m[p * n + i]);
            std::swap(v[k], v[p]);
        }
        if (m[k * n + k] == 0.) return false;
        for (int j = k + 1; j < n; j++) {
            const double a = -m[j * n + k] / m[k * n + k];
            for (int i = k; i < n; i++) m[j * n + i] = m[j * n + i] + a * m[k * n + i];
            v[j] = v[j] + a * v[k];
        }
    }
    for (int k = n - 1; k >= 0; k--) {
        x[k] = v[k];
        for (int i = k + 1; i < n; i++) x[k] -= m[k * n + i] * x[i];
        x[k] = x[k] / m[k * n + k];
    }
    return true;
}

struct Geo {
    int W, H, width, height, vblsz, hblsz;
};
Geo geometry(int W, int H)
{
    Geo g;
    g.W = W; g.H = H; g.width = W + (W & 1); g.height = H;
    const int vz1 = (g.height + border2) % (ts - border2) == 0 ? 1 : 0;
    const int hz1 = (g.width + border2) % (ts - border2) == 0 ? 1 : 0;
    g.vblsz = (int)std::ceil((float)(g.height + border2) / (ts - border2) + 2 + vz1);
    g.hblsz = (int)std::ceil((float)(g.width + border2) / (ts - border2) + 2 + hz1);
    return g;
}

// the reference's per-thread tile buffer (L260-287, float offsets of `data`): rgb[0..2] and the six filter planes of pass 1, each
// after a 64-byte pad; pass 2 puts grbdiff / gshift where rbhpfh / rbhpfv are (L844-846)
struct Tile {
    std::vector<float> buf;
    float *rgb[3], *rbhpfh, *rbhpfv, *rblpfh, *rblpfv, *grblpfh, *grblpfv;
    Tile() : buf(4 * ts * ts + 2 * ts * tsh + 8 * 16)
    {
        float *p = buf.data();
        rgb[0] = p;
        rgb[1] = p + ts * tsh + 16;
        rgb[2] = p + ts * ts + ts * tsh + 32;
        rbhpfh = p + 2 * ts * ts + 48;
        rbhpfv = p + 2 * ts * ts + ts * tsh + 64;
        rblpfh = p + 3 * ts * ts + 80;
        rblpfv = p + 3 * ts * ts + ts * tsh + 96;
        grblpfh = p + 4 * ts * ts + 112;
        grblpfv = p + 4 * ts * ts + ts * tsh + 128;
    }
    void clear() { std::fill(buf.begin(), buf.end(), 0.f); }
    // rgb[c][(rr * ts + cc) >> ((c & 1) ^ 1)], as the reference indexes it: rows / columns past the tile included
    void put(int c, int rr, int cc, float v) { rgb[c][(rr * ts + cc) >> ((c & 1) ^ 1)] = v; }
    float get(int c, int rr, int cc) const { return rgb[c][(rr * ts + cc) >> ((c & 1) ^ 1)]; }
};

struct TileBox {
    int top, left, vblock, hblock, rr1, cc1, rrmin, rrmax, ccmin, ccmax;
};
TileBox tile_box(const Geo &g, int top, int left)
{
    TileBox t;
    t.top = top; t.left = left;
    t.vblock = (top + border) / (ts - border2) + 1;
    t.hblock = (left + border) / (ts - border2) + 1;
    const int bottom = std::min(top + ts, g.height + border);
    const int right = std::min(left + ts, g.width - (g.W & 1) + border);
    t.rr1 = bottom - top;
    t.cc1 = right - left;
    t.rrmin = top < 0 ? border : 0;
    t.rrmax = bottom > g.height ? g.height - top : t.rr1;
    t.ccmin = left < 0 ? border : 0;
    t.ccmax = (right > g.width - (g.W & 1)) ? g.width - (g.W & 1) - left : t.cc1;
    return t;
}

inline float RAW(const float *raw, const Geo &g, int r, int c) { return raw[(size_t)r * g.W + c]; }

// pass-1 directional G at a non-green site (L441-470; vector and scalar forms agree)
inline float g_interp(const Tile &T, int c, int indx)
{
    const float *g = T.rgb[1], *n = T.rgb[c];
    const float wtu = 1.f / SQR(eps + std::fabs(g[indx + v1] - g[indx - v1]) + std::fabs(n[indx >> 1] - n[(indx - v2) >> 1]) + std::fabs(g[indx - v1] - g[indx - v3]));
    const float wtd = 1.f / SQR(eps + std::fabs(g[indx - v1] - g[indx + v1]) + std::fabs(n[indx >> 1] - n[(indx + v2) >> 1]) + std::fabs(g[indx + v1] - g[indx + v3]));
    const float wtl = 1.f / SQR(eps + std::fabs(g[indx + 1] - g[indx - 1]) + std::fabs(n[indx >> 1] - n[(indx - 2) >> 1]) + std::fabs(g[indx - 1] - g[indx - 3]));
    const float wtr = 1.f / SQR(eps + std::fabs(g[indx - 1] - g[indx + 1]) + std::fabs(n[indx >> 1] - n[(indx + 2) >> 1]) + std::fabs(g[indx + 1] - g[indx + 3]));
    return (wtu * g[indx - v1] + wtd * g[indx + v1] + wtl * g[indx - 1] + wtr * g[indx + 1]) / (wtu + wtd + wtl + wtr);
}

// ------------------------------------------------------------------------------------------------ pass 1 (L303-686)
void pass1_tile(const float *raw, const Geo &g, const Cfa &cfa, const TileBox &t, Tile &T, float *Gtmp, float *blockwt,
                float (*blockshifts)[2][2], float blockave[2][2], float blocksqave[2][2], float blockdenom[2][2])
{
    T.clear();
    const int rr1 = t.rr1, cc1 = t.cc1, top = t.top, left = t.left;
    const int height = g.height, width = g.width;
    for (int rr = t.rrmin; rr < t.rrmax; rr++) {
        const int row = rr + top;
        int cc = t.ccmin;
        int c0 = cfa(rr, cc);
        if (c0 == 1) { T.rgb[1][rr * ts + cc] = RAW(raw, g, row, cc + left) / 65535.f; cc++; c0 = cfa(rr, cc); }
        for (; cc < t.ccmax - 7; cc += 8)            // vector loader: all 8 samples into rgb[1]
            for (int k = 0; k < 8; ++k) {
                const float v = RAW(raw, g, row, cc + k + left) / 65535.f;
                T.rgb[1][rr * ts + cc + k] = v;
                if ((k & 1) == 0) T.rgb[c0][(rr * ts + cc + k) >> 1] = v;
            }
        for (; cc < t.ccmax; cc++) T.put(cfa(rr, cc), rr, cc, RAW(raw, g, row, cc + left) / 65535.f);
    }
    if (t.rrmin > 0)
        for (int rr = 0; rr < border; rr++)
            for (int cc = t.ccmin; cc < t.ccmax; cc++) { const int c = cfa(rr, cc); T.put(c, rr, cc, T.get(c, border2 - rr, cc)); }
    if (t.rrmax < rr1)
        for (int rr = 0; rr < border; rr++)
            for (int cc = t.ccmin; cc < t.ccmax; cc++) T.put(cfa(rr, cc), t.rrmax + rr, cc, RAW(raw, g, height - rr - 2, left + cc) / 65535.f);
    if (t.ccmin > 0)
        for (int rr = t.rrmin; rr < t.rrmax; rr++)
            for (int cc = 0; cc < border; cc++) { const int c = cfa(rr, cc); T.put(c, rr, cc, T.get(c, rr, border2 - cc)); }
    if (t.ccmax < cc1)
        for (int rr = t.rrmin; rr < t.rrmax; rr++)
            for (int cc = 0; cc < border; cc++) T.put(cfa(rr, cc), rr, t.ccmax + cc, RAW(raw, g, top + rr, width - cc - 2) / 65535.f);
    if (t.rrmin > 0 && t.ccmin > 0)
        for (int rr = 0; rr < border; rr++)
            for (int cc = 0; cc < border; cc++) T.put(cfa(rr, cc), rr, cc, RAW(raw, g, border2 - rr, border2 - cc) / 65535.f);
    if (t.rrmax < rr1 && t.ccmax < cc1)
        for (int rr = 0; rr < border; rr++)
            for (int cc = 0; cc < border; cc++) T.put(cfa(rr, cc), t.rrmax + rr, t.ccmax + cc, RAW(raw, g, height - rr - 2, width - cc - 2) / 65535.f);
    if (t.rrmin > 0 && t.ccmax < cc1)
        for (int rr = 0; rr < border; rr++)
            for (int cc = 0; cc < border; cc++) T.put(cfa(rr, cc), rr, t.ccmax + cc, RAW(raw, g, border2 - rr, width - cc - 2) / 65535.f);
    if (t.rrmax < rr1 && t.ccmin > 0)
        for (int rr = 0; rr < border; rr++)
            for (int cc = 0; cc < border; cc++) T.put(cfa(rr, cc), t.rrmax + rr, cc, RAW(raw, g, height - rr - 2, border2 - cc) / 65535.f);

    // G at R/B sites, and the frame-wide half plane Gtmp
    for (int rr = 3; rr < rr1 - 3; rr++) {
        const int row = rr + top;
        int cc = 3 + (cfa(rr, 3) & 1);
        const int c = cfa(rr, cc);
        for (int indx = rr * ts + cc; cc < cc1 - 3; cc += 2, indx += 2) T.rgb[1][indx] = g_interp(T, c, indx);
        if (row > -1 && row < height) {
            const int offset = cfa(row, std::max(left + 3, 0)) & 1;
            int col = std::max(left + 3, 0) + offset;
            int indx = rr * ts + 3 - (left < 0 ? (left + 3) : 0) + offset;
            for (; col < std::min(cc1 + left - 3, width); col += 2, indx += 2) Gtmp[(row * width + col) >> 1] = T.rgb[1][indx];
        }
    }

    // filters (L490-538): 4-lane body over cc < cc1 - 10, scalar tail to cc1 - 4
    const float *G = T.rgb[1];
    for (int rr = 4; rr < rr1 - 4; rr++) {
        int cc = 4 + (cfa(rr, 2) & 1);
        const int c = cfa(rr, cc);
        const float *n = T.rgb[c];
        int vend = cc;
        while (vend < cc1 - 10) vend += 8;
        for (int indx = rr * ts + cc; cc < cc1 - 4; cc += 2, indx += 2) {
            const int h = indx >> 1;
            if (cc < vend) {
                const float g0 = G[indx], c0 = n[h];
                T.rbhpfv[h] = std::fabs(std::fabs((g0 - c0) - (G[indx + v4] - n[(indx + v4) >> 1])) +
                                        std::fabs(G[indx - v4] - n[(indx - v4) >> 1] - g0 + c0) -
                                        std::fabs(G[indx - v4] - n[(indx - v4) >> 1] - G[indx + v4] + n[(indx + v4) >> 1]));
                T.rbhpfh[h] = std::fabs(std::fabs((g0 - c0) - (G[indx + 4] - n[(indx + 4) >> 1])) +
                                        std::fabs(G[indx - 4] - n[(indx - 4) >> 1] - g0 + c0) -
                                        std::fabs(G[indx - 4] - n[(indx - 4) >> 1] - G[indx + 4] + n[(indx + 4) >> 1]));
            } else {
                T.rbhpfv[h] = std::fabs(std::fabs((G[indx] - n[h]) - (G[indx + v4] - n[(indx + v4) >> 1])) +
                                        std::fabs((G[indx - v4] - n[(indx - v4) >> 1]) - (G[indx] - n[h])) -
                                        std::fabs((G[indx - v4] - n[(indx - v4) >> 1]) - (G[indx + v4] - n[(indx + v4) >> 1])));
                T.rbhpfh[h] = std::fabs(std::fabs((G[indx] - n[h]) - (G[indx + 4] - n[(indx + 4) >> 1])) +
                                        std::fabs((G[indx - 4] - n[(indx - 4) >> 1]) - (G[indx] - n[h])) -
                                        std::fabs((G[indx - 4] - n[(indx - 4) >> 1]) - (G[indx + 4] - n[(indx + 4) >> 1])));
            }
            const float glpfv = (2.f * G[indx] + G[indx + v2] + G[indx - v2]);
            const float glpfh = (2.f * G[indx] + G[indx + 2] + G[indx - 2]);
            T.rblpfv[h] = 0.25f * std::fabs(glpfv - (2.f * n[h] + n[(indx + v2) >> 1] + n[(indx - v2) >> 1]));
            T.rblpfh[h] = 0.25f * std::fabs(glpfh - (2.f * n[h] + n[(indx + 2) >> 1] + n[(indx - 2) >> 1]));
            T.grblpfv[h] = 0.25f * (glpfv + (2.f * n[h] + n[(indx + v2) >> 1] + n[(indx - v2) >> 1]));
            T.grblpfh[h] = 0.25f * (glpfh + (2.f * n[h] + n[(indx + 2) >> 1] + n[(indx - 2) >> 1]));
        }
    }

    // coefficient sums (L556-629)
    float coeff[2][3][2] = {};
    for (int rr = 8; rr < rr1 - 8; rr++) {
        int cc = 8 + (cfa(rr, 2) & 1);
        int indx = rr * ts + cc;
        const int c = cfa(rr, cc);
        const float *n = T.rgb[c];
        float lane[6][4] = {};
        for (; cc < cc1 - 14; cc += 8, indx += 8)
            for (int l = 0; l < 4; ++l) {
                const int ix = indx + 2 * l, h = ix >> 1;
                const float temp1 = 0.3f * (G[ix + ts + 1] - G[ix - ts - 1]);
                const float temp2 = 0.3f * (G[ix - ts + 1] - G[ix + ts - 1]);
                const float gdiffv = (G[ix + ts] - G[ix - ts]) + (temp1 - temp2);
                const float deltgrb = n[h] - G[ix];
                const float gradwtv = (T.rbhpfv[h] + 0.5f * (T.rbhpfv[h + 1] + T.rbhpfv[h - 1])) * (T.grblpfv[h - v1] + T.grblpfv[h + v1]) /
                                      (eps + 0.1f * (T.grblpfv[h - v1] + T.grblpfv[h + v1]) + T.rblpfv[h - v1] + T.rblpfv[h + v1]);
                lane[0][l] += gradwtv * deltgrb * deltgrb;
                lane[1][l] += gradwtv * gdiffv * deltgrb;
                lane[2][l] += gradwtv * gdiffv * gdiffv;
                const float gdiffh = (G[ix + 1] - G[ix - 1]) + (temp1 + temp2);
                const float gradwth = (T.rbhpfh[h] + 0.5f * (T.rbhpfh[h + v1] + T.rbhpfh[h - v1])) * (T.grblpfh[h - 1] + T.grblpfh[h + 1]) /
                                      (eps + 0.1f * (T.grblpfh[h - 1] + T.grblpfh[h + 1]) + T.rblpfh[h - 1] + T.rblpfh[h + 1]);
                lane[3][l] += gradwth * deltgrb * deltgrb;
                lane[4][l] += gradwth * gdiffh * deltgrb;
                lane[5][l] += gradwth * gdiffh * gdiffh;
            }
        for (int k = 0; k < 6; ++k) coeff[k / 3][k % 3][c >> 1] += (lane[k][0] + lane[k][2]) + (lane[k][1] + lane[k][3]);
        for (; cc < cc1 - 8; cc += 2, indx += 2) {
            const int h = indx >> 1;
            float gdiff = (G[indx + ts] - G[indx - ts]) + 0.3f * (G[indx + ts + 1] - G[indx - ts + 1] + G[indx + ts - 1] - G[indx - ts - 1]);
            const float deltgrb = (n[h] - G[indx]);
            float gradwt = (T.rbhpfv[h] + 0.5f * (T.rbhpfv[h + 1] + T.rbhpfv[h - 1])) * (T.grblpfv[h - v1] + T.grblpfv[h + v1]) /
                           (eps + 0.1f * (T.grblpfv[h - v1] + T.grblpfv[h + v1]) + T.rblpfv[h - v1] + T.rblpfv[h + v1]);
            coeff[0][0][c >> 1] += gradwt * deltgrb * deltgrb;
            coeff[0][1][c >> 1] += gradwt * gdiff * deltgrb;
            coeff[0][2][c >> 1] += gradwt * gdiff * gdiff;
            gdiff = (G[indx + 1] - G[indx - 1]) + 0.3f * (G[indx + 1 + ts] - G[indx - 1 + ts] + G[indx + 1 - ts] - G[indx - 1 - ts]);
            gradwt = (T.rbhpfh[h] + 0.5f * (T.rbhpfh[h + v1] + T.rbhpfh[h - v1])) * (T.grblpfh[h - 1] + T.grblpfh[h + 1]) /
                     (eps + 0.1f * (T.grblpfh[h - 1] + T.grblpfh[h + 1]) + T.rblpfh[h - 1] + T.rblpfh[h + 1]);
            coeff[1][0][c >> 1] += gradwt * deltgrb * deltgrb;
            coeff[1][1][c >> 1] += gradwt * gdiff * deltgrb;
            coeff[1][2][c >> 1] += gradwt * gdiff * gdiff;
        }
    }
    for (int dir = 0; dir < 2; dir++)
        for (int k = 0; k < 3; k++)
            for (int c = 0; c < 2; c++) {
                coeff[dir][k][c] *= 0.25f;
                if (k == 1) coeff[dir][k][c] *= 0.3125f;
                else if (k == 2) coeff[dir][k][c] *= SQR(0.3125f);
            }
    const int blk = t.vblock * g.hblsz + t.hblock;
    for (int c = 0; c < 2; c++)
        for (int dir = 0; dir < 2; dir++) {
            float shift;
            if (coeff[dir][2][c] > eps2) {
                shift = coeff[dir][1][c] / coeff[dir][2][c];
                blockwt[blk] = coeff[dir][2][c] / (eps + coeff[dir][0][c]);
            } else {
                shift = 17.0;
                blockwt[blk] = 0;
            }
            if (std::fabs(shift) < 2.0f) {
                blockave[dir][c] += shift;
                blocksqave[dir][c] += SQR(shift);
                blockdenom[dir][c] += 1;
            }
            blockshifts[blk][c][dir] = shift;
        }
}

// ------------------------------------------------------------------------------------------------ fit (L693-837)
bool fit(const Geo &g, float *blockwt, float (*blockshifts)[2][2], float blockave[2][2], float blocksqave[2][2], float blockdenom[2][2],
         double fitparams[2][2][16], int *polyord_out)
{
    const int vblsz = g.vblsz, hblsz = g.hblsz;
    constexpr float caAutostrength = 8.f;
    bool pp = true;
    float blockvar[2][2] = {};
    for (int dir = 0; dir < 2; dir++)
        for (int c = 0; c < 2; c++) {
            if (blockdenom[dir][c]) blockvar[dir][c] = blocksqave[dir][c] / blockdenom[dir][c] - SQR(blockave[dir][c] / blockdenom[dir][c]);
            else { pp = false; break; }
        }
    int polyord = 4, numpar = 16;
    *polyord_out = polyord;
    if (!pp) return false;
    for (int vb = 1; vb < vblsz - 1; vb++)
        for (int c = 0; c < 2; c++)
            for (int i = 0; i < 2; i++) {
                blockshifts[vb * hblsz][c][i] = blockshifts[vb * hblsz + 2][c][i];
                blockshifts[vb * hblsz + hblsz - 1][c][i] = blockshifts[vb * hblsz + hblsz - 3][c][i];
            }
    for (int hb = 0; hb < hblsz; hb++)
        for (int c = 0; c < 2; c++)
            for (int i = 0; i < 2; i++) {
                blockshifts[hb][c][i] = blockshifts[2 * hblsz + hb][c][i];
                blockshifts[(vblsz - 1) * hblsz + hb][c][i] = blockshifts[(vblsz - 3) * hblsz + hb][c][i];
            }
    static double polymat[2][2][256], shiftmat[2][2][16];
    std::memset(polymat, 0, sizeof polymat);
    std::memset(shiftmat, 0, sizeof shiftmat);
    int numblox[2] = {0, 0};
    for (int vb = 1; vb < vblsz - 1; vb++)
        for (int hb = 1; hb < hblsz - 1; hb++)
            for (int c = 0; c < 2; c++) {
                float bstemp[2];
                for (int dir = 0; dir < 2; dir++) {
                    std::array<float, 9> p;
                    int k = 0;
                    for (int dv = -1; dv <= 1; ++dv)
                        for (int dh = -1; dh <= 1; ++dh) p[k++] = blockshifts[(vb + dv) * hblsz + hb + dh][c][dir];
                    bstemp[dir] = median9(p);
                }
                if (SQR(bstemp[0]) > caAutostrength * blockvar[0][c] || SQR(bstemp[1]) > caAutostrength * blockvar[1][c]) continue;
                numblox[c]++;
                const double bw = blockwt[vb * hblsz + hb];
                for (int dir = 0; dir < 2; dir++) {
                    double pvi = 1.0;
                    for (int i = 0; i < polyord; i++) {
                        double phi = 1.0;
                        for (int j = 0; j < polyord; j++) {
                            double pv = pvi;
                            for (int m = 0; m < polyord; m++) {
                                double ph = phi;
                                for (int n = 0; n < polyord; n++) {
                                    polymat[c][dir][numpar * (polyord * i + j) + (polyord * m + n)] += pv * ph * bw;
                                    ph *= hb;
                                }
                                pv *= vb;
                            }
                            shiftmat[c][dir][(polyord * i + j)] += pvi * phi * (double)bstemp[dir] * bw;
                            phi *= hb;
                        }
                        pvi *= vb;
                    }
                }
            }
    numblox[1] = std::min(numblox[0], numblox[1]);
    if (numblox[1] < 32) {
        polyord = 2;
        numpar = 4;
        if (numblox[1] < 10) pp = false;
    }
    *polyord_out = polyord;
    if (pp)
        for (int c = 0; c < 2; c++)
            for (int dir = 0; dir < 2; dir++)
                if (!lin_eq_solve(numpar, polymat[c][dir], shiftmat[c][dir], fitparams[c][dir])) pp = false;
    return pp;
}

// ------------------------------------------------------------------------------------------------ pass 2 (L850-1250)
void pass2_tile(const float *raw, const Geo &g, const Cfa &cfa, const TileBox &t, Tile &T, const float *Gtmp, float *RawDataTmp,
                bool autoCA, double cared, double cablue, const double fitparams[2][2][16], int polyord)
{
    T.clear();
    const int rr1 = t.rr1, cc1 = t.cc1, top = t.top, left = t.left;
    const int height = g.height, width = g.width;
    float *G = T.rgb[1];
    float *grbdiff = T.rbhpfh, *gshift = T.rbhpfv;
    for (int rr = t.rrmin; rr < t.rrmax; rr++) {
        const int row = rr + top;
        for (int cc = t.ccmin; cc < t.ccmax; cc++) {
            const int col = cc + left, c = cfa(rr, cc);
            T.put(c, rr, cc, RAW(raw, g, row, col) / 65535.f);
            if ((c & 1) == 0) G[rr * ts + cc] = Gtmp[(row * width + col) >> 1];
        }
    }
    if (t.rrmin > 0)
        for (int rr = 0; rr < border; rr++)
            for (int cc = t.ccmin; cc < t.ccmax; cc++) {
                const int c = cfa(rr, cc);
                T.put(c, rr, cc, T.get(c, border2 - rr, cc));
                G[rr * ts + cc] = G[(border2 - rr) * ts + cc];
            }
    if (t.rrmax < rr1)
        for (int rr = 0; rr < std::min(border, rr1 - t.rrmax); rr++)
            for (int cc = t.ccmin; cc < t.ccmax; cc++) {
                const int c = cfa(rr, cc);
                T.put(c, t.rrmax + rr, cc, RAW(raw, g, height - rr - 2, left + cc) / 65535.f);
                if ((c & 1) == 0) G[(t.rrmax + rr) * ts + cc] = Gtmp[((height - rr - 2) * width + left + cc) >> 1];
            }
    if (t.ccmin > 0)
        for (int rr = t.rrmin; rr < t.rrmax; rr++)
            for (int cc = 0; cc < border; cc++) {
                const int c = cfa(rr, cc);
                T.put(c, rr, cc, T.get(c, rr, border2 - cc));
                G[rr * ts + cc] = G[rr * ts + border2 - cc];
            }
    if (t.ccmax < cc1)
        for (int rr = t.rrmin; rr < t.rrmax; rr++)
            for (int cc = 0; cc < std::min(border, cc1 - t.ccmax); cc++) {
                const int c = cfa(rr, cc);
                T.put(c, rr, t.ccmax + cc, RAW(raw, g, top + rr, width - cc - 2) / 65535.f);
                if ((c & 1) == 0) G[rr * ts + t.ccmax + cc] = Gtmp[((top + rr) * width + (width - cc - 2)) >> 1];
            }
    if (t.rrmin > 0 && t.ccmin > 0)
        for (int rr = 0; rr < border; rr++)
            for (int cc = 0; cc < border; cc++) {
                const int c = cfa(rr, cc);
                T.put(c, rr, cc, RAW(raw, g, border2 - rr, border2 - cc) / 65535.f);
                if ((c & 1) == 0) G[rr * ts + cc] = Gtmp[((border2 - rr) * width + border2 - cc) >> 1];
            }
    if (t.rrmax < rr1 && t.ccmax < cc1)
        for (int rr = 0; rr < std::min(border, rr1 - t.rrmax); rr++)
            for (int cc = 0; cc < std::min(border, cc1 - t.ccmax); cc++) {
                const int c = cfa(rr, cc);
                T.put(c, t.rrmax + rr, t.ccmax + cc, RAW(raw, g, height - rr - 2, width - cc - 2) / 65535.f);
                if ((c & 1) == 0) G[(t.rrmax + rr) * ts + t.ccmax + cc] = Gtmp[((height - rr - 2) * width + (width - cc - 2)) >> 1];
            }
    if (t.rrmin > 0 && t.ccmax < cc1)
        for (int rr = 0; rr < border; rr++)
            for (int cc = 0; cc < std::min(border, cc1 - t.ccmax); cc++) {
                const int c = cfa(rr, cc);
                T.put(c, rr, t.ccmax + cc, RAW(raw, g, border2 - rr, width - cc - 2) / 65535.f);
                if ((c & 1) == 0) G[rr * ts + t.ccmax + cc] = Gtmp[((border2 - rr) * width + (width - cc - 2)) >> 1];
            }
    if (t.rrmax < rr1 && t.ccmin > 0)
        for (int rr = 0; rr < std::min(border, rr1 - t.rrmax); rr++)
            for (int cc = 0; cc < border; cc++) {
                const int c = cfa(rr, cc);
                T.put(c, t.rrmax + rr, cc, RAW(raw, g, height - rr - 2, border2 - cc) / 65535.f);
                if ((c & 1) == 0) G[(t.rrmax + rr) * ts + cc] = Gtmp[((height - rr - 2) * width + (border2 - cc)) >> 1];
            }

    if (!autoCA)
        for (int rr = 3; rr < rr1 - 3; rr++) {
            int cc = 3 + cfa(rr, 1);
            const int c = cfa(rr, cc);
            for (int indx = rr * ts + cc; cc < cc1 - 3; cc += 2, indx += 2) G[indx] = g_interp(T, c, indx);
        }

    float lbs[2][2];
    if (!autoCA) {
        const float hfrac = -((float)(t.hblock - 0.5) / (g.hblsz - 2) - 0.5);
        const float vfrac = -((float)(t.vblock - 0.5) / (g.vblsz - 2) - 0.5) * height / width;
        lbs[0][0] = 2 * vfrac * cared;
        lbs[0][1] = 2 * hfrac * cared;
        lbs[1][0] = 2 * vfrac * cablue;
        lbs[1][1] = 2 * hfrac * cablue;
        // no limit in the reference; past +-60 px its G reads would leave rgb[0] .. rgb[2] (held there, as the device does)
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) lbs[a][b] = fmax_(-60.f, fmin_(lbs[a][b], 60.f));
    } else {
        lbs[0][0] = lbs[0][1] = lbs[1][0] = lbs[1][1] = 0;
        double pv = 1.0;
        for (int i = 0; i < polyord; i++) {
            double ph = pv;
            for (int j = 0; j < polyord; j++) {
                lbs[0][0] += ph * fitparams[0][0][polyord * i + j];
                lbs[0][1] += ph * fitparams[0][1][polyord * i + j];
                lbs[1][0] += ph * fitparams[1][0][polyord * i + j];
                lbs[1][1] += ph * fitparams[1][1][polyord * i + j];
                ph *= t.hblock;
            }
            pv *= t.vblock;
        }
        constexpr float bslim = 3.99;
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) lbs[a][b] = fmax_(-bslim, fmin_(lbs[a][b], bslim));
    }
    int GRBdir[2][3], shifthfloor[3], shiftvfloor[3], shifthceil[3], shiftvceil[3];
    float shifthfrac[3], shiftvfrac[3];
    for (int c = 0; c < 3; c += 2) {
        shiftvfloor[c] = std::floor((float)lbs[c >> 1][0]);
        shiftvceil[c] = std::ceil((float)lbs[c >> 1][0]);
        if (lbs[c >> 1][0] < 0.f) std::swap(shiftvfloor[c], shiftvceil[c]);
        shiftvfrac[c] = std::fabs(lbs[c >> 1][0] - shiftvfloor[c]);
        shifthfloor[c] = std::floor((float)lbs[c >> 1][1]);
        shifthceil[c] = std::ceil((float)lbs[c >> 1][1]);
        if (lbs[c >> 1][1] < 0.f) std::swap(shifthfloor[c], shifthceil[c]);
        shifthfrac[c] = std::fabs(lbs[c >> 1][1] - shifthfloor[c]);
        GRBdir[0][c] = lbs[c >> 1][0] > 0 ? 2 : -2;
        GRBdir[1][c] = lbs[c >> 1][1] > 0 ? 2 : -2;
    }
    for (int rr = 4; rr < rr1 - 4; rr++) {
        int cc = 4 + (cfa(rr, 2) & 1);
        const int c = cfa(rr, cc);
        int indx = (rr * ts + cc) >> 1;
        int indxfc = (rr + shiftvfloor[c]) * ts + cc + shifthceil[c];
        int indxff = (rr + shiftvfloor[c]) * ts + cc + shifthfloor[c];
        int indxcc = (rr + shiftvceil[c]) * ts + cc + shifthceil[c];
        int indxcf = (rr + shiftvceil[c]) * ts + cc + shifthfloor[c];
        for (; cc < cc1 - 4; cc += 2, indxfc += 2, indxff += 2, indxcc += 2, indxcf += 2, ++indx) {
            const float Ginthfloor = intp(shifthfrac[c], G[indxfc], G[indxff]);
            const float Ginthceil = intp(shifthfrac[c], G[indxcc], G[indxcf]);
            const float Gint = intp(shiftvfrac[c], Ginthceil, Ginthfloor);
            grbdiff[indx] = Gint - T.rgb[c][indx];
            gshift[indx] = Gint;
        }
    }
    shifthfrac[0] /= 2.f; shifthfrac[2] /= 2.f; shiftvfrac[0] /= 2.f; shiftvfrac[2] /= 2.f;
    for (int rr = 8; rr < rr1 - 8; rr++) {
        int cc = 8 + (cfa(rr, 2) & 1);
        const int c = cfa(rr, cc);
        const int d0 = GRBdir[0][c], d1 = GRBdir[1][c];
        float *n = T.rgb[c];
        for (int indx = rr * ts + cc; cc < cc1 - 8; cc += 2, indx += 2) {
            const float grbdiffold = G[indx] - n[indx >> 1];
            const float hf = intp(shifthfrac[c], grbdiff[(indx - d1) >> 1], grbdiff[indx >> 1]);
            const float hc = intp(shifthfrac[c], grbdiff[((rr - d0) * ts + cc - d1) >> 1], grbdiff[((rr - d0) * ts + cc) >> 1]);
            float grbdiffint = intp(shiftvfrac[c], hc, hf);
            const float RBint = G[indx] - grbdiffint;
            if (std::fabs(RBint - n[indx >> 1]) < 0.25f * (RBint + n[indx >> 1])) {
                if (std::fabs(grbdiffold) > std::fabs(grbdiffint)) n[indx >> 1] = RBint;
            } else {
                const float p0 = 1.f / (eps + std::fabs(G[indx] - gshift[indx >> 1]));
                const float p1 = 1.f / (eps + std::fabs(G[indx] - gshift[(indx - d1) >> 1]));
                const float p2 = 1.f / (eps + std::fabs(G[indx] - gshift[((rr - d0) * ts + cc) >> 1]));
                const float p3 = 1.f / (eps + std::fabs(G[indx] - gshift[((rr - d0) * ts + cc - d1) >> 1]));
                grbdiffint = (p0 * grbdiff[indx >> 1] + p1 * grbdiff[(indx - d1) >> 1] + p2 * grbdiff[((rr - d0) * ts + cc) >> 1] +
                              p3 * grbdiff[((rr - d0) * ts + cc - d1) >> 1]) / (p0 + p1 + p2 + p3);
                if (std::fabs(grbdiffold) > std::fabs(grbdiffint)) n[indx >> 1] = G[indx] - grbdiffint;
            }
            if (grbdiffold * grbdiffint < 0) n[indx >> 1] = G[indx] - 0.5f * (grbdiffold + grbdiffint);
        }
    }
    for (int rr = border; rr < rr1 - border; rr++) {
        const int c = cfa(rr + top, left + border + (cfa(rr + top, 2) & 1));
        const int row = rr + top;
        const int cc = border + (cfa(rr, 2) & 1);
        int indx = (row * width + cc + left) >> 1;
        int indx1 = (rr * ts + cc) >> 1;
        for (; indx < (row * width + cc1 - border + left) >> 1; indx++, indx1++) RawDataTmp[indx] = 65535.f * T.rgb[c][indx1];
    }
}

template <typename F>
void for_tiles(const Geo &g, F f)
{
    for (int top = -border; top < g.height; top += ts - border2)
        for (int left = -border; left < g.width - (g.W & 1); left += ts - border2) f(tile_box(g, top, left));
}

} // namespace

extern "C" {

// sizes: [0] Gtmp / RawDataTmp floats each (H * width / 2), [1] blockwt + blockshifts floats (vblsz * hblsz * 5),
// [2] factor plane width, [3] factor plane height, [4] oldraw width, [5] oldraw height, [6] vblsz, [7] hblsz
void ca_ref_sizes(int W, int H, int out[8])
{
    const Geo g = geometry(W, H);
    out[0] = (int)((size_t)g.height * g.width / 2);
    out[1] = g.vblsz * g.hblsz * 5;
    out[2] = (W + 1 - 2 * cb) / 2;
    out[3] = (H + 1 - 2 * cb) / 2;
    out[4] = (W + 1 - 2 * cb) / 2;
    out[5] = H - 2 * cb;
    out[6] = g.vblsz;
    out[7] = g.hblsz;
}

// the colour-shift guard's copy of the non-green samples before the correction (L168-181)
void ca_ref_capture(const float *raw, int W, int H, unsigned filters, float *oldraw)
{
    const Cfa cfa = make_cfa(filters);
    const int ow = (W + 1 - 2 * cb) / 2;
    for (int i = cb; i < H - cb; ++i)
        for (int j = cb + (cfa(i, 0) & 1); j < W - cb; j += 2) oldraw[(size_t)(i - cb) * ow + (j - cb) / 2] = raw[(size_t)i * W + j];
}

// one iteration of the correction loop body up to the colour-shift guard: pass 1 + fit (auto) and pass 2 + copy back, in place on
// raw.  blocks (vblsz * hblsz * 5 floats) is zeroed by the caller once per call, like the reference (L208); Gtmp / RawDataTmp and
// fitparams (64 doubles, [c][dir][16]) persist across iterations.  Returns processpasstwo; *polyord_out gets the fit order.
int ca_ref_iteration(float *raw, int W, int H, unsigned filters, int autoCA, double cared, double cablue, float *Gtmp, float *RawDataTmp,
                     float *blocks, double *fitparams_flat, int *polyord_out)
{
    const Cfa cfa = make_cfa(filters);
    const Geo g = geometry(W, H);
    float *blockwt = blocks;
    float(*blockshifts)[2][2] = (float(*)[2][2])(blocks + g.vblsz * g.hblsz);
    double(*fitparams)[2][16] = (double(*)[2][16])fitparams_flat;
    Tile T;
    bool pp = true;
    int polyord = 4;
    if (autoCA) {
        float blockave[2][2] = {}, blocksqave[2][2] = {}, blockdenom[2][2] = {};
        for_tiles(g, [&](const TileBox &t) { pass1_tile(raw, g, cfa, t, T, Gtmp, blockwt, blockshifts, blockave, blocksqave, blockdenom); });
        pp = fit(g, blockwt, blockshifts, blockave, blocksqave, blockdenom, fitparams, &polyord);
    }
    *polyord_out = polyord;
    if (!pp) return 0;
    for_tiles(g, [&](const TileBox &t) { pass2_tile(raw, g, cfa, t, T, Gtmp, RawDataTmp, autoCA != 0, cared, cablue, fitparams, polyord); });
    for (int row = cb; row < g.height - cb; row++) {
        int col = cb + (cfa(row, 0) & 1);
        int indx = (row * g.width + col) >> 1;
        for (; col < g.width - cb; col += 2, indx++) raw[(size_t)row * W + col] = std::max(0.f, RawDataTmp[indx]);
    }
    return 1;
}

// factor planes of the colour-shift guard (L1293-1335), before the blur; red / blue are fw x fh
void ca_ref_factors(const float *raw, const float *oldraw, int W, int H, unsigned filters, float *red, float *blue)
{
    const Cfa cfa = make_cfa(filters);
    const int fw = (W + 1 - 2 * cb) / 2, fh = (H + 1 - 2 * cb) / 2, ow = (W + 1 - 2 * cb) / 2;
    for (int i = 0; i < H - 2 * cb; ++i) {
        const int firstCol = cfa(i, 0) & 1;
        const int colour = cfa(i, firstCol);
        float *ng = colour == 0 ? red : blue;
        for (int j = firstCol; j < W - 2 * cb; j += 2) {
            const float nv = raw[(size_t)(i + cb) * W + j + cb], ov = oldraw[(size_t)i * ow + j / 2];
            ng[(size_t)(i / 2) * fw + j / 2] = (nv <= 1.f || ov <= 1.f) ? 1.f : fmax_(0.5f, fmin_(ov / nv, 2.f));
        }
    }
    if (H % 2)
        for (int j = 0; j < fw; ++j) {
            red[(size_t)(fh - 1) * fw + j] = red[(size_t)(fh - 2) * fw + j];
            blue[(size_t)(fh - 1) * fw + j] = blue[(size_t)(fh - 2) * fw + j];
        }
    if (W % 2) {
        const int ngRow = 1 - (cfa(0, 0) & 1);
        const int ngCol = cfa(ngRow, 0) & 1;
        float *ng = cfa(ngRow, ngCol) == 0 ? red : blue;
        for (int i = 0; i < fh; ++i) ng[(size_t)i * fw + fw - 1] = ng[(size_t)i * fw + fw - 2];
    }
}

// raw *= blurred factors (L1345-1352)
void ca_ref_apply(float *raw, int W, int H, unsigned filters, const float *red, const float *blue)
{
    const Cfa cfa = make_cfa(filters);
    const int fw = (W + 1 - 2 * cb) / 2;
    for (int i = 0; i < H - 2 * cb; ++i) {
        const int firstCol = cfa(i, 0) & 1;
        const float *ng = cfa(i, firstCol) == 0 ? red : blue;
        for (int j = firstCol; j < W - 2 * cb; j += 2) raw[(size_t)(i + cb) * W + j + cb] *= ng[(size_t)(i / 2) * fw + j / 2];
    }
}

} // extern "C"
