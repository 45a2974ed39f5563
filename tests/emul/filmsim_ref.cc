// tests/emul/filmsim_ref.cc -- CPU checker for artgpu_film_simulation: CLUTApplication's HaldCLUT path (rtengine/clutstore.cc:1502-1615
// CLUTApplication::do_apply) over HaldCLUT::getRGB in its __SSE2__ form (clutstore.cc:178-288, getClutValues L104-131), restated serially row
// by row with the reference's line buffers.  Test infrastructure only; built on first use with -ffp-contract=off.
//
// The leaves are liboracle's restatements of LUTf::operator[](float): oracle_lutf for a table that clips on both sides (Color::gamma2curve)
// and oracle_lutf_noclip for one constructed with flags 0 (Color::igammatab_srgb).  clutstore.cc itself needs lcms2, glibmm and the image
// classes and is not compiled anywhere: the loop is parity-unpinned, its leaves are pinned.
// The 4-wide loops (L1518-1532, L1581-1595; vintpf and the vfloat overloads of Color::rgbxyz / Color::xyz2rgb) are written lane by lane in
// float, the tails (L1536-1544, L1599-1607) with the double matrices.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

extern "C" {
float oracle_lutf(const float *data, int size, float index);
float oracle_lutf_noclip(const float *data, int size, float index);
}

extern "C" {
struct fs_ref_params {             // the layout of artgpu_film_simulation_params
    float strength;
    int32_t same_profile;
    double work_to_xyz[9], xyz_to_clut[9], clut_to_xyz[9], xyz_to_work[9];
};
struct fs_ref_counts {
    long long body, tail;                          // pixels converted by the 4-wide and by the scalar form (both zero with same_profile)
    long long below_zero, above_max;               // gamma_srgbclipped: channel values below 0 / above 65535
    long long at_max, frac_one;                    // getRGB: encoded values of exactly 65535 / channel fractions of exactly 1
    long long cell_first[3], cell_last[3];         // per axis: channel values in cell 0 / in cell level - 2
    long long igamma_below, igamma_above;          // igamma_srgb: lookups below 0 / above 65535
};
}

namespace {

inline float vintpf(float a, float b, float c) { return a * b + (1.f - a) * c; }       // sleefsseavx.h:1435-1442

struct Tables {
    std::vector<float> gamma, igamma;
    Tables() : gamma(65536), igamma(65536)
    {
        // Color::init (color.cc:239-255) with gamma2 / igamma2 (color.h:1122-1147)
        for (int i = 0; i < 65536; i++) {
            const double x = i / 65535.0;
            gamma[i] = x <= 0.003040 ? x * 12.92310 : 1.055 * std::exp(std::log(x) / 2.4) - 0.055;
        }
        for (int i = 0; i < 65536; i++) gamma[i] *= 65535.f;
        for (int i = 0; i < 65536; i++) {
            const double x = i / 65535.0;
            igamma[i] = x <= 0.039286 ? x / 12.92310 : std::exp(std::log((x + 0.055) / 1.055) * 2.4);
        }
        for (int i = 0; i < 65536; i++) igamma[i] *= 65535.f;
    }
};
const Tables &tables() { static const Tables t; return t; }

// Color::rgbxyz then Color::xyz2rgb: the vfloat overloads, one lane (color.cc:841-846, 888-893) ...
void convert_v(float &r, float &g, float &b, const float m1[9], const float m2[9])
{
    const float x = m1[0] * r + m1[1] * g + m1[2] * b;
    const float y = m1[3] * r + m1[4] * g + m1[5] * b;
    const float z = m1[6] * r + m1[7] * g + m1[8] * b;
    r = m2[0] * x + m2[1] * y + m2[2] * z;
    g = m2[3] * x + m2[4] * y + m2[5] * z;
    b = m2[6] * x + m2[7] * y + m2[8] * z;
}
// ... and the scalar overloads with double matrices (color.cc:826-831, 849-878)
void convert_s(float &r, float &g, float &b, const double m1[9], const double m2[9])
{
    const float x = m1[0] * r + m1[1] * g + m1[2] * b;
    const float y = m1[3] * r + m1[4] * g + m1[5] * b;
    const float z = m1[6] * r + m1[7] * g + m1[8] * b;
    r = m2[0] * x + m2[1] * y + m2[2] * z;
    g = m2[3] * x + m2[4] * y + m2[5] * z;
    b = m2[6] * x + m2[7] * y + m2[8] * z;
}

} // namespace

extern "C" {

int fs_ref_sizes(int which) { return which == 0 ? (int)sizeof(fs_ref_params) : (int)sizeof(fs_ref_counts); }

void fs_ref_tables(float *gamma, float *igamma)
{
    std::copy(tables().gamma.begin(), tables().gamma.end(), gamma);
    std::copy(tables().igamma.begin(), tables().igamma.end(), igamma);
}

// 0: done; 2: bad arguments.  `cells` (or null): 3 * W * H ints, the cell each channel of each pixel landed in
int fs_ref_tool(float *R, float *G, float *B, int W, int H, const uint16_t *table, int level, int channels, const fs_ref_params *p, fs_ref_counts *cn, int32_t *cells)
{
    fs_ref_counts dummy = {};
    if (!cn) cn = &dummy;
    bool level_ok = false;
    for (int k = 2; k <= 16; ++k) level_ok = level_ok || level == k * k;
    if (!R || !G || !B || !table || !p || W < 1 || H < 1 || !level_ok || (channels != 3 && channels != 4)) return 2;
    const Tables &t = tables();
    // loadFile's buffer (clutstore.cc:83-96): RGBX, "loads one pixel in advance"
    const size_t n = (size_t)level * level * level;
    std::vector<uint16_t> image(n * 4 + 4, 0);
    for (size_t i = 0; i < n; ++i)
        for (int c = 0; c < 3; ++c) image[i * 4 + c] = table[i * channels + c];
    const unsigned ulevel = level, level_square = ulevel * ulevel;
    const float flevel_minus_one = static_cast<float>(level - 1) / 65535.0f, flevel_minus_two = static_cast<float>(level - 2);      // L155-156
    const float strength = p->strength;
    float mf[4][9];
    const double *md[4] = {p->work_to_xyz, p->xyz_to_clut, p->clut_to_xyz, p->xyz_to_work};
    for (int k = 0; k < 4; ++k)
        for (int i = 0; i < 9; ++i) mf[k][i] = md[k][i];                              // F2V(wprof_[i][j]) (L1100-1107)
    std::vector<float> clutr(W), clutg(W), clutb(W), out_rgbx(4 * (size_t)W);
    for (int y = 0; y < H; ++y) {
        float *r = R + (size_t)y * W, *g = G + (size_t)y * W, *b = B + (size_t)y * W;
        for (int j = 0; j < W; ++j) { clutr[j] = r[j]; clutg[j] = g[j]; clutb[j] = b[j]; }
        if (!p->same_profile) {
            int j = 0;
            for (; j < W - 3; j += 4)
                for (int k = 0; k < 4; ++k) { convert_v(clutr[j + k], clutg[j + k], clutb[j + k], mf[0], mf[1]); ++cn->body; }
            for (; j < W; j++) { convert_s(clutr[j], clutg[j], clutb[j], md[0], md[1]); ++cn->tail; }
        }
        for (int j = 0; j < W; j++) {                                                  // L1551-1560
            float *v[3] = {&clutr[j], &clutg[j], &clutb[j]};
            for (int c = 0; c < 3; ++c) {
                if (*v[c] < 0.f) ++cn->below_zero;
                if (*v[c] > 65535.f) ++cn->above_max;
                *v[c] = oracle_lutf(t.gamma.data(), 65536, *v[c]);
            }
        }
        // HaldCLUT::getRGB(strength_, W, clutr, clutg, clutb, out_rgbx), the __SSE2__ form
        for (int j = 0; j < W; ++j) {
            const float in[3] = {clutr[j], clutg[j], clutb[j]};
            unsigned cell[3];
            float frac[3];
            for (int c = 0; c < 3; ++c) {
                cell[c] = std::min(flevel_minus_two, in[c] * flevel_minus_one);                              // L196-198
                const float v_tmp = in[c] * flevel_minus_one;                                                // L250
                const float lim = v_tmp < flevel_minus_two ? v_tmp : flevel_minus_two;                       // vminf
                frac[c] = v_tmp - (float)(int)lim;                                                           // _mm_cvtepi32_ps(_mm_cvttps_epi32(.))
                if (in[c] == 65535.f) ++cn->at_max;
                if (frac[c] == 1.f) ++cn->frac_one;
                if (cell[c] == 0) ++cn->cell_first[c];
                if (cell[c] == ulevel - 2) ++cn->cell_last[c];
                if (cells) cells[((size_t)y * W + j) * 3 + c] = (int32_t)cell[c];
            }
            const unsigned color = cell[0] + cell[1] * ulevel + cell[2] * level_square;
            const auto value = [&](size_t index, int c, int next) -> float { return (float)image[index + 4 * next + c]; };      // getClutValues: .x, .y
            for (int c = 0; c < 3; ++c) {
                size_t index = (size_t)color * 4;
                float v_tmp1 = vintpf(frac[0], value(index, c, 1), value(index, c, 0));                      // L258
                index = ((size_t)color + ulevel) * 4;
                float v_tmp2 = vintpf(frac[0], value(index, c, 1), value(index, c, 0));                      // L263
                float v_out = vintpf(frac[1], v_tmp2, v_tmp1);                                               // L267
                index = ((size_t)color + level_square) * 4;
                v_tmp1 = vintpf(frac[0], value(index, c, 1), value(index, c, 0));                            // L272
                index = ((size_t)color + ulevel + level_square) * 4;
                v_tmp2 = vintpf(frac[0], value(index, c, 1), value(index, c, 0));                            // L277
                v_tmp1 = vintpf(frac[1], v_tmp2, v_tmp1);                                                    // L279
                v_out = vintpf(frac[2], v_tmp1, v_out);                                                      // L283
                out_rgbx[(size_t)j * 4 + c] = vintpf(strength, v_out, in[c]);                                // L285
            }
        }
        for (int j = 0; j < W; j++) {                                                  // L1564-1573
            float *v[3] = {&clutr[j], &clutg[j], &clutb[j]};
            for (int c = 0; c < 3; ++c) {
                const float x = out_rgbx[(size_t)j * 4 + c];
                if (x < 0.f) ++cn->igamma_below;
                if (x > 65535.f) ++cn->igamma_above;
                *v[c] = oracle_lutf_noclip(t.igamma.data(), 65536, x);
            }
        }
        if (!p->same_profile) {
            int j = 0;
            for (; j < W - 3; j += 4)
                for (int k = 0; k < 4; ++k) convert_v(clutr[j + k], clutg[j + k], clutb[j + k], mf[2], mf[3]);
            for (; j < W; j++) convert_s(clutr[j], clutg[j], clutb[j], md[2], md[3]);
        }
        for (int j = 0; j < W; j++) { r[j] = clutr[j]; g[j] = clutg[j]; b[j] = clutb[j]; }
    }
    return 0;
}

} // extern "C"
