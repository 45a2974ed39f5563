// tests/emul/local_contrast_ref.cc -- CPU checker for artgpu_local_contrast: what local_contrast_wavelets does between its
// wavelet_decomposition and its reconstruct (rtengine/iplocalcontrast.cc:268-417), restated in the reference's serial order on the
// bands and coeff0 of the oracle's decomposition (tests/lc_lib.py wraps it in oracle_wavelet_decompose / _reconstruct).
// Test infrastructure only; built on first use with -ffp-contract=off -msse2 (rtengine is built without contraction).
//
// xlogf, xexpf and LUTf::operator[](float) are liboracle's pinned restatements (oracle_xlogf_s, oracle_xexpf_s, oracle_lutf), not a
// third copy.
//
// log(MaxP[level]), log(insigma), log(rapX) (L373-376): the argument is a float, the result is assigned to a float.  Conclusion on the
// overload: the double one.  The calls are unqualified inside namespace rtengine; rtengine's own include chain from
// iplocalcontrast.cc (improcfun.h, gauss.h, array2D.h, cplx_wavelet_dec.h, curves.h, masks.h and what they include) reaches <cmath>
// only -- rng.h and boxblur.h, the two rtengine headers that include <math.h>, are not on it -- and libstdc++'s <cmath> declares
// log(float) in namespace std alone, so ::log(double) from the C header is the one candidate: the float is widened, the double result
// narrowed.  The float overload would be reached only if a system header on the chain included <math.h> itself (libstdc++'s wrapper
// of that name adds `using std::log;` to the global namespace).  lcms2.h, the candidate named in the feature request, includes
// stdio.h, limits.h, time.h and stddef.h (math.h is in lcms2_plugin.h, which rtengine does not include); the glib / gtk headers
// could not be inspected for this.  One function below (ref_log) holds the choice; art_amd/csrc/localcontrast.hip makes the same one.
#include <cfloat>
#include <cmath>
#include <cstdint>

extern "C" {
float oracle_xlogf_s(float d);
float oracle_xexpf_s(float d);
float oracle_lutf(const float *data, int size, float index);
}

namespace {
inline float ref_log(float x) { return (float)std::log((double)x); }
template <typename T> inline const T &rt_min(const T &a, const T &b) { return b < a ? b : a; }   // rt_math.h:55-58
template <typename T> inline const T &rt_max(const T &a, const T &b) { return a < b ? b : a; }   // rt_math.h:73-76
inline float SQR(float x) { return x * x; }

// eval_avg (L97-156), positive side
void eval_avg(const float *DataList, int datalen, float &averagePlus, float &max)
{
    int countP = 0;
    double averaP = 0.0;
    const float thres = 5.f;
    max = 0.f;
    float lmax = 0.f;
    for (int i = 0; i < datalen; i++) {
        if (DataList[i] >= thres) {
            averaP += DataList[i];
            if (DataList[i] > lmax) lmax = DataList[i];
            countP++;
        }
    }
    max = max > lmax ? max : lmax;
    if (countP > 0) averagePlus = averaP / countP;
    else averagePlus = 0;
}

// eval_sigma (L159-189), positive side
void eval_sigma(const float *DataList, int datalen, float averagePlus, float &sigmaPlus)
{
    int countP = 0;
    double variP = 0.0;
    const float thres = 5.f;
    for (int i = 0; i < datalen; i++) {
        if (DataList[i] >= thres) {
            variP += SQR(DataList[i] - averagePlus);
            countP++;
        }
    }
    if (countP > 0) sigmaPlus = sqrt(variP / countP);
    else sigmaPlus = 0;
}
} // namespace

extern "C" {

// the layout of artgpu_local_contrast_info
typedef struct {
    int32_t nlevels;
    float ave, min0, max0;
    float mean[10], sigma[10], maxp[10];
} lc_ref_info;

typedef struct {
    long long branch_max;      // |val| >= mean + sigma: the xlogf / xexpf branch
    long long branch_mid;      // |val| >= mean
    long long branch_low;      // below mean
    long long clipped_above;   // lookups LUTf::operator[] clipped at the top (index > 499: the entry 500 is returned)
    long long floor_hits;      // kinterm <= 0 -> 0.01f
    long long c0_skipped;      // coeff0 entries the `< 32768` test left alone
    long long nan_left;        // NaN coefficients left alone
    long long levels_skipped;  // levels whose MaxP / mean / sigma test failed (L371)
} lc_ref_counts;

// wavelet_level = 7, lowered while (1 << wavelet_level) >= min(W, H) and > 1 (L256-260)
int lc_ref_levels(int W, int H)
{
    int wavelet_level = 7;
    int dim = W < H ? W : H;
    while ((1 << wavelet_level) >= dim && wavelet_level > 1) --wavelet_level;
    return wavelet_level;
}

// bands[3 * level + dir - 1] = level_coeffs(level)[dir], each W_L * H_L = n floats, modified in place like coeff0.
// curve: the 501 entries of WavOpacityCurveWL's LUT, NULL = unset (operator[] returns 0).
// stats_in == NULL: the function's own statistics; otherwise ave / min0 / max0 / mean / sigma / maxp are taken from it.
// stats_out receives the statistics used.
void lc_ref_apply(float *const *bands, float *coeff0, int n, int maxlvl, double params_contrast, const float *curve,
                  const lc_ref_info *stats_in, lc_ref_info *stats_out, lc_ref_counts *counts)
{
    lc_ref_info st = {};
    lc_ref_counts cn = {};
    st.nlevels = maxlvl;
    const float contrast = params_contrast;

    if (contrast != 0) {
        float *wl0 = coeff0;
        float maxh = 2.5f;
        float maxl = 2.5f;
        float multL = contrast * (maxl - 1.f) / 100.f + 1.f;
        float multH = contrast * (maxh - 1.f) / 100.f + 1.f;
        double avedbl = 0.0;
        float max0 = 0.f;
        float min0 = FLT_MAX;
        for (int i = 0; i < n; i++) avedbl += wl0[i];
        {
            float lminL = FLT_MAX;
            float lmaxL = 0.f;
            for (int i = 0; i < n; i++) {
                lminL = rt_min(lminL, wl0[i]);
                lmaxL = rt_max(lmaxL, wl0[i]);
            }
            min0 = rt_min(min0, lminL);
            max0 = rt_max(max0, lmaxL);
        }
        float ave = avedbl / double(n);
        if (stats_in) { ave = stats_in->ave; min0 = stats_in->min0; max0 = stats_in->max0; }
        st.ave = ave; st.min0 = min0; st.max0 = max0;
        max0 /= 327.68f;
        min0 /= 327.68f;
        float av = ave / 327.68f;
        float ah = (multH - 1.f) / (av - max0);
        float bh = 1.f - max0 * ah;
        float al = (multL - 1.f) / (av - min0);
        float bl = 1.f - min0 * al;

        if (max0 > 0.0) {
            for (int i = 0; i < n; i++) {
                if (wl0[i] < 32768.f) {
                    float prov;
                    if (wl0[i] > ave) {
                        float kh = ah * (wl0[i] / 327.68f) + bh;
                        prov = wl0[i];
                        wl0[i] = ave + kh * (wl0[i] - ave);
                    } else {
                        float kl = al * (wl0[i] / 327.68f) + bl;
                        prov = wl0[i];
                        wl0[i] = ave - kl * (ave - wl0[i]);
                    }
                    float diflc = wl0[i] - prov;
                    wl0[i] = prov + diflc;
                } else {
                    ++cn.c0_skipped;
                }
            }
        }
    }

    float mean[10] = {}, sigma[10] = {}, MaxP[10] = {};
    for (int lvl = 0; lvl < maxlvl; lvl++) {
        // eval_level (L192-233)
        float avLP[4], maxL[4], sigP[4];
        for (int dir = 1; dir < 4; dir++) {
            eval_avg(bands[3 * lvl + dir - 1], n, avLP[dir], maxL[dir]);
            eval_sigma(bands[3 * lvl + dir - 1], n, avLP[dir], sigP[dir]);
        }
        float AvL = 0.f, SL = 0.f, maxLP = 0.f;
        for (int dir = 1; dir < 4; dir++) {
            AvL += avLP[dir];
            SL += sigP[dir];
            maxLP += maxL[dir];
        }
        AvL /= 3;
        SL /= 3;
        maxLP /= 3;
        mean[lvl] = AvL;
        sigma[lvl] = SL;
        MaxP[lvl] = maxLP;
    }
    if (stats_in)
        for (int lvl = 0; lvl < maxlvl; lvl++) { mean[lvl] = stats_in->mean[lvl]; sigma[lvl] = stats_in->sigma[lvl]; MaxP[lvl] = stats_in->maxp[lvl]; }
    for (int lvl = 0; lvl < maxlvl; lvl++) { st.mean[lvl] = mean[lvl]; st.sigma[lvl] = sigma[lvl]; st.maxp[lvl] = MaxP[lvl]; }

    for (int dir = 1; dir < 4; dir++) {
        for (int level = 0; level < maxlvl; ++level) {
            float *wl = bands[3 * level + dir - 1];
            if (MaxP[level] > 0.f && mean[level] != 0.f && sigma[level] != 0.f) {
                float insigma = 0.666f;
                float logmax = ref_log(MaxP[level]);
                float rapX = (mean[level] + sigma[level]) / MaxP[level];
                float inx = ref_log(insigma);
                float iny = ref_log(rapX);
                float rap = inx / iny;
                float asig = 0.166f / sigma[level];
                float bsig = 0.5f - asig * mean[level];
                float amean = 0.5f / mean[level];

                for (int i = 0; i < n; i++) {
                    float absciss;
                    float &val = wl[i];
                    if (std::isnan(val)) {
                        ++cn.nan_left;
                        continue;
                    }
                    if (fabsf(val) >= (mean[level] + sigma[level])) {
                        float valcour = oracle_xlogf_s(fabsf(val));
                        float valc = valcour - logmax;
                        float vald = valc * rap;
                        absciss = oracle_xexpf_s(vald);
                        ++cn.branch_max;
                    } else if (fabsf(val) >= mean[level]) {
                        absciss = asig * fabsf(val) + bsig;
                        ++cn.branch_mid;
                    } else {
                        absciss = amean * fabsf(val);
                        ++cn.branch_low;
                    }
                    const float index = absciss * 500.f;
                    if (curve && index > 499.f) ++cn.clipped_above;
                    float kc = (curve ? oracle_lutf(curve, 501, index) : 0.f) - 0.5f;
                    float reduceeffect = kc <= 0.f ? 1.f : 1.5f;
                    float kinterm = 1.f + reduceeffect * kc;
                    if (kinterm <= 0.f) ++cn.floor_hits;
                    kinterm = kinterm <= 0.f ? 0.01f : kinterm;
                    val *= kinterm;
                }
            } else if (dir == 1) {
                ++cn.levels_skipped;
            }
        }
    }
    if (stats_out) *stats_out = st;
    if (counts) *counts = cn;
}

} // extern "C"
