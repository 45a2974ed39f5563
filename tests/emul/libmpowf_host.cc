// tests/emul/libmpowf_host.cc -- art_amd/csrc/libmpowf.h compiled for the host, so that its text can be held to the host's powf
// (tests/test_libmpowf.py).  Built with -ffp-contract=off, as the device code is.
#include <cmath>
#include <cstdint>
#include <cstring>

#define LIBMPOWF_HOST
#define __device__
#define __forceinline__ inline
static inline unsigned __float_as_uint(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }
static inline float __uint_as_float(unsigned u) { float f; std::memcpy(&f, &u, 4); return f; }
static inline long long __double_as_longlong(double d) { long long u; std::memcpy(&u, &d, 8); return u; }
static inline double __longlong_as_double(long long u) { double d; std::memcpy(&d, &u, 8); return d; }
#include "../../art_amd/csrc/libmpowf.h"

extern "C" {

void pw_ref_powf(const float *x, float y, float *mine, float *host, long long n)
{
    for (long long k = 0; k < n; ++k) {
        mine[k] = artgpu::libm_powf(x[k], y);
        host[k] = std::pow(x[k], y);
    }
}

}
