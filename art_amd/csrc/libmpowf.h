// art_amd/csrc/libmpowf.h -- powf with the bits of the host's libm, for the per-pixel powf of PQ / PQ_inv outside their tables (jzazbzdev.h).
// The reference calls std::pow on floats there (color.cc:67-84), i.e. glibc's powf, and PQ_inv has a pole at X = 3.2: beside it one ulp of
// the inner powf is tens of units of the pixel, so a powf that is merely accurate does not give the reference's pixel.  glibc 2.28 and later
// (sysdeps/ieee754/flt-32/e_powf.c, from the ARM optimized routines' powf.c) compute log2(x) from a 16-entry table and a degree-5
// polynomial and 2^(y log2 x) from a 32-entry table and a degree-3 polynomial, all in double without contraction; the tables and
// coefficients below are theirs.  The same steps in the same order give the same float.
//
// LIBMPOWF_OPAQUE, defined ahead of the include: the constants are read through an index the compiler cannot see through, so that they are
// loaded where the rare branch needs them and do not sit in scalar registers across the whole pixel loop (colorcorrection.hip, whose
// three-region kernel has none to spare).  Without it they fold into the instructions (tonecurve.hip, whose 1024-lane kernel has no vector
// registers to spare).
#pragma once
#ifndef LIBMPOWF_HOST             // tests/emul/libmpowf_host.cc compiles this text for the host, with the four bit casts as functions
#include <hip/hip_runtime.h>
#endif

namespace artgpu {

static __device__ const double pw_data[75] = {
    // [0, 32): log2's table, 1 / c and log2(c) of sixteen intervals of [0x1.66p-1, 0x1.66p0)
    0x1.661ec79f8f3bep+0, -0x1.efec65b963019p-2, 0x1.571ed4aaf883dp+0, -0x1.b0b6832d4fca4p-2,
    0x1.49539f0f010b0p+0, -0x1.7418b0a1fb77bp-2, 0x1.3c995b0b80385p+0, -0x1.39de91a6dcf7bp-2,
    0x1.30d190c8864a5p+0, -0x1.01d9bf3f2b631p-2, 0x1.25e227b0b8ea0p+0, -0x1.97c1d1b3b7af0p-3,
    0x1.1bb4a4a1a343fp+0, -0x1.2f9e393af3c9fp-3, 0x1.12358f08ae5bap+0, -0x1.960cbbf788d5cp-4,
    0x1.0953f419900a7p+0, -0x1.a6f9db6475fcep-5, 0x1.0000000000000p+0, 0x0.0p+0,
    0x1.e608cfd9a47acp-1, 0x1.338ca9f24f53dp-4, 0x1.ca4b31f026aa0p-1, 0x1.476a9543891bap-3,
    0x1.b2036576afce6p-1, 0x1.e840b4ac4e4d2p-3, 0x1.9c2d163a1aa2dp-1, 0x1.40645f0c6651cp-2,
    0x1.886e6037841edp-1, 0x1.88e9c2c1b9ff8p-2, 0x1.767dcf5534862p-1, 0x1.ce0a44eb17bccp-2,
    // [32, 64): exp2's table, 2^(i / 32) with i << 47 taken off its bit pattern
    0x1.0000000000000p+0, 0x1.fd9b0d3158574p-1, 0x1.fb5586cf9890fp-1, 0x1.f9301d0125b51p-1,
    0x1.f72b83c7d517bp-1, 0x1.f54873168b9aap-1, 0x1.f387a6e756238p-1, 0x1.f1e9df51fdee1p-1,
    0x1.f06fe0a31b715p-1, 0x1.ef1a7373aa9cbp-1, 0x1.edea64c123422p-1, 0x1.ece086061892dp-1,
    0x1.ebfdad5362a27p-1, 0x1.eb42b569d4f82p-1, 0x1.eab07dd485429p-1, 0x1.ea47eb03a5585p-1,
    0x1.ea09e667f3bcdp-1, 0x1.e9f75e8ec5f74p-1, 0x1.ea11473eb0187p-1, 0x1.ea589994cce13p-1,
    0x1.eace5422aa0dbp-1, 0x1.eb737b0cdc5e5p-1, 0x1.ec49182a3f090p-1, 0x1.ed503b23e255dp-1,
    0x1.ee89f995ad3adp-1, 0x1.eff76f2fb5e47p-1, 0x1.f199bdd85529cp-1, 0x1.f3720dcef9069p-1,
    0x1.f5818dcfba487p-1, 0x1.f7c97337b9b5fp-1, 0x1.fa4afa2a490dap-1, 0x1.fd0765b6e4540p-1,
    // [64, 69): log2's polynomial; [69, 72): exp2's; [72]: exp2's rounding shift; [73], [74]: the ends of y log2 x
    0x1.27616c9496e0bp-2, -0x1.71969a075c67ap-2, 0x1.ec70a6ca7baddp-2, -0x1.7154748bef6c8p-1, 0x1.71547652ab82bp+0,
    0x1.c6af84b912394p-5, 0x1.ebfce50fac4f3p-3, 0x1.62e42ff0c52d6p-1, 0x1.8p47, 0x1.fffffffd1d571p+6, -150.0
};

// powf(x, y) for any x and a y that is finite, positive and no integer (the four exponents of PQ / PQ_inv): glibc's steps for a positive
// finite x, subnormals scaled by 2^23 first as it does, and its results at the ends (overflow to inf above y log2 x = 0x1.fffffffd1d571p+6,
// 0 at and below -150, subnormal results through the conversion in between); NaN for a NaN or a negative finite x, 0 for +-0, inf for +-inf.
__device__ __forceinline__ float libm_powf(float x, float y)
{
#ifdef LIBMPOWF_OPAQUE
    int zero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zero));
    const double *c = pw_data + zero;
#else
    const double *c = pw_data;
#endif
    unsigned ix = __float_as_uint(x);
    if (ix - 1u < 0x007fffffu) ix = __float_as_uint(x * 0x1p23f) - (23u << 23);
    const unsigned tmp = ix - 0x3f330000u;
    const int i = (tmp >> 19) % 16;
    const unsigned top = tmp & 0xff800000u;
    const int k = (int)top >> 23;
    const double z = (double)__uint_as_float(ix - top);
    const double r = z * c[2 * i] - 1;
    const double y0 = c[2 * i + 1] + (double)k;
    const double r2 = r * r;
    double l = c[64] * r + c[65];
    const double p = c[66] * r + c[67];
    const double r4 = r2 * r2;
    double q = c[68] * r + y0;
    q = p * r2 + q;
    l = l * r4 + q;
    const double xd = (double)y * l;
    const double shift = c[72];
    double kd = xd + shift;
    const unsigned long long ki = (unsigned long long)__double_as_longlong(kd);
    kd -= shift;
    const double rr = xd - kd;
    const double s = __longlong_as_double(__double_as_longlong(c[32 + (int)(ki % 32)]) + (long long)(ki << 47));
    const double zz = c[69] * rr + c[70];
    double e = c[71] * rr + 1;
    e = zz * (rr * rr) + e;
    float res = (float)(e * s);
    if (xd > c[73]) res = __uint_as_float(0x7f800000u);
    if (xd <= c[74]) res = 0.f;
    const unsigned ax = __float_as_uint(x) & 0x7fffffffu;
    if (ax == 0u) res = 0.f;
    else if (ax == 0x7f800000u) res = __uint_as_float(0x7f800000u);
    else if (ax > 0x7f800000u || (__float_as_uint(x) >> 31)) res = __uint_as_float(0x7fc00000u);
    return res;
}

} // namespace artgpu
