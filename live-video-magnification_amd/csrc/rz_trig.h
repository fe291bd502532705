/* rz_trig.h -- ONE implementation of the three transcendental functions of the Riesz (Phase) mode, for both sides of the parity
 * tests: plain C that compiles as C (oracle/lvm_oracle.c under LVMO_VAR_PORTABLE_TRIG), as HIP device code (csrc/riesz.hip under
 * LVM_RZ_PORTABLE_TRIG in the exact flavour) and in the CPU emulation build.  Device libm and glibc disagree in the last ulp of
 * acosf / sinf / cosf; these functions cannot: they use + - * / on float64, one float32 square root, comparisons and integer
 * conversions only -- every one of them an IEEE operation with one defined result -- and no libm call.  Both sides are built with
 * -ffp-contract=off, so no product is fused into a sum.  Each function evaluates in float64 and rounds ONCE to float32: the float64
 * value is within 2^-40 (relative) of the true one, so the float32 result is the correctly rounded one or its neighbour (<= 1 ulp;
 * measured shares in DESIGN.md 5).
 *
 * Domains (every float gives a defined result):
 *   rz_acosf  [-1, 1]: <= 1 ulp.  x > 1 -> 0, x < -1 -> the float nearest pi (the value at the nearer end; the Riesz kernels never
 *             ask: arc_cos clamps before the call).  NaN -> NaN.
 *   rz_sinf / rz_cosf  |x| <= RZ_TRIG_ACCURATE (100 pi): <= 1 ulp.  The kernels only ask for [0, pi] (the angle is min(magnitude *
 *             alpha, coWavelength * pi / 100), coWavelength <= 100).  Up to RZ_TRIG_XMAX the same code keeps running (the reduction
 *             stays exact well beyond 100 pi, nothing is promised); above RZ_TRIG_XMAX the functions give sin -> 0, cos -> 1.  Finite
 *             and |y| <= 1 for every finite x.  +-inf and NaN -> NaN.
 * Constants named RZ_BP_* are the branch points of the code below (tests/test_rz_trig.py samples around each of them). */
#ifndef LVM_RZ_TRIG_H
#define LVM_RZ_TRIG_H

#ifndef RZ_TRIG_FN
#define RZ_TRIG_FN static inline
#endif

#define RZ_BP_ACOS_HALF 0.5f          /* |x| <= 0.5: pi/2 - asin(x); beyond: the half-angle form */
#define RZ_BP_ACOS_ONE 1.0f           /* |x| >= 1: the end values */
#define RZ_BP_TRIG_XMAX 1048576.0f    /* |x| > 2^20: no reduction (quadrant counts up to 2^20 keep the first reduction step exact) */
#define RZ_TRIG_ACCURATE 314.15927f   /* 100 pi: the range of the 1-ulp statement */

/* asin(s) / s - 1 = z P(z), z = s^2 <= 1/4: the Taylor series (2k)! / (4^k k!^2 (2k+1)), 20 terms (the 21st is below 1e-15 at z = 1/4) */
RZ_TRIG_FN double rz_asin_poly(double z) {
    double p = 0x1.90cb77f60c7cep-9;
    p = p * z + 0x1.b026f57b13b14p-9;
    p = p * z + 0x1.d3d2a8e0dd67dp-9;
    p = p * z + 0x1.fcaf8fb6db6dbp-9;
    p = p * z + 0x1.15ee9d45d1746p-8;
    p = p * z + 0x1.31683bdef7bdfp-8;
    p = p * z + 0x1.51ba308d3dcb1p-8;
    p = p * z + 0x1.782dda12f684cp-8;
    p = p * z + 0x1.a6863d70a3d71p-8;
    p = p * z + 0x1.df3bd37a6f4dfp-8;
    p = p * z + 0x1.12ef3cf3cf3cfp-7;
    p = p * z + 0x1.3fde50d79435ep-7;
    p = p * z + 0x1.7a87878787878p-7;
    p = p * z + 0x1.c99999999999ap-7;
    p = p * z + 0x1.1c4ec4ec4ec4fp-6;
    p = p * z + 0x1.6e8ba2e8ba2e9p-6;
    p = p * z + 0x1.f1c71c71c71c7p-6;
    p = p * z + 0x1.6db6db6db6db7p-5;
    p = p * z + 0x1.3333333333333p-4;
    p = p * z + 0x1.5555555555555p-3;
    return p * z;
}

RZ_TRIG_FN float rz_acosf(float x) {
    const double PI = 0x1.921fb54442d18p+1, PIO2 = 0x1.921fb54442d18p+0;
    if (x != x) return x + x;
    if (x >= RZ_BP_ACOS_ONE) return 0.0f;
    if (x <= -RZ_BP_ACOS_ONE) return (float)PI;
    const double xd = (double)x;
    if (x <= RZ_BP_ACOS_HALF && x >= -RZ_BP_ACOS_HALF) {
        const double as = xd + xd * rz_asin_poly(xd * xd);
        return (float)(PIO2 - as);
    }
    /* acos(x) = 2 asin(sqrt((1 - x) / 2)) for x > 1/2, pi - 2 asin(sqrt((1 + x) / 2)) for x < -1/2.  z is exact, in float too (1 - |x| has
     * at most 24 bits).  Its root: the float32 square root (correctly rounded, 2^-24) and one Newton step in float64 (2^-49) -- no
     * float64 square root is asked of either side. */
    const double z = (x > 0.0f ? 1.0 - xd : 1.0 + xd) * 0.5;
    const double s0 = (double)__builtin_sqrtf((float)z);
    const double s = s0 + 0.5 * (z - s0 * s0) / s0;
    const double as2 = 2.0 * (s + s * rz_asin_poly(z));
    return (float)(x > 0.0f ? as2 : PI - as2);
}

/* x = k pi/2 + r, |r| <= pi/4 (a little more at a rounded boundary); returns r, *quadrant = k mod 4.  pi/2 = P1 + P1T: P1 holds its
 * first 33 bits, so k * P1 (k < 2^20) and x - k * P1 are exact; k * P1T is rounded at 2^-53 of a term below 2^-13. */
RZ_TRIG_FN double rz_trig_reduce(double xd, int* quadrant) {
    const double INV_PIO2 = 0x1.45f306dc9c883p-1, P1 = 0x1.921fb544p+0, P1T = 0x1.0b4611a626331p-34;
    const double t = xd * INV_PIO2;
    const int k = (int)(t >= 0.0 ? t + 0.5 : t - 0.5);
    const double kd = (double)k;
    *quadrant = k & 3;
    return (xd - kd * P1) - kd * P1T;
}
/* sin(r) = r (1 + z S(z)), cos(r) = 1 + z C(z), z = r^2: Taylor series to r^17 and r^16 (the next terms are below 1e-17 at pi/4) */
RZ_TRIG_FN double rz_sin_kernel(double r) {
    const double z = r * r;
    double p = 0x1.952c77030ad4ap-49;
    p = p * z + -0x1.ae7f3e733b81fp-41;
    p = p * z + 0x1.6124613a86d09p-33;
    p = p * z + -0x1.ae64567f544e4p-26;
    p = p * z + 0x1.71de3a556c734p-19;
    p = p * z + -0x1.a01a01a01a01ap-13;
    p = p * z + 0x1.1111111111111p-7;
    p = p * z + -0x1.5555555555555p-3;
    return r * (1.0 + z * p);                   /* (this form keeps the sign of a zero argument) */
}
RZ_TRIG_FN double rz_cos_kernel(double r) {
    const double z = r * r;
    double p = 0x1.ae7f3e733b81fp-45;
    p = p * z + -0x1.93974a8c07c9dp-37;
    p = p * z + 0x1.1eed8eff8d898p-29;
    p = p * z + -0x1.27e4fb7789f5cp-22;
    p = p * z + 0x1.a01a01a01a01ap-16;
    p = p * z + -0x1.6c16c16c16c17p-10;
    p = p * z + 0x1.5555555555555p-5;
    p = p * z + -0x1.0p-1;
    return 1.0 + z * p;
}

RZ_TRIG_FN float rz_sinf(float x) {
    const float ax = x < 0.0f ? -x : x;
    if (!(ax <= RZ_BP_TRIG_XMAX)) return (x != x || ax > 3.4028234663852886e38f) ? x - x : 0.0f;
    int q;
    const double r = rz_trig_reduce((double)x, &q);
    const double v = (q & 1) ? rz_cos_kernel(r) : rz_sin_kernel(r);
    return (float)((q & 2) ? -v : v);
}

RZ_TRIG_FN float rz_cosf(float x) {
    const float ax = x < 0.0f ? -x : x;
    if (!(ax <= RZ_BP_TRIG_XMAX)) return (x != x || ax > 3.4028234663852886e38f) ? x - x : 1.0f;
    int q;
    const double r = rz_trig_reduce((double)x, &q);
    const double v = (q & 1) ? rz_sin_kernel(r) : rz_cos_kernel(r);
    return (float)(((q + 1) & 2) ? -v : v);
}

#endif
