// carrier_dev.hpp -- step functions of carrier recovery, shared by both kernels of carrier.hip, the CPU hook and the drop-in.
//
//   bpsk_costas_loop_cc   libcsdr.c:2108-2142   nco = e^(j phase); out = in * nco; error = PI out.i out.q, or the decision-directed atan2 form;
//                                               freq += error beta; dphase = clamp(error alpha + freq); phase = wrap(phase + dphase) into (0, 2 PI]
//   pll_cc                libcsdr.c:1874-1915   phase = wrap(phase + dphase) into [-PI, PI]; nco = (sin, cos); error = wrap(atan2(in.i, in.q) - phase);
//                                               P: dphase = error alpha;  PI: dphase = wrap(error alpha + freq), freq += error beta;  output -dphase
//
// Every float operation is the reference's, in its order (the sources build with -ffp-contract=off).  cos, sin and atan2 are taken in double from the float
// argument and rounded to float, as the reference's e_powj and atan2 calls on float operands do: cos and sin by carrier_sincos below (the same bits on host
// and device), atan2 by the library.  The device's double atan2 (ocml) and the host's (glibc) are both within an ulp of the exact value but need not round
// alike, so a decision-directed or PLL value may differ in its last float bit at a rounding boundary between a kernel and the CPU hook: equal in practice,
// not by proof.  Between the two kernels, and between any two ways of cutting or batching, the bits are equal by construction.
//
// The reference's `while (x > lim) x -= 2 PI` wraps are kept as loops (a closed form rounds differently) but end after CARRIER_WRAP_MAX turns: a phase that far
// out has the reference itself on its way to a hang (x - 2 PI == x from 2^26 on), and a kernel has to end.  create and set_channel keep parameters and state
// where a Costas loop never comes near the limit; a PLL's integrator can get there only on an input it has lost for good.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace csdr_amd {

enum { CARRIER_COSTAS = 0, CARRIER_COSTAS_DD = 1, CARRIER_PLL_P = 2, CARRIER_PLL_PI = 3 };
constexpr int CARRIER_WRAP_MAX = 1024;

struct CarrierCfg { int mode; float alpha, beta, dphase_max; int reset_to_zero; };
struct CarrierChan { float phase, dphase, freq; };                       // nco_phase / output_phase, dphase, current_freq / iir_temp
struct CarrierSample { float2 out; float error, dphase; float2 nco; };  // what one input sample gives (PLL modes: nco and dphase only)

#define CARRIER_PI ((float)3.14159265358979323846)                      // libcsdr.h:65: a float

// (float)sin((double)w) and (float)cos((double)w) in one evaluation.  The library's double sin and cos are the longest part of the serial chain (general
// argument reduction, twice); a loop's phase lies within a turn, so here: k = rint(w 2 / PI), r = w - k PI/2 with PI/2 in two doubles (two fma, exact to an
// ulp of r), the classic degree-13 / degree-14 minimax kernels on |r| <= PI/4 (below an ulp of the double result, both polynomials side by side), and the
// quadrant swap.  The float rounding of a double within an ulp of the exact value equals the correctly rounded float except within ~2^-29 of a rounding
// boundary, so this returns the bits of the C library's double functions rounded to float in practice (the tests compare them on every input), and the same
// bits on the host and on the device by construction (fma is exact on both).
__host__ __device__ inline void carrier_sincos(float w, float *sn, float *cs)
{
    const double x = (double)w;
    const double kd = rint(x * 6.36619772367581382433e-01);                 // 2 / PI
    double r = fma(-kd, 1.57079632679489655800e+00, x);                     // PI / 2, head
    r = fma(-kd, 6.12323399573676603587e-17, r);                            // PI / 2, tail
    const double z = r * r;
    double ps = fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
    double pc = fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
    ps = fma(z, ps, 2.75573137070700676789e-06); pc = fma(z, pc, -2.75573143513906633035e-07);
    ps = fma(z, ps, -1.98412698298579493134e-04); pc = fma(z, pc, 2.48015872894767294178e-05);
    ps = fma(z, ps, 8.33333333332248946124e-03); pc = fma(z, pc, -1.38888888888741095749e-03);
    pc = fma(z, pc, 4.16666666666666019037e-02);
    const double s = fma(z * r, fma(z, ps, -1.66666666666666324348e-01), r);      // r + r^3 (S1 + z ps)
    const double c = 1.0 - fma(0.5, z, -(z * (z * pc)));                           // 1 - (z / 2 - z^2 pc)
    const int q = (int)kd & 3;
    const double sv = (q & 1) ? c : s, cv = (q & 1) ? s : c;
    *sn = (float)((q & 2) ? -sv : sv);
    *cs = (float)(((q + 1) & 2) ? -cv : cv);
}
__host__ __device__ inline float carrier_atan2(float y, float x) { return (float)atan2((double)y, (double)x); }

// while (x > hi) x -= 2 PI;  while (x < lo) x += 2 PI   (libcsdr.c:1879-1880)
__host__ __device__ inline float carrier_wrap_pm_pi(float x)
{
    for (int k = 0; k < CARRIER_WRAP_MAX && x > CARRIER_PI; k++) x -= 2 * CARRIER_PI;
    for (int k = 0; k < CARRIER_WRAP_MAX && x < -CARRIER_PI; k++) x += 2 * CARRIER_PI;
    return x;
}

// libcsdr.c:2110-2141, one sample
__host__ __device__ inline void costas_step(const CarrierCfg &c, CarrierChan &s, float xi, float xq, CarrierSample &o)
{
    float ni, nq;
    carrier_sincos(s.phase, &nq, &ni);                                  // e_powj: (cos, sin)
    const float oi = xi * ni - xq * nq, oq = xi * nq + ni * xq;          // cmult(out, in, nco)
    float error;
    if (c.mode == CARRIER_COSTAS_DD) {
        const float ph = carrier_atan2(oq, oi);
        if (fabsf(ph) < CARRIER_PI / 2) error = -ph;
        else {
            error = CARRIER_PI - ph;
            for (int k = 0; k < CARRIER_WRAP_MAX && error > CARRIER_PI; k++) error -= 2 * CARRIER_PI;
        }
    } else error = CARRIER_PI * oi * oq;
    s.freq += error * c.beta;
    float d = error * c.alpha + s.freq;
    if (d > c.dphase_max) d = c.reset_to_zero ? 0.f : c.dphase_max;
    if (d < -c.dphase_max) d = c.reset_to_zero ? 0.f : -c.dphase_max;
    s.dphase = d;
    float p = s.phase + d;
    for (int k = 0; k < CARRIER_WRAP_MAX && p > 2 * CARRIER_PI; k++) p -= 2 * CARRIER_PI;
    for (int k = 0; k < CARRIER_WRAP_MAX && p <= 0; k++) p += 2 * CARRIER_PI;
    s.phase = p;
    o.out = make_float2(oi, oq); o.error = error; o.dphase = d; o.nco = make_float2(ni, nq);
}

// libcsdr.c:1878-1912, one sample.  The phase detector is atan2(i, q) and the NCO (sin, cos): the reference's operand order.
__host__ __device__ inline void pll_step(const CarrierCfg &c, CarrierChan &s, float xi, float xq, CarrierSample &o)
{
    s.phase = carrier_wrap_pm_pi(s.phase + s.dphase);
    float sn, cs;
    carrier_sincos(s.phase, &sn, &cs);
    o.nco = make_float2(sn, cs);
    const float nd = carrier_wrap_pm_pi(carrier_atan2(xi, xq) - s.phase);
    if (c.mode == CARRIER_PLL_PI) {
        const float d = nd * c.alpha + s.freq;
        s.freq += nd * c.beta;
        s.dphase = carrier_wrap_pm_pi(d);
    } else s.dphase = nd * c.alpha;
    o.dphase = -s.dphase;
    o.out = make_float2(0.f, 0.f); o.error = 0.f;
}

__host__ __device__ inline void carrier_step(const CarrierCfg &c, CarrierChan &s, float xi, float xq, CarrierSample &o)
{
    if (c.mode <= CARRIER_COSTAS_DD) costas_step(c, s, xi, xq, o); else pll_step(c, s, xi, xq, o);
}

// ---- coefficients, in the reference's precision
// init_bpsk_costas_loop_cc libcsdr.c:2098-2104: all in float, PI the float constant.  The denominator 1 + 2 damping bw + bw bw is summed as the reference's
// -ffast-math build sums it, (bw bw + 1) + 2 (damping bw): the other factors of 2 and 4 are exact in any order
inline void costas_coefficients(float bandwidth, float damping, float *alpha, float *beta, float *dphase_max)
{
    const float bw = 2 * CARRIER_PI * bandwidth;
    const float den = (bw * bw + 1) + 2 * (damping * bw);
    *alpha = (4 * damping * bw) / den;
    *beta = (4 * bw * bw) / den;
    *dphase_max = bw;
}
// pll_cc_init_pi_controller libcsdr.c:1860-1863: 2 * M_PI * bandwidth in double, stored to float; sampling_rate = 1
inline void pll_pi_coefficients(float bandwidth, float ko, float kd, float damping, float *alpha, float *beta)
{
    const float bw = (float)(2 * M_PI * (double)bandwidth);
    const float sampling_rate = 1;
    *alpha = (damping * 2 * bw) / (ko * kd);
    *beta = (bw * bw) / (sampling_rate * ko * kd);
}

} // namespace csdr_amd
