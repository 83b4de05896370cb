// cfir_dev.hpp -- the step functions of the complex-tap FIR (apply_fir_cc libcsdr.c:2261-2273), shared by the kernels (cfir.hip) and their CPU debug entry.
//
//   y[o] = sum_{t < T} x[o + t] h[t]                 complex x complex, n - T + 1 outputs of n samples, no zero history
//
// Over the interleaved floats xf of x each part of an output is ONE fmaf chain over tap floats j = 0 .. 2T-1 in order, starting from 0:
//   y.re[o] = sum_j a_0[j] xf[2 o + j]               a_0[2t] = h[t].re, a_0[2t + 1] = -h[t].im
//   y.im[o] = sum_j a_1[j] xf[2 o + j]               a_1[2t] = h[t].im, a_1[2t + 1] =  h[t].re
// exactly what a k-ordered v_mfma_f32_16x16x4_f32 chain gives for the Toeplitz band of a_c (the band's zeros add nothing to finite inputs), so the
// matrix-core kernel, the generic kernel and this CPU code give the same bits whatever the call cuts or batch position.  The reference's own order
// (per tap re*re - im*im, then +=, under -ffast-math) differs: it matches within a float64 gate (tests/cfir_model.py), not bit for bit.
// Inf / NaN inputs: the matrix-core path multiplies them by the band's zeros (NaN), the other paths do not; equal bits are promised for finite inputs.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace csdr_amd {

// One channel's state between calls
struct CfirChan {
    int hist_len;                                  // complex samples of history (< T) in front of the next call's input
};

// tap float j (0 .. 2T-1) of part c (0: re, 1: im)
__host__ __device__ inline float cfir_tap(const float2 *h, int c, int j)
{
    const float2 v = h[j >> 1];
    if (c) return (j & 1) ? v.x : v.y;
    return (j & 1) ? -v.y : v.x;
}

// one output from the T samples at x (an accessor: x(t) is sample t of the window)
template <typename X>
__host__ __device__ inline float2 cfir_output(const float2 *h, int T, X x)
{
    float re = 0.f, im = 0.f;
    for (int t = 0; t < T; t++) {
        const float2 v = x(t);
        re = fmaf(cfir_tap(h, 0, 2 * t), v.x, re); re = fmaf(cfir_tap(h, 0, 2 * t + 1), v.y, re);
        im = fmaf(cfir_tap(h, 1, 2 * t), v.x, im); im = fmaf(cfir_tap(h, 1, 2 * t + 1), v.y, im);
    }
    return make_float2(re, im);
}

} // namespace csdr_amd
