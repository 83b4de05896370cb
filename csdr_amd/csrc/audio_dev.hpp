// audio_dev.hpp -- what the audio-rate blocks of audio.hip share with the WFM receive bank (wfmrx.hip): the per-sample expressions of fmdemod_quadri_cf,
// fractional_decimator_ff's Lagrange coefficient, deemphasis_wfm_ff's step and convert_f_s16 as device functions, and the fractional decimator's host object
// with its plan.  One definition each, so that a kernel which fuses the stages computes the bits of the stages run one after the other.
// Files that include this are built with -ffp-contract=off: products and sums round separately like the reference's SSE code.
#pragma once
#include "common.hpp"
#include <vector>

namespace csdr_amd {

// fractional_decimator_ff's plan for rates that are exact in float (audio.hip): one record per CLI window
struct FdWin { int base; float w0; int first_out; int count; };

#ifdef __HIPCC__
// fmdemod_quadri_cf (libcsdr.c:1040-1071) of sample (xi, xq) behind (pi, pq)
__device__ __forceinline__ float fmdemod_quadri(float xi, float xq, float pi, float pq)
{
    const float Kf = 0.340447550238101026565118445432744920253753662109375f;   // libcsdr.c:1021
    const float dq = xq - pq, di = xi - pi;
    const float num = xi * dq - xq * di;
    const float den = xi * xi + xq * xq;
    // the reference scales and divides in double (:1067) and rounds once; a float product with a Newton-refined reciprocal is within a few ulp of
    // that (tests/audio_model.py derives the gate) and avoids the ~25-instruction fp64 division sequence that made this kernel arithmetic bound.
    // v_rcp_f32 takes a subnormal den as 0 (-> inf, and the refinement then gives NaN) and flushes 1 / den to 0 above den = 2^126, and Kf * num
    // loses bits once it is subnormal: outside a window that leaves all three (and the refinement's residual) far inside the normal range the
    // reference's own expression runs instead.  Signals at |x| ~ 1 never leave the window; the compare is the only cost there.
    const float an = fabsf(num);
    if (den >= 0x1p-60f && den <= 0x1p60f && (an >= 0x1p-100f || an == 0.f)) {
        float rd = __builtin_amdgcn_rcpf(den);
        rd = fmaf(fmaf(-den, rd, 1.0f), rd, rd);
        return (Kf * num) * rd;
    }
    return (den != 0.f) ? (float)(0.340447550238101026565118445432744920253753662109375 * (double)num / (double)den) : 0.f;
}

// coefficient w of the P-point Lagrange interpolation at fractional position fx (libcsdr.c:774-786): P - 1 factors in the reference's order, then the division
__device__ __forceinline__ float fracdec_coeff(float fx, int w, int P, int xifirst, float denom_w)
{
    const int a = xifirst + w;
    float prod = 1;
    for (int b = xifirst; b < xifirst + P; b++) if (a != b) prod *= (fx - b);
    return prod / denom_w;
}

// deemphasis_wfm_ff's recurrence (libcsdr.c:1094-1095), operation for operation
__device__ __forceinline__ float deemph_wfm_step(float alpha, float one_minus, float x, float y) { return alpha * x + one_minus * y; }

// convert_f_s16 (libcsdr.c:2397, x86 truncation semantics) -> the low 16 bits
__device__ __forceinline__ int f_to_s16(float x)
{
    const float scaled = __fmul_rn(x, 32767.0f);
    return ((scaled >= -2147483648.0f && scaled < 2147483648.0f) ? (int)scaled : (int)0x80000000) & 0xffff;
}
#endif

// the plan of a call of csdr_amd_fractional_decimator_ff over input_size samples from d's state: the outputs' first input samples and fractional positions on
// the device (d->d_lo, d->d_frac, d->d_denom, d->d_taps), d->plan_outputs of them.  The state moves on with fracdec_commit.  0 or a negative error.
int fracdec_plan(struct ::csdr_amd_ctx *c, struct ::csdr_amd_fracdec *d, int input_size);

} // namespace csdr_amd

struct csdr_amd_fracdec {
    float where, rate; int input_processed, num_poly_points, xifirst, xilast, taps_length;
    std::vector<float> denom, taps;
    // cached plan
    float plan_where; int plan_n; bool plan_valid; int plan_outputs, plan_processed; float plan_where_after;
    int cli_bufsize, plan_bufsize;   // > 0: replay the CLI's loop over the_bufsize-sample windows (csdr.c:1511-1524) instead of one call over the whole array
    std::vector<int> lo; std::vector<float> frac;      // per output: first input sample of its window, fractional position (the coefficients are the kernel's)
    csdr_amd::DevBuf<int> d_lo; csdr_amd::DevBuf<float> d_frac, d_denom, d_taps; size_t d_cap;
    csdr_amd::DevBuf<csdr_amd::FdWin> d_win; size_t win_cap;                      // exact rates: the windows of the plan (the outputs' positions are evaluated on the device)
};

namespace csdr_amd {
// what the reference's function leaves in its state behind the planned call (libcsdr.c:790-791)
inline void fracdec_commit(csdr_amd_fracdec *d) { d->input_processed = d->plan_processed; d->where = d->plan_where_after; }
} // namespace csdr_amd
