// modem_dev.hpp -- step functions of the pulse-shaped symbol modem, shared by the kernels of modem.hip and its CPU debug entry.
//
//   psk_modulator_u8_c | plain_interpolate_cc I | apply_real_fir_cc (T taps)     libcsdr.c:1772-1782, 2499-2506, 2276-2291
//   generic_slicer_f_u8                                                           libcsdr.c:1731-1765
//   pack_bits_1to8_u8_u8 / pack_bits_8to1_u8_u8                                    libcsdr.c:1810-1827
//
// The transmit stream of a channel: c[m], m >= 0, its symbols since the last reset; x[j] = c[j / I] where I divides j, else 0; y[i] = sum over t < T of
// x[i + t] * taps[t].  Output i has products only at t = ph, ph + I, ... < T with ph = (-i) mod I, on the symbols ceil(i / I), ceil(i / I) + 1, ...; they are
// accumulated in ascending t with fmaf, the skipped 0 * tap terms left out (§4p).  After n symbols the stream holds the outputs 0 .. n I - T.
//
// A call works in coordinates relative to its own start.  With n0 symbols and N0 = max(0, n0 I - T + 1) outputs in front of it: r0 = N0 mod I, hb = n0 - N0 / I
// (how many symbols in front of the call its first output reaches back, at most H = ceil((T - 1) / I), the held history).  Output o of the call is stream output
// N0 + o; its first symbol is e = ceil((r0 + o) / I) - hb relative to the call's first new symbol: e < 0 is hist[H + e], 0 <= e < n is the call's input.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "psk31_dev.hpp"

namespace csdr_amd {

enum { PULSETX_MOD = 0, PULSETX_SHAPE = 1 };

struct PulseTxCfg {
    int first, last;
    int I, T;                      // interpolation and taps
    int K;                         // ceil(T / I): the most products of one output
    int H;                         // ceil((T - 1) / I): symbols held per channel between calls
};

// One call's geometry (the same for every channel: all channels have taken the same number of symbols)
struct PulseTxCall {
    int r0, hb;                    // see above
    int n;                         // new symbols
    int n_out;                     // outputs of this call
};

// Where one channel's symbols are: the held history, and the call's input as bytes (through the 256 symbols) or as complexf
struct PulseTxSrc {
    const float2 *hist;            // H symbols: the last H in front of the call, oldest first (zeros where the stream has not begun)
    const uint8_t *in_b;           // first_stage MOD
    const float2 *in_c;            // first_stage SHAPE
    const float2 *sym;             // 256 symbols (csdr_amd_psk31tx_tables)
};

// symbol e relative to the call's first new one (-H <= e); 0 + 0i at and beyond the call's end
__host__ __device__ inline float2 pulsetx_symbol(const PulseTxCfg &c, const PulseTxCall &k, const PulseTxSrc &s, int e)
{
    if (e < 0) return s.hist[c.H + e];
    if (e >= k.n) return make_float2(0.f, 0.f);
    return s.in_b ? s.sym[s.in_b[e]] : s.in_c[e];
}

// output o < n_out of the call
__host__ __device__ inline float2 pulsetx_output(const PulseTxCfg &c, const PulseTxCall &k, const PulseTxSrc &s, const float *taps, int o)
{
    const long long u = (long long)k.r0 + o;
    const int j = (int)(u % c.I);
    const int e0 = (int)(u / c.I) + (j > 0) - k.hb;
    float ai = 0.f, aq = 0.f;
    int e = e0;
    for (int t = j ? c.I - j : 0; t < c.T; t += c.I, e++) {
        const float2 x = pulsetx_symbol(c, k, s, e);
        const float w = taps[t];
        ai = fmaf(x.x, w, ai); aq = fmaf(x.y, w, aq);
    }
    return make_float2(ai, aq);
}

// entry h < H of the history behind the call: the symbol n - H + h relative to the call's first new one
__host__ __device__ inline float2 pulsetx_next_hist(const PulseTxCfg &c, const PulseTxCall &k, const PulseTxSrc &s, int h)
{
    return pulsetx_symbol(c, k, s, k.n - c.H + h);
}

// generic_slicer_f_u8: the thresholds in float as the reference computes them (separate multiply and add).  d = (float)(2.0 / (n_symbols - 1)).
// An input that no symbol claims (NaN; a value in a rounding gap between one symbol's upper and the next one's lower limit) gives 0.
__host__ __device__ inline uint8_t generic_slicer_step(float x, int n_symbols, float d)
{
    const float half = d / 2;
    for (int j = 0; j < n_symbols; j++) {
        const float jd = (float)j * d;
        const float center = -1 + jd;
        const float lo = center - half, hi = center + half;
        if (j == 0) { if (x < hi) return 0; }
        else if (j == n_symbols - 1) { if (x >= lo) return (uint8_t)j; }
        else if (x >= lo && x < hi) return (uint8_t)j;
    }
    return 0;
}

// ---- the receive stream: pulse_shaping_filter_cc (matched filter) | timing_recovery_cc | [realpart_cf |] gain_ff | generic_slicer_f_u8      (§4q)
//
// x: a channel's complexf input since its last reset.  FILTER: f[i] = sum over t < T of x[i + t] taps[t], i = 0 .. n - T (apply_real_fir_cc, no zeros in
// front); from the stage TIMING on, f = x, bits kept.  TIMING: timing_recovery_cc applied once to the whole of f (psk31_dev.hpp's positions, error and
// correction).  SLICE: gain * re (slice_q: gain * re, then gain * im) through generic_slicer_step.  f is never stored: it is evaluated at the three positions
// of each symbol only, and the symbol whose right point is the next one's left point (GARDNER, no correction) hands that value on.
//
// The order of the T products is part of the definition, since the timing loop truncates a float to an int: 16 partial sums, sum r over the t = r (mod 16)
// in ascending t with fmaf from 0, then p[r] += p[r + s] for r < s, s = 8, 4, 2, 1, the lower index as the left operand.  A group of G = 1, 2, 4, 8 or 16
// lanes shares it: lane g holds the sums r = g (mod G), folds them for s >= G by itself and for s < G with lane g ^ s.
enum { PULSERX_FILTER = 0, PULSERX_TIMING = 1, PULSERX_SLICE = 2 };

struct PulseRxCfg {
    Psk31Cfg t;                    // the timing loop's part (algorithm, D, hb, qb, wing, use_q, loop_gain, max_error, hb_sign, reset_lo, reset_hi)
    int first, last;
    int T, Tm1;                    // taps (1 from TIMING on) and how far a filtered sample reaches beyond its index: T - 1, or 0 from TIMING on
    float gain, d;                 // gain_ff's factor and the slicer's (float)(2.0 / (n_symbols - 1))
    int n_symbols, slice_q;
};

// One channel's state between calls; its raw unconsumed tail (tail_len <= 3 D/2 + Tm1 samples from the current symbol start on) lies beside it
struct PulseRxChan {
    int tail_len;
    int corr;                      // last_correction_offset
    uint32_t base;                 // absolute index of the tail's first sample
};

struct PulseRxOut {
    float2 *c;                     // last == TIMING: the sampled symbols
    uint8_t *b;                    // last == SLICE: one byte per symbol, or two (I, Q)
    float *err;                    // optional, last == TIMING: the unclamped timing error per symbol
    unsigned *idx;                 // optional, last == TIMING: absolute sample index per symbol
};

// the fold of the 16 partial sums
__host__ __device__ inline float pulserx_fold(float *p)
{
#pragma unroll
    for (int s = 8; s >= 1; s >>= 1)
#pragma unroll
        for (int r = 0; r < s; r++) p[r] = p[r] + p[r + s];
    return p[0];
}

// f[i] in the defined order; x(t) is the raw sample i + t
template <class X> __host__ __device__ inline float2 pulserx_dot(X x, const float *taps, int T)
{
    float pi[16], pq[16];
#pragma unroll
    for (int r = 0; r < 16; r++) pi[r] = pq[r] = 0.f;
    int t0 = 0;
    for (; t0 + 16 <= T; t0 += 16) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float2 v = x(t0 + r);
            const float w = taps[t0 + r];
            pi[r] = fmaf(v.x, w, pi[r]); pq[r] = fmaf(v.y, w, pq[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; r++) {
        if (t0 + r < T) {
            const float2 v = x(t0 + r);
            const float w = taps[t0 + r];
            pi[r] = fmaf(v.x, w, pi[r]); pq[r] = fmaf(v.y, w, pq[r]);
        }
    }
    return make_float2(pulserx_fold(pi), pulserx_fold(pq));
}

// one symbol out at stage `last`; k counts this call's outputs (bytes from SLICE)
__host__ __device__ inline void pulserx_emit(const PulseRxCfg &c, const PulseRxOut &o, int &k, float2 xo, float error, uint32_t index)
{
    if (c.last == PULSERX_TIMING) {
        o.c[k] = xo;
        if (o.err) o.err[k] = error;
        if (o.idx) o.idx[k] = index;
        k++;
        return;
    }
    o.b[k++] = generic_slicer_step(c.gain * xo.x, c.n_symbols, c.d);
    if (c.slice_q) o.b[k++] = generic_slicer_step(c.gain * xo.y, c.n_symbols, c.d);
}

// One call for one channel: n new samples behind the tail (capacity 3 D/2 + T).  Returns the number of outputs written.
__host__ __device__ inline int pulserx_walk(const PulseRxCfg &c, PulseRxChan &s, float2 *tail, const float2 *in, long long n, const float *taps, const PulseRxOut &o)
{
    const long long T0 = s.tail_len, nV = T0 + n;
    auto raw = [&](long long p) -> float2 { return p < T0 ? tail[p] : in[p - T0]; };
    auto f = [&](long long p) -> float2 {
        if (c.first != PULSERX_FILTER) return raw(p);
        return pulserx_dot([&](int t) { return raw(p + t); }, taps, c.T);
    };
    long long cbi = 0, held_at = -1;
    float2 held = make_float2(0.f, 0.f);
    int corr = s.corr, k = 0;
    while (cbi + c.t.hb * 3 + c.Tm1 < nV) {                                       // libcsdr.c:1998 on the filtered stream's length nV - Tm1
        long long pl, pm, pr;
        psk31_positions(c.t, cbi, &corr, &pl, &pm, &pr);
        const float2 xl = pl == held_at ? held : f(pl), xm = f(pm), xr = f(pr);
        held = xr; held_at = pr;
        const float error = psk31_timing_error(c.t, xl, xm, xr);
        pulserx_emit(c, o, k, c.t.algorithm == 1 ? xm : xl, error, s.base + (uint32_t)(c.t.algorithm == 1 ? pm : pl));
        corr = psk31_correction(c.t, error);
        cbi += c.t.D + corr;
    }
    const int nt = (int)(nV - cbi);
    if (cbi > 0) for (int j = 0; j < nt; j++) tail[j] = raw(cbi + j);             // forward: source index >= destination index
    else for (long long j = T0; j < nV; j++) tail[j] = in[j - T0];
    s.tail_len = nt;
    s.corr = corr;
    s.base += (uint32_t)cbi;
    return k;
}

// pack_bits_8to1_u8_u8: eight bytes, the first one the MSB, each taken as !!byte
__host__ __device__ inline uint8_t pack_bits_8to1_step(const uint8_t *x)
{
    unsigned v = 0;
    for (int i = 0; i < 8; i++) v = (v << 1) | (x[i] != 0);
    return (uint8_t)v;
}

} // namespace csdr_amd
