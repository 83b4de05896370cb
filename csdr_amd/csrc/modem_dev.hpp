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

// pack_bits_8to1_u8_u8: eight bytes, the first one the MSB, each taken as !!byte
__host__ __device__ inline uint8_t pack_bits_8to1_step(const uint8_t *x)
{
    unsigned v = 0;
    for (int i = 0; i < 8; i++) v = (v << 1) | (x[i] != 0);
    return (uint8_t)v;
}

} // namespace csdr_amd
