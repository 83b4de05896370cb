// rtty_dev.hpp -- per-output and per-channel step functions of the RTTY receive chain, shared by the kernels (rtty.hip) and their CPU debug entry.
//
//   bfsk_demod_cf              libcsdr.c:2335-2350   y = |sum_t x[i+t] m[t]|^2 - |sum_t x[i+t] s[t]|^2
//   serial_line_decoder_f_u8   libcsdr.c:1662-1728   start / data / stop bits of one window, with the reference's int / float / double index arithmetic
//   rtty_baudot_decoder_lookup libcsdr.c:1606-1613   Baudot code -> ASCII, letters / figures shift carried in *fig_mode
//   rtty_baudot_decoder_push   libcsdr.c:1615-1655   the bit-per-sample UART state machine behind binary_slicer_f_u8
//
// The discriminator sums each of its four real outputs (mark re / im, space re / im) as ONE fmaf chain over the interleaved taps, tap float j = 0 .. 2L-1 in
// order: exactly what a k-ordered v_mfma_f32_16x16x4_f32 chain gives for the Toeplitz band (the band's zeros add nothing), so the matrix-core kernel, the
// generic kernel and this CPU code give the same bits whatever the call cuts or batch position.  The reference's own order (per tap re*re - im*im, then +=)
// differs: the discriminator matches it within a float64 gate (tests/rtty_model.py), not bit for bit.
// The serial decoder's bit sums are sequential float32 adds in source order.  Separate mul / add: the sources build with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace csdr_amd {

enum { RTTY_BFSK = 0, RTTY_SERIAL = 1, RTTY_BAUDOT = 2 };

struct RttyCfg {
    int L;                                         // filter_length (bfsk_demod_cf)
    float spb, stopbits, ratio;                    // samples_per_bits, stopbits, bit_sampling_width_ratio
    int databits, B;                               // databits (1 .. 8 on the object), the CLI's window B
    float all_bits;                                // 1 + databits + stopbits, in float as libcsdr.c:1683
    int first, last;                               // stage range, RTTY_BFSK .. RTTY_BAUDOT
};

// One channel's state between calls
struct RttyChan {
    int hist_len;                                  // first == BFSK: complex samples of history (< L) in front of the next call's input
    int rem_len;                                   // last >= SERIAL: discriminator / line samples not yet consumed (< B), in front of the next call's
    int fig_mode;                                  // last == BAUDOT: the letters / figures shift
    int pad;
};

// The four interleaved tap sequences hf_c (2 L floats each): hf_c[2t], hf_c[2t + 1] multiply x[t].re, x[t].im of output part c.
//   c = 0 mark re: ( m.re, -m.im)   1 mark im: ( m.im, m.re)   2 space re: ( s.re, -s.im)   3 space im: ( s.im, s.re)
__host__ __device__ inline float bfsk_tap(const float2 *mark, const float2 *space, int c, int j)
{
    const float2 h = (c < 2 ? mark : space)[j >> 1];
    if (c & 1) return (j & 1) ? h.x : h.y;
    return (j & 1) ? -h.y : h.x;
}

// the epilogue, in the reference's order: -(|space|^2) + |mark|^2
__host__ __device__ inline float bfsk_power(float mr, float mi, float sr, float si)
{
    const float m = mr * mr + mi * mi, s = sr * sr + si * si;
    return -s + m;
}

// one output from the L samples at x (an accessor: x(t) is sample t of the window)
template <typename X>
__host__ __device__ inline float bfsk_output(const float2 *mark, const float2 *space, int L, X x)
{
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int t = 0; t < L; t++) {
        const float2 v = x(t), m = mark[t], s = space[t];
        a0 = fmaf(m.x, v.x, a0); a0 = fmaf(-m.y, v.y, a0);
        a1 = fmaf(m.y, v.x, a1); a1 = fmaf(m.x, v.y, a1);
        a2 = fmaf(s.x, v.x, a2); a2 = fmaf(-s.y, v.y, a2);
        a3 = fmaf(s.y, v.x, a3); a3 = fmaf(s.x, v.y, a3);
    }
    return bfsk_power(a0, a1, a2, a3);
}

// element size of a stage range's output
__host__ __device__ inline int rtty_out_elem(const RttyCfg &c)
{
    if (c.last == RTTY_BFSK) return 4;
    if (c.last == RTTY_SERIAL) return c.databits <= 8 ? 1 : c.databits <= 16 ? 2 : 4;
    return 1;
}

// libcsdr.c:1577-1613: the Baudot table indexed by code, letters and figures; 0b11011 / 0b11111 select figures / letters
__host__ __device__ inline uint8_t rtty_baudot_lookup(int *fig_mode, unsigned c)
{
    const uint8_t LTR[32] = {0, 'T', '\r', 'O', ' ', 'H', 'N', 'M', '\n', 'L', 'R', 'G', 'I', 'P', 'C', 'V',
                             'E', 'Z', 'D', 'B', 'S', 'Y', 'F', 'X', 'A', 'W', 'J', 0, 'U', 'Q', 'K', 0};
    const uint8_t FIG[32] = {0, '5', '\r', '9', ' ', '$', ',', '.', '\n', ')', '4', '*', '8', '0', ':', '=',
                             '3', '+', '#', '?', '\'', '6', '@', '/', '-', '2', '\a', 0, '7', '1', '(', 0};
    if (c == 0x1B) { *fig_mode = 1; return 0; }
    if (c == 0x1F) { *fig_mode = 0; return 0; }
    if (c >= 32) return 0;
    return *fig_mode ? FIG[c] : LTR[c];
}

// rtty_baudot_decoder_t (libcsdr.h:252-259) as the push function sees it
struct RttyPush { int fig_mode, character_received, shr, bit_cntr, state; };
enum { RTTY_WAITING_STOP = 0, RTTY_WAITING_START = 1, RTTY_RECEIVING = 2 };

// libcsdr.c:1615-1655, one symbol (any nonzero byte is a 1)
__host__ __device__ inline uint8_t rtty_baudot_push(RttyPush *s, unsigned symbol)
{
    const int bit = symbol != 0;
    switch (s->state) {
    case RTTY_WAITING_STOP:
        if (bit == 1) { s->state = RTTY_WAITING_START; if (s->character_received) return rtty_baudot_lookup(&s->fig_mode, (unsigned)(s->shr & 31)); }
        else s->character_received = 0;
        break;
    case RTTY_WAITING_START:
        s->character_received = 0;
        if (bit == 0) { s->state = RTTY_RECEIVING; s->shr = 0; s->bit_cntr = 0; }
        break;
    case RTTY_RECEIVING:
        s->shr = (uint16_t)((s->shr << 1) | bit);
        if (s->bit_cntr++ == 4) { s->state = RTTY_WAITING_STOP; s->character_received = 1; }
        break;
    default: break;
    }
    return 0;
}

// serial_line_decoder_f_u8 (libcsdr.c:1662-1728) on one window of n samples, x(p) = sample p of the window.  emit(shr) receives every decoded character.
// Returns input_used.  Index arithmetic as the reference compiles it: data-bit bounds in double, stop-bit bounds (int + float) in float then + double,
// the fit test and samples_used_up_now in float; all relative to the position inside the call.
// find(off, n): the first i in [1, n) with x(off + i) < 0 && x(off + i - 1) > 0, or -1 (serial_edge here; the wave-wide ballot in rtty.hip).
template <typename X>
struct SerialEdge {
    X &x;
    __host__ __device__ int operator()(int off, int n) const
    {
        for (int i = 1; i < n; i++) if (x(off + i) < 0 && x(off + i - 1) > 0) return i;
        return -1;
    }
};

template <typename X, typename E, typename F>
__host__ __device__ inline int serial_window_with(const RttyCfg &c, X &x, int n, E &emit, const F &find)
{
    int used = 0, off = 0;
    const double lo = 0.5 * (double)(1 - c.ratio), hi = 0.5 * (double)(1 + c.ratio);
    const double slo = (double)c.stopbits * 0.5 * (double)(1 - c.ratio), shi = (double)c.stopbits * 0.5 * (double)(1 + c.ratio);
    for (;;) {
        const int ss = find(off, n);
        if (ss == -1) return used + (n > 1 ? n : 1);                // the scan loop's i: n, or 1 when it never ran
        if ((float)ss + c.spb * c.all_bits >= (float)n) return used + (ss - 2 > 0 ? ss - 2 : 0);
        unsigned shr = 0;
        for (int di = 0; di < c.databits; di++) {
            const int a = (int)((double)ss + ((double)(1 + di) + lo) * (double)c.spb);
            const int b = (int)((double)ss + ((double)(1 + di) + hi) * (double)c.spb);
            float acc = 0;
            for (int p = a; p < b; p++) acc += x(off + p);
            shr = (shr << 1) | (acc > 0 ? 1u : 0u);
        }
        const float sb = (float)ss + (float)(1 + c.databits) * c.spb;
        const int a = (int)((double)sb + slo * (double)c.spb), b = (int)((double)sb + shi * (double)c.spb);
        float acc = 0;
        for (int p = a; p < b; p++) acc += x(off + p);
        if (acc < 0) return used + (ss + 1 < n ? ss + 1 : n);
        emit(shr);
        const float u = (float)ss + c.all_bits * c.spb;
        const int now = (int)((u > (float)n) ? (float)n : u);
        used += now; off += now; n -= now;
        if (!n) return used;
    }
}

template <typename X, typename E>
__host__ __device__ inline int serial_window(const RttyCfg &c, X x, int n, E &emit)
{
    const SerialEdge<X> f{x};
    return serial_window_with(c, x, n, emit, f);
}

// One call of the SERIAL (and BAUDOT) part for one channel: the stream V = remainder (rem_len samples at rem) ++ n new samples in(0 .. n), walked in windows
// of B as the CLI's bigbufs loop (csdr.c:2511-2524) does; the remainder (< B samples) goes back to rem.  emit: decoded bytes (shr, or Baudot characters).
template <typename I, typename E>
__host__ __device__ inline void serial_walk(const RttyCfg &c, RttyChan &s, float *rem, I &in, long long n, E &emit)
{
    const long long R = s.rem_len, nV = R + n;
    auto V = [&](long long p) { return p < R ? rem[p] : in(p - R); };
    long long pos = 0;
    while (nV - pos >= c.B) {
        const long long p0 = pos;
        pos += serial_window(c, [&](int p) { return V(p0 + p); }, c.B, emit);
    }
    const int nt = (int)(nV - pos);
    if (pos > 0) for (int j = 0; j < nt; j++) rem[j] = V(pos + j);      // forward: source index >= destination index
    else for (long long j = R; j < nV; j++) rem[j] = in(j - R);
    s.rem_len = nt;
}

} // namespace csdr_amd
