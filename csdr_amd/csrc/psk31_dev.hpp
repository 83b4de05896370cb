// psk31_dev.hpp -- per-channel step functions of the BPSK31 receive chain, shared by the kernel (psk31.hip) and its CPU debug entry.
//
//   simple_agc_cc        libcsdr.c:2201-2217   g = (ideal - g) rate + g (1 - rate), ideal = clamp(reference / |x|, 0, max_gain), out = g x
//   timing_recovery_cc   libcsdr.c:1977-2075   GARDNER / EARLYLATE, one symbol per decimation samples, cut-invariant through the unconsumed tail
//   dbpsk_decoder_c_u8   libcsdr.c:2319-2333   bit = |phase(x) - phase(last)| <= PI/2, phases by double atan2 rounded to float
//   psk31_varicode_decoder_push  libcsdr.c:1536-1549, as an O(1) lookup of the code between two 00 separators
//
// Every float operation is the reference's, in its order, with IEEE sqrt and division (the reference's -ffast-math build approximates both: ≤ 4 ulp apart) and
// the compiled order of the correction_offset product, (error * loop_gain) * (float)(D/2 * sign).  Separate mul / add: the sources build with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace csdr_amd {

enum { PSK31_AGC = 0, PSK31_TIMING = 1, PSK31_DBPSK = 2, PSK31_VARICODE = 3 };

struct Psk31Cfg {
    float rate, rate_1minus, reference, max_gain;
    int algorithm, D, hb, qb, wing, use_q;         // hb, qb, wing: D/2, D/4, (int)(D * 0.25f)
    float loop_gain, max_error, hb_sign;           // hb_sign: (float)(D/2 * error_sign)
    double reset_lo, reset_hi;                     // correction_offset resets when <= -qb*0.9 or >= 0.9*qb (libcsdr.c:2002)
    int first, last;                               // stage range, PSK31_AGC .. PSK31_VARICODE
};

// One channel's state between calls.  With first == PSK31_AGC, gain is the gain in front of the tail's first sample (the tail is kept raw and re-walked);
// with first == last == PSK31_AGC it is the gain after the last sample, as the reference carries it.
struct Psk31Chan {
    float gain;
    int tail_len;                  // < 3 D/2 + 1 samples of the stream not yet consumed by timing recovery
    int corr;                      // last_correction_offset
    uint32_t base;                 // absolute index of the tail's first sample (unsigned, as the CLI's --output_indexes)
    float last_i, last_q;          // dbpsk_decoder_c_u8's last_input
    unsigned long long shr;        // the varicode shift register
};

struct Psk31Out {
    float2 *c;                     // last <= PSK31_TIMING: AGC'd samples or symbols
    uint8_t *b;                    // last >= PSK31_DBPSK: bits or decoded characters
    float *err;                    // optional, last == PSK31_TIMING: the unclamped timing error per symbol
    unsigned *idx;                 // optional, last == PSK31_TIMING: absolute sample index per symbol
};

__host__ __device__ inline float psk31_ideal_gain(float i, float q, float reference, float max_gain)
{
    const float ii = i * i, qq = q * q;
    const float amplitude = sqrtf(ii + qq);        // correctly rounded (device: no bare v_sqrt_f32 / v_rsq_f32, checked in the ISA)
    float ideal = reference / amplitude;           // correctly rounded division; amplitude 0 gives inf, clamped to max_gain
    if (ideal > max_gain) ideal = max_gain;
    if (ideal <= 0) ideal = 0;
    return ideal;
}

__host__ __device__ inline float psk31_agc_step(float g, float ideal, float rate, float rate_1minus)
{
    const float a = (ideal - g) * rate, b = g * rate_1minus;
    return a + b;
}

// libcsdr.c:1536-1549.  A table entry matches when the register ends in 00 code 00; varicodes start with 1 and hold no 00, so the code is the run of bits
// below the lowest 00 above the final 00, and at most one entry can match.  dec[code] (1024 entries) gives its character, 0 for none.
__host__ __device__ inline uint8_t psk31_varicode_push(unsigned long long *shr, int bit, const uint8_t *dec)
{
    *shr = (*shr << 1) | (unsigned long long)(bit != 0);
    if (*shr & 3) return 0;
    const unsigned long long v = *shr >> 2, z = ~v & (~v >> 1);     // z: bit p set where bits p, p+1 of v are both 0 (bit 62 always is)
#ifdef __HIP_DEVICE_COMPILE__
    const int L = __ffsll((long long)z) - 1;
#else
    const int L = __builtin_ctzll(z);
#endif
    if (L < 1 || L > 10) return 0;
    return dec[v & ((1u << L) - 1)];
}

// double atan2 rounded to float, as the reference on float inputs.  The device's double atan2 (ocml) and the host's (glibc) are both within an ulp of
// the exact value but need not round alike, so a phase may differ in its last float bit at a rounding boundary: the bits are equal in practice, not by proof.
__host__ __device__ inline float psk31_phase(float i, float q) { return (float)atan2((double)q, (double)i); }

// dbpsk_decoder_c_u8 on one symbol whose phase is `phase`, against the previous symbol's phase
__host__ __device__ inline int psk31_dbpsk_bit(float phase, float last_phase)
{
    const float PI_F = 3.14159265358979323846f;
    float dphase = phase - last_phase;
    while (dphase < -PI_F) dphase += 2 * PI_F;
    while (dphase >= PI_F) dphase -= 2 * PI_F;
    return (dphase > (PI_F / 2) || dphase < (-PI_F / 2)) ? 0 : 1;
}

// The chain behind timing recovery: one symbol in, written at stage `last`.  k counts this call's outputs.
struct Psk31Tail {
    const Psk31Cfg *c; Psk31Chan *s; const Psk31Out *o; const uint8_t *dec; float last_phase; int k;
    __host__ __device__ void bit(int b)
    {
        if (c->last == PSK31_DBPSK) { o->b[k++] = (uint8_t)b; return; }
        const uint8_t ch = psk31_varicode_push(&s->shr, b, dec);
        if (ch) o->b[k++] = ch;                    // 0 (no character, or NUL) is not output (csdr.c:2418-2431)
    }
    __host__ __device__ void symbol(float i, float q)
    {
        const float ph = psk31_phase(i, q);
        const int b = psk31_dbpsk_bit(ph, last_phase);
        last_phase = ph; s->last_i = i; s->last_q = q;
        bit(b);
    }
};

// timing_recovery_cc's sample positions of the symbol at cbi (libcsdr.c:2002-2026); resets the incoming correction_offset as the reference does.
// I: the caller's index type (long long; int where a call's stream is known to stay below 2^31 samples)
template <class I> __host__ __device__ inline void psk31_positions(const Psk31Cfg &c, I cbi, int *corr, I *pl, I *pm, I *pr)
{
    if (*corr <= c.reset_lo || *corr >= c.reset_hi) *corr = 0;
    if (c.algorithm == 1) { *pr = cbi + c.wing * 3; *pl = cbi + c.wing - *corr; *pm = cbi + c.hb; }
    else { *pr = cbi + c.hb * 3; *pl = cbi + c.hb; *pm = cbi + c.hb * 2; }
}

// The timing error of one symbol from the samples at its three positions, unclamped (libcsdr.c:2027-2040)
__host__ __device__ inline float psk31_timing_error(const Psk31Cfg &c, float2 xl, float2 xm, float2 xr)
{
    float error = (xr.x - xl.x) * xm.x;
    if (c.use_q) {
        error += (xr.y - xl.y) * xm.y;
        error /= 2;
    }
    return error;
}

// The next correction_offset from a symbol's timing error (libcsdr.c:2064-2069).  A NaN error (an inf or NaN sample) corrects by 0: the conversion of a
// NaN to int is not defined, gives 0 on the device and INT_MIN on an x86 host, and the latter would walk the symbol start backwards out of the tail.
__host__ __device__ inline int psk31_correction(const Psk31Cfg &c, float error)
{
    if (!(error == error)) error = 0.f;
    if (error > c.max_error) error = c.max_error;
    if (error < -c.max_error) error = -c.max_error;
    return (int)((error * c.loop_gain) * c.hb_sign);
}

// One symbol from the (AGC'd) samples at its three positions: written at stage `last`; returns the next correction_offset (libcsdr.c:2027-2069)
__host__ __device__ inline int psk31_symbol(const Psk31Cfg &c, Psk31Chan &s, Psk31Tail &t, const Psk31Out &o, float2 xl, float2 xm, float2 xr, long long po)
{
    const float2 xo = c.algorithm == 1 ? xm : xl;
    const float error = psk31_timing_error(c, xl, xm, xr);
    if (c.last == PSK31_TIMING) {
        o.c[t.k] = xo;
        if (o.err) o.err[t.k] = error;
        if (o.idx) o.idx[t.k] = s.base + (uint32_t)po;
        t.k++;
    } else t.symbol(xo.x, xo.y);
    return psk31_correction(c, error);
}

// The stream V = tail ++ in that timing recovery reads, and the AGC walker over it: g is the gain in front of sample pos.  Symbol positions only grow, except
// that the next symbol's first position may lie behind the current one's last (by up to D/2): the walker then resumes from the latest snapshot in front of it
// (taken at the current symbol's first and mid positions, and at the stream start), which needs no history of gains.
struct Psk31Stream {
    const Psk31Cfg *c; const float2 *tail; const float2 *in; long long T0;
    long long pos, sp[3]; float g, sg[3];
    __host__ __device__ float2 raw(long long p) const { return p < T0 ? tail[p] : in[p - T0]; }
    __host__ __device__ void step(long long p)
    {
        const float2 x = raw(p);
        g = psk31_agc_step(g, psk31_ideal_gain(x.x, x.y, c->reference, c->max_gain), c->rate, c->rate_1minus);
    }
    __host__ __device__ void seek(long long p)
    {
        if (p < pos) { const int w = p >= sp[2] ? 2 : p >= sp[1] ? 1 : 0; pos = sp[w]; g = sg[w]; }
        for (; pos < p; pos++) step(pos);
    }
    // the AGC'd sample p; snap 1 / 2 records the snapshot in front of it
    __host__ __device__ float2 at(long long p, int snap)
    {
        seek(p);
        if (snap) { sp[snap] = p; sg[snap] = g; }
        step(p);
        pos = p + 1;
        const float2 x = raw(p);
        return make_float2(g * x.x, g * x.y);
    }
};

// simple_agc_cc alone: every sample out; returns the gain after the last one
__host__ __device__ inline float psk31_agc_run(const Psk31Cfg &c, float g, const float2 *in, float2 *out, long long n)
{
    for (long long j = 0; j < n; j++) {
        const float2 x = in[j];
        g = psk31_agc_step(g, psk31_ideal_gain(x.x, x.y, c.reference, c.max_gain), c.rate, c.rate_1minus);
        out[j] = make_float2(g * x.x, g * x.y);
    }
    return g;
}

// One call of the chain for one channel: n new samples (complex for first <= PSK31_DBPSK, bits for PSK31_VARICODE).  tail: this channel's tail buffer
// (complex, capacity 3 D/2 + 1).  Returns the number of outputs written.
__host__ __device__ inline int psk31_walk(const Psk31Cfg &c, Psk31Chan &s, float2 *tail, const float2 *in, const uint8_t *in_bits, long long n,
                                          const Psk31Out &o, const uint8_t *dec)
{
    if (c.first == PSK31_VARICODE) {
        Psk31Tail t{&c, &s, &o, dec, 0.f, 0};
        for (long long j = 0; j < n; j++) t.bit(in_bits[j]);
        return t.k;
    }
    if (c.first == PSK31_DBPSK) {
        Psk31Tail t{&c, &s, &o, dec, psk31_phase(s.last_i, s.last_q), 0};
        for (long long j = 0; j < n; j++) t.symbol(in[j].x, in[j].y);
        return t.k;
    }
    if (c.last == PSK31_AGC) { s.gain = psk31_agc_run(c, s.gain, in, o.c, n); return (int)n; }
    // timing recovery over V = tail ++ in
    const long long T0 = s.tail_len, nV = T0 + n;
    const bool agc = c.first == PSK31_AGC;
    Psk31Stream v{&c, tail, in, T0, 0, {0, 0, 0}, s.gain, {s.gain, s.gain, s.gain}};
    Psk31Tail t{&c, &s, &o, dec, c.last >= PSK31_DBPSK ? psk31_phase(s.last_i, s.last_q) : 0.f, 0};
    long long cbi = 0;
    int corr = s.corr;
    while (cbi + c.hb * 3 < nV) {                                                 // libcsdr.c:1998
        long long pl, pm, pr;
        psk31_positions(c, cbi, &corr, &pl, &pm, &pr);
        float2 xl, xm, xr;
        if (agc) { xl = v.at(pl, 1); xm = v.at(pm, 2); xr = v.at(pr, 0); }
        else { xl = v.raw(pl); xm = v.raw(pm); xr = v.raw(pr); }
        corr = psk31_symbol(c, s, t, o, xl, xm, xr, c.algorithm == 1 ? pm : pl);
        cbi += c.D + corr;
    }
    // the unconsumed tail V[cbi ..) stays, raw, with the gain in front of it
    if (agc) { v.seek(cbi); s.gain = v.g; }
    const int nt = (int)(nV - cbi);
    if (cbi > 0) for (int j = 0; j < nt; j++) tail[j] = v.raw(cbi + j);           // forward: source index >= destination index
    else for (long long j = T0; j < nV; j++) tail[j] = in[j - T0];
    s.tail_len = nt;
    s.corr = corr;
    s.base += (uint32_t)cbi;
    return t.k;
}

} // namespace csdr_amd
