// psk31tx_dev.hpp -- per-channel step functions of the BPSK31 transmit chain, shared by the generic kernel (psk31tx.hip) and its CPU debug entry.
//
//   psk31_varicode_encoder_u8_u8   libcsdr.c:1551-1575   a table character's code MSB first, then 00, one bit per byte; other bytes give nothing
//   differential_codec (encode)    libcsdr.c:1836-1841   a zero byte toggles the state, the output is the state
//   psk_modulator_u8_c             libcsdr.c:1772-1782   (cos, sin) of float(2 pi / n_psk) * byte: a lookup in the 256 symbols the host computed
//   psk31_interpolate_sine_cc      libcsdr.c:1793-1808   out = sym * rate[j] + last * (1 - rate[j]), j < I, then last = sym
//
// Every float operation is the reference's, in its order: separate mul / add (the sources build with -ffp-contract=off), rate and 1 - rate as floats
// from the host's tables, and the sum rate + (1 - rate) computed also when a symbol repeats.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace csdr_amd {

enum { PSK31TX_VARICODE = 0, PSK31TX_DIFF = 1, PSK31TX_MOD = 2, PSK31TX_SHAPE = 3 };

struct Psk31TxCfg { int first, last, I; };

// One channel's state between calls (mirrors csdr_amd_psk31tx_chan)
struct Psk31TxChan {
    uint8_t diff_state;            // differential_codec's state: 0 or 1
    float last_i, last_q;          // psk31_interpolate_sine_cc's last_input
};

// Device (or host) tables of one object
struct Psk31TxTab {
    const uint16_t *vc;            // 128 entries: code | length << 10
    const float2 *sym;             // 256 symbols of psk_modulator_u8_c
    const float *rate, *rate1m;    // I entries each: rate[j] and 1 - rate[j]
};

__host__ __device__ inline int psk31tx_popc(unsigned v)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __popc(v);
#else
    return __builtin_popcount(v);
#endif
}

// length + 2 of character c's code (0: not a table character) and the parity of its zero bits, the two separators included
__host__ __device__ inline int psk31tx_char_bits(const uint16_t *vc, uint8_t c, int *zero_parity)
{
    if (c >= 128) { *zero_parity = 0; return 0; }
    const unsigned e = vc[c], len = e >> 10;
    *zero_parity = (int)((len - psk31tx_popc(e & 1023u) + 2) & 1);
    return (int)len + 2;
}

// bit bi < len + 2 of an entry: the code MSB first, then two zeros
__host__ __device__ inline int psk31tx_code_bit(unsigned e, int bi)
{
    const int len = (int)(e >> 10);
    return bi < len ? (int)((e >> (len - bi - 1)) & 1u) : 0;
}

__host__ __device__ inline float2 psk31tx_shape(float2 x, float2 last, float rate, float rate1m)
{
    const float ai = x.x * rate, bi = last.x * rate1m, aq = x.y * rate, bq = last.y * rate1m;
    return make_float2(ai + bi, aq + bq);
}

// The chain behind one stage's output: an item goes in at its stage and is written at stage `last`.  k counts this call's outputs.
struct Psk31TxTail {
    const Psk31TxCfg *c; Psk31TxChan *s; const Psk31TxTab *t; uint8_t *ob; float2 *oc; long long k;
    __host__ __device__ void symbol(float2 x)
    {
        const float2 last = make_float2(s->last_i, s->last_q);
        for (int j = 0; j < c->I; j++) oc[k++] = psk31tx_shape(x, last, t->rate[j], t->rate1m[j]);
        s->last_i = x.x; s->last_q = x.y;
    }
    __host__ __device__ void index(uint8_t v)
    {
        const float2 x = t->sym[v];
        if (c->last == PSK31TX_MOD) oc[k++] = x; else symbol(x);
    }
    __host__ __device__ void diff(uint8_t b)
    {
        if (!b) s->diff_state = !s->diff_state;
        if (c->last == PSK31TX_DIFF) ob[k++] = s->diff_state; else index(s->diff_state);
    }
    __host__ __device__ void bit(uint8_t b) { if (c->last == PSK31TX_VARICODE) ob[k++] = b; else diff(b); }
    __host__ __device__ void character(uint8_t ch)
    {
        if (ch >= 128) return;
        const unsigned e = t->vc[ch];
        const int n = (int)(e >> 10) + 2;
        for (int bi = 0; bi < n; bi++) bit((uint8_t)psk31tx_code_bit(e, bi));
    }
};

// One call of the chain for one channel: n new items (bytes, or complex when first is SHAPE).  Returns the number of outputs written.
__host__ __device__ inline long long psk31tx_walk(const Psk31TxCfg &c, Psk31TxChan &s, const Psk31TxTab &t, const uint8_t *in_b, const float2 *in_c, long long n,
                                                  uint8_t *out_b, float2 *out_c)
{
    Psk31TxTail w{&c, &s, &t, out_b, out_c, 0};
    switch (c.first) {
        case PSK31TX_VARICODE: for (long long j = 0; j < n; j++) w.character(in_b[j]); break;
        case PSK31TX_DIFF:     for (long long j = 0; j < n; j++) w.diff(in_b[j]); break;
        case PSK31TX_MOD:      for (long long j = 0; j < n; j++) w.index(in_b[j]); break;
        default:               for (long long j = 0; j < n; j++) w.symbol(in_c[j]); break;
    }
    return w.k;
}

} // namespace csdr_amd
