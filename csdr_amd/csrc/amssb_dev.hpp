// amssb_dev.hpp -- step functions of the AM / SSB audio tail, shared by both kernels of amssb.hip and the CPU hook: the single definition of its arithmetic.
//
//   AM    amdemod_cf       libcsdr.c:861-870     sqrt(i i + q q): the float sum, its square root correctly rounded to float
//         fastdcblock_ff   libcsdr.c:920-941     per block of B samples: avg = sum / B; out[i] = x[i] - (last_dc + (avg - last_dc) ((float)i / B)); last_dc = avg
//   SSB   realpart_cf      csdr.c:634-645
//   both  agc_ff           libcsdr_gpl.c:163-260 one call per block: out[0] = last_gain in[0], counters zeroed, last_peak = reference / last_gain
//         limit_ff         libcsdr.c:1130-1137
//         convert_f_s16    libcsdr.c:2397        x86 truncation semantics: NaN and values beyond int32 give 0x80000000, whose low half is 0
//
// Every float operation is the reference's, in its order (the sources build with -ffp-contract=off), with one exception that has to be fixed somewhere: the
// order of the block sum.  The reference adds the B samples one after the other (its -ffast-math build in whatever order the vectoriser chose); here the
// order is amssb_block_sum's, once: 64 partial sums, partial l over the samples l, l + 64, l + 128, ... in rising order, then a pairwise tree
// p[l] += p[l + w] for w = 32, 16, ... 1.  A wave forms the partials one per lane and the tree with five lane shifts; the one-lane kernel and the hook run the
// same additions from an array.
//
// agc_ff's nested ifs are evaluated branch free, as k_agc_coop (f2blocks.hip) does: every path's values are formed and the taken one selected, so the
// operations on the taken path, and with them the values, are the reference's.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace csdr_amd {

enum { AMSSB_AM = 0, AMSSB_SSB = 1 };

struct AmSsbCfg { int mode, block; float reference, attack_rate, decay_rate, max_gain; int hang_time, attack_wait_time; float alpha, limit_max; };
struct AmSsbChan { float last_dc, last_gain; };                         // what the CLI's fastdcblock_ff and agc_ff loops carry (csdr.c:957, 1365)
struct AgcCall { float gain, last_gain, last_peak; int hang, aw; };     // the locals of one agc_ff call

// amdemod_cf of one sample.  The square root of a float taken in double and rounded to float is the correctly rounded float square root.
__host__ __device__ inline float amssb_envelope(float i, float q) { const float s = i * i + q * q; return (float)sqrt((double)s); }

// the block sum of x(0) .. x(n - 1) in the fixed order, from one lane
template <class F> __host__ __device__ inline float amssb_block_sum(int n, F x)
{
    float p[64];
#pragma unroll
    for (int l = 0; l < 64; l++) p[l] = 0.f;
    for (int i0 = 0; i0 < n; i0 += 64) {
#pragma unroll
        for (int l = 0; l < 64; l++)
            if (i0 + l < n) p[l] = p[l] + x(i0 + l);
    }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) {
#pragma unroll
        for (int l = 0; l < 32; l++)
            if (l < w) p[l] = p[l] + p[l + w];
    }
    return p[0];
}
__host__ __device__ inline float amssb_block_mean(float sum, int block) { return sum / block; }
// fastdcblock_ff's output i of a block
__host__ __device__ inline float amssb_dc_ramp(float x, float last_dc, float avg, int i, int block)
{
    const float avgdiff = avg - last_dc;
    const float level = last_dc + avgdiff * ((float)i / block);
    return x - level;
}

// reference / |x|: the state-independent division of agc_ff's error
__host__ __device__ inline float amssb_agc_ratio(const AmSsbCfg &c, float v) { return c.reference / fabsf(v); }

// a call's first sample: out[0] = last_gain * in[0]; returns that factor
__host__ __device__ inline float agc_call_begin(const AmSsbCfg &c, AgcCall &a, float last_gain)
{
    a.hang = 0; a.aw = 0;
    a.gain = last_gain; a.last_gain = last_gain; a.last_peak = c.reference / last_gain;
    return last_gain;
}
// every further sample v, r = amssb_agc_ratio(v): returns the filtered gain that scales it
__host__ __device__ inline float agc_call_step(const AmSsbCfg &c, AgcCall &a, float v, float r)
{
    const float av = fabsf(v);
    const float error = r - a.gain;
    const bool nz = v != 0, neg = error < 0;
    // error < 0: attack (with its wait counter and the peak estimate)
    const bool newpeak = a.last_peak < av;
    const int aw_a = newpeak ? c.attack_wait_time : a.aw;
    const float lp_a = newpeak ? av : a.last_peak;
    const bool waiting = aw_a > 0;
    const float dg_a = waiting ? 0.f : error * c.attack_rate;
    const int aw_a2 = waiting ? aw_a - 1 : aw_a;
    const int hang_a = waiting ? a.hang : c.hang_time;
    // error >= 0: decay (behind the hang counter)
    const bool hanging = a.hang > 0;
    const float dg_d = hanging ? 0.f : error * c.decay_rate;
    const int hang_d = hanging ? a.hang - 1 : a.hang;
    const float dgain = neg ? dg_a : dg_d;
    const float g1 = nz ? a.gain + dgain : a.gain;
    if (nz) { a.hang = neg ? hang_a : hang_d; a.aw = neg ? aw_a2 : a.aw; a.last_peak = neg ? lp_a : a.last_peak; }
    float g2 = g1 > c.max_gain ? c.max_gain : g1;
    g2 = g2 < 0 ? 0.f : g2;
    a.gain = g2 + a.last_gain - c.alpha * a.last_gain;
    a.last_gain = a.gain;
    return a.gain;
}

// agc_call_step for v == 0, as a map of the gain alone: nz is false, so the hang counter, the wait counter and the peak stay, g1 is the gain, and gain ==
// last_gain holds at every step of a call.  The operations below are agc_call_step's from g2 on, in its order.
__host__ __device__ inline float amssb_agc_zero_step(const AmSsbCfg &c, float g)
{
    float g2 = g > c.max_gain ? c.max_gain : g;
    g2 = g2 < 0 ? 0.f : g2;
    return g2 + g - c.alpha * g;
}
__host__ __device__ inline uint32_t amssb_float_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
// The gain after n applications of amssb_agc_zero_step.  The map is a pure function of one float, so once a gain repeats one of the four before it, bit
// for bit, the sequence is periodic from there and the rest is an index into those four.  Without a repeat (none is known: in float32 the map runs into a
// cycle of period 1 to 3 for every parameter set tried) every step is taken.  *steps_iterated: the applications actually performed.
__host__ __device__ inline float amssb_agc_zero_run(const AmSsbCfg &c, float g, long long n, long long *steps_iterated = nullptr)
{
    float h0 = g, h1 = g, h2 = g, h3 = g;                // the gains 1, 2, 3, 4 steps back (before that many steps exist: the start, which comes first in the search)
    long long i = 0;
    float out = g;
    while (i < n) {
        const float gn = amssb_agc_zero_step(c, h0);
        i++;
        const uint32_t b = amssb_float_bits(gn);
        const int p = b == amssb_float_bits(h0) ? 1 : b == amssb_float_bits(h1) ? 2 : b == amssb_float_bits(h2) ? 3 : b == amssb_float_bits(h3) ? 4 : 0;
        if (p) {                                         // step i equals step i - p: step i + r is step i - p + (r mod p), the gain p - (r mod p) steps back
            const int k = p - (int)((n - i) % p);
            out = k == 1 ? h0 : k == 2 ? h1 : k == 3 ? h2 : h3;
            break;
        }
        h3 = h2; h2 = h1; h1 = h0; h0 = gn;
        out = gn;
    }
    if (steps_iterated) *steps_iterated = i;
    return out;
}

// agc_ff's scaling, limit_ff and convert_f_s16 of one sample: x the pre-AGC sample, g its gain
__host__ __device__ inline int16_t amssb_finish(const AmSsbCfg &c, float g, float x)
{
    float v = g * x;
    v = (c.limit_max < v) ? c.limit_max : v; v = (-c.limit_max > v) ? -c.limit_max : v;      // libcsdr.c:1133-1136
    const float scaled = v * 32767.0f;
    const int t = (scaled >= -2147483648.0f && scaled < 2147483648.0f) ? (int)scaled : (int)0x80000000;
    return (int16_t)(t & 0xffff);
}

} // namespace csdr_amd
