// noise_dev.hpp -- the noise sources and the AWGN channel (get_random_samples_f / get_random_gaussian_samples_c libcsdr.c:2444-2466, awgn_cc csdr.c:3035-3091),
// shared by the kernels (noise.hip), their CPU debug entry and the drop-ins (compat.cpp).
//
// The reference turns 32-bit words read from a FILE* into samples; only where the words come from is left open.  Here they come from Philox4x32-10
// (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85: Salmon et al., SC'11), a counter-based generator, so a channel's stream is a
// pure function of (seed, stream id, sample index): reproducible, seekable and independent of how the calls cut it.
//   block(kind, s, j) = philox(ctr = (j lo, j hi, s, kind), key = (seed lo, seed hi))          kind 0 Gaussian, 1 uniform; s the channel's stream id
//   Gaussian complex sample i: words 2 (i & 1), 2 (i & 1) + 1 of block(0, s, i >> 1)           (the reference's pioutput[2 i], pioutput[2 i + 1])
//   uniform float k:           word k & 3 of block(1, s, k >> 2)
// Words to samples, as the reference has it:
//   uniform   (float)(int)w / 2147483648.0f                                                     in [-1, 1]
//   Gaussian  u_k = (float)(0.5 + 0.49999999 * (double)((float)(int)w_k / 2147483648.0f));  r = sqrt(-2 ln u_0);  I = r cos(2 pi u_1), Q = r sin(2 pi u_1)
// ln, sin(2 pi u) and cos(2 pi u) are written out below from +, *, fmaf, integer and bit operations (and sqrtf, correctly rounded in both builds), so that
// the host build and the gfx950 build of this header give the same bits: the kernels are held to the CPU entry bit for bit, and the CPU entry to a float64
// model within a gate.  -ffp-contract=off (the Makefile): a product and a sum stay two roundings unless the source says fmaf.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace csdr_amd {

enum { NOISE_GAUSSIAN = 0, NOISE_UNIFORM = 1 };

// One channel's state between calls (mirrored by csdr_amd_noise_chan)
struct NoiseChan {
    unsigned long long pos;                        // index of the next sample of the channel's stream
    unsigned stream_id;
    float a_signal, g_noise;                       // awgn_cc: out = in * a_signal + noise * g_noise
    unsigned pad;
};

struct PhiloxBlock { uint32_t w[4]; };

__host__ __device__ inline PhiloxBlock philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return PhiloxBlock{{c0, c1, c2, c3}};
}

__host__ __device__ inline PhiloxBlock noise_block(int kind, unsigned long long seed, unsigned stream_id, unsigned long long j)
{
    return philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), stream_id, (uint32_t)kind, (uint32_t)seed, (uint32_t)(seed >> 32));
}

__host__ __device__ inline float noise_uniform(uint32_t w) { return (float)(int32_t)w * 4.656612873077393e-10f; }     // 2^-31: exact, as the division is

// u_k: 1e-8 (w = INT_MIN) .. 1.0f (w = INT_MAX, whose float is 2^31); formed in double as the reference forms it
__host__ __device__ inline float noise_unit(uint32_t w) { return (float)(0.5 + 0.49999999 * (double)noise_uniform(w)); }

// ln u for a normal positive float: u = m 2^e with m in [sqrt(1/2), sqrt(2)), f = m - 1 (exact), ln m = f - f^2/2 + f^3 G(f) with G the degree-9
// interpolant of (log1p(f) - f + f^2/2) / f^3 at the Chebyshev points of the interval (5e-10 of ln m before rounding), e ln 2 added in two parts
__host__ __device__ inline float noise_ln(float u)
{
    const uint32_t b = __builtin_bit_cast(uint32_t, u);
    const int e = (int)(b - 0x3f3504f3u) >> 23;
    const float f = __builtin_bit_cast(float, b - ((uint32_t)e << 23)) - 1.0f;
    float g = -0.062015000730752945f;
    g = fmaf(g, f, 0.1053086444735527f);
    g = fmaf(g, f, -0.10646191984415054f);
    g = fmaf(g, f, 0.11037783324718475f);
    g = fmaf(g, f, -0.12450743466615677f);
    g = fmaf(g, f, 0.14286524057388306f);
    g = fmaf(g, f, -0.1666800081729889f);
    g = fmaf(g, f, 0.2000001072883606f);
    g = fmaf(g, f, -0.24999989569187164f);
    g = fmaf(g, f, 0.3333333432674408f);
    const float l = fmaf(f * f, fmaf(f, g, -0.5f), f);
    const float fe = (float)e;
    return fmaf(fe, 6.9313812256e-01f, fmaf(fe, 9.0580006145e-06f, l));            // fe * ln2_hi is exact (ln2_hi has 16 bits)
}

// sin and cos of 2 pi u for u in [0, 1]: q = round(4 u), f = u - q / 4 (exact, |f| <= 1/8), x = 2 pi f with 2 pi in two parts, the Taylor sums of sin x
// and cos x to x^9 and x^10 (|x| <= pi/4: 2e-9 and 1e-10 left out), then the quarter turn q
__host__ __device__ inline void noise_sincos2pi(float u, float *s, float *c)
{
    const int q = (int)fmaf(4.f, u, 0.5f);
    const float f = fmaf(-0.25f, (float)q, u);
    const float x = fmaf(f, 6.2831855f, f * -1.7484555e-07f), x2 = x * x;
    float ps = 2.7557319e-06f;
    ps = fmaf(ps, x2, -1.9841270e-04f);
    ps = fmaf(ps, x2, 8.3333333e-03f);
    ps = fmaf(ps, x2, -1.6666667e-01f);
    const float sx = fmaf(x * x2, ps, x);
    float pc = -2.7557319e-07f;
    pc = fmaf(pc, x2, 2.4801587e-05f);
    pc = fmaf(pc, x2, -1.3888889e-03f);
    pc = fmaf(pc, x2, 4.1666667e-02f);
    pc = fmaf(pc, x2, -0.5f);
    const float cx = fmaf(x2, pc, 1.0f);
    switch (q & 3) {
    case 0: *s = sx; *c = cx; break;
    case 1: *s = cx; *c = 0.f - sx; break;
    case 2: *s = 0.f - sx; *c = 0.f - cx; break;
    default: *s = 0.f - cx; *c = sx; break;
    }
}

// one Gaussian complex sample from its two words; w0 = INT_MAX: u_0 == 1, r == +0 and the sample is 0
__host__ __device__ inline float2 noise_gauss(uint32_t w0, uint32_t w1)
{
    const float r = sqrtf(0.f - 2.f * noise_ln(noise_unit(w0)));
    float s, c;
    noise_sincos2pi(noise_unit(w1), &s, &c);
    return make_float2(r * c, r * s);
}

// sample i of a channel's stream
__host__ __device__ inline float2 noise_gauss_at(unsigned long long seed, unsigned stream_id, unsigned long long i)
{
    const PhiloxBlock b = noise_block(NOISE_GAUSSIAN, seed, stream_id, i >> 1);
    return (i & 1) ? noise_gauss(b.w[2], b.w[3]) : noise_gauss(b.w[0], b.w[1]);
}
__host__ __device__ inline float noise_uniform_at(unsigned long long seed, unsigned stream_id, unsigned long long k)
{
    return noise_uniform(noise_block(NOISE_UNIFORM, seed, stream_id, k >> 2).w[k & 3]);
}

// awgn_cc's sample (csdr.c:3078-3087: gain_ff, gain_ff, add_ff): two rounded products, then one rounded sum, per part
__host__ __device__ inline float2 awgn_mix(float2 x, float2 nz, float a_signal, float g_noise)
{
    const float sr = x.x * a_signal, si = x.y * a_signal, nr = nz.x * g_noise, ni = nz.y * g_noise;
    return make_float2(sr + nr, si + ni);
}

// normalized_timing_variance_u32_f libcsdr.c:2293-2317 on `n` sample indexes (idx(i)): the reference's unsigned arithmetic and running mean, rad(i)
// recomputed in the second pass in place of its temp buffer.  n == 1 divides 0 by 0 as the reference does: NaN.  n == 0: 0.
template <typename Idx>
__host__ __device__ inline float timing_variance(Idx idx, int n, int samples_per_symbol, int initial_sample_offset)
{
    const unsigned sps = (unsigned)samples_per_symbol, off = (unsigned)initial_sample_offset;
    auto rad = [&](int i) {
        const unsigned v = idx(i);
        unsigned nearest = (v - off) / sps;
        if ((v - off) % sps > sps / 2) nearest++;
        const unsigned correct = off + nearest * sps;
        int d = (int)(correct - v);
        if (d < 0) d = -d;
        return (float)d / (float)samples_per_symbol * 3.14159265358979323846f;
    };
    float mean = 0.f;
    for (int i = 0; i < n; i++) mean = mean * ((float)i / (float)(i + 1)) + rad(i) / (float)(i + 1);
    float result = 0.f;
    for (int i = 0; i < n; i++) { const float d = rad(i) - mean; result += d * d / (float)(n - 1); }
    return result;
}

} // namespace csdr_amd
