// squelch_dev.hpp -- step functions of squelch_and_smeter_cc, shared by every kernel of squelch.hip and by the CPU hook.
//
//   get_power_c / get_power_f   libcsdr.c:1144-1162   P = sum over s = 0, d, 2d, .. < B of (i*i + q*q) / B     (the divisor is B, not the term count)
//   squelch_and_smeter_cc       csdr.c:2192-2243      a block passes if level == 0 || P >= level (a NaN power closes the gate unless level == 0);
//                                                     block k reports its power when k mod (report_every_nth + 2) == report_every_nth + 1
//
// The summation order (the reference sums sequentially; the library's order is its own and is the same everywhere):
//   term(s)  = (i*i + q*q) / (float)B, every operation rounded on its own (the sources build with -ffp-contract=off)
//   chain[c] = the terms of the samples s with s mod 512 == c, added in increasing s, from +0        c = 0 .. 511   (samples with s mod d != 0 add nothing)
//   tree     = for h = 256, 128, .., 1:  chain[c] += chain[c + h]  for c < h;   P = chain[0]
// A lane that holds the samples 2 l, 2 l + 1 of every row of 128 (one wave per block) or of 512 (one workgroup per block) owns its chains outright, so the
// chains run in parallel and the tree is register adds, LDS reads and lane shifts.  The power bits of a block therefore do not depend on the kernel that
// served it, its position in the batch or how the calls cut the stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace csdr_amd {

constexpr int SQ_CHAINS = 512;

__host__ __device__ inline float squelch_term_c(float i, float q, float fB) { return (i * i + q * q) / fB; }
__host__ __device__ inline float squelch_term_f(float x, float fB) { return (x * x) / fB; }

// the tree over n chains (n a power of two <= 512), in place; chain[0] is the result
__host__ __device__ inline float squelch_tree(float *chain, int n)
{
    for (int h = n / 2; h >= 1; h >>= 1)
        for (int c = 0; c < h; c++) chain[c] = chain[c] + chain[c + h];
    return chain[0];
}

// the whole power of one block on one thread: term_at(s) gives the term of sample s
template <class Term> __host__ __device__ inline float squelch_power_serial(int B, int d, Term term_at)
{
    float chain[SQ_CHAINS];
    for (int c = 0; c < SQ_CHAINS; c++) chain[c] = 0.f;
    for (long long s = 0; s < B; s += d) chain[s & (SQ_CHAINS - 1)] = chain[s & (SQ_CHAINS - 1)] + term_at((int)s);
    return squelch_tree(chain, SQ_CHAINS);
}

// csdr.c:2230
__host__ __device__ inline bool squelch_open(float power, float level) { return level == 0.f || power >= level; }

// csdr.c:2224-2229: `if (report_cntr++ > report_every_nth) report_cntr = 0` fires on the blocks k with k mod (report_every_nth + 2) == report_every_nth + 1
__host__ __device__ inline bool squelch_report_due(int report_every_nth, long long block_index)
{
    const long long period = (long long)report_every_nth + 2;
    return block_index >= 0 && block_index % period == period - 1;
}

#ifdef __HIPCC__
// Device: the last 128 chains' worth of the tree for one wave.  a[k][e] = chain[128 k + 2 lane + e]; every lane returns P.
__device__ __forceinline__ float squelch_wave_tree(float (&a)[4][2])
{
#pragma unroll
    for (int e = 0; e < 2; e++) { a[0][e] = a[0][e] + a[2][e]; a[1][e] = a[1][e] + a[3][e]; }      // h = 256
#pragma unroll
    for (int e = 0; e < 2; e++) a[0][e] = a[0][e] + a[1][e];                                        // h = 128
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {                                                          // h = 64 .. 2: chain 2 l + e takes chain 2 (l + h / 2) + e
        const float u0 = __shfl_down(a[0][0], sh), u1 = __shfl_down(a[0][1], sh);
        a[0][0] = a[0][0] + u0; a[0][1] = a[0][1] + u1;
    }
    return __shfl(a[0][0] + a[0][1], 0);                                                            // h = 1
}
// Device: the 512 chains of a workgroup of 256 (thread t: chains 2 t, 2 t + 1; sh: SQ_CHAINS floats of LDS) -> P in every thread
__device__ __forceinline__ float squelch_wg_tree(float (&acc)[2], float *sh)
{
    *reinterpret_cast<float2 *>(sh + 2 * threadIdx.x) = make_float2(acc[0], acc[1]);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    float t[4][2];
#pragma unroll
    for (int k = 0; k < 4; k++) { const float2 u = *reinterpret_cast<const float2 *>(sh + 128 * k + 2 * lane); t[k][0] = u.x; t[k][1] = u.y; }
    return squelch_wave_tree(t);
}
#endif

} // namespace csdr_amd
