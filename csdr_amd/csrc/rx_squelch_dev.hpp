// rx_squelch_dev.hpp -- the squelch in front of a receive bank's fused path: what a gated launch knows about the squelch (FmrxSq), the power pass and the carry of
// the samples behind the last whole block.  Shared by the two banks that gate their front kernels: csdr_amd_fmrx (fmrx.hip) and csdr_amd_wfmrx (wfmrx.hip): one
// definition, so both compute csdr_amd_squelch's bits (squelch_dev.hpp's order: 512 chains by sample index, then the tree).
#pragma once
#include "common.hpp"
#include "squelch_dev.hpp"

namespace csdr_amd {
namespace {

// the squelch in front of a gated launch: the call's gated sample k is held[k] for k < h, else in[k - h], and (0, 0) when flags[k / B] is 0
struct FmrxSq { const float2 *held; const uint8_t *flags; size_t fl_pitch; int h, B, shift; };      // held [n_ch][B], flags [n_ch][fl_pitch]; shift: log2 B, or -1
__device__ __forceinline__ int fmrx_sq_block(const FmrxSq &q, int k) { return q.shift >= 0 ? k >> q.shift : k / q.B; }      // (k >= 0; the branch is the same for every lane)

// grid (ceil(nb n_ch / 4)), 256 threads, one wave per (channel, block): block k of channel ch over (held ++ call) in squelch_dev.hpp's order -> its power and
// open flag to the object's rows (q.flags' layout) and to the caller's (pitch power_pitch) where given.  Lane l takes the samples 128 r + 2 l, + 1 of the
// block's rows r of 128, four rows' loads at a time: chains 128 (r mod 4) + 2 l, + 1, each added to in increasing sample order; pairs in the call's rows on an
// even row index are one 16-byte load.  lv: n_ch levels of the blocks this call starts, then n_ch of the block begun earlier.
__global__ __launch_bounds__(256) void k_fmrx_power(const float2 *__restrict__ in, size_t in_pitch, FmrxSq q, int d, int nb, int n_ch, const float *__restrict__ lv,
                                                    float *__restrict__ own_power, uint8_t *__restrict__ own_flags, float *__restrict__ power, uint8_t *__restrict__ flags,
                                                    size_t power_pitch)
{
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= (long long)n_ch * nb) return;                              // (the whole wave)
    const int ch = (int)(g / nb), k = (int)(g % nb), B = q.B;
    const float2 *cr = q.held + (size_t)ch * B, *x = in + (size_t)ch * in_pitch;
    const long long j0 = (long long)k * B - q.h;                        // the block's first sample as a row index (negative: held)
    const float fB = (float)B;
    float acc[4][2] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
    for (int s0 = 0; s0 < B; s0 += 512) {
        float2 u[4][2];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int s = s0 + 128 * r + 2 * lane;
            const long long j = j0 + s;
            u[r][0] = u[r][1] = make_float2(0.f, 0.f);
            if (s + 1 < B && j >= 0 && !(j & 1)) {
                const float4 v = *reinterpret_cast<const float4 *>(x + j);
                u[r][0] = make_float2(v.x, v.y); u[r][1] = make_float2(v.z, v.w);
            } else {
#pragma unroll
                for (int e = 0; e < 2; e++) if (s + e < B) u[r][e] = j + e < 0 ? cr[j + e + q.h] : x[j + e];
            }
        }
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const int s = s0 + 128 * r + 2 * lane + e;
                if (s < B && (d == 1 || s % d == 0)) acc[r][e] = acc[r][e] + squelch_term_c(u[r][e].x, u[r][e].y, fB);
            }
    }
    const float P = squelch_wave_tree(acc);
    const bool open = squelch_open(P, lv[(k == 0 && q.h > 0 ? n_ch : 0) + ch]);
    if (lane == 0) {
        own_power[(size_t)ch * q.fl_pitch + k] = P; own_flags[(size_t)ch * q.fl_pitch + k] = open;
        if (power) power[(size_t)ch * power_pitch + k] = P;
        if (flags) flags[(size_t)ch * power_pitch + k] = open;
    }
}

// grid (ceil(min(n_in, B) / 256), n_ch): what lies behind the call's last whole block, to the channel's row of `carry`.  m == 0 (no whole block): the call's samples
// are appended behind the h held ones, in the buffer that holds them; otherwise all that is left lies in the call's rows, from m - h on
__global__ __launch_bounds__(256) void k_fmrx_sq_carry(const float2 *__restrict__ in, size_t in_pitch, int n_in, float2 *__restrict__ carry, int h, int B, int m)
{
    const int ch = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const float2 *x = in + (size_t)ch * in_pitch;
    float2 *cr = carry + (size_t)ch * B;
    if (m == 0) { if (j < n_in) cr[h + j] = x[j]; }
    else if (j < h + n_in - m) cr[j] = x[m - h + j];
}

} // namespace
} // namespace csdr_amd
