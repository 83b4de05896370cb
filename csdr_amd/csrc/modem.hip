// modem.hip -- the pulse-shaped symbol modem for n_channels channels per call (MI355X / gfx950):
//   psk_modulator_u8_c n_psk | plain_interpolate_cc I | pulse_shaping_filter_cc (apply_real_fir_cc, T taps)        (modem_dev.hpp: the definitions)
// as one object, and the flat operators generic_slicer_f_u8, plain_interpolate_cc, pack_bits_1to8_u8_u8, pack_bits_8to1_u8_u8, apply_real_fir_cc and the
// designs firdes_rrc_f / firdes_cosine_f; and the receive side, the matched filter | timing_recovery_cc | [realpart_cf |] gain_ff | generic_slicer_f_u8 as
// one object that evaluates the filter only where the timing loop reads it (k_pulserx_tiled, k_pulserx_generic: described where they stand).
//
// The composed chain writes the zero-stuffed stream (8 I bytes per symbol), reads it back through a T-tap FIR in which all but ceil(T / I) products are zero,
// and writes the result.  The object reads a byte (or a complexf) per symbol and writes every output once.
//   k_pulsetx_poly     a workgroup of 256 lanes per (channel, tile of TILE_O = 4096 outputs = 32 KiB): the symbols the tile reaches (the held history, the
//                      call's bytes through the 256-symbol table, or its complexf) and the taps, padded with zeros to K I, in LDS.  A lane computes two consecutive
//                      outputs per step and stores them as one 16-byte store, a wave 1 KiB of a row per instruction.  The two outputs start on the same symbol
//                      or on neighbours, so one LDS read per product serves both; the taps a wave reads for one k are consecutive words, I-periodic.
//                      A row that starts on an odd complex sample pairs its samples one further; its first and last sample go out as 8-byte stores.
//   k_pulsetx_generic  one thread per output, symbols and taps from global memory (modem_dev.hpp's pulsetx_output); every stage range and shape.
//   k_pulsetx_hist     the H symbols behind the call into the other half of the history buffer.
// Both output kernels add the same products in the same order (ascending t, fmaf), so they give the same bits.
#include "bank.hpp"
#include "modem_dev.hpp"
#include <limits.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>

using namespace csdr_amd;

namespace {

constexpr int POLY_THREADS = 256;
#ifndef PULSETX_POLY_STEPS
#define PULSETX_POLY_STEPS 8
#endif
constexpr int POLY_STEPS = PULSETX_POLY_STEPS;                    // 16-byte stores per lane
constexpr int TILE_O = 2 * POLY_THREADS * POLY_STEPS;             // 4096 outputs (32 KiB) per workgroup
constexpr int POLY_LDS = 63 * 1024;
constexpr int POLY_MAX_KT = 16;                                    // the most taps per phase that k_pulsetx_poly keeps in registers
constexpr int MAX_I = 1 << 20, MAX_T = 1 << 24;

// the taps padded to K I words (an even count: the symbols behind them are 8-byte words), and the symbols a tile can reach: TILE_O / I + K + 2
size_t poly_lds_bytes(int I, int K)
{
    const size_t ki = ((size_t)K * I + 1) & ~(size_t)1;
    return sizeof(float) * ki + sizeof(float2) * ((size_t)TILE_O / I + K + 4);
}

__device__ __forceinline__ PulseTxSrc channel_src(const PulseTxCfg &c, int ch, const float2 *symtab, const float2 *hist, const void *in, size_t in_pitch)
{
    PulseTxSrc s;
    s.hist = hist + (size_t)ch * c.H;
    s.in_b = c.first == PULSETX_MOD ? (const uint8_t *)in + (size_t)ch * in_pitch : nullptr;
    s.in_c = c.first == PULSETX_SHAPE ? (const float2 *)in + (size_t)ch * in_pitch : nullptr;
    s.sym = symtab;
    return s;
}

// blockIdx.x = channel * n_tiles + tile.  Dynamic LDS: the padded taps, then the tile's symbols.  step_q, step_j: quotient and remainder of 2 POLY_THREADS / I.
// KT = 0: any shape.  KT = K > 0: I divides 2 POLY_THREADS (step_j = 0), so a lane keeps its two phases over all its steps: its 2 K taps stay in registers,
// the K + 1 symbols of a step are read once for both outputs, and only the last product of an output can be one the phase does not have.
template <int KT>
__global__ __launch_bounds__(POLY_THREADS) void k_pulsetx_poly(PulseTxCfg c, PulseTxCall k, int step_q, int step_j, const float *__restrict__ taps,
                                                               const float2 *__restrict__ symtab, const float2 *__restrict__ hist, const void *__restrict__ in,
                                                               size_t in_pitch, int n_tiles, float2 *__restrict__ out, size_t out_pitch)
{
    extern __shared__ __align__(16) float lds[];
    const int I = c.I, K = c.K, KI = K * I;
    float *l_taps = lds;
    float2 *l_sym = (float2 *)(lds + ((KI + 1) & ~1));
    const int ch = blockIdx.x / n_tiles, tile = blockIdx.x - ch * n_tiles, tid = threadIdx.x;
    float2 *row = out + (size_t)ch * out_pitch;
    const int a = (int)(((uintptr_t)row >> 3) & 1);               // 1: the row starts on an odd complex sample, so sample 2 p - 1 opens the 16-byte pair p
    const long long s_lo = (long long)tile * TILE_O - a;          // the tile's outputs: s_lo .. s_lo + TILE_O - 1
    if (s_lo >= k.n_out) return;
    const int s_first = s_lo < 0 ? 0 : (int)s_lo, s_last = (s_lo + TILE_O < k.n_out ? (int)(s_lo + TILE_O) : k.n_out) - 1;
    // the symbols the tile reads, counted from N0 / I: c_lo .. c_hi (the last one only as the neighbour a pair looks at)
    const int c_lo = (int)(((long long)k.r0 + s_first + I - 1) / I), c_hi = (int)(((long long)k.r0 + s_last + I - 1) / I) + K;
    const int n_sym = c_hi - c_lo + 1;
    const PulseTxSrc src = channel_src(c, ch, symtab, hist, in, in_pitch);
    for (int j = tid; j < n_sym; j += POLY_THREADS) l_sym[j] = pulsetx_symbol(c, k, src, c_lo + j - k.hb);
    for (int j = tid; j < KI; j += POLY_THREADS) l_taps[j] = j < c.T ? taps[j] : 0.f;
    __syncthreads();
    const int thr = c.T - (K - 1) * I;                            // a phase >= thr has K - 1 products, a smaller one K
    // output with r0 + s = q I + j: phase ph = (I - j) mod I, first symbol q + (j > 0)
    auto one = [&](int q, int j) -> float2 {
        const int ph = j ? I - j : 0, kp = K - (ph >= thr);
        const float2 *x = l_sym + (q + (j > 0) - c_lo);
        float ai = 0.f, aq = 0.f;
        for (int kk = 0; kk < kp; kk++) { const float w = l_taps[ph + kk * I]; ai = fmaf(x[kk].x, w, ai); aq = fmaf(x[kk].y, w, aq); }
        return make_float2(ai, aq);
    };
    long long s = s_lo + 2 * tid;
    const long long u = (long long)k.r0 + s;                      // >= -1
    int q, j;
    if (u < 0) { q = -1; j = I - 1; } else { q = (int)(u / I); j = (int)(u - (long long)q * I); }
    if constexpr (KT > 0) {
        int q1 = q, j1 = j + 1;
        if (j1 == I) { j1 = 0; q1++; }
        const int ph0 = j ? I - j : 0, ph1 = j1 ? I - j1 : 0;
        const bool full0 = ph0 < thr, full1 = ph1 < thr;            // the phase has all K products
        const bool next_symbol = q1 + (j1 > 0) != q + (j > 0);      // the second output starts one symbol further (its phase wrapped)
        float w0[KT], w1[KT];
#pragma unroll
        for (int kk = 0; kk < KT; kk++) { w0[kk] = l_taps[ph0 + kk * I]; w1[kk] = l_taps[ph1 + kk * I]; }
        int c0 = q + (j > 0) - c_lo;
#pragma unroll 2
        for (int it = 0; it < POLY_STEPS; it++) {
            const bool v0 = s >= 0 && s < k.n_out, v1 = s + 1 < k.n_out;
            if (v0 && v1) {
                float2 x[KT + 1];
#pragma unroll
                for (int kk = 0; kk <= KT; kk++) x[kk] = l_sym[c0 + kk];
                float ai0 = 0.f, aq0 = 0.f, ai1 = 0.f, aq1 = 0.f;
#pragma unroll
                for (int kk = 0; kk < KT - 1; kk++) {
                    const float2 x1 = next_symbol ? x[kk + 1] : x[kk];
                    ai0 = fmaf(x[kk].x, w0[kk], ai0); aq0 = fmaf(x[kk].y, w0[kk], aq0);
                    ai1 = fmaf(x1.x, w1[kk], ai1); aq1 = fmaf(x1.y, w1[kk], aq1);
                }
                {
                    const float2 x0 = x[KT - 1], x1 = next_symbol ? x[KT] : x[KT - 1];
                    const float bi0 = fmaf(x0.x, w0[KT - 1], ai0), bq0 = fmaf(x0.y, w0[KT - 1], aq0);
                    const float bi1 = fmaf(x1.x, w1[KT - 1], ai1), bq1 = fmaf(x1.y, w1[KT - 1], aq1);
                    ai0 = full0 ? bi0 : ai0; aq0 = full0 ? bq0 : aq0; ai1 = full1 ? bi1 : ai1; aq1 = full1 ? bq1 : aq1;
                }
                *(float4 *)(row + s) = make_float4(ai0, aq0, ai1, aq1);
            } else if (v0) {
                row[s] = one(q, j);
            } else if (v1) {
                row[s + 1] = one(q1, j1);
            }
            s += 2 * POLY_THREADS;
            q += step_q; q1 += step_q; c0 += step_q;
        }
    } else {
#pragma unroll 2
        for (int it = 0; it < POLY_STEPS; it++) {
            int q1 = q, j1 = j + 1;
            if (j1 == I) { j1 = 0; q1++; }
            const bool v0 = s >= 0 && s < k.n_out, v1 = s + 1 < k.n_out;
            if (v0 && v1) {
                const int ph0 = j ? I - j : 0, ph1 = j1 ? I - j1 : 0, kp0 = K - (ph0 >= thr), kp1 = K - (ph1 >= thr);
                const int c0 = q + (j > 0) - c_lo;
                const bool next_symbol = q1 + (j1 > 0) != q + (j > 0);   // the second output starts one symbol further (its phase wrapped)
                const float2 *x = l_sym + c0;
                float2 prev = x[0];
                float ai0 = 0.f, aq0 = 0.f, ai1 = 0.f, aq1 = 0.f;
                for (int kk = 0; kk < K; kk++) {
                    const float2 next = x[kk + 1];
                    const float2 x1 = next_symbol ? next : prev;
                    const float w0 = l_taps[ph0 + kk * I], w1 = l_taps[ph1 + kk * I];
                    if (kk < kp0) { ai0 = fmaf(prev.x, w0, ai0); aq0 = fmaf(prev.y, w0, aq0); }
                    if (kk < kp1) { ai1 = fmaf(x1.x, w1, ai1); aq1 = fmaf(x1.y, w1, aq1); }
                    prev = next;
                }
                *(float4 *)(row + s) = make_float4(ai0, aq0, ai1, aq1);
            } else if (v0) {
                row[s] = one(q, j);
            } else if (v1) {
                row[s + 1] = one(q1, j1);
            }
            s += 2 * POLY_THREADS;
            q += step_q; j += step_j;
            if (j >= I) { j -= I; q++; }
        }
    }
}

__global__ __launch_bounds__(256) void k_pulsetx_generic(PulseTxCfg c, PulseTxCall k, const float *__restrict__ taps, const float2 *__restrict__ symtab,
                                                         const float2 *__restrict__ hist, const void *__restrict__ in, size_t in_pitch, int n_ch,
                                                         float2 *__restrict__ out, size_t out_pitch)
{
    const long long total = (long long)n_ch * k.n_out;
    for (long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x; l < total; l += (long long)gridDim.x * blockDim.x) {
        const int ch = (int)(l / k.n_out), o = (int)(l - (long long)ch * k.n_out);
        float2 *y = out + (size_t)ch * out_pitch + o;
        if (c.last == PULSETX_MOD) { *y = symtab[((const uint8_t *)in)[(size_t)ch * in_pitch + o]]; continue; }
        *y = pulsetx_output(c, k, channel_src(c, ch, symtab, hist, in, in_pitch), taps, o);
    }
}

__global__ __launch_bounds__(256) void k_pulsetx_hist(PulseTxCfg c, PulseTxCall k, const float2 *__restrict__ symtab, const float2 *__restrict__ hist,
                                                      const void *__restrict__ in, size_t in_pitch, int n_ch, float2 *__restrict__ hist_next)
{
    const long long total = (long long)n_ch * c.H;
    for (long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x; l < total; l += (long long)gridDim.x * blockDim.x) {
        const int ch = (int)(l / c.H), h = (int)(l - (long long)ch * c.H);
        hist_next[l] = pulsetx_next_hist(c, k, channel_src(c, ch, symtab, hist, in, in_pitch), h);
    }
}

__global__ void k_generic_slicer(const float *__restrict__ in, uint8_t *__restrict__ out, long long n, size_t in_pitch, size_t out_pitch, int n_symbols, float d)
{
    const float *x = in + (size_t)blockIdx.y * in_pitch;
    uint8_t *y = out + (size_t)blockIdx.y * out_pitch;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) y[i] = generic_slicer_step(x[i], n_symbols, d);
}

__global__ void k_plain_interpolate(const float2 *__restrict__ in, float2 *__restrict__ out, long long n_out, size_t in_pitch, size_t out_pitch, int I)
{
    const float2 *x = in + (size_t)blockIdx.y * in_pitch;
    float2 *y = out + (size_t)blockIdx.y * out_pitch;
    for (long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x; l < n_out; l += (long long)gridDim.x * blockDim.x) {
        const long long m = l / I;
        y[l] = l == m * I ? x[m] : make_float2(0.f, 0.f);
    }
}

__global__ void k_pack_bits_1to8(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, long long n_out, size_t in_pitch, size_t out_pitch)
{
    const uint8_t *x = in + (size_t)blockIdx.y * in_pitch;
    uint8_t *y = out + (size_t)blockIdx.y * out_pitch;
    for (long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x; l < n_out; l += (long long)gridDim.x * blockDim.x) y[l] = (x[l >> 3] >> (l & 7)) & 1;
}

__global__ void k_pack_bits_8to1(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, long long n_out, size_t in_pitch, size_t out_pitch)
{
    const uint8_t *x = in + (size_t)blockIdx.y * in_pitch;
    uint8_t *y = out + (size_t)blockIdx.y * out_pitch;
    for (long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x; l < n_out; l += (long long)gridDim.x * blockDim.x) y[l] = pack_bits_8to1_step(x + 8 * l);
}

// ---- the receive object (modem_dev.hpp: the stream)
//   k_pulserx_tiled<G>  a one-wave workgroup holds C <= 64 / G channels, G = 16, 8 or 4 lanes each (C = 1 or 2: G = 16).  All 64 lanes stage a tile of RX_TILE = 128 samples of every
//                       channel into its LDS ring with one 16-byte load per lane and channel (a row that starts on an odd complex sample is read one sample
//                       earlier), the next tile's loads in flight while this one is worked on.  For every symbol whose three positions (+ T - 1) are in the ring
//                       the channel's lanes run the defined order: lane g the partial sums r = g (mod G), the mid and right point together so that a tap is read
//                       once for both, folded across lanes by data-parallel moves (lower index as the left operand); every lane of the group then holds the three
//                       samples and steps the timing loop, the group's first lane writes.  Under GARDNER without a correction the left point is the last
//                       symbol's right point and is not computed again.  Bytes go to an LDS staging row per channel and out in runs of 64 or more.
//   k_pulserx_generic   one lane per channel, modem_dev.hpp's pulserx_walk straight from global memory.
constexpr int RX_TILE = 128, RX_LDS = 63 * 1024, RX_OBUF = 512, RX_MAX_RING = 8192;

// the ring: the unconsumed span (at most 3 D/2 + T - 1 samples) and a tile, rounded up to a power of two (a slot is a masked position); 0: not for the tiled kernel
int rx_ring(const PulseRxCfg &c)
{
    const long long need = 3LL * c.t.hb + c.Tm1 + RX_TILE;
    if (need > RX_MAX_RING) return 0;
    int r = 256;
    while (r < need) r <<= 1;
    return r;
}
size_t rx_lds(const PulseRxCfg &c, int C, int R)
{
    return sizeof(float2) * (size_t)C * R + sizeof(float) * (((size_t)c.T + 1) & ~(size_t)1) + (c.last == PULSERX_SLICE ? (size_t)C * RX_OBUF : 0);
}

// the value lane (lane ^ S) of the same row of 16 lanes holds, S = 1, 2, 4 or 8, as a data-parallel move between VALU lanes (no trip through the LDS
// crossbar, whose latency would stand four times in every symbol's critical path): the quad permutations [1,0,3,2] and [2,3,0,1], a row rotation by 8, and
// for 4 a shift either way, of which a lane takes the one that comes from its partner.  gl: the lane's index in its group (bit 2 is the lane's own).
template <int S> __device__ __forceinline__ float rx_lane_xor(float v, int gl)
{
    const int x = __float_as_int(v);
    int r;
    if constexpr (S == 1) r = __builtin_amdgcn_update_dpp(x, x, 0xB1, 0xF, 0xF, false);
    else if constexpr (S == 2) r = __builtin_amdgcn_update_dpp(x, x, 0x4E, 0xF, 0xF, false);
    else if constexpr (S == 8) r = __builtin_amdgcn_update_dpp(x, x, 0x128, 0xF, 0xF, false);          // row_ror:8
    else {
        const int up = __builtin_amdgcn_update_dpp(x, x, 0x104, 0xF, 0xF, false);                       // row_shl:4: from lane + 4
        const int dn = __builtin_amdgcn_update_dpp(x, x, 0x114, 0xF, 0xF, false);                       // row_shr:4: from lane - 4
        r = (gl & 4) ? dn : up;
    }
    return __int_as_float(r);
}
// one step of the fold across lanes: with lane g ^ S, the lower lane's sum on the left
template <int S> __device__ __forceinline__ float rx_fold_step(float v, int gl)
{
    const float o = rx_lane_xor<S>(v, gl);
    return (gl & S) ? o + v : v + o;
}

// NPOS filtered samples at the ring slots slot[] by a group of G lanes; every lane of the group returns the sums
template <int G, int NPOS>
__device__ __forceinline__ void rx_group_dot(const float2 *ring, int mask, const float *l_taps, int T, int gl, const int *slot, float2 *res)
{
    constexpr int NP = 16 / G;
    float ai[NPOS][NP], aq[NPOS][NP];
#pragma unroll
    for (int q = 0; q < NPOS; q++)
#pragma unroll
        for (int j = 0; j < NP; j++) ai[q][j] = aq[q][j] = 0.f;
    int t0 = 0;
#pragma unroll 4
    for (; t0 + 16 <= T; t0 += 16) {                      // (unrolled: the LDS reads of four rounds are in flight together)
#pragma unroll
        for (int j = 0; j < NP; j++) {
            const int t = t0 + gl + G * j;
            const float w = l_taps[t];
#pragma unroll
            for (int q = 0; q < NPOS; q++) {
                const float2 v = ring[(slot[q] + t) & mask];
                ai[q][j] = fmaf(v.x, w, ai[q][j]); aq[q][j] = fmaf(v.y, w, aq[q][j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NP; j++) {
        const int t = t0 + gl + G * j;
        if (t < T) {
            const float w = l_taps[t];
#pragma unroll
            for (int q = 0; q < NPOS; q++) {
                const float2 v = ring[(slot[q] + t) & mask];
                ai[q][j] = fmaf(v.x, w, ai[q][j]); aq[q][j] = fmaf(v.y, w, aq[q][j]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NPOS; q++) {
#pragma unroll
        for (int sj = NP / 2; sj >= 1; sj >>= 1)          // s = G sj >= G: both sums are this lane's
#pragma unroll
            for (int j = 0; j < sj; j++) { ai[q][j] = ai[q][j] + ai[q][j + sj]; aq[q][j] = aq[q][j] + aq[q][j + sj]; }
        float vi = ai[q][0], vq = aq[q][0];               // s < G: across lanes
        if constexpr (G >= 16) { vi = rx_fold_step<8>(vi, gl); vq = rx_fold_step<8>(vq, gl); }
        if constexpr (G >= 8) { vi = rx_fold_step<4>(vi, gl); vq = rx_fold_step<4>(vq, gl); }
        vi = rx_fold_step<2>(vi, gl); vq = rx_fold_step<2>(vq, gl);
        vi = rx_fold_step<1>(vi, gl); vq = rx_fold_step<1>(vq, gl);
        res[q] = make_float2(vi, vq);
    }
}

template <int G>
__global__ __launch_bounds__(64) void k_pulserx_tiled(PulseRxCfg c, PulseRxChan *__restrict__ st, float2 *__restrict__ tails, int tail_cap, int n_ch, int C, int R,
                                                      const float *__restrict__ taps, const float2 *__restrict__ in, long long n_in, size_t in_pitch,
                                                      void *__restrict__ out, size_t out_pitch, int *__restrict__ counts, float *__restrict__ err,
                                                      unsigned *__restrict__ idx)
{
    constexpr int CMAX = 64 / G;
    extern __shared__ __align__(16) float lds[];
    __shared__ int s_t0[CMAX], s_k[CMAX];
    float2 *ring = (float2 *)lds;
    float *l_taps = lds + 2 * (size_t)C * R;
    uint8_t *l_out = (uint8_t *)(l_taps + ((c.T + 1) & ~1));
    const int mask = R - 1, lane = threadIdx.x, ch0 = blockIdx.x * C, nc = min(C, n_ch - ch0);
    const bool filt = c.first == PULSERX_FILTER;
    if (lane < CMAX) { s_t0[lane] = lane < nc ? st[ch0 + lane].tail_len : 0; s_k[lane] = 0; }
    if (filt) for (int j = lane; j < c.T; j += 64) l_taps[j] = taps[j];
    __syncthreads();
    for (int cc = 0; cc < nc; cc++) {                    // the tails: stream positions 0 .. tail_len - 1
        const float2 *tl = tails + (size_t)(ch0 + cc) * tail_cap;
        for (int p = lane; p < s_t0[cc]; p += 64) ring[(size_t)cc * R + p] = tl[p];
    }

    const int grp = lane / G, gl = lane % G;
    const bool active = grp < nc;
    const int ch = ch0 + grp;
    PulseRxChan s{0, 0, 0};
    float2 *oc = nullptr; float *oe = nullptr; unsigned *oi = nullptr;
    int my_a = 0;
    if (active) {
        s = st[ch];
        const size_t oo = (size_t)ch * out_pitch;
        if (c.last == PULSERX_TIMING) { oc = (float2 *)out + oo; oe = err ? err + oo : nullptr; oi = idx ? idx + oo : nullptr; }
        my_a = (int)(((uintptr_t)(in + (size_t)ch * in_pitch) >> 3) & 1);
    }
    const float2 *rme = ring + (size_t)(active ? grp : 0) * R;
    uint8_t *ome = l_out + (size_t)(active ? grp : 0) * RX_OBUF;
    const int nV = s.tail_len + (int)n_in;              // (n_in <= 2^30 and the tail is short: positions stay in an int)
    int cbi = 0, held_at = -1;
    float2 held = make_float2(0.f, 0.f);
    int corr = s.corr, k = 0;

    // lane j holds the input samples jb + 2 j - a and the next one of every channel (a = 1: the row starts on an odd complex sample), loaded one tile ahead
    float4 nx[CMAX];
    auto fetch = [&](long long jb) {
#pragma unroll
        for (int cc = 0; cc < CMAX; cc++) {
            if (cc < nc) {
                const float2 *row = in + (size_t)(ch0 + cc) * in_pitch;
                const long long i0 = jb + 2 * lane - (long long)(((uintptr_t)row >> 3) & 1);
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (i0 >= 0 && i0 + 1 < n_in) v = *(const float4 *)(row + i0);
                else {
                    if (i0 >= 0 && i0 < n_in) { const float2 u = row[i0]; v.x = u.x; v.y = u.y; }
                    if (i0 + 1 >= 0 && i0 + 1 < n_in) { const float2 u = row[i0 + 1]; v.z = u.x; v.w = u.y; }
                }
                nx[cc] = v;
            }
        }
    };
    int fl[CMAX];                                        // bytes of each channel already stored
#pragma unroll
    for (int cc = 0; cc < CMAX; cc++) fl[cc] = 0;
    auto flush = [&](bool all) {
#pragma unroll
        for (int cc = 0; cc < CMAX; cc++) {
            if (cc < nc) {
                const int kk = s_k[cc];
                if (kk - fl[cc] >= 64 || all) {
                    uint8_t *row = (uint8_t *)out + (size_t)(ch0 + cc) * out_pitch;
#pragma unroll 1
                    for (int j = fl[cc] + lane; j < kk; j += 64) row[j] = l_out[cc * RX_OBUF + (j & (RX_OBUF - 1))];
                    fl[cc] = kk;
                }
            }
        }
    };

    fetch(0);
    for (long long jb = 0; jb < n_in + 1; jb += RX_TILE) {
#pragma unroll
        for (int cc = 0; cc < CMAX; cc++) {              // stage: input sample i is stream position tail_len + i
            if (cc < nc) {
                const float2 *row = in + (size_t)(ch0 + cc) * in_pitch;
                const long long i0 = jb + 2 * lane - (long long)(((uintptr_t)row >> 3) & 1);
                const int p0 = s_t0[cc] + (int)i0;
                float2 *rg = ring + (size_t)cc * R;
                if (i0 >= 0 && i0 < n_in) rg[p0 & mask] = make_float2(nx[cc].x, nx[cc].y);
                if (i0 + 1 >= 0 && i0 + 1 < n_in) rg[(p0 + 1) & mask] = make_float2(nx[cc].z, nx[cc].w);
            }
        }
        __syncthreads();
        if (jb + RX_TILE < n_in + 1) fetch(jb + RX_TILE);
        if (active) {
            const int end = s.tail_len + (int)min(n_in, jb + RX_TILE - my_a);
            while (cbi + c.t.hb * 3 + c.Tm1 < end) {
                int pl, pm, pr;
                psk31_positions(c.t, cbi, &corr, &pl, &pm, &pr);
                float2 xl, xm, xr;
                if (filt) {
                    if (pl == held_at) xl = held;
                    else { const int sl = pl & mask; rx_group_dot<G, 1>(rme, mask, l_taps, c.T, gl, &sl, &xl); }
                    const int s2[2] = {pm & mask, pr & mask};
                    float2 r2[2];
                    rx_group_dot<G, 2>(rme, mask, l_taps, c.T, gl, s2, r2);
                    xm = r2[0]; xr = r2[1];
                } else { xl = rme[pl & mask]; xm = rme[pm & mask]; xr = rme[pr & mask]; }
                held = xr; held_at = pr;
                const float error = psk31_timing_error(c.t, xl, xm, xr);
                const float2 xo = c.t.algorithm == 1 ? xm : xl;
                if (c.last == PULSERX_TIMING) {
                    if (gl == 0) {
                        oc[k] = xo;
                        if (oe) oe[k] = error;
                        if (oi) oi[k] = s.base + (uint32_t)(c.t.algorithm == 1 ? pm : pl);
                    }
                    k++;
                } else {
                    if (gl == 0) {
                        ome[k & (RX_OBUF - 1)] = generic_slicer_step(c.gain * xo.x, c.n_symbols, c.d);
                        if (c.slice_q) ome[(k + 1) & (RX_OBUF - 1)] = generic_slicer_step(c.gain * xo.y, c.n_symbols, c.d);
                    }
                    k += 1 + c.slice_q;
                }
                corr = psk31_correction(c.t, error);
                cbi += c.t.D + corr;
            }
            if (gl == 0) s_k[grp] = k;
        }
        __syncthreads();
        if (c.last == PULSERX_SLICE) flush(false);       // (a tile adds at most 2 (RX_TILE + 1) bytes, at D = 2, to the < 64 waiting: within RX_OBUF)
    }
    if (c.last == PULSERX_SLICE) flush(true);
    if (!active) return;
    // the unconsumed tail V[cbi ..) (at most 3 D/2 + T - 1 samples, all still in the ring) goes back raw
    const int nt = nV - cbi;
    float2 *tl = tails + (size_t)ch * tail_cap;
    for (int j = gl; j < nt; j += G) tl[j] = rme[(cbi + j) & mask];
    if (gl == 0) {
        s.tail_len = nt; s.corr = corr; s.base += (uint32_t)cbi;
        st[ch] = s;
        counts[ch] = k;
    }
}

__global__ __launch_bounds__(64) void k_pulserx_generic(PulseRxCfg c, PulseRxChan *__restrict__ st, float2 *__restrict__ tails, int tail_cap, int n_ch, int lanes,
                                                        const float *__restrict__ taps, const float2 *__restrict__ in, long long n_in, size_t in_pitch,
                                                        void *__restrict__ out, size_t out_pitch, int *__restrict__ counts, float *__restrict__ err,
                                                        unsigned *__restrict__ idx)
{
    if ((int)threadIdx.x >= lanes) return;
    const int ch = blockIdx.x * lanes + threadIdx.x;
    if (ch >= n_ch) return;
    const size_t oo = (size_t)ch * out_pitch;
    PulseRxOut o{nullptr, nullptr, err ? err + oo : nullptr, idx ? idx + oo : nullptr};
    if (c.last == PULSERX_TIMING) o.c = (float2 *)out + oo; else o.b = (uint8_t *)out + oo;
    PulseRxChan s = st[ch];
    counts[ch] = pulserx_walk(c, s, tails + (size_t)ch * tail_cap, in + (size_t)ch * in_pitch, n_in, taps, o);
    st[ch] = s;
}

static_assert(sizeof(PulseRxChan) == sizeof(csdr_amd_pulserx_chan), "PulseRxChan mirrors csdr_amd_pulserx_chan");

int make_rx_cfg(const csdr_amd_pulserx_params *p, int first, int last, PulseRxCfg *c)
{
    if (!p) return fail_msg(-3, "pulserx: null params");
    if (first < PULSERX_FILTER || first > PULSERX_TIMING || last < PULSERX_TIMING || last > PULSERX_SLICE)
        return fail_msg(-3, "pulserx: first_stage is 0 (FILTER) or 1 (TIMING), last_stage 1 (TIMING) or 2 (SLICE)");
    if (first == PULSERX_FILTER && (!p->taps || p->taps_length <= 0 || p->taps_length > MAX_T)) return fail_msg(-3, "pulserx: taps_length should be >0 (and <= 16777216)");
    if (p->algorithm != 0 && p->algorithm != 1) return fail_msg(-3, "pulserx: algorithm is 0 (GARDNER) or 1 (EARLYLATE)");
    // (the library function takes any decimation; only the reference's command line asks for a multiple of 4 above 4.  From 2 on every symbol moves on.)
    if (p->decimation < 2 || p->decimation > (1 << 20)) return fail_msg(-3, "pulserx: decimation factor should be 2 .. 1048576");
    if (!(p->max_error >= 0) || !(fabsf(p->loop_gain) * p->max_error <= 1.f))
        return fail_msg(-3, "pulserx: need max_error >= 0 and |loop_gain| * max_error <= 1 (a symbol then moves on by D/2 .. 3D/2 samples)");
    if (last == PULSERX_SLICE && (p->n_symbols < 2 || p->n_symbols > 256)) return fail_msg(-3, "pulserx: n_symbols should be between 2 and 256");
    memset(c, 0, sizeof *c);
    Psk31Cfg &t = c->t;
    t.algorithm = p->algorithm; t.D = p->decimation; t.hb = p->decimation / 2; t.qb = p->decimation / 4;
    t.wing = (int)(p->decimation * 0.25f); t.use_q = p->use_q != 0;
    t.loop_gain = p->loop_gain; t.max_error = p->max_error;
    t.hb_sign = (float)(t.hb * (p->algorithm == 0 ? -1 : 1));
    t.reset_lo = -t.qb * 0.9; t.reset_hi = 0.9 * t.qb;
    c->first = first; c->last = last;
    c->T = first == PULSERX_FILTER ? p->taps_length : 1; c->Tm1 = c->T - 1;
    c->gain = p->gain; c->n_symbols = last == PULSERX_SLICE ? p->n_symbols : 2; c->slice_q = last == PULSERX_SLICE && p->slice_q != 0;
    c->d = (float)(2.0 / (c->n_symbols - 1));
    return 0;
}

// channels per wave of k_pulserx_tiled for a request: 16, 8, 4, 2 or 1 (the largest of them within it), then the next smaller one while the rings do not fit
int rx_tiled_channels(const PulseRxCfg &c, int R, int want, int *G)
{
    int C = want >= 16 ? 16 : want >= 8 ? 8 : want >= 4 ? 4 : want >= 2 ? 2 : 1;
    while (C > 0 && rx_lds(c, C, R) > (size_t)RX_LDS) C /= 2;
    *G = C > 4 ? 64 / C : 16;                             // fewer than four channels: groups of 16 lanes, the other lanes stage only
    return C;
}

// channels per wave when the caller leaves it open.  k_pulserx_tiled: a symbol's chain (positions, LDS reads, sixteen partial sums, the fold, the loop's
// arithmetic) is serial, so the kernel runs at the chain's latency until the waves of a SIMD fill its issue slots: the fewest channels per wave that keep
// the batch within two waves per SIMD (4096 channels on 256 CUs: 2; profiles/pulserx_bench.json has every choice).  k_pulserx_generic: one wave per CU, as k_psk31.
int default_rx_lanes(int cus, int n_ch, bool tiled)
{
    if (tiled) { int C = 1; while (C < 16 && (long long)n_ch > (long long)cus * 4 * 2 * C) C *= 2; return C; }
    return std::max(1, std::min(64, (int)cdiv(n_ch, (size_t)cus)));
}

unsigned flat_blocks(long long n) { return (unsigned)std::min<long long>((n + 255) / 256, 4096); }

int check_cfg(int n_psk, int interpolation, int taps_length, int first, int last)
{
    if (first < PULSETX_MOD || last > PULSETX_SHAPE || first > last) return fail_msg(-3, "pulsetx: need 0 <= first_stage <= last_stage <= 1");
    if (n_psk <= 0 || n_psk > 256) return fail_msg(-3, "pulsetx: n_psk should be between 1 and 256");
    if (interpolation <= 0 || interpolation > MAX_I) return fail_msg(-3, "pulsetx: interpolation should be >0 (and <= 1048576)");
    if (taps_length <= 0 || taps_length > MAX_T) return fail_msg(-3, "pulsetx: taps_length should be >0 (and <= 16777216)");
    return 0;
}

PulseTxCfg make_cfg(int interpolation, int taps_length, int first, int last)
{
    PulseTxCfg c;
    c.first = first; c.last = last; c.I = interpolation; c.T = taps_length;
    c.K = (taps_length + interpolation - 1) / interpolation;
    c.H = (taps_length - 1 + interpolation - 1) / interpolation;
    return c;
}

// the geometry of a call of n symbols behind n0
PulseTxCall make_call(const PulseTxCfg &c, long long n0, long long n)
{
    const long long N0 = std::max(0LL, n0 * c.I - c.T + 1), N1 = std::max(0LL, (n0 + n) * c.I - c.T + 1);
    PulseTxCall k;
    k.r0 = (int)(N0 % c.I); k.hb = (int)(n0 - N0 / c.I); k.n = (int)n;
    k.n_out = c.last == PULSETX_MOD ? (int)n : (int)(N1 - N0);
    return k;
}

} // namespace

// firdes_rrc_f with the reference's arithmetic: float expressions where its operands are float (PI is a float), double where libm's sin / cos / sqrt enter,
// every tap rounded to float when stored; then normalize_fir_f.  Only indexes < taps_length are written (an even length leaves out the reference's
// taps[taps_length]).
void csdr_amd::firdes_rrc_below(float *taps, int taps_length, int samples_per_symbol, float beta)
{
    const int middle_i = taps_length / 2;
    const float sps = (float)samples_per_symbol;
    taps[middle_i] = (1 / sps) * (1 + beta * (4 / PI_F - 1));
    for (int i = 1; i < 1 + taps_length / 2; i++) {
        float v;
        if ((float)i == sps / (4 * beta))
            v = (float)(((double)beta / (samples_per_symbol * sqrt(2.0))) *
                        ((double)(1 + (2 / PI_F)) * sin((double)(PI_F / (4 * beta))) + (double)(1 - (2 / PI_F)) * cos((double)(PI_F / (4 * beta)))));
        else {
            const float r = (float)i / sps;
            const double num = sin((double)(PI_F * r * (1 - beta))) + (double)(4 * beta * r) * cos((double)(PI_F * r * (1 + beta)));
            const float den = PI_F * r * (1 - powf(4 * beta * r, 2));
            v = (float)((double)(1 / sps) * num / (double)den);
        }
        if (middle_i + i < taps_length) taps[middle_i + i] = v;
        taps[middle_i - i] = v;
    }
    float sum = 0;
    for (int i = 0; i < taps_length; i++) sum += taps[i];
    for (int i = 0; i < taps_length; i++) taps[i] = taps[i] / sum;
}

struct csdr_amd_pulsetx : Bank {
    PulseTxCfg cfg; bool fits;
    long long total = 0;                                          // symbols every channel has taken since the last reset
    int cur = 0;                                                  // the half of d_hist that holds the history
    DevBuf<float2> d_sym, d_hist; DevBuf<float> d_taps;           // d_hist: 2 x n_ch x H
    size_t hist_half() const { return (size_t)n_ch * cfg.H; }
};

struct csdr_amd_pulserx : ChanBank<PulseRxChan> {
    PulseRxCfg cfg; int tail_cap, cus, ring;                      // ring: samples per channel in k_pulserx_tiled's LDS, 0: the shape runs on k_pulserx_generic
    DevBuf<float2> d_tail; DevBuf<float> d_taps;
};

extern "C" {

csdr_amd_pulsetx *csdr_amd_pulsetx_create(csdr_amd_ctx *c, int n_channels, int n_psk, int interpolation, const float *host_taps, int taps_length, int first_stage,
                                          int last_stage)
{
    if (bank_create_check("pulsetx", c, n_channels) < 0) return nullptr;
    if (first_stage == PULSETX_MOD && last_stage == PULSETX_MOD) { if (taps_length < 1) taps_length = 1; if (interpolation < 1) interpolation = 1; host_taps = nullptr; }
    else if (!host_taps) { fail_msg(-3, "pulsetx: taps are required up to the stage SHAPE"); return nullptr; }
    if (check_cfg(n_psk, interpolation, taps_length, first_stage, last_stage) < 0) return nullptr;
    Owned<csdr_amd_pulsetx, csdr_amd_pulsetx_destroy> p(new csdr_amd_pulsetx());
    p->c = c; p->cfg = make_cfg(interpolation, taps_length, first_stage, last_stage); p->n_ch = n_channels;
    p->fits = last_stage == PULSETX_SHAPE && poly_lds_bytes(p->cfg.I, p->cfg.K) <= (size_t)POLY_LDS;
    csdr_complexf sym[256];
    if (csdr_amd_psk31tx_tables(n_psk, 1, sym, nullptr) < 0) return nullptr;
    if (dev_alloc(p->d_sym, sizeof sym) != hipSuccess || dev_alloc(p->d_taps, sizeof(float) * taps_length) != hipSuccess ||
        dev_alloc(p->d_hist, sizeof(float2) * 2 * std::max<size_t>(p->hist_half(), 1)) != hipSuccess) { fail_msg(-2, "pulsetx: out of device memory"); return nullptr; }
    const float one = 1.f;
    if (csdr_amd_h2d(c, p->d_sym.get(), sym, sizeof sym) < 0 ||
        (host_taps ? csdr_amd_h2d(c, p->d_taps.get(), host_taps, sizeof(float) * taps_length) : csdr_amd_h2d(c, p->d_taps.get(), &one, sizeof one)) < 0 ||
        csdr_amd_pulsetx_reset(p.get()) < 0) return nullptr;
    return p.release();
}

int csdr_amd_pulsetx_reset(csdr_amd_pulsetx *p)
{
    if (!p) return fail_msg(-3, "pulsetx: null object");
    p->total = 0; p->cur = 0;
    return csdr_amd_memset(p->c, p->d_hist.get(), 0, sizeof(float2) * 2 * std::max<size_t>(p->hist_half(), 1));
}

long long csdr_amd_pulsetx_max_out(const csdr_amd_pulsetx *p, long long n_in)
{
    if (!p || n_in < 0) return 0;
    return p->cfg.last == PULSETX_SHAPE ? n_in * p->cfg.I : n_in;
}

int csdr_amd_pulsetx_tile(const csdr_amd_pulsetx *p) { return p ? std::max(1, TILE_O / p->cfg.I) : 0; }

int csdr_amd_pulsetx_process(csdr_amd_pulsetx *p, const void *in, long long n_in, size_t in_pitch, void *out, size_t out_pitch, long long *n_out)
{
    if (!p) return fail_msg(-3, "pulsetx: null object");
    if (n_in < 0 || n_in > (1LL << 30) || (n_in > 0 && (!in || in_pitch < (size_t)n_in))) return fail_msg(-3, "pulsetx: need in_pitch >= n_in >= 0 (n_in <= 2^30)");
    if (!n_out) return fail_msg(-3, "pulsetx: n_out is required");
    const long long mo = csdr_amd_pulsetx_max_out(p, n_in);
    if (mo > INT_MAX) return fail_msg(-3, "pulsetx: max_out %lld of this call is above 2^31 - 1", mo);
    if (mo > 0 && (!out || out_pitch < (size_t)mo)) return fail_msg(-3, "pulsetx: out_pitch %zu below max_out %lld", out_pitch, mo);
    *n_out = 0;
    if (!n_in) return 0;
    csdr_amd_ctx *c = p->c;
    const PulseTxCfg &g = p->cfg;
    const PulseTxCall k = make_call(g, p->total, n_in);
    const float2 *hist = p->d_hist.get() + (size_t)p->cur * p->hist_half();
    float2 *hist_next = p->d_hist.get() + (size_t)(p->cur ^ 1) * p->hist_half();
    const long long n_tiles = ((long long)k.n_out + 1 + TILE_O - 1) / TILE_O;   // (+ 1: a row that starts on an odd sample is one sample further in its pairs)
    if (k.n_out > 0) {
        if (p->fits && !p->force_generic && n_tiles * p->n_ch <= INT_MAX) {
            const int step_q = (2 * POLY_THREADS) / g.I, step_j = (2 * POLY_THREADS) % g.I;
#define PULSETX_POLY(KTV) hipLaunchKernelGGL(k_pulsetx_poly<KTV>, dim3((unsigned)(n_tiles * p->n_ch)), dim3(POLY_THREADS), poly_lds_bytes(g.I, g.K), c->stream, g, k, \
                                             step_q, step_j, p->d_taps.get(), p->d_sym.get(), hist, in, in_pitch, (int)n_tiles, (float2 *)out, out_pitch)
            switch (step_j == 0 && g.K <= POLY_MAX_KT ? g.K : 0) {
                case 1: PULSETX_POLY(1); break;   case 2: PULSETX_POLY(2); break;   case 3: PULSETX_POLY(3); break;   case 4: PULSETX_POLY(4); break;
                case 5: PULSETX_POLY(5); break;   case 6: PULSETX_POLY(6); break;   case 7: PULSETX_POLY(7); break;   case 8: PULSETX_POLY(8); break;
                case 9: PULSETX_POLY(9); break;   case 10: PULSETX_POLY(10); break; case 11: PULSETX_POLY(11); break; case 12: PULSETX_POLY(12); break;
                case 13: PULSETX_POLY(13); break; case 14: PULSETX_POLY(14); break; case 15: PULSETX_POLY(15); break; case 16: PULSETX_POLY(16); break;
                default: PULSETX_POLY(0); break;
            }
#undef PULSETX_POLY
            p->last_kernel = "k_pulsetx_poly";
        } else {
            const unsigned blocks = (unsigned)std::min<long long>(((long long)p->n_ch * k.n_out + 255) / 256, 1 << 20);
            hipLaunchKernelGGL(k_pulsetx_generic, dim3(blocks), dim3(256), 0, c->stream, g, k, p->d_taps.get(), p->d_sym.get(), hist, in, in_pitch, p->n_ch,
                               (float2 *)out, out_pitch);
            p->last_kernel = "k_pulsetx_generic";
        }
        CSDR_LAUNCH_CHECK();
    }
    if (g.last == PULSETX_SHAPE && g.H > 0) {
        const unsigned blocks = (unsigned)std::min<long long>(((long long)p->hist_half() + 255) / 256, 1 << 20);
        hipLaunchKernelGGL(k_pulsetx_hist, dim3(blocks), dim3(256), 0, c->stream, g, k, p->d_sym.get(), hist, in, in_pitch, p->n_ch, hist_next);
        CSDR_LAUNCH_CHECK();
        p->cur ^= 1;
    }
    p->total += n_in;
    *n_out = k.n_out;
    return 0;
}

int csdr_amd_pulsetx_force_generic(csdr_amd_pulsetx *p, int on) { return bank_force_generic(p, "pulsetx", on); }
const char *csdr_amd_pulsetx_kernel_name(const csdr_amd_pulsetx *p) { return bank_kernel_name(p); }

void csdr_amd_pulsetx_destroy(csdr_amd_pulsetx *p) { destroy_on_stream(p); }

// CPU run of the object's definition (modem_dev.hpp) for one channel, the n items cut into calls of cuts[0], cuts[1], ... items (the rest in one more call).
// Outputs of all calls are concatenated.  Returns the output count.
long long csdr_amd_debug_pulsetx_walk(int n_psk, int interpolation, const float *taps, int taps_length, int first_stage, int last_stage, const void *in, long long n,
                                      const long long *cuts, int n_cuts, void *out)
{
    const float one = 1.f;
    if (first_stage == PULSETX_MOD && last_stage == PULSETX_MOD) { taps = &one; taps_length = 1; if (interpolation < 1) interpolation = 1; }
    if (check_cfg(n_psk, interpolation, taps_length, first_stage, last_stage) < 0) return -3;
    if (!taps || n < 0 || n > (1LL << 30) || (n > 0 && (!in || !out)) || n_cuts < 0 || (n_cuts && !cuts)) return fail_msg(-3, "debug_pulsetx_walk: bad arguments");
    const PulseTxCfg g = make_cfg(interpolation, taps_length, first_stage, last_stage);
    if (n * (last_stage == PULSETX_SHAPE ? g.I : 1) > INT_MAX) return fail_msg(-3, "debug_pulsetx_walk: more than 2^31 - 1 outputs");
    csdr_complexf symc[256];
    if (csdr_amd_psk31tx_tables(n_psk, 1, symc, nullptr) < 0) return -3;
    float2 sym[256];
    memcpy(sym, symc, sizeof sym);
    std::vector<float2> hist(std::max(g.H, 1), make_float2(0.f, 0.f)), next(hist);
    const size_t isz = first_stage == PULSETX_SHAPE ? sizeof(float2) : 1;
    float2 *y = (float2 *)out;
    long long w = 0;
    for_each_call(n, cuts, n_cuts, [&](long long done, long long m) {
        if (!m) return;
        const char *x = (const char *)in + done * isz;
        const PulseTxCall k = make_call(g, done, m);
        const PulseTxSrc s{hist.data(), first_stage == PULSETX_MOD ? (const uint8_t *)x : nullptr, first_stage == PULSETX_SHAPE ? (const float2 *)x : nullptr, sym};
        if (last_stage == PULSETX_MOD) for (int o = 0; o < k.n_out; o++) y[w++] = sym[s.in_b[o]];
        else {
            for (int o = 0; o < k.n_out; o++) y[w++] = pulsetx_output(g, k, s, taps, o);
            for (int h = 0; h < g.H; h++) next[h] = pulsetx_next_hist(g, k, s, h);
            hist.swap(next);
        }
    });
    return w;
}

csdr_amd_pulserx *csdr_amd_pulserx_create(csdr_amd_ctx *c, const csdr_amd_pulserx_params *params, int n_channels, int first_stage, int last_stage)
{
    PulseRxCfg cfg;
    if (bank_create_check("pulserx", c, n_channels) < 0 || make_rx_cfg(params, first_stage, last_stage, &cfg) < 0) return nullptr;
    Owned<csdr_amd_pulserx, csdr_amd_pulserx_destroy> p(new csdr_amd_pulserx());
    p->c = c; p->cfg = cfg; p->n_ch = n_channels;
    p->tail_cap = 3 * cfg.t.hb + cfg.T;
    p->cus = current_device_cu_count();
    p->ring = rx_ring(cfg);
    int G;
    if (p->ring && rx_tiled_channels(cfg, p->ring, 1, &G) < 1) p->ring = 0;                        // 0: the shape runs on k_pulserx_generic
    if (dev_alloc(p->d_st, sizeof(PulseRxChan) * n_channels) != hipSuccess || dev_alloc(p->d_tail, sizeof(float2) * (size_t)p->tail_cap * n_channels) != hipSuccess ||
        dev_alloc(p->d_taps, sizeof(float) * cfg.T) != hipSuccess) { fail_msg(-2, "pulserx: out of device memory"); return nullptr; }
    const float one = 1.f;
    if (csdr_amd_h2d(c, p->d_taps.get(), first_stage == PULSERX_FILTER ? params->taps : &one, sizeof(float) * cfg.T) < 0 || csdr_amd_pulserx_reset(p.get()) < 0) return nullptr;
    return p.release();
}

int csdr_amd_pulserx_reset(csdr_amd_pulserx *p) { return bank_reset(p, "pulserx", (const PulseRxChan *)nullptr); }
int csdr_amd_pulserx_reset_channel(csdr_amd_pulserx *p, int ch) { return bank_reset_channel(p, "pulserx", ch, PulseRxChan{0, 0, 0}); }
int csdr_amd_pulserx_get_channel(csdr_amd_pulserx *p, int ch, csdr_amd_pulserx_chan *out) { return bank_get_channel(p, "pulserx", ch, out); }

int csdr_amd_pulserx_set_channel(csdr_amd_pulserx *p, int ch, const csdr_amd_pulserx_chan *s)
{
    return bank_set_channel(p, "pulserx", ch, s, [&] {
        return s->tail_len >= 0 && s->tail_len <= p->tail_cap - 1 ? 0 : fail_msg(-3, "pulserx: tail_len out of range");
    });
}

int csdr_amd_pulserx_set_lanes(csdr_amd_pulserx *p, int lanes) { return bank_set_lanes(p, "pulserx", lanes); }

long long csdr_amd_pulserx_max_out(const csdr_amd_pulserx *p, long long n_in)
{
    if (!p || n_in < 0) return 0;
    return ((n_in + p->tail_cap) / p->cfg.t.hb + 1) * (1 + p->cfg.slice_q);                      // every symbol moves on by at least D/2 samples
}

int csdr_amd_pulserx_process(csdr_amd_pulserx *p, const csdr_complexf *in, long long n_in, size_t in_pitch, void *out, size_t out_pitch, int *counts, float *err,
                             unsigned *idx)
{
    if (!p) return fail_msg(-3, "pulserx: null object");
    if (n_in < 0 || n_in > (1LL << 30) || (n_in > 0 && (!in || in_pitch < (size_t)n_in))) return fail_msg(-3, "pulserx: need in_pitch >= n_in >= 0 (n_in <= 2^30)");
    if (!counts) return fail_msg(-3, "pulserx: counts is required");
    if ((err || idx) && p->cfg.last != PULSERX_TIMING) return fail_msg(-3, "pulserx: error and index outputs need last_stage == timing recovery");
    const long long mo = csdr_amd_pulserx_max_out(p, n_in);
    if (!out || out_pitch < (size_t)mo) return fail_msg(-3, "pulserx: out_pitch %zu below max_out %lld", out_pitch, mo);
    csdr_amd_ctx *c = p->c;
    int C = 0, G = 16;
    if (p->ring && !p->force_generic) C = rx_tiled_channels(p->cfg, p->ring, bank_lanes(p, default_rx_lanes(p->cus, p->n_ch, true)), &G);
    if (C > 0) {
        p->last_kernel = "k_pulserx_tiled";
#define PULSERX_TILED(GV) hipLaunchKernelGGL(k_pulserx_tiled<GV>, dim3(cdiv(p->n_ch, C)), dim3(64), rx_lds(p->cfg, C, p->ring), c->stream, p->cfg, p->d_st.get(), \
                                             p->d_tail.get(), p->tail_cap, p->n_ch, C, p->ring, p->d_taps.get(), (const float2 *)in, n_in, in_pitch, out, out_pitch, \
                                             counts, err, idx)
        if (G == 4) PULSERX_TILED(4); else if (G == 8) PULSERX_TILED(8); else PULSERX_TILED(16);
#undef PULSERX_TILED
    } else {
        const int lanes = bank_launch_lanes(p, "k_pulserx_generic", default_rx_lanes(p->cus, p->n_ch, false));
        hipLaunchKernelGGL(k_pulserx_generic, dim3(cdiv(p->n_ch, lanes)), dim3(64), 0, c->stream, p->cfg, p->d_st.get(), p->d_tail.get(), p->tail_cap, p->n_ch, lanes,
                           p->d_taps.get(), (const float2 *)in, n_in, in_pitch, out, out_pitch, counts, err, idx);
    }
    CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_pulserx_force_generic(csdr_amd_pulserx *p, int on) { return bank_force_generic(p, "pulserx", on); }

int csdr_amd_pulserx_lanes(const csdr_amd_pulserx *p)
{
    if (!p) return 0;
    const bool tiled = p->ring && !p->force_generic;
    const int want = bank_lanes(p, default_rx_lanes(p->cus, p->n_ch, tiled));
    int G;
    return tiled ? rx_tiled_channels(p->cfg, p->ring, want, &G) : want;
}

const char *csdr_amd_pulserx_kernel_name(const csdr_amd_pulserx *p) { return bank_kernel_name(p); }

void csdr_amd_pulserx_destroy(csdr_amd_pulserx *p) { destroy_on_stream(p); }

// CPU run of the receive object's walk for one channel, the stream cut into calls of cuts[0], cuts[1], ... samples (the rest of n in one more call).
// Outputs of all calls are concatenated; state_io (may be NULL: a fresh channel) carries the channel state in and out.  Returns the output count.
long long csdr_amd_debug_pulserx_walk(const csdr_amd_pulserx_params *params, int first_stage, int last_stage, const csdr_complexf *in, long long n,
                                      const long long *cuts, int n_cuts, void *out, float *err, unsigned *idx, csdr_amd_pulserx_chan *state_io)
{
    PulseRxCfg cfg;
    if (make_rx_cfg(params, first_stage, last_stage, &cfg) < 0) return -3;
    if (n < 0 || n > (1LL << 30) || (n > 0 && (!in || !out)) || n_cuts < 0 || (n_cuts && !cuts)) return fail_msg(-3, "debug_pulserx_walk: bad arguments");
    if ((err || idx) && last_stage != PULSERX_TIMING) return fail_msg(-3, "debug_pulserx_walk: error and index outputs need last_stage == timing recovery");
    PulseRxChan s{0, 0, 0};
    if (state_io) memcpy(&s, state_io, sizeof s);
    if (s.tail_len != 0) return fail_msg(-3, "debug_pulserx_walk: a state with a tail cannot be carried in");
    std::vector<float2> tail(3 * (size_t)cfg.t.hb + cfg.T + 1);
    const float one = 1.f;
    const float *taps = first_stage == PULSERX_FILTER ? params->taps : &one;
    long long k = 0;
    for_each_call(n, cuts, n_cuts, [&](long long done, long long m) {
        PulseRxOut o{nullptr, nullptr, err ? err + k : nullptr, idx ? idx + k : nullptr};
        if (last_stage == PULSERX_TIMING) o.c = (float2 *)out + k; else o.b = (uint8_t *)out + k;
        k += pulserx_walk(cfg, s, tail.data(), (const float2 *)in + done, m, taps, o);
    });
    if (state_io) memcpy(state_io, &s, sizeof s);
    return k;
}

int csdr_amd_generic_slicer_f_u8(csdr_amd_ctx *c, const float *in, unsigned char *out, int n_streams, long long n, size_t in_pitch, size_t out_pitch, int n_symbols)
{
    if (!c || n_streams < 1 || n_streams > 65535) return fail_msg(-3, "generic_slicer_f_u8: need a context and 1 <= n_streams <= 65535");
    if (n_symbols < 2 || n_symbols > 256) return fail_msg(-3, "generic_slicer_f_u8: n_symbols should be between 2 and 256");
    if (n < 0 || (n > 0 && (!in || !out || in_pitch < (size_t)n || out_pitch < (size_t)n))) return fail_msg(-3, "generic_slicer_f_u8: need pitches >= n >= 0");
    if (!n) return 0;
    const float d = (float)(2.0 / (n_symbols - 1));
    hipLaunchKernelGGL(k_generic_slicer, dim3(flat_blocks(n), n_streams), dim3(256), 0, c->stream, in, out, n, in_pitch, out_pitch, n_symbols, d);
    CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_plain_interpolate_cc(csdr_amd_ctx *c, const csdr_complexf *in, csdr_complexf *out, int n_streams, long long n, size_t in_pitch, size_t out_pitch,
                                  int interpolation)
{
    if (!c || n_streams < 1 || n_streams > 65535) return fail_msg(-3, "plain_interpolate_cc: need a context and 1 <= n_streams <= 65535");
    if (interpolation <= 0) return fail_msg(-3, "plain_interpolate_cc: interpolation should be >0");
    if (n < 0 || n > LLONG_MAX / 16 / interpolation) return fail_msg(-3, "plain_interpolate_cc: need n >= 0 (and n * interpolation within range)");
    const long long n_out = n * interpolation;
    if (n_out > 0 && (!in || !out || in == out || in_pitch < (size_t)n || out_pitch < (size_t)n_out))
        return fail_msg(-3, "plain_interpolate_cc: need in_pitch >= n, out_pitch >= n * interpolation and out apart from in");
    if (!n_out) return 0;
    hipLaunchKernelGGL(k_plain_interpolate, dim3(flat_blocks(n_out), n_streams), dim3(256), 0, c->stream, (const float2 *)in, (float2 *)out, n_out, in_pitch, out_pitch,
                       interpolation);
    CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_pack_bits_1to8_u8_u8(csdr_amd_ctx *c, const unsigned char *in, unsigned char *out, int n_streams, long long n, size_t in_pitch, size_t out_pitch)
{
    if (!c || n_streams < 1 || n_streams > 65535) return fail_msg(-3, "pack_bits_1to8_u8_u8: need a context and 1 <= n_streams <= 65535");
    if (n < 0 || n > LLONG_MAX / 16) return fail_msg(-3, "pack_bits_1to8_u8_u8: need n >= 0");
    if (n > 0 && (!in || !out || in == out || in_pitch < (size_t)n || out_pitch < (size_t)(8 * n)))
        return fail_msg(-3, "pack_bits_1to8_u8_u8: need in_pitch >= n, out_pitch >= 8 n and out apart from in");
    if (!n) return 0;
    hipLaunchKernelGGL(k_pack_bits_1to8, dim3(flat_blocks(8 * n), n_streams), dim3(256), 0, c->stream, in, out, 8 * n, in_pitch, out_pitch);
    CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_pack_bits_8to1_u8_u8(csdr_amd_ctx *c, const unsigned char *in, unsigned char *out, int n_streams, long long n, size_t in_pitch, size_t out_pitch)
{
    if (!c || n_streams < 1 || n_streams > 65535) return fail_msg(-3, "pack_bits_8to1_u8_u8: need a context and 1 <= n_streams <= 65535");
    if (n < 0 || (n & 7)) return fail_msg(-3, "pack_bits_8to1_u8_u8: n should be a multiple of 8 (and >= 0)");
    if (n > 0 && (!in || !out || in == out || in_pitch < (size_t)n || out_pitch < (size_t)(n / 8)))
        return fail_msg(-3, "pack_bits_8to1_u8_u8: need in_pitch >= n, out_pitch >= n / 8 and out apart from in");
    if (!n) return 0;
    hipLaunchKernelGGL(k_pack_bits_8to1, dim3(flat_blocks(n / 8), n_streams), dim3(256), 0, c->stream, in, out, n / 8, in_pitch, out_pitch);
    CSDR_LAUNCH_CHECK();
    return 0;
}

// apply_real_fir_cc (libcsdr.c:2276-2291): the FIR decimator at decimation 1
int csdr_amd_apply_real_fir_cc(csdr_amd_ctx *c, const csdr_complexf *in, csdr_complexf *out, int n_streams, int input_size, size_t in_pitch, size_t out_pitch,
                               const float *taps, int taps_length)
{
    if (!c || n_streams < 1) return fail_msg(-3, "apply_real_fir_cc: need a context and n_streams >= 1");
    if (taps_length <= 0 || !taps) return fail_msg(-3, "apply_real_fir_cc: taps_length should be >0");
    if (input_size < taps_length) return 0;
    if (!in || !out || in_pitch < (size_t)input_size || out_pitch < (size_t)(input_size - taps_length + 1))
        return fail_msg(-3, "apply_real_fir_cc: need in_pitch >= input_size and out_pitch >= input_size - taps_length + 1");
    return csdr_amd_fir_decimate_cc(c, in, out, n_streams, input_size, in_pitch, out_pitch, 1, taps, taps_length);
}

// firdes_rrc_f (libcsdr.c:2482-2497), normalize_fir_f included.  taps_length odd: for an even length the reference writes taps[taps_length].
int csdr_amd_firdes_rrc_f(float *taps, int taps_length, int samples_per_symbol, float beta)
{
    if (!taps || taps_length < 1 || !(taps_length & 1)) return fail_msg(-3, "firdes_rrc_f: taps_length should be odd (and >0)");
    if (samples_per_symbol < 1) return fail_msg(-3, "firdes_rrc_f: samples_per_symbol should be >0");
    firdes_rrc_below(taps, taps_length, samples_per_symbol, beta);
    return 0;
}

// firdes_cosine_f (libcsdr.c:2473-2480), meant for taps_length = 2 samples_per_symbol + 1.  The reference writes the middle 2 samples_per_symbol - 1 taps
// only; the others (the two end taps of the intended length) are 0 here.
int csdr_amd_firdes_cosine_f(float *taps, int taps_length, int samples_per_symbol)
{
    if (!taps || samples_per_symbol < 1) return fail_msg(-3, "firdes_cosine_f: samples_per_symbol should be >0");
    const int middle_i = taps_length / 2;
    if (taps_length < 1 || middle_i - (samples_per_symbol - 1) < 0 || middle_i + samples_per_symbol - 1 >= taps_length)
        return fail_msg(-3, "firdes_cosine_f: taps_length should be at least 2 * samples_per_symbol - 1");
    for (int i = 0; i < taps_length; i++) taps[i] = 0.f;
    for (int i = 0; i < samples_per_symbol; i++)
        taps[middle_i + i] = taps[middle_i - i] = (float)((1 + cos((double)(PI_F * (float)i / (float)samples_per_symbol))) / 2);
    float sum = 0;
    for (int i = 0; i < taps_length; i++) sum += taps[i];
    for (int i = 0; i < taps_length; i++) taps[i] = taps[i] / sum;
    return 0;
}

} // extern "C"
