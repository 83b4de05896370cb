// modem.hip -- the pulse-shaped symbol modem for n_channels channels per call (MI355X / gfx950):
//   psk_modulator_u8_c n_psk | plain_interpolate_cc I | pulse_shaping_filter_cc (apply_real_fir_cc, T taps)        (modem_dev.hpp: the definitions)
// as one object, and the flat operators generic_slicer_f_u8, plain_interpolate_cc, pack_bits_1to8_u8_u8, pack_bits_8to1_u8_u8, apply_real_fir_cc and the
// designs firdes_rrc_f / firdes_cosine_f.
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
