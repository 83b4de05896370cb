// txmod.hip -- the transmit side (MI355X / gfx950): the analog modulators fmmod_fc, dsb_fc, add_dcoffset_cc, fixed_amplitude_cc and convert_f_samplerf
// (libcsdr.c:1174-1208, csdr.c:2084-2127), and the fused up-converter bank csdr_amd_txbank_* for n_streams s16 audio streams:
//
//     convert_s16_f | gain_ff g | fmmod_fc or dsb_fc q [| add_dcoffset_cc] | fir_interpolate_cc I (taps) | shift_addition_cc r_s | [convert_f_u8]
//
//   k_fmmod       the FM phase chain is serial per stream (float32: product, sum, wrap) and cheap; cos and sin of the stored phases are not serial.  One wave takes C
//                 streams: per tile of 64 samples all lanes stage the C rows' increments into LDS (coalesced, the next tile's loads in flight), lane c walks row c
//                 and leaves the phases there, and all 64 lanes take cos and sin of every row and write it back coalesced.
//   k_tx_mod_am   dsb_fc [| add_dcoffset_cc] on the converted audio: elementwise.
//   Both write the modulated baseband at the AUDIO rate into a row per stream in HBM, behind the K samples of history the interpolator keeps: 1 / I of the output traffic.
//   k_tx_seeds    shift_addition_cc restarts its phasor every 1024 samples from (cos, sin) of a float phase carried from chunk to chunk (csdr.c:911-918): one lane per
//                 stream replays that float chain for the chunks of the call with seeds.hpp's wrap plan.
//   k_tx_ckpt     inside a chunk the phasor is the float recurrence c' = c cosd - s sind, s' = s cosd + c sind (libcsdr_gpl.c:40-44).  It has to be replayed rounding
//                 for rounding: on rates with a short period (0.05, 0.2, 0.25, ...) its rounding errors add up coherently, to 1e-5 relative RMS within one chunk
//                 against the exact power of the rounded step.  One lane per (stream, chunk) walks the 1024 steps once and keeps every 16th phasor: half a byte
//                 of table per output sample.
//   k_tx_up       the hot kernel.  A workgroup takes P input positions of one stream: the baseband tile plus halo and the polyphase taps go to LDS, a lane evaluates
//                 8 branches of 2 positions (16 outputs: every tap is read once for 2 products, every sample once for 8) and stages the results in LDS; a lane per
//                 run of 16 outputs then takes the run's checkpoint, steps the recurrence and rotates the staged values in place; and all lanes convert and store
//                 them in 16-byte pieces: each output byte is written once, coalesced.
//   k_tx_up_generic   one output per lane straight from and to global memory, any pointer and pitch.  The same operations in the same order: the same bits.
#include "bank.hpp"
#include "txmod_dev.hpp"
#include "seeds.hpp"
#include <string.h>
#include <math.h>
#include <algorithm>
#include <vector>

using namespace csdr_amd;

namespace {

// ------------------------------------------------------------------ fmmod_fc
constexpr int FT = 64;                                   // samples per tile (= lanes per wave)
constexpr int FTP = FT + 1;                              // odd row stride: the chain lanes' same-column accesses fall in different banks
constexpr int FCMAX = 16;                                // streams per wave at most (one sample per stream is held ahead in registers)

struct FmArgs {
    const void *in; size_t in_pitch; float gain;         // S16: convert_s16_f | gain_ff in front
    float *out; size_t out_pitch; int out_al8;           // complex rows; out_al8: rows can be written as float2
    long long n; int n_streams, C; float *phase_io;
};

template <bool S16>
__global__ __launch_bounds__(64) void k_fmmod(FmArgs a)
{
    __shared__ float d[FCMAX * FTP];
    const int lane = threadIdx.x, s0 = blockIdx.x * a.C;
    const int nc = min(a.C, a.n_streams - s0);
    const bool chain = lane < nc;
    float p = chain ? a.phase_io[s0 + lane] : 0.f;
    const int me = lane * FTP;

    float nx[FCMAX];
    auto fetch = [&](long long b) {
#pragma unroll
        for (int cc = 0; cc < FCMAX; cc++) {
            if (cc < nc) {
                const size_t g = (size_t)(s0 + cc) * a.in_pitch + b + lane;
                if (b + lane < a.n) nx[cc] = S16 ? tx_audio(((const int16_t *)a.in)[g], a.gain) : ((const float *)a.in)[g];
                else nx[cc] = 0.f;
            }
        }
    };
    fetch(0);
    for (long long base = 0; base < a.n; base += FT) {
#pragma unroll
        for (int cc = 0; cc < FCMAX; cc++)               // 1. stage: lane j holds the increment of sample base + j of stream cc
            if (cc < nc) d[cc * FTP + lane] = fmmod_delta(nx[cc]);
        __syncthreads();
        if (base + FT < a.n) fetch(base + FT);
        if (chain) {                                     // 2. lane c walks stream c
            const int m = (int)min((long long)FT, a.n - base);
            for (int j0 = 0; j0 < m; j0 += 8) {
                float v[8];                              // 8 increments to registers first: the LDS latency stays off the chain
#pragma unroll
                for (int j = 0; j < 8; j++) v[j] = d[me + j0 + j];
#pragma unroll
                for (int j = 0; j < 8; j++)
                    if (j0 + j < m) { p = fmmod_phase_step(p, v[j]); d[me + j0 + j] = p; }
            }
        }
        __syncthreads();
        if (base + lane < a.n) {                         // 3. cos and sin on all lanes, written back coalesced
            for (int cc = 0; cc < nc; cc++) {
                const float2 o = fmmod_output(d[cc * FTP + lane]);
                const size_t g = (size_t)(s0 + cc) * a.out_pitch + base + lane;
                if (a.out_al8) ((float2 *)a.out)[g] = o;
                else { a.out[2 * g] = o.x; a.out[2 * g + 1] = o.y; }
            }
        }
    }
    if (chain) a.phase_io[s0 + lane] = p;
}

// ------------------------------------------------------------------ the elementwise operators
enum { EW_DSB = 0, EW_DCOFFSET = 1, EW_FIXAMP = 2 };
template <int OP>
__global__ __launch_bounds__(256) void k_tx_elementwise(const float *__restrict__ in, float *__restrict__ out, size_t n, float param)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        float2 o;
        if (OP == EW_DSB) o = dsb_value(in[k], param);
        else if (OP == EW_DCOFFSET) o = add_dcoffset_value(make_float2(in[2 * k], in[2 * k + 1]));
        else o = fixed_amplitude_value(make_float2(in[2 * k], in[2 * k + 1]), param);
        out[2 * k] = o.x; out[2 * k + 1] = o.y;
    }
}

__global__ __launch_bounds__(256) void k_samplerf(const float *__restrict__ in, uint32_t *__restrict__ out, size_t n, uint32_t wait)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        const unsigned long long b = (unsigned long long)__double_as_longlong((double)in[k]);
        out[4 * k] = (uint32_t)b; out[4 * k + 1] = (uint32_t)(b >> 32); out[4 * k + 2] = wait; out[4 * k + 3] = 0u;
    }
}

inline unsigned grid1(size_t n) { size_t g = (n + 255) / 256; if (g < 1) g = 1; if (g > 4096) g = 4096; return (unsigned)g; }

// ------------------------------------------------------------------ the bank: audio-rate modulation of the AM family
__global__ __launch_bounds__(256) void k_tx_mod_am(const int16_t *__restrict__ in, size_t in_pitch, float2 *__restrict__ bb, size_t bb_pitch, long long n,
                                                   float gain, float q_value, int dcoffset)
{
    const int s = blockIdx.y;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < (size_t)n; k += stride) {
        float2 v = dsb_value(tx_audio(in[(size_t)s * in_pitch + k], gain), q_value);
        if (dcoffset) v = add_dcoffset_value(v);
        bb[(size_t)s * bb_pitch + k] = v;
    }
}

// the interpolator's history: the last `keep` of the `have` samples from `from` on move to the front of the row, to end at index K
__global__ __launch_bounds__(256) void k_tx_keep(float2 *__restrict__ bb, size_t bb_pitch, int from, int have, int keep, int K)
{
    float2 *row = bb + (size_t)blockIdx.x * bb_pitch;
    float2 v[4];                                         // keep <= K <= 1024
#pragma unroll
    for (int r = 0; r < 4; r++) { const int j = threadIdx.x + 256 * r; if (j < keep) v[r] = row[from + have - keep + j]; }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; r++) { const int j = threadIdx.x + 256 * r; if (j < keep) row[K - keep + j] = v[r]; }
}

// ------------------------------------------------------------------ the bank: rotator bookkeeping
struct RotState { float *phase; int *off; const float *rate; };      // per stream: phase in front of the current chunk, outputs already in it, shift rate

__global__ __launch_bounds__(64) void k_tx_seeds(RotState r, int n_streams, long long n_out, float *__restrict__ seeds, size_t seed_pitch, int *__restrict__ off_call)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_streams) return;
    float ph = r.phase[s];
    const int off = r.off[s];
    off_call[s] = off;
    const float step = r.rate[s] * 2 * TXMOD_PI * 1024.f;                // d.rate PI n, d.rate the doubled rate (libcsdr_gpl.c:50, 83)
    WrapPlan w;
    wrap_plan_init(w, step);
    const long long total = off + n_out, full = total >> 10;
    for (long long c = 0; c <= full; c++) {
        seeds[(size_t)s * seed_pitch + c] = ph;
        if (c < full) ph = wrap_plan_apply(w, ph + step);
    }
    r.phase[s] = ph; r.off[s] = (int)(total & 1023);
}

constexpr int CK = 16;                                   // outputs per checkpoint of the phasor recurrence
constexpr int CKN = 1024 / CK;                           // checkpoints per chunk

__device__ __forceinline__ float2 rot_step(float2 p, float sd, float cd) { return make_float2(p.x * cd - p.y * sd, p.y * cd + p.x * sd); }   // libcsdr_gpl.c:40-44

// lane = (stream, chunk of the call): the chunk's phasors at offsets 0, 16, 32, ...
__global__ __launch_bounds__(64) void k_tx_ckpt(const float *__restrict__ seeds, size_t seed_pitch, const int *__restrict__ off_call, long long n_out,
                                                const float2 *__restrict__ sdcd, float2 *__restrict__ ckpt)
{
    const int s = blockIdx.y;
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c > ((off_call[s] + n_out) >> 10)) return;
    const float sd = sdcd[s].x, cd = sdcd[s].y;
    float sn, cs;
    carrier_sincos(seeds[(size_t)s * seed_pitch + c], &sn, &cs);         // (float)cos((double)phase), (float)sin((double)phase): libcsdr_gpl.c:33-34
    float2 p = make_float2(cs, sn);
    float2 *o = ckpt + ((size_t)s * seed_pitch + c) * CKN;
    for (int j = 0; j < CKN; j++) {
        o[j] = p;
#pragma unroll
        for (int i = 0; i < CK; i++) p = rot_step(p, sd, cd);
    }
}

// a retune: the phase moves on over the outputs of the chunk that ends here, and a new chunk grid starts with the next output
__global__ void k_tx_retune(RotState r, float *rate_w, float2 *sdcd, int s, float rate, float sd, float cd)
{
    const int off = r.off[s];
    if (off > 0) r.phase[s] = tx_rot_advance(r.phase[s], r.rate[s] * 2, off);
    r.off[s] = 0;
    rate_w[s] = rate; sdcd[s] = make_float2(sd, cd);
}

// ------------------------------------------------------------------ the bank: interpolate, shift, convert
struct UpArgs {
    const float2 *bb; size_t bb_pitch; int first, n_valid;   // position 0 of the call is sample bb[first]; n_valid samples from there on
    long long npos;                                       // positions of the call: I outputs each
    int I, K, Ipad;                                       // K taps per branch, branches padded to a multiple of 8
    const float *tapT;                                    // [K][Ipad]: tapT[k][ip] = taps[(k + 1) I - ip], 0 beyond the filter
    const float2 *ckpt; size_t seed_pitch; const int *off; const float2 *sdcd;   // phasor checkpoints [stream][chunk][CKN]
    void *out; size_t out_pitch; int u8, P;
};

__device__ __forceinline__ float2 tx_rotate(float2 x, float2 p) { return make_float2(p.x * x.x - p.y * x.y, p.y * x.x + p.x * x.y); }      // libcsdr_gpl.c:38-39

__global__ __launch_bounds__(256) void k_tx_up_generic(UpArgs a)
{
    const int s = blockIdx.y;
    const long long n_out = a.npos * a.I;
    const float2 *row = a.bb + (size_t)s * a.bb_pitch + a.first;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const float sd = a.sdcd[s].x, cd = a.sdcd[s].y;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_out; e += stride) {
        const long long pos = e / a.I;
        const int ip = (int)(e - pos * a.I);
        float2 acc = make_float2(0.f, 0.f);
        for (int k = 0; k < a.K; k++) {
            const float2 x = row[pos + k];
            const float t = a.tapT[(size_t)k * a.Ipad + ip];
            acc.x = fmaf(x.x, t, acc.x); acc.y = fmaf(x.y, t, acc.y);
        }
        const long long q = a.off[s] + e;                               // the output's place in the stream's chunk grid
        float2 ph = a.ckpt[((size_t)s * a.seed_pitch + (q >> 10)) * CKN + ((int)(q & 1023) >> 4)];
        for (int i = 0; i < (int)(q & 15); i++) ph = rot_step(ph, sd, cd);
        const float2 y = tx_rotate(acc, ph);
        const size_t g = (size_t)s * a.out_pitch + e;
        if (a.u8) { ((uint8_t *)a.out)[2 * g] = (uint8_t)tx_to_u8(y.x); ((uint8_t *)a.out)[2 * g + 1] = (uint8_t)tx_to_u8(y.y); }
        else { ((float *)a.out)[2 * g] = y.x; ((float *)a.out)[2 * g + 1] = y.y; }
    }
}

inline size_t up_xs_len(int P, int K) { return (size_t)((P + K + 2) & ~1); }
inline size_t up_stg_len(int P, int I) { return (size_t)P * I + ((size_t)P * I + 15) / 16 + 2; }   // one pad per run of 16: the runs' lanes fall in different banks
inline size_t up_lds(int P, int I, int K, int Ipad) { return sizeof(float) * (size_t)K * Ipad + sizeof(float2) * (up_xs_len(P, K) + up_stg_len(P, I)); }

__global__ __launch_bounds__(256) void k_tx_up(UpArgs a)
{
    extern __shared__ float4 lds4[];
    float *tp = (float *)lds4;                                           // [K][Ipad]
    float2 *xs = (float2 *)(tp + (size_t)a.K * a.Ipad);                  // the tile's samples and halo
    float2 *stg = xs + ((a.P + a.K + 2) & ~1);                           // [P][I] filter outputs, one pad in front of every run of 16
    const int s = blockIdx.y, t = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * a.P;
    const int np = (int)min((long long)a.P, a.npos - p0);
    const float2 *row = a.bb + (size_t)s * a.bb_pitch + a.first;
    const int n_out = np * a.I;                                           // the tile's outputs, from e0 on
    const long long e0 = p0 * a.I, q0 = a.off[s] + e0;                    // q0: the first one's place in the stream's chunk grid
    const int al = (int)(q0 & 15);                                        // runs of 16 on that grid begin at e = 16 r - al
#define STG(e) stg[(e) + (((e) + al) >> 4)]

    for (int j = t; j < a.K * a.Ipad; j += 256) tp[j] = a.tapT[j];
    for (int j = t; j < a.P + a.K + 1; j += 256) xs[j] = p0 + j < a.n_valid ? row[p0 + j] : make_float2(0.f, 0.f);
    __syncthreads();

    const int G = a.Ipad >> 3, items = ((np + 1) >> 1) * G;
    for (int it = t; it < items; it += 256) {
        const int pp = it / G, b8 = (it - pp * G) << 3, p = 2 * pp;
        float2 acc0[8], acc1[8];
#pragma unroll
        for (int v = 0; v < 8; v++) { acc0[v] = make_float2(0.f, 0.f); acc1[v] = make_float2(0.f, 0.f); }
        float2 xa = xs[p];
        for (int k = 0; k < a.K; k++) {
            const float2 xb = xs[p + 1 + k];
            const float4 t0 = *(const float4 *)&tp[k * a.Ipad + b8], t1 = *(const float4 *)&tp[k * a.Ipad + b8 + 4];
            const float tv[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
            for (int v = 0; v < 8; v++) {
                acc0[v].x = fmaf(xa.x, tv[v], acc0[v].x); acc0[v].y = fmaf(xa.y, tv[v], acc0[v].y);
                acc1[v].x = fmaf(xb.x, tv[v], acc1[v].x); acc1[v].y = fmaf(xb.y, tv[v], acc1[v].y);
            }
            xa = xb;
        }
#pragma unroll
        for (int v = 0; v < 8; v++) {
            if (b8 + v < a.I) {
                STG(p * a.I + b8 + v) = acc0[v];
                if (p + 1 < np) STG((p + 1) * a.I + b8 + v) = acc1[v];
            }
        }
    }
    __syncthreads();

    {   // a lane per run: the run's checkpoint, then the recurrence, the staged values rotated in place
        const float sd = a.sdcd[s].x, cd = a.sdcd[s].y;
        const int runs = (n_out + al + 15) >> 4;
        for (int r = t; r < runs; r += 256) {
            const long long q = q0 - al + 16 * (long long)r;
            float2 ph = a.ckpt[((size_t)s * a.seed_pitch + (q >> 10)) * CKN + ((int)(q & 1023) >> 4)];
            float2 *run = stg + 17 * r - al;                              // STG(16 r - al + i) = run[i]
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int e = 16 * r - al + i;
                if (e >= 0 && e < n_out) run[i] = tx_rotate(run[i], ph);
                ph = rot_step(ph, sd, cd);
            }
        }
    }
    __syncthreads();

    if (a.u8) {                                                           // convert, store 16 bytes per lane
        uint8_t *o = (uint8_t *)a.out + 2 * ((size_t)s * a.out_pitch + e0);
        const int nvec = n_out >> 3;
        for (int vi = t; vi < nvec; vi += 256) {
            uint32_t w[4];
#pragma unroll
            for (int h = 0; h < 4; h++) {
                const float2 y0 = STG(8 * vi + 2 * h), y1 = STG(8 * vi + 2 * h + 1);
                w[h] = (uint32_t)tx_to_u8(y0.x) | ((uint32_t)tx_to_u8(y0.y) << 8) | ((uint32_t)tx_to_u8(y1.x) << 16) | ((uint32_t)tx_to_u8(y1.y) << 24);
            }
            *(uint4 *)(o + 16 * (size_t)vi) = make_uint4(w[0], w[1], w[2], w[3]);
        }
        for (int e = 8 * nvec + t; e < n_out; e += 256) {
            const float2 y = STG(e);
            o[2 * e] = (uint8_t)tx_to_u8(y.x); o[2 * e + 1] = (uint8_t)tx_to_u8(y.y);
        }
    } else {
        float *o = (float *)a.out + 2 * ((size_t)s * a.out_pitch + e0);
        const int nvec = n_out >> 1;
        for (int vi = t; vi < nvec; vi += 256) {
            const float2 y0 = STG(2 * vi), y1 = STG(2 * vi + 1);
            *(float4 *)(o + 4 * (size_t)vi) = make_float4(y0.x, y0.y, y1.x, y1.y);
        }
        if ((n_out & 1) && t == 0) {
            const float2 y = STG(n_out - 1);
            o[2 * (n_out - 1)] = y.x; o[2 * (n_out - 1) + 1] = y.y;
        }
    }
#undef STG
}

int check_ew(const char *name, const void *in, const void *out, size_t n)
{
    if (n > ((size_t)1 << 40)) return fail_msg(-3, "%s: n is too large", name);
    if (n && (!in || !out)) return fail_msg(-3, "%s: null pointer", name);
    if (((uintptr_t)in | (uintptr_t)out) & 3) return fail_msg(-3, "%s: pointers must be 4-byte aligned", name);
    return 0;
}

} // namespace

struct csdr_amd_txbank : Bank {                           // (n_ch: the streams)
    int mode, I, T, K, Ipad, u8; float gain, q_value; size_t max_in;
    long long hist = 0;                                   // samples the interpolator holds in front of the next call: min(total, K)
    std::vector<float> h_rates;
    size_t bb_pitch, seed_pitch;
    DevBuf<float2> d_bb, d_ckpt, d_sdcd;
    DevBuf<float> d_tapT, d_seeds, d_fm_phase, d_rot_phase, d_rate;
    DevBuf<int> d_rot_off, d_off_call;
};

namespace {
void shift_deltas(float rate, float *sd, float *cd)
{
    const float inc = rate * 2 * PI_F;                   // shift_addition_init: rate *= 2; sin(rate PI), cos(rate PI)  (libcsdr_gpl.c:81-89, the host's libm as there)
    *sd = (float)sin((double)inc); *cd = (float)cos((double)inc);
}
int check_rate(float r) { return (r >= -0.5f && r <= 0.5f) ? 0 : fail_msg(-3, "txbank: a shift rate should be -0.5 .. 0.5"); }
}

extern "C" {

int csdr_amd_fmmod_fc(csdr_amd_ctx *c, const float *in, csdr_complexf *out, int n_streams, size_t n, size_t in_pitch, size_t out_pitch, float *phase_io)
{
    if (!c) return fail_msg(-3, "fmmod_fc: null context");
    if (n_streams < 1 || n_streams > (1 << 22)) return fail_msg(-3, "fmmod_fc: n_streams should be 1 .. 4194304");
    if (n > ((size_t)1 << 30)) return fail_msg(-3, "fmmod_fc: n should be 0 .. 2^30");
    if (!phase_io) return fail_msg(-3, "fmmod_fc: phase_io is required (device float[n_streams])");
    if (n && (!in || !out || in_pitch < n || out_pitch < n)) return fail_msg(-3, "fmmod_fc: need in, out, in_pitch >= n and out_pitch >= n");
    if (((uintptr_t)in | (uintptr_t)out | (uintptr_t)phase_io) & 3) return fail_msg(-3, "fmmod_fc: pointers must be 4-byte aligned");
    if (!n) return 0;
    FmArgs a;
    a.in = in; a.in_pitch = in_pitch; a.gain = 1.f; a.out = (float *)out; a.out_pitch = out_pitch; a.out_al8 = !((uintptr_t)out & 7);
    a.n = (long long)n; a.n_streams = n_streams; a.C = std::min(FCMAX, n_streams); a.phase_io = phase_io;
    hipLaunchKernelGGL((k_fmmod<false>), dim3(cdiv(n_streams, a.C)), dim3(64), 0, c->stream, a);
    CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_dsb_fc(csdr_amd_ctx *c, const float *in, csdr_complexf *out, size_t n, float q_value)
{
    if (!c) return fail_msg(-3, "dsb_fc: null context");
    if (int rc = check_ew("dsb_fc", in, out, n)) return rc;
    if (!n) return 0;
    hipLaunchKernelGGL((k_tx_elementwise<EW_DSB>), dim3(grid1(n)), dim3(256), 0, c->stream, in, (float *)out, n, q_value); CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_add_dcoffset_cc(csdr_amd_ctx *c, const csdr_complexf *in, csdr_complexf *out, size_t n)
{
    if (!c) return fail_msg(-3, "add_dcoffset_cc: null context");
    if (int rc = check_ew("add_dcoffset_cc", in, out, n)) return rc;
    if (!n) return 0;
    hipLaunchKernelGGL((k_tx_elementwise<EW_DCOFFSET>), dim3(grid1(n)), dim3(256), 0, c->stream, (const float *)in, (float *)out, n, 0.f); CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_fixed_amplitude_cc(csdr_amd_ctx *c, const csdr_complexf *in, csdr_complexf *out, size_t n, float new_amplitude)
{
    if (!c) return fail_msg(-3, "fixed_amplitude_cc: null context");
    if (int rc = check_ew("fixed_amplitude_cc", in, out, n)) return rc;
    if (!n) return 0;
    hipLaunchKernelGGL((k_tx_elementwise<EW_FIXAMP>), dim3(grid1(n)), dim3(256), 0, c->stream, (const float *)in, (float *)out, n, new_amplitude); CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_convert_f_samplerf(csdr_amd_ctx *c, const float *in, void *out, size_t n, unsigned wait_for_this_sample)
{
    if (!c) return fail_msg(-3, "convert_f_samplerf: null context");
    if (int rc = check_ew("convert_f_samplerf", in, out, n)) return rc;
    if (!n) return 0;
    hipLaunchKernelGGL(k_samplerf, dim3(grid1(n)), dim3(256), 0, c->stream, in, (uint32_t *)out, n, (uint32_t)wait_for_this_sample); CSDR_LAUNCH_CHECK();
    return 0;
}

// CPU run of the phase step function for one stream, the samples cut into calls of cuts[0], cuts[1], ... and the rest: the phase after every sample (phases, may
// be NULL), the outputs (out, may be NULL); state_io (may be NULL: phase 0) carries last_phase in and out.  Returns n.
long long csdr_amd_debug_fmmod_walk(const float *in, long long n, const long long *cuts, int n_cuts, float *phases, csdr_complexf *out, float *state_io)
{
    if (n < 0 || (n > 0 && !in) || n_cuts < 0 || (n_cuts && !cuts)) return fail_msg(-3, "debug_fmmod_walk: bad arguments");
    float s = state_io ? *state_io : 0.f;
    for_each_call(n, cuts, n_cuts, [&](long long done, long long m) {
        float p = s;                                     // a call: last_phase in, samples, last_phase out
        for (long long j = done; j < done + m; j++) {
            p = fmmod_phase_step(p, fmmod_delta(in[j]));
            if (phases) phases[j] = p;
            if (out) { const float2 o = fmmod_output(p); out[j].i = o.x; out[j].q = o.y; }
        }
        s = p;
    });
    if (state_io) *state_io = s;
    return n;
}

// ------------------------------------------------------------------ the bank
csdr_amd_txbank *csdr_amd_txbank_create(csdr_amd_ctx *c, int n_streams, int mode, float gain, float q_value, int interpolation, const float *host_taps,
                                        int taps_length, const float *shift_rates, int out_format, size_t max_in_samples)
{
    if (bank_create_check("txbank", c, n_streams, 65535, "n_streams") < 0) return nullptr;
    if (mode < CSDR_TX_FM || mode > CSDR_TX_DSB) { fail_msg(-3, "txbank: mode is 0 (FM), 1 (AM) or 2 (DSB)"); return nullptr; }
    if (out_format != CSDR_TX_OUT_CF32 && out_format != CSDR_TX_OUT_U8) { fail_msg(-3, "txbank: out_format is 0 (cf32) or 1 (u8)"); return nullptr; }
    if (!(fabsf(gain) <= 1e30f) || !(fabsf(q_value) <= 1e30f)) { fail_msg(-3, "txbank: gain and q_value should be finite"); return nullptr; }
    if (interpolation < 1 || interpolation > 4096) { fail_msg(-3, "txbank: interpolation should be 1 .. 4096"); return nullptr; }
    if (!host_taps || taps_length < 2 || taps_length > (1 << 20)) { fail_msg(-3, "txbank: need taps, taps_length 2 .. 1048576"); return nullptr; }
    const int I = interpolation, T = taps_length, K = (T - 1 + I - 1) / I;
    if (K > 1024) { fail_msg(-3, "txbank: at most 1024 taps per branch (taps_length <= 1024 interpolation)"); return nullptr; }
    if (!shift_rates) { fail_msg(-3, "txbank: shift_rates is required (n_streams floats)"); return nullptr; }
    for (int s = 0; s < n_streams; s++) if (check_rate(shift_rates[s]) < 0) return nullptr;
    if (max_in_samples < 1 || max_in_samples * (size_t)I > ((size_t)1 << 30)) { fail_msg(-3, "txbank: max_in_samples should be 1 .. 2^30 / interpolation"); return nullptr; }

    Owned<csdr_amd_txbank, csdr_amd_txbank_destroy> p(new csdr_amd_txbank());
    p->c = c; p->n_ch = n_streams; p->mode = mode; p->I = I; p->T = T; p->K = K; p->Ipad = (I + 7) & ~7; p->u8 = out_format == CSDR_TX_OUT_U8;
    p->gain = gain; p->q_value = q_value; p->max_in = max_in_samples;
    p->h_rates.assign(shift_rates, shift_rates + n_streams);
    p->bb_pitch = ((size_t)K + max_in_samples + 1) & ~(size_t)1;
    p->seed_pitch = (max_in_samples * I + 1023) / 1024 + 2;
    const size_t ns = n_streams;
    if (dev_alloc(p->d_bb, sizeof(float2) * ns * p->bb_pitch) != hipSuccess || dev_alloc(p->d_seeds, sizeof(float) * ns * p->seed_pitch) != hipSuccess ||
        dev_alloc(p->d_ckpt, sizeof(float2) * ns * p->seed_pitch * CKN) != hipSuccess || dev_alloc(p->d_sdcd, sizeof(float2) * ns) != hipSuccess ||
        dev_alloc(p->d_tapT, sizeof(float) * (size_t)K * p->Ipad) != hipSuccess || dev_alloc(p->d_fm_phase, sizeof(float) * ns) != hipSuccess ||
        dev_alloc(p->d_rot_phase, sizeof(float) * ns) != hipSuccess || dev_alloc(p->d_rate, sizeof(float) * ns) != hipSuccess ||
        dev_alloc(p->d_rot_off, sizeof(int) * ns) != hipSuccess || dev_alloc(p->d_off_call, sizeof(int) * ns) != hipSuccess) {
        fail_msg(-2, "txbank: out of device memory"); return nullptr;
    }
    // polyphase table: output i I + ip is the sum over k of x[i + k] taps[(k + 1) I - ip]  (libcsdr.c:590-600)
    std::vector<float> tapT((size_t)K * p->Ipad, 0.f);
    for (int k = 0; k < K; k++)
        for (int ip = 0; ip < I; ip++) { const long long ti = (long long)(k + 1) * I - ip; if (ti < T) tapT[(size_t)k * p->Ipad + ip] = host_taps[ti]; }
    std::vector<float2> sdcd(ns);
    for (int s = 0; s < n_streams; s++) shift_deltas(shift_rates[s], &sdcd[s].x, &sdcd[s].y);
    if (csdr_amd_ctx_sync(c) < 0) return nullptr;
    if (csdr_amd_h2d(c, p->d_tapT.get(), tapT.data(), sizeof(float) * tapT.size()) < 0 || csdr_amd_h2d(c, p->d_sdcd.get(), sdcd.data(), sizeof(float2) * ns) < 0 ||
        csdr_amd_h2d(c, p->d_rate.get(), shift_rates, sizeof(float) * ns) < 0) return nullptr;
    if (csdr_amd_txbank_reset(p.get()) < 0) return nullptr;
    return p.release();
}

// stream start: FM phase 0, no interpolator history, rotator phase 0 with the chunk grid at the next output.  The shift rates stay as they were last set.
int csdr_amd_txbank_reset(csdr_amd_txbank *p)
{
    if (!p) return fail_msg(-3, "txbank: null object");
    const size_t ns = p->n_ch;
    p->hist = 0;
    if (int rc = csdr_amd_memset(p->c, p->d_fm_phase.get(), 0, sizeof(float) * ns)) return rc;
    if (int rc = csdr_amd_memset(p->c, p->d_rot_phase.get(), 0, sizeof(float) * ns)) return rc;
    return csdr_amd_memset(p->c, p->d_rot_off.get(), 0, sizeof(int) * ns);
}

int csdr_amd_txbank_set_rate(csdr_amd_txbank *p, int stream, float rate)
{
    if (!p || stream < 0 || stream >= p->n_ch) return fail_msg(-3, "txbank: stream out of range");
    if (int rc = check_rate(rate)) return rc;
    CSDR_HIP(hipSetDevice(p->c->device));
    float sd, cd;
    shift_deltas(rate, &sd, &cd);
    const RotState r{p->d_rot_phase.get(), p->d_rot_off.get(), p->d_rate.get()};
    hipLaunchKernelGGL(k_tx_retune, dim3(1), dim3(1), 0, p->c->stream, r, p->d_rate.get(), p->d_sdcd.get(), stream, rate, sd, cd); CSDR_LAUNCH_CHECK();
    p->h_rates[stream] = rate;
    return 0;
}

float csdr_amd_txbank_get_rate(const csdr_amd_txbank *p, int stream)
{
    if (!p || stream < 0 || stream >= p->n_ch) { fail_msg(-3, "txbank: stream out of range"); return 0.f; }
    return p->h_rates[stream];
}

long long csdr_amd_txbank_max_out(const csdr_amd_txbank *p, long long n_in) { return p && n_in > 0 ? n_in * p->I : 0; }
int csdr_amd_txbank_force_generic(csdr_amd_txbank *p, int on) { return bank_force_generic(p, "txbank", on); }
const char *csdr_amd_txbank_kernel_name(const csdr_amd_txbank *p) { return bank_kernel_name(p); }

void csdr_amd_txbank_destroy(csdr_amd_txbank *p) { destroy_on_stream(p); }

int csdr_amd_txbank_process(csdr_amd_txbank *p, const int16_t *in_s16, size_t in_pitch, long long n_in, void *out, size_t out_pitch, long long *n_out)
{
    if (!p) return fail_msg(-3, "txbank: null object");
    if (n_out) *n_out = 0;
    if (n_in < 0 || (size_t)n_in > p->max_in) return fail_msg(-3, "txbank: n_in should be 0 .. max_in_samples (%zu)", p->max_in);
    if (!n_in) return 0;
    if (!in_s16 || in_pitch < (size_t)n_in || ((uintptr_t)in_s16 & 1)) return fail_msg(-3, "txbank: need in_s16 (2-byte aligned) and in_pitch >= n_in");
    const int K = p->K, I = p->I;
    const long long have = p->hist + n_in, npos = std::max(0LL, have - K), no = npos * I;
    if (no > 0 && (!out || out_pitch < (size_t)no)) return fail_msg(-3, "txbank: need out and out_pitch >= %lld outputs", no);
    if (no > 0 && !p->u8 && ((uintptr_t)out & 3)) return fail_msg(-3, "txbank: a cf32 output must be 4-byte aligned");
    CSDR_HIP(hipSetDevice(p->c->device));
    hipStream_t st = p->c->stream;
    const int ns = p->n_ch;

    // 1. modulate at the audio rate, behind the history: row = [K - hist, K) history, [K, K + n_in) new
    if (p->mode == CSDR_TX_FM) {
        FmArgs a;
        a.in = in_s16; a.in_pitch = in_pitch; a.gain = p->gain; a.out = (float *)(p->d_bb.get() + K); a.out_pitch = p->bb_pitch; a.out_al8 = 1;
        a.n = n_in; a.n_streams = ns; a.C = std::min(FCMAX, ns); a.phase_io = p->d_fm_phase.get();
        hipLaunchKernelGGL((k_fmmod<true>), dim3(cdiv(ns, a.C)), dim3(64), 0, st, a);
    } else {
        const unsigned gx = std::max(1u, std::min(cdiv(n_in, 256), 65535u / std::min(ns, 4096) + 1));
        hipLaunchKernelGGL(k_tx_mod_am, dim3(gx, ns), dim3(256), 0, st, in_s16, in_pitch, p->d_bb.get() + K, p->bb_pitch, n_in, p->gain, p->q_value,
                           p->mode == CSDR_TX_AM ? 1 : 0);
    }
    CSDR_LAUNCH_CHECK();

    if (npos > 0) {
        // 2. the chunk seeds of the call's outputs, and the phasor checkpoints inside the chunks
        const RotState r{p->d_rot_phase.get(), p->d_rot_off.get(), p->d_rate.get()};
        hipLaunchKernelGGL(k_tx_seeds, dim3(cdiv(ns, 64)), dim3(64), 0, st, r, ns, no, p->d_seeds.get(), p->seed_pitch, p->d_off_call.get()); CSDR_LAUNCH_CHECK();
        const long long max_chunks = ((1023 + no) >> 10) + 1;
        hipLaunchKernelGGL(k_tx_ckpt, dim3(cdiv(max_chunks, 64), ns), dim3(64), 0, st, p->d_seeds.get(), p->seed_pitch, p->d_off_call.get(), no, p->d_sdcd.get(),
                           p->d_ckpt.get());
        CSDR_LAUNCH_CHECK();

        // 3. interpolate, shift, convert
        UpArgs a;
        a.bb = p->d_bb.get(); a.bb_pitch = p->bb_pitch; a.first = (int)(K - p->hist); a.n_valid = (int)have; a.npos = npos;
        a.I = I; a.K = K; a.Ipad = p->Ipad; a.tapT = p->d_tapT.get();
        a.ckpt = p->d_ckpt.get(); a.seed_pitch = p->seed_pitch; a.off = p->d_off_call.get(); a.sdcd = p->d_sdcd.get();
        a.out = out; a.out_pitch = out_pitch; a.u8 = p->u8;
        const int P = std::max(8, std::min(512, (4096 / I) & ~7));
        a.P = P;
        const size_t esz = p->u8 ? 2 : 8, lds = up_lds(P, I, K, p->Ipad);
        const bool aligned = !((uintptr_t)out & 15) && !((out_pitch * esz) & 15);
        if (!p->force_generic && aligned && lds <= 64 * 1024) {
            hipLaunchKernelGGL(k_tx_up, dim3(cdiv(npos, P), ns), dim3(256), lds, st, a);
            p->last_kernel = "k_tx_up";
        } else {
            const unsigned gx = std::max(1u, std::min(cdiv(no, 256), 65535u / std::min(ns, 4096) + 1));
            hipLaunchKernelGGL(k_tx_up_generic, dim3(gx, ns), dim3(256), 0, st, a);
            p->last_kernel = "k_tx_up_generic";
        }
        CSDR_LAUNCH_CHECK();
    }

    // 4. the last min(have, K) samples become the history
    const int keep = (int)std::min<long long>(have, K);
    hipLaunchKernelGGL(k_tx_keep, dim3(ns), dim3(256), 0, st, p->d_bb.get(), p->bb_pitch, (int)(K - p->hist), (int)have, keep, K); CSDR_LAUNCH_CHECK();
    p->hist = keep;
    if (n_out) *n_out = no;
    return 0;
}

} // extern "C"
