// rtty.hip -- the RTTY receive chain for n_channels channels per call (MI355X / gfx950):
//   bfsk_demod_cf | serial_line_decoder_f_u8 | rtty_baudot2ascii_u8_u8      (rtty_dev.hpp: the per-output and per-channel step functions)
// and the bit-per-sample variant's binary_slicer_f_u8 and rtty_line_decoder_u8_u8.
//
// The discriminator is the arithmetic: two complex L-tap correlations per output, 16 L flops against 8 input bytes.  k_bfsk_mfma runs it on the fp32
// matrix cores as one Toeplitz-band product per output part, C_c[i][n] = sum_k A_c[i][k] B[k][n]:
//   A_c[i][k] = hf_c[k - 2 i]            the interleaved taps of part c (mark re / im, space re / im; rtty_dev.hpp), zero outside [0, 2 L)
//   B[k][n]   = xf[32 n + k]             the staged window, interleaved floats: column n = 16 consecutive outputs
// so C_c[i][n] is part c of output 16 n + i.  The four parts share each B operand, and a lane ends up holding all four parts of its outputs: the power
// difference is formed in registers.  v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain and each accumulator covers the whole K range, so every output is
// the single chain over tap floats j = 0 .. 2L-1 that k_bfsk_generic and the CPU walk compute: same bits, wherever a call starts.
// The serial decoder walks each channel's windows with one wave per channel (k_rtty_walk): the start-edge scan takes 64 samples per step, the bit sums
// and the reference's index arithmetic run in the shared step function; the remainder of a channel's window (< B samples) and its complex history
// (< L samples) stay on the device between calls.
#include "bank.hpp"
#include "rtty_dev.hpp"
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>

using namespace csdr_amd;

namespace {

static_assert(sizeof(RttyChan) == 16, "RttyChan is four ints");

int make_cfg(const csdr_amd_rtty_params *p, int first, int last, RttyCfg *c)
{
    if (!p) return fail_msg(-3, "rtty: null params");
    if (first < RTTY_BFSK || last > RTTY_BAUDOT || first > last) return fail_msg(-3, "rtty: need 0 <= first_stage <= last_stage <= 2");
    memset(c, 0, sizeof *c);
    c->first = first; c->last = last;
    if (first == RTTY_BFSK && (p->filter_length < 1 || p->filter_length > 65536)) return fail_msg(-3, "rtty: filter_length should be 1 .. 65536");
    c->L = p->filter_length;
    if (first <= RTTY_SERIAL && last >= RTTY_SERIAL) {
        if (!(p->samples_per_bits >= 1)) return fail_msg(-3, "rtty: samples_per_bits should be at least 1");
        const int maxdb = last == RTTY_SERIAL ? 32 : 8;
        if (p->databits < 1 || p->databits > maxdb) return fail_msg(-3, "rtty: databits should be between 1 and %d", maxdb);
        if (!(p->stopbits >= 1)) return fail_msg(-3, "rtty: stopbits should be equal or above 1");
        if (!(p->bit_sampling_width_ratio >= 0 && p->bit_sampling_width_ratio <= 1)) return fail_msg(-3, "rtty: bit_sampling_width_ratio should be 0 .. 1");
        if (p->cli_bufsize < 1 || p->cli_bufsize > (1 << 24)) return fail_msg(-3, "rtty: cli_bufsize should be 1 .. 16777216");
        c->spb = p->samples_per_bits; c->databits = p->databits; c->stopbits = p->stopbits; c->ratio = p->bit_sampling_width_ratio; c->B = p->cli_bufsize;
        c->all_bits = (float)(1 + p->databits) + p->stopbits;
        // a start bit at 1 or 2 whose character does not fit consumes nothing: the reference CLI stops with "got stuck" (csdr.c:2521)
        if ((float)2 + c->spb * c->all_bits >= (float)c->B)
            return fail_msg(-3, "rtty: a character (%g samples) does not fit in a window of %d samples: serial_line_decoder_f_u8 would get stuck", (double)(c->spb * c->all_bits), c->B);
    }
    return 0;
}

struct Emit {
    const RttyCfg *c; uint8_t *o; long long k; int *fig;
    __host__ __device__ void operator()(unsigned shr)
    {
        if (c->last == RTTY_SERIAL) {
            if (c->databits <= 8) o[k] = (uint8_t)shr;
            else if (c->databits <= 16) ((uint16_t *)o)[k] = (uint16_t)shr;
            else ((uint32_t *)o)[k] = shr;
            k++;
            return;
        }
        const uint8_t ch = rtty_baudot_lookup(fig, shr);
        if (ch) o[k++] = ch;
    }
};

// ---------------------------------------------------------------- the discriminator
// V(p) of channel ch: its history (h samples) then its input
struct VRow {
    const float2 *hist; const float2 *in; int h;
    __device__ float2 operator()(long long p) const { return p < h ? hist[p] : in[p - h]; }
};

constexpr int MF_NB = 2;                        // column blocks of 16 groups per wave and tile: 512 outputs
constexpr int MF_TO = 256 * MF_NB;
constexpr int MF_MAXL = 256;                    // longest filter on the matrix cores (the window below stays within MF_MAXP samples per lane)
__host__ __device__ constexpr int mf_steps(int L) { return (2 * L + 30 + 3) / 4; }
__host__ __device__ constexpr int mf_wf(int L) { return 32 * (16 * MF_NB - 1) + 4 * mf_steps(L) + 4; }     // window floats read
__host__ __device__ constexpr int mf_ws(int L) { return (mf_wf(L) + 1) / 2; }                             // window samples staged
__host__ __device__ constexpr int mf_hz(int L) { return 4 * mf_steps(L) + 32; }                            // floats per padded tap row
constexpr int MF_MAXP = (mf_ws(MF_MAXL) + 63) / 64;
__host__ __device__ inline int swz(int a) { return a + 2 * (a >> 5); }     // two pad floats per 32: the 16 columns' B reads fall in 32 different banks
size_t mf_lds(int L) { return sizeof(float) * ((size_t)4 * mf_hz(L) + swz(2 * mf_ws(L)) + 8); }

typedef float f32x4_mfma __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(64) void k_bfsk_mfma(const float2 *__restrict__ in, size_t in_pitch, long long n_in, const float2 *__restrict__ hist, int hist_cap,
                                                  const RttyChan *__restrict__ st, float *__restrict__ out, size_t out_pitch, const float2 *__restrict__ mark, const float2 *__restrict__ space, int L,
                                                  int wpc, int tpw)
{
    extern __shared__ float lds_f[];
    const int S = mf_steps(L), HZ = mf_hz(L), WS = mf_ws(L);
    float *hz = lds_f;                          // 4 rows of HZ: 30 zeros, the 2 L interleaved taps, zeros
    float *xw = lds_f + 4 * HZ;                 // the window, swizzled
    const int ch = blockIdx.x / wpc, w = blockIdx.x % wpc, lane = threadIdx.x;
    const int h = st ? st[ch].hist_len : 0;
    const long long nV = h + n_in, n_out = nV - (L - 1);
    if (n_out <= 0) return;
    const long long tiles = (n_out + MF_TO - 1) / MF_TO, t0 = (long long)w * tpw, t1 = std::min(t0 + tpw, tiles);
    if (t0 >= t1) return;
    const VRow V{hist ? hist + (size_t)ch * hist_cap : nullptr, in + (size_t)ch * in_pitch, h};
    float2 nx[MF_MAXP];
    auto fetch = [&](long long tile) {
        const long long o0 = tile * MF_TO;
#pragma unroll
        for (int u = 0; u < MF_MAXP; u++) {
            const int p = 64 * u + lane;
            if (p < WS) nx[u] = o0 + p < nV ? V(o0 + p) : make_float2(0.f, 0.f);
        }
    };
    fetch(t0);
    for (int m = lane; m < 4 * HZ; m += 64) {
        const int c = m / HZ, j = m % HZ - 30;
        hz[m] = (j >= 0 && j < 2 * L) ? bfsk_tap(mark, space, c, j) : 0.f;
    }
    const int i = lane & 15, kk = lane >> 4, n = lane & 15;
    const float *ap = hz + 30 + kk - 2 * i;                       // + c HZ + 4 s
    const int bb = 34 * n + kk;                                    // + 34 * 16 b + 4 s + 2 (s >> 3)
    for (long long tile = t0; tile < t1; tile++) {
        __syncthreads();                                           // (the previous tile's reads are done)
#pragma unroll
        for (int u = 0; u < MF_MAXP; u++) {
            const int p = 64 * u + lane;
            if (p < WS) *reinterpret_cast<float2 *>(xw + swz(2 * p)) = nx[u];
        }
        __syncthreads();
        if (tile + 1 < t1) fetch(tile + 1);                        // in flight during the products
        f32x4_mfma acc[4][MF_NB];
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int b = 0; b < MF_NB; b++) acc[c][b] = (f32x4_mfma){0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < S; s++) {
            float a[4], bv[MF_NB];
#pragma unroll
            for (int c = 0; c < 4; c++) a[c] = ap[c * HZ + 4 * s];
            const int bo = bb + 4 * s + 2 * (s >> 3);
#pragma unroll
            for (int b = 0; b < MF_NB; b++) bv[b] = xw[bo + 544 * b];
#pragma unroll
            for (int b = 0; b < MF_NB; b++)
#pragma unroll
                for (int c = 0; c < 4; c++) acc[c][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], bv[b], acc[c][b], 0, 0, 0);
        }
        // C layout: column n = lane & 15 (group), row 4 (lane >> 4) + r (output within the group)
        const long long o0 = tile * MF_TO;
        float *orow = out + (size_t)ch * out_pitch;
#pragma unroll
        for (int b = 0; b < MF_NB; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const long long o = o0 + 16 * (16 * b + n) + 4 * kk + r;
                if (o < n_out) orow[o] = bfsk_power(acc[0][b][r], acc[1][b][r], acc[2][b][r], acc[3][b][r]);
            }
    }
}

// one thread per output: the same chains straight from global memory (any filter length)
__global__ __launch_bounds__(256) void k_bfsk_generic(const float2 *__restrict__ in, size_t in_pitch, long long n_in, const float2 *__restrict__ hist, int hist_cap,
                                                      const RttyChan *__restrict__ st, float *__restrict__ out, size_t out_pitch, const float2 *__restrict__ mark,
                                                      const float2 *__restrict__ space, int L, int bpc)
{
    const int ch = blockIdx.x / bpc;
    const long long o = (long long)(blockIdx.x % bpc) * 256 + threadIdx.x;
    const int h = st ? st[ch].hist_len : 0;
    const long long n_out = h + n_in - (L - 1);
    if (o >= n_out) return;
    const VRow V{hist ? hist + (size_t)ch * hist_cap : nullptr, in + (size_t)ch * in_pitch, h};
    out[(size_t)ch * out_pitch + o] = bfsk_output(mark, space, L, [&](int t) { return V(o + t); });
}

// after the discriminator: each channel's output count, and its new history (the last min(L - 1, h + n_in) samples of V)
__global__ __launch_bounds__(64) void k_bfsk_hist(const float2 *__restrict__ in, size_t in_pitch, long long n_in, float2 *__restrict__ hist, int hist_cap,
                                                  RttyChan *__restrict__ st, int n_ch, int L, int *__restrict__ counts)
{
    const int ch = blockIdx.x * 64 + threadIdx.x;
    if (ch >= n_ch) return;
    RttyChan s = st[ch];
    const long long nV = s.hist_len + n_in, n_out = nV - (L - 1);
    if (counts) counts[ch] = n_out > 0 ? (int)n_out : 0;
    const int h2 = (int)std::min((long long)(L - 1), nV);
    float2 *hr = hist + (size_t)ch * hist_cap;
    const float2 *x = in + (size_t)ch * in_pitch;
    const long long from = nV - h2;
    for (int j = 0; j < h2; j++) { const long long p = from + j; hr[j] = p < s.hist_len ? hr[p] : x[p - s.hist_len]; }     // forward: p >= j
    s.hist_len = h2;
    st[ch] = s;
}

// ---------------------------------------------------------------- the serial decoder and Baudot, one lane per channel
// k_rtty_walk: one wave per channel for the serial decoder.  The start-edge scan, where the walk spends most of its samples, takes 64 samples per
// step (coalesced loads and a ballot for the first edge: the sequential loop's answer); the bit sums and the index arithmetic are serial_window_with's,
// run identically by every lane (their loads are broadcasts); lane 0 writes the characters; the remainder is copied 64 samples per step.
struct WaveEdge {
    const float *rem; const float *in; long long R, p0;
    __device__ float v(long long p) const { return p < R ? rem[p] : in[p - R]; }
    __device__ int operator()(int off, int n) const
    {
        const int lane = threadIdx.x;
        for (int b = 1; b < n; b += 64) {
            const int i = b + lane;
            const bool hit = i < n && v(p0 + off + i) < 0 && v(p0 + off + i - 1) > 0;
            const unsigned long long m = __ballot(hit);
            if (m) return b + __ffsll((long long)m) - 1;
        }
        return -1;
    }
};

struct EmitLane0 {
    Emit e;
    __device__ void operator()(unsigned shr)
    {
        if (threadIdx.x == 0) { e(shr); return; }
        // the other lanes keep k and the shift state in step without writing
        if (e.c->last == RTTY_SERIAL) { e.k++; return; }
        if (rtty_baudot_lookup(e.fig, shr)) e.k++;
    }
};

__global__ __launch_bounds__(64) void k_rtty_walk(RttyCfg c, RttyChan *__restrict__ st, float *__restrict__ rem, int n_ch, const float *__restrict__ xin,
                                                       size_t xpitch, long long n_in, const int *__restrict__ cnt, void *__restrict__ out, size_t out_pitch,
                                                       int *__restrict__ counts)
{
    const int ch = blockIdx.x, lane = threadIdx.x;
    RttyChan s = st[ch];
    float *rm = rem + (size_t)ch * c.B;
    const float *x = xin + (size_t)ch * xpitch;
    const long long R = s.rem_len, n = cnt ? cnt[ch] : n_in, nV = R + n;
    EmitLane0 e{Emit{&c, (uint8_t *)out + (size_t)ch * out_pitch * rtty_out_elem(c), 0, &s.fig_mode}};
    long long pos = 0;
    while (nV - pos >= c.B) {
        const long long p0 = pos;
        const WaveEdge f{rm, x, R, p0};
        auto xv = [&](int p) { return f.v(p0 + p); };
        pos += serial_window_with(c, xv, c.B, e, f);
    }
    const int nt = (int)(nV - pos);
    for (int j0 = 0; j0 < nt; j0 += 64) {                           // forward in steps of 64: a step reads at >= its own writes' indices, past every earlier step's
        const int j = j0 + lane;
        const float v = j < nt ? (pos + j < R ? rm[pos + j] : x[pos + j - R]) : 0.f;
        if (j < nt) rm[j] = v;
    }
    if (lane == 0) {
        s.rem_len = nt;
        st[ch] = s;
        counts[ch] = (int)e.e.k;
    }
}

// k_rtty_baudot: rtty_baudot2ascii_u8_u8 alone (first == BAUDOT), one lane per channel over its bytes
__global__ __launch_bounds__(64) void k_rtty_baudot(RttyCfg c, RttyChan *__restrict__ st, int n_ch, const uint8_t *__restrict__ xin, size_t xpitch, long long n_in,
                                                    uint8_t *__restrict__ out, size_t out_pitch, int *__restrict__ counts)
{
    const int ch = blockIdx.x * 64 + threadIdx.x;
    if (ch >= n_ch) return;
    RttyChan s = st[ch];
    Emit e{&c, out + (size_t)ch * out_pitch, 0, &s.fig_mode};
    const uint8_t *x = xin + (size_t)ch * xpitch;
    for (long long j = 0; j < n_in; j++) e(x[j]);
    st[ch] = s;
    counts[ch] = (int)e.k;
}

__global__ void k_binary_slicer(const float *__restrict__ in, uint8_t *__restrict__ out, long long n, size_t in_pitch, size_t out_pitch)
{
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const size_t s = blockIdx.y;
    out[s * out_pitch + j] = in[s * in_pitch + j] > 0;
}

__global__ __launch_bounds__(64) void k_rtty_line(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, int n_streams, long long n, size_t in_pitch,
                                                  size_t out_pitch, RttyPush *__restrict__ state, int *__restrict__ counts)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_streams) return;
    RttyPush p = state[s];
    const uint8_t *x = in + (size_t)s * in_pitch;
    uint8_t *o = out + (size_t)s * out_pitch;
    int k = 0;
    for (long long j = 0; j < n; j++) { const uint8_t ch = rtty_baudot_push(&p, x[j]); if (ch) o[k++] = ch; }
    state[s] = p;
    counts[s] = k;
}

// serial_line_decoder_f_u8 as the library call: one window of n samples per stream; used[s] = input_used
__global__ __launch_bounds__(64) void k_serial_window(RttyCfg c, const float *__restrict__ in, int n_streams, int n, size_t in_pitch, void *__restrict__ out,
                                                      size_t out_pitch, int *__restrict__ counts, int *__restrict__ used)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_streams) return;
    const float *x = in + (size_t)s * in_pitch;
    int fig = 0;
    Emit e{&c, (uint8_t *)out + (size_t)s * out_pitch * rtty_out_elem(c), 0, &fig};
    used[s] = n > 0 ? serial_window(c, [&](int p) { return x[p]; }, n, e) : 0;
    counts[s] = (int)e.k;
}

const char *g_bfsk_last = "";          // the kernel behind the last csdr_amd_bfsk_demod_cf call

RttyChan fresh_chan() { RttyChan s; memset(&s, 0, sizeof s); return s; }

// csdr.c:3286-3287: mark at +spacing/2, space at -spacing/2, Hamming, normalised; ms = mark (L) then space (L)
void bfsk_taps(const csdr_amd_rtty_params *p, std::vector<float2> &ms)
{
    const int L = p->filter_length;
    ms.assign((size_t)2 * L, make_float2(0.f, 0.f));
    csdr_amd_firdes_peak_c((csdr_complexf *)ms.data(), L, p->spacing / 2, CSDR_WINDOW_HAMMING);
    csdr_amd_firdes_peak_c((csdr_complexf *)ms.data() + L, L, -p->spacing / 2, CSDR_WINDOW_HAMMING);
}

// the discriminator over n_ch rows: k_bfsk_mfma where the filter fits, else k_bfsk_generic; returns the kernel's name
const char *launch_bfsk(hipStream_t stream, bool generic, const float2 *in, size_t in_pitch, long long n_in, const float2 *hist, int hist_cap, const RttyChan *st,
                        float *out, size_t out_pitch, const float2 *mark, const float2 *space, int L, int n_ch)
{
    if (n_in <= 0) return "";
    if (!generic && L <= MF_MAXL) {
        const long long tiles = (n_in + MF_TO - 1) / MF_TO;       // (at most: a channel has n_in + h - L + 1 <= n_in outputs)
        const int tpw = (int)std::max(1LL, std::min(16LL, tiles * n_ch / (256 * 32)));
        const int wpc = (int)((tiles + tpw - 1) / tpw);
        hipLaunchKernelGGL(k_bfsk_mfma, dim3((unsigned)((size_t)wpc * n_ch)), dim3(64), mf_lds(L), stream, in, in_pitch, n_in, hist, hist_cap, st, out, out_pitch,
                           mark, space, L, wpc, tpw);
        return "k_bfsk_mfma";
    }
    const int bpc = (int)((n_in + 255) / 256);
    hipLaunchKernelGGL(k_bfsk_generic, dim3((unsigned)((size_t)bpc * n_ch)), dim3(256), 0, stream, in, in_pitch, n_in, hist, hist_cap, st, out, out_pitch, mark, space, L, bpc);
    return "k_bfsk_generic";
}

} // namespace

struct csdr_amd_rtty : ChanBank<RttyChan> {
    RttyCfg cfg; int hist_cap, cus; size_t mid_cap = 0;
    DevBuf<float2> d_hist; DevBuf<float> d_rem, d_mid; DevBuf<float2> d_taps; DevBuf<int> d_mid_cnt;
};

extern "C" {

csdr_amd_rtty *csdr_amd_rtty_create(csdr_amd_ctx *c, const csdr_amd_rtty_params *params, int n_channels, int first_stage, int last_stage)
{
    RttyCfg cfg;
    if (bank_create_check("rtty", c, n_channels) < 0 || make_cfg(params, first_stage, last_stage, &cfg) < 0) return nullptr;
    Owned<csdr_amd_rtty, csdr_amd_rtty_destroy> p(new csdr_amd_rtty());
    p->c = c; p->cfg = cfg; p->n_ch = n_channels;
    p->cus = current_device_cu_count();
    const bool bfsk = first_stage == RTTY_BFSK, serial = first_stage <= RTTY_SERIAL && last_stage >= RTTY_SERIAL;
    p->hist_cap = bfsk ? std::max(1, cfg.L - 1) : 1;
    if (dev_alloc(p->d_st, sizeof(RttyChan) * n_channels) != hipSuccess ||
        (bfsk && dev_alloc(p->d_hist, sizeof(float2) * (size_t)p->hist_cap * n_channels) != hipSuccess) ||
        (bfsk && dev_alloc(p->d_taps, sizeof(float2) * 2 * (size_t)cfg.L) != hipSuccess) ||
        (serial && dev_alloc(p->d_rem, sizeof(float) * (size_t)cfg.B * n_channels) != hipSuccess) ||
        dev_alloc(p->d_mid_cnt, sizeof(int) * n_channels) != hipSuccess) { fail_msg(-2, "rtty: out of device memory"); return nullptr; }
    if (bfsk) {
        std::vector<float2> ms;
        bfsk_taps(params, ms);
        if (csdr_amd_h2d(c, p->d_taps.get(), ms.data(), sizeof(float2) * ms.size()) < 0) return nullptr;
    }
    if (csdr_amd_rtty_reset(p.get()) < 0) return nullptr;
    return p.release();
}

int csdr_amd_rtty_reset(csdr_amd_rtty *p) { const RttyChan s = fresh_chan(); return bank_reset(p, "rtty", &s); }
int csdr_amd_rtty_reset_channel(csdr_amd_rtty *p, int ch) { return bank_reset_channel(p, "rtty", ch, fresh_chan()); }

long long csdr_amd_rtty_max_out(const csdr_amd_rtty *p, long long n_in)
{
    if (!p || n_in < 0) return 0;
    const RttyCfg &c = p->cfg;
    if (c.last == RTTY_BFSK || c.first == RTTY_BAUDOT) return n_in;
    // every character moves the window on by at least floor(spb * all_bits) >= 3 samples; the walk sees at most B - 1 + n_in of them
    const long long step = std::max(1LL, (long long)(c.spb * c.all_bits));
    return (n_in + c.B) / step + 1;
}

int csdr_amd_rtty_process(csdr_amd_rtty *p, const void *in, long long n_in, size_t in_pitch, void *out, size_t out_pitch, int *counts)
{
    if (!p) return fail_msg(-3, "rtty: null object");
    if (n_in < 0 || n_in > (1LL << 30) || (n_in > 0 && (!in || in_pitch < (size_t)n_in))) return fail_msg(-3, "rtty: need in_pitch >= n_in >= 0 (n_in <= 2^30)");
    if (!counts) return fail_msg(-3, "rtty: counts is required");
    const long long mo = csdr_amd_rtty_max_out(p, n_in);
    if (mo > 0 && (!out || out_pitch < (size_t)mo)) return fail_msg(-3, "rtty: out_pitch %zu below max_out %lld", out_pitch, mo);
    csdr_amd_ctx *c = p->c;
    const RttyCfg &cfg = p->cfg;
    const void *xin = in; size_t xpitch = in_pitch; const int *cnt = nullptr;
    if (cfg.first == RTTY_BFSK) {
        float *dst = (float *)out; size_t dpitch = out_pitch;
        if (cfg.last > RTTY_BFSK) {                                    // the discriminator rows go to the object's own buffer
            const size_t mp = (size_t)std::max(1LL, n_in), need = mp * p->n_ch;
            if (need > p->mid_cap) {
                if (csdr_amd_ctx_sync(c) < 0) return -5;
                p->d_mid.reset();
                if (dev_alloc(p->d_mid, sizeof(float) * need) != hipSuccess) { p->mid_cap = 0; return fail_msg(-2, "rtty: out of device memory"); }
                p->mid_cap = need;
            }
            dst = p->d_mid.get(); dpitch = mp;
            xin = dst; xpitch = dpitch; cnt = p->d_mid_cnt.get();
        }
        p->last_kernel = launch_bfsk(c->stream, p->force_generic, (const float2 *)in, in_pitch, n_in, p->d_hist.get(), p->hist_cap, p->d_st.get(), dst, dpitch,
                                     p->d_taps.get(), p->d_taps.get() + cfg.L, cfg.L, p->n_ch);
        if (!*p->last_kernel) p->last_kernel = p->force_generic || cfg.L > MF_MAXL ? "k_bfsk_generic" : "k_bfsk_mfma";
        hipLaunchKernelGGL(k_bfsk_hist, dim3(cdiv(p->n_ch, 64)), dim3(64), 0, c->stream, (const float2 *)in, in_pitch, n_in, p->d_hist.get(), p->hist_cap,
                           p->d_st.get(), p->n_ch, cfg.L, cfg.last == RTTY_BFSK ? counts : p->d_mid_cnt.get());
        CSDR_LAUNCH_CHECK();
        if (cfg.last == RTTY_BFSK) return 0;
    }
    if (cfg.first == RTTY_BAUDOT) {                                 // a byte per lane and channel: one lane per channel
        hipLaunchKernelGGL(k_rtty_baudot, dim3(cdiv(p->n_ch, 64)), dim3(64), 0, c->stream, cfg, p->d_st.get(), p->n_ch, (const uint8_t *)xin, xpitch, n_in,
                           (uint8_t *)out, out_pitch, counts);
    } else {
        hipLaunchKernelGGL(k_rtty_walk, dim3(p->n_ch), dim3(64), 0, c->stream, cfg, p->d_st.get(), p->d_rem.get(), p->n_ch, (const float *)xin, xpitch,
                           n_in, cnt, out, out_pitch, counts);
    }
    if (cfg.first != RTTY_BFSK) p->last_kernel = cfg.first == RTTY_BAUDOT ? "k_rtty_baudot" : "k_rtty_walk";
    CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_rtty_force_generic(csdr_amd_rtty *p, int on) { return bank_force_generic(p, "rtty", on); }
const char *csdr_amd_rtty_kernel_name(const csdr_amd_rtty *p) { return bank_kernel_name(p); }

void csdr_amd_rtty_destroy(csdr_amd_rtty *p) { destroy_on_stream(p); }

// bfsk_demod_cf libcsdr.c:2335-2350 with caller taps (device) on n_streams independent streams: n - L + 1 outputs each
int csdr_amd_bfsk_demod_cf(csdr_amd_ctx *c, const csdr_complexf *in, float *out, int n_streams, long long n, size_t in_pitch, size_t out_pitch,
                           const csdr_complexf *mark_filter, const csdr_complexf *space_filter, int taps_length, int force_generic)
{
    if (!c || n_streams < 1 || !mark_filter || !space_filter || taps_length < 1 || taps_length > 65536) return fail_msg(-3, "bfsk_demod_cf: bad arguments");
    if (n < 0 || n > (1LL << 30) || (n > 0 && (!in || in_pitch < (size_t)n))) return fail_msg(-3, "bfsk_demod_cf: need in_pitch >= n >= 0");
    const long long no = n - taps_length + 1;
    if (no <= 0) return 0;
    if (!out || out_pitch < (size_t)no) return fail_msg(-3, "bfsk_demod_cf: out_pitch below n - taps_length + 1");
    g_bfsk_last = launch_bfsk(c->stream, force_generic != 0, (const float2 *)in, in_pitch, n, nullptr, 1, nullptr, out, out_pitch, (const float2 *)mark_filter,
                              (const float2 *)space_filter, taps_length, n_streams);
    CSDR_LAUNCH_CHECK();
    return 0;
}

const char *csdr_amd_bfsk_last_kernel(void) { return g_bfsk_last; }

int csdr_amd_binary_slicer_f_u8(csdr_amd_ctx *c, const float *in, uint8_t *out, int n_streams, long long n, size_t in_pitch, size_t out_pitch)
{
    if (!c || n_streams < 1 || n_streams > 65535 || n < 0 || (n > 0 && (!in || !out || in_pitch < (size_t)n || out_pitch < (size_t)n))) return fail_msg(-3, "binary_slicer_f_u8: bad arguments");
    if (!n) return 0;
    hipLaunchKernelGGL(k_binary_slicer, dim3(cdiv(n, 256), n_streams), dim3(256), 0, c->stream, in, out, n, in_pitch, out_pitch);
    CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_rtty_line_decoder_u8_u8(csdr_amd_ctx *c, const uint8_t *in, uint8_t *out, int n_streams, long long n, size_t in_pitch, size_t out_pitch,
                                     csdr_amd_rtty_push_state *state, int *counts)
{
    if (!c || n_streams < 1 || !state || !counts || n < 0 || (n > 0 && (!in || !out || in_pitch < (size_t)n || out_pitch < (size_t)n))) return fail_msg(-3, "rtty_line_decoder_u8_u8: bad arguments");
    static_assert(sizeof(RttyPush) == sizeof(csdr_amd_rtty_push_state), "RttyPush mirrors csdr_amd_rtty_push_state");
    hipLaunchKernelGGL(k_rtty_line, dim3(cdiv(n_streams, 64)), dim3(64), 0, c->stream, in, out, n_streams, n, in_pitch, out_pitch, (RttyPush *)state, counts);
    CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_serial_line_decoder_f_u8(csdr_amd_ctx *c, const float *in, void *out, int n_streams, int n, size_t in_pitch, size_t out_pitch,
                                      float samples_per_bits, int databits, float stopbits, float bit_sampling_width_ratio, int *counts, int *used)
{
    if (!c || n_streams < 1 || !counts || !used || n < 0 || (n > 0 && (!in || !out || in_pitch < (size_t)n || out_pitch < (size_t)n)))
        return fail_msg(-3, "serial_line_decoder_f_u8: bad arguments");
    if (databits < 1 || databits > 32) return fail_msg(-3, "serial_line_decoder_f_u8: databits should be 1 .. 32");
    RttyCfg cfg; memset(&cfg, 0, sizeof cfg);
    cfg.spb = samples_per_bits; cfg.databits = databits; cfg.stopbits = stopbits; cfg.ratio = bit_sampling_width_ratio; cfg.B = n;
    cfg.all_bits = (float)(1 + databits) + stopbits; cfg.first = cfg.last = RTTY_SERIAL;
    hipLaunchKernelGGL(k_serial_window, dim3(cdiv(n_streams, 64)), dim3(64), 0, c->stream, cfg, in, n_streams, n, in_pitch, out, out_pitch, counts, used);
    CSDR_LAUNCH_CHECK();
    return 0;
}

char csdr_amd_rtty_baudot_decoder_lookup(unsigned char *fig_mode, unsigned char c)
{
    int f = *fig_mode;
    const char r = (char)rtty_baudot_lookup(&f, c);
    *fig_mode = (unsigned char)f;
    return r;
}

char csdr_amd_rtty_baudot_decoder_push(csdr_amd_rtty_push_state *s, unsigned char symbol) { return (char)rtty_baudot_push((RttyPush *)s, symbol); }

// CPU run of the object's walk for one channel, the stream cut into calls of cuts[0], cuts[1], ... items (the rest of n in one more call); outputs
// concatenated.  Returns the output count.
long long csdr_amd_debug_rtty_walk(const csdr_amd_rtty_params *params, int first_stage, int last_stage, const void *in, long long n, const long long *cuts,
                                   int n_cuts, void *out)
{
    RttyCfg cfg;
    if (make_cfg(params, first_stage, last_stage, &cfg) < 0) return -3;
    if (n < 0 || (n > 0 && (!in || !out)) || n_cuts < 0 || (n_cuts && !cuts)) return fail_msg(-3, "debug_rtty_walk: bad arguments");
    RttyChan s = fresh_chan();
    std::vector<float> rem(cfg.B > 0 ? cfg.B : 1), mid;
    std::vector<float2> hist(std::max(1, cfg.L)), ms;
    if (first_stage == RTTY_BFSK) bfsk_taps(params, ms);
    const size_t isz = first_stage == RTTY_BFSK ? 8 : first_stage == RTTY_SERIAL ? 4 : 1, osz = rtty_out_elem(cfg);
    long long k = 0;
    for_each_call(n, cuts, n_cuts, [&](long long done, long long m) {
        const char *x = (const char *)in + done * isz;
        uint8_t *o = (uint8_t *)out + k * osz;
        const float *xf = (const float *)x;
        long long nx = m;
        if (first_stage == RTTY_BFSK) {
            const float2 *xc = (const float2 *)x;
            const int h = s.hist_len;
            const long long nV = h + m, no = std::max(0LL, nV - (cfg.L - 1));
            auto V = [&](long long p) { return p < h ? hist[p] : xc[p - h]; };
            float *dst = last_stage == RTTY_BFSK ? (float *)o : (mid.resize(std::max(1LL, no)), mid.data());
            for (long long j = 0; j < no; j++) dst[j] = bfsk_output(ms.data(), ms.data() + cfg.L, cfg.L, [&](int t) { return V(j + t); });
            const int h2 = (int)std::min((long long)(cfg.L - 1), nV);
            for (int j = 0; j < h2; j++) { const long long p = nV - h2 + j; hist[j] = V(p); }
            s.hist_len = h2;
            if (last_stage == RTTY_BFSK) { k += no; return; }
            xf = dst; nx = no;
        }
        Emit e{&cfg, o, 0, &s.fig_mode};
        if (first_stage == RTTY_BAUDOT) for (long long j = 0; j < m; j++) e(((const uint8_t *)x)[j]);
        else { auto r = [&](long long q) { return xf[q]; }; serial_walk(cfg, s, rem.data(), r, nx, e); }
        k += e.k;
    });
    return k;
}

} // extern "C"
