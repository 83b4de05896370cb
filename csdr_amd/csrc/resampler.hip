// resampler.hip -- rational_resampler_ff (libcsdr.c:607-640) and fir_interpolate_cc (libcsdr.c:579-605) for n_streams streams per call (MI355X / gfx950).
//
// Both objects keep, per stream, the last H input samples on the device.  A call's kernels read the virtual buffer V = history[H] ++ new input[n_in]; the
// history then moves on by n_in (double-buffered: the old one is read while the new one is written).
//
// rational_resampler_ff.  Output o reads input[s_o ..] against taps[d_o + i I], i < K(d_o) = (T - d_o) / I.  From any output on, with x_j = j D - d_0:
//   s_j = s_0 + ceil(x_j / I),  d_j = (s_j - s_0) I - x_j                                                               (rr_step)
// which is the reference's startingi / delayi (libcsdr.c:621-623) with last_taps_delay = d_0.  The phases repeat every P = I / g outputs (g = gcd(I, D)) and each
// period advances the input by Dg = D / g.  A call's outputs are a list of segments {s in V, d_0, first output, count}: one per call while streaming, one per
// window of the reference's CLI loop (csdr.c:1441-1459) in the cli_bufsize mode.
//
// k_rr_poly: one workgroup per tile of P x M outputs of one segment.  The tile's input is staged once into LDS in the polyphase layout x[n] -> row n mod Dg,
// column n / Dg, so that output j = p + P m (local phase p, period m) reads row (s_p + i) mod Dg, column (s_p + i) / Dg + m.  A wave takes one phase and 64
// consecutive m: its taps are wave-uniform and its lanes read 64 consecutive LDS words.  The LDS offsets of the samples and the phase's taps come from host
// tables by scalar loads, so the tap loop does no index arithmetic.  The results go through LDS and leave as one contiguous run.
// k_rr_generic: one thread per output, straight from global memory -- shapes whose tile does not fit.  Both kernels sum one output as
// acc = fmaf(x[s + i], tap[d + i I], acc) over i ascending, then acc * I: the same bits whichever kernel runs and however the stream is cut into calls.
//
// fir_interpolate_cc.  Input position i gives the I outputs out[i I + ip] = sum_k x[i + k] taps[(k + 1) I - ip], (k + 1) I - ip < T; position i is computed once
// i I + I - 1 + T <= total I.  k_interp_poly: one thread per position, the positions' input staged in LDS, the phases in wave-uniform chunks of IC (taps are
// scalar loads); each chunk's outputs are staged through LDS and written row by row, so consecutive lanes store consecutive complex values (for I <= 8 the
// tile's output is one contiguous run).  k_interp_generic: one thread per output.  Same summation order (k ascending, fmaf per component) in both.
#include "bank.hpp"
#include <math.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <vector>

using namespace csdr_amd;

namespace {

struct RrSeg { int s, d0, out0, count; };

constexpr int RR_LDS_BUDGET = 80 * 1024;         // two workgroups per CU (160 KiB)
constexpr int RR_MAX_M = 1024;
constexpr int RR_STAGE = 8;                      // k_rr_poly: staging loads in flight per lane
constexpr int RR_THREADS = 512;                  // k_rr_poly: 8 waves per workgroup, two workgroups per CU at the LDS budget: 4 waves per SIMD
constexpr int IP_LDS_BUDGET = 64 * 1024;

__host__ __device__ inline void rr_step(long long j, int I, int D, int d0, long long *ds, int *d)
{
    const long long x = j * (long long)D - d0;             // >= -d0 > -I
    const long long c = (x + I - 1) / I;
    *ds = c; *d = (int)(c * I - x);
}
__host__ __device__ inline int rr_taps(int T, int I, int d) { return T > d ? (T - d) / I : 0; }     // libcsdr.c:626 (0 when T - d < I)
inline int interp_taps(int T, int I, int ip) { const int a = T - (I - ip); return a > 0 ? (a + I - 1) / I : 0; }   // k with (k + 1) I - ip < T

template <class E> __device__ __forceinline__ E vload(const E *hist, int H, const E *in, long long v, long long n_in)
{
    if (v < H) return hist[v];
    v -= H;
    if (v < n_in) return in[v];
    E z; memset(&z, 0, sizeof(E)); return z;
}

__global__ __launch_bounds__(256) void k_rr_generic(const float *__restrict__ hist, int H, size_t hist_pitch, const float *__restrict__ in, size_t in_pitch, long long n_in,
                                                    float *__restrict__ out, size_t out_pitch, const RrSeg *__restrict__ segs, int n_segs, int n_out,
                                                    int I, int D, int T, const float *__restrict__ taps)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_out) return;
    int a = 0, b = n_segs - 1;                                           // the last segment whose first output is <= k
    while (a < b) { const int m = (a + b + 1) >> 1; if (segs[m].out0 <= k) a = m; else b = m - 1; }
    const RrSeg g = segs[a];
    long long ds; int d; rr_step(k - g.out0, I, D, g.d0, &ds, &d);
    const long long s = g.s + ds;
    const int K = rr_taps(T, I, d);
    const float *hs = hist + blockIdx.y * hist_pitch, *xs = in + blockIdx.y * in_pitch;
    float acc = 0.f;
    for (int i = 0; i < K; i++) acc = __fmaf_rn(vload(hs, H, xs, s + i, n_in), taps[d + i * I], acc);
    out[blockIdx.y * out_pitch + k] = acc * (float)I;
}

// tiles: segments cut into runs of at most P*M outputs (each starts on a period boundary of its segment).  LDS: xs[Dg][Cp], ys[P*M], then the phase table.
// offt[t] = (t mod Dg) Cp + t / Dg: where tile-relative sample t lives in xs (host table, so the tap loop does no index arithmetic of its own);
// tpm: the taps phase-major, row d = taps[d + i I], zero-padded to Kpad.  Both tables are padded so that the next group of 8 can always be loaded ahead.
__global__ __launch_bounds__(RR_THREADS) void k_rr_poly(const float *__restrict__ hist, int H, size_t hist_pitch, const float *__restrict__ in, size_t in_pitch,
                                                        long long n_in, float *__restrict__ out, size_t out_pitch, const RrSeg *__restrict__ tiles,
                                                        int I, int D, int T, int P, int Dg, int M, int Cp, const float *__restrict__ tpm, int Kpad,
                                                        const int *__restrict__ offt)
{
    extern __shared__ float lds[];
    float *xs = lds, *ys = lds + (size_t)Dg * Cp;
    const RrSeg tl = tiles[blockIdx.x];
    const float *hs = hist + blockIdx.y * hist_pitch, *xin = in + blockIdx.y * in_pitch;
    const int S = Dg * Cp;
    const float inv = 1.0f / (float)Dg;
    for (int n0 = threadIdx.x; n0 < S; n0 += RR_THREADS * RR_STAGE) {   // RR_STAGE loads in flight per lane, then their LDS stores
        float v[RR_STAGE];
#pragma unroll
        for (int u = 0; u < RR_STAGE; u++) { const int n = n0 + u * RR_THREADS; v[u] = n < S ? vload(hs, H, xin, (long long)tl.s + n, n_in) : 0.f; }
#pragma unroll
        for (int u = 0; u < RR_STAGE; u++) {
            const int n = n0 + u * RR_THREADS;
            if (n >= S) break;
            int q = (int)((float)n * inv), r = n - q * Dg;              // n / Dg, n % Dg (n < 2^24: off by at most one before the fix-up)
            if (r < 0) { q--; r += Dg; } else if (r >= Dg) { q++; r -= Dg; }
            xs[r * Cp + q] = v[u];
        }
    }
    int2 *ph = (int2 *)(lds + (((size_t)Dg * Cp + (size_t)P * M + 1) & ~(size_t)1));   // (8-byte aligned)                           // per phase of the tile: (first sample, tap phase), one division each, on the vector unit
    for (int p = threadIdx.x; p < P; p += RR_THREADS) { const int x = p * D - tl.d0, ds = (x + I - 1) / I; ph[p] = make_int2(ds, ds * I - x); }   // rr_step
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int G = M >> 6;                                                // items: (phase p, group of 64 periods), P G of them over the waves
    int p = wave % P, g = wave / P;
    for (; g < G; ) {
        const int m = g * 64 + lane;
        const int2 pd = ph[p];
        const int ds = __builtin_amdgcn_readfirstlane(pd.x), d = __builtin_amdgcn_readfirstlane(pd.y);
        const int K = rr_taps(T, I, d);
        const int *ot = offt + ds;
        const float *tp = tpm + (size_t)d * Kpad;
        const float *xm = xs + m;
        float acc = 0.f;
        int on[8]; float tn[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { on[u] = ot[u]; tn[u] = tp[u]; }
        int i = 0;
        for (; i + 8 <= K; i += 8) {                                     // this group's 8 samples from LDS while the next group's offsets and taps load
            int o[8]; float t[8], xv[8];
#pragma unroll
            for (int u = 0; u < 8; u++) { o[u] = on[u]; t[u] = tn[u]; }
#pragma unroll
            for (int u = 0; u < 8; u++) { on[u] = ot[i + 8 + u]; tn[u] = tp[i + 8 + u]; }
#pragma unroll
            for (int u = 0; u < 8; u++) xv[u] = xm[o[u]];
#pragma unroll
            for (int u = 0; u < 8; u++) acc = __fmaf_rn(xv[u], t[u], acc);
        }
        for (; i < K; i++) acc = __fmaf_rn(xm[ot[i]], tp[i], acc);
        const int j = p + P * m;
        if (j < tl.count) ys[j] = acc * (float)I;
        for (p += RR_THREADS / 64; p >= P; p -= P) g++;                  // next item of this wave, without a division
    }
    __syncthreads();
    float *o = out + blockIdx.y * out_pitch + tl.out0;
    for (int j = threadIdx.x; j < tl.count; j += RR_THREADS) o[j] = ys[j];
}

__global__ __launch_bounds__(256) void k_interp_generic(const float2 *__restrict__ hist, int H, size_t hist_pitch, const float2 *__restrict__ in, size_t in_pitch,
                                                        long long n_in, float2 *__restrict__ out, size_t out_pitch, int pos0, int n_pos, int I, int T,
                                                        const float *__restrict__ taps)
{
    const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= (long long)n_pos * I) return;
    const int p = (int)(o / I), ip = (int)(o - (long long)p * I);
    const float2 *hs = hist + blockIdx.y * hist_pitch, *xs = in + blockIdx.y * in_pitch;
    float ai = 0.f, aq = 0.f;
    for (int k = 0; (k + 1) * I - ip < T; k++) {
        const float2 x = vload(hs, H, xs, (long long)pos0 + p + k, n_in);
        const float t = taps[(k + 1) * I - ip];
        ai = __fmaf_rn(x.x, t, ai); aq = __fmaf_rn(x.y, t, aq);
    }
    out[blockIdx.y * out_pitch + o] = make_float2(ai, aq);
}

template <int IC>
__global__ __launch_bounds__(256) void k_interp_poly(const float2 *__restrict__ hist, int H, size_t hist_pitch, const float2 *__restrict__ in, size_t in_pitch,
                                                     long long n_in, float2 *__restrict__ out, size_t out_pitch, int pos0, int n_pos, int I, int T, int Kmax,
                                                     const float *__restrict__ taps)
{
    extern __shared__ float2 xl[];                                      // [256 + Kmax] input, then [256 * IC] outputs of one phase chunk
    float2 *yl = xl + 256 + Kmax;
    const int t0 = blockIdx.x * 256;
    const float2 *hs = hist + blockIdx.y * hist_pitch, *xs = in + blockIdx.y * in_pitch;
    for (int n = threadIdx.x; n < 256 + Kmax; n += 256) xl[n] = vload(hs, H, xs, (long long)pos0 + t0 + n, n_in);
    __syncthreads();
    const int np = min(256, n_pos - t0);                                 // positions of this tile
    float2 *o = out + blockIdx.y * out_pitch + (size_t)t0 * I;
    for (int c0 = 0; c0 < I; c0 += IC) {
        const int icn = min(IC, I - c0);
        float ai[IC], aq[IC];
#pragma unroll
        for (int c = 0; c < IC; c++) { ai[c] = 0.f; aq[c] = 0.f; }
        for (int k = 0; k < Kmax; k++) {
            const float2 x = xl[threadIdx.x + k];
#pragma unroll
            for (int c = 0; c < IC; c++) {
                const int ti = (k + 1) * I - (c0 + c);
                if (c0 + c < I && ti < T) { const float t = taps[ti]; ai[c] = __fmaf_rn(x.x, t, ai[c]); aq[c] = __fmaf_rn(x.y, t, aq[c]); }
            }
        }
#pragma unroll
        for (int c = 0; c < IC; c++) if (c < icn) yl[threadIdx.x * icn + c] = make_float2(ai[c], aq[c]);
        __syncthreads();
        // the chunk's outputs leave row by row: icn == I (every I <= 8) makes the tile's whole output one contiguous run
        for (int e = threadIdx.x; e < np * icn; e += 256) { const int q = e / icn; o[(size_t)q * I + c0 + (e - q * icn)] = yl[e]; }
        __syncthreads();
    }
}

// new history = the last H elements of old history ++ in[n_in]
template <class E>
__global__ __launch_bounds__(256) void k_rs_hist(const E *__restrict__ hist, E *__restrict__ hist_new, int H, size_t hist_pitch, const E *__restrict__ in, size_t in_pitch, long long n_in)
{
    const E *hs = hist + blockIdx.y * hist_pitch, *xs = in + blockIdx.y * in_pitch;
    E *hn = hist_new + blockIdx.y * hist_pitch;
    for (int k = blockIdx.x * 256 + threadIdx.x; k < H; k += gridDim.x * 256) hn[k] = vload(hs, H, xs, n_in + k, n_in);
}

template <class E> int hist_advance(csdr_amd_ctx *c, const E *hist, E *hist_new, int H, size_t hist_pitch, const E *in, size_t in_pitch, long long n_in, int n_streams)
{
    unsigned gx = cdiv(H, 256); if (gx > 64) gx = 64;
    hipLaunchKernelGGL(k_rs_hist<E>, dim3(gx, n_streams), dim3(256), 0, c->stream, hist, hist_new, H, hist_pitch, in, in_pitch, n_in);
    CSDR_LAUNCH_CHECK();
    return 0;
}

int upload_table(csdr_amd_ctx *c, DevBuf<RrSeg> &buf, int &cap, const std::vector<RrSeg> &t)
{
    if ((int)t.size() > cap) {
        CSDR_HIP(hipStreamSynchronize(c->stream));                       // an earlier launch may still read the old table
        cap = (int)t.size() + t.size() / 2 + 16;
        CSDR_HIP(dev_alloc(buf, sizeof(RrSeg) * cap));
    }
    void *h = c->pinned_acquire(sizeof(RrSeg) * t.size());
    if (!h) return fail_msg(-2, "resampler: pinned staging failed");
    memcpy(h, t.data(), sizeof(RrSeg) * t.size());
    return c->pinned_upload(buf.get(), sizeof(RrSeg) * t.size());
}

} // namespace

struct csdr_amd_resampler : Bank {                        // (n_ch: the streams)
    int I, D, T, P, Dg, H, cli_bufsize = 0;
    int M, Cp; size_t lds;                                                // k_rr_poly's tile (M = 0: the shape runs on k_rr_generic)
    long long total;                                                      // input samples per stream seen since the last reset
    long long s_next; int d_next;                                         // streaming: the next output (absolute input index, tap phase)
    long long emitted;                                                    // streaming: outputs per stream since the last reset
    long long win_a; int win_L;                                           // cli_bufsize mode: the next window's first input sample, last_taps_delay
    int cli_pmin;                                                         // cli_bufsize mode: the fewest samples a window moves on by
    int Kpad; int cur; DevBuf<float> d_hist[2], d_taps, d_tpm; DevBuf<int> d_offt; DevBuf<RrSeg> d_tab; int tab_cap;
};

struct csdr_amd_interp : Bank {                           // (n_ch: the streams)
    int I, T, H, Kmax, cli_bufsize = 0;
    long long total, pos_next;
    int cur; DevBuf<float2> d_hist[2]; DevBuf<float> d_taps;
};

namespace {

int rr_alloc_hist(csdr_amd_resampler *r)
{
    const int need = std::max({r->T / r->I + 2, r->D / r->I + 3, r->cli_bufsize}) + 2;      // (a capped output waits up to D/I + 1 samples back)
    r->H = (need + 3) & ~3;
    for (auto &h : r->d_hist) CSDR_HIP(dev_alloc(h, sizeof(float) * (size_t)r->H * r->n_ch + 256));
    return 0;
}

int ip_alloc_hist(csdr_amd_interp *p)
{
    const int need = p->T / p->I + 3 + p->cli_bufsize;
    p->H = (need + 3) & ~3;
    for (auto &h : p->d_hist) CSDR_HIP(dev_alloc(h, sizeof(float2) * (size_t)p->H * p->n_ch + 256));
    return 0;
}

// one call of the reference function over a window of B samples with last_taps_delay L: outputs, input_processed, the returned last_taps_delay
void rr_window(int I, int D, int T, int B, int L, int *count, int *processed, int *L_out)
{
    const int cap = (int)((long long)B * I / D);
    const long long lb = (long long)B - T / I - 1;
    const long long brk = lb >= 0 ? (lb * I + L) / D + 1 : 0;
    long long ds = 0; int d = L;
    if (brk < cap) { *count = (int)brk; rr_step(brk, I, D, L, &ds, &d); }      // break exit: the first output that does not fit
    else if (cap > 0) { *count = cap; rr_step(cap - 1, I, D, L, &ds, &d); }   // cap exit: the last computed output's state
    else *count = 0;
    *processed = (int)ds; *L_out = d;
}

} // namespace

extern "C" {

void csdr_amd_rational_resampler_get_lowpass_f(float *output, int output_size, int interpolation, int decimation, int window)
{   // libcsdr.c:665-673
    const float ci = 1.0 / interpolation, cd = 1.0 / decimation;
    const float cutoff = ci < cd ? ci : cd;
    csdr_amd_firdes_lowpass_f(output, output_size, cutoff / 2, window);
}

int csdr_amd_debug_resampler_schedule(int I, int D, int T, int last_taps_delay, int n, int *out)
{
    if (I < 1 || D < 1 || T < 1 || n < 0 || last_taps_delay < 0 || last_taps_delay >= I) return fail_msg(-3, "resampler schedule: need I, D, T >= 1 and 0 <= last_taps_delay < I");
    for (int k = 0; k < n; k++) {
        long long ds; int d; rr_step(k, I, D, last_taps_delay, &ds, &d);
        out[3 * k] = (int)ds; out[3 * k + 1] = d; out[3 * k + 2] = rr_taps(T, I, d);
    }
    return 0;
}

csdr_amd_resampler *csdr_amd_resampler_create(csdr_amd_ctx *c, int interpolation, int decimation, const float *host_taps, int taps_length, int n_streams)
{
    if (!c || interpolation < 1 || decimation < 1 || !host_taps || taps_length < 1 || n_streams < 1 || n_streams > 65535) {
        fail_msg(-3, "resampler: need interpolation, decimation, taps_length >= 1, 1 <= n_streams <= 65535 and taps");
        return nullptr;
    }
    Owned<csdr_amd_resampler, csdr_amd_resampler_destroy> r(new csdr_amd_resampler());
    r->c = c; r->I = interpolation; r->D = decimation; r->T = taps_length; r->n_ch = n_streams;
    const int g = std::gcd(interpolation, decimation);
    r->P = interpolation / g; r->Dg = decimation / g; r->cli_pmin = 1; r->tab_cap = 0;
    // k_rr_poly's tile: the largest M (a multiple of 64) whose LDS fits the budget
    const int Kmax = taps_length / interpolation;
    r->M = 0; r->Cp = 0; r->lds = 0;
    for (int M = RR_MAX_M; M >= 64; M -= 64) {
        int Cp = M + (Kmax + r->Dg - 1) / r->Dg + 2; Cp |= 1;
        const size_t lds = sizeof(float) * ((size_t)r->Dg * Cp + (size_t)r->P * M + 2 * (size_t)r->P + 2);
        if (lds <= (size_t)RR_LDS_BUDGET && (long long)r->Dg * Cp < (1 << 24)) { r->M = M; r->Cp = Cp; r->lds = lds; break; }
    }
    if (r->M && lds_attr_once((const void *)k_rr_poly, r->lds)) return nullptr;
    if (dev_alloc(r->d_taps, sizeof(float) * taps_length) != hipSuccess || rr_alloc_hist(r.get()) < 0) { fail_msg(-2, "resampler: device allocation failed"); return nullptr; }
    // k_rr_poly's tables: the taps phase-major (row d = taps[d + i I], i < K(d), zero-padded to Kpad) and the LDS offset of each tile-relative sample;
    // both with 16 entries to spare, as the tap loop loads the next group of 8 ahead of the current one
    r->Kpad = ((Kmax + 7) & ~7) + 16;
    std::vector<float> tpm((size_t)interpolation * r->Kpad, 0.f);
    for (int d = 0; d < interpolation; d++)
        for (int i = 0; i < rr_taps(taps_length, interpolation, d); i++) tpm[(size_t)d * r->Kpad + i] = host_taps[d + (size_t)i * interpolation];
    std::vector<int> offt((size_t)r->Dg + Kmax + 17, 0);
    if (r->M) for (size_t t = 0; t < offt.size(); t++) offt[t] = (int)(t % r->Dg) * r->Cp + (int)(t / r->Dg);
    if (dev_alloc(r->d_tpm, sizeof(float) * tpm.size()) != hipSuccess || dev_alloc(r->d_offt, sizeof(int) * offt.size()) != hipSuccess) {
        fail_msg(-2, "resampler: device allocation failed"); return nullptr;
    }
    if (csdr_amd_h2d(c, r->d_taps.get(), host_taps, sizeof(float) * taps_length) < 0 || csdr_amd_h2d(c, r->d_tpm.get(), tpm.data(), sizeof(float) * tpm.size()) < 0 ||
        csdr_amd_h2d(c, r->d_offt.get(), offt.data(), sizeof(int) * offt.size()) < 0 || csdr_amd_resampler_reset(r.get()) < 0) return nullptr;
    return r.release();
}

int csdr_amd_resampler_reset(csdr_amd_resampler *r)
{
    if (!r) return fail_msg(-3, "resampler: null object");
    r->total = 0; r->s_next = 0; r->d_next = 0; r->emitted = 0; r->win_a = 0; r->win_L = 0; r->cur = 0;
    // (positions before the stream's start are never read)
    return csdr_amd_memset(r->c, r->d_hist[0].get(), 0, sizeof(float) * (size_t)r->H * r->n_ch) < 0 ? -5 : 0;
}

int csdr_amd_resampler_set_cli_bufsize(csdr_amd_resampler *r, int the_bufsize)
{
    if (!r) return fail_msg(-3, "resampler: null object");
    if (the_bufsize < 0 || (the_bufsize > 0 && (long long)the_bufsize * r->I / r->D < 1)) return fail_msg(-3, "resampler: the_bufsize * I / D must be >= 1");
    CSDR_HIP(hipStreamSynchronize(r->c->stream));
    r->cli_bufsize = the_bufsize;
    r->cli_pmin = the_bufsize;
    for (int L = 0; L < r->I && the_bufsize; L++) {
        int cnt, processed, L_out; rr_window(r->I, r->D, r->T, the_bufsize, L, &cnt, &processed, &L_out);
        if (processed > 0 && processed < r->cli_pmin) r->cli_pmin = processed;
    }
    if (rr_alloc_hist(r) < 0) return -2;
    return csdr_amd_resampler_reset(r);
}

int csdr_amd_resampler_set_last_taps_delay(csdr_amd_resampler *r, int last_taps_delay)
{
    if (!r) return fail_msg(-3, "resampler: null object");
    if (last_taps_delay < 0 || last_taps_delay >= r->I) return fail_msg(-3, "resampler: last_taps_delay must be in [0, I)");
    r->d_next = r->win_L = last_taps_delay;
    return 0;
}

int csdr_amd_resampler_window(int I, int D, int T, int input_size, int last_taps_delay, int *state)
{
    if (I < 1 || D < 1 || T < 1 || input_size < 0 || last_taps_delay < 0 || last_taps_delay >= I) return fail_msg(-3, "resampler window: need I, D, T >= 1 and 0 <= last_taps_delay < I");
    rr_window(I, D, T, input_size, last_taps_delay, &state[1], &state[0], &state[2]);
    return 0;
}

int csdr_amd_resampler_force_generic(csdr_amd_resampler *r, int on) { return bank_force_generic(r, "resampler", on); }
const char *csdr_amd_resampler_kernel_name(const csdr_amd_resampler *r) { return bank_kernel_name(r); }

void csdr_amd_resampler_destroy(csdr_amd_resampler *r) { destroy_on_stream(r); }

long long csdr_amd_resampler_max_out(const csdr_amd_resampler *r, long long n_in)
{
    if (!r) return 0;
    if (!r->cli_bufsize) return n_in * r->I / r->D + 2;
    return ((n_in + r->cli_bufsize) / r->cli_pmin + 1) * ((long long)r->cli_bufsize * r->I / r->D);     // windows this call can complete x outputs per window
}

int csdr_amd_resampler_process(csdr_amd_resampler *r, const float *in, long long n_in, size_t in_pitch, float *out, size_t out_pitch, long long *n_out)
{
    if (n_out) *n_out = 0;
    if (!r) return fail_msg(-3, "resampler: null object");
    if (n_in < 0 || (n_in > 0 && (!in || in_pitch < (size_t)n_in))) return fail_msg(-3, "resampler: need in_pitch >= n_in >= 0");
    if (!n_in) return 0;
    if ((long long)r->H + n_in >= (1LL << 31)) return fail_msg(-3, "resampler: %lld samples per call is too many", n_in);
    csdr_amd_ctx *c = r->c;
    const long long v0 = r->total - r->H, total_after = r->total + n_in;        // V[0] is absolute sample v0
    std::vector<RrSeg> segs; long long n = 0;
    if (!r->cli_bufsize) {
        const long long L = total_after - r->T / r->I - 1 - r->s_next;           // outputs j with s_j + T/I + 1 <= total_after (libcsdr.c:624)
        long long cnt = L >= 0 ? (L * r->I + r->d_next) / r->D + 1 : 0;
        cnt = std::min(cnt, total_after * r->I / r->D - r->emitted);          // ... and the reference's output_size = input_size * I / D (libcsdr.c:616)
        if (cnt > 0) {
            segs.push_back(RrSeg{(int)(r->s_next - v0), r->d_next, 0, (int)cnt});
            long long ds; int d; rr_step(cnt, r->I, r->D, r->d_next, &ds, &d);
            r->s_next += ds; r->d_next = d; r->emitted += cnt; n = cnt;
        }
    } else {
        const int B = r->cli_bufsize;
        while (r->win_a + B <= total_after) {                                   // csdr.c:1441-1459
            int cnt, processed, L;
            rr_window(r->I, r->D, r->T, B, r->win_L, &cnt, &processed, &L);
            if (cnt > 0) { segs.push_back(RrSeg{(int)(r->win_a - v0), r->win_L, (int)n, cnt}); n += cnt; }
            r->win_a += processed ? processed : B;                              // input_processed == 0: a whole fresh buffer is read
            r->win_L = L;
            if (n >= (1LL << 31) - (1LL << 20)) return fail_msg(-3, "resampler: too many outputs in one call");
        }
    }
    if (n > 0) {
        if (out_pitch < (size_t)n) return fail_msg(-3, "resampler: out_pitch %zu below the %lld outputs of this call", out_pitch, n);
        const bool poly = r->M && !r->force_generic;
        if (poly) {
            std::vector<RrSeg> tiles;
            const int per = r->P * r->M;
            for (const RrSeg &g : segs)
                for (int t = 0; (long long)t * per < g.count; t++)
                    tiles.push_back(RrSeg{g.s + t * r->M * r->Dg, g.d0, g.out0 + t * per, std::min(per, g.count - t * per)});
            if (upload_table(c, r->d_tab, r->tab_cap, tiles) < 0) return -5;
            hipLaunchKernelGGL(k_rr_poly, dim3((unsigned)tiles.size(), r->n_ch), dim3(RR_THREADS), r->lds, c->stream, r->d_hist[r->cur].get(), r->H, (size_t)r->H,
                               in, in_pitch, n_in, out, out_pitch, r->d_tab.get(), r->I, r->D, r->T, r->P, r->Dg, r->M, r->Cp, r->d_tpm.get(), r->Kpad, r->d_offt.get());
        } else {
            if (upload_table(c, r->d_tab, r->tab_cap, segs) < 0) return -5;
            hipLaunchKernelGGL(k_rr_generic, dim3(cdiv(n, 256), r->n_ch), dim3(256), 0, c->stream, r->d_hist[r->cur].get(), r->H, (size_t)r->H,
                               in, in_pitch, n_in, out, out_pitch, r->d_tab.get(), (int)segs.size(), (int)n, r->I, r->D, r->T, r->d_taps.get());
        }
        CSDR_LAUNCH_CHECK();
        r->last_kernel = poly ? "k_rr_poly" : "k_rr_generic";
    }
    if (hist_advance(c, r->d_hist[r->cur].get(), r->d_hist[r->cur ^ 1].get(), r->H, (size_t)r->H, in, in_pitch, n_in, r->n_ch) < 0) return -5;
    r->cur ^= 1;
    r->total = total_after;
    if (n_out) *n_out = n;
    return 0;
}

// ------------------------------------------------------------------ fir_interpolate_cc
csdr_amd_interp *csdr_amd_interp_create(csdr_amd_ctx *c, int interpolation, const float *host_taps, int taps_length, int n_streams)
{
    if (!c || interpolation < 1 || !host_taps || taps_length < 1 || n_streams < 1 || n_streams > 65535) {
        fail_msg(-3, "interp: need interpolation, taps_length >= 1, 1 <= n_streams <= 65535 and taps");
        return nullptr;
    }
    Owned<csdr_amd_interp, csdr_amd_interp_destroy> p(new csdr_amd_interp());
    p->c = c; p->I = interpolation; p->T = taps_length; p->n_ch = n_streams;
    p->Kmax = 0;
    for (int ip = 0; ip < interpolation; ip++) p->Kmax = std::max(p->Kmax, interp_taps(taps_length, interpolation, ip));
    if (sizeof(float2) * (256 * 9 + (size_t)p->Kmax) <= (size_t)IP_LDS_BUDGET) {
        const size_t lds = sizeof(float2) * (256 * 9 + (size_t)p->Kmax);
        if (lds_attr_once((const void *)k_interp_poly<1>, lds) || lds_attr_once((const void *)k_interp_poly<2>, lds) ||
            lds_attr_once((const void *)k_interp_poly<4>, lds) || lds_attr_once((const void *)k_interp_poly<8>, lds)) return nullptr;
    }
    if (dev_alloc(p->d_taps, sizeof(float) * taps_length) != hipSuccess || ip_alloc_hist(p.get()) < 0) { fail_msg(-2, "interp: device allocation failed"); return nullptr; }
    if (csdr_amd_h2d(c, p->d_taps.get(), host_taps, sizeof(float) * taps_length) < 0 || csdr_amd_interp_reset(p.get()) < 0) return nullptr;
    return p.release();
}

int csdr_amd_interp_reset(csdr_amd_interp *p)
{
    if (!p) return fail_msg(-3, "interp: null object");
    p->total = p->cli_bufsize; p->pos_next = 0; p->cur = 0;                 // cli_bufsize mode: the CLI's first pass runs over a buffer of zeros (csdr.c:1218-1221)
    return csdr_amd_memset(p->c, p->d_hist[0].get(), 0, sizeof(float2) * (size_t)p->H * p->n_ch) < 0 ? -5 : 0;
}

int csdr_amd_interp_set_cli_bufsize(csdr_amd_interp *p, int the_bufsize)
{
    if (!p) return fail_msg(-3, "interp: null object");
    if (the_bufsize < 0) return fail_msg(-3, "interp: the_bufsize must be >= 0");
    CSDR_HIP(hipStreamSynchronize(p->c->stream));
    p->cli_bufsize = the_bufsize;
    if (ip_alloc_hist(p) < 0) return -2;
    return csdr_amd_interp_reset(p);
}

int csdr_amd_interp_force_generic(csdr_amd_interp *p, int on) { return bank_force_generic(p, "interp", on); }
const char *csdr_amd_interp_kernel_name(const csdr_amd_interp *p) { return bank_kernel_name(p); }

void csdr_amd_interp_destroy(csdr_amd_interp *p) { destroy_on_stream(p); }

long long csdr_amd_interp_max_out(const csdr_amd_interp *p, long long n_in)
{
    return p ? (n_in + p->cli_bufsize + 1) * (long long)p->I : 0;
}

int csdr_amd_interp_process(csdr_amd_interp *p, const csdr_complexf *in, long long n_in, size_t in_pitch, csdr_complexf *out, size_t out_pitch, long long *n_out)
{
    if (n_out) *n_out = 0;
    if (!p) return fail_msg(-3, "interp: null object");
    if (n_in < 0 || (n_in > 0 && (!in || in_pitch < (size_t)n_in))) return fail_msg(-3, "interp: need in_pitch >= n_in >= 0");
    if (!n_in) return 0;
    if (((long long)p->H + n_in) * p->I >= (1LL << 31)) return fail_msg(-3, "interp: %lld samples per call is too many", n_in);
    csdr_amd_ctx *c = p->c;
    const long long v0 = p->total - p->H, total_after = p->total + n_in;
    const long long num = total_after * p->I - p->I + 1 - p->T;              // positions i with i I + I - 1 + T <= total I (libcsdr.c:589)
    const long long last = num >= 0 ? num / p->I : -1;
    const long long n_pos = std::max(0LL, last + 1 - p->pos_next);
    const long long n = n_pos * p->I;
    if (n > 0) {
        if (out_pitch < (size_t)n) return fail_msg(-3, "interp: out_pitch %zu below the %lld outputs of this call", out_pitch, n);
        const int pos0 = (int)(p->pos_next - v0);
        const float2 *h = (const float2 *)p->d_hist[p->cur].get(); const float2 *x = (const float2 *)in; float2 *o = (float2 *)out;
        const int IC = p->I >= 8 ? 8 : p->I >= 4 ? 4 : p->I >= 2 ? 2 : 1;
        const size_t lds = sizeof(float2) * (256 * (1 + (size_t)IC) + (size_t)p->Kmax);
        const bool poly = sizeof(float2) * (256 * 9 + (size_t)p->Kmax) <= (size_t)IP_LDS_BUDGET && !p->force_generic;
        if (poly) {
            const dim3 grid(cdiv(n_pos, 256), p->n_ch);
#define IP_LAUNCH(ICV) hipLaunchKernelGGL(k_interp_poly<ICV>, grid, dim3(256), lds, c->stream, h, p->H, (size_t)p->H, x, in_pitch, n_in, o, out_pitch, pos0, (int)n_pos, p->I, p->T, p->Kmax, p->d_taps.get())
            if (IC == 8) IP_LAUNCH(8); else if (IC == 4) IP_LAUNCH(4); else if (IC == 2) IP_LAUNCH(2); else IP_LAUNCH(1);
#undef IP_LAUNCH
        } else {
            hipLaunchKernelGGL(k_interp_generic, dim3(cdiv(n, 256), p->n_ch), dim3(256), 0, c->stream, h, p->H, (size_t)p->H, x, in_pitch, n_in, o, out_pitch,
                               pos0, (int)n_pos, p->I, p->T, p->d_taps.get());
        }
        CSDR_LAUNCH_CHECK();
        p->last_kernel = poly ? "k_interp_poly" : "k_interp_generic";
        p->pos_next += n_pos;
    }
    if (hist_advance(c, (const float2 *)p->d_hist[p->cur].get(), p->d_hist[p->cur ^ 1].get(), p->H, (size_t)p->H, (const float2 *)in, in_pitch, n_in, p->n_ch) < 0) return -5;
    p->cur ^= 1;
    p->total = total_after;
    if (n_out) *n_out = n;
    return 0;
}

} // extern "C"
