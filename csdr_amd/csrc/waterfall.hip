// waterfall.hip -- the spectrum side of a web receiver as one batched object: `fft_cc N E [window] | logaveragepower_cf A N AVG | fft_exchange_sides_ff N
// [| compress_fft_adpcm_f_u8 N]` (csdr.c:1569-1641, 1663-1714, 1745-1768) for n_streams streams per call, optionally behind convert_u8_f (libcsdr.c:2363-2366).
//
// One-pass form (fft 1024 / 2048 / 4096 / 8192, k_wf_onepass): one workgroup of N/16 threads per (stream, row segment).  For every frame of the segment each
// thread loads 16 samples (t, t + N/16, ...: coalesced), converts and windows them, and runs a Stockham radix-16 / 16 / {4, 8, 16, 16 x 2} forward transform:
// the first and last passes in registers, the exchanges between passes through LDS (N + N/16 padded float2).  The last pass leaves each thread the same 16 bins
// in every frame, so |X|^2 is summed in registers.  Window values and one base twiddle per butterfly come from small cache-resident tables every frame (the
// powers a point needs are formed by a multiplication tree): kept in registers they pushed the 8192-point form into scratch.  After the last
// frame the row is 10 log10(acc) + add_db', swapped and written -- as float dB, or compressed by thread 0 from shorts staged in LDS.  The input is read once
// (plus the overlap of neighbouring frames); the rows are the only output.
// Generic form (every other power of two): k_wf_frame writes the windowed frames of a group of streams, hipFFT transforms them in place, k_wf_post sums,
// averages, takes the log, swaps and compresses in one pass over the spectra.  k_wf_post (without framing) is also logaveragepower_cf and
// fft_exchange_sides_ff (csdr_amd_logaveragepower_cf / csdr_amd_fft_exchange_sides_ff).
// Summation order, both forms: per bin, frame by frame in stream order, acc += re*re + im*im in float32 starting from 0 (the reference's
// accumulate_power_cf, libcsdr.c:1305-1308); a row split across calls carries acc in float, so the split changes nothing (two buffers: a call's first
// segment reads the carried row while its last segment writes the next one).
// Frame schedule = fft_cc's (csdr.c:1608-1625): frame k covers stream samples [k E + off, k E + off + N), off = min(0, E - N); samples before 0 are the
// zeros of the reference's fresh sliding buffer.  All streams of an object advance in lockstep, so the schedule is host-side scalars; each stream keeps the
// last N raw input samples (the overlap history) and its partial row (acc in device memory).
//
// Real input (CSDR_AMD_WF_IN_F32 / _S16): `[convert_s16_f |] fft_fc M E [window] | logaveragepower_cf A M AVG [| compress_fft_adpcm_f_u8 M]` (csdr.c:3414-3498).
// fft_size is M, the number of output bins; a frame is 2M real samples, loaded as the M complex points z[n] = w[2n] x[2n] + i w[2n+1] x[2n+1].  The M-point
// passes run unchanged on z; one more exchange through the same LDS (Z in natural order, every thread reads its bins' partners) untangles Z into the real
// signal's spectrum, X[k] = 1/2 (Z[k] + conj Z[(M-k) mod M]) - (i/2) e^(-i pi k / M) (Z[k] - conj Z[(M-k) mod M]), k < M (the Nyquist bin is not formed, as
// fft_fc does not write it).  Rows are in display order already: no exchange of halves.  The generic form packs the same way, runs the M-point hipFFT plan
// and untangles in k_wf_post.  Frame schedule = fft_fc's, in real samples: E <= 2M: frame k covers [k E + E - 2M, k E + E); E > 2M: the reference's skip loop
// reads complexf-sized items from the float stream (csdr.c:3466-3469), so it drops 2 (E - 2M) floats and frame k covers [k P, k P + 2M), P = 2 E - 2M.
// The eight real instantiations take 181 - 240 VGPRs and no scratch (two waves per SIMD).  At M = 8192 a workgroup holds a CU alone, so its compressed rows
// are not encoded by thread 0 inside the kernel but by k_wf_post's stand-alone mode over dB rows in scratch (run_onepass).
//
// The one-pass stages are __host__ __device__: csdr_amd_debug_waterfall_row runs them on the CPU thread by thread (same index maps, same accumulation order).
#include "common.hpp"
#include "convert_dev.hpp"
#include "adpcm_dev.hpp"
// no bit-exact contract on the transform (float FFT paths are gated at 1e-5 relative RMS): the butterflies may contract into FMAs
#pragma clang fp contract(fast)
#include "fft_butterflies.hpp"
#include <hipfft/hipfft.h>
#include <math.h>
#include <array>
#include <map>
#include <string.h>
#include <vector>

using namespace csdr_amd;

#define WF_HD __host__ __device__ __forceinline__

namespace {

// ---- the one-pass transform: passes R0 x R1 x R2 [x R3], N/16 threads, 16 points per thread and pass
template <int N> struct WfPlan;
template <> struct WfPlan<1024> { static constexpr int NP = 3, R[4] = {16, 16, 4, 1}; };
template <> struct WfPlan<2048> { static constexpr int NP = 3, R[4] = {16, 16, 8, 1}; };
template <> struct WfPlan<4096> { static constexpr int NP = 3, R[4] = {16, 16, 16, 1}; };
template <> struct WfPlan<8192> { static constexpr int NP = 4, R[4] = {16, 16, 16, 2}; };

template <int N> struct WfGeom {
    static constexpr int T = N / 16;                                    // threads per workgroup
    static constexpr int DATA = N + N / 16;                             // padded LDS points
    static constexpr size_t LDS_BYTES = (size_t)DATA * sizeof(float2);
};
WF_HD constexpr int wf_pad(int p) { return p + (p >> 4); }

template <int R> struct WfDft;
template <> struct WfDft<16> { template <int O> static WF_HD void run(float2 *v) { float2 (&a)[16] = *reinterpret_cast<float2 (*)[16]>(v + O); dft16<false>(a); } };
template <> struct WfDft<8>  { template <int O> static WF_HD void run(float2 *v) { float2 (&a)[8] = *reinterpret_cast<float2 (*)[8]>(v + O); dft8<false>(a); } };
template <> struct WfDft<4>  { template <int O> static WF_HD void run(float2 *v) { dft4<false>(v[O], v[O + 1], v[O + 2], v[O + 3]); } };
template <> struct WfDft<2>  { template <int O> static WF_HD void run(float2 *v) { const float2 a = v[O], b = v[O + 1]; v[O] = cadd(a, b); v[O + 1] = csub(a, b); } };

// w^k, k < R, by a multiplication tree of depth <= 4: w^k = w^h w^(k-h), h the largest power of two <= k
template <int R> WF_HD void wf_powers(float2 w, float2 (&p)[R])
{
    p[0] = make_float2(1.f, 0.f);
    if (R > 1) p[1] = w;
#pragma unroll
    for (int k = 2; k < R; k++) {
        const int h = 1 << (31 - __builtin_clz(k));
        p[k] = cmul(p[h == k ? h / 2 : h], p[h == k ? h / 2 : k - h]);
    }
}

// Stockham pass P (Ns = R0 ... R(P-1) points already transformed): butterfly j = t + b T (b < 16/R) reads points j + r N/R, multiplies point r by
// W_(Ns R)^(r (j mod Ns)), runs the R-point DFT and writes point r to (j / Ns) Ns R + (j mod Ns) + r Ns.  Register slot of point r of butterfly b: b R + r.
template <int N, int P> struct WfPass {
    static constexpr int R = WfPlan<N>::R[P], B = 16 / R, T = WfGeom<N>::T;
    static constexpr int NS = P == 0 ? 1 : P == 1 ? WfPlan<N>::R[0] : P == 2 ? WfPlan<N>::R[0] * WfPlan<N>::R[1] : WfPlan<N>::R[0] * WfPlan<N>::R[1] * WfPlan<N>::R[2];
    // both maps are a per-thread base plus a per-slot constant; the constant is a multiple of 16 or the base is (pass 0's dst), so
    // wf_pad(base + off) = wf_pad(base) + wf_pad(off) and the LDS offsets fold into the instructions
    static_assert(T % NS == 0 || NS * R == N, "a pass whose butterflies span several groups per thread is the last one");
    static constexpr bool SPLIT = T % NS == 0;
    static WF_HD int src_base(int t) { return t; }
    static constexpr int src_off(int slot) { return (slot / R) * T + (slot % R) * (N / R); }
    static WF_HD int dst_base(int t) { return SPLIT ? (t / NS) * NS * R + t % NS : t; }
    static constexpr int dst_off(int slot) { return SPLIT ? (slot / R) * T * R + (slot % R) * NS : (slot / R) * T + (slot % R) * NS; }
    static WF_HD int src(int t, int slot) { return src_base(t) + src_off(slot); }
    static WF_HD int dst(int t, int slot) { return dst_base(t) + dst_off(slot); }
    // thread t's base twiddle W_(Ns R)^(j mod Ns) of each of its butterflies (table: exp(-2 pi i m / N)); point r takes its r-th power
    static WF_HD void twiddles(int t, const float2 *table, float2 (&w)[8])
    {
#pragma unroll
        for (int b = 0; b < B; b++) w[b] = table[((t + b * T) % NS) * (N / (NS * R))];
    }
    static WF_HD void compute(float2 (&v)[16], const float2 (&w)[8])
    {
        if (P > 0) {
#pragma unroll
            for (int b = 0; b < B; b++) {
                float2 pw[R];
                wf_powers<R>(w[b], pw);
#pragma unroll
                for (int r = 1; r < R; r++) v[b * R + r] = cmul(v[b * R + r], pw[r]);
            }
        }
        if constexpr (B >= 1) WfDft<R>::template run<0>(v);
        if constexpr (B >= 2) WfDft<R>::template run<R>(v);
        if constexpr (B >= 4) { WfDft<R>::template run<2 * R>(v); WfDft<R>::template run<3 * R>(v); }
        if constexpr (B >= 8) { WfDft<R>::template run<4 * R>(v); WfDft<R>::template run<5 * R>(v); WfDft<R>::template run<6 * R>(v); WfDft<R>::template run<7 * R>(v); }
    }
    static WF_HD void lds_read(const float2 *lds, int t, float2 (&v)[16])
    {
#pragma unroll
        for (int s = 0; s < 16; s++) v[s] = lds[wf_pad(src_base(t)) + wf_pad(src_off(s))];
    }
    static WF_HD void lds_write(float2 *lds, int t, const float2 (&v)[16])
    {
#pragma unroll
        for (int s = 0; s < 16; s++) lds[wf_pad(dst_base(t)) + wf_pad(dst_off(s))] = v[s];
    }
};
// bin of register slot s after the last pass
template <int N> WF_HD int wf_bin(int t, int s) { return WfPass<N, WfPlan<N>::NP - 1>::dst(t, s); }

// the base twiddles of passes 1 .. NP-1 of one thread (the CPU run keeps them per thread; the kernel re-reads them per frame)
template <int N> struct WfConst { float2 w1[8], w2[8], w3[8]; };
template <int N> WF_HD void wf_const(int t, const float2 *table, WfConst<N> &c)
{
    WfPass<N, 1>::twiddles(t, table, c.w1);
    WfPass<N, 2>::twiddles(t, table, c.w2);
    if constexpr (WfPlan<N>::NP > 3) WfPass<N, 3>::twiddles(t, table, c.w3);
}

// bytes per raw unit of the schedule: a complex sample (cf32, u8 IQ) or a real one (f32, s16)
template <int IN> constexpr int wf_elem() { return IN == CSDR_AMD_WF_IN_U8 || IN == CSDR_AMD_WF_IN_S16 ? 2 : IN == CSDR_AMD_WF_IN_F32 ? 4 : 8; }
template <int IN> constexpr bool wf_real() { return IN == CSDR_AMD_WF_IN_F32 || IN == CSDR_AMD_WF_IN_S16; }

// one raw sample as a complex float: u8 IQ through convert_u8_f's arithmetic, or cf32
template <int IN> WF_HD float2 wf_to_c(const void *p, long long idx)
{
    if (IN == CSDR_AMD_WF_IN_U8) {
        const uint8_t *b = (const uint8_t *)p + 2 * idx;
#ifdef __HIP_DEVICE_COMPILE__
        return make_float2(to_float<0>(b[0]), to_float<0>(b[1]));
#else
        return make_float2((float)((float)b[0] / (255 / 2.0) - 1.0), (float)((float)b[1] / (255 / 2.0) - 1.0));   // libcsdr.c:2365 (the device form equals it for all codes)
#endif
    }
    const csdr_complexf c = ((const csdr_complexf *)p)[idx];
    return make_float2(c.i, c.q);
}
// stream sample p (p >= base - hist_len) windowed: the call's input from base on, the history before it; positions before the stream's start are the
// zeros of the fresh sliding buffer (complex zeros also for u8 input: the reference converts before it frames)
template <int IN> WF_HD float2 wf_windowed(const void *in, const void *hist, long long base, int hist_len, long long p, float w)
{
    const float2 x = p < 0 ? make_float2(0.f, 0.f) : p >= base ? wf_to_c<IN>(in, p - base) : wf_to_c<IN>(hist, p - base + hist_len);
    return make_float2(x.x * w, x.y * w);
}
// the frame's samples and window, pass 0 (radix 16, no twiddles)
template <int N, int IN> WF_HD void wf_load(const void *in, const void *hist, long long base, int hist_len, long long start, int t, const float *window, float2 (&v)[16])
{
    if (start >= base) {                                                 // (uniform) the whole frame lies in this call's input: one base address per thread
        const char *x = (const char *)in + (size_t)(start - base + t) * wf_elem<IN>();
        const float *wt = window + t;
#pragma unroll
        for (int s = 0; s < 16; s++) {
            const float2 y = wf_to_c<IN>(x, WfPass<N, 0>::src_off(s));
            const float w = wt[WfPass<N, 0>::src_off(s)];
            v[s] = make_float2(y.x * w, y.y * w);
        }
        return;
    }
#pragma unroll
    for (int s = 0; s < 16; s++) v[s] = wf_windowed<IN>(in, hist, base, hist_len, start + WfPass<N, 0>::src(t, s), window[WfPass<N, 0>::src(t, s)]);
}
// ---- real input: one raw sample as a float (s16 through convert_s16_f's arithmetic), the packed load, the untangle
WF_HD float wf_s16_f(int raw)
{
#ifdef __HIP_DEVICE_COMPILE__
    return to_float<2>(raw);
#else
    return (float)raw * (1.0f / 32767.0f);                               // libcsdr.c:2370 as the reference's -ffast-math build forms it (convert_dev.hpp)
#endif
}
template <int IN> WF_HD float wf_to_r(const void *p, long long idx)
{
    if (IN == CSDR_AMD_WF_IN_S16) return wf_s16_f(((const int16_t *)p)[idx]);
    return ((const float *)p)[idx];
}
// samples 2n and 2n+1 of p as one load (p aligned to a pair)
template <int IN> WF_HD float2 wf_pair(const void *p, int n)
{
    if (IN == CSDR_AMD_WF_IN_S16) {
        const uint32_t u = ((const uint32_t *)p)[n];
        return make_float2(wf_s16_f((int16_t)(u & 0xffff)), wf_s16_f((int16_t)(u >> 16)));
    }
    return ((const float2 *)p)[n];
}
// packed point n of the frame that starts at real sample `start`: (w[2n] x[start + 2n], w[2n+1] x[start + 2n + 1]); positions as wf_windowed's
template <int IN> WF_HD float2 wf_packed(const void *in, const void *hist, long long base, int hist_len, long long start, int n, const float *window)
{
    float x[2];
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const long long p = start + 2 * n + e;
        x[e] = p < 0 ? 0.f : p >= base ? wf_to_r<IN>(in, p - base) : wf_to_r<IN>(hist, p - base + hist_len);
    }
    const float2 w = reinterpret_cast<const float2 *>(window)[n];
    return make_float2(x[0] * w.x, x[1] * w.y);
}
template <int N, int IN> WF_HD void wf_load_r(const void *in, const void *hist, long long base, int hist_len, long long start, int t, const float *window, float2 (&v)[16])
{
    if (start >= base) {                                                 // (uniform) the whole frame lies in this call's input
        const char *x = (const char *)in + (size_t)(start - base + 2 * t) * wf_elem<IN>();
        const float2 *wt = reinterpret_cast<const float2 *>(window) + t;
        if (((size_t)x & (2 * wf_elem<IN>() - 1)) == 0) {                // (uniform: the threads' addresses differ by whole pairs) a pair per load
#pragma unroll
            for (int s = 0; s < 16; s++) {
                const float2 y = wf_pair<IN>(x, WfPass<N, 0>::src_off(s)), w = wt[WfPass<N, 0>::src_off(s)];
                v[s] = make_float2(y.x * w.x, y.y * w.y);
            }
            return;
        }
#pragma unroll
        for (int s = 0; s < 16; s++) {
            const float2 w = wt[WfPass<N, 0>::src_off(s)];
            v[s] = make_float2(wf_to_r<IN>(x, 2 * WfPass<N, 0>::src_off(s)) * w.x, wf_to_r<IN>(x, 2 * WfPass<N, 0>::src_off(s) + 1) * w.y);
        }
        return;
    }
#pragma unroll
    for (int s = 0; s < 16; s++) v[s] = wf_packed<IN>(in, hist, base, hist_len, start, WfPass<N, 0>::src(t, s), window);
}
// bin k of the real signal's spectrum from Z[k], zm = Z[(M - k) mod M] and h = e^(-i pi k / M)
// (products and sums as written, in every kernel that inlines it: `fft_fc | logaveragepower_cf` then equals the generic form's rows bit for bit)
WF_HD float2 wf_untangle1(float2 z, float2 zm, float2 h)
{
#pragma clang fp contract(off)
    const float ax = 0.5f * (z.x + zm.x), ay = 0.5f * (z.y - zm.y), bx = 0.5f * (z.x - zm.x), by = 0.5f * (z.y + zm.y);
    const float cx = h.x * bx - h.y * by, cy = h.x * by + h.y * bx;      // c = h b
    return make_float2(ax + cy, ay - cx);                                // a - i c
}
// lds: Z in natural order (padded), written by the last pass's lds_write; every thread untangles the bins it holds
template <int N> WF_HD void wf_untangle(const float2 *lds, int t, const float2 *half, float2 (&v)[16])
{
#pragma unroll
    for (int s = 0; s < 16; s++) {
        const int k = wf_bin<N>(t, s);
        v[s] = wf_untangle1(v[s], lds[wf_pad((N - k) & (N - 1))], half[k]);
    }
}
template <int N> WF_HD void wf_accumulate(const float2 (&v)[16], float (&acc)[16])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int s = 0; s < 16; s++) acc[s] += v[s].x * v[s].x + v[s].y * v[s].y;       // accumulate_power_cf (libcsdr.c:1305-1308)
}
// log_ff (libcsdr.c:1310-1314): double log10 of the float sum, rounded, then 10 * it + add_db in float -- logpower_cf's arithmetic (f2blocks.hip)
WF_HD float wf_db(float acc, float add_db)
{
#pragma clang fp contract(off)
    return 10 * (float)log10((double)acc) + add_db;
}

// one segment of frames of one row: frames k0 .. k0 + n - 1 (absolute frame numbers); flags: LOAD = acc starts from the partial row, EMIT = the row is complete
// (written as output row `row`), otherwise acc goes back to the partial row
enum { WF_LOAD = 1, WF_EMIT = 2 };
struct WfSeg { long long k0; int n, flags, row, frame0; };             // frame0: index of frame k0 among this call's frames (generic form)

struct WfArgs {
    const void *in; size_t in_pitch;                                    // samples
    const void *hist; void *hist_new; int hist_len;                      // [stream][hist_len] raw samples: positions [base - hist_len, base)
    long long base; int every, off;
    const float *window; const float2 *table;                            // real input: window of 2N entries, table = [exp(-2 pi i m / N), m < N | exp(-i pi k / N), k < N]
    const float *acc_in; float *acc_out;                                 // [stream][N]: the partial row, natural bin order -- read from one buffer, written to the
                                                                         // other (the call's first segment reads it while its last one writes the next)
    void *out; size_t out_pitch; int out_format; float add_db;           // out_pitch: bytes
    const WfSeg *segs;
};


// thread 0 of a workgroup: the swapped row (as the shorts of csdr.c:1763, staged in LDS) -> (N + 10) / 2 bytes, encoder from the zero state (csdr.c:1764)
__device__ void wf_adpcm_row(const int16_t *q, int n, uint8_t *y)
{
    St st{0, 0};
    const int pad = q[0];
    for (int k = 0; k < 5; k++) { const unsigned lo = enc_one(pad, st), hi = enc_one(pad, st); y[k] = (uint8_t)(lo | (hi << 4)); }
    for (int k = 0; k < n / 2; k += 4) {
        const int4 w = *reinterpret_cast<const int4 *>(q + 2 * k);          // 8 shorts per LDS read
        const int v[4] = {w.x, w.y, w.z, w.w};
        uint32_t word = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const unsigned lo = enc_one((int)(int16_t)(v[e] & 0xffff), st), hi = enc_one(v[e] >> 16, st);
            word |= (lo | (hi << 4)) << (8 * e);
        }
        y[5 + k] = (uint8_t)word; y[6 + k] = (uint8_t)(word >> 8); y[7 + k] = (uint8_t)(word >> 16); y[8 + k] = (uint8_t)(word >> 24);
    }
}

template <int N, int IN>
__device__ __forceinline__ void wf_onepass(const WfArgs &a, float2 *wf_lds)
{
    constexpr int NP = WfPlan<N>::NP;
    constexpr bool REAL = wf_real<IN>();
    constexpr int SWAP = REAL ? 0 : N / 2;                               // a one-sided row is in display order already
    const int t = threadIdx.x, s = blockIdx.y;
    const WfSeg sg = a.segs[blockIdx.x];
    float2 w[8];                                                         // base twiddles of the pass at hand (re-read per frame: cache-resident, and registers are short)
    const char *in = (const char *)a.in + (size_t)s * a.in_pitch * wf_elem<IN>();
    const char *hist = (const char *)a.hist + (size_t)s * a.hist_len * wf_elem<IN>();
    const float *acc_in = a.acc_in + (size_t)s * N;
    float acc[16];
#pragma unroll
    for (int k = 0; k < 16; k++) acc[k] = (sg.flags & WF_LOAD) ? acc_in[wf_bin<N>(t, k)] : 0.f;
    float2 v[16];
    for (int f = 0; f < sg.n; f++) {
        const long long start = (sg.k0 + f) * a.every + a.off;
        if constexpr (REAL) wf_load_r<N, IN>(in, hist, a.base, a.hist_len, start, t, a.window, v);
        else wf_load<N, IN>(in, hist, a.base, a.hist_len, start, t, a.window, v);
        WfPass<N, 0>::compute(v, w);
        WfPass<N, 0>::lds_write(wf_lds, t, v);
        __syncthreads();
        WfPass<N, 1>::lds_read(wf_lds, t, v);
        WfPass<N, 1>::twiddles(t, a.table, w);
        WfPass<N, 1>::compute(v, w);
        __syncthreads();
        WfPass<N, 1>::lds_write(wf_lds, t, v);
        __syncthreads();
        WfPass<N, 2>::lds_read(wf_lds, t, v);
        WfPass<N, 2>::twiddles(t, a.table, w);
        WfPass<N, 2>::compute(v, w);
        if constexpr (NP > 3) {
            __syncthreads();
            WfPass<N, 2>::lds_write(wf_lds, t, v);
            __syncthreads();
            WfPass<N, 3>::lds_read(wf_lds, t, v);
            WfPass<N, 3>::twiddles(t, a.table, w);
            WfPass<N, 3>::compute(v, w);
        }
        if constexpr (REAL) {
            __syncthreads();
            WfPass<N, NP - 1>::lds_write(wf_lds, t, v);                  // Z in natural order
            __syncthreads();
            wf_untangle<N>(wf_lds, t, a.table + N, v);
        }
        wf_accumulate<N>(v, acc);
        __syncthreads();                                                 // (the next frame's first write)
    }
    if (!(sg.flags & WF_EMIT)) {
#pragma unroll
        for (int k = 0; k < 16; k++) a.acc_out[(size_t)s * N + wf_bin<N>(t, k)] = acc[k];
        return;
    }
    char *orow = (char *)a.out + (size_t)s * a.out_pitch;
    if (a.out_format == CSDR_AMD_WF_OUT_DB) {
        float *o = (float *)orow + (size_t)sg.row * N;
#pragma unroll
        for (int k = 0; k < 16; k++) o[(wf_bin<N>(t, k) + SWAP) & (N - 1)] = wf_db(acc[k], a.add_db);
        return;
    }
    int16_t *q = reinterpret_cast<int16_t *>(wf_lds);
#pragma unroll
    for (int k = 0; k < 16; k++) q[(wf_bin<N>(t, k) + SWAP) & (N - 1)] = (int16_t)db_to_short(wf_db(acc[k], a.add_db));
    __syncthreads();
    if (t == 0) wf_adpcm_row(q, N, (uint8_t *)orow + (size_t)sg.row * ((N + 10) / 2));
}
template <int N, int IN>
__global__ __launch_bounds__(N / 16) void k_wf_onepass(WfArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float2 wf_lds[];
    wf_onepass<N, IN>(a, wf_lds);
}
// the real-input form (N = output bins, IN = CSDR_AMD_WF_IN_F32 / _S16): a name of its own in traces
template <int N, int IN>
__global__ __launch_bounds__(N / 16) void k_wf_onepass_real(WfArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float2 wf_lds[];
    wf_onepass<N, IN>(a, wf_lds);
}

// new history = the last hist_len samples of [history | input]  (raw samples as 16-bit units: u8 rows may start on any even byte)
__global__ __launch_bounds__(256) void k_wf_hist(const uint8_t *__restrict__ in, size_t in_pitch_b, const uint8_t *__restrict__ hist, uint8_t *__restrict__ hist_new,
                                                 size_t hist_b, size_t n_in_b)
{
    const int s = blockIdx.y;
    const uint16_t *x = (const uint16_t *)(in + (size_t)s * in_pitch_b);
    const uint16_t *h = (const uint16_t *)(hist + (size_t)s * hist_b);
    uint16_t *o = (uint16_t *)(hist_new + (size_t)s * hist_b);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < hist_b / 2; i += (size_t)gridDim.x * 256) {
        const size_t g = n_in_b + 2 * i;                                   // byte position in [history | input], history first
        o[i] = g >= hist_b ? x[(g - hist_b) / 2] : h[g / 2];
    }
}

// ---- generic form: framing (all streams of a group, this call's frames) -> frames [stream][frame][N] windowed cf32
template <int IN>
__global__ __launch_bounds__(256) void k_wf_frame(WfArgs a, int fft, long long k_first, int n_frames, float2 *__restrict__ frames, int s0)
{
    const int f = blockIdx.y, sl = blockIdx.z, s = s0 + sl;
    const char *in = (const char *)a.in + (size_t)s * a.in_pitch * wf_elem<IN>();
    const char *hist = (const char *)a.hist + (size_t)s * a.hist_len * wf_elem<IN>();
    const long long start = (k_first + f) * a.every + a.off;
    float2 *y = frames + ((size_t)sl * n_frames + f) * fft;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < fft; i += gridDim.x * 256) {
        if constexpr (wf_real<IN>()) y[i] = wf_packed<IN>(in, hist, a.base, a.hist_len, start, i, a.window);   // fft packed points of 2 fft real samples
        else y[i] = wf_windowed<IN>(in, hist, a.base, a.hist_len, start + i, a.window[i]);
    }
}

// post-FFT pass: POWER = sum |X|^2 over the segment's spectra, log, optional swap, dB or compressed row; !POWER = float rows, swap only
// (fft_exchange_sides_ff).  spectra: [stream][frame][fft], frames of segment = frame0 .. frame0 + n - 1.  One workgroup per (segment, stream).
// segs == nullptr: the stand-alone operations, row r = frames r avg .. r avg + avg - 1
// half_tw != nullptr (real input): the spectra are the transforms Z of packed frames; bin b of a frame is untangled from Z[b] and Z[(fft - b) mod fft]
template <bool POWER>
__global__ __launch_bounds__(256) void k_wf_post(const void *__restrict__ spectra, int fft, int n_frames, int avg, const WfSeg *__restrict__ segs, const float *__restrict__ acc_in, float *__restrict__ acc_out,
                                                 void *__restrict__ out, size_t out_pitch, int out_format, float add_db, int swap, int s0, int16_t *__restrict__ q_scratch,
                                                 const float2 *__restrict__ half_tw)
{
#pragma clang fp contract(off)
    const int sl = blockIdx.y, s = s0 + sl;
    WfSeg sg;
    if (segs) sg = segs[blockIdx.x];
    else { sg.k0 = (long long)blockIdx.x * avg; sg.n = avg; sg.flags = WF_EMIT; sg.row = blockIdx.x; sg.frame0 = blockIdx.x * avg; }
    const int half = swap ? fft / 2 : 0;
    char *orow = (char *)out + (size_t)s * out_pitch;
    int16_t *q = q_scratch ? q_scratch + ((size_t)sl * gridDim.x + blockIdx.x) * fft : nullptr;
    for (int b = threadIdx.x; b < fft; b += 256) {
        float v;
        if (POWER) {
            const float2 *x = (const float2 *)spectra + ((size_t)sl * n_frames + sg.frame0) * fft + b;
            float acc = (sg.flags & WF_LOAD) ? acc_in[(size_t)s * fft + b] : 0.f;
            if (half_tw) {
                const float2 *xm = x - b + ((fft - b) & (fft - 1));
                const float2 h = half_tw[b];
                for (int f = 0; f < sg.n; f++) { const float2 z = wf_untangle1(x[(size_t)f * fft], xm[(size_t)f * fft], h); acc += z.x * z.x + z.y * z.y; }
            } else
            for (int f = 0; f < sg.n; f++) { const float2 z = x[(size_t)f * fft]; acc += z.x * z.x + z.y * z.y; }
            if (!(sg.flags & WF_EMIT)) { acc_out[(size_t)s * fft + b] = acc; continue; }
            v = wf_db(acc, add_db);
        } else {
            v = ((const float *)spectra)[((size_t)sl * n_frames + sg.frame0) * fft + b];
        }
        const int o = (b + half) & (fft - 1);
        if (out_format == CSDR_AMD_WF_OUT_DB) ((float *)orow)[(size_t)sg.row * fft + o] = v;
        else q[o] = (int16_t)db_to_short(v);
    }
    if (out_format == CSDR_AMD_WF_OUT_DB || !(sg.flags & WF_EMIT)) return;
    __syncthreads();                                                     // (workgroup scope: q's global writes are visible to thread 0)
    if (threadIdx.x == 0) {
        uint8_t *y = (uint8_t *)orow + (size_t)sg.row * ((fft + 10) / 2);
        St st{0, 0};
        const int pad = q[0];
        for (int k = 0; k < 5; k++) { const unsigned lo = enc_one(pad, st), hi = enc_one(pad, st); y[k] = (uint8_t)(lo | (hi << 4)); }
        for (int k = 0; k < fft / 2; k++) { const unsigned lo = enc_one(q[2 * k], st), hi = enc_one(q[2 * k + 1], st); y[5 + k] = (uint8_t)(lo | (hi << 4)); }
    }
}

__global__ __launch_bounds__(256) void k_accumulate_power(const csdr_complexf *__restrict__ in, float *__restrict__ acc, size_t n)
{
#pragma clang fp contract(off)
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (size_t)gridDim.x * 256) acc[k] += in[k].i * in[k].i + in[k].q * in[k].q;
}
__global__ __launch_bounds__(256) void k_log_ff(const float *__restrict__ in, float *__restrict__ out, size_t n, float add_db)
{
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (size_t)gridDim.x * 256) out[k] = wf_db(in[k], add_db);
}

void twiddle_table(int n, std::vector<float2> &t)
{
    t.resize(n);
    for (int m = 0; m < n; m++) { const double a = -2.0 * M_PI * (double)m / n; t[m] = make_float2((float)cos(a), (float)sin(a)); }
}
// appends exp(-i pi k / n), k < n: the untangle's half-step twiddles
void half_table(int n, std::vector<float2> &t)
{
    for (int k = 0; k < n; k++) { const double a = -M_PI * (double)k / n; t.push_back(make_float2((float)cos(a), (float)sin(a))); }
}
// transforms per hipFFT plan execution (about 2 Mi points): one fixed batch for every call of the generic form and of the stand-alone fft_fc
int plan_batch(int n) { return n >= (1 << 21) ? 1 : (1 << 21) / n; }
bool onepass_size(int n) { return n == 1024 || n == 2048 || n == 4096 || n == 8192; }

template <int N, int IN> void *onepass_kernel()
{
    if constexpr (wf_real<IN>()) return (void *)&k_wf_onepass_real<N, IN>;
    else return (void *)&k_wf_onepass<N, IN>;
}
template <int N> void *onepass_kernel(int in_format)
{
    return in_format == CSDR_AMD_WF_IN_U8 ? onepass_kernel<N, 1>() : in_format == CSDR_AMD_WF_IN_F32 ? onepass_kernel<N, 2>() :
           in_format == CSDR_AMD_WF_IN_S16 ? onepass_kernel<N, 3>() : onepass_kernel<N, 0>();
}

} // namespace

struct csdr_amd_waterfall {
    csdr_amd_ctx *c; int fft, every, avg, in_format, out_format, n_streams; float add_db; size_t max_in;
    int len, period, off;                                                // the schedule in raw units: frame k covers [k period + off, k period + off + len)
    bool onepass, force_generic; const char *last_kernel;
    long long total, frames_done;                                        // samples per stream seen, frames completed (lockstep)
    int hist_len, cur, acc_cur; DevBuf<> d_hist[2]; DevBuf<float> d_w; DevBuf<float2> d_tw; DevBuf<float> d_acc; DevBuf<WfSeg> d_segs; int segs_cap;   // d_acc: two [stream][N] buffers
    DevBuf<float2> d_frames; size_t frames_cap; DevBuf<int16_t> d_q; size_t q_cap; std::map<int, FftPlan> plans;
};

namespace {

bool real_format(int in_format) { return in_format == CSDR_AMD_WF_IN_F32 || in_format == CSDR_AMD_WF_IN_S16; }
bool known_format(int in_format) { return in_format == CSDR_AMD_WF_IN_CF32 || in_format == CSDR_AMD_WF_IN_U8 || real_format(in_format); }
int elem_bytes(int in_format) { return in_format == CSDR_AMD_WF_IN_U8 || in_format == CSDR_AMD_WF_IN_S16 ? 2 : in_format == CSDR_AMD_WF_IN_F32 ? 4 : 8; }

// fft_cc's schedule in complex samples, fft_fc's in real ones (the header of this file): len, period, off
void wf_schedule(int fft, int every, bool real, int *len, int *period, int *off)
{
    *len = real ? 2 * fft : fft;
    *period = real && every > *len ? 2 * every - *len : every;
    *off = every < *len ? every - *len : 0;
}
// frames completed by the first `total` units: frame k ends at k period + off + len
long long frames_by(long long total, int len, int period, int off)
{
    const long long first_end = (long long)off + len;
    return total < first_end ? 0 : (total - first_end) / period + 1;
}

// the call's frames [k0, k1) grouped by row
void make_segments(const csdr_amd_waterfall *w, long long k0, long long k1, std::vector<WfSeg> &segs, int *rows)
{
    segs.clear(); *rows = 0;
    for (long long k = k0; k < k1;) {
        const long long row = k / w->avg, row_end = (row + 1) * w->avg;
        const long long e = row_end < k1 ? row_end : k1;
        WfSeg g; g.k0 = k; g.n = (int)(e - k); g.frame0 = (int)(k - k0);
        g.flags = (k % w->avg ? WF_LOAD : 0) | (e == row_end ? WF_EMIT : 0);
        g.row = (g.flags & WF_EMIT) ? (*rows)++ : -1;
        segs.push_back(g);
        k = e;
    }
}

int run_onepass(csdr_amd_waterfall *w, const WfArgs &a, int n_segs, int rows)
{
    csdr_amd_ctx *c = w->c;
    void *k = nullptr;
    // The compressor is one lane walking the row.  The real 8192-bin form's workgroup (8 waves at ~240 registers) holds a CU alone, so inside the kernel
    // the rows of a CU are compressed one after the other (measured: 5.2 ms per step where the transform takes 0.2 ms); that form writes dB rows to
    // scratch and k_wf_post's stand-alone mode compresses them, one small workgroup per row, many per CU -- the same db_to_short and encoder, the same bytes.
    const bool split_tail = real_format(w->in_format) && w->fft == 8192 && w->out_format == CSDR_AMD_WF_OUT_ADPCM && rows > 0;
    const size_t cells = (size_t)w->n_streams * rows * w->fft;
    if (split_tail) {
        if (4 * cells > w->frames_cap) {
            w->d_frames.reset(); w->frames_cap = 4 * cells;
            w->d_frames.reset((float2 *)csdr_amd_malloc(c, w->frames_cap));
            if (!w->d_frames) { w->frames_cap = 0; return fail_msg(-2, "waterfall: row buffer allocation failed"); }
        }
        if (2 * cells > w->q_cap) {
            w->d_q.reset(); w->q_cap = 2 * cells; w->d_q.reset((int16_t *)csdr_amd_malloc(c, w->q_cap));
            if (!w->d_q) { w->q_cap = 0; return fail_msg(-2, "waterfall: scratch allocation failed"); }
        }
    }
    size_t lds = 0; int threads = w->fft / 16;
    switch (w->fft) {
        case 1024: k = onepass_kernel<1024>(w->in_format); lds = WfGeom<1024>::LDS_BYTES; break;
        case 2048: k = onepass_kernel<2048>(w->in_format); lds = WfGeom<2048>::LDS_BYTES; break;
        case 4096: k = onepass_kernel<4096>(w->in_format); lds = WfGeom<4096>::LDS_BYTES; break;
        default:   k = onepass_kernel<8192>(w->in_format); lds = WfGeom<8192>::LDS_BYTES; break;
    }
    if (lds_attr_once(k, lds) < 0) return -5;
    WfArgs aa = a;
    if (split_tail) { aa.out = w->d_frames.get(); aa.out_pitch = 4 * (size_t)rows * w->fft; aa.out_format = CSDR_AMD_WF_OUT_DB; }
    void *args[] = {&aa};
    CSDR_HIP(hipLaunchKernel(k, dim3((unsigned)n_segs, (unsigned)w->n_streams), dim3(threads), args, lds, c->stream));
    if (split_tail) {
        hipLaunchKernelGGL(k_wf_post<false>, dim3(rows, w->n_streams), dim3(256), 0, c->stream, (const void *)w->d_frames.get(), w->fft, rows, 1, (const WfSeg *)nullptr,
                           (const float *)nullptr, (float *)nullptr, a.out, a.out_pitch, (int)CSDR_AMD_WF_OUT_ADPCM, 0.f, 0, 0, w->d_q.get(), (const float2 *)nullptr);
        CSDR_LAUNCH_CHECK();
    }
    return 0;
}

int run_generic(csdr_amd_waterfall *w, const WfArgs &a, long long k0, int n_frames, int n_segs)
{
    csdr_amd_ctx *c = w->c;
    const int N = w->fft;
    const bool real = real_format(w->in_format);
    if (n_frames > 65535) return fail_msg(-3, "waterfall: %d frames in one call on the generic path (at most 65535: pass fewer samples per call)", n_frames);
    // streams per group: the frames of a group stay within ~256 MiB
    const size_t per_stream = (size_t)n_frames * N * 8;
    const size_t fit = ((size_t)256 << 20) / per_stream;
    const int group = fit < 1 ? 1 : fit > (size_t)w->n_streams ? w->n_streams : (int)fit;
    // one plan of a fixed batch (about 2 Mi points per execution) for every call: hipFFT picks its kernels by batch count, and rows must not depend on how
    // the stream was cut into calls; the frame buffer is padded to whole plan batches (the padding's transforms are never read)
    const int pb = plan_batch(N);
    const size_t need = ((size_t)group * n_frames + pb - 1) / pb * pb * N * 8;
    if (need > w->frames_cap) {
        w->d_frames.reset(); w->frames_cap = need;
        w->d_frames.reset((float2 *)csdr_amd_malloc(c, w->frames_cap));
        if (!w->d_frames) { w->frames_cap = 0; return fail_msg(-2, "waterfall: frame buffer allocation failed"); }
    }
    if (w->out_format == CSDR_AMD_WF_OUT_ADPCM) {
        const size_t q = (size_t)group * n_segs * N * 2;
        if (q > w->q_cap) {
            w->d_q.reset(); w->q_cap = q; w->d_q.reset((int16_t *)csdr_amd_malloc(c, q));
            if (!w->d_q) { w->q_cap = 0; return fail_msg(-2, "waterfall: scratch allocation failed"); }
        }
    }
    if (!w->plans.count(pb)) {
        hipfftHandle h; int n[1] = {N};
        if (hipfftPlanMany(&h, 1, n, nullptr, 1, N, nullptr, 1, N, HIPFFT_C2C, pb) != HIPFFT_SUCCESS) return fail_msg(-5, "waterfall: hipfftPlanMany(%d x %d) failed", N, pb);
        w->plans[pb].reset(h);
        hipfftSetStream(h, c->stream);
    }
    for (int s0 = 0; s0 < w->n_streams; s0 += group) {
        const int g = s0 + group <= w->n_streams ? group : w->n_streams - s0;
        const unsigned gx = cdiv(N, 256) > 16 ? 16 : cdiv(N, 256);
        if (w->in_format == CSDR_AMD_WF_IN_U8) hipLaunchKernelGGL(k_wf_frame<1>, dim3(gx, n_frames, g), dim3(256), 0, c->stream, a, N, k0, n_frames, w->d_frames.get(), s0);
        else if (w->in_format == CSDR_AMD_WF_IN_F32) hipLaunchKernelGGL(k_wf_frame<2>, dim3(gx, n_frames, g), dim3(256), 0, c->stream, a, N, k0, n_frames, w->d_frames.get(), s0);
        else if (w->in_format == CSDR_AMD_WF_IN_S16) hipLaunchKernelGGL(k_wf_frame<3>, dim3(gx, n_frames, g), dim3(256), 0, c->stream, a, N, k0, n_frames, w->d_frames.get(), s0);
        else hipLaunchKernelGGL(k_wf_frame<0>, dim3(gx, n_frames, g), dim3(256), 0, c->stream, a, N, k0, n_frames, w->d_frames.get(), s0);
        CSDR_LAUNCH_CHECK();
        const size_t used = (size_t)g * n_frames, padded = (used + pb - 1) / pb * pb;
        if (padded > used) CSDR_HIP(hipMemsetAsync(w->d_frames.get() + used * N, 0, (padded - used) * N * 8, c->stream));   // (defined values in the plan's idle slots)
        for (size_t f = 0; f < used; f += pb) {
            hipfftComplex *z = (hipfftComplex *)(w->d_frames.get() + f * N);
            if (hipfftExecC2C(w->plans[pb].get(), z, z, HIPFFT_FORWARD) != HIPFFT_SUCCESS) return fail_msg(-5, "waterfall: hipfftExecC2C failed");
        }
        hipLaunchKernelGGL(k_wf_post<true>, dim3(n_segs, g), dim3(256), 0, c->stream, (const void *)w->d_frames.get(), N, n_frames, w->avg, a.segs, a.acc_in, a.acc_out, a.out, a.out_pitch,
                           w->out_format, a.add_db, real ? 0 : 1, s0, w->out_format == CSDR_AMD_WF_OUT_ADPCM ? w->d_q.get() : nullptr, real ? a.table + N : (const float2 *)nullptr);
        CSDR_LAUNCH_CHECK();
    }
    return 0;
}

// the CPU run of the one-pass stages for row `row` of a stream given from its start (csdr_amd_debug_waterfall_row / _row_at)
template <int N, int IN>
void host_row(int period, int off, int row, const float *window, int avg, float add_db, const void *in, float *db_row, float *power_row)
{
    constexpr int T = WfGeom<N>::T, NP = WfPlan<N>::NP;
    constexpr bool REAL = wf_real<IN>();
    std::vector<float2> table; twiddle_table(N, table);
    if (REAL) half_table(N, table);
    std::vector<float2> lds(WfGeom<N>::DATA);
    std::vector<WfConst<N>> cst(T);
    std::vector<std::array<float2, 16>> v(T);
    std::vector<std::array<float, 16>> acc(T);
    for (int t = 0; t < T; t++) { wf_const<N>(t, table.data(), cst[t]); acc[t].fill(0.f); }
    auto as_regs = [](std::array<float2, 16> &a) -> float2 (&)[16] { return *reinterpret_cast<float2 (*)[16]>(a.data()); };
    for (int f = 0; f < avg; f++) {
        const long long start = ((long long)row * avg + f) * period + off;
        for (int t = 0; t < T; t++) {
            float2 (&r)[16] = as_regs(v[t]);
            for (int s = 0; s < 16; s++) {
                if constexpr (REAL) r[s] = wf_packed<IN>(in, nullptr, 0, 0, start, WfPass<N, 0>::src(t, s), window);
                else r[s] = wf_windowed<IN>(in, nullptr, 0, 0, start + WfPass<N, 0>::src(t, s), window[WfPass<N, 0>::src(t, s)]);
            }
            WfPass<N, 0>::compute(r, cst[t].w1);
            WfPass<N, 0>::lds_write(lds.data(), t, r);
        }
        for (int t = 0; t < T; t++) { WfPass<N, 1>::lds_read(lds.data(), t, as_regs(v[t])); WfPass<N, 1>::compute(as_regs(v[t]), cst[t].w1); }
        for (int t = 0; t < T; t++) WfPass<N, 1>::lds_write(lds.data(), t, as_regs(v[t]));
        for (int t = 0; t < T; t++) { WfPass<N, 2>::lds_read(lds.data(), t, as_regs(v[t])); WfPass<N, 2>::compute(as_regs(v[t]), cst[t].w2); }
        if constexpr (NP > 3) {
            for (int t = 0; t < T; t++) WfPass<N, 2>::lds_write(lds.data(), t, as_regs(v[t]));
            for (int t = 0; t < T; t++) { WfPass<N, 3>::lds_read(lds.data(), t, as_regs(v[t])); WfPass<N, 3>::compute(as_regs(v[t]), cst[t].w3); }
        }
        if constexpr (REAL) {
            for (int t = 0; t < T; t++) WfPass<N, NP - 1>::lds_write(lds.data(), t, as_regs(v[t]));
            for (int t = 0; t < T; t++) wf_untangle<N>(lds.data(), t, table.data() + N, as_regs(v[t]));
        }
        for (int t = 0; t < T; t++) wf_accumulate<N>(as_regs(v[t]), *reinterpret_cast<float (*)[16]>(acc[t].data()));
    }
    for (int t = 0; t < T; t++)
        for (int s = 0; s < 16; s++) {
            const int o = (wf_bin<N>(t, s) + (REAL ? 0 : N / 2)) & (N - 1);
            if (db_row) db_row[o] = wf_db(acc[t][s], add_db);
            if (power_row) power_row[o] = acc[t][s];
        }
}

template <int N>
void host_row_of(int in_format, int period, int off, int row, const float *window, int avg, float add_db, const void *in, float *db_row, float *power_row)
{
    if (in_format == CSDR_AMD_WF_IN_U8) host_row<N, 1>(period, off, row, window, avg, add_db, in, db_row, power_row);
    else if (in_format == CSDR_AMD_WF_IN_F32) host_row<N, 2>(period, off, row, window, avg, add_db, in, db_row, power_row);
    else if (in_format == CSDR_AMD_WF_IN_S16) host_row<N, 3>(period, off, row, window, avg, add_db, in, db_row, power_row);
    else host_row<N, 0>(period, off, row, window, avg, add_db, in, db_row, power_row);
}

} // namespace

extern "C" {

csdr_amd_waterfall *csdr_amd_waterfall_create(csdr_amd_ctx *c, int fft_size, int every_n_samples, int window, int avgnumber, float add_db, int in_format, int out_format,
                                              int n_streams, size_t max_samples_per_call)
{
    if (fft_size < 2 || (fft_size & (fft_size - 1)) || every_n_samples <= 0 || avgnumber <= 0 || n_streams <= 0 || !max_samples_per_call ||
        every_n_samples > (1 << 29) || fft_size > (1 << 29) || !known_format(in_format) || (out_format != CSDR_AMD_WF_OUT_DB && out_format != CSDR_AMD_WF_OUT_ADPCM)) {
        fail_msg(-3, "waterfall: fft_size must be a power of two >= 2; every_n, avgnumber, n_streams, max_samples_per_call positive; formats CSDR_AMD_WF_*");
        return nullptr;
    }
    Owned<csdr_amd_waterfall, csdr_amd_waterfall_destroy> w(new csdr_amd_waterfall());
    w->c = c; w->fft = fft_size; w->every = every_n_samples; w->avg = avgnumber; w->in_format = in_format; w->out_format = out_format; w->n_streams = n_streams;
    w->add_db = (float)(add_db - 10.0 * log10((double)avgnumber));                // csdr.c:1678
    w->max_in = max_samples_per_call; w->onepass = onepass_size(fft_size); w->force_generic = false; w->last_kernel = "";
    const bool real = real_format(in_format);
    wf_schedule(fft_size, every_n_samples, real, &w->len, &w->period, &w->off);
    w->total = 0; w->frames_done = 0; w->cur = 0; w->hist_len = w->len;
    const size_t hb = (size_t)n_streams * w->len * elem_bytes(in_format);
    w->d_hist[0].reset(csdr_amd_malloc(c, hb + 256)); w->d_hist[1].reset(csdr_amd_malloc(c, hb + 256));
    w->d_w.reset((float *)csdr_amd_malloc(c, 4 * (size_t)w->len));
    w->d_tw.reset((float2 *)csdr_amd_malloc(c, 8 * (size_t)w->len));
    w->d_acc.reset((float *)csdr_amd_malloc(c, 2 * 4 * (size_t)n_streams * fft_size));
    if (!w->d_hist[0] || !w->d_hist[1] || !w->d_w || !w->d_tw || !w->d_acc) return nullptr;
    std::vector<float> win(w->len); csdr_amd_precalculate_window(win.data(), w->len, window);
    std::vector<float2> tw; twiddle_table(fft_size, tw);
    if (real) half_table(fft_size, tw);
    if (csdr_amd_h2d(c, w->d_w.get(), win.data(), 4 * win.size()) < 0 || csdr_amd_h2d(c, w->d_tw.get(), tw.data(), 8 * tw.size()) < 0 ||
        csdr_amd_waterfall_reset(w.get()) < 0) return nullptr;
    return w.release();
}

int csdr_amd_waterfall_reset(csdr_amd_waterfall *w)
{
    // (history positions before the stream's start are read as zeros whatever the buffer holds: wf_windowed)
    w->total = 0; w->frames_done = 0; w->cur = 0; w->acc_cur = 0;
    const size_t hb = (size_t)w->n_streams * w->len * elem_bytes(w->in_format);
    if (csdr_amd_memset(w->c, w->d_hist[0].get(), 0, hb) < 0) return -5;
    return 0;
}

const char *csdr_amd_waterfall_kernel_name(const csdr_amd_waterfall *w) { return w ? w->last_kernel : ""; }
int csdr_amd_waterfall_force_generic(csdr_amd_waterfall *w, int on) { if (!w) return -3; w->force_generic = on != 0; return 0; }

void csdr_amd_waterfall_destroy(csdr_amd_waterfall *w)
{
    if (!w) return;
    (void)hipSetDevice(w->c->device);
    delete w;
}

int csdr_amd_waterfall_process(csdr_amd_waterfall *w, const void *in, size_t n_in, size_t in_pitch, void *out, size_t out_pitch, int *rows_out)
{
    if (rows_out) *rows_out = 0;
    if (!w) return fail_msg(-3, "waterfall: null object");
    if (n_in > w->max_in) return fail_msg(-3, "waterfall: %zu samples per call, the object was created for at most %zu", n_in, w->max_in);
    if (!n_in) return 0;
    if (in_pitch < n_in) return fail_msg(-3, "waterfall: in_pitch must be >= n_in");
    csdr_amd_ctx *c = w->c;
    const long long k0 = w->frames_done, k1 = frames_by(w->total + (long long)n_in, w->len, w->period, w->off);
    std::vector<WfSeg> segs; int rows = 0;
    make_segments(w, k0, k1, segs, &rows);
    const size_t row_bytes = w->out_format == CSDR_AMD_WF_OUT_DB ? 4 * (size_t)w->fft : (size_t)(w->fft + 10) / 2;
    if (rows && out_pitch < (size_t)rows * row_bytes && w->n_streams > 1) return fail_msg(-3, "waterfall: out_pitch %zu below the %d rows of %zu bytes of this call", out_pitch, rows, row_bytes);
    WfArgs a;
    a.in = in; a.in_pitch = in_pitch; a.hist = w->d_hist[w->cur].get(); a.hist_new = w->d_hist[w->cur ^ 1].get(); a.hist_len = w->hist_len;
    a.base = w->total; a.every = w->period; a.off = w->off;
    a.window = w->d_w.get(); a.table = w->d_tw.get();
    a.acc_in = w->d_acc.get() + (size_t)w->acc_cur * w->n_streams * w->fft; a.acc_out = w->d_acc.get() + (size_t)(w->acc_cur ^ 1) * w->n_streams * w->fft; a.out = out; a.out_pitch = out_pitch; a.out_format = w->out_format; a.add_db = w->add_db;
    if (!segs.empty()) {
        if ((int)segs.size() > w->segs_cap) {
            w->d_segs.reset(); w->segs_cap = (int)segs.size() + 64;
            w->d_segs.reset((WfSeg *)csdr_amd_malloc(c, sizeof(WfSeg) * w->segs_cap));
            if (!w->d_segs) { w->segs_cap = 0; return fail_msg(-2, "waterfall: segment table allocation failed"); }
        }
        void *h = c->pinned_acquire(sizeof(WfSeg) * segs.size());
        if (!h) return fail_msg(-2, "waterfall: pinned staging failed");
        memcpy(h, segs.data(), sizeof(WfSeg) * segs.size());
        if (c->pinned_upload(w->d_segs.get(), sizeof(WfSeg) * segs.size()) < 0) return -5;
        a.segs = w->d_segs.get();
        const bool onepass = w->onepass && !w->force_generic;
        const int rc = onepass ? run_onepass(w, a, (int)segs.size(), rows) : run_generic(w, a, k0, (int)(k1 - k0), (int)segs.size());
        if (rc < 0) return rc;
        w->acc_cur ^= 1;
        w->last_kernel = !onepass ? (real_format(w->in_format) ? "k_wf_post (generic real: framing + hipFFT + untangle)" : "k_wf_post (generic: framing + hipFFT)") :
                         w->in_format == CSDR_AMD_WF_IN_U8 ? "k_wf_onepass (u8)" : w->in_format == CSDR_AMD_WF_IN_F32 ? "k_wf_onepass_real (f32)" :
                         w->in_format == CSDR_AMD_WF_IN_S16 ? "k_wf_onepass_real (s16)" : "k_wf_onepass (cf32)";
    }
    // the history moves on by n_in samples (after every read of the old one: same stream)
    const size_t eb = elem_bytes(w->in_format), hb = (size_t)w->hist_len * eb;
    hipLaunchKernelGGL(k_wf_hist, dim3(cdiv(hb / 2, 256) > 64 ? 64 : cdiv(hb / 2, 256), (unsigned)w->n_streams), dim3(256), 0, c->stream,
                       (const uint8_t *)in, in_pitch * eb, (const uint8_t *)w->d_hist[w->cur].get(), (uint8_t *)w->d_hist[w->cur ^ 1].get(), hb, n_in * eb);
    CSDR_LAUNCH_CHECK();
    w->cur ^= 1;
    w->total += (long long)n_in; w->frames_done = k1;
    if (rows_out) *rows_out = rows;
    return rows;
}

int csdr_amd_logaveragepower_cf(csdr_amd_ctx *c, const csdr_complexf *in, float *out, int n_rows, int fft_size, int avgnumber, float add_db)
{
    if (n_rows <= 0) return 0;
    if (fft_size < 2 || (fft_size & (fft_size - 1)) || avgnumber <= 0) return fail_msg(-3, "logaveragepower_cf: fft_size must be a power of two >= 2, avgnumber positive");
    const float a = (float)(add_db - 10.0 * log10((double)avgnumber));     // csdr.c:1678
    // one "stream" whose segments are the n_rows rows, no swap
    hipLaunchKernelGGL(k_wf_post<true>, dim3(n_rows, 1), dim3(256), 0, c->stream, (const void *)in, fft_size, n_rows * avgnumber, avgnumber, (const WfSeg *)nullptr,
                       (const float *)nullptr, (float *)nullptr, (void *)out, (size_t)0, (int)CSDR_AMD_WF_OUT_DB, a, 0, 0, (int16_t *)nullptr, (const float2 *)nullptr);
    CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_fft_exchange_sides_ff(csdr_amd_ctx *c, const float *in, float *out, int n_rows, int fft_size)
{
    if (n_rows <= 0) return 0;
    if (fft_size < 2 || (fft_size & (fft_size - 1))) return fail_msg(-3, "fft_exchange_sides_ff: fft_size must be a power of two >= 2");
    hipLaunchKernelGGL(k_wf_post<false>, dim3(n_rows, 1), dim3(256), 0, c->stream, (const void *)in, fft_size, n_rows, 1, (const WfSeg *)nullptr,
                       (const float *)nullptr, (float *)nullptr, (void *)out, (size_t)0, (int)CSDR_AMD_WF_OUT_DB, 0.f, 1, 0, (int16_t *)nullptr, (const float2 *)nullptr);
    CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_accumulate_power_cf(csdr_amd_ctx *c, const csdr_complexf *in, float *acc_io, size_t n)
{
    if (!n) return 0;
    hipLaunchKernelGGL(k_accumulate_power, dim3(cdiv(n, 256) > 4096 ? 4096 : cdiv(n, 256)), dim3(256), 0, c->stream, in, acc_io, n); CSDR_LAUNCH_CHECK();
    return 0;
}
int csdr_amd_log_ff(csdr_amd_ctx *c, const float *in, float *out, size_t n, float add_db)
{
    if (!n) return 0;
    hipLaunchKernelGGL(k_log_ff, dim3(cdiv(n, 256) > 4096 ? 4096 : cdiv(n, 256)), dim3(256), 0, c->stream, in, out, n, add_db); CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_debug_waterfall_row(int fft_size, int every_n_samples, int window, int avgnumber, float add_db, int in_format, const void *in, long long n_in,
                                 float *db_row, float *power_row)
{
    return csdr_amd_debug_waterfall_row_at(fft_size, every_n_samples, window, avgnumber, add_db, in_format, in, n_in, 0, db_row, power_row);
}

int csdr_amd_debug_waterfall_row_at(int fft_size, int every_n_samples, int window, int avgnumber, float add_db, int in_format, const void *in, long long n_in,
                                    int row, float *db_row, float *power_row)
{
    if (row < 0 || !onepass_size(fft_size) || every_n_samples <= 0 || every_n_samples > (1 << 29) || avgnumber <= 0 || !known_format(in_format)) return -3;
    int len, period, off;
    wf_schedule(fft_size, every_n_samples, real_format(in_format), &len, &period, &off);
    if (n_in < ((long long)(row + 1) * avgnumber - 1) * period + off + len) return -3;   // the row's last frame must be complete
    std::vector<float> win(len); csdr_amd_precalculate_window(win.data(), len, window);
    const float a = (float)(add_db - 10.0 * log10((double)avgnumber));
    switch (fft_size) {
        case 1024: host_row_of<1024>(in_format, period, off, row, win.data(), avgnumber, a, in, db_row, power_row); break;
        case 2048: host_row_of<2048>(in_format, period, off, row, win.data(), avgnumber, a, in, db_row, power_row); break;
        case 4096: host_row_of<4096>(in_format, period, off, row, win.data(), avgnumber, a, in, db_row, power_row); break;
        default:   host_row_of<8192>(in_format, period, off, row, win.data(), avgnumber, a, in, db_row, power_row); break;
    }
    return 0;
}

} // extern "C"

// ------------------------------------------------------------------ fft_fc and fft_one_side_ff as stand-alone stages (csdr.c:3414-3498, 1717-1734)
namespace {

// spectra of packed frames -> the first fft bins of the real frames' spectra: out[f][k] from Z[f][k] and Z[f][(fft - k) mod fft]
__global__ __launch_bounds__(256) void k_fftfc_untangle(const float2 *__restrict__ z, float2 *__restrict__ out, int fft, const float2 *__restrict__ half)
{
    const float2 *zf = z + (size_t)blockIdx.y * fft;
    float2 *o = out + (size_t)blockIdx.y * fft;
    for (int k = blockIdx.x * 256 + threadIdx.x; k < fft; k += gridDim.x * 256) o[k] = wf_untangle1(zf[k], zf[(fft - k) & (fft - 1)], half[k]);
}
__global__ __launch_bounds__(256) void k_one_side(const float *__restrict__ in, float *__restrict__ out, int half_size, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = in[i / half_size * 2 * half_size + i % half_size];
}

} // namespace

// one stream: the schedule, the sliding buffer (the last 2M floats) and the samples still to skip are the waterfall object's, without the row stage
struct csdr_amd_fftfc {
    csdr_amd_ctx *c; int fft, len, period, off, pb; size_t max_in, max_frames;
    long long total, frames_done; int cur;
    DevBuf<float> d_hist[2]; DevBuf<float> d_w; DevBuf<float2> d_half; DevBuf<float2> d_frames; FftPlan plan;
};

extern "C" {

csdr_amd_fftfc *csdr_amd_fftfc_create(csdr_amd_ctx *c, int fft_out_size, int every_n_samples, int window, size_t max_samples_per_call)
{
    if (fft_out_size < 2 || (fft_out_size & (fft_out_size - 1)) || fft_out_size > (1 << 29) || every_n_samples <= 0 || every_n_samples > (1 << 29) || !max_samples_per_call) {
        fail_msg(-3, "fft_fc: fft_out_size must be a power of two >= 2, every_n and max_samples_per_call positive");
        return nullptr;
    }
    Owned<csdr_amd_fftfc, csdr_amd_fftfc_destroy> f(new csdr_amd_fftfc());
    f->c = c; f->fft = fft_out_size; f->max_in = max_samples_per_call; f->total = 0; f->frames_done = 0; f->cur = 0;
    wf_schedule(fft_out_size, every_n_samples, true, &f->len, &f->period, &f->off);
    f->max_frames = (max_samples_per_call + f->period - 1) / f->period;
    if (f->max_frames > 65535) { fail_msg(-3, "fft_fc: %zu frames per call (at most 65535: fewer samples per call)", f->max_frames); return nullptr; }
    // the generic waterfall's plan (one fixed batch for every call: spectra must not depend on how the stream is cut into calls, and they are the
    // spectra that object sums); the frame buffer holds whole batches
    f->pb = plan_batch(fft_out_size);
    const size_t frames_cap = (f->max_frames + f->pb - 1) / f->pb * f->pb * (size_t)f->fft;
    f->d_hist[0].reset((float *)csdr_amd_malloc(c, 4 * (size_t)f->len)); f->d_hist[1].reset((float *)csdr_amd_malloc(c, 4 * (size_t)f->len));
    f->d_w.reset((float *)csdr_amd_malloc(c, 4 * (size_t)f->len));
    f->d_half.reset((float2 *)csdr_amd_malloc(c, 8 * (size_t)f->fft));
    f->d_frames.reset((float2 *)csdr_amd_malloc(c, 8 * frames_cap));
    if (!f->d_hist[0] || !f->d_hist[1] || !f->d_w || !f->d_half || !f->d_frames) return nullptr;
    std::vector<float> win(f->len); csdr_amd_precalculate_window(win.data(), f->len, window);
    std::vector<float2> half; half_table(f->fft, half);
    if (csdr_amd_h2d(c, f->d_w.get(), win.data(), 4 * win.size()) < 0 || csdr_amd_h2d(c, f->d_half.get(), half.data(), 8 * half.size()) < 0 ||
        csdr_amd_memset(c, f->d_hist[0].get(), 0, 4 * (size_t)f->len) < 0 || csdr_amd_memset(c, f->d_frames.get(), 0, 8 * frames_cap) < 0) return nullptr;
    hipfftHandle h; int n[1] = {f->fft};
    if (hipfftPlanMany(&h, 1, n, nullptr, 1, f->fft, nullptr, 1, f->fft, HIPFFT_C2C, f->pb) != HIPFFT_SUCCESS) { fail_msg(-5, "fft_fc: hipfftPlanMany(%d x %d) failed", f->fft, f->pb); return nullptr; }
    f->plan.reset(h);
    hipfftSetStream(h, c->stream);
    return f.release();
}

void csdr_amd_fftfc_destroy(csdr_amd_fftfc *f)
{
    if (!f) return;
    (void)hipSetDevice(f->c->device);
    delete f;
}

int csdr_amd_fftfc_process(csdr_amd_fftfc *f, const float *in, size_t n_in, csdr_complexf *out)
{
    if (!f) return fail_msg(-3, "fft_fc: null object");
    if (n_in > f->max_in) return fail_msg(-3, "fft_fc: %zu samples per call, the object was created for at most %zu", n_in, f->max_in);
    if (!n_in) return 0;
    csdr_amd_ctx *c = f->c;
    const long long k0 = f->frames_done, k1 = frames_by(f->total + (long long)n_in, f->len, f->period, f->off);
    const int n_frames = (int)(k1 - k0), M = f->fft;
    if (n_frames > 0) {
        WfArgs a = {};
        a.in = in; a.in_pitch = n_in; a.hist = f->d_hist[f->cur].get(); a.hist_len = f->len; a.base = f->total; a.every = f->period; a.off = f->off; a.window = f->d_w.get();
        const unsigned gx = cdiv(M, 256) > 16 ? 16 : cdiv(M, 256);
        hipLaunchKernelGGL(k_wf_frame<CSDR_AMD_WF_IN_F32>, dim3(gx, n_frames, 1), dim3(256), 0, c->stream, a, M, k0, n_frames, f->d_frames.get(), 0);
        CSDR_LAUNCH_CHECK();
        for (int g = 0; g < n_frames; g += f->pb) {
            hipfftComplex *z = (hipfftComplex *)(f->d_frames.get() + (size_t)g * M);
            if (hipfftExecC2C(f->plan.get(), z, z, HIPFFT_FORWARD) != HIPFFT_SUCCESS) return fail_msg(-5, "fft_fc: hipfftExecC2C failed");
        }
        hipLaunchKernelGGL(k_fftfc_untangle, dim3(gx, n_frames), dim3(256), 0, c->stream, (const float2 *)f->d_frames.get(), (float2 *)out, M, (const float2 *)f->d_half.get());
        CSDR_LAUNCH_CHECK();
    }
    const size_t hb = 4 * (size_t)f->len;
    hipLaunchKernelGGL(k_wf_hist, dim3(cdiv(hb / 2, 256) > 64 ? 64 : cdiv(hb / 2, 256), 1), dim3(256), 0, c->stream,
                       (const uint8_t *)in, n_in * 4, (const uint8_t *)f->d_hist[f->cur].get(), (uint8_t *)f->d_hist[f->cur ^ 1].get(), hb, n_in * 4);
    CSDR_LAUNCH_CHECK();
    f->cur ^= 1;
    f->total += (long long)n_in; f->frames_done = k1;
    return n_frames;
}

int csdr_amd_fft_one_side_ff(csdr_amd_ctx *c, const float *in, float *out, int n_rows, int fft_size)
{
    if (n_rows <= 0) return 0;
    if (fft_size < 2 || (fft_size & 1)) return fail_msg(-3, "fft_one_side_ff: fft_size must be even and >= 2");
    const size_t n = (size_t)n_rows * (fft_size / 2);
    hipLaunchKernelGGL(k_one_side, dim3(cdiv(n, 256) > 4096 ? 4096 : cdiv(n, 256)), dim3(256), 0, c->stream, in, out, fft_size / 2, n); CSDR_LAUNCH_CHECK();
    return 0;
}

} // extern "C"
