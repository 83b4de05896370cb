// cfir.hip -- the complex-tap FIR for n_channels channels per call (MI355X / gfx950): apply_fir_cc libcsdr.c:2261-2273 with its own taps per channel,
// as the stateless call csdr_amd_apply_fir_cc and as the bank object csdr_amd_cfir_* (history kept on the device, taps retunable between calls;
// peaks_fir_cc csdr.c:2975-3016 is the object with set_peaks).  cfir_dev.hpp holds the definition: each part of an output is one fmaf chain over the
// 2 T interleaved tap floats.
//
// 8 T flops against 16 bytes per output: the arithmetic binds, and it is fp32.  k_cfir_mfma runs it on the fp32 matrix cores as the Toeplitz-band
// product of k_bfsk_mfma (rtty.hip) with two output parts instead of four, C_c[i][n] = sum_k A_c[i][k] B[k][n]:
//   A_c[i][k] = a_c[k - 2 i]             the interleaved taps of part c (re, im) of the wave's OWN channel, zero outside [0, 2 T)
//   B[k][n]   = xf[32 n + k]             the staged window, interleaved floats: column n = 16 consecutive outputs
// so C_c[i][n] is part c of output 16 n + i.  Both parts share each B operand.  A wave takes two column blocks per tile (512 outputs) as the discriminator
// does: with half its accumulators the kernel needs 108 registers, four waves per SIMD.  (Three and four column blocks cut the A reads per product and
// the window's halo per output, but need 139 and 168 registers, three waves, and measured slower at 31 and 101 taps: DESIGN 4r.)  v_mfma_f32_16x16x4_f32 is a k-ordered fmaf
// chain and each accumulator covers the whole K range, so every output part is the single chain of cfir_output: same bits, wherever a call starts.
// The C layout leaves both parts of four consecutive outputs in one lane: they leave as two 16-byte stores where the row is 16-byte aligned.
#include "bank.hpp"
#include "cfir_dev.hpp"
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>

using namespace csdr_amd;

namespace {

static_assert(sizeof(CfirChan) == 4, "CfirChan is one int");

// V(p) of channel ch: its history (h samples) then its input
struct VRow {
    const float2 *hist; const float2 *in; int h;
    __device__ float2 operator()(long long p) const { return p < h ? hist[p] : in[p - h]; }
};

constexpr int CF_NB = 2;                        // column blocks of 16 groups per wave and tile (3 and 4 measured slower at 31 and 101 taps)
constexpr int CF_TO = 256 * CF_NB;              // outputs per tile: 512
constexpr int CF_MAXT = 256;                    // longest filter on the matrix cores (the window below stays within CF_MAXP samples per lane)
constexpr int CF_MAX_TAPS = 65536;              // longest filter at all
constexpr long long CF_MAX_CELLS = 1LL << 27;   // n_channels x taps_length: the taps and the history are buffers of that many samples (1 GiB each)
__host__ __device__ constexpr int cf_steps(int T) { return (2 * T + 30 + 3) / 4; }                         // K steps of 4: tap floats and the band's 30 zeros in front
__host__ __device__ constexpr int cf_wf(int T) { return 32 * (16 * CF_NB - 1) + 4 * cf_steps(T) + 4; }     // window floats read
__host__ __device__ constexpr int cf_ws(int T) { return (cf_wf(T) + 1) / 2; }                             // window samples staged
__host__ __device__ constexpr int cf_hz(int T) { return 4 * cf_steps(T) + 32; }                            // floats per padded tap row
constexpr int CF_MAXP = (cf_ws(CF_MAXT) + 63) / 64;
__host__ __device__ inline int cf_swz(int a) { return a + 2 * (a >> 5); }  // two pad floats per 32: the 16 columns' B reads fall in 32 different banks
size_t cf_lds(int T) { return sizeof(float) * ((size_t)2 * cf_hz(T) + cf_swz(2 * cf_ws(T)) + 8); }

typedef float f32x4_mfma __attribute__((ext_vector_type(4)));

// taps: channel ch's row is taps + ch * taps_pitch (taps_pitch 0: one row for all).  amdgpu_waves_per_eu: with an occupancy target the compiler keeps the
// accumulators in VGPRs (108 VGPR + 0 AGPR) instead of AGPRs (98 + 20), four waves per SIMD either way; measured 4 % - 12 % faster.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) void k_cfir_mfma(const float2 *__restrict__ in, size_t in_pitch, long long n_in, const float2 *__restrict__ hist, int hist_cap,
                                                  const CfirChan *__restrict__ st, float2 *__restrict__ out, size_t out_pitch, const float2 *__restrict__ taps,
                                                  size_t taps_pitch, int T, int wpc, int tpw)
{
    extern __shared__ float lds_f[];
    const int S = cf_steps(T), HZ = cf_hz(T), WS = cf_ws(T);
    float *hz = lds_f;                          // 2 rows of HZ: 30 zeros, the 2 T interleaved taps, zeros
    float *xw = lds_f + 2 * HZ;                 // the window, swizzled
    const int ch = blockIdx.x / wpc, w = blockIdx.x % wpc, lane = threadIdx.x;
    const int h = st ? st[ch].hist_len : 0;
    const long long nV = h + n_in, n_out = nV - (T - 1);
    if (n_out <= 0) return;
    const long long tiles = (n_out + CF_TO - 1) / CF_TO, t0 = (long long)w * tpw, t1 = std::min(t0 + tpw, tiles);
    if (t0 >= t1) return;
    const VRow V{hist ? hist + (size_t)ch * hist_cap : nullptr, in + (size_t)ch * in_pitch, h};
    const float2 *hc = taps + (size_t)ch * taps_pitch;
    float2 nx[CF_MAXP];
    auto fetch = [&](long long tile) {
        const long long o0 = tile * CF_TO;
#pragma unroll
        for (int u = 0; u < CF_MAXP; u++) {
            const int p = 64 * u + lane;
            if (p < WS) nx[u] = o0 + p < nV ? V(o0 + p) : make_float2(0.f, 0.f);
        }
    };
    fetch(t0);
    for (int m = lane; m < 2 * HZ; m += 64) {
        const int c = m / HZ, j = m % HZ - 30;
        hz[m] = (j >= 0 && j < 2 * T) ? cfir_tap(hc, c, j) : 0.f;
    }
    const int i = lane & 15, kk = lane >> 4, n = lane & 15;
    const float *ap = hz + 30 + kk - 2 * i;                       // + c HZ + 4 s: within [0, 4 S + 30) of the row
    const int bb = 34 * n + kk;                                    // + 34 * 16 b + 4 s + 2 (s >> 3) = cf_swz(32 (16 b + n) + 4 s + kk)
    float2 *orow = out + (size_t)ch * out_pitch;
    const bool wide = ((uintptr_t)orow & 15) == 0;                 // a lane's first output is a multiple of 4: 32 bytes into the row
    for (long long tile = t0; tile < t1; tile++) {
        __syncthreads();                                           // (the previous tile's reads are done)
#pragma unroll
        for (int u = 0; u < CF_MAXP; u++) {
            const int p = 64 * u + lane;
            if (p < WS) *reinterpret_cast<float2 *>(xw + cf_swz(2 * p)) = nx[u];
        }
        __syncthreads();
        if (tile + 1 < t1) fetch(tile + 1);                        // in flight during the products
        f32x4_mfma acc[2][CF_NB];
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int b = 0; b < CF_NB; b++) acc[c][b] = (f32x4_mfma){0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < S; s++) {
            float a[2], bv[CF_NB];
#pragma unroll
            for (int c = 0; c < 2; c++) a[c] = ap[c * HZ + 4 * s];
            const int bo = bb + 4 * s + 2 * (s >> 3);
#pragma unroll
            for (int b = 0; b < CF_NB; b++) bv[b] = xw[bo + 544 * b];
#pragma unroll
            for (int b = 0; b < CF_NB; b++)
#pragma unroll
                for (int c = 0; c < 2; c++) acc[c][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], bv[b], acc[c][b], 0, 0, 0);
        }
        // C layout: column n = lane & 15 (group), row 4 (lane >> 4) + r (output within the group): outputs o .. o + 3 of a lane are consecutive
        const long long o0 = tile * CF_TO;
#pragma unroll
        for (int b = 0; b < CF_NB; b++) {
            const long long o = o0 + 16 * (16 * b + n) + 4 * kk;
            if (wide && o + 3 < n_out) {
                float4 *q = reinterpret_cast<float4 *>(orow + o);
                q[0] = make_float4(acc[0][b][0], acc[1][b][0], acc[0][b][1], acc[1][b][1]);
                q[1] = make_float4(acc[0][b][2], acc[1][b][2], acc[0][b][3], acc[1][b][3]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; r++)
                    if (o + r < n_out) orow[o + r] = make_float2(acc[0][b][r], acc[1][b][r]);
            }
        }
    }
}

// one thread per output: the same chains straight from global memory (any filter length)
__global__ __launch_bounds__(256) void k_cfir_generic(const float2 *__restrict__ in, size_t in_pitch, long long n_in, const float2 *__restrict__ hist, int hist_cap,
                                                      const CfirChan *__restrict__ st, float2 *__restrict__ out, size_t out_pitch, const float2 *__restrict__ taps,
                                                      size_t taps_pitch, int T, int bpc)
{
    const int ch = blockIdx.x / bpc;
    const long long o = (long long)(blockIdx.x % bpc) * 256 + threadIdx.x;
    const int h = st ? st[ch].hist_len : 0;
    const long long n_out = h + n_in - (T - 1);
    if (o >= n_out) return;
    const VRow V{hist ? hist + (size_t)ch * hist_cap : nullptr, in + (size_t)ch * in_pitch, h};
    out[(size_t)ch * out_pitch + o] = cfir_output(taps + (size_t)ch * taps_pitch, T, [&](int t) { return V(o + t); });
}

// after the filter: each channel's output count, and its new history (the last min(T - 1, h + n_in) samples of V)
__global__ __launch_bounds__(64) void k_cfir_hist(const float2 *__restrict__ in, size_t in_pitch, long long n_in, float2 *__restrict__ hist, int hist_cap,
                                                  CfirChan *__restrict__ st, int n_ch, int T, int *__restrict__ counts)
{
    const int ch = blockIdx.x * 64 + threadIdx.x;
    if (ch >= n_ch) return;
    CfirChan s = st[ch];
    const long long nV = s.hist_len + n_in, n_out = nV - (T - 1);
    if (counts) counts[ch] = n_out > 0 ? (int)n_out : 0;
    const int h2 = (int)std::min((long long)(T - 1), nV);
    float2 *hr = hist + (size_t)ch * hist_cap;
    const float2 *x = in + (size_t)ch * in_pitch;
    const long long from = nV - h2;
    for (int j = 0; j < h2; j++) { const long long p = from + j; hr[j] = p < s.hist_len ? hr[p] : x[p - s.hist_len]; }     // forward: p >= j
    s.hist_len = h2;
    st[ch] = s;
}

const char *g_cfir_last = "";          // the kernel behind the last csdr_amd_apply_fir_cc call

const char *cfir_kernel_for(bool generic, int T) { return !generic && T <= CF_MAXT ? "k_cfir_mfma" : "k_cfir_generic"; }

// the filter over n_ch rows: k_cfir_mfma where the filter fits, else k_cfir_generic.  0, or the error.
int launch_cfir(hipStream_t stream, bool generic, const float2 *in, size_t in_pitch, long long n_in, const float2 *hist, int hist_cap, const CfirChan *st,
                float2 *out, size_t out_pitch, const float2 *taps, size_t taps_pitch, int T, int n_ch)
{
    if (n_in <= 0) return 0;
    if (!generic && T <= CF_MAXT) {
        const long long tiles = (n_in + CF_TO - 1) / CF_TO;       // (at most: a channel has n_in + h - T + 1 <= n_in outputs)
        const int tpw = (int)std::max(1LL, std::min(16LL, tiles * n_ch / (256 * 32)));
        const long long wpc = (tiles + tpw - 1) / tpw;
        if (wpc * n_ch > 0x7fffffffLL) return fail_msg(-3, "cfir: %d channels of %lld samples are more than one launch takes", n_ch, n_in);
        hipLaunchKernelGGL(k_cfir_mfma, dim3((unsigned)(wpc * n_ch)), dim3(64), cf_lds(T), stream, in, in_pitch, n_in, hist, hist_cap, st, out, out_pitch, taps,
                           taps_pitch, T, (int)wpc, tpw);
        return 0;
    }
    const long long bpc = (n_in + 255) / 256;
    if (bpc * n_ch > 0x7fffffffLL) return fail_msg(-3, "cfir: %d channels of %lld samples are more than one launch takes", n_ch, n_in);
    hipLaunchKernelGGL(k_cfir_generic, dim3((unsigned)(bpc * n_ch)), dim3(256), 0, stream, in, in_pitch, n_in, hist, hist_cap, st, out, out_pitch, taps, taps_pitch, T,
                       (int)bpc);
    return 0;
}

int check_rows(const char *tag, const void *in, long long n, size_t in_pitch)
{
    if (n < 0 || n > (1LL << 30) || (n > 0 && (!in || in_pitch < (size_t)n))) return fail_msg(-3, "%s: need in_pitch >= n >= 0 (n <= 2^30) and an input", tag);
    if ((uintptr_t)in & 7) return fail_msg(-3, "%s: complex rows should be 8-byte aligned", tag);
    return 0;
}

// csdr.c:2997-3002: every peak added into zeroed taps, the sum normalised with the last one
void peaks_taps(std::vector<float2> &t, int T, const float *rates, int n_rates, int window)
{
    t.assign((size_t)T, make_float2(0.f, 0.f));
    for (int k = 0; k < n_rates; k++) csdr_amd_firdes_add_peak_c((csdr_complexf *)t.data(), T, rates[k], window, 1, k == n_rates - 1);
}

} // namespace

struct csdr_amd_cfir : ChanBank<CfirChan> {
    int T, hist_cap;
    DevBuf<float2> d_hist, d_taps;                 // [n_ch][hist_cap], [n_ch][T]
};

extern "C" {

csdr_amd_cfir *csdr_amd_cfir_create(csdr_amd_ctx *c, int n_channels, int taps_length)
{
    if (bank_create_check("cfir", c, n_channels) < 0) return nullptr;
    if (taps_length < 1 || taps_length > CF_MAX_TAPS) { fail_msg(-3, "cfir: taps_length should be 1 .. %d", CF_MAX_TAPS); return nullptr; }
    if ((long long)n_channels * taps_length > CF_MAX_CELLS) { fail_msg(-3, "cfir: n_channels x taps_length should be at most %lld", CF_MAX_CELLS); return nullptr; }
    Owned<csdr_amd_cfir, csdr_amd_cfir_destroy> p(new csdr_amd_cfir());
    p->c = c; p->n_ch = n_channels; p->T = taps_length;
    p->hist_cap = std::max(1, taps_length - 1);
    p->last_kernel = cfir_kernel_for(false, taps_length);
    const size_t tb = sizeof(float2) * (size_t)taps_length * n_channels;
    if (dev_alloc(p->d_st, sizeof(CfirChan) * n_channels) != hipSuccess || dev_alloc(p->d_hist, sizeof(float2) * (size_t)p->hist_cap * n_channels) != hipSuccess ||
        dev_alloc(p->d_taps, tb) != hipSuccess) { fail_msg(-2, "cfir: out of device memory"); return nullptr; }
    if (csdr_amd_memset(c, p->d_taps.get(), 0, tb) < 0 || csdr_amd_cfir_reset(p.get()) < 0) return nullptr;
    return p.release();
}

int csdr_amd_cfir_set_taps(csdr_amd_cfir *p, int channel, const csdr_complexf *host_taps)
{
    if (!p) return fail_msg(-3, "cfir: null object");
    if (!host_taps) return fail_msg(-3, "cfir: null taps");
    if (channel < -1 || channel >= p->n_ch) return fail_msg(-3, "cfir: channel out of range");
    if (channel >= 0) return csdr_amd_h2d(p->c, p->d_taps.get() + (size_t)channel * p->T, host_taps, sizeof(float2) * p->T);
    std::vector<float2> all((size_t)p->T * p->n_ch);
    for (int ch = 0; ch < p->n_ch; ch++) memcpy(all.data() + (size_t)ch * p->T, host_taps, sizeof(float2) * p->T);
    return csdr_amd_h2d(p->c, p->d_taps.get(), all.data(), sizeof(float2) * all.size());
}

int csdr_amd_cfir_set_peaks(csdr_amd_cfir *p, int channel, const float *rates, int n_rates, int window)
{
    if (!p) return fail_msg(-3, "cfir: null object");
    if (!rates) return fail_msg(-3, "cfir: null rates");
    if (n_rates < 1) return fail_msg(-3, "cfir: need at least one peak rate");
    if (channel < -1 || channel >= p->n_ch) return fail_msg(-3, "cfir: channel out of range");
    std::vector<float2> t;
    peaks_taps(t, p->T, rates, n_rates, window);
    return csdr_amd_cfir_set_taps(p, channel, (const csdr_complexf *)t.data());
}

int csdr_amd_cfir_reset(csdr_amd_cfir *p) { return bank_reset(p, "cfir", (const CfirChan *)nullptr); }
int csdr_amd_cfir_reset_channel(csdr_amd_cfir *p, int ch) { return bank_reset_channel(p, "cfir", ch, CfirChan{0}); }

long long csdr_amd_cfir_max_out(const csdr_amd_cfir *p, long long n_in) { return !p || n_in < 0 ? 0 : n_in; }     // the history holds at most T - 1 samples

int csdr_amd_cfir_process(csdr_amd_cfir *p, const csdr_complexf *in, long long n_in, size_t in_pitch, csdr_complexf *out, size_t out_pitch, int *counts)
{
    if (!p) return fail_msg(-3, "cfir: null object");
    if (check_rows("cfir", in, n_in, in_pitch) < 0) return -3;
    if (n_in > 0 && (!out || out_pitch < (size_t)n_in || ((uintptr_t)out & 7))) return fail_msg(-3, "cfir: need an 8-byte aligned output of out_pitch >= max_out(n_in)");
    csdr_amd_ctx *c = p->c;
    p->last_kernel = cfir_kernel_for(p->force_generic, p->T);
    if (launch_cfir(c->stream, p->force_generic, (const float2 *)in, in_pitch, n_in, p->d_hist.get(), p->hist_cap, p->d_st.get(), (float2 *)out, out_pitch,
                    p->d_taps.get(), (size_t)p->T, p->T, p->n_ch) < 0) return -3;
    hipLaunchKernelGGL(k_cfir_hist, dim3(cdiv(p->n_ch, 64)), dim3(64), 0, c->stream, (const float2 *)in, in_pitch, n_in, p->d_hist.get(), p->hist_cap, p->d_st.get(),
                       p->n_ch, p->T, counts);
    CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_cfir_force_generic(csdr_amd_cfir *p, int on) { return bank_force_generic(p, "cfir", on); }
const char *csdr_amd_cfir_kernel_name(const csdr_amd_cfir *p) { return bank_kernel_name(p); }
void csdr_amd_cfir_destroy(csdr_amd_cfir *p) { destroy_on_stream(p); }

int csdr_amd_apply_fir_cc(csdr_amd_ctx *c, const csdr_complexf *in, csdr_complexf *out, int n_streams, long long n, size_t in_pitch, size_t out_pitch,
                          const csdr_complexf *taps, size_t taps_pitch, int taps_length, int force_generic)
{
    if (!c) return fail_msg(-3, "apply_fir_cc: null context");
    if (n_streams < 1) return fail_msg(-3, "apply_fir_cc: n_streams should be at least 1");
    if (taps_length < 1 || taps_length > CF_MAX_TAPS) return fail_msg(-3, "apply_fir_cc: taps_length should be 1 .. %d", CF_MAX_TAPS);
    if (!taps || ((uintptr_t)taps & 7)) return fail_msg(-3, "apply_fir_cc: null or unaligned taps");
    if (taps_pitch && taps_pitch < (size_t)taps_length) return fail_msg(-3, "apply_fir_cc: taps_pitch should be 0 (shared) or at least taps_length");
    if (check_rows("apply_fir_cc", in, n, in_pitch) < 0) return -3;
    const long long no = n - taps_length + 1;
    if (no <= 0) return 0;
    if (!out || out_pitch < (size_t)no || ((uintptr_t)out & 7)) return fail_msg(-3, "apply_fir_cc: need an 8-byte aligned output of out_pitch >= n - taps_length + 1");
    g_cfir_last = cfir_kernel_for(force_generic != 0, taps_length);
    if (launch_cfir(c->stream, force_generic != 0, (const float2 *)in, in_pitch, n, nullptr, 1, nullptr, (float2 *)out, out_pitch, (const float2 *)taps, taps_pitch,
                    taps_length, n_streams) < 0) return -3;
    CSDR_LAUNCH_CHECK();
    return 0;
}

const char *csdr_amd_apply_fir_last_kernel(void) { return g_cfir_last; }

void csdr_amd_firdes_peaks_c(csdr_complexf *taps, int length, const float *rates, int n_rates, int window)
{
    std::vector<float2> t;
    peaks_taps(t, length, rates, n_rates, window);
    memcpy(taps, t.data(), sizeof(float2) * (size_t)length);
}

// CPU run of the object's walk for one channel, the stream cut into calls of cuts[0], cuts[1], ... samples (the rest of n in one more call); outputs
// concatenated.  Returns the output count.
long long csdr_amd_debug_cfir_walk(const csdr_complexf *taps, int taps_length, const csdr_complexf *in, long long n, const long long *cuts, int n_cuts, csdr_complexf *out)
{
    const int T = taps_length;
    if (T < 1 || T > CF_MAX_TAPS) return fail_msg(-3, "cfir: taps_length should be 1 .. %d", CF_MAX_TAPS);
    if (!taps) return fail_msg(-3, "cfir: null taps");
    if (n < 0 || (n > 0 && (!in || !out)) || n_cuts < 0 || (n_cuts && !cuts)) return fail_msg(-3, "debug_cfir_walk: bad arguments");
    const float2 *h = (const float2 *)taps, *x = (const float2 *)in;
    std::vector<float2> hist(T);
    CfirChan s{0};
    long long k = 0;
    for_each_call(n, cuts, n_cuts, [&](long long done, long long m) {
        const float2 *xc = x + done;
        const int hl = s.hist_len;
        const long long nV = hl + m, no = std::max(0LL, nV - (T - 1));
        auto V = [&](long long p) { return p < hl ? hist[p] : xc[p - hl]; };
        float2 *o = (float2 *)out + k;
        for (long long j = 0; j < no; j++) o[j] = cfir_output(h, T, [&](int t) { return V(j + t); });
        const int h2 = (int)std::min((long long)(T - 1), nV);
        for (int j = 0; j < h2; j++) hist[j] = V(nV - h2 + j);
        s.hist_len = h2;
        k += no;
    });
    return k;
}

} // extern "C"
