// noise.hip -- the noise sources and the AWGN channel for n_channels channels per call (MI355X / gfx950): uniform_noise_f, gaussian_noise_c and awgn_cc
// (csdr.c:3035-3119) as the object csdr_amd_noise_*, the flat csdr_amd_awgn_cc on a caller's noise rows (the --awgnfile path), and the link measurements
// total_logpower_cf, normalized_timing_variance_u32_f and an exact symbol error count.  noise_dev.hpp holds the definition: a channel's stream is a pure
// function of (seed, stream id, sample index), so nothing here depends on how the calls cut a stream or where a channel sits in the batch.
//
// k_noise_gauss: one lane per Philox block = two complex samples = 16 bytes of output, NZ_U blocks per lane NZ_T blocks apart (coalesced).  A channel whose
// position is odd starts in the middle of a block: the lane's samples are k0 = 2 jb - (pos & 1) and k0 + 1, each stored if it lies in [0, n); both as one
// 16-byte access where they exist and the addresses allow.  The fused AWGN forms (MODE 1, 2) read the input sample, scale both parts and add them in the
// same lane: the noise never reaches memory.  MODE 2 also sums the power of the two scaled parts for snr_out, in a fixed order:
//   lane:      its samples in ascending index, each (float)(re * re + im * im) added to a double
//   wave:      lane l += lane l ^ m for m = 32, 16, 8, 4, 2, 1
//   workgroup: wave 0 + wave 1 + wave 2 + wave 3, stored as the channel's partial of this workgroup
//   channel:   k_power_final adds the partials in ascending order in double, then (float)(10 log10(ps / n)) - (float)(10 log10(pn / n))
#include "bank.hpp"
#include "noise_dev.hpp"
#include <math.h>
#include <stddef.h>
#include <string.h>
#include <algorithm>
#include <vector>

using namespace csdr_amd;

namespace {

static_assert(sizeof(NoiseChan) == 24 && sizeof(csdr_amd_noise_chan) == 24, "csdr_amd_noise_chan mirrors NoiseChan");

constexpr int NZ_T = 256;                       // lanes per workgroup
constexpr int NZ_U = 4;                         // Philox blocks per lane
constexpr int NZ_BLK = NZ_T * NZ_U;             // Philox blocks per workgroup: 2048 complex samples or 4096 floats
constexpr long long NZ_MAX_N = 1LL << 30;

// the sum of a workgroup's (a, b) pairs in the order of the header comment; valid in thread 0
__device__ inline void wg_sum2(double &a, double &b)
{
    __shared__ double red[NZ_T / 64][2];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { a += __shfl_xor(a, m); b += __shfl_xor(b, m); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = a; red[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = red[0][0]; b = red[0][1];
#pragma unroll
        for (int w = 1; w < NZ_T / 64; w++) { a += red[w][0]; b += red[w][1]; }
    }
}

// MODE 0: gaussian_noise_c; 1: awgn_cc; 2: awgn_cc with the power partials.  in and out may be the same rows.
template <int MODE>
__global__ __launch_bounds__(NZ_T) void k_noise_gauss(const NoiseChan *__restrict__ st, unsigned long long seed, const float2 *in, size_t in_pitch, float2 *out,
                                                      size_t out_pitch, long long n, int bpc, double *__restrict__ partials)
{
    const int ch = blockIdx.x / bpc, wb = blockIdx.x % bpc;
    const NoiseChan s = st[ch];
    const unsigned long long j0 = s.pos >> 1;
    const int odd = (int)(s.pos & 1);
    const float2 *irow = MODE ? in + (size_t)ch * in_pitch : nullptr;
    float2 *orow = out + (size_t)ch * out_pitch;
    double ps = 0.0, pn = 0.0;
#pragma unroll
    for (int u = 0; u < NZ_U; u++) {
        const long long jb = (long long)wb * NZ_BLK + u * NZ_T + threadIdx.x;
        const long long k0 = 2 * jb - odd;                             // >= -1
        if (k0 >= n) continue;
        const bool v0 = k0 >= 0, v1 = k0 + 1 < n;
        const PhiloxBlock b = noise_block(NOISE_GAUSSIAN, seed, s.stream_id, j0 + (unsigned long long)jb);
        float2 g0 = make_float2(0.f, 0.f), g1 = g0, x0 = g0, x1 = g0;
        if (v0) g0 = noise_gauss(b.w[0], b.w[1]);
        if (v1) g1 = noise_gauss(b.w[2], b.w[3]);
        const bool wide = v0 && v1 && ((uintptr_t)(orow + k0) & 15) == 0 && (!MODE || ((uintptr_t)(irow + k0) & 15) == 0);
        if (MODE) {
            if (wide) {
                const float4 x = *reinterpret_cast<const float4 *>(irow + k0);
                x0 = make_float2(x.x, x.y); x1 = make_float2(x.z, x.w);
            } else {
                if (v0) x0 = irow[k0];
                if (v1) x1 = irow[k0 + 1];
            }
            if (MODE == 2) {                                           // (a sample that is not there adds +0 twice)
                const float s0r = x0.x * s.a_signal, s0i = x0.y * s.a_signal, n0r = g0.x * s.g_noise, n0i = g0.y * s.g_noise;
                const float s1r = x1.x * s.a_signal, s1i = x1.y * s.a_signal, n1r = g1.x * s.g_noise, n1i = g1.y * s.g_noise;
                ps += (double)(s0r * s0r + s0i * s0i); pn += (double)(n0r * n0r + n0i * n0i);
                ps += (double)(s1r * s1r + s1i * s1i); pn += (double)(n1r * n1r + n1i * n1i);
            }
            g0 = awgn_mix(x0, g0, s.a_signal, s.g_noise);
            g1 = awgn_mix(x1, g1, s.a_signal, s.g_noise);
        }
        if (wide) *reinterpret_cast<float4 *>(orow + k0) = make_float4(g0.x, g0.y, g1.x, g1.y);
        else {
            if (v0) orow[k0] = g0;
            if (v1) orow[k0 + 1] = g1;
        }
    }
    if (MODE == 2) {
        wg_sum2(ps, pn);
        if (threadIdx.x == 0) { partials[2 * (size_t)blockIdx.x] = ps; partials[2 * (size_t)blockIdx.x + 1] = pn; }
    }
}

// uniform_noise_f: one lane per Philox block = four floats
__global__ __launch_bounds__(NZ_T) void k_noise_uniform(const NoiseChan *__restrict__ st, unsigned long long seed, float *__restrict__ out, size_t out_pitch,
                                                        long long n, int bpc)
{
    const int ch = blockIdx.x / bpc, wb = blockIdx.x % bpc;
    const NoiseChan s = st[ch];
    const unsigned long long j0 = s.pos >> 2;
    const int off = (int)(s.pos & 3);
    float *orow = out + (size_t)ch * out_pitch;
#pragma unroll
    for (int u = 0; u < NZ_U; u++) {
        const long long jb = (long long)wb * NZ_BLK + u * NZ_T + threadIdx.x;
        const long long k0 = 4 * jb - off;                             // >= -3
        if (k0 >= n) continue;
        const PhiloxBlock b = noise_block(NOISE_UNIFORM, seed, s.stream_id, j0 + (unsigned long long)jb);
        if (k0 >= 0 && k0 + 3 < n && ((uintptr_t)(orow + k0) & 15) == 0)
            *reinterpret_cast<float4 *>(orow + k0) = make_float4(noise_uniform(b.w[0]), noise_uniform(b.w[1]), noise_uniform(b.w[2]), noise_uniform(b.w[3]));
        else {
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (k0 + r >= 0 && k0 + r < n) orow[k0 + r] = noise_uniform(b.w[r]);
        }
    }
}

__global__ __launch_bounds__(64) void k_noise_advance(NoiseChan *__restrict__ st, int n_ch, long long n)
{
    const int ch = blockIdx.x * 64 + threadIdx.x;
    if (ch < n_ch) st[ch].pos += (unsigned long long)n;
}

// the flat awgn_cc: the noise from the caller's rows
__global__ __launch_bounds__(NZ_T) void k_awgn_flat(const float2 *in, size_t in_pitch, const float2 *__restrict__ noise, size_t noise_pitch, float2 *out, size_t out_pitch,
                                                    long long n, int bpc, const float *__restrict__ a_signal, const float *__restrict__ g_noise)
{
    const int ch = blockIdx.x / bpc;
    const float a = a_signal[ch], g = g_noise[ch];
#pragma unroll
    for (int u = 0; u < NZ_U; u++) {
        const long long k = (long long)(blockIdx.x % bpc) * NZ_BLK + u * NZ_T + threadIdx.x;
        if (k < n) out[(size_t)ch * out_pitch + k] = awgn_mix(in[(size_t)ch * in_pitch + k], noise[(size_t)ch * noise_pitch + k], a, g);
    }
}

// the power of a row's samples per workgroup, in the order of the header comment (the second sum stays 0)
__global__ __launch_bounds__(NZ_T) void k_power_partials(const float2 *__restrict__ in, size_t in_pitch, long long n, int bpc, double *__restrict__ partials)
{
    const int ch = blockIdx.x / bpc;
    double p = 0.0, z = 0.0;
#pragma unroll
    for (int u = 0; u < NZ_U; u++) {
        const long long k = (long long)(blockIdx.x % bpc) * NZ_BLK + u * NZ_T + threadIdx.x;
        if (k < n) { const float2 v = in[(size_t)ch * in_pitch + k]; p += (double)(v.x * v.x + v.y * v.y); }
    }
    wg_sum2(p, z);
    if (threadIdx.x == 0) { partials[2 * (size_t)blockIdx.x] = p; partials[2 * (size_t)blockIdx.x + 1] = 0.0; }
}

// SNR: out[ch] = total_logpower(first sums) - total_logpower(second sums); else total_logpower(first sums)
template <bool SNR>
__global__ __launch_bounds__(64) void k_power_final(const double *__restrict__ partials, int bpc, int n_ch, long long n, float *__restrict__ out)
{
    const int ch = blockIdx.x * 64 + threadIdx.x;
    if (ch >= n_ch) return;
    double a = 0.0, b = 0.0;
    for (int w = 0; w < bpc; w++) { a += partials[2 * ((size_t)ch * bpc + w)]; b += partials[2 * ((size_t)ch * bpc + w) + 1]; }
    const float la = (float)(10.0 * log10(a / (double)n));
    out[ch] = SNR ? la - (float)(10.0 * log10(b / (double)n)) : la;
}

__global__ __launch_bounds__(64) void k_timing_variance(const unsigned *__restrict__ idx, size_t pitch, const int *__restrict__ counts, int n_all, int n_rows, int sps,
                                                        int offset, float *__restrict__ out)
{
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= n_rows) return;
    const unsigned *row = idx + (size_t)r * pitch;
    const int n = counts ? std::min(std::max(counts[r], 0), n_all) : n_all;
    out[r] = timing_variance([&](int i) { return row[i]; }, n, sps, offset);
}

__global__ __launch_bounds__(256) void k_count_errors(const uint8_t *__restrict__ a, size_t a_pitch, long long a_len, const uint8_t *__restrict__ b, size_t b_pitch, long long b_len,
                                                      const int *__restrict__ lags, const int *__restrict__ counts, int *__restrict__ errors)
{
    __shared__ int red[4];
    const int ch = blockIdx.x;
    const long long lag = lags ? std::max(lags[ch], 0) : 0;
    const long long want = counts ? (long long)counts[ch] : b_len;
    const long long n = std::max(0LL, std::min(std::min(want, b_len), a_len - lag));
    const uint8_t *ar = a + (size_t)ch * a_pitch + lag, *br = b + (size_t)ch * b_pitch;
    int e = 0;
    for (long long i = threadIdx.x; i < n; i += 256) e += ar[i] != br[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) e += __shfl_xor(e, m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) errors[ch] = red[0] + red[1] + red[2] + red[3];
}

int check_rows(const char *tag, const void *p, long long n, size_t pitch, int align, const char *what)
{
    if (n > 0 && (!p || pitch < (size_t)n || ((uintptr_t)p & (align - 1)))) return fail_msg(-3, "%s: need a %d-byte aligned %s with a pitch >= n", tag, align, what);
    return 0;
}

// workgroups per channel for n items, `per` of them per Philox block: a start inside a block (the positions live on the device) touches
// (n + per - 2) / per + 1 blocks at most
long long noise_bpc(long long n, int per) { return ((n + per - 2) / per + 1 + NZ_BLK - 1) / NZ_BLK; }

} // namespace

struct csdr_amd_noise : ChanBank<NoiseChan> {
    int kind;
    unsigned long long seed;
    std::vector<NoiseChan> cfg;                    // stream ids and gains as the host set them (pos: 0); the positions live on the device
};

extern "C" {

void csdr_amd_awgn_gains(float snr_db, float *a_signal, float *a_noise_scaled)
{   // csdr.c:3050-3052 and the 0.707 of csdr.c:3079, in the reference's types
    const float spn = (float)pow(10, snr_db / 20);
    const float as = (float)(spn / (spn + 1.0)), an = (float)(1.0 / (spn + 1.0));
    if (a_signal) *a_signal = as;
    if (a_noise_scaled) *a_noise_scaled = (float)(an * 0.707);
}

csdr_amd_noise *csdr_amd_noise_create(csdr_amd_ctx *c, int n_channels, int kind, unsigned long long seed, const unsigned *stream_ids)
{
    if (bank_create_check("noise", c, n_channels) < 0) return nullptr;
    if (kind != NOISE_GAUSSIAN && kind != NOISE_UNIFORM) { fail_msg(-3, "noise: kind should be 0 (Gaussian) or 1 (uniform)"); return nullptr; }
    Owned<csdr_amd_noise, csdr_amd_noise_destroy> p(new csdr_amd_noise());
    p->c = c; p->n_ch = n_channels; p->kind = kind; p->seed = seed;
    p->last_kernel = kind == NOISE_GAUSSIAN ? "k_noise_gauss" : "k_noise_uniform";
    p->cfg.resize(n_channels);
    for (int ch = 0; ch < n_channels; ch++) p->cfg[ch] = NoiseChan{0ULL, stream_ids ? stream_ids[ch] : (unsigned)ch, 1.f, 0.f, 0u};
    if (dev_alloc(p->d_st, sizeof(NoiseChan) * n_channels) != hipSuccess) { fail_msg(-2, "noise: out of device memory"); return nullptr; }
    if (csdr_amd_noise_reset(p.get()) < 0) return nullptr;
    return p.release();
}

int csdr_amd_noise_reset(csdr_amd_noise *p)
{
    if (!p) return fail_msg(-3, "noise: null object");
    if (csdr_amd_ctx_sync(p->c) < 0) return -5;
    return csdr_amd_h2d(p->c, p->d_st.get(), p->cfg.data(), sizeof(NoiseChan) * p->n_ch);
}

int csdr_amd_noise_reset_channel(csdr_amd_noise *p, int ch)
{
    if (!p || ch < 0 || ch >= p->n_ch) return fail_msg(-3, "noise: channel out of range");
    return bank_reset_channel(p, "noise", ch, p->cfg[ch]);
}

int csdr_amd_noise_get_channel(csdr_amd_noise *p, int ch, csdr_amd_noise_chan *out) { return bank_get_channel(p, "noise", ch, out); }

long long csdr_amd_noise_position(csdr_amd_noise *p, int ch)
{
    csdr_amd_noise_chan s;
    if (csdr_amd_noise_get_channel(p, ch, &s) < 0) return -1;
    return (long long)s.position;
}

int csdr_amd_noise_set_position(csdr_amd_noise *p, int ch, long long pos)
{
    if (!p || ch < 0 || ch >= p->n_ch) return fail_msg(-3, "noise: channel out of range");
    if (pos < 0) return fail_msg(-3, "noise: a position is a sample index >= 0");
    if (csdr_amd_ctx_sync(p->c) < 0) return -5;
    const unsigned long long v = (unsigned long long)pos;
    return csdr_amd_h2d(p->c, (char *)(p->d_st.get() + ch) + offsetof(NoiseChan, pos), &v, sizeof v);
}

int csdr_amd_noise_set_snr_db(csdr_amd_noise *p, int ch, float snr_db)
{
    if (!p || ch < 0 || ch >= p->n_ch) return fail_msg(-3, "noise: channel out of range");
    if (p->kind != NOISE_GAUSSIAN) return fail_msg(-3, "noise: an SNR belongs to a Gaussian object");
    NoiseChan &s = p->cfg[ch];
    csdr_amd_awgn_gains(snr_db, &s.a_signal, &s.g_noise);
    if (csdr_amd_ctx_sync(p->c) < 0) return -5;
    static_assert(offsetof(NoiseChan, g_noise) == offsetof(NoiseChan, a_signal) + 4, "the two gains are adjacent");
    return csdr_amd_h2d(p->c, (char *)(p->d_st.get() + ch) + offsetof(NoiseChan, a_signal), &s.a_signal, 8);
}

int csdr_amd_noise_set_snrs(csdr_amd_noise *p, const float *snr_db)
{
    if (!p || !snr_db) return fail_msg(-3, "noise: null object or SNRs");
    for (int ch = 0; ch < p->n_ch; ch++)
        if (const int rc = csdr_amd_noise_set_snr_db(p, ch, snr_db[ch])) return rc;
    return 0;
}

int csdr_amd_noise_get_gains(const csdr_amd_noise *p, int ch, float *a_signal, float *a_noise_scaled)
{
    if (!p || ch < 0 || ch >= p->n_ch) return fail_msg(-3, "noise: channel out of range");
    if (a_signal) *a_signal = p->cfg[ch].a_signal;
    if (a_noise_scaled) *a_noise_scaled = p->cfg[ch].g_noise;
    return 0;
}

int csdr_amd_noise_generate(csdr_amd_noise *p, void *out, long long n, size_t out_pitch)
{
    if (!p) return fail_msg(-3, "noise: null object");
    if (n < 0 || n > NZ_MAX_N) return fail_msg(-3, "noise: n should be 0 .. 2^30");
    const bool gauss = p->kind == NOISE_GAUSSIAN;
    if (check_rows("noise", out, n, out_pitch, gauss ? 8 : 4, "output") < 0) return -3;
    if (n == 0) return 0;
    csdr_amd_ctx *c = p->c;
    const long long bpc = noise_bpc(n, gauss ? 2 : 4);
    if (bpc * p->n_ch > 0x7fffffffLL) return fail_msg(-3, "noise: %d channels of %lld samples are more than one launch takes", p->n_ch, n);
    if (gauss) {
        p->last_kernel = "k_noise_gauss";
        hipLaunchKernelGGL(k_noise_gauss<0>, dim3((unsigned)(bpc * p->n_ch)), dim3(NZ_T), 0, c->stream, p->d_st.get(), p->seed, (const float2 *)nullptr, (size_t)0,
                           (float2 *)out, out_pitch, n, (int)bpc, (double *)nullptr);
    } else {
        p->last_kernel = "k_noise_uniform";
        hipLaunchKernelGGL(k_noise_uniform, dim3((unsigned)(bpc * p->n_ch)), dim3(NZ_T), 0, c->stream, p->d_st.get(), p->seed, (float *)out, out_pitch, n, (int)bpc);
    }
    hipLaunchKernelGGL(k_noise_advance, dim3(cdiv(p->n_ch, 64)), dim3(64), 0, c->stream, p->d_st.get(), p->n_ch, n);
    CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_noise_awgn_cc(csdr_amd_noise *p, const csdr_complexf *in, long long n, size_t in_pitch, csdr_complexf *out, size_t out_pitch, float *snr_out)
{
    if (!p) return fail_msg(-3, "noise: null object");
    if (p->kind != NOISE_GAUSSIAN) return fail_msg(-3, "noise: awgn_cc needs a Gaussian object");
    if (n < 0 || n > NZ_MAX_N) return fail_msg(-3, "noise: n should be 0 .. 2^30");
    if (check_rows("noise", in, n, in_pitch, 8, "input") < 0 || check_rows("noise", out, n, out_pitch, 8, "output") < 0) return -3;
    if (n == 0) return 0;                                             // (snr_out is left as it is: no samples, no powers)
    csdr_amd_ctx *c = p->c;
    const long long bpc = noise_bpc(n, 2);
    if (bpc * p->n_ch > 0x7fffffffLL) return fail_msg(-3, "noise: %d channels of %lld samples are more than one launch takes", p->n_ch, n);
    const dim3 grid((unsigned)(bpc * p->n_ch));
    if (snr_out) {
        double *partials = (double *)c->get_scratch(0, sizeof(double) * 2 * (size_t)(bpc * p->n_ch));
        if (!partials) return -2;
        p->last_kernel = "k_noise_gauss<awgn+snr>";
        hipLaunchKernelGGL(k_noise_gauss<2>, grid, dim3(NZ_T), 0, c->stream, p->d_st.get(), p->seed, (const float2 *)in, in_pitch, (float2 *)out, out_pitch, n, (int)bpc,
                           partials);
        hipLaunchKernelGGL(k_power_final<true>, dim3(cdiv(p->n_ch, 64)), dim3(64), 0, c->stream, partials, (int)bpc, p->n_ch, n, snr_out);
    } else {
        p->last_kernel = "k_noise_gauss<awgn>";
        hipLaunchKernelGGL(k_noise_gauss<1>, grid, dim3(NZ_T), 0, c->stream, p->d_st.get(), p->seed, (const float2 *)in, in_pitch, (float2 *)out, out_pitch, n, (int)bpc,
                           (double *)nullptr);
    }
    hipLaunchKernelGGL(k_noise_advance, dim3(cdiv(p->n_ch, 64)), dim3(64), 0, c->stream, p->d_st.get(), p->n_ch, n);
    CSDR_LAUNCH_CHECK();
    return 0;
}

const char *csdr_amd_noise_kernel_name(const csdr_amd_noise *p) { return bank_kernel_name(p); }
void csdr_amd_noise_destroy(csdr_amd_noise *p) { destroy_on_stream(p); }

int csdr_amd_awgn_cc(csdr_amd_ctx *c, const csdr_complexf *in, const csdr_complexf *noise, csdr_complexf *out, int n_channels, long long n, size_t in_pitch,
                     size_t noise_pitch, size_t out_pitch, const float *a_signal, const float *a_noise_scaled)
{
    if (!c) return fail_msg(-3, "awgn_cc: null context");
    if (n_channels < 1 || n < 0 || n > NZ_MAX_N) return fail_msg(-3, "awgn_cc: need n_channels >= 1 and n 0 .. 2^30");
    if (!a_signal || !a_noise_scaled) return fail_msg(-3, "awgn_cc: null gains");
    if (check_rows("awgn_cc", in, n, in_pitch, 8, "input") < 0 || check_rows("awgn_cc", noise, n, noise_pitch, 8, "noise") < 0 ||
        check_rows("awgn_cc", out, n, out_pitch, 8, "output") < 0) return -3;
    if (n == 0) return 0;
    const long long bpc = (n + NZ_BLK - 1) / NZ_BLK;
    if (bpc * n_channels > 0x7fffffffLL) return fail_msg(-3, "awgn_cc: %d channels of %lld samples are more than one launch takes", n_channels, n);
    hipLaunchKernelGGL(k_awgn_flat, dim3((unsigned)(bpc * n_channels)), dim3(NZ_T), 0, c->stream, (const float2 *)in, in_pitch, (const float2 *)noise, noise_pitch,
                       (float2 *)out, out_pitch, n, (int)bpc, a_signal, a_noise_scaled);
    CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_total_logpower_cf(csdr_amd_ctx *c, const csdr_complexf *in, int n_rows, long long n, size_t in_pitch, float *out)
{
    if (!c) return fail_msg(-3, "total_logpower_cf: null context");
    if (n_rows < 1 || n < 1 || n > NZ_MAX_N || !out) return fail_msg(-3, "total_logpower_cf: need n_rows >= 1, n 1 .. 2^30 and an output");
    if (check_rows("total_logpower_cf", in, n, in_pitch, 8, "input") < 0) return -3;
    const long long bpc = (n + NZ_BLK - 1) / NZ_BLK;
    if (bpc * n_rows > 0x7fffffffLL) return fail_msg(-3, "total_logpower_cf: %d rows of %lld samples are more than one launch takes", n_rows, n);
    double *partials = (double *)c->get_scratch(0, sizeof(double) * 2 * (size_t)(bpc * n_rows));
    if (!partials) return -2;
    hipLaunchKernelGGL(k_power_partials, dim3((unsigned)(bpc * n_rows)), dim3(NZ_T), 0, c->stream, (const float2 *)in, in_pitch, n, (int)bpc, partials);
    hipLaunchKernelGGL(k_power_final<false>, dim3(cdiv(n_rows, 64)), dim3(64), 0, c->stream, partials, (int)bpc, n_rows, n, out);
    CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_normalized_timing_variance_u32_f(csdr_amd_ctx *c, const unsigned *idx, size_t pitch, int n, const int *counts, int n_rows, int samples_per_symbol,
                                              int initial_sample_offset, float *out)
{
    if (!c) return fail_msg(-3, "normalized_timing_variance_u32_f: null context");
    if (n_rows < 1 || n < 0 || !out || samples_per_symbol < 1) return fail_msg(-3, "normalized_timing_variance_u32_f: need n_rows >= 1, n >= 0, samples_per_symbol >= 1 and an output");
    if (check_rows("normalized_timing_variance_u32_f", idx, n, pitch, 4, "input") < 0) return -3;
    hipLaunchKernelGGL(k_timing_variance, dim3(cdiv(n_rows, 64)), dim3(64), 0, c->stream, idx, pitch, counts, n, n_rows, samples_per_symbol, initial_sample_offset, out);
    CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_count_errors_u8(csdr_amd_ctx *c, const unsigned char *a, size_t a_pitch, long long a_len, const unsigned char *b, size_t b_pitch, long long b_len,
                             int n_channels, const int *lags, const int *counts, int *errors)
{
    if (!c) return fail_msg(-3, "count_errors_u8: null context");
    if (n_channels < 1 || a_len < 0 || b_len < 0 || a_len > 0x7fffffffLL || b_len > 0x7fffffffLL || !errors)
        return fail_msg(-3, "count_errors_u8: need n_channels >= 1, row lengths 0 .. 2^31 - 1 and an output");
    if (check_rows("count_errors_u8", a, a_len, a_pitch, 1, "first input") < 0 || check_rows("count_errors_u8", b, b_len, b_pitch, 1, "second input") < 0) return -3;
    hipLaunchKernelGGL(k_count_errors, dim3((unsigned)n_channels), dim3(256), 0, c->stream, a, a_pitch, a_len, b, b_pitch, b_len, lags, counts, errors);
    CSDR_LAUNCH_CHECK();
    return 0;
}

// ---- CPU entries: the header's functions on the host
void csdr_amd_debug_philox(const unsigned *ctr, const unsigned *key, unsigned *out)
{
    const PhiloxBlock b = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
    memcpy(out, b.w, sizeof b.w);
}

// kind 0: n complex samples from 2 n words; kind 1: n floats from n words
int csdr_amd_debug_noise_words(int kind, const unsigned *words, long long n, void *out)
{
    if ((kind != NOISE_GAUSSIAN && kind != NOISE_UNIFORM) || n < 0 || (n > 0 && (!words || !out))) return fail_msg(-3, "debug_noise_words: bad arguments");
    for (long long i = 0; i < n; i++) {
        if (kind == NOISE_GAUSSIAN) ((float2 *)out)[i] = noise_gauss(words[2 * i], words[2 * i + 1]);
        else ((float *)out)[i] = noise_uniform(words[i]);
    }
    return 0;
}

// One channel's stream from `position` on, cut into calls of cuts[0], cuts[1], ... samples and the rest.  in == NULL: the noise itself; in != NULL
// (Gaussian): awgn_cc of those n samples at snr_db.
long long csdr_amd_debug_noise_walk(int kind, unsigned long long seed, unsigned stream_id, long long position, long long n, const long long *cuts, int n_cuts,
                                    const csdr_complexf *in, float snr_db, void *out)
{
    if ((kind != NOISE_GAUSSIAN && kind != NOISE_UNIFORM) || position < 0 || n < 0 || (n > 0 && !out) || n_cuts < 0 || (n_cuts && !cuts) ||
        (in && kind != NOISE_GAUSSIAN)) return fail_msg(-3, "debug_noise_walk: bad arguments");
    NoiseChan s{(unsigned long long)position, stream_id, 1.f, 0.f, 0u};
    if (in) csdr_amd_awgn_gains(snr_db, &s.a_signal, &s.g_noise);
    for_each_call(n, cuts, n_cuts, [&](long long done, long long m) {
        for (long long k = 0; k < m; k++) {
            if (kind == NOISE_UNIFORM) { ((float *)out)[done + k] = noise_uniform_at(seed, stream_id, s.pos + k); continue; }
            const float2 g = noise_gauss_at(seed, stream_id, s.pos + k);
            ((float2 *)out)[done + k] = in ? awgn_mix(((const float2 *)in)[done + k], g, s.a_signal, s.g_noise) : g;
        }
        s.pos += (unsigned long long)m;
    });
    return n;
}

// the flat awgn_cc on the host: n samples of in and of the caller's noise at snr_db
int csdr_amd_debug_awgn_cc(const csdr_complexf *in, const csdr_complexf *noise, long long n, float snr_db, csdr_complexf *out)
{
    if (n < 0 || (n > 0 && (!in || !noise || !out))) return fail_msg(-3, "debug_awgn_cc: bad arguments");
    float a, g;
    csdr_amd_awgn_gains(snr_db, &a, &g);
    for (long long k = 0; k < n; k++) ((float2 *)out)[k] = awgn_mix(((const float2 *)in)[k], ((const float2 *)noise)[k], a, g);
    return 0;
}

float csdr_amd_debug_timing_variance(const unsigned *idx, int n, int samples_per_symbol, int initial_sample_offset)
{
    if (n < 0 || (n > 0 && !idx) || samples_per_symbol < 1) { fail_msg(-3, "debug_timing_variance: bad arguments"); return 0.f; }
    return timing_variance([&](int i) { return idx[i]; }, n, samples_per_symbol, initial_sample_offset);
}

} // extern "C"
