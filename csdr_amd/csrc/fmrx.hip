// fmrx.hip -- the narrow-band FM receive bank on baseband (csdr_amd_fmrx): n_channels rows of decimated complexf samples, resident in HBM, to n_channels rows of
// s16 audio through
//
//   fmdemod_quadri_cf | limit_ff [max_amp] | deemphasis_nfm_ff <audio_rate> | fastagc_ff [block [reference]] | convert_f_s16
//
// per channel: the tail of csdr_amd_nfm (nfm.hip) without its u8 front end, for the rows that csdr_amd_fastddc_bank, csdr_amd_ddc_process or csdr_amd_fir_decimate_cc
// leave on the device.  Stream model and arithmetic are csdr_amd_nfm's (nfm_dev.hpp, nfm_demod.hpp): the de-emphasis FIR runs over (1024 zeros ++ limited stream)
// as an exact integer band product on three base-256 digit planes, for whole AGC blocks only; what the filter has not consumed waits in the object.  The integer sums
// are exact, so an output's bits depend neither on the tiling nor on how the stream is cut into calls, and the two paths below agree bit for bit.
//
//   generic  k_nfm_demod_limit -> digit planes behind the carry, k_nfm_deemph_mfma, fastagc_ff_s16, k_nfm_move_front_planes: csdr_amd_nfm's launches with its
//            fusions off.  Every shape.
//   fused    k_fmrx_front: one workgroup = 16 channels x 1024 outputs reads the complexf rows itself (float4 loads, four samples a lane), demodulates and limits every
//            staged sample once and writes the digit bytes of four samples as one LDS word per plane where the matrix cores' B operands are read from; the
//            digit planes never go to HBM.
//            The 240-sample window tail of a span (and the 256 samples the two staging passes of a span share) are demodulated again instead.  The span's
//            peak |out| goes to fastagc_peaks_buffer, so fastagc_ff_s16 needs no peak pass.  k_fmrx_keep then writes the digits of the samples the call keeps
//            (fewer than taps + agc_block) into the OTHER of two small carry buffers: k_fmrx_front only reads the one it was given.
//            Needs agc_block == 1024, 16-byte aligned rows and an even in_pitch.
#include "bank.hpp"
#include "nfm_dev.hpp"
#include <string.h>

using namespace csdr_amd;

namespace {

constexpr int FMRX_PREFIX = 1024;          // `csdr deemphasis_nfm_ff` filters the_bufsize zeros ++ stream (csdr.c:1076-1081) at the default buffer size
constexpr int FMRX_CARRY = 2048;           // bytes per channel and plane of a carry buffer: the held input is FMRX_PREFIX or fewer than taps + agc_block <= 241 + 1536 samples

struct FmrxArgs {
    const float2 *in; size_t in_pitch; int n_in;       // the call's rows
    const float2 *last;                                // [n_ch]: the sample in front of in[.][0]
    const int8_t *carry; size_t carry_plane;           // [3][n_ch][FMRX_CARRY]: the digits of the fill samples held from earlier calls
    int fill, n_ch;
    float max_amp, q_per_amp;
};

// the three digit bytes of filter input i0 + l (l: index in the staged row) -> dst[0], dst[plane], dst[2 plane]; i < fill: held digits; i >= fill: sample
// k = i - fill of the call (x, its predecessor p); behind the call's samples: zeros (they meet zero weights)
__device__ __forceinline__ void fmrx_put(const FmrxArgs &a, int8_t *dst, int plane, int k, float2 x, float2 p, const int8_t *held)
{
    int d[3] = {0, 0, 0};
    if (k < 0) { d[0] = held[0]; d[1] = held[a.carry_plane]; d[2] = held[2 * a.carry_plane]; }
    else if (k < a.n_in) nfm_demod_digits(x, p, a.max_amp, a.q_per_amp, d);
    dst[0] = (int8_t)d[0]; dst[plane] = (int8_t)d[1]; dst[2 * plane] = (int8_t)d[2];
}

// sample k of a row, k = -1: the stream's sample in front of the call; outside [-1, n_in): not used, (0, 0)
__device__ __forceinline__ float2 fmrx_sample(const FmrxArgs &a, const float2 *x, int st, int k)
{
    if (k >= 0 && k < a.n_in) return x[k];
    return k == -1 ? a.last[st] : make_float2(0.f, 0.f);
}

// the low bytes of the three digits of filter input i (i < fill: the held ones at `held`; else sample k = i - fill of the call, x, with its predecessor p; behind
// the call's samples: zeros) shifted to byte `e` of the words w[0 .. 2], one word per plane
__device__ __forceinline__ void fmrx_pack(const FmrxArgs &a, unsigned (&w)[3], int e, int k, float2 x, float2 p, const int8_t *held)
{
    int d[3] = {0, 0, 0};
    if (k < 0) { d[0] = held[0]; d[1] = held[a.carry_plane]; d[2] = held[2 * a.carry_plane]; }
    else if (k < a.n_in) nfm_demod_digits(x, p, a.max_amp, a.q_per_amp, d);
#pragma unroll
    for (int j = 0; j < 3; j++) w[j] |= (unsigned)(d[j] & 255) << (8 * e);
}

// grid (ne / 1024, ceil(n_ch / 16)), 256 threads.  out[ch][o] for the span's 1024 outputs, peaks[ch * peak_pitch + 2 + span].
__global__ __launch_bounds__(256) void k_fmrx_front(FmrxArgs a, const v4i *__restrict__ frags, float scale, float *__restrict__ out, size_t out_pitch,
                                                    float *__restrict__ peaks, int peak_pitch)
{
    __shared__ __attribute__((aligned(16))) int8_t lds[3 * 16 * NFM_FIR_RP];
    __shared__ float wpeak[4][16];
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, q = lane >> 4, wv = tid >> 6;
    v4i A[NFM_FIR_NK * 3];
#pragma unroll
    for (int i = 0; i < NFM_FIR_NK * 3; i++) A[i] = frags[i * 64 + lane];
    const int last = a.n_ch - 1;
    const int stream = (int)blockIdx.y * 16 + col;
    const int8_t *row = lds + col * NFM_FIR_RP + 16 * q;
    float pmax = 0.f;
    constexpr int QUADS = NFM_FIR_ROW / 4;                              // a lane stages four consecutive filter inputs: one whole LDS word per plane, no word shared by two lanes
    for (int sub = 0; sub < NFM_FIR_SPAN / NFM_FIR_SUB; sub++) {
        const int tile0 = blockIdx.x * NFM_FIR_SPAN + sub * NFM_FIR_SUB;
        if (sub) __syncthreads();                                     // everyone has read the previous pass's rows
        // stage [3 planes][16 channels][NFM_FIR_ROW]: the filter inputs i0 .. i0 + NFM_FIR_ROW - 1; wave wv takes the channels 4 wv .. 4 wv + 3 (rows of channels
        // past the last one re-read it)
        const int i0 = tile0 * 16, k0 = i0 - a.fill;
        for (int idx = lane; idx < 4 * QUADS; idx += 64) {
            const int r = 4 * wv + idx / QUADS, l = 4 * (idx % QUADS);
            const int st = min((int)blockIdx.y * 16 + r, last);
            const float2 *x = a.in + (size_t)st * a.in_pitch;
            const int k = k0 + l;                                      // the call's samples k - 1 (the first one's predecessor) .. k + 3
            float2 s[5];
            if (k >= 1 && k + 3 < a.n_in) {                            // two 16-byte loads on even sample indexes and the odd one out, whatever the parity of fill
                if (k & 1) {
                    const float4 u = *reinterpret_cast<const float4 *>(x + k - 1), v = *reinterpret_cast<const float4 *>(x + k + 1);
                    s[0] = make_float2(u.x, u.y); s[1] = make_float2(u.z, u.w); s[2] = make_float2(v.x, v.y); s[3] = make_float2(v.z, v.w); s[4] = x[k + 3];
                } else {
                    const float4 u = *reinterpret_cast<const float4 *>(x + k), v = *reinterpret_cast<const float4 *>(x + k + 2);
                    s[0] = x[k - 1]; s[1] = make_float2(u.x, u.y); s[2] = make_float2(u.z, u.w); s[3] = make_float2(v.x, v.y); s[4] = make_float2(v.z, v.w);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 5; e++) s[e] = fmrx_sample(a, x, st, k - 1 + e);
            }
            const int8_t *held = a.carry + (size_t)st * FMRX_CARRY + (i0 + l);      // read for sample indexes < 0 only: i0 + l + e < fill
            unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
            for (int e = 0; e < 4; e++) fmrx_pack(a, w, e, k + e, s[e + 1], s[e], held + e);
#pragma unroll
            for (int pl = 0; pl < 3; pl++) *reinterpret_cast<unsigned *>(lds + (pl * 16 + r) * NFM_FIR_RP + l) = w[pl];
        }
        __syncthreads();
        nfm_deemph_tiles(row, A, scale, out, out_pitch, stream, a.n_ch, tile0, NFM_FIR_SUB, wv, q, pmax);
    }
    nfm_store_span_peaks(pmax, wpeak, a.n_ch, peaks, peak_pitch);
}

// grid (ceil(rem / 256), n_ch): the digits of the filter inputs ne .. ne + rem - 1, which the call keeps, to keep[.][ch][0 .. rem).  keep == a.carry (a call without
// output: ne == 0): only the call's samples are appended.  Thread 0 of a channel leaves the call's last sample in last_out.
__global__ __launch_bounds__(256) void k_fmrx_keep(FmrxArgs a, int ne, int rem, int8_t *keep, float2 *__restrict__ last_out)
{
    const int st = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const float2 *x = a.in + (size_t)st * a.in_pitch;
    if (j == 0) last_out[st] = x[a.n_in - 1];
    if (j >= rem) return;
    const int i = ne + j, k = i - a.fill;
    if (k < 0 && keep == a.carry) return;
    fmrx_put(a, keep + (size_t)st * FMRX_CARRY + j, (int)a.carry_plane, k, fmrx_sample(a, x, st, k), fmrx_sample(a, x, st, k - 1), a.carry + (size_t)st * FMRX_CARRY + i);
}

} // namespace

struct csdr_amd_fmrx : Bank {
    int Ld, agc_block, fill;
    float limit, agc_ref;
    size_t max_n;
    DevBuf<cf32> d_last[2]; int lflip;              // the sample in front of the next call, read from one and written to the other
    DevBuf<int8_t> d_planes; size_t plane_bytes, dl_pitch;        // generic path: [3][n_ch][dl_pitch], the held input in front, the call's digits behind it
    DevBuf<int8_t> d_carry[2]; int cflip;           // fused path: [3][n_ch][FMRX_CARRY] each
    enum { HELD_BOTH, HELD_PLANES, HELD_CARRY } held;             // where the held input's digits are (both after a reset: zeros)
    DevBuf<> d_fir_frags; float fir_scale;
    DevBuf<float> d_de; size_t a_pitch;             // de-emphasised blocks
    DevBuf<float> d_agc_state;
};

extern "C" {

int csdr_amd_fmrx_plan(int fill, long long n_in, int taps_length, int agc_block, long long *ne, int *new_fill)
{
    if (fill < 0 || n_in < 0 || taps_length < 1 || agc_block < 1) return fail_msg(-3, "fmrx: plan needs fill >= 0, n_in >= 0, taps_length >= 1, agc_block >= 1");
    const long long all = fill + n_in - taps_length;                  // deemphasis_nfm_ff produces input - taps outputs (libcsdr.c:1121); whole AGC blocks of them are run
    const long long e = all > 0 && n_in > 0 ? all / agc_block * agc_block : 0;      // (a call without input does nothing)
    if (fill + n_in - e > 0x7fffffffLL) return fail_msg(-3, "fmrx: plan: the held input exceeds an int");
    if (ne) *ne = e;
    if (new_fill) *new_fill = (int)(fill + n_in - e);
    return 0;
}

csdr_amd_fmrx *csdr_amd_fmrx_create(csdr_amd_ctx *ctx, int n_channels, int audio_rate, int agc_block, float agc_reference, float limit_max, size_t max_samples_per_call)
{
    if (bank_create_check("fmrx", ctx, n_channels, 65535) < 0) return nullptr;                 // (a channel, or a group of 16, is a grid row)
    if (agc_block < 16 || agc_block > 2048 - 512 || (agc_block % 16)) { fail_msg(-3, "fmrx: agc_block should be a multiple of 16 in 16 .. 1536"); return nullptr; }
    if (!(limit_max > 0)) { fail_msg(-3, "fmrx: limit_max should be > 0"); return nullptr; }
    if (max_samples_per_call < 1 || max_samples_per_call > ((size_t)1 << 30)) { fail_msg(-3, "fmrx: max_samples_per_call should be 1 .. 2^30"); return nullptr; }
    const float *dt = nullptr;
    const int Ld = csdr_amd_nfm_deemph_taps(audio_rate, &dt);
    if (!Ld) { fail_msg(-3, "fmrx: no de-emphasis table for sample rate %d (libcsdr.c:1115-1119)", audio_rate); return nullptr; }
    if (Ld + 15 > 64 * NFM_FIR_NK) { fail_msg(-3, "fmrx: %d de-emphasis taps exceed the matrix-core tile", Ld); return nullptr; }
    static_assert(FMRX_PREFIX <= FMRX_CARRY && 64 * NFM_FIR_NK - 15 + (2048 - 512) - 1 <= FMRX_CARRY, "a carry row holds the most input an object keeps");
    Owned<csdr_amd_fmrx, csdr_amd_fmrx_destroy> p(new csdr_amd_fmrx());
    p->c = ctx; p->n_ch = n_channels; p->Ld = Ld; p->agc_block = agc_block; p->limit = limit_max; p->agc_ref = agc_reference; p->max_n = max_samples_per_call;
    p->dl_pitch = (p->max_n + FMRX_CARRY + NFM_FIR_ROW + 63) & ~(size_t)63;        // + the last workgroup's staged span beyond the valid samples (zero weights)
    p->a_pitch = (p->max_n + FMRX_CARRY + 15) & ~(size_t)15;
    p->plane_bytes = p->dl_pitch * n_channels;
    hipError_t e = hipSuccess;
    auto alloc = [&](auto &b, size_t bytes) { if (e == hipSuccess) e = dev_alloc(b, bytes); };
    alloc(p->d_last[0], sizeof(cf32) * n_channels); alloc(p->d_last[1], sizeof(cf32) * n_channels);
    alloc(p->d_planes, 3 * p->plane_bytes);
    alloc(p->d_carry[0], (size_t)3 * FMRX_CARRY * n_channels); alloc(p->d_carry[1], (size_t)3 * FMRX_CARRY * n_channels);
    alloc(p->d_fir_frags, (size_t)NFM_FIR_NK * 3 * 64 * 16);
    alloc(p->d_de, sizeof(float) * p->a_pitch * n_channels);
    alloc(p->d_agc_state, sizeof(float) * (size_t)n_channels * (2 * agc_block + 4));
    if (e != hipSuccess) { fail_msg(-2, "fmrx: out of device memory"); return nullptr; }
    std::vector<int8_t> fr;
    p->fir_scale = nfm_fir_table(dt, Ld, limit_max, fr);
    if (csdr_amd_h2d(ctx, p->d_fir_frags.get(), fr.data(), fr.size()) < 0) return nullptr;
    if (csdr_amd_fmrx_reset(p.get()) < 0) return nullptr;
    return p.release();
}

int csdr_amd_fmrx_reset(csdr_amd_fmrx *p)
{
    if (!p) return fail_msg(-3, "fmrx: null object");
    hipStream_t st = p->c->stream;
    p->fill = FMRX_PREFIX; p->lflip = p->cflip = 0; p->held = csdr_amd_fmrx::HELD_BOTH;      // the prefix: zeros, cleared below
    CSDR_HIP(hipMemsetAsync(p->d_planes.get(), 0, 3 * p->plane_bytes, st));                        // bytes behind the valid samples meet zero weights, but must be initialised
    for (int k = 0; k < 2; k++) {
        CSDR_HIP(hipMemsetAsync(p->d_carry[k].get(), 0, (size_t)3 * FMRX_CARRY * p->n_ch, st));
        CSDR_HIP(hipMemsetAsync(p->d_last[k].get(), 0, sizeof(cf32) * p->n_ch, st));               // the CLI starts fmdemod from (0, 0) (csdr.c:1044)
    }
    CSDR_HIP(hipMemsetAsync(p->d_agc_state.get(), 0, sizeof(float) * (size_t)p->n_ch * (2 * p->agc_block + 4), st));   // calloc'ed fastagc state (csdr.c:1393-1394)
    return 0;
}

// one channel's held input, previous sample and AGC state to zero; the count of held samples is the bank's and stays
int csdr_amd_fmrx_reset_channel(csdr_amd_fmrx *p, int ch)
{
    if (!p || ch < 0 || ch >= p->n_ch) return fail_msg(-3, "fmrx: channel out of range");
    hipStream_t st = p->c->stream;
    for (int pl = 0; pl < 3; pl++) {
        CSDR_HIP(hipMemsetAsync(p->d_planes.get() + pl * p->plane_bytes + (size_t)ch * p->dl_pitch, 0, p->dl_pitch, st));
        for (int k = 0; k < 2; k++) CSDR_HIP(hipMemsetAsync(p->d_carry[k].get() + ((size_t)pl * p->n_ch + ch) * FMRX_CARRY, 0, FMRX_CARRY, st));
    }
    for (int k = 0; k < 2; k++) CSDR_HIP(hipMemsetAsync(p->d_last[k].get() + ch, 0, sizeof(cf32), st));
    CSDR_HIP(hipMemsetAsync(p->d_agc_state.get() + (size_t)ch * (2 * p->agc_block + 4), 0, sizeof(float) * (2 * p->agc_block + 4), st));
    return 0;
}

void csdr_amd_fmrx_destroy(csdr_amd_fmrx *p) { destroy_on_stream(p); }
int csdr_amd_fmrx_force_generic(csdr_amd_fmrx *p, int on) { return bank_force_generic(p, "fmrx", on); }
const char *csdr_amd_fmrx_kernel_name(const csdr_amd_fmrx *p) { return bank_kernel_name(p); }
int csdr_amd_fmrx_fill(const csdr_amd_fmrx *p) { return p ? p->fill : -1; }

long long csdr_amd_fmrx_max_output(const csdr_amd_fmrx *p, long long n_in)
{
    if (!p || n_in < 0) return 0;
    long long ne = 0;
    // the most an object holds: the prefix after a reset, or one sample short of another block
    (void)csdr_amd_fmrx_plan(std::max(FMRX_PREFIX, p->Ld + p->agc_block - 1), n_in, p->Ld, p->agc_block, &ne, nullptr);
    return ne;
}
long long csdr_amd_fmrx_max_out(const csdr_amd_fmrx *p, long long n_in) { return csdr_amd_fmrx_max_output(p, n_in); }

// the held digits from where the other path left them to where this one reads them: 3 x n_ch rows of fill bytes
static int fmrx_move_held(csdr_amd_fmrx *p, bool to_planes)
{
    int8_t *carry = p->d_carry[p->cflip].get();
    for (int pl = 0; pl < 3 && p->fill > 0; pl++) {
        int8_t *pr = p->d_planes.get() + pl * p->plane_bytes, *cr = carry + (size_t)pl * p->n_ch * FMRX_CARRY;
        if (to_planes) CSDR_HIP(hipMemcpy2DAsync(pr, p->dl_pitch, cr, FMRX_CARRY, p->fill, p->n_ch, hipMemcpyDeviceToDevice, p->c->stream));
        else CSDR_HIP(hipMemcpy2DAsync(cr, FMRX_CARRY, pr, p->dl_pitch, p->fill, p->n_ch, hipMemcpyDeviceToDevice, p->c->stream));
    }
    return 0;
}

long long csdr_amd_fmrx_process(csdr_amd_fmrx *p, const csdr_complexf *in, size_t in_pitch, long long n_in, int16_t *audio_s16, float *audio_f, size_t out_pitch)
{
    if (!p) return fail_msg(-3, "fmrx: null object");
    if (n_in < 0 || (size_t)n_in > p->max_n) return fail_msg(-3, "fmrx: n_in should be 0 .. max_samples_per_call (%zu)", p->max_n);
    if (!n_in) return 0;
    if (!in || (in_pitch < (size_t)n_in && p->n_ch > 1)) return fail_msg(-3, "fmrx: in_pitch below n_in");
    long long ne64 = 0; int rem = 0;
    if (csdr_amd_fmrx_plan(p->fill, n_in, p->Ld, p->agc_block, &ne64, &rem) < 0) return -3;
    const int ne = (int)ne64, nb = ne / p->agc_block, S = p->n_ch, fill = p->fill;
    if ((size_t)ne > out_pitch && S > 1) return fail_msg(-3, "fmrx: out_pitch %zu smaller than the %d audio samples of this call", out_pitch, ne);
    if (rem > FMRX_CARRY) return fail_msg(-3, "fmrx: internal carry of %d samples", rem);
    csdr_amd_ctx *c = p->c; hipStream_t st = c->stream;
    cf32 *last_in = p->d_last[p->lflip].get(), *last_out = p->d_last[p->lflip ^ 1].get();
    const float q_per_amp = NFM_XQ / p->limit;
    const bool fused = !p->force_generic && p->agc_block == 16 * NFM_FIR_SPAN && !((uintptr_t)in & 15) && !(in_pitch & 1);
    if (fused) {
        p->last_kernel = "k_fmrx_front";
        if (p->held == csdr_amd_fmrx::HELD_PLANES) { const int rc = fmrx_move_held(p, false); if (rc) return rc; }
        FmrxArgs a;
        a.in = (const float2 *)in; a.in_pitch = in_pitch; a.n_in = (int)n_in; a.last = (const float2 *)last_in; a.carry = p->d_carry[p->cflip].get();
        a.carry_plane = (size_t)S * FMRX_CARRY; a.fill = fill; a.n_ch = S; a.max_amp = p->limit; a.q_per_amp = q_per_amp;
        if (nb > 0) {
            float *peaks = fastagc_peaks_buffer(c, S, nb);
            if (!peaks) return -2;
            hipLaunchKernelGGL(k_fmrx_front, dim3(nb, cdiv(S, 16)), dim3(256), 0, st, a, (const v4i *)p->d_fir_frags.get(), p->fir_scale, p->d_de.get(), p->a_pitch, peaks, nb + 2);
            CSDR_LAUNCH_CHECK();
            const int rc = fastagc_ff_s16(c, p->d_de.get(), audio_f, audio_s16, S, nb, p->agc_block, p->a_pitch, out_pitch, out_pitch, p->agc_ref, p->d_agc_state.get(), true);
            if (rc) return rc;
        }
        // what the call keeps: into the other carry buffer behind a call with output, appended in place behind one without
        int8_t *keep = p->d_carry[nb > 0 ? p->cflip ^ 1 : p->cflip].get();
        hipLaunchKernelGGL(k_fmrx_keep, dim3(cdiv(rem, 256), S), dim3(256), 0, st, a, ne, rem, keep, (float2 *)last_out);
        CSDR_LAUNCH_CHECK();
        if (nb > 0) p->cflip ^= 1;
        p->held = csdr_amd_fmrx::HELD_CARRY;
    } else {
        p->last_kernel = "k_nfm_deemph_mfma";
        if (p->held == csdr_amd_fmrx::HELD_CARRY) { const int rc = fmrx_move_held(p, true); if (rc) return rc; }
        // fmdemod_quadri_cf | limit_ff, appended behind the filter's unconsumed input
        hipLaunchKernelGGL(k_nfm_demod_limit, dim3(cdiv(n_in, 256), S), dim3(256), 0, st, in, in_pitch, (int)n_in, last_in, p->d_planes.get(), p->plane_bytes, p->dl_pitch, fill, p->limit, q_per_amp);
        CSDR_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_nfm_store_last, dim3(cdiv(S, 64)), dim3(64), 0, st, in, in_pitch, (int)n_in, last_out, S);
        CSDR_LAUNCH_CHECK();
        if (nb > 0) {
            const int n_tiles = ne / 16;
            hipLaunchKernelGGL(k_nfm_deemph_mfma, dim3(cdiv(n_tiles, NFM_FIR_SPAN), cdiv(S, 16)), dim3(256), 0, st, p->d_planes.get(), p->plane_bytes, p->dl_pitch, (const v4i *)p->d_fir_frags.get(),
                               p->fir_scale, p->d_de.get(), p->a_pitch, n_tiles, S, (float *)nullptr, 0);
            CSDR_LAUNCH_CHECK();
            const int rc = fastagc_ff_s16(c, p->d_de.get(), audio_f, audio_s16, S, nb, p->agc_block, p->a_pitch, out_pitch, out_pitch, p->agc_ref, p->d_agc_state.get(), false);
            if (rc) return rc;
            // keep the unconsumed filter input in front
            hipLaunchKernelGGL(k_nfm_move_front_planes, dim3(S, 3), dim3(256), 0, st, p->d_planes.get(), p->plane_bytes, p->dl_pitch, ne, rem);
            CSDR_LAUNCH_CHECK();
        }
        p->held = csdr_amd_fmrx::HELD_PLANES;
    }
    p->lflip ^= 1;
    p->fill = rem;
    return ne;
}

} // extern "C"
