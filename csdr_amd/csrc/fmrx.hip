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
//
// With a squelch in front (csdr_amd_fmrx_create_squelched: squelch_and_smeter_cc | the chain above) the channel's input is cut into blocks of B samples counted
// from the reset; whole blocks go on, gated, and what lies behind the last whole block (fewer than B complexf per channel) waits in the object.  The power is
// squelch_dev.hpp's (512 chains by sample index, then the tree), the gate squelch_open, the level of a block the one in force when its first sample arrived.
//   generic  an internal csdr_amd_squelch writes the gated rows to a scratch buffer; the generic path above runs over them.  Every shape.
//   fused    k_fmrx_power: one wave per (channel, block) reads held ++ call once and writes the power and the open flag, nothing else.  k_fmrx_front<true>
//            and k_fmrx_keep<true> ("k_fmrx_front_sq") then read the call's gated sample k as held[k] for k < h, else in[k - h], and as (0, 0) when the flag
//            of block k / B is closed: the gated rows never exist in HBM.  A lane's five samples that lie in one block, behind the held ones, are fetched with
//            the two 16-byte loads of the plain kernel (the parity branch decides on k - h) or, in a closed block, not at all (their digits are zeros); five
//            that straddle two blocks or the held / call seam are fetched one by one, each under its own block's flag.  k_fmrx_sq_carry moves what the call
//            leaves behind its last whole block into the OTHER of two carry buffers.  Any call length; the preconditions are the plain kernel's.
#include "bank.hpp"
#include "nfm_dev.hpp"
#include "rx_squelch_dev.hpp"
#include <string.h>

using namespace csdr_amd;

namespace {

constexpr int FMRX_PREFIX = 1024;          // `csdr deemphasis_nfm_ff` filters the_bufsize zeros ++ stream (csdr.c:1076-1081) at the default buffer size
constexpr int FMRX_CARRY = 2048;           // bytes per channel and plane of a carry buffer: the held input is FMRX_PREFIX or fewer than taps + agc_block <= 241 + 1536 samples

struct FmrxArgs {
    const float2 *in; size_t in_pitch; int n_in;       // the call's rows; gated launches: n_in = the gated samples, h of them from sq.held
    const float2 *last;                                // [n_ch]: the sample in front of in[.][0]
    const int8_t *carry; size_t carry_plane;           // [3][n_ch][FMRX_CARRY]: the digits of the fill samples held from earlier calls
    int fill, n_ch;
    float max_amp, q_per_amp;
    FmrxSq sq;                                         // gated launches only
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
template <bool SQ> __device__ __forceinline__ float2 fmrx_sample(const FmrxArgs &a, const float2 *x, int st, int k)
{
    if (k >= 0 && k < a.n_in) {
        if (!SQ) return x[k];
        if (!a.sq.flags[(size_t)st * a.sq.fl_pitch + fmrx_sq_block(a.sq, k)]) return make_float2(0.f, 0.f);
        return k < a.sq.h ? a.sq.held[(size_t)st * a.sq.B + k] : x[k - a.sq.h];
    }
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

// grid (ne / 1024, ceil(n_ch / 16)), 256 threads.  out[ch][o] for the span's 1024 outputs, peaks[ch * peak_pitch + 2 + span].  SQ: the gated launch.
template <bool SQ> __global__ __launch_bounds__(256) void k_fmrx_front(FmrxArgs a, const v4i *__restrict__ frags, float scale, float *__restrict__ out, size_t out_pitch,
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
        // how the lane fetches the five samples of quad idx: 1 = all in the call's rows (gated: and in one open block), 0 = in one closed block: nothing to fetch,
        // 2 = one by one.  Gated, the flag is asked for one quad ahead, so that its load is under way while the quad in front is demodulated.
        auto fetch_kind = [&](int idx) -> int {
            if (idx >= 4 * QUADS) return 2;
            const int k = k0 + 4 * (idx % QUADS), j = SQ ? k - a.sq.h : k;
            if (!(j >= 1 && k + 3 < a.n_in)) return 2;
            if (!SQ) return 1;
            const int b = fmrx_sq_block(a.sq, k - 1);
            if (k + 3 - b * a.sq.B >= a.sq.B) return 2;               // the five straddle two blocks
            return a.sq.flags[(size_t)min((int)blockIdx.y * 16 + 4 * wv + idx / QUADS, last) * a.sq.fl_pitch + b] != 0;
        };
        int kind_next = fetch_kind(lane);
        for (int idx = lane; idx < 4 * QUADS; idx += 64) {
            const int r = 4 * wv + idx / QUADS, l = 4 * (idx % QUADS);
            const int st = min((int)blockIdx.y * 16 + r, last);
            const float2 *x = a.in + (size_t)st * a.in_pitch;
            const int k = k0 + l;                                      // the call's samples k - 1 (the first one's predecessor) .. k + 3
            float2 s[5];
            const int j = SQ ? k - a.sq.h : k;                         // the row index of gated sample k
            const int kind = kind_next;
            if (SQ) kind_next = fetch_kind(idx + 64); else kind_next = 1;
            const bool rows = SQ ? kind == 1 : (j >= 1 && k + 3 < a.n_in);
            if (SQ && kind == 0) {                                     // a closed block is not loaded: zeros behind any sample demodulate to the digits 0, 0, 0
#pragma unroll
                for (int pl = 0; pl < 3; pl++) *reinterpret_cast<unsigned *>(lds + (pl * 16 + r) * NFM_FIR_RP + l) = 0u;
                continue;
            }
            if (rows) {                                                // two 16-byte loads on even row indexes and the odd one out, whatever the parity of fill (and of h)
                if (j & 1) {
                    const float4 u = *reinterpret_cast<const float4 *>(x + j - 1), v = *reinterpret_cast<const float4 *>(x + j + 1);
                    s[0] = make_float2(u.x, u.y); s[1] = make_float2(u.z, u.w); s[2] = make_float2(v.x, v.y); s[3] = make_float2(v.z, v.w); s[4] = x[j + 3];
                } else {
                    const float4 u = *reinterpret_cast<const float4 *>(x + j), v = *reinterpret_cast<const float4 *>(x + j + 2);
                    s[0] = x[j - 1]; s[1] = make_float2(u.x, u.y); s[2] = make_float2(u.z, u.w); s[3] = make_float2(v.x, v.y); s[4] = make_float2(v.z, v.w);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 5; e++) s[e] = fmrx_sample<SQ>(a, x, st, k - 1 + e);
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
// output: ne == 0): only the call's samples are appended.  Thread 0 of a channel leaves the call's last (gated) sample in last_out.
template <bool SQ> __global__ __launch_bounds__(256) void k_fmrx_keep(FmrxArgs a, int ne, int rem, int8_t *keep, float2 *__restrict__ last_out)
{
    const int st = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const float2 *x = a.in + (size_t)st * a.in_pitch;
    if (j == 0) last_out[st] = fmrx_sample<SQ>(a, x, st, a.n_in - 1);
    if (j >= rem) return;
    const int i = ne + j, k = i - a.fill;
    if (k < 0 && keep == a.carry) return;
    fmrx_put(a, keep + (size_t)st * FMRX_CARRY + j, (int)a.carry_plane, k, fmrx_sample<SQ>(a, x, st, k), fmrx_sample<SQ>(a, x, st, k - 1), a.carry + (size_t)st * FMRX_CARRY + i);
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
    // the squelch in front (create_squelched; sqB == 0: none)
    int sqB = 0, sqd = 1, sq_h = 0; long long sq_blk = 0;          // block, use_every_nth, held samples per channel, blocks since the reset
    size_t max_m;                                   // the most samples a call hands to the chain: max_n, + sqB - 1 behind a squelch
    std::vector<float> lv, lv_started; bool lv_dirty = false;      // csdr_amd_squelch's levels: of the blocks a call starts, of the block begun earlier
    DevBuf<float> d_lv;                             // [2][n_ch]: lv, lv_started
    DevBuf<float2> d_sq_carry[2]; int sflip = 0;    // fused path: [n_ch][sqB] each, the held samples in d_sq_carry[sflip]
    DevBuf<float> d_pw; DevBuf<uint8_t> d_fl; size_t fl_pitch = 0; // fused path: the call's powers and open flags, [n_ch][fl_pitch]
    Owned<csdr_amd_squelch, csdr_amd_squelch_destroy> sq; float2 *sq_obj_carry = nullptr;     // generic path: the squelch and its held samples [n_ch][sqB]
    DevBuf<float2> d_gated; size_t g_pitch = 0;     // generic path: the gated rows [n_ch][g_pitch]
    enum { SQ_NOWHERE, SQ_OWN, SQ_OBJ } sq_where = SQ_NOWHERE;     // where the held samples are (nowhere: none held since the reset)
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

// squelch_block 0: no squelch
static csdr_amd_fmrx *fmrx_create(csdr_amd_ctx *ctx, int n_channels, int audio_rate, int agc_block, float agc_reference, float limit_max, size_t max_samples_per_call,
                                  int squelch_block, int use_every_nth, const float *levels)
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
    p->sqB = squelch_block; p->sqd = use_every_nth;
    p->max_m = p->max_n + (squelch_block ? squelch_block - 1 : 0);                 // a squelched call hands on up to sqB - 1 held samples more
    p->dl_pitch = (p->max_m + FMRX_CARRY + NFM_FIR_ROW + 63) & ~(size_t)63;        // + the last workgroup's staged span beyond the valid samples (zero weights)
    p->a_pitch = (p->max_m + FMRX_CARRY + 15) & ~(size_t)15;
    p->plane_bytes = p->dl_pitch * n_channels;
    hipError_t e = hipSuccess;
    auto alloc = [&](auto &b, size_t bytes) { if (e == hipSuccess) e = dev_alloc(b, bytes); };
    alloc(p->d_last[0], sizeof(cf32) * n_channels); alloc(p->d_last[1], sizeof(cf32) * n_channels);
    alloc(p->d_planes, 3 * p->plane_bytes);
    alloc(p->d_carry[0], (size_t)3 * FMRX_CARRY * n_channels); alloc(p->d_carry[1], (size_t)3 * FMRX_CARRY * n_channels);
    alloc(p->d_fir_frags, (size_t)NFM_FIR_NK * 3 * 64 * 16);
    alloc(p->d_de, sizeof(float) * p->a_pitch * n_channels);
    alloc(p->d_agc_state, sizeof(float) * (size_t)n_channels * (2 * agc_block + 4));
    if (squelch_block) {
        const int B = squelch_block;
        p->lv.assign(n_channels, 0.f);
        if (levels) p->lv.assign(levels, levels + n_channels);
        p->fl_pitch = (p->max_n + B - 1) / B;                                      // (B - 1 held + max_n) / B blocks at the most
        p->g_pitch = (p->max_m + 1) & ~(size_t)1;
        alloc(p->d_lv, sizeof(float) * 2 * n_channels);
        alloc(p->d_sq_carry[0], sizeof(float2) * (size_t)B * n_channels); alloc(p->d_sq_carry[1], sizeof(float2) * (size_t)B * n_channels);
        alloc(p->d_pw, sizeof(float) * p->fl_pitch * n_channels); alloc(p->d_fl, p->fl_pitch * n_channels);
        alloc(p->d_gated, sizeof(float2) * p->g_pitch * n_channels);
        if (e == hipSuccess) {
            p->sq.reset(csdr_amd_squelch_create(ctx, n_channels, B, use_every_nth, levels, (long long)p->max_n));
            if (!p->sq) return nullptr;
            p->sq_obj_carry = (float2 *)squelch_adopt(p->sq.get(), 0, 0, p->lv.data(), p->lv.data());
        }
    }
    if (e != hipSuccess) { fail_msg(-2, "fmrx: out of device memory"); return nullptr; }
    std::vector<int8_t> fr;
    p->fir_scale = nfm_fir_table(dt, Ld, limit_max, fr);
    if (csdr_amd_h2d(ctx, p->d_fir_frags.get(), fr.data(), fr.size()) < 0) return nullptr;
    if (csdr_amd_fmrx_reset(p.get()) < 0) return nullptr;
    return p.release();
}

csdr_amd_fmrx *csdr_amd_fmrx_create(csdr_amd_ctx *ctx, int n_channels, int audio_rate, int agc_block, float agc_reference, float limit_max, size_t max_samples_per_call)
{
    return fmrx_create(ctx, n_channels, audio_rate, agc_block, agc_reference, limit_max, max_samples_per_call, 0, 1, nullptr);
}

csdr_amd_fmrx *csdr_amd_fmrx_create_squelched(csdr_amd_ctx *ctx, int n_channels, int audio_rate, int agc_block, float agc_reference, float limit_max,
                                              size_t max_samples_per_call, int squelch_block, int use_every_nth, const float *levels)
{
    if (squelch_block < 1 || squelch_block > 65536) { fail_msg(-3, "fmrx: squelch_block should be 1 .. 65536"); return nullptr; }
    if (use_every_nth < 1) { fail_msg(-3, "fmrx: use_every_nth should be >= 1"); return nullptr; }
    return fmrx_create(ctx, n_channels, audio_rate, agc_block, agc_reference, limit_max, max_samples_per_call, squelch_block, use_every_nth, levels);
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
    if (p->sqB) {                                                          // the block count and the held samples start over; the levels stay
        p->sq_h = 0; p->sq_blk = 0; p->sflip = 0; p->sq_where = csdr_amd_fmrx::SQ_NOWHERE; p->lv_started = p->lv; p->lv_dirty = true;
    }
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
    if (p->sqB) {                                                          // the channel's held squelch samples; the block phase is the bank's and stays
        for (int k = 0; k < 2; k++) CSDR_HIP(hipMemsetAsync(p->d_sq_carry[k].get() + (size_t)ch * p->sqB, 0, sizeof(float2) * p->sqB, st));
        CSDR_HIP(hipMemsetAsync(p->sq_obj_carry + (size_t)ch * p->sqB, 0, sizeof(float2) * p->sqB, st));
    }
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
    if (p->sqB) n_in = (n_in + p->sqB - 1) / p->sqB * p->sqB;             // the whole blocks of the call and the most a squelch holds in front
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

// the plan of a call that hands n_in >= 1 samples to the chain, checked against the caller's rows and the carry: 0, or the error
static int fmrx_plan_checked(const csdr_amd_fmrx *p, long long n_in, size_t out_pitch, int *ne, int *rem)
{
    long long ne64 = 0;
    if (csdr_amd_fmrx_plan(p->fill, n_in, p->Ld, p->agc_block, &ne64, rem) < 0) return -3;
    *ne = (int)ne64;
    if ((size_t)*ne > out_pitch && p->n_ch > 1) return fail_msg(-3, "fmrx: out_pitch %zu smaller than the %d audio samples of this call", out_pitch, *ne);
    if (*rem > FMRX_CARRY) return fail_msg(-3, "fmrx: internal carry of %d samples", *rem);
    return 0;
}

static bool fmrx_fused_shape(const csdr_amd_fmrx *p, const void *in, size_t in_pitch)
{
    return !p->force_generic && p->agc_block == 16 * NFM_FIR_SPAN && !((uintptr_t)in & 15) && !(in_pitch & 1);
}

// One call of the chain on n_in >= 1 samples per channel, planned (ne, rem: fmrx_plan_checked) and checked by the caller.  sq: the gated launch of the fused
// path (n_in gated samples, sq->h of them held in front of the rows at `in`), else null: the samples are the rows at `in`.
static long long fmrx_run(csdr_amd_fmrx *p, const csdr_complexf *in, size_t in_pitch, int n_in, int ne, int rem, int16_t *audio_s16, float *audio_f, size_t out_pitch,
                          bool fused, const FmrxSq *sq)
{
    const int nb = ne / p->agc_block, S = p->n_ch, fill = p->fill;
    csdr_amd_ctx *c = p->c; hipStream_t st = c->stream;
    cf32 *last_in = p->d_last[p->lflip].get(), *last_out = p->d_last[p->lflip ^ 1].get();
    const float q_per_amp = NFM_XQ / p->limit;
    if (fused) {
        p->last_kernel = sq ? "k_fmrx_front_sq" : "k_fmrx_front";
        if (p->held == csdr_amd_fmrx::HELD_PLANES) { const int rc = fmrx_move_held(p, false); if (rc) return rc; }
        FmrxArgs a;
        a.in = (const float2 *)in; a.in_pitch = in_pitch; a.n_in = (int)n_in; a.last = (const float2 *)last_in; a.carry = p->d_carry[p->cflip].get();
        a.carry_plane = (size_t)S * FMRX_CARRY; a.fill = fill; a.n_ch = S; a.max_amp = p->limit; a.q_per_amp = q_per_amp;
        a.sq = sq ? *sq : FmrxSq{nullptr, nullptr, 0, 0, 1, 0};
        const dim3 front_grid(nb, cdiv(S, 16));
        if (nb > 0) {
            float *peaks = fastagc_peaks_buffer(c, S, nb);
            if (!peaks) return -2;
            if (sq) hipLaunchKernelGGL(k_fmrx_front<true>, front_grid, dim3(256), 0, st, a, (const v4i *)p->d_fir_frags.get(), p->fir_scale, p->d_de.get(), p->a_pitch, peaks, nb + 2);
            else hipLaunchKernelGGL(k_fmrx_front<false>, front_grid, dim3(256), 0, st, a, (const v4i *)p->d_fir_frags.get(), p->fir_scale, p->d_de.get(), p->a_pitch, peaks, nb + 2);
            CSDR_LAUNCH_CHECK();
            const int rc = fastagc_ff_s16(c, p->d_de.get(), audio_f, audio_s16, S, nb, p->agc_block, p->a_pitch, out_pitch, out_pitch, p->agc_ref, p->d_agc_state.get(), true);
            if (rc) return rc;
        }
        // what the call keeps: into the other carry buffer behind a call with output, appended in place behind one without
        int8_t *keep = p->d_carry[nb > 0 ? p->cflip ^ 1 : p->cflip].get();
        if (sq) hipLaunchKernelGGL(k_fmrx_keep<true>, dim3(cdiv(rem, 256), S), dim3(256), 0, st, a, ne, rem, keep, (float2 *)last_out);
        else hipLaunchKernelGGL(k_fmrx_keep<false>, dim3(cdiv(rem, 256), S), dim3(256), 0, st, a, ne, rem, keep, (float2 *)last_out);
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

long long csdr_amd_fmrx_process(csdr_amd_fmrx *p, const csdr_complexf *in, size_t in_pitch, long long n_in, int16_t *audio_s16, float *audio_f, size_t out_pitch)
{
    if (!p) return fail_msg(-3, "fmrx: null object");
    if (p->sqB) return csdr_amd_fmrx_process_squelched(p, in, in_pitch, n_in, audio_s16, audio_f, out_pitch, nullptr, 0, nullptr, nullptr);
    if (n_in < 0 || (size_t)n_in > p->max_n) return fail_msg(-3, "fmrx: n_in should be 0 .. max_samples_per_call (%zu)", p->max_n);
    if (!n_in) return 0;
    if (!in || (in_pitch < (size_t)n_in && p->n_ch > 1)) return fail_msg(-3, "fmrx: in_pitch below n_in");
    int ne = 0, rem = 0;
    if (const int rc = fmrx_plan_checked(p, n_in, out_pitch, &ne, &rem)) return rc;
    return fmrx_run(p, in, in_pitch, (int)n_in, ne, rem, audio_s16, audio_f, out_pitch, fmrx_fused_shape(p, in, in_pitch), nullptr);
}

// ---- the squelch in front
int csdr_amd_fmrx_squelch_plan(int held, long long n_in, int block, long long *m, int *new_held)
{
    if (held < 0 || n_in < 0 || block < 1 || held >= block) return fail_msg(-3, "fmrx: squelch_plan needs block >= 1, 0 <= held < block, n_in >= 0");
    const long long e = (held + n_in) / block * block;                 // whole blocks go on; the rest waits
    if (m) *m = e;
    if (new_held) *new_held = (int)(held + n_in - e);
    return 0;
}

static int fmrx_squelched(const csdr_amd_fmrx *p)
{
    if (!p) return fail_msg(-3, "fmrx: null object");
    if (!p->sqB) return fail_msg(-3, "fmrx: the object was created without a squelch (csdr_amd_fmrx_create_squelched)");
    return 0;
}

int csdr_amd_fmrx_set_squelch_level(csdr_amd_fmrx *p, int ch, float level)
{
    if (const int rc = fmrx_squelched(p)) return rc;
    if (ch < -1 || ch >= p->n_ch) return fail_msg(-3, "fmrx: channel out of range");
    for (int k = (ch < 0 ? 0 : ch); k < (ch < 0 ? p->n_ch : ch + 1); k++) {
        p->lv[k] = level;
        if (p->sq_h == 0) p->lv_started[k] = level;                    // no block is under way: the next one starts under this level
    }
    p->lv_dirty = true;
    return 0;
}

int csdr_amd_fmrx_get_squelch_level(const csdr_amd_fmrx *p, int ch, float *level)
{
    if (const int rc = fmrx_squelched(p)) return rc;
    if (ch < 0 || ch >= p->n_ch || !level) return fail_msg(-3, "fmrx: channel out of range");
    *level = p->lv[ch];
    return 0;
}

int csdr_amd_fmrx_squelch_held(const csdr_amd_fmrx *p) { if (const int rc = fmrx_squelched(p)) return rc; return p->sq_h; }
long long csdr_amd_fmrx_squelch_block_index(const csdr_amd_fmrx *p) { if (const int rc = fmrx_squelched(p)) return rc; return p->sq_blk; }

long long csdr_amd_fmrx_process_squelched(csdr_amd_fmrx *p, const csdr_complexf *in, size_t in_pitch, long long n_in, int16_t *audio_s16, float *audio_f, size_t out_pitch,
                                          float *power, size_t power_pitch, uint8_t *open_flags, int *n_blocks)
{
    if (const int rc = fmrx_squelched(p)) return rc;
    if (n_in < 0 || (size_t)n_in > p->max_n) return fail_msg(-3, "fmrx: n_in should be 0 .. max_samples_per_call (%zu)", p->max_n);
    if (n_blocks) *n_blocks = 0;
    if (!n_in) return 0;
    if (!in || (in_pitch < (size_t)n_in && p->n_ch > 1)) return fail_msg(-3, "fmrx: in_pitch below n_in");
    const int B = p->sqB, S = p->n_ch, h = p->sq_h;
    long long m64 = 0; int nh = 0;
    if (csdr_amd_fmrx_squelch_plan(h, n_in, B, &m64, &nh) < 0) return -3;
    const int m = (int)m64, nbk = m / B;
    if ((power || open_flags) && (size_t)nbk > power_pitch) return fail_msg(-3, "fmrx: power_pitch %zu below the %d squelch blocks of this call", power_pitch, nbk);
    int ne = 0, rem = p->fill;
    if (m > 0) if (const int rc = fmrx_plan_checked(p, m, out_pitch, &ne, &rem)) return rc;
    csdr_amd_ctx *c = p->c; hipStream_t st = c->stream;
    const size_t carry_bytes = sizeof(float2) * (size_t)B * S;
    const bool fused = fmrx_fused_shape(p, in, in_pitch);
    if (fused) {
        if (p->lv_dirty) {
            float *hl = (float *)c->pinned_acquire(sizeof(float) * 2 * S); if (!hl) return -2;
            memcpy(hl, p->lv.data(), sizeof(float) * S); memcpy(hl + S, p->lv_started.data(), sizeof(float) * S);
            if (const int rc = c->pinned_upload(p->d_lv.get(), sizeof(float) * 2 * S)) return rc;
            p->lv_dirty = false;
        }
        if (p->sq_where == csdr_amd_fmrx::SQ_OBJ && h > 0) CSDR_HIP(hipMemcpyAsync(p->d_sq_carry[p->sflip].get(), p->sq_obj_carry, carry_bytes, hipMemcpyDeviceToDevice, st));
        const FmrxSq q{p->d_sq_carry[p->sflip].get(), p->d_fl.get(), p->fl_pitch, h, B, (B & (B - 1)) ? -1 : __builtin_ctz(B)};
        if (nbk > 0) {
            hipLaunchKernelGGL(k_fmrx_power, dim3(cdiv((size_t)nbk * S, 4)), dim3(256), 0, st, (const float2 *)in, in_pitch, q, p->sqd, nbk, S, p->d_lv.get(), p->d_pw.get(),
                               p->d_fl.get(), power, open_flags, power_pitch);
            CSDR_LAUNCH_CHECK();
            const long long rc = fmrx_run(p, in, in_pitch, m, ne, rem, audio_s16, audio_f, out_pitch, true, &q);
            if (rc < 0) return rc;
        }
        if (nh > 0) {                                                  // what waits for the next call: appended in place behind a call without a block
            float2 *keep = p->d_sq_carry[nbk > 0 ? p->sflip ^ 1 : p->sflip].get();
            hipLaunchKernelGGL(k_fmrx_sq_carry, dim3(cdiv((size_t)std::min<long long>(n_in, B), 256), S), dim3(256), 0, st, (const float2 *)in, in_pitch, (int)n_in, keep, h, B, m);
            CSDR_LAUNCH_CHECK();
            if (nbk > 0) p->sflip ^= 1;
        }
        p->sq_where = csdr_amd_fmrx::SQ_OWN;
        p->last_kernel = "k_fmrx_front_sq";
    } else {
        if (p->sq_where == csdr_amd_fmrx::SQ_OWN && h > 0) CSDR_HIP(hipMemcpyAsync(p->sq_obj_carry, p->d_sq_carry[p->sflip].get(), carry_bytes, hipMemcpyDeviceToDevice, st));
        (void)squelch_adopt(p->sq.get(), h, p->sq_blk, p->lv.data(), p->lv_started.data());
        const int got = csdr_amd_squelch_process(p->sq.get(), in, n_in, S > 1 ? in_pitch : std::max(in_pitch, (size_t)n_in), (csdr_complexf *)p->d_gated.get(), p->g_pitch, power,
                                                 power_pitch, open_flags, nullptr);
        if (got < 0) return got;
        if (got != nbk) return fail_msg(-4, "fmrx: the squelch completed %d blocks where %d were planned", got, nbk);
        if (nbk > 0) {
            const long long rc = fmrx_run(p, (const csdr_complexf *)p->d_gated.get(), p->g_pitch, m, ne, rem, audio_s16, audio_f, out_pitch, false, nullptr);
            if (rc < 0) return rc;
        }
        p->sq_where = csdr_amd_fmrx::SQ_OBJ;
        p->last_kernel = "k_nfm_deemph_mfma";
    }
    p->sq_h = nh; p->sq_blk += nbk;
    // a block that is under way behind this call's whole blocks was started by this call: its level is the one in force now
    if (nbk > 0 && memcmp(p->lv_started.data(), p->lv.data(), sizeof(float) * S)) { p->lv_started = p->lv; p->lv_dirty = true; }
    if (n_blocks) *n_blocks = nbk;
    return ne;
}

} // extern "C"
