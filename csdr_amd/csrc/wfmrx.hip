// wfmrx.hip -- the wide-band FM receive bank on baseband (csdr_amd_wfmrx): n_channels rows of decimated complexf samples, resident in HBM, to n_channels rows of
// s16 audio through
//
//   fmdemod_quadri_cf | fractional_decimator_ff <rate> [num_poly_points] [--prefilter] | deemphasis_wfm_ff <audio_rate> <tau> | convert_f_s16
//
// per channel: the tail of the reference README's first receive line, for the rows that csdr_amd_fastddc_bank, csdr_amd_ddc_process or csdr_amd_fir_decimate_cc
// leave on the device.  The stream model is the four commands' at the default buffer size: the decimator runs on windows of W demodulated samples from the first
// unprocessed one (csdr.c:1513-1524), what no whole window covers yet waits in the object (fewer than W floats per channel), `where` is carried, the de-emphasis
// is the reference's serial recurrence from state 0.  Positions (csdr_amd_fracdec's plan, audio.hip) depend on the stream's length only, sample values on the
// stream only, so an output's bits depend neither on the tiling nor on how the stream is cut into calls, and the two paths below agree bit for bit.
//
//   generic  csdr_amd_fmdemod_quadri_cf behind the held floats, csdr_amd_fractional_decimator_ff (k_fracdec), csdr_amd_deemphasis_wfm_ff, csdr_amd_convert_f_s16:
//            the stand-alone entry points on object-owned buffers.  Every shape.
//   fused    k_wfmrx_front: one workgroup = WF_G channels x up to WF_TO consecutive outputs reads the complexf rows itself (two 16-byte loads per four samples),
//            demodulates every staged sample once into LDS, evaluates an output's Lagrange coefficients once and applies them to every channel of the group; the
//            demodulated floats never go to HBM.  k_wfmrx_keep then writes the samples the call keeps (fewer than W) into the OTHER of two small carry buffers:
//            k_wfmrx_front only reads the one it was given.  k_wfmrx_tail runs de-emphasis and convert_f_s16 over LDS tiles: one wave walks 16 channels' recurrences
//            while the other three store the tile before and fetch the next one.  Needs no prefilter, num_poly_points <= 16, a rate at which a tile's inputs fit the LDS rows, 16-byte
//            aligned rows and an even in_pitch.
//
// With a squelch in front (csdr_amd_wfmrx_create_squelched: squelch_and_smeter_cc | the chain above) the channel's input is cut into blocks of B samples counted
// from the reset; whole blocks go on, gated, and what lies behind the last whole block (fewer than B complexf per channel) waits in the object.  Power, gate and
// levels are csdr_amd_squelch's, exactly as in fmrx.hip, whose power pass and carry kernel serve here too (rx_squelch_dev.hpp).
//   generic  an internal csdr_amd_squelch writes the gated rows to a scratch buffer; the generic path above runs over them.  Every shape.
//   fused    k_fmrx_power: one wave per (channel, block) reads held ++ call once and writes the power and the open flag.  k_wfmrx_front<P, true> and
//            k_wfmrx_keep<true> ("k_wfmrx_front_sq") read the call's gated sample k as held[k] for k < h, else in[k - h], and as (0, 0) when the flag of block
//            k / B is closed: the gated rows never exist in HBM.  The staged span starts on an even ROW index k - h, so a quad that lies with its predecessor in
//            one open block behind the held samples takes the plain kernel's two 16-byte loads; a quad in one closed block loads nothing and stages four zeros;
//            any other quad (two blocks, the held / call seam, the call's edges) goes sample by sample, each under its own block's flag.  k_fmrx_sq_carry moves
//            what the call leaves behind its last whole block into the OTHER of two carry buffers.  Any call length; the preconditions are the plain kernel's.
#include "bank.hpp"
#include "audio_dev.hpp"
#include "rx_squelch_dev.hpp"
#include <math.h>
#include <string.h>

using namespace csdr_amd;

namespace {

constexpr int WF_G = 8;                    // channels of a workgroup of k_wfmrx_front
constexpr int WF_TO = 256;                 // outputs of a workgroup at most: one per thread
constexpr int WF_SPAN = 1536;              // filter inputs a workgroup stages per channel at most
constexpr int WF_BATCH = 3;                // quads of four inputs a lane loads at a time while it stages a channel
constexpr int WF_RP = WF_SPAN + 4;         // LDS row pitch in floats: rows stay 16-byte aligned and start four banks apart
constexpr int WF_PAD = 4;                  // floats in front of a generic-path row: index -1 of a fresh two-point stream reads a zero

struct WfmrxArgs {
    const float2 *in; size_t in_pitch; int n_in;       // the call's rows
    const float2 *last;                                // [n_ch]: the sample in front of in[.][0]
    const float *carry; int carry_pitch;               // [n_ch][carry_pitch]: the demodulated samples held from earlier calls
    int held, n_ch;
    FmrxSq sq;                                         // gated launches only: n_in gated samples, sq.h of them from sq.held, the others the rows' first n_in - sq.h
};

// sample k < n_in of the call, k == -1: the stream's sample in front of the call.  SQ: the gated stream, a sample of a closed block is (0, 0) and is not fetched
template <bool SQ> __device__ __forceinline__ float2 wfmrx_sample(const WfmrxArgs &a, const float2 *x, int ch, int k)
{
    if (k < 0) return a.last[ch];
    if (!SQ) return x[k];
    if (!a.sq.flags[(size_t)ch * a.sq.fl_pitch + fmrx_sq_block(a.sq, k)]) return make_float2(0.f, 0.f);
    return k < a.sq.h ? a.sq.held[(size_t)ch * a.sq.B + k] : x[k - a.sq.h];
}

// filter input i of channel ch (its row x, its held floats): i < 0: zero; i < held: a held float; then sample i - held of the call, demodulated; behind the
// call's samples: zero (not used by any output)
template <bool SQ> __device__ __forceinline__ float wfmrx_input(const WfmrxArgs &a, const float2 *x, const float *held, int ch, int i)
{
    if (i < 0) return 0.f;
    if (i < a.held) return held[i];
    const int k = i - a.held;
    if (k >= a.n_in) return 0.f;
    if (!SQ) {
        const float2 s = x[k], p = k ? x[k - 1] : a.last[ch];
        return fmdemod_quadri(s.x, s.y, p.x, p.y);
    }
    const float2 s = wfmrx_sample<SQ>(a, x, ch, k), p = wfmrx_sample<SQ>(a, x, ch, k - 1);
    return fmdemod_quadri(s.x, s.y, p.x, p.y);
}

// One channel's staged span into its LDS row: the filter inputs s0 .. s0 + 4 nquads - 1 (s0 - a.held is an even sample of the call), a lane demodulates four
// consecutive samples at a time.  The loads of WF_BATCH such quads are issued in front of their arithmetic (from clamped, always valid addresses: a quad at the
// call's edges takes the slow path and does not use them), so a wave waits for memory once per batch, not once per quad.
__device__ __forceinline__ void wfmrx_stage_plain(const WfmrxArgs &a, const float2 *x, const float *held, int ch, int s0, int nquads, int lane, float *row)
{
    const bool can = a.n_in >= 6;
    const int k_hi = (a.n_in - 4) & ~1;
    for (int j0 = 0; 64 * j0 < nquads; j0 += WF_BATCH) {
        float4 U[WF_BATCH], V[WF_BATCH]; float2 Q[WF_BATCH];
        if (can) {
#pragma unroll
            for (int j = 0; j < WF_BATCH; j++) {
                const int qd = lane + 64 * (j0 + j), k = s0 - a.held + 4 * qd;      // k is even
                const int kc = qd < nquads ? min(max(k, 2), k_hi) : 2;
                Q[j] = x[kc - 1];
                U[j] = *reinterpret_cast<const float4 *>(x + kc); V[j] = *reinterpret_cast<const float4 *>(x + kc + 2);
            }
        }
#pragma unroll
        for (int j = 0; j < WF_BATCH; j++) {
            const int qd = lane + 64 * (j0 + j), i = s0 + 4 * qd, k = i - a.held;
            if (qd >= nquads) continue;
            float4 d;
            if (k >= 2 && k + 3 < a.n_in) {
                const float4 u = U[j], v = V[j]; const float2 p = Q[j];
                d.x = fmdemod_quadri(u.x, u.y, p.x, p.y); d.y = fmdemod_quadri(u.z, u.w, u.x, u.y);
                d.z = fmdemod_quadri(v.x, v.y, u.z, u.w); d.w = fmdemod_quadri(v.z, v.w, v.x, v.y);
            } else {
                d.x = wfmrx_input<false>(a, x, held, ch, i); d.y = wfmrx_input<false>(a, x, held, ch, i + 1);
                d.z = wfmrx_input<false>(a, x, held, ch, i + 2); d.w = wfmrx_input<false>(a, x, held, ch, i + 3);
            }
            *reinterpret_cast<float4 *>(row + 4 * qd) = d;
        }
    }
}

// The same behind the squelch (s0 - a.held - a.sq.h, the ROW index, is even).  How the lane fetches quad qd (the call's samples k .. k + 3): 1 = the four and
// their predecessor lie in one open block, all in the call's rows: the plain kernel's loads; 0 = the four lie in one closed block: nothing to fetch, four zeros
// (a zero sample demodulates to 0 behind any predecessor); 2 = sample by sample.  The flag is uniform over a block, so the wave first asks for the kind of a
// whole run of 64 quads (the 256 samples its lanes stage at one batch slot), with scalar arithmetic and one scalar flag load: 1 and 0 as above for all of them,
// 2 = the run crosses a block boundary, the held / call seam or an edge, and only then every lane asks for its own quad.  The run kinds of a batch are asked
// for one batch ahead: their flag loads are under way while the batch in front is demodulated.
__device__ __forceinline__ void wfmrx_stage_gated(const WfmrxArgs &a, const float2 *x, const float *held, int ch, int s0, int nquads, int lane, float *row)
{
    const int h = a.sq.h;
    const int chu = __builtin_amdgcn_readfirstlane(ch);
    auto run_kind = [&](int q0) -> int {                               // q0: the run's first quad, the same in every lane
        const int k = s0 - a.held + 4 * q0;
        if (q0 + 64 > nquads || k - h < 2 || k + 255 >= a.n_in) return 2;
        const int b = fmrx_sq_block(a.sq, k - 1);
        if (k + 255 - b * a.sq.B >= a.sq.B) return 2;
        return a.sq.flags[(size_t)chu * a.sq.fl_pitch + b] != 0;
    };
    auto quad_kind = [&](int qd) -> int {
        const int k = s0 - a.held + 4 * qd;
        if (qd >= nquads || k < 0 || k + 3 >= a.n_in) return 2;
        const int b = fmrx_sq_block(a.sq, k), off = k - b * a.sq.B;
        if (off + 3 >= a.sq.B) return 2;                               // the four straddle two blocks
        if (!a.sq.flags[(size_t)ch * a.sq.fl_pitch + b]) return 0;
        return off >= 1 && k - h >= 2 ? 1 : 2;                         // (the predecessor: in the same block, and in the rows)
    };
    int kind_next[WF_BATCH];
#pragma unroll
    for (int j = 0; j < WF_BATCH; j++) kind_next[j] = run_kind(64 * j);
    for (int j0 = 0; 64 * j0 < nquads; j0 += WF_BATCH) {
        float4 U[WF_BATCH], V[WF_BATCH]; float2 Q[WF_BATCH];
        int kind[WF_BATCH];
#pragma unroll
        for (int j = 0; j < WF_BATCH; j++) {
            kind[j] = kind_next[j];
            if (kind[j] == 2) kind[j] = quad_kind(lane + 64 * (j0 + j));
            if (kind[j] == 1) {
                const int r = s0 - a.held + 4 * (lane + 64 * (j0 + j)) - h;         // the row index: even, >= 2, r + 3 < n_in - h
                Q[j] = x[r - 1];
                U[j] = *reinterpret_cast<const float4 *>(x + r); V[j] = *reinterpret_cast<const float4 *>(x + r + 2);
            }
        }
#pragma unroll
        for (int j = 0; j < WF_BATCH; j++) kind_next[j] = run_kind(64 * (j0 + WF_BATCH + j));
#pragma unroll
        for (int j = 0; j < WF_BATCH; j++) {
            const int qd = lane + 64 * (j0 + j), i = s0 + 4 * qd;
            if (qd >= nquads) continue;
            float4 d;
            if (kind[j] == 0) {
                d = make_float4(0.f, 0.f, 0.f, 0.f);
            } else if (kind[j] == 1) {
                const float4 u = U[j], v = V[j]; const float2 p = Q[j];
                d.x = fmdemod_quadri(u.x, u.y, p.x, p.y); d.y = fmdemod_quadri(u.z, u.w, u.x, u.y);
                d.z = fmdemod_quadri(v.x, v.y, u.z, u.w); d.w = fmdemod_quadri(v.z, v.w, v.x, v.y);
            } else {
                d.x = wfmrx_input<true>(a, x, held, ch, i); d.y = wfmrx_input<true>(a, x, held, ch, i + 1);
                d.z = wfmrx_input<true>(a, x, held, ch, i + 2); d.w = wfmrx_input<true>(a, x, held, ch, i + 3);
            }
            *reinterpret_cast<float4 *>(row + 4 * qd) = d;
        }
    }
}

// grid (ceil(n_out / tile_out), ceil(n_ch / WF_G)), 256 threads.  out[ch][k] = sum_w coeff_w(frac[k]) * input[lo[k] + w] for the tile's outputs.
// The host chooses tile_out <= WF_TO so that the inputs of tile_out consecutive outputs (and the alignment's spare ones) fit WF_SPAN.  SQ: the gated launch.
template <int P, bool SQ>
__global__ __launch_bounds__(256) void k_wfmrx_front(WfmrxArgs a, const int *__restrict__ lo, const float *__restrict__ frac, int n_out, int tile_out,
                                                     const float *__restrict__ denom, float *__restrict__ out, size_t out_pitch)
{
    __shared__ __attribute__((aligned(16))) float rows[WF_G * WF_RP];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int k0 = blockIdx.x * tile_out, kn = min(tile_out, n_out - k0);
    const int c0 = blockIdx.y * WF_G;
    const int first = lo[k0];
    const int h = SQ ? a.sq.h : 0;                                     // gated: the call's sample k is row index k - h
    const int s0 = first - ((first - a.held - h) & 1);                 // the staged span starts on an even row index of the call: 16-byte loads
    const int len = min(lo[k0 + kn - 1] + P - s0, WF_SPAN);
    const int nquads = (len + 3) >> 2;
    // wave wv stages the channels wv, wv + 4 (rows of channels past the last one re-read it)
    for (int g = wv; g < WF_G; g += 4) {
        const int ch = min(c0 + g, a.n_ch - 1);
        const float2 *x = a.in + (size_t)ch * a.in_pitch;
        const float *held = a.carry + (size_t)ch * a.carry_pitch;
        if constexpr (SQ) wfmrx_stage_gated(a, x, held, ch, s0, nquads, lane, rows + g * WF_RP);
        else wfmrx_stage_plain(a, x, held, ch, s0, nquads, lane, rows + g * WF_RP);
    }
    __syncthreads();
    if (tid >= kn) return;
    const float fx = frac[k0 + tid];
    const int l = min(max(lo[k0 + tid] - s0, 0), WF_SPAN - P);
    float cf[P];
#pragma unroll
    for (int w = 0; w < P; w++) cf[w] = fracdec_coeff(fx, w, P, -(P / 2) + 1, denom[w]);
#pragma unroll
    for (int g = 0; g < WF_G; g++) {
        if (c0 + g >= a.n_ch) break;
        const float *r = rows + g * WF_RP + l;
        float acc = 0.f;
#pragma unroll
        for (int w = 0; w < P; w++) acc += cf[w] * r[w];
        out[(size_t)(c0 + g) * out_pitch + k0 + tid] = acc;
    }
}

// grid (max(ceil(rem / 256), 1), n_ch): the filter inputs from .. from + rem - 1, which the call keeps, to keep[ch][0 .. rem).  keep == a.carry (a call without a
// window: from == 0): only the call's samples are appended.  Thread 0 of a channel leaves the call's last (gated) sample in last_out.
template <bool SQ> __global__ __launch_bounds__(256) void k_wfmrx_keep(WfmrxArgs a, int from, int rem, float *keep, float2 *__restrict__ last_out)
{
    const int ch = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const float2 *x = a.in + (size_t)ch * a.in_pitch;
    if (j == 0) last_out[ch] = wfmrx_sample<SQ>(a, x, ch, a.n_in - 1);
    if (j >= rem) return;
    const int i = from + j;
    if (i < a.held && keep == a.carry) return;
    keep[(size_t)ch * a.carry_pitch + j] = wfmrx_input<SQ>(a, x, a.carry + (size_t)ch * a.carry_pitch, ch, i);
}

// deemphasis_wfm_ff | convert_f_s16 for rows of pre-de-emphasis floats.  grid (ceil(n_ch / WT_CH)), 256 threads; time is walked in tiles of WT_T samples through
// three LDS buffers (row stride WT_T + 1 floats: conflict free for lanes walking their own rows).  Wave 0 runs the channels' recurrences over tile t (the
// reference's, operation for operation: the serial part, two dependent operations per sample) while waves 1 .. 3 convert and store tile t - 1 and fetch tile t + 1,
// all with coalesced rows: the recurrence never waits for memory.
constexpr int WT_CH = 16, WT_T = 256, WT_RP = WT_T + 1, WT_U = 16;
__device__ __forceinline__ void wfmrx_tail_load(float *buf, const float *__restrict__ in, size_t in_pitch, int c0, int nrows, int t0, int n, int w3, int lane)
{
    for (int r = w3; r < nrows; r += 3) {
        const float *src = in + (size_t)(c0 + r) * in_pitch + t0;
#pragma unroll
        for (int q = 0; q < WT_T / 64; q++) if (t0 + lane + 64 * q < n) buf[r * WT_RP + lane + 64 * q] = src[lane + 64 * q];
    }
}
__device__ __forceinline__ void wfmrx_tail_store(const float *buf, int16_t *__restrict__ out_s16, float *__restrict__ out_f, size_t out_pitch, int c0, int nrows, int t0, int n,
                                                 int w, int nw, int lane)
{
    for (int r = w; r < nrows; r += nw) {
        const size_t o = (size_t)(c0 + r) * out_pitch + t0;
#pragma unroll
        for (int q = 0; q < WT_T / 64; q++) {
            const int t = lane + 64 * q;
            if (t0 + t >= n) continue;
            const float v = buf[r * WT_RP + t];
            if (out_f) out_f[o + t] = v;
            if (out_s16) out_s16[o + t] = (int16_t)f_to_s16(v);
        }
    }
}
__global__ __launch_bounds__(256) void k_wfmrx_tail(const float *__restrict__ in, size_t in_pitch, int n_ch, int n, float alpha, float *__restrict__ state,
                                                    int16_t *__restrict__ out_s16, float *__restrict__ out_f, size_t out_pitch)
{
    __shared__ float tile[3][WT_CH * WT_RP];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c0 = blockIdx.x * WT_CH, nrows = min(WT_CH, n_ch - c0);
    const float one_minus = 1 - alpha;
    float y = 0.f;
    if (wv == 0 && lane < nrows) { y = state[c0 + lane]; if (y != y) y = 0.f; }      // NaN state reset, libcsdr.c:1092
    if (wv) wfmrx_tail_load(tile[0], in, in_pitch, c0, nrows, 0, n, wv - 1, lane);
    __syncthreads();
    const int n_tiles = (n + WT_T - 1) / WT_T;
    for (int t = 0; t < n_tiles; t++) {
        const int t0 = t * WT_T, cols = min(WT_T, n - t0);
        if (wv == 0) {
            if (lane < nrows) {
                float *row = tile[t % 3] + lane * WT_RP;
                int k = 0;
                for (; k + WT_U <= cols; k += WT_U) {                  // WT_U samples at a time: their LDS reads are in flight together
                    float v[WT_U];
#pragma unroll
                    for (int e = 0; e < WT_U; e++) v[e] = row[k + e];
#pragma unroll
                    for (int e = 0; e < WT_U; e++) { y = deemph_wfm_step(alpha, one_minus, v[e], y); v[e] = y; }
#pragma unroll
                    for (int e = 0; e < WT_U; e++) row[k + e] = v[e];
                }
                for (; k < cols; k++) { y = deemph_wfm_step(alpha, one_minus, row[k], y); row[k] = y; }
            }
        } else {
            if (t) wfmrx_tail_store(tile[(t - 1) % 3], out_s16, out_f, out_pitch, c0, nrows, t0 - WT_T, n, wv - 1, 3, lane);
            if (t + 1 < n_tiles) wfmrx_tail_load(tile[(t + 1) % 3], in, in_pitch, c0, nrows, t0 + WT_T, n, wv - 1, lane);
        }
        __syncthreads();
    }
    wfmrx_tail_store(tile[(n_tiles - 1) % 3], out_s16, out_f, out_pitch, c0, nrows, (n_tiles - 1) * WT_T, n, wv, 4, lane);
    if (wv == 0 && lane < nrows) state[c0 + lane] = y;
}

// the windows a call of csdr_amd_fractional_decimator_ff walks in CLI mode, positions only (libcsdr.c:763, 790-791; csdr.c:1513-1524)
struct WfmrxWalk { long long n_out; float where; long long base; };
WfmrxWalk wfmrx_walk(float rate, int P, int taps, int W, float where, long long total)
{
    WfmrxWalk r{0, where, 0};
    const int xifirst = -(P / 2) + 1;
    while (r.base + W <= total) {
        int hi;
        for (; (hi = (int)ceilf(r.where)) + P + taps < W; r.where += rate) r.n_out++;
        const int processed = (hi - 1) + xifirst;
        r.where -= processed;
        if (processed <= 0) break;
        r.base += processed;
    }
    return r;
}

// what create and plan refuse: 0 or the error
int wfmrx_check(float rate, int P, int taps, int W)
{
    if (!(rate > 1.0f) || !(rate <= 1e6f)) return fail_msg(-3, "wfmrx: rate should be > 1 (and at most 1e6)");
    if (P < 2 || P > 64 || (P & 1)) return fail_msg(-3, "wfmrx: num_poly_points should be even, 2 .. 64");
    if (taps < 0 || taps > (1 << 16)) return fail_msg(-3, "wfmrx: taps_length should be 0 .. 65536");
    if (W > (1 << 24)) return fail_msg(-3, "wfmrx: window should be at most 2^24");
    if (W < 3 * P / 2 + taps + 1) return fail_msg(-3, "wfmrx: window %d is too short: a window call advances by at least one sample from 3 * num_poly_points / 2 + taps_length + 1 = %d on", W, 3 * P / 2 + taps + 1);
    if (ceilf(rate) > (float)(3 * P / 2 + taps + 1)) return fail_msg(-3, "wfmrx: rate %g is too large for %d points and %d taps: a window call would advance beyond its window (ceil(rate) <= 3 * num_poly_points / 2 + taps_length + 1)", rate, P, taps);
    return 0;
}

} // namespace

struct csdr_amd_wfmrx : Bank {
    float rate, tau, alpha; int P, taps_length, W, audio_rate, held, tile_out;
    size_t max_n, d_pitch, a_pitch;
    Owned<csdr_amd_fracdec, csdr_amd_fracdec_destroy> fd;      // `where` and the plan
    DevBuf<cf32> d_last[2]; int lflip;              // the sample in front of the next call: the fused path reads one and writes the other
    DevBuf<float> d_dem;                            // generic path: [n_ch][d_pitch], WF_PAD zeros, the held floats, the call's demodulated samples behind them
    DevBuf<float> d_carry[2]; int cflip;            // the held floats between calls: [n_ch][W] each
    enum { HELD_BOTH, HELD_DEM, HELD_CARRY } where_held;          // where the held floats are (both after a reset: there are none)
    DevBuf<float> d_pre;                            // [n_ch][a_pitch]: the decimator's outputs
    DevBuf<int16_t> d_s16;                          // generic path: convert_f_s16 of d_pre, flat
    DevBuf<float> d_state;                          // [n_ch]: deemphasis_wfm_ff's last output
    // the squelch in front (create_squelched; sqB == 0: none), as csdr_amd_fmrx's
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

int csdr_amd_wfmrx_plan(float rate, int num_poly_points, int taps_length, int window, float where, int held, long long n_in, long long *n_out, float *new_where, int *new_held)
{
    const int W = window ? window : 1024;
    if (const int rc = wfmrx_check(rate, num_poly_points, taps_length, W)) return rc;
    if (held < 0 || n_in < 0 || !(where >= 0.f) || !(where <= (float)W)) return fail_msg(-3, "wfmrx: plan needs held >= 0, n_in >= 0 and 0 <= where <= window");
    WfmrxWalk r{0, where, 0};
    if (n_in > 0) r = wfmrx_walk(rate, num_poly_points, taps_length, W, where, held + n_in);      // (a call without input does nothing)
    if (held + n_in - r.base > 0x7fffffffLL) return fail_msg(-3, "wfmrx: plan: the held input exceeds an int");
    if (n_out) *n_out = r.n_out;
    if (new_where) *new_where = r.where;
    if (new_held) *new_held = (int)(held + n_in - r.base);
    return 0;
}

// squelch_block 0: no squelch
static csdr_amd_wfmrx *wfmrx_create(csdr_amd_ctx *ctx, int n_channels, float rate, int num_poly_points, const float *host_prefilter_taps, int taps_length, int window,
                                    float tau, int audio_rate, size_t max_samples_per_call, int squelch_block, int use_every_nth, const float *levels)
{
    if (bank_create_check("wfmrx", ctx, n_channels, 65535) < 0) return nullptr;                // (a channel, or a group of them, is a grid row)
    const int W = window ? window : 1024, nt = host_prefilter_taps ? taps_length : 0;
    if (wfmrx_check(rate, num_poly_points, nt, W) < 0) return nullptr;
    if (!(tau > 0) || audio_rate < 1) { fail_msg(-3, "wfmrx: tau should be > 0 and audio_rate >= 1"); return nullptr; }
    if (max_samples_per_call < 1 || max_samples_per_call > ((size_t)1 << 30)) { fail_msg(-3, "wfmrx: max_samples_per_call should be 1 .. 2^30"); return nullptr; }
    Owned<csdr_amd_wfmrx, csdr_amd_wfmrx_destroy> p(new csdr_amd_wfmrx());
    p->c = ctx; p->n_ch = n_channels; p->rate = rate; p->P = num_poly_points; p->taps_length = nt; p->W = W; p->tau = tau; p->audio_rate = audio_rate;
    p->max_n = max_samples_per_call;
    p->sqB = squelch_block; p->sqd = use_every_nth;
    p->max_m = p->max_n + (squelch_block ? squelch_block - 1 : 0);     // a squelched call hands on up to sqB - 1 held samples more
    const float dt = (float)(1.0 / audio_rate);                        // libcsdr.c:1090-1091, as csdr_amd_deemphasis_wfm_ff
    p->alpha = dt / (tau + dt);
    // outputs of a workgroup of the fused kernel: the inputs of tile_out consecutive outputs, P more, one for the even start and three for the last quad fit WF_SPAN
    p->tile_out = (int)std::min((double)WF_TO, floor((WF_SPAN - num_poly_points - 8) / (double)rate));
    p->fd.reset(csdr_amd_fracdec_create(rate, num_poly_points, host_prefilter_taps, nt));
    if (!p->fd) return nullptr;
    csdr_amd_fracdec_set_cli_bufsize(p->fd.get(), W);
    p->d_pitch = (WF_PAD + (size_t)W + p->max_m + 3) & ~(size_t)3;
    p->a_pitch = ((size_t)csdr_amd_wfmrx_max_output(p.get(), (long long)p->max_n) + 7) & ~(size_t)3;
    hipError_t e = hipSuccess;
    auto alloc = [&](auto &b, size_t bytes) { if (e == hipSuccess) e = dev_alloc(b, bytes); };
    alloc(p->d_last[0], sizeof(cf32) * n_channels); alloc(p->d_last[1], sizeof(cf32) * n_channels);
    alloc(p->d_dem, sizeof(float) * p->d_pitch * n_channels);
    alloc(p->d_carry[0], sizeof(float) * (size_t)W * n_channels); alloc(p->d_carry[1], sizeof(float) * (size_t)W * n_channels);
    alloc(p->d_pre, sizeof(float) * p->a_pitch * n_channels);
    alloc(p->d_s16, sizeof(int16_t) * p->a_pitch * n_channels);
    alloc(p->d_state, sizeof(float) * n_channels);
    if (squelch_block) {
        const int B = squelch_block;
        p->lv.assign(n_channels, 0.f);
        if (levels) p->lv.assign(levels, levels + n_channels);
        p->fl_pitch = (p->max_n + B - 1) / B;                          // (B - 1 held + max_n) / B blocks at the most
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
    if (e != hipSuccess) { fail_msg(-2, "wfmrx: out of device memory"); return nullptr; }
    if (hipMemsetAsync(p->d_pre.get(), 0, sizeof(float) * p->a_pitch * n_channels, ctx->stream) != hipSuccess) { fail_msg(-2, "wfmrx: memset"); return nullptr; }
    if (csdr_amd_wfmrx_reset(p.get()) < 0) return nullptr;
    return p.release();
}

csdr_amd_wfmrx *csdr_amd_wfmrx_create(csdr_amd_ctx *ctx, int n_channels, float rate, int num_poly_points, const float *host_prefilter_taps, int taps_length, int window,
                                      float tau, int audio_rate, size_t max_samples_per_call)
{
    return wfmrx_create(ctx, n_channels, rate, num_poly_points, host_prefilter_taps, taps_length, window, tau, audio_rate, max_samples_per_call, 0, 1, nullptr);
}

csdr_amd_wfmrx *csdr_amd_wfmrx_create_squelched(csdr_amd_ctx *ctx, int n_channels, float rate, int num_poly_points, const float *host_prefilter_taps, int taps_length,
                                                int window, float tau, int audio_rate, size_t max_samples_per_call, int squelch_block, int use_every_nth,
                                                const float *levels)
{
    if (squelch_block < 1 || squelch_block > 65536) { fail_msg(-3, "wfmrx: squelch_block should be 1 .. 65536"); return nullptr; }
    if (use_every_nth < 1) { fail_msg(-3, "wfmrx: use_every_nth should be >= 1"); return nullptr; }
    return wfmrx_create(ctx, n_channels, rate, num_poly_points, host_prefilter_taps, taps_length, window, tau, audio_rate, max_samples_per_call, squelch_block,
                        use_every_nth, levels);
}

int csdr_amd_wfmrx_reset(csdr_amd_wfmrx *p)
{
    if (!p) return fail_msg(-3, "wfmrx: null object");
    hipStream_t st = p->c->stream;
    p->held = 0; p->lflip = p->cflip = 0; p->where_held = csdr_amd_wfmrx::HELD_BOTH;
    csdr_amd_fracdec_set_where(p->fd.get(), (float)(p->P / 2 - 1));                               // fractional_decimator_ff_init, libcsdr.c:736
    CSDR_HIP(hipMemsetAsync(p->d_dem.get(), 0, sizeof(float) * p->d_pitch * p->n_ch, st));
    for (int k = 0; k < 2; k++) {
        CSDR_HIP(hipMemsetAsync(p->d_carry[k].get(), 0, sizeof(float) * (size_t)p->W * p->n_ch, st));
        CSDR_HIP(hipMemsetAsync(p->d_last[k].get(), 0, sizeof(cf32) * p->n_ch, st));               // the CLI starts fmdemod from (0, 0) (csdr.c:1044)
    }
    CSDR_HIP(hipMemsetAsync(p->d_state.get(), 0, sizeof(float) * p->n_ch, st));                    // deemphasis_wfm_ff starts from 0 (csdr.c:1059)
    if (p->sqB) {                                                          // the block count and the held samples start over; the levels stay
        p->sq_h = 0; p->sq_blk = 0; p->sflip = 0; p->sq_where = csdr_amd_wfmrx::SQ_NOWHERE; p->lv_started = p->lv; p->lv_dirty = true;
    }
    return 0;
}

// one channel's held floats, previous sample and de-emphasis state to zero; the count of held samples and `where` are the bank's and stay
int csdr_amd_wfmrx_reset_channel(csdr_amd_wfmrx *p, int ch)
{
    if (!p || ch < 0 || ch >= p->n_ch) return fail_msg(-3, "wfmrx: channel out of range");
    hipStream_t st = p->c->stream;
    CSDR_HIP(hipMemsetAsync(p->d_dem.get() + (size_t)ch * p->d_pitch, 0, sizeof(float) * p->d_pitch, st));
    for (int k = 0; k < 2; k++) {
        CSDR_HIP(hipMemsetAsync(p->d_carry[k].get() + (size_t)ch * p->W, 0, sizeof(float) * p->W, st));
        CSDR_HIP(hipMemsetAsync(p->d_last[k].get() + ch, 0, sizeof(cf32), st));
    }
    CSDR_HIP(hipMemsetAsync(p->d_state.get() + ch, 0, sizeof(float), st));
    if (p->sqB) {                                                          // the channel's held squelch samples; the block phase is the bank's and stays
        for (int k = 0; k < 2; k++) CSDR_HIP(hipMemsetAsync(p->d_sq_carry[k].get() + (size_t)ch * p->sqB, 0, sizeof(float2) * p->sqB, st));
        CSDR_HIP(hipMemsetAsync(p->sq_obj_carry + (size_t)ch * p->sqB, 0, sizeof(float2) * p->sqB, st));
    }
    return 0;
}

void csdr_amd_wfmrx_destroy(csdr_amd_wfmrx *p) { destroy_on_stream(p); }
int csdr_amd_wfmrx_force_generic(csdr_amd_wfmrx *p, int on) { return bank_force_generic(p, "wfmrx", on); }
const char *csdr_amd_wfmrx_kernel_name(const csdr_amd_wfmrx *p) { return bank_kernel_name(p); }
int csdr_amd_wfmrx_held(const csdr_amd_wfmrx *p) { return p ? p->held : -1; }
float csdr_amd_wfmrx_where(const csdr_amd_wfmrx *p) { return p ? csdr_amd_fracdec_get_where(p->fd.get()) : -1.f; }

long long csdr_amd_wfmrx_max_output(const csdr_amd_wfmrx *p, long long n_in)
{
    if (!p || n_in <= 0) return 0;
    // every output moves the position on by `rate`, the windows' advances sum to at most held + n_in <= W - 1 + n_in, and what the position is ahead of them
    // changes by less than one sample over a call; + 2 for the float arithmetic of the positions
    // (behind a squelch a call hands on up to sqB - 1 held samples more)
    return (long long)floor(((double)p->W + (double)n_in + (double)(p->sqB ? p->sqB - 1 : 0)) / (double)p->rate) + 2;
}
long long csdr_amd_wfmrx_max_out(const csdr_amd_wfmrx *p, long long n_in) { return csdr_amd_wfmrx_max_output(p, n_in); }

// the held floats from where the other path left them to where this one reads them: n_ch rows of `held` floats
static int wfmrx_move_held(csdr_amd_wfmrx *p, bool to_dem)
{
    if (!p->held) return 0;
    float *carry = p->d_carry[p->cflip].get(), *dem = p->d_dem.get() + WF_PAD;
    const size_t cp = sizeof(float) * p->W, dp = sizeof(float) * p->d_pitch, w = sizeof(float) * p->held;
    if (to_dem) CSDR_HIP(hipMemcpy2DAsync(dem, dp, carry, cp, w, p->n_ch, hipMemcpyDeviceToDevice, p->c->stream));
    else CSDR_HIP(hipMemcpy2DAsync(carry, cp, dem, dp, w, p->n_ch, hipMemcpyDeviceToDevice, p->c->stream));
    return 0;
}

// the plan of a call that hands n_in >= 1 samples to the chain, checked against the caller's rows and the object's buffers: 0, or the error
static int wfmrx_plan_checked(const csdr_amd_wfmrx *p, long long n_in, size_t out_pitch, int *n_out, int *rem)
{
    long long n_out64 = 0; float where_after = 0;
    if (csdr_amd_wfmrx_plan(p->rate, p->P, p->taps_length, p->W, p->fd->where, p->held, n_in, &n_out64, &where_after, rem) < 0) return -3;
    *n_out = (int)n_out64;
    if ((size_t)*n_out > out_pitch && p->n_ch > 1) return fail_msg(-3, "wfmrx: out_pitch %zu smaller than the %d audio samples of this call", out_pitch, *n_out);
    if (*rem >= p->W || (size_t)*n_out > p->a_pitch) return fail_msg(-3, "wfmrx: internal: %d held samples, %d outputs", *rem, *n_out);
    return 0;
}

static bool wfmrx_fused_shape(const csdr_amd_wfmrx *p, const void *in, size_t in_pitch)
{
    return !p->force_generic && !p->taps_length && p->P <= 16 && p->tile_out >= 16 && !((uintptr_t)in & 15) && !(in_pitch & 1);
}

// One call of the chain on n_in >= 1 samples per channel, planned (n_out, rem: wfmrx_plan_checked) and checked by the caller.  sq: the gated launch of the fused
// path (n_in gated samples, sq->h of them held in front of the rows at `in`), else null: the samples are the rows at `in`.
static long long wfmrx_run(csdr_amd_wfmrx *p, const csdr_complexf *in, size_t in_pitch, int n_in, int n_out, int rem, int16_t *audio_s16, float *audio_f, size_t out_pitch,
                           bool fused, const FmrxSq *sq)
{
    csdr_amd_fracdec *fd = p->fd.get();
    const int S = p->n_ch, held = p->held, total = held + n_in, from = total - rem;
    csdr_amd_ctx *c = p->c; hipStream_t st = c->stream;
    const bool windows = total >= p->W;                                // (the decimator is never handed less than a window: it would take it for a stream's end)
    if (fused) {
        p->last_kernel = sq ? "k_wfmrx_front_sq" : "k_wfmrx_front";
        if (p->where_held == csdr_amd_wfmrx::HELD_DEM) { const int rc = wfmrx_move_held(p, false); if (rc) return rc; }
        WfmrxArgs a;
        a.in = (const float2 *)in; a.in_pitch = in_pitch; a.n_in = (int)n_in; a.last = (const float2 *)p->d_last[p->lflip].get();
        a.carry = p->d_carry[p->cflip].get(); a.carry_pitch = p->W; a.held = held; a.n_ch = S;
        a.sq = sq ? *sq : FmrxSq{nullptr, nullptr, 0, 0, 1, 0};
        if (windows) {
            if (const int rc = fracdec_plan(c, fd, total)) return rc;
            if (fd->plan_outputs != n_out || fd->plan_processed != from) return fail_msg(-3, "wfmrx: internal: the plans disagree (%d / %d outputs, %d / %d samples)", fd->plan_outputs, n_out, fd->plan_processed, from);
            fracdec_commit(fd);
        }
        if (n_out > 0) {
            const dim3 grid(cdiv(n_out, p->tile_out), cdiv(S, WF_G));
#define WF_FRONT(PV, SQ) hipLaunchKernelGGL((k_wfmrx_front<PV, SQ>), grid, dim3(256), 0, st, a, (const int *)fd->d_lo.get(), (const float *)fd->d_frac.get(), n_out, p->tile_out, (const float *)fd->d_denom.get(), p->d_pre.get(), p->a_pitch)
#define WF_FRONTS(SQ) switch (p->P) { \
            case 2: WF_FRONT(2, SQ); break; case 4: WF_FRONT(4, SQ); break; case 6: WF_FRONT(6, SQ); break; case 8: WF_FRONT(8, SQ); break; \
            case 10: WF_FRONT(10, SQ); break; case 12: WF_FRONT(12, SQ); break; case 14: WF_FRONT(14, SQ); break; default: WF_FRONT(16, SQ); break; \
            }
            if (sq) { WF_FRONTS(true) } else { WF_FRONTS(false) }
#undef WF_FRONTS
#undef WF_FRONT
            CSDR_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_wfmrx_tail, dim3(cdiv(S, WT_CH)), dim3(256), 0, st, (const float *)p->d_pre.get(), p->a_pitch, S, n_out, p->alpha, p->d_state.get(), audio_s16, audio_f, out_pitch);
            CSDR_LAUNCH_CHECK();
        }
        // what the call keeps: into the other carry buffer behind a call with a window, appended in place behind one without
        float *keep = p->d_carry[from > 0 ? p->cflip ^ 1 : p->cflip].get();
        if (sq) hipLaunchKernelGGL(k_wfmrx_keep<true>, dim3(std::max(cdiv(rem, 256), 1u), S), dim3(256), 0, st, a, from, rem, keep, (float2 *)p->d_last[p->lflip ^ 1].get());
        else hipLaunchKernelGGL(k_wfmrx_keep<false>, dim3(std::max(cdiv(rem, 256), 1u), S), dim3(256), 0, st, a, from, rem, keep, (float2 *)p->d_last[p->lflip ^ 1].get());
        CSDR_LAUNCH_CHECK();
        if (from > 0) p->cflip ^= 1;
        p->lflip ^= 1;
        p->where_held = csdr_amd_wfmrx::HELD_CARRY;
    } else {
        p->last_kernel = "k_fracdec";
        if (p->where_held == csdr_amd_wfmrx::HELD_CARRY) { const int rc = wfmrx_move_held(p, true); if (rc) return rc; }
        float *dem = p->d_dem.get() + WF_PAD;
        int rc = csdr_amd_fmdemod_quadri_cf(c, in, dem + held, S, (size_t)n_in, in_pitch, p->d_pitch, p->d_last[p->lflip].get());
        if (rc) return rc;
        p->where_held = csdr_amd_wfmrx::HELD_DEM;
        if (windows) {
            int processed = 0;
            const int got = csdr_amd_fractional_decimator_ff(c, fd, dem, p->d_pre.get(), S, total, p->d_pitch, p->a_pitch, &processed);
            if (got < 0) return got;
            if (got != n_out || processed != from) return fail_msg(-3, "wfmrx: internal: the plans disagree (%d / %d outputs, %d / %d samples)", got, n_out, processed, from);
        }
        if (n_out > 0) {
            const size_t op = std::max(out_pitch, (size_t)n_out);       // (one channel: the row is as long as the caller says)
            rc = csdr_amd_deemphasis_wfm_ff(c, p->d_pre.get(), p->d_pre.get(), S, (size_t)n_out, p->a_pitch, p->a_pitch, p->tau, p->audio_rate, p->d_state.get());
            if (rc) return rc;
            if (audio_f) CSDR_HIP(hipMemcpy2DAsync(audio_f, sizeof(float) * op, p->d_pre.get(), sizeof(float) * p->a_pitch, sizeof(float) * n_out, S, hipMemcpyDeviceToDevice, st));
            if (audio_s16) {
                rc = csdr_amd_convert_f_s16(c, p->d_pre.get(), p->d_s16.get(), p->a_pitch * S);
                if (rc) return rc;
                CSDR_HIP(hipMemcpy2DAsync(audio_s16, sizeof(int16_t) * op, p->d_s16.get(), sizeof(int16_t) * p->a_pitch, sizeof(int16_t) * n_out, S, hipMemcpyDeviceToDevice, st));
            }
        }
        if (from > 0) {                                                 // the unprocessed tail: through the carry buffer, back in front at the next call
            if (rem) CSDR_HIP(hipMemcpy2DAsync(p->d_carry[p->cflip].get(), sizeof(float) * p->W, dem + from, sizeof(float) * p->d_pitch, sizeof(float) * rem, S, hipMemcpyDeviceToDevice, st));
            p->where_held = csdr_amd_wfmrx::HELD_CARRY;
        }
    }
    p->held = rem;
    return n_out;
}

long long csdr_amd_wfmrx_process(csdr_amd_wfmrx *p, const csdr_complexf *in, size_t in_pitch, long long n_in, int16_t *audio_s16, float *audio_f, size_t out_pitch)
{
    if (!p) return fail_msg(-3, "wfmrx: null object");
    if (p->sqB) return csdr_amd_wfmrx_process_squelched(p, in, in_pitch, n_in, audio_s16, audio_f, out_pitch, nullptr, 0, nullptr, nullptr);
    if (n_in < 0 || (size_t)n_in > p->max_n) return fail_msg(-3, "wfmrx: n_in should be 0 .. max_samples_per_call (%zu)", p->max_n);
    if (!n_in) return 0;
    if (!in || (in_pitch < (size_t)n_in && p->n_ch > 1)) return fail_msg(-3, "wfmrx: in_pitch below n_in");
    int n_out = 0, rem = 0;
    if (const int rc = wfmrx_plan_checked(p, n_in, out_pitch, &n_out, &rem)) return rc;
    return wfmrx_run(p, in, in_pitch, (int)n_in, n_out, rem, audio_s16, audio_f, out_pitch, wfmrx_fused_shape(p, in, in_pitch), nullptr);
}

// ---- the squelch in front
int csdr_amd_wfmrx_squelch_plan(int held, long long n_in, int block, long long *m, int *new_held)
{
    if (held < 0 || n_in < 0 || block < 1 || held >= block) return fail_msg(-3, "wfmrx: squelch_plan needs block >= 1, 0 <= held < block, n_in >= 0");
    const long long e = (held + n_in) / block * block;                 // whole blocks go on; the rest waits
    if (m) *m = e;
    if (new_held) *new_held = (int)(held + n_in - e);
    return 0;
}

static int wfmrx_squelched(const csdr_amd_wfmrx *p)
{
    if (!p) return fail_msg(-3, "wfmrx: null object");
    if (!p->sqB) return fail_msg(-3, "wfmrx: the object was created without a squelch (csdr_amd_wfmrx_create_squelched)");
    return 0;
}

int csdr_amd_wfmrx_set_squelch_level(csdr_amd_wfmrx *p, int ch, float level)
{
    if (const int rc = wfmrx_squelched(p)) return rc;
    if (ch < -1 || ch >= p->n_ch) return fail_msg(-3, "wfmrx: channel out of range");
    for (int k = (ch < 0 ? 0 : ch); k < (ch < 0 ? p->n_ch : ch + 1); k++) {
        p->lv[k] = level;
        if (p->sq_h == 0) p->lv_started[k] = level;                    // no block is under way: the next one starts under this level
    }
    p->lv_dirty = true;
    return 0;
}

int csdr_amd_wfmrx_get_squelch_level(const csdr_amd_wfmrx *p, int ch, float *level)
{
    if (const int rc = wfmrx_squelched(p)) return rc;
    if (ch < 0 || ch >= p->n_ch || !level) return fail_msg(-3, "wfmrx: channel out of range");
    *level = p->lv[ch];
    return 0;
}

int csdr_amd_wfmrx_squelch_held(const csdr_amd_wfmrx *p) { if (const int rc = wfmrx_squelched(p)) return rc; return p->sq_h; }
long long csdr_amd_wfmrx_squelch_block_index(const csdr_amd_wfmrx *p) { if (const int rc = wfmrx_squelched(p)) return rc; return p->sq_blk; }

long long csdr_amd_wfmrx_process_squelched(csdr_amd_wfmrx *p, const csdr_complexf *in, size_t in_pitch, long long n_in, int16_t *audio_s16, float *audio_f, size_t out_pitch,
                                           float *power, size_t power_pitch, uint8_t *open_flags, int *n_blocks)
{
    if (const int rc = wfmrx_squelched(p)) return rc;
    if (n_in < 0 || (size_t)n_in > p->max_n) return fail_msg(-3, "wfmrx: n_in should be 0 .. max_samples_per_call (%zu)", p->max_n);
    if (n_blocks) *n_blocks = 0;
    if (!n_in) return 0;
    if (!in || (in_pitch < (size_t)n_in && p->n_ch > 1)) return fail_msg(-3, "wfmrx: in_pitch below n_in");
    const int B = p->sqB, S = p->n_ch, h = p->sq_h;
    long long m64 = 0; int nh = 0;
    if (csdr_amd_wfmrx_squelch_plan(h, n_in, B, &m64, &nh) < 0) return -3;
    const int m = (int)m64, nbk = m / B;
    if ((power || open_flags) && (size_t)nbk > power_pitch) return fail_msg(-3, "wfmrx: power_pitch %zu below the %d squelch blocks of this call", power_pitch, nbk);
    int n_out = 0, rem = p->held;
    if (m > 0) if (const int rc = wfmrx_plan_checked(p, m, out_pitch, &n_out, &rem)) return rc;
    csdr_amd_ctx *c = p->c; hipStream_t st = c->stream;
    const size_t carry_bytes = sizeof(float2) * (size_t)B * S;
    const bool fused = wfmrx_fused_shape(p, in, in_pitch);
    if (fused) {
        if (p->lv_dirty) {
            float *hl = (float *)c->pinned_acquire(sizeof(float) * 2 * S); if (!hl) return -2;
            memcpy(hl, p->lv.data(), sizeof(float) * S); memcpy(hl + S, p->lv_started.data(), sizeof(float) * S);
            if (const int rc = c->pinned_upload(p->d_lv.get(), sizeof(float) * 2 * S)) return rc;
            p->lv_dirty = false;
        }
        if (p->sq_where == csdr_amd_wfmrx::SQ_OBJ && h > 0) CSDR_HIP(hipMemcpyAsync(p->d_sq_carry[p->sflip].get(), p->sq_obj_carry, carry_bytes, hipMemcpyDeviceToDevice, st));
        const FmrxSq q{p->d_sq_carry[p->sflip].get(), p->d_fl.get(), p->fl_pitch, h, B, (B & (B - 1)) ? -1 : __builtin_ctz(B)};
        if (nbk > 0) {
            hipLaunchKernelGGL(k_fmrx_power, dim3(cdiv((size_t)nbk * S, 4)), dim3(256), 0, st, (const float2 *)in, in_pitch, q, p->sqd, nbk, S, p->d_lv.get(), p->d_pw.get(),
                               p->d_fl.get(), power, open_flags, power_pitch);
            CSDR_LAUNCH_CHECK();
            const long long rc = wfmrx_run(p, in, in_pitch, m, n_out, rem, audio_s16, audio_f, out_pitch, true, &q);
            if (rc < 0) return rc;
        }
        if (nh > 0) {                                                  // what waits for the next call: appended in place behind a call without a block
            float2 *keep = p->d_sq_carry[nbk > 0 ? p->sflip ^ 1 : p->sflip].get();
            hipLaunchKernelGGL(k_fmrx_sq_carry, dim3(cdiv((size_t)std::min<long long>(n_in, B), 256), S), dim3(256), 0, st, (const float2 *)in, in_pitch, (int)n_in, keep, h, B, m);
            CSDR_LAUNCH_CHECK();
            if (nbk > 0) p->sflip ^= 1;
        }
        p->sq_where = csdr_amd_wfmrx::SQ_OWN;
        p->last_kernel = "k_wfmrx_front_sq";
    } else {
        if (p->sq_where == csdr_amd_wfmrx::SQ_OWN && h > 0) CSDR_HIP(hipMemcpyAsync(p->sq_obj_carry, p->d_sq_carry[p->sflip].get(), carry_bytes, hipMemcpyDeviceToDevice, st));
        (void)squelch_adopt(p->sq.get(), h, p->sq_blk, p->lv.data(), p->lv_started.data());
        const int got = csdr_amd_squelch_process(p->sq.get(), in, n_in, S > 1 ? in_pitch : std::max(in_pitch, (size_t)n_in), (csdr_complexf *)p->d_gated.get(), p->g_pitch, power,
                                                 power_pitch, open_flags, nullptr);
        if (got < 0) return got;
        if (got != nbk) return fail_msg(-4, "wfmrx: the squelch completed %d blocks where %d were planned", got, nbk);
        if (nbk > 0) {
            const long long rc = wfmrx_run(p, (const csdr_complexf *)p->d_gated.get(), p->g_pitch, m, n_out, rem, audio_s16, audio_f, out_pitch, false, nullptr);
            if (rc < 0) return rc;
        }
        p->sq_where = csdr_amd_wfmrx::SQ_OBJ;
        p->last_kernel = "k_fracdec";
    }
    p->sq_h = nh; p->sq_blk += nbk;
    // a block that is under way behind this call's whole blocks was started by this call: its level is the one in force now
    if (nbk > 0 && memcmp(p->lv_started.data(), p->lv.data(), sizeof(float) * S)) { p->lv_started = p->lv; p->lv_dirty = true; }
    if (n_blocks) *n_blocks = nbk;
    return n_out;
}

} // extern "C"
