// amssb.hip -- the AM and SSB receive chains for n_channels channels per call (MI355X / gfx950), README.md:95 and :110 of the reference:
//
//   AM    ... | amdemod_cf | fastdcblock_ff | agc_ff | limit_ff | convert_f_s16
//   SSB   ... | bandpass_fir_fft_cc lo hi tbw | realpart_cf | agc_ff | limit_ff | convert_f_s16
//
// The object is the demodulator and the audio tail (CF32 input: decimated complex baseband, as the channelizer or a front end leaves it), optionally behind an owned
// csdr_amd_ddc (U8 input: convert_u8_f | shift_addition_cc | fir_decimate_cc) and, in SSB, an owned csdr_amd_fftfilt.  The tail is serial within a channel (agc_ff
// is a state machine with a float recursion) and independent across channels; the parameters are shared, the state {last_dc, last_gain} is per channel and stays on
// the device between calls.  It works on whole blocks of B samples, fastdcblock_ff's buffer and agc_ff's call length: samples short of a block wait in the object.
//   k_amssb_tiled<MODE>     C channels per one-wave workgroup.  AM first takes each channel's block sum cooperatively (lane l the partial l, a five-step tree).
//                           Per tile of 64 samples all lanes stage each channel's row (one coalesced 512-byte load per channel, the next tile's loads already in
//                           flight), form the envelope, the DC ramp and reference / |x| and leave them in LDS; lane c walks channel c's AGC over the tile from LDS;
//                           all lanes scale, limit, convert and store the s16 rows (and the float pre-AGC rows, when asked for) coalesced.
//   k_amssb_generic<MODE>   one lane per channel, straight from and to global memory, float by float: any pointer alignment, any block size.  force_generic(1)
//                           takes it always.
// Both run amssb_dev.hpp's functions on the same samples in the same order: the same bits, for every C, every cut into calls and every pitch, as the CPU hook.
#include "bank.hpp"
#include "amssb_dev.hpp"
#include "squelch_dev.hpp"
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>

using namespace csdr_amd;

namespace {

static_assert(sizeof(AmSsbChan) == sizeof(csdr_amd_amssb_chan), "AmSsbChan mirrors csdr_amd_amssb_chan");

// The samples of a call are the object's carried ones (fill of them per channel, rows `block` samples apart) followed by the call's own.
struct AmSsbArgs {
    AmSsbCfg cfg; AmSsbChan *st; int n_ch, lanes;
    const float *carry; int fill;
    const float *in; size_t in_pitch;
    int n_blocks;
    int16_t *s16; float *pre; size_t out_pitch;
};
// the gate at the tail's input (csdr_amd_amssb_enable_squelch): flags[ch][blk] is 0 where block blk of the call is closed.  Read by the <.., true> instances only
// zeros: one tile of (0, 0) samples, what the tiled kernel reads in a closed channel's place
struct AmSsbSq { const uint8_t *flags; size_t fl_pitch; const float2 *zeros; };

__device__ __forceinline__ float2 sample_any(const AmSsbArgs &a, int ch, long long v)      // float by float: any alignment
{
    const float *p = v < a.fill ? a.carry + 2 * ((size_t)ch * a.cfg.block + v) : a.in + 2 * ((size_t)ch * a.in_pitch + (v - a.fill));
    return make_float2(p[0], p[1]);
}

// SQ: a closed block's samples are (0, 0).  Its envelope and mean are +0, so it is walked on the ramp from last_dc to 0 without a load; once last_dc is +-0
// (SSB: at once) every pre-AGC sample is +0, every s16 is 0 and the walk is amssb_agc_zero_run: a zero block
template <int MODE, bool SQ> __global__ __launch_bounds__(64) void k_amssb_generic(AmSsbArgs a, AmSsbSq q)
{
    if ((int)threadIdx.x >= a.lanes) return;
    const int ch = blockIdx.x * a.lanes + threadIdx.x;
    if (ch >= a.n_ch) return;
    AmSsbChan s = a.st[ch];
    const int B = a.cfg.block;
    for (int blk = 0; blk < a.n_blocks; blk++) {
        const long long base = (long long)blk * B;
        const size_t o = (size_t)ch * a.out_pitch + base;
        const bool open = !SQ || q.flags[(size_t)ch * q.fl_pitch + blk];
        if (SQ && !open && (MODE == AMSSB_SSB || s.last_dc == 0.f)) {
            for (int i = 0; i < B; i++) { a.s16[o + i] = 0; if (a.pre) a.pre[o + i] = 0.f; }
            s.last_gain = amssb_agc_zero_run(a.cfg, s.last_gain, B - 1);
            if (MODE == AMSSB_AM) s.last_dc = 0.f;
            continue;
        }
        float avg = 0.f;
        if (MODE == AMSSB_AM && open)
            avg = amssb_block_mean(amssb_block_sum(B, [&](int i) { const float2 v = sample_any(a, ch, base + i); return amssb_envelope(v.x, v.y); }), B);
        AgcCall g;
        for (int i = 0; i < B; i++) {
            const float2 v = open ? sample_any(a, ch, base + i) : make_float2(0.f, 0.f);
            const float x = MODE == AMSSB_AM ? amssb_dc_ramp(amssb_envelope(v.x, v.y), s.last_dc, avg, i, B) : v.x;
            const float gn = i == 0 ? agc_call_begin(a.cfg, g, s.last_gain) : agc_call_step(a.cfg, g, x, amssb_agc_ratio(a.cfg, x));
            a.s16[o + i] = amssb_finish(a.cfg, gn, x);
            if (a.pre) a.pre[o + i] = x;
        }
        s.last_gain = g.gain;
        if (MODE == AMSSB_AM) s.last_dc = avg;
    }
    a.st[ch] = s;
}

constexpr int AT = 64;                                   // samples per tile (= lanes per wave: one coalesced row per load)
constexpr int ATP = AT + 1;                              // odd row stride: the chain lanes' same-column accesses fall in different banks
constexpr int ACMAX = 64;                                // channels per workgroup at most (one sample per channel is held ahead in registers)
constexpr size_t tiled_lds(int C) { return (size_t)C * ATP * 2 * sizeof(float); }      // at most 33 280 bytes

// block % 64 == 0, 8-byte aligned input rows
// SQ: per block, bit cc of `open` is channel cc's flag, the same in every lane.  A closed channel is never loaded: its tile is (0, 0) in registers and its mean
// +0, and beside open channels it goes through the stages below like them (the lanes of a wave walk in lockstep: a lane that stood still would save nothing,
// and a zero run beside the walk would add to it).  A workgroup whose channels are all in zero blocks (k_amssb_generic) skips the mean pass, the tile loop and
// its barriers: the rows are stored as zeros and every lane takes the zero run.  The flags of the next block are fetched a block ahead, so that the prefetch
// across the block seam knows them.
template <int MODE, bool SQ> __global__ __launch_bounds__(64) void k_amssb_tiled(AmSsbArgs a, int C, AmSsbSq q)
{
    extern __shared__ float lds_f[];
    float *xr = lds_f, *rr = lds_f + (size_t)C * ATP;    // the pre-AGC samples; reference / |x|, then the gains
    const int lane = threadIdx.x, ch0 = blockIdx.x * C;
    const int nc = min(C, a.n_ch - ch0);
    const bool chain = lane < nc;
    const int B = a.cfg.block;
    const long long total = (long long)a.n_blocks * B;
    const float2 *carry = (const float2 *)a.carry, *in = (const float2 *)a.in;
    auto sample = [&](int cc, long long v) {
        return v < a.fill ? carry[(size_t)(ch0 + cc) * B + v] : in[(size_t)(ch0 + cc) * a.in_pitch + (v - a.fill)];
    };
    auto sample_at = [&](int cc, long long v) {
        return v < a.fill ? carry + (size_t)(ch0 + cc) * B + v : in + (size_t)(ch0 + cc) * a.in_pitch + (v - a.fill);
    };
    AmSsbChan s{0.f, 1.f};
    if (chain) s = a.st[ch0 + lane];
    const int me = lane * ATP;
    float my_avg = 0.f;
    AgcCall g{0.f, 0.f, 0.f, 0, 0};

    typedef unsigned long long mask_t;
    const mask_t live = nc >= 64 ? ~(mask_t)0 : (((mask_t)1 << nc) - 1);
    mask_t open = live, open_next = live;
    const bool wide16 = !(((uintptr_t)a.s16 | (a.out_pitch * 2)) & 15), wide32 = !(((uintptr_t)a.pre | (a.out_pitch * 4)) & 15);
    auto flags_of = [&](int blk) {
        bool f = false;
        if (chain && blk < a.n_blocks) f = q.flags[(size_t)(ch0 + lane) * q.fl_pitch + blk] != 0;
        return (mask_t)__ballot(f);
    };
    if (SQ) open_next = flags_of(0);

    float2 nx[ACMAX];                                    // the next tile, loaded while the chain lanes walk this one
    auto fetch = [&](long long b, mask_t m) {
#pragma unroll
        for (int cc = 0; cc < ACMAX; cc++)
            if (cc < nc) {                               // (whole tiles only: b + lane < total)
                if (!SQ) nx[cc] = sample(cc, b + lane);
                else nx[cc] = *(((m >> cc) & 1) ? sample_at(cc, b + lane) : q.zeros + lane);      // a closed channel: the zero tile, from cache, never its rows
            }
    };
    fetch(0, open_next);
    int blk = 0;
    for (long long base = 0; base < total; base += B, blk++) {
        bool skip = false;
        if (SQ) {
            open = open_next; open_next = flags_of(blk + 1);
            // every channel of the workgroup in a zero block: no tile, no barrier; the rows as 16-byte stores where they are aligned so (B is a multiple of 64)
            skip = open == 0 && (mask_t)__ballot(chain && (MODE == AMSSB_SSB || s.last_dc == 0.f)) == live;
            if (skip) {
                for (int cc = 0; cc < nc; cc++) {
                    const size_t o = (size_t)(ch0 + cc) * a.out_pitch + base;
                    if (wide16) for (int i = lane; i < B / 8; i += AT) reinterpret_cast<int4 *>(a.s16 + o)[i] = make_int4(0, 0, 0, 0);
                    else for (int i = lane; i < B; i += AT) a.s16[o + i] = 0;
                    if (a.pre) {
                        if (wide32) for (int i = lane; i < B / 4; i += AT) reinterpret_cast<float4 *>(a.pre + o)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                        else for (int i = lane; i < B; i += AT) a.pre[o + i] = 0.f;
                    }
                }
            }
        }
        if (MODE == AMSSB_AM && !(SQ && skip)) {                         // 0. the block's mean per channel: lane l sums the samples l, l + 64, ..., then the tree
            for (int cc = 0; cc < nc; cc++) {
                float avg = 0.f;                         // (a closed block's mean: +0 / B)
                if (!SQ || ((open >> cc) & 1)) {
                    float p = 0.f;
#pragma unroll 4
                    for (int i = lane; i < B; i += AT) { const float2 v = sample(cc, base + i); p = p + amssb_envelope(v.x, v.y); }
#pragma unroll
                    for (int w = 32; w > 0; w >>= 1) p = p + __shfl_down(p, w);
                    avg = amssb_block_mean(__shfl(p, 0), B);
                }
                if (lane == cc) my_avg = avg;
            }
        }
        for (int t0 = SQ && skip ? B - AT : 0; t0 < B; t0 += AT) {          // (a skipped block: the fetch across its end only)
#pragma unroll
            for (int cc = 0; cc < ACMAX; cc++) {         // 1. stage: lane j holds sample t0 + j of channel cc's block
                if (cc < nc && !(SQ && skip)) {
                    float x = nx[cc].x;
                    if (MODE == AMSSB_AM) x = amssb_dc_ramp(amssb_envelope(nx[cc].x, nx[cc].y), __shfl(s.last_dc, cc), __shfl(my_avg, cc), t0 + lane, B);
                    xr[cc * ATP + lane] = x;
                    rr[cc * ATP + lane] = amssb_agc_ratio(a.cfg, x);
                }
            }
            if (!(SQ && skip)) __syncthreads();
            if (base + t0 + AT < total) fetch(base + t0 + AT, t0 + AT < B ? open : open_next);
            if (SQ && skip) break;
            if (chain) {                                 // 2. lane c walks channel c
                for (int j0 = 0; j0 < AT; j0 += 8) {
                    float xv[8], rv[8];                  // 8 samples to registers first: the LDS latency stays off the chain
#pragma unroll
                    for (int j = 0; j < 8; j++) { xv[j] = xr[me + j0 + j]; rv[j] = rr[me + j0 + j]; }
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        float gn;
                        if (j == 0 && t0 + j0 == 0) gn = agc_call_begin(a.cfg, g, s.last_gain);      // (uniform) a call's first sample
                        else gn = agc_call_step(a.cfg, g, xv[j], rv[j]);
                        rr[me + j0 + j] = gn;
                    }
                }
            }
            __syncthreads();
            for (int cc = 0; cc < nc; cc++) {            // 3. write back: lane j finishes and stores sample t0 + j of every channel
                const size_t o = (size_t)(ch0 + cc) * a.out_pitch + base + t0 + lane;
                const float x = xr[cc * ATP + lane];
                a.s16[o] = amssb_finish(a.cfg, rr[cc * ATP + lane], x);
                if (a.pre) a.pre[o] = x;
            }
            __syncthreads();                             // (the rows are free for the next tile)
        }
        if (SQ && skip) {
            s.last_gain = amssb_agc_zero_run(a.cfg, s.last_gain, B - 1);
            if (MODE == AMSSB_AM) s.last_dc = 0.f;
        } else {
            s.last_gain = g.gain;
            if (MODE == AMSSB_AM) s.last_dc = my_avg;
        }
    }
    if (chain) a.st[ch0 + lane] = s;
}

// The power pass of a gated call: grid (ceil(n_blocks n_ch / 4)), 256 threads, one wave per (channel, block) over (carry ++ call) in squelch_dev.hpp's order: lane l
// takes the samples 128 r + 2 l, + 1 of the block's rows r of 128, chains 128 (r mod 4) + 2 l, + 1, each added to in increasing sample order.  -> the power
// and the open flag, to the object's rows (pitch fl_pitch) and to the caller's where given.  lv: n_ch levels of the blocks this call starts, then n_ch of the
// block begun earlier.  A8: 8-byte aligned input rows, a sample is one load (fmrx.hip's k_fmrx_power asks 16-byte rows of its caller and cannot serve here).
template <bool A8> __global__ __launch_bounds__(256) void k_amssb_power(AmSsbArgs a, int d, const float *__restrict__ lv, float *__restrict__ own_power,
                                                                        uint8_t *__restrict__ own_flags, size_t fl_pitch, float *__restrict__ power,
                                                                        uint8_t *__restrict__ flags, size_t power_pitch)
{
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (long long)a.n_ch * a.n_blocks) return;                    // (the whole wave)
    const int ch = (int)(w / a.n_blocks), k = (int)(w % a.n_blocks), B = a.cfg.block;
    const long long base = (long long)k * B;
    const float fB = (float)B;
    const float2 *carry = (const float2 *)a.carry, *in = (const float2 *)a.in;
    float acc[4][2] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
    for (int s0 = 0; s0 < B; s0 += 512) {
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const int s = s0 + 128 * r + 2 * lane + e;
                if (s < B && (d == 1 || s % d == 0)) {
                    const long long v = base + s;
                    float2 u;
                    if (A8) u = v < a.fill ? carry[(size_t)ch * B + v] : in[(size_t)ch * a.in_pitch + (v - a.fill)];
                    else u = sample_any(a, ch, v);
                    acc[r][e] = acc[r][e] + squelch_term_c(u.x, u.y, fB);
                }
            }
    }
    const float P = squelch_wave_tree(acc);
    const bool open = squelch_open(P, lv[(k == 0 && a.fill > 0 ? a.n_ch : 0) + ch]);
    if (lane == 0) {
        own_power[(size_t)ch * fl_pitch + k] = P; own_flags[(size_t)ch * fl_pitch + k] = open;
        if (power) power[(size_t)ch * power_pitch + k] = P;
        if (flags) flags[(size_t)ch * power_pitch + k] = open;
    }
}

// dst[ch][dst_off .. dst_off + count) = src[ch][src_off .. src_off + count), complex samples, float by float
__global__ __launch_bounds__(256) void k_amssb_copy(const float *__restrict__ src, size_t src_pitch, long long src_off, float *__restrict__ dst, size_t dst_pitch,
                                                    long long dst_off, long long count, int n_ch)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * count) return;
    for (int ch = blockIdx.y; ch < n_ch; ch += gridDim.y)
        dst[2 * ((size_t)ch * dst_pitch + dst_off) + i] = src[2 * ((size_t)ch * src_pitch + src_off) + i];
}
__global__ void k_amssb_reset(AmSsbChan *st, int n_ch)
{
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch < n_ch) st[ch] = AmSsbChan{0.f, 1.f};
}

// channels per wave when the caller leaves it open.  A wave's time is its walk plus the staging and write-back of its C rows per tile, which the walking wave
// issues itself, so fewer channels per wave is faster as long as every wave still finds a SIMD of its own: the smallest of 1, 4 and 16 that leaves at most one
// wave per SIMD, the carrier object's 16 beyond (measured at 256, 4096 and 16384 channels: DESIGN section 4o holds the sweeps)
int default_lanes(int n_ch, bool tiled)
{
    if (!tiled) return std::max(1, std::min(64, n_ch));
    const unsigned simds = 4u * (unsigned)current_device_cu_count();
    for (int C : {1, 4}) if (cdiv(n_ch, C) <= simds) return C;
    return 16;
}

int check_params(const csdr_amd_amssb_params *p, AmSsbCfg *c)
{
    if (!p) return fail_msg(-3, "amssb: null params");
    if (p->mode != AMSSB_AM && p->mode != AMSSB_SSB) return fail_msg(-3, "amssb: mode is 0 (AM) or 1 (SSB)");
    if (p->block < 2 || p->block > 16384) return fail_msg(-3, "amssb: need 2 <= block <= 16384");
    if (p->hang_time < 0 || p->attack_wait_time < 0) return fail_msg(-3, "amssb: hang_time and attack_wait_time are not negative");
    c->mode = p->mode; c->block = p->block; c->reference = p->reference; c->attack_rate = p->attack_rate; c->decay_rate = p->decay_rate; c->max_gain = p->max_gain;
    c->hang_time = p->hang_time; c->attack_wait_time = p->attack_wait_time; c->alpha = p->gain_filter_alpha; c->limit_max = p->limit_max;
    return 0;
}

// one channel's tail on the CPU: the kernels' walk
void walk_host(const AmSsbCfg &cfg, const cf32 *in, int n_blocks, AmSsbChan &s, int16_t *s16, float *pre)
{
    const int B = cfg.block;
    for (int blk = 0; blk < n_blocks; blk++) {
        const cf32 *x = in + (size_t)blk * B;
        const size_t o = (size_t)blk * B;
        float avg = 0.f;
        if (cfg.mode == AMSSB_AM) avg = amssb_block_mean(amssb_block_sum(B, [&](int i) { return amssb_envelope(x[i].i, x[i].q); }), B);
        AgcCall g;
        for (int i = 0; i < B; i++) {
            const float v = cfg.mode == AMSSB_AM ? amssb_dc_ramp(amssb_envelope(x[i].i, x[i].q), s.last_dc, avg, i, B) : x[i].i;
            const float gn = i == 0 ? agc_call_begin(cfg, g, s.last_gain) : agc_call_step(cfg, g, v, amssb_agc_ratio(cfg, v));
            if (s16) s16[o + i] = amssb_finish(cfg, gn, v);
            if (pre) pre[o + i] = v;
        }
        s.last_gain = g.gain;
        if (cfg.mode == AMSSB_AM) s.last_dc = avg;
    }
}

inline dim3 copy_grid(long long count, int n_ch) { return dim3(cdiv((size_t)(2 * count), 256), (unsigned)std::min(n_ch, 65535)); }

} // namespace

struct csdr_amd_amssb : ChanBank<AmSsbChan> {
    AmSsbCfg cfg;
    size_t max_in, max_tail;                             // most samples per call at the interface and in front of the tail
    DevBuf<float> d_carry; int fill = 0;                 // [n_ch][block] complex: the samples short of a whole block
    int inp = 0; DevBuf<float> d_fin, d_filt; size_t f_pitch = 0; int f_fill = 0;      // SSB: the filter's input (what is short of one input_size in front) and output
    int D = 1; DevBuf<float> d_y; size_t y_pitch = 0;    // U8: the front end's decimation and output
    Owned<csdr_amd_fftfilt, csdr_amd_fftfilt_destroy> filt; int taps_len;
    std::vector<float> band;                             // [n_ch][2]: the edges set_passband gave a channel last (NaN: none, or taps of the caller's own)
    Owned<csdr_amd_ddc, csdr_amd_ddc_destroy> ddc;
    // the gate at the tail's input (csdr_amd_amssb_enable_squelch; sq false: none).  Its block is cfg.block and its held samples are d_carry's
    bool fed = false;                                              // a sample has come in since the create or the last reset
    bool sq = false; int sqd = 1; long long sq_blk = 0;              // use_every_nth, blocks since the reset
    std::vector<float> lv, lv_started; bool lv_dirty = false;      // csdr_amd_squelch's levels: of the blocks a call starts, of the block begun earlier
    DevBuf<float2> d_zero;                                         // AT samples of (0, 0)
    DevBuf<float> d_lv, d_pw; DevBuf<uint8_t> d_fl; size_t fl_pitch = 0;      // [2][n_ch]; the powers and flags of a call's blocks, [n_ch][fl_pitch]
};
// what a gated call hands back besides the audio
struct SqOut { float *power; size_t power_pitch; uint8_t *flags; int *n_blocks; };

namespace {

csdr_amd_amssb *create_impl(csdr_amd_ctx *c, const csdr_amd_amssb_params *params, int n_channels, bool u8, const float *rates, bool per_channel, int decimation,
                            const float *ddc_taps, int ddc_taps_length, const csdr_complexf *taps, int taps_length, int fft_size, size_t max_samples_per_call)
{
    AmSsbCfg cfg;
    if (bank_create_check("amssb", c, n_channels) < 0 || check_params(params, &cfg) < 0) return nullptr;
    if (taps_length < 0 || (taps_length > 0 && (!taps || cfg.mode != AMSSB_SSB))) { fail_msg(-3, "amssb: taps belong to SSB mode"); return nullptr; }
    if (max_samples_per_call < 1 || max_samples_per_call > ((size_t)1 << 30)) { fail_msg(-3, "amssb: max_samples_per_call should be 1 .. 2^30"); return nullptr; }
    Owned<csdr_amd_amssb, csdr_amd_amssb_destroy> p(new csdr_amd_amssb());
    p->c = c; p->cfg = cfg; p->n_ch = n_channels;
    p->max_in = max_samples_per_call; p->max_tail = max_samples_per_call;
    hipError_t e = hipSuccess;
    auto alloc = [&](auto &b, size_t bytes) { if (e == hipSuccess) e = dev_alloc(b, bytes); };
    if (u8) {
        if (max_samples_per_call < 1024) p->max_in = max_samples_per_call = 1024;
        p->ddc.reset(per_channel ? csdr_amd_ddc_create_rates(c, n_channels, rates, decimation, ddc_taps, ddc_taps_length, max_samples_per_call)
                                 : csdr_amd_ddc_create(c, n_channels, rates[0], decimation, ddc_taps, ddc_taps_length, max_samples_per_call));
        if (!p->ddc) return nullptr;
        p->D = decimation;
        p->max_tail = max_samples_per_call / decimation + 2;
        p->y_pitch = (p->max_tail + 15) & ~(size_t)15;
        alloc(p->d_y, sizeof(cf32) * p->y_pitch * n_channels);
    }
    if (taps_length > 0) {
        if (fft_size < 4 || (fft_size & (fft_size - 1)) || taps_length > fft_size) { fail_msg(-3, "amssb: need a power-of-two fft_size >= taps_length"); return nullptr; }
        p->inp = fft_size - taps_length + 1;
        p->f_pitch = (p->inp + p->max_tail + 15) & ~(size_t)15;
        p->filt.reset(csdr_amd_fftfilt_create(c, fft_size, taps, taps_length, n_channels, (int)(p->f_pitch / p->inp) + 1));
        if (!p->filt) return nullptr;
        p->taps_len = taps_length; p->band.assign((size_t)2 * n_channels, NAN);
        alloc(p->d_fin, sizeof(cf32) * p->f_pitch * n_channels);
        alloc(p->d_filt, sizeof(cf32) * p->f_pitch * n_channels);
        p->max_tail = p->f_pitch;
    }
    alloc(p->d_st, sizeof(AmSsbChan) * n_channels);
    alloc(p->d_carry, sizeof(cf32) * (size_t)cfg.block * n_channels);
    if (e != hipSuccess) { fail_msg(-2, "amssb: out of device memory"); return nullptr; }
    if (csdr_amd_amssb_reset(p.get()) < 0) return nullptr;
    return p.release();
}

// the filter in front of the SSB tail: n new samples per channel at x -> the whole filter blocks that became available, at *y
long long run_filter(csdr_amd_amssb *p, const float *x, size_t xp, long long n, const float **y, size_t *yp)
{
    hipStream_t st = p->c->stream;
    if (n > 0) {
        hipLaunchKernelGGL(k_amssb_copy, copy_grid(n, p->n_ch), dim3(256), 0, st, x, xp, 0LL, p->d_fin.get(), p->f_pitch, (long long)p->f_fill, n, p->n_ch);
        CSDR_LAUNCH_CHECK();
    }
    const long long total = p->f_fill + n;
    const int nb = (int)(total / p->inp);
    *y = p->d_filt.get(); *yp = p->f_pitch;
    if (!nb) { p->f_fill = (int)total; return 0; }
    const int rc = csdr_amd_fftfilt_process(p->filt.get(), (const csdr_complexf *)p->d_fin.get(), (csdr_complexf *)p->d_filt.get(), nb, p->f_pitch, p->f_pitch);
    if (rc < 0) return rc;
    const long long used = (long long)nb * p->inp, rem = total - used;      // rem < input_size <= used: the ranges do not overlap
    if (rem > 0) {
        hipLaunchKernelGGL(k_amssb_copy, copy_grid(rem, p->n_ch), dim3(256), 0, st, p->d_fin.get(), p->f_pitch, used, p->d_fin.get(), p->f_pitch, 0LL, rem, p->n_ch);
        CSDR_LAUNCH_CHECK();
    }
    p->f_fill = (int)rem;
    return used;
}

// the tail: n new complex samples per channel at x -> the whole blocks that became available
long long run_tail(csdr_amd_amssb *p, const float *x, size_t xp, long long n, int16_t *s16, float *pre, size_t out_pitch, const SqOut *so)
{
    hipStream_t st = p->c->stream;
    const int B = p->cfg.block;
    const long long total = p->fill + n;
    const long long nb = total / B, rem = total - nb * B;
    if (nb > 0) {
        if (!s16 || out_pitch < (size_t)(nb * B)) return fail_msg(-3, "amssb: need audio_s16 and out_pitch >= the %lld samples of this call", nb * B);
        AmSsbArgs a;
        a.cfg = p->cfg; a.st = p->d_st.get(); a.n_ch = p->n_ch;
        a.carry = p->d_carry.get(); a.fill = p->fill; a.in = x; a.in_pitch = xp; a.n_blocks = (int)nb;
        a.s16 = s16; a.pre = pre; a.out_pitch = out_pitch;
        const bool am = p->cfg.mode == AMSSB_AM, a8 = !((uintptr_t)x & 7);
        const AmSsbSq q{p->d_fl.get(), p->fl_pitch, p->d_zero.get()};
        if (p->sq) {                                     // the power pass: every block's power and flag, in front of the kernel that reads the flags
            if ((size_t)nb > p->fl_pitch) return fail_msg(-4, "amssb: %lld blocks in a call where %zu were planned", nb, p->fl_pitch);
            if (p->lv_dirty) {
                const size_t S = (size_t)p->n_ch;
                float *hl = (float *)p->c->pinned_acquire(sizeof(float) * 2 * S); if (!hl) return -2;
                memcpy(hl, p->lv.data(), sizeof(float) * S); memcpy(hl + S, p->lv_started.data(), sizeof(float) * S);
                if (const int rc = p->c->pinned_upload(p->d_lv.get(), sizeof(float) * 2 * S)) return rc;
                p->lv_dirty = false;
            }
            const dim3 pg(cdiv((size_t)nb * p->n_ch, 4));
            if (a8) hipLaunchKernelGGL(k_amssb_power<true>, pg, dim3(256), 0, st, a, p->sqd, p->d_lv.get(), p->d_pw.get(), p->d_fl.get(), p->fl_pitch, so ? so->power : nullptr,
                                       so ? so->flags : nullptr, so ? so->power_pitch : 0);
            else hipLaunchKernelGGL(k_amssb_power<false>, pg, dim3(256), 0, st, a, p->sqd, p->d_lv.get(), p->d_pw.get(), p->d_fl.get(), p->fl_pitch, so ? so->power : nullptr,
                                    so ? so->flags : nullptr, so ? so->power_pitch : 0);
            CSDR_LAUNCH_CHECK();
        }
        if (!p->force_generic && B % AT == 0 && a8) {
            static const char *const names[2][2] = {{"k_amssb_tiled<AM>", "k_amssb_tiled<SSB>"}, {"k_amssb_tiled_sq<AM>", "k_amssb_tiled_sq<SSB>"}};
            const int C = a.lanes = bank_launch_lanes(p, names[p->sq][!am], default_lanes(p->n_ch, true), ACMAX);
            const dim3 grid(cdiv(p->n_ch, C));
            if (!p->sq) {
                if (am) hipLaunchKernelGGL((k_amssb_tiled<AMSSB_AM, false>), grid, dim3(64), tiled_lds(C), st, a, C, q);
                else hipLaunchKernelGGL((k_amssb_tiled<AMSSB_SSB, false>), grid, dim3(64), tiled_lds(C), st, a, C, q);
            } else {
                if (am) hipLaunchKernelGGL((k_amssb_tiled<AMSSB_AM, true>), grid, dim3(64), tiled_lds(C), st, a, C, q);
                else hipLaunchKernelGGL((k_amssb_tiled<AMSSB_SSB, true>), grid, dim3(64), tiled_lds(C), st, a, C, q);
            }
        } else {
            static const char *const names[2][2] = {{"k_amssb_generic<AM>", "k_amssb_generic<SSB>"}, {"k_amssb_generic_sq<AM>", "k_amssb_generic_sq<SSB>"}};
            a.lanes = bank_launch_lanes(p, names[p->sq][!am], default_lanes(p->n_ch, false));
            const dim3 grid(cdiv(p->n_ch, a.lanes));
            if (!p->sq) {
                if (am) hipLaunchKernelGGL((k_amssb_generic<AMSSB_AM, false>), grid, dim3(64), 0, st, a, q);
                else hipLaunchKernelGGL((k_amssb_generic<AMSSB_SSB, false>), grid, dim3(64), 0, st, a, q);
            } else {
                if (am) hipLaunchKernelGGL((k_amssb_generic<AMSSB_AM, true>), grid, dim3(64), 0, st, a, q);
                else hipLaunchKernelGGL((k_amssb_generic<AMSSB_SSB, true>), grid, dim3(64), 0, st, a, q);
            }
        }
        CSDR_LAUNCH_CHECK();
    }
    // what is short of a block waits in front of the next call's samples.  After a call that wrote blocks it lies in the call's own samples (rem < B <= nb B)
    const long long keep = nb > 0 ? rem : n, from = nb > 0 ? n - rem : 0, to = nb > 0 ? 0 : p->fill;
    if (keep > 0) {
        hipLaunchKernelGGL(k_amssb_copy, copy_grid(keep, p->n_ch), dim3(256), 0, st, x, xp, from, p->d_carry.get(), (size_t)B, to, keep, p->n_ch);
        CSDR_LAUNCH_CHECK();
    }
    p->fill = (int)rem;
    if (p->sq) {
        p->sq_blk += nb;
        // a block that is under way behind this call's whole blocks was started by this call: its level is the one in force now
        if (nb > 0 && memcmp(p->lv_started.data(), p->lv.data(), sizeof(float) * p->n_ch)) { p->lv_started = p->lv; p->lv_dirty = true; }
        if (so && so->n_blocks) *so->n_blocks = (int)nb;
    }
    return nb * B;
}

// the most blocks a call of n_in samples can complete: exact without a front end, whose output count is known only behind it (there: max_out's bound)
long long blocks_bound(const csdr_amd_amssb *p, long long n_in)
{
    if (p->ddc) return csdr_amd_amssb_max_out(p, n_in) / p->cfg.block;
    long long n = n_in;
    if (p->filt) n = (p->f_fill + n) / p->inp * p->inp;
    return (p->fill + n) / p->cfg.block;
}

int squelched(const csdr_amd_amssb *p)
{
    if (!p) return fail_msg(-3, "amssb: null object");
    if (!p->sq) return fail_msg(-3, "amssb: the object has no squelch (csdr_amd_amssb_enable_squelch)");
    return 0;
}

long long process_impl(csdr_amd_amssb *p, const void *in, size_t in_pitch, long long n_in, int16_t *audio_s16, float *pre_agc_f, size_t out_pitch, const SqOut *so)
{
    if (n_in < 0 || (size_t)n_in > p->max_in) return fail_msg(-3, "amssb: n_in should be 0 .. the max_samples_per_call given to create (%zu)", p->max_in);
    if (n_in > 0 && (!in || in_pitch < (size_t)n_in)) return fail_msg(-3, "amssb: need in and in_pitch >= n_in");
    if (so && (so->power || so->flags) && (long long)so->power_pitch < blocks_bound(p, n_in))
        return fail_msg(-3, "amssb: power_pitch %zu below the %lld blocks this call may complete", so->power_pitch, blocks_bound(p, n_in));
    if (so && so->n_blocks) *so->n_blocks = 0;
    if (n_in > 0) p->fed = true;
    const float *x = (const float *)in; size_t xp = in_pitch; long long n = n_in;
    if (p->ddc) {
        if (n_in > 0) {
            n = csdr_amd_ddc_process(p->ddc.get(), (const uint8_t *)in, in_pitch, (size_t)n_in, (csdr_complexf *)p->d_y.get(), p->y_pitch);
            if (n < 0) return n;
            if ((size_t)n > p->y_pitch) return fail_msg(-3, "amssb: the front end produced more than the planned %zu samples", p->y_pitch);
        }
        x = p->d_y.get(); xp = p->y_pitch;
    } else if (n_in > 0 && ((uintptr_t)in & 3)) return fail_msg(-3, "amssb: in should be 4-byte aligned");
    if (p->filt) {
        n = run_filter(p, x, xp, n, &x, &xp);
        if (n < 0) return n;
    }
    return run_tail(p, x, xp, n, audio_s16, pre_agc_f, out_pitch, so);
}

} // namespace

extern "C" {

int csdr_amd_amssb_params_default(csdr_amd_amssb_params *p, int mode)
{
    if (!p) return fail_msg(-3, "amssb_params_default: null params");
    if (mode != AMSSB_AM && mode != AMSSB_SSB) return fail_msg(-3, "amssb: mode is 0 (AM) or 1 (SSB)");
    memset(p, 0, sizeof *p);
    p->mode = mode; p->block = 1024;
    p->hang_time = 200; p->reference = 0.2; p->attack_rate = 0.01; p->decay_rate = 0.0001; p->max_gain = 65536;      // csdr.c:1342-1361
    p->attack_wait_time = 0; p->gain_filter_alpha = 0.999;
    p->limit_max = 1.0;                                                                                             // csdr.c: limit_ff's default
    return 0;
}

csdr_amd_amssb *csdr_amd_amssb_create_cf32(csdr_amd_ctx *c, const csdr_amd_amssb_params *params, int n_channels, const csdr_complexf *taps, int taps_length,
                                           int fft_size, size_t max_samples_per_call)
{
    return create_impl(c, params, n_channels, false, nullptr, false, 0, nullptr, 0, taps, taps_length, fft_size, max_samples_per_call);
}

csdr_amd_amssb *csdr_amd_amssb_create(csdr_amd_ctx *c, const csdr_amd_amssb_params *params, int n_channels, float shift_rate, int decimation, const float *ddc_taps,
                                      int ddc_taps_length, const csdr_complexf *taps, int taps_length, int fft_size, size_t max_samples_per_call)
{
    return create_impl(c, params, n_channels, true, &shift_rate, false, decimation, ddc_taps, ddc_taps_length, taps, taps_length, fft_size, max_samples_per_call);
}

csdr_amd_amssb *csdr_amd_amssb_create_rates(csdr_amd_ctx *c, const csdr_amd_amssb_params *params, int n_channels, const float *shift_rates, int decimation,
                                            const float *ddc_taps, int ddc_taps_length, const csdr_complexf *taps, int taps_length, int fft_size,
                                            size_t max_samples_per_call)
{
    if (!shift_rates) { fail_msg(-3, "amssb_create_rates: no rates"); return nullptr; }
    return create_impl(c, params, n_channels, true, shift_rates, true, decimation, ddc_taps, ddc_taps_length, taps, taps_length, fft_size, max_samples_per_call);
}

int csdr_amd_amssb_set_rate(csdr_amd_amssb *p, int channel, float shift_rate)
{
    if (!p || !p->ddc) return fail_msg(-3, "amssb: set_rate needs an object with U8 input");
    return csdr_amd_ddc_set_rate(p->ddc.get(), channel, shift_rate);
}
float csdr_amd_amssb_get_rate(const csdr_amd_amssb *p, int channel) { return p && p->ddc ? csdr_amd_ddc_get_rate(p->ddc.get(), channel) : 0.f; }
csdr_amd_ddc *csdr_amd_amssb_front_end(csdr_amd_amssb *p) { return p ? p->ddc.get() : nullptr; }

// A channel's passband.  The owned filter takes it from its next call on, that is from the first sample it has not consumed: what waits in d_fin (short of one
// input_size) is filtered with the new taps already.
static int passband_target(const csdr_amd_amssb *p, int channel)
{
    if (!p) return fail_msg(-3, "amssb: null object");
    if (!p->filt) return fail_msg(-3, "amssb: a passband needs an SSB object with a filter (AM has none)");
    if (channel < 0 || channel >= p->n_ch) return fail_msg(-3, "amssb: channel out of range");
    return 0;
}
int csdr_amd_amssb_set_channel_taps(csdr_amd_amssb *p, int channel, const csdr_complexf *taps, int taps_length)
{
    if (const int rc = passband_target(p, channel)) return rc;
    if (!taps || taps_length != p->taps_len) return fail_msg(-3, "amssb: a channel's taps have the object's length (%d)", p->taps_len);
    const int rc = csdr_amd_fftfilt_set_stream_taps(p->filt.get(), channel, taps, taps_length);
    if (rc < 0) return rc;
    p->band[2 * (size_t)channel] = p->band[2 * (size_t)channel + 1] = NAN;
    return 0;
}
int csdr_amd_amssb_set_passband(csdr_amd_amssb *p, int channel, float low, float high, int window)
{
    if (const int rc = passband_target(p, channel)) return rc;
    if (!(low < high) || low < -0.5f || high > 0.5f) return fail_msg(-3, "amssb: need -0.5 <= low < high <= 0.5");
    if (window < CSDR_WINDOW_BOXCAR || window > CSDR_WINDOW_HAMMING) return fail_msg(-3, "amssb: unknown window");
    std::vector<csdr_complexf> taps((size_t)p->taps_len);
    csdr_amd_firdes_bandpass_c(taps.data(), p->taps_len, low, high, window);
    const int rc = csdr_amd_fftfilt_set_stream_taps(p->filt.get(), channel, taps.data(), p->taps_len);
    if (rc < 0) return rc;
    p->band[2 * (size_t)channel] = low; p->band[2 * (size_t)channel + 1] = high;
    return 0;
}
int csdr_amd_amssb_get_passband(const csdr_amd_amssb *p, int channel, float *low, float *high)
{
    if (const int rc = passband_target(p, channel)) return rc;
    if (low) *low = p->band[2 * (size_t)channel];
    if (high) *high = p->band[2 * (size_t)channel + 1];
    return 0;
}

// every channel back to last_dc = 0, last_gain = 1 (csdr.c:957, 1365), nothing waiting, the filter's overlap and the front end as created
int csdr_amd_amssb_reset(csdr_amd_amssb *p)
{
    if (!p) return fail_msg(-3, "amssb: null object");
    hipLaunchKernelGGL(k_amssb_reset, dim3(cdiv(p->n_ch, 256)), dim3(256), 0, p->c->stream, p->d_st.get(), p->n_ch);
    CSDR_LAUNCH_CHECK();
    p->fill = 0; p->f_fill = 0;
    p->fed = false; p->sq_blk = 0; p->lv_started = p->lv; p->lv_dirty = true;       // (the levels stay)
    if (p->filt && csdr_amd_fftfilt_reset(p->filt.get()) < 0) return -5;
    if (p->ddc && csdr_amd_ddc_reset(p->ddc.get()) < 0) return -5;
    return 0;
}

// one channel's two state words back to their start; its samples short of a block stay
int csdr_amd_amssb_reset_channel(csdr_amd_amssb *p, int ch) { return bank_reset_channel(p, "amssb", ch, AmSsbChan{0.f, 1.f}); }
int csdr_amd_amssb_get_channel(csdr_amd_amssb *p, int ch, csdr_amd_amssb_chan *out) { return bank_get_channel(p, "amssb", ch, out); }
int csdr_amd_amssb_set_channel(csdr_amd_amssb *p, int ch, const csdr_amd_amssb_chan *s) { return bank_set_channel(p, "amssb", ch, s, [] { return 0; }); }

int csdr_amd_amssb_set_lanes(csdr_amd_amssb *p, int lanes) { return bank_set_lanes(p, "amssb", lanes); }
int csdr_amd_amssb_lanes(const csdr_amd_amssb *p)
{
    if (!p) return 0;
    return p->force_generic ? bank_lanes(p, default_lanes(p->n_ch, false)) : bank_lanes(p, default_lanes(p->n_ch, true), ACMAX);
}

int csdr_amd_amssb_force_generic(csdr_amd_amssb *p, int on) { return bank_force_generic(p, "amssb", on); }
const char *csdr_amd_amssb_kernel_name(const csdr_amd_amssb *p) { return bank_kernel_name(p); }

void csdr_amd_amssb_destroy(csdr_amd_amssb *p) { destroy_on_stream(p); }

// the most audio samples per channel that a call of n_in input samples can write
long long csdr_amd_amssb_max_out(const csdr_amd_amssb *p, long long n_in)
{
    if (!p || n_in < 0) return 0;
    long long n = n_in;
    if (p->ddc) n = n / p->D + 2;
    if (p->filt) n = (p->inp - 1 + n) / p->inp * p->inp;
    return (p->cfg.block - 1 + n) / p->cfg.block * p->cfg.block;
}

long long csdr_amd_amssb_process(csdr_amd_amssb *p, const void *in, size_t in_pitch, long long n_in, int16_t *audio_s16, float *pre_agc_f, size_t out_pitch)
{
    if (!p) return fail_msg(-3, "amssb: null object");
    return process_impl(p, in, in_pitch, n_in, audio_s16, pre_agc_f, out_pitch, nullptr);
}

// ---- the gate at the tail's input
int csdr_amd_amssb_enable_squelch(csdr_amd_amssb *p, int use_every_nth, const float *levels)
{
    if (!p) return fail_msg(-3, "amssb: null object");
    if (use_every_nth < 1) return fail_msg(-3, "amssb: use_every_nth should be at least 1");
    if (p->fed)
        return fail_msg(-3, "amssb: enable_squelch needs an object that holds no sample (fresh, or after reset)");
    // a closed block's audio is g * 0 behind limit_ff: 0 for every g only where limit_max is not negative (and not NaN)
    if (!(p->cfg.limit_max >= 0)) return fail_msg(-3, "amssb: a squelch needs limit_max >= 0");
    const size_t S = (size_t)p->n_ch, fl_pitch = p->max_tail / p->cfg.block + 2;
    DevBuf<float> lv, pw; DevBuf<uint8_t> fl; DevBuf<float2> zero;
    if (dev_alloc(zero, sizeof(float2) * AT) != hipSuccess || dev_alloc(lv, sizeof(float) * 2 * S) != hipSuccess || dev_alloc(pw, sizeof(float) * fl_pitch * S) != hipSuccess || dev_alloc(fl, fl_pitch * S) != hipSuccess)
        return fail_msg(-2, "amssb: out of device memory");
    CSDR_HIP(hipMemsetAsync(zero.get(), 0, sizeof(float2) * AT, p->c->stream));
    p->d_zero = std::move(zero); p->d_lv = std::move(lv); p->d_pw = std::move(pw); p->d_fl = std::move(fl); p->fl_pitch = fl_pitch;
    p->lv.assign(S, 0.f);
    if (levels) p->lv.assign(levels, levels + S);
    p->lv_started = p->lv; p->lv_dirty = true;
    p->sq = true; p->sqd = use_every_nth; p->sq_blk = 0;
    return 0;
}

int csdr_amd_amssb_set_squelch_level(csdr_amd_amssb *p, int ch, float level)
{
    if (const int rc = squelched(p)) return rc;
    if (ch < -1 || ch >= p->n_ch) return fail_msg(-3, "amssb: channel out of range");
    for (int k = (ch < 0 ? 0 : ch); k < (ch < 0 ? p->n_ch : ch + 1); k++) {
        p->lv[k] = level;
        if (p->fill == 0) p->lv_started[k] = level;                    // no block is under way: the next one starts under this level
    }
    p->lv_dirty = true;
    return 0;
}

int csdr_amd_amssb_get_squelch_level(const csdr_amd_amssb *p, int ch, float *level)
{
    if (const int rc = squelched(p)) return rc;
    if (ch < 0 || ch >= p->n_ch || !level) return fail_msg(-3, "amssb: channel out of range");
    *level = p->lv[ch];
    return 0;
}

long long csdr_amd_amssb_squelch_block_index(const csdr_amd_amssb *p) { if (const int rc = squelched(p)) return rc; return p->sq_blk; }

long long csdr_amd_amssb_process_squelched(csdr_amd_amssb *p, const void *in, size_t in_pitch, long long n_in, int16_t *audio_s16, float *pre_agc_f, size_t out_pitch,
                                           float *power, size_t power_pitch, uint8_t *open_flags, int *n_blocks_out)
{
    if (const int rc = squelched(p)) return rc;
    const SqOut so{power, power_pitch, open_flags, n_blocks_out};
    return process_impl(p, in, in_pitch, n_in, audio_s16, pre_agc_f, out_pitch, &so);
}

// amssb_agc_zero_run on the host, the source the kernels run: the gain after n agc_ff steps on zero samples, and how many of them were taken one by one
float csdr_amd_debug_amssb_zero_run(const csdr_amd_amssb_params *params, float gain, long long n, long long *steps_iterated)
{
    AmSsbCfg cfg;
    if (check_params(params, &cfg) < 0 || n < 0) { fail_msg(-3, "debug_amssb_zero_run: bad arguments"); return NAN; }
    return amssb_agc_zero_run(cfg, gain, n, steps_iterated);
}

// CPU run of the kernels' functions for one channel (params->mode says which chain): in holds n_blocks * params->block complex samples; state_io (may be NULL: a
// fresh channel) carries {last_dc, last_gain} in and out; either output may be NULL.  Returns the samples written, n_blocks * block.
long long csdr_amd_debug_amssb_walk(const csdr_amd_amssb_params *params, const csdr_complexf *in, int n_blocks, csdr_amd_amssb_chan *state_io, int16_t *s16_out,
                                    float *pre_agc_out)
{
    AmSsbCfg cfg;
    if (check_params(params, &cfg) < 0) return -3;
    if (n_blocks < 0 || (n_blocks > 0 && !in)) return fail_msg(-3, "debug_amssb_walk: bad arguments");
    AmSsbChan s{0.f, 1.f};
    if (state_io) memcpy(&s, state_io, sizeof s);
    walk_host(cfg, in, n_blocks, s, s16_out, pre_agc_out);
    if (state_io) memcpy(state_io, &s, sizeof s);
    return (long long)n_blocks * cfg.block;
}

} // extern "C"
