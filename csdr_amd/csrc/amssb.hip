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

__device__ __forceinline__ float2 sample_any(const AmSsbArgs &a, int ch, long long v)      // float by float: any alignment
{
    const float *p = v < a.fill ? a.carry + 2 * ((size_t)ch * a.cfg.block + v) : a.in + 2 * ((size_t)ch * a.in_pitch + (v - a.fill));
    return make_float2(p[0], p[1]);
}

template <int MODE> __global__ __launch_bounds__(64) void k_amssb_generic(AmSsbArgs a)
{
    if ((int)threadIdx.x >= a.lanes) return;
    const int ch = blockIdx.x * a.lanes + threadIdx.x;
    if (ch >= a.n_ch) return;
    AmSsbChan s = a.st[ch];
    const int B = a.cfg.block;
    for (int blk = 0; blk < a.n_blocks; blk++) {
        const long long base = (long long)blk * B;
        float avg = 0.f;
        if (MODE == AMSSB_AM)
            avg = amssb_block_mean(amssb_block_sum(B, [&](int i) { const float2 v = sample_any(a, ch, base + i); return amssb_envelope(v.x, v.y); }), B);
        AgcCall g;
        const size_t o = (size_t)ch * a.out_pitch + base;
        for (int i = 0; i < B; i++) {
            const float2 v = sample_any(a, ch, base + i);
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
template <int MODE> __global__ __launch_bounds__(64) void k_amssb_tiled(AmSsbArgs a, int C)
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
    AmSsbChan s{0.f, 1.f};
    if (chain) s = a.st[ch0 + lane];
    const int me = lane * ATP;
    float my_avg = 0.f;
    AgcCall g{0.f, 0.f, 0.f, 0, 0};

    float2 nx[ACMAX];                                    // the next tile, loaded while the chain lanes walk this one
    auto fetch = [&](long long b) {
#pragma unroll
        for (int cc = 0; cc < ACMAX; cc++)
            if (cc < nc) nx[cc] = sample(cc, b + lane);  // (whole tiles only: b + lane < total)
    };
    fetch(0);
    for (long long base = 0; base < total; base += B) {
        if (MODE == AMSSB_AM) {                          // 0. the block's mean per channel: lane l sums the samples l, l + 64, ..., then the tree
            for (int cc = 0; cc < nc; cc++) {
                float p = 0.f;
#pragma unroll 4
                for (int i = lane; i < B; i += AT) { const float2 v = sample(cc, base + i); p = p + amssb_envelope(v.x, v.y); }
#pragma unroll
                for (int w = 32; w > 0; w >>= 1) p = p + __shfl_down(p, w);
                const float avg = amssb_block_mean(__shfl(p, 0), B);
                if (lane == cc) my_avg = avg;
            }
        }
        for (int t0 = 0; t0 < B; t0 += AT) {
#pragma unroll
            for (int cc = 0; cc < ACMAX; cc++) {         // 1. stage: lane j holds sample t0 + j of channel cc's block
                if (cc < nc) {
                    float x = nx[cc].x;
                    if (MODE == AMSSB_AM) x = amssb_dc_ramp(amssb_envelope(nx[cc].x, nx[cc].y), __shfl(s.last_dc, cc), __shfl(my_avg, cc), t0 + lane, B);
                    xr[cc * ATP + lane] = x;
                    rr[cc * ATP + lane] = amssb_agc_ratio(a.cfg, x);
                }
            }
            __syncthreads();
            if (base + t0 + AT < total) fetch(base + t0 + AT);
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
        s.last_gain = g.gain;
        if (MODE == AMSSB_AM) s.last_dc = my_avg;
    }
    if (chain) a.st[ch0 + lane] = s;
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
};

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
long long run_tail(csdr_amd_amssb *p, const float *x, size_t xp, long long n, int16_t *s16, float *pre, size_t out_pitch)
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
        const bool am = p->cfg.mode == AMSSB_AM;
        if (!p->force_generic && B % AT == 0 && !((uintptr_t)x & 7)) {
            const int C = a.lanes = bank_launch_lanes(p, am ? "k_amssb_tiled<AM>" : "k_amssb_tiled<SSB>", default_lanes(p->n_ch, true), ACMAX);
            if (am) hipLaunchKernelGGL(k_amssb_tiled<AMSSB_AM>, dim3(cdiv(p->n_ch, C)), dim3(64), tiled_lds(C), st, a, C);
            else hipLaunchKernelGGL(k_amssb_tiled<AMSSB_SSB>, dim3(cdiv(p->n_ch, C)), dim3(64), tiled_lds(C), st, a, C);
        } else {
            a.lanes = bank_launch_lanes(p, am ? "k_amssb_generic<AM>" : "k_amssb_generic<SSB>", default_lanes(p->n_ch, false));
            if (am) hipLaunchKernelGGL(k_amssb_generic<AMSSB_AM>, dim3(cdiv(p->n_ch, a.lanes)), dim3(64), 0, st, a);
            else hipLaunchKernelGGL(k_amssb_generic<AMSSB_SSB>, dim3(cdiv(p->n_ch, a.lanes)), dim3(64), 0, st, a);
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
    return nb * B;
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
    if (n_in < 0 || (size_t)n_in > p->max_in) return fail_msg(-3, "amssb: n_in should be 0 .. the max_samples_per_call given to create (%zu)", p->max_in);
    if (n_in > 0 && (!in || in_pitch < (size_t)n_in)) return fail_msg(-3, "amssb: need in and in_pitch >= n_in");
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
    return run_tail(p, x, xp, n, audio_s16, pre_agc_f, out_pitch);
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
