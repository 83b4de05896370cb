// psk31.hip -- the BPSK31 receive chain for n_channels channels per call (MI355X / gfx950):
//   simple_agc_cc | timing_recovery_cc | dbpsk_decoder_c_u8 | psk31_varicode_decoder_u8_u8      (psk31_dev.hpp: the per-channel step functions)
//
// The chain is sample-serial within a channel (the gain recurrence, the timing loop's data-dependent symbol positions, the shift register) and independent
// across channels, so k_psk31 runs one lane per channel and walks the whole stage range in one launch.  The fused form reads each input sample once and
// writes only the stage range's last output and per-channel counts: timing recovery asks the AGC for three positions per symbol, so the AGC'd stream never
// leaves the lane.  Each channel's state (gain, unconsumed tail, correction_offset, last symbol, shift register) stays on the device between calls.
// The fused range (AGC first, timing recovery or later last) runs on k_psk31_tiled: the input is staged through LDS in coalesced tiles, the independent part
// of the AGC is computed there by all lanes, and one lane per channel is left with the gain recurrence and the per-symbol work.  Every other stage range,
// and a decimation whose ring does not fit in LDS, runs on k_psk31 (one lane per channel, straight from global memory).  Both give the same bits.
// csdr_amd_psk31_set_lanes sets the channels per wave, csdr_amd_psk31_force_generic(1) takes k_psk31 always.
#include "bank.hpp"
#include "psk31_dev.hpp"
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>

using namespace csdr_amd;

namespace {

// The PSK31 varicode (G3PLX), characters 0..127 as {code, length}: codes start with 1 and contain no 00.
const struct { uint16_t code; uint8_t bits; } VARICODE[128] = {
    {0x2AB, 10}, {0x2DB, 10}, {0x2ED, 10}, {0x377, 10}, {0x2EB, 10}, {0x35F, 10}, {0x2EF, 10}, {0x2FD, 10},     // NUL SOH STX ETX EOT ENQ ACK BEL
    {0x2FF, 10}, {0xEF, 8},   {0x1D, 5},   {0x36F, 10}, {0x2DD, 10}, {0x1F, 5},   {0x375, 10}, {0x3AB, 10},     // BS HT LF VT FF CR SO SI
    {0x2F7, 10}, {0x2F5, 10}, {0x3AD, 10}, {0x3AF, 10}, {0x35B, 10}, {0x36B, 10}, {0x36D, 10}, {0x357, 10},     // DLE DC1 DC2 DC3 DC4 NAK SYN ETB
    {0x37B, 10}, {0x37D, 10}, {0x3B7, 10}, {0x355, 10}, {0x35D, 10}, {0x3BB, 10}, {0x2FB, 10}, {0x37F, 10},     // CAN EM SUB ESC FS GS RS US
    {0x1, 1},    {0x1FF, 9},  {0x15F, 9},  {0x1F5, 9},  {0x1DB, 9},  {0x2D5, 10}, {0x2BB, 10}, {0x17F, 9},      // space ! " # $ % & '
    {0xFB, 8},   {0xF7, 8},   {0x16F, 9},  {0x1DF, 9},  {0x75, 7},   {0x35, 6},   {0x57, 7},   {0x1AF, 9},      // ( ) * + , - . /
    {0xB7, 8},   {0xBD, 8},   {0xED, 8},   {0xFF, 8},   {0x177, 9},  {0x15B, 9},  {0x16B, 9},  {0x1AD, 9},      // 0 .. 7
    {0x1AB, 9},  {0x1B7, 9},  {0xF5, 8},   {0x1BD, 9},  {0x1ED, 9},  {0x55, 7},   {0x1D7, 9},  {0x2AF, 10},     // 8 9 : ; < = > ?
    {0x2BD, 10}, {0x7D, 7},   {0xEB, 8},   {0xAD, 8},   {0xB5, 8},   {0x77, 7},   {0xDB, 8},   {0xFD, 8},       // @ A .. G
    {0x155, 9},  {0x7F, 7},   {0x1FD, 9},  {0x17D, 9},  {0xD7, 8},   {0xBB, 8},   {0xDD, 8},   {0xAB, 8},       // H .. O
    {0xD5, 8},   {0x1DD, 9},  {0xAF, 8},   {0x6F, 7},   {0x6D, 7},   {0x157, 9},  {0x1B5, 9},  {0x15D, 9},      // P .. W
    {0x175, 9},  {0x17B, 9},  {0x2AD, 10}, {0x1F7, 9},  {0x1EF, 9},  {0x1FB, 9},  {0x2BF, 10}, {0x16D, 9},      // X Y Z [ \ ] ^ _
    {0x2DF, 10}, {0xB, 4},    {0x5F, 7},   {0x2F, 6},   {0x2D, 6},   {0x3, 2},    {0x3D, 6},   {0x5B, 7},       // ` a .. g
    {0x2B, 6},   {0xD, 4},    {0x1EB, 9},  {0xBF, 8},   {0x1B, 5},   {0x3B, 6},   {0xF, 4},    {0x7, 3},        // h .. o
    {0x3F, 6},   {0x1BF, 9},  {0x15, 5},   {0x17, 5},   {0x5, 3},    {0x37, 6},   {0x7B, 7},   {0x6B, 7},       // p .. w
    {0xDF, 8},   {0x5D, 7},   {0x1D5, 9},  {0x2B7, 10}, {0x1BB, 9},  {0x2B5, 10}, {0x2D7, 10}, {0x3B5, 10},     // x y z { | } ~ DEL
};

struct VaricodeDec {
    uint8_t t[1024];
    VaricodeDec() { memset(t, 0, sizeof t); for (int a = 0; a < 128; a++) t[VARICODE[a].code] = (uint8_t)a; }
};
const VaricodeDec &varicode_dec() { static const VaricodeDec d; return d; }

static_assert(sizeof(Psk31Chan) == sizeof(csdr_amd_psk31_chan), "Psk31Chan mirrors csdr_amd_psk31_chan");

int make_cfg(const csdr_amd_psk31_params *p, int first, int last, Psk31Cfg *c)
{
    if (!p) return fail_msg(-3, "psk31: null params");
    if (first < PSK31_AGC || last > PSK31_VARICODE || first > last) return fail_msg(-3, "psk31: need 0 <= first_stage <= last_stage <= 3");
    if (first == PSK31_AGC && !(p->rate > 0 && p->reference > 0 && p->max_gain > 0)) return fail_msg(-3, "psk31: rate, reference and max_gain should be > 0");
    const bool timing = first <= PSK31_TIMING && last >= PSK31_TIMING;
    if (timing) {
        if (p->algorithm != 0 && p->algorithm != 1) return fail_msg(-3, "psk31: algorithm is 0 (GARDNER) or 1 (EARLYLATE)");
        if (p->decimation <= 4 || (p->decimation & 3) || p->decimation > (1 << 20)) return fail_msg(-3, "psk31: decimation factor should be a positive integer divisible by 4");
        if (!(p->max_error >= 0) || !(fabsf(p->loop_gain) * p->max_error <= 1.f))
            return fail_msg(-3, "psk31: need max_error >= 0 and |loop_gain| * max_error <= 1 (a symbol then moves on by D/2 .. 3D/2 samples)");
    }
    memset(c, 0, sizeof *c);
    c->rate = p->rate; c->rate_1minus = 1 - p->rate; c->reference = p->reference; c->max_gain = p->max_gain;
    c->algorithm = p->algorithm; c->D = p->decimation; c->hb = p->decimation / 2; c->qb = p->decimation / 4;
    c->wing = (int)(p->decimation * 0.25f); c->use_q = p->use_q != 0;
    c->loop_gain = p->loop_gain; c->max_error = p->max_error;
    c->hb_sign = (float)(c->hb * (p->algorithm == 0 ? -1 : 1));
    c->reset_lo = -c->qb * 0.9; c->reset_hi = 0.9 * c->qb;
    c->first = first; c->last = last;
    return 0;
}

__global__ __launch_bounds__(64) void k_psk31(Psk31Cfg c, Psk31Chan *__restrict__ st, float2 *__restrict__ tails, int tail_cap, int n_ch, int lanes,
                                              const void *__restrict__ in, long long n_in, size_t in_pitch, void *__restrict__ out, size_t out_pitch,
                                              int *__restrict__ counts, float *__restrict__ err, unsigned *__restrict__ idx, const uint8_t *__restrict__ dec)
{
    if ((int)threadIdx.x >= lanes) return;
    const int ch = blockIdx.x * lanes + threadIdx.x;
    if (ch >= n_ch) return;
    const size_t io = (size_t)ch * in_pitch, oo = (size_t)ch * out_pitch;
    Psk31Out o{nullptr, nullptr, err ? err + oo : nullptr, idx ? idx + oo : nullptr};
    if (c.last <= PSK31_TIMING) o.c = (float2 *)out + oo; else o.b = (uint8_t *)out + oo;
    Psk31Chan s = st[ch];
    const float2 *xc = c.first <= PSK31_DBPSK ? (const float2 *)in + io : nullptr;
    const uint8_t *xb = c.first == PSK31_VARICODE ? (const uint8_t *)in + io : nullptr;
    counts[ch] = psk31_walk(c, s, tails + (size_t)ch * tail_cap, xc, xb, n_in, o, dec);
    st[ch] = s;
}

// k_psk31_tiled: the fused form (first stage AGC, last stage timing recovery or later) for C channels per one-wave workgroup.  Per tile of PT samples:
//   1. all 64 lanes stage the tile of every channel into an LDS ring (one channel row of 64 consecutive samples per load: coalesced) and compute the
//      independent part of the AGC there, ideal = clamp(reference / |x|) with correctly rounded sqrt and division;
//   2. lane c walks channel c's gain recurrence over the tile (three dependent ops per sample; the gain overwrites `ideal` in the ring), then runs timing
//      recovery, DBPSK and varicode for every symbol whose three positions are in the ring.
// The ring (R samples, R >= 3 D/2 + PT + 2) keeps every position a pending symbol or the unconsumed tail can still read, so nothing is walked twice.
// At the end the tail V[cbi ..) goes back to the device state raw, with the gain in front of it: the same state and bits as k_psk31's walk.
constexpr int PT = 64;                                   // samples per tile (= lanes per wave: one coalesced row per load)
constexpr int TILED_LDS = 63 * 1024;                     // ring budget per workgroup (within the 64 KiB a launch gets without an attribute)

int tiled_ring(int hb) { const int r = 3 * hb + PT + 2; return (r + PT - 1) / PT * PT; }
size_t tiled_lds(int C, int R) { const int RP = R + 1; return sizeof(float) * (((size_t)C * RP + 1) & ~(size_t)1) + sizeof(float2) * (size_t)C * RP; }

__global__ __launch_bounds__(64) void k_psk31_tiled(Psk31Cfg c, Psk31Chan *__restrict__ st, float2 *__restrict__ tails, int tail_cap, int n_ch, int C, int R,
                                                    const float2 *__restrict__ in, long long n_in, size_t in_pitch, void *__restrict__ out, size_t out_pitch,
                                                    int *__restrict__ counts, float *__restrict__ err, unsigned *__restrict__ idx, const uint8_t *__restrict__ dec)
{
    extern __shared__ float lds[];
    __shared__ int s_t0[64];
    const int RP = R + 1;                                // odd row stride: the chain lanes' same-slot accesses fall in different banks
    float *gr = lds;
    float2 *xr = (float2 *)(lds + (((size_t)C * RP + 1) & ~(size_t)1));
    const int lane = threadIdx.x, ch0 = blockIdx.x * C;
    const int nc = min(C, n_ch - ch0);
    if (lane < nc) s_t0[lane] = st[ch0 + lane].tail_len;
    __syncthreads();
    int t0max = 0;
    for (int k = 0; k < nc; k++) t0max = max(t0max, s_t0[k]);
    const long long nVmax = t0max + n_in;

    const bool chain = lane < nc;
    const int ch = ch0 + lane;
    Psk31Chan s;
    Psk31Out o{nullptr, nullptr, nullptr, nullptr};
    long long nV = 0, cbi = 0;
    int corr = 0;
    float g = 0.f;
    if (chain) {
        s = st[ch];
        nV = s.tail_len + n_in;
        corr = s.corr; g = s.gain;
        const size_t oo = (size_t)ch * out_pitch;
        o.err = err ? err + oo : nullptr; o.idx = idx ? idx + oo : nullptr;
        if (c.last <= PSK31_TIMING) o.c = (float2 *)out + oo; else o.b = (uint8_t *)out + oo;
    }
    Psk31Tail t{&c, &s, &o, dec, (chain && c.last >= PSK31_DBPSK) ? psk31_phase(s.last_i, s.last_q) : 0.f, 0};
    const float g0 = g;
    float *gme = gr + (size_t)lane * RP;
    float2 *xme = xr + (size_t)lane * RP;

    // the tile's samples, loaded one tile ahead: the next tile's global loads are in flight while the chain lanes walk this one
    constexpr int CMAX = 16;
    float2 nx[CMAX];
    auto fetch = [&](long long b) {
#pragma unroll
        for (int cc = 0; cc < CMAX; cc++) {
            if (cc < nc) {
                const long long p = b + lane, T0 = s_t0[cc];
                nx[cc] = p < T0 + n_in ? (p < T0 ? tails[(size_t)(ch0 + cc) * tail_cap + p] : in[(size_t)(ch0 + cc) * in_pitch + (p - T0)]) : make_float2(0.f, 0.f);
            }
        }
    };
    fetch(0);
    for (long long base = 0; base < nVmax; base += PT) {
        const int slot0 = (int)((unsigned)base % (unsigned)R);
#pragma unroll
        for (int cc = 0; cc < CMAX; cc++) {              // 1. stage: lane j holds sample base + j of channel cc
            if (cc < nc && base + lane < s_t0[cc] + n_in) {
                const float2 x = nx[cc];
                xr[(size_t)cc * RP + slot0 + lane] = x;
                gr[(size_t)cc * RP + slot0 + lane] = psk31_ideal_gain(x.x, x.y, c.reference, c.max_gain);
            }
        }
        __syncthreads();
        if (base + PT < nVmax) fetch(base + PT);
        if (chain && base < nV) {                        // 2. the chain lane
            const int m = (int)min((long long)PT, nV - base);
            float *gp = gme + slot0;
            if (m == PT) {
                for (int j0 = 0; j0 < PT; j0 += 16) {    // 16 ideals to registers first: the LDS latency stays off the chain
                    float v[16];
#pragma unroll
                    for (int j = 0; j < 16; j++) v[j] = gp[j0 + j];
#pragma unroll
                    for (int j = 0; j < 16; j++) { g = psk31_agc_step(g, v[j], c.rate, c.rate_1minus); v[j] = g; }
#pragma unroll
                    for (int j = 0; j < 16; j++) gp[j0 + j] = v[j];
                }
            } else {
                for (int j = 0; j < m; j++) { g = psk31_agc_step(g, gp[j], c.rate, c.rate_1minus); gp[j] = g; }
            }
            const long long end = base + m;
            while (cbi + c.hb * 3 < end) {
                long long pl, pm, pr;
                psk31_positions(c, cbi, &corr, &pl, &pm, &pr);
                const int sl = (int)((unsigned)pl % (unsigned)R), sm = (int)((unsigned)pm % (unsigned)R), sr = (int)((unsigned)pr % (unsigned)R);   // (positions < 2^31)
                const float2 a = xme[sl], b = xme[sm], d = xme[sr];
                const float gl = gme[sl], gm = gme[sm], gq = gme[sr];
                corr = psk31_symbol(c, s, t, o, make_float2(gl * a.x, gl * a.y), make_float2(gm * b.x, gm * b.y), make_float2(gq * d.x, gq * d.y),
                                    c.algorithm == 1 ? pm : pl);
                cbi += c.D + corr;
            }
        }
        __syncthreads();
    }
    if (!chain) return;
    // the unconsumed tail V[cbi ..) (at most 3 D/2 samples, all still in the ring), raw, with the gain in front of it
    const int nt = (int)(nV - cbi);
    float2 *tl = tails + (size_t)ch * tail_cap;
    for (int j = 0; j < nt; j++) tl[j] = xme[(int)((cbi + j) % R)];
    s.gain = cbi > 0 ? gme[(int)((cbi - 1) % R)] : g0;
    s.tail_len = nt;
    s.corr = corr;
    s.base += (uint32_t)cbi;
    st[ch] = s;
    counts[ch] = t.k;
}

__global__ __launch_bounds__(64) void k_simple_agc(Psk31Cfg c, const float2 *__restrict__ in, float2 *__restrict__ out, int n_streams, long long n, size_t in_pitch,
                                                   size_t out_pitch, float *__restrict__ gain_io)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_streams) return;
    gain_io[s] = psk31_agc_run(c, gain_io[s], in + (size_t)s * in_pitch, out + (size_t)s * out_pitch, n);
}

// channels per wave when the caller leaves it open.  k_psk31_tiled: about two waves per SIMD (4096 channels on 256 CUs: 2); k_psk31: one wave per CU.
// profiles/psk31_lanes.txt holds the runs behind both choices.
int default_lanes(int cus, int n_ch, bool tiled)
{
    if (tiled) return std::max(1, std::min(16, (int)cdiv(n_ch, (size_t)cus * 8)));
    return std::max(1, std::min(64, (int)cdiv(n_ch, (size_t)cus)));
}

Psk31Chan fresh_chan() { Psk31Chan s; memset(&s, 0, sizeof s); s.gain = 1.f; return s; }      // the CLI starts the gain at 1 (csdr.c:2917)

} // namespace

struct csdr_amd_psk31 : ChanBank<Psk31Chan> {
    Psk31Cfg cfg; int tail_cap, cus, ring;
    DevBuf<float2> d_tail; DevBuf<uint8_t> d_dec;
};

extern "C" {

csdr_amd_psk31 *csdr_amd_psk31_create(csdr_amd_ctx *c, const csdr_amd_psk31_params *params, int n_channels, int first_stage, int last_stage)
{
    Psk31Cfg cfg;
    if (bank_create_check("psk31", c, n_channels) < 0 || make_cfg(params, first_stage, last_stage, &cfg) < 0) return nullptr;
    Owned<csdr_amd_psk31, csdr_amd_psk31_destroy> p(new csdr_amd_psk31());
    p->c = c; p->cfg = cfg; p->n_ch = n_channels;
    const bool timing = first_stage <= PSK31_TIMING && last_stage >= PSK31_TIMING;
    p->tail_cap = timing ? 3 * cfg.hb + 1 : 1;
    p->cus = current_device_cu_count();
    p->ring = first_stage == PSK31_AGC && last_stage >= PSK31_TIMING ? tiled_ring(cfg.hb) : 0;     // 0: the stage range runs on k_psk31
    if (dev_alloc(p->d_st, sizeof(Psk31Chan) * n_channels) != hipSuccess || dev_alloc(p->d_tail, sizeof(float2) * (size_t)p->tail_cap * n_channels) != hipSuccess ||
        dev_alloc(p->d_dec, 1024) != hipSuccess) { fail_msg(-2, "psk31: out of device memory"); return nullptr; }
    if (csdr_amd_h2d(c, p->d_dec.get(), varicode_dec().t, 1024) < 0 || csdr_amd_psk31_reset(p.get()) < 0) return nullptr;
    return p.release();
}

int csdr_amd_psk31_reset(csdr_amd_psk31 *p) { const Psk31Chan s = fresh_chan(); return bank_reset(p, "psk31", &s); }
int csdr_amd_psk31_reset_channel(csdr_amd_psk31 *p, int ch) { return bank_reset_channel(p, "psk31", ch, fresh_chan()); }
int csdr_amd_psk31_get_channel(csdr_amd_psk31 *p, int ch, csdr_amd_psk31_chan *out) { return bank_get_channel(p, "psk31", ch, out); }

int csdr_amd_psk31_set_channel(csdr_amd_psk31 *p, int ch, const csdr_amd_psk31_chan *s)
{
    return bank_set_channel(p, "psk31", ch, s, [&] {
        const bool ok = s->tail_len >= 0 && s->tail_len <= p->tail_cap - 1 && !(s->tail_len && p->tail_cap == 1);
        return ok ? 0 : fail_msg(-3, "psk31: tail_len out of range");
    });
}

int csdr_amd_psk31_set_lanes(csdr_amd_psk31 *p, int lanes) { return bank_set_lanes(p, "psk31", lanes); }

long long csdr_amd_psk31_max_out(const csdr_amd_psk31 *p, long long n_in)
{
    if (!p || n_in < 0) return 0;
    if (p->cfg.first >= PSK31_DBPSK || p->cfg.last == PSK31_AGC) return n_in;
    return (n_in + p->tail_cap) / p->cfg.hb + 1;           // every symbol moves on by at least D/2 samples
}

int csdr_amd_psk31_process(csdr_amd_psk31 *p, const void *in, long long n_in, size_t in_pitch, void *out, size_t out_pitch, int *counts,
                           float *err, unsigned *idx)
{
    if (!p) return fail_msg(-3, "psk31: null object");
    if (n_in < 0 || n_in > (1LL << 30) || (n_in > 0 && (!in || in_pitch < (size_t)n_in))) return fail_msg(-3, "psk31: need in_pitch >= n_in >= 0 (n_in <= 2^30)");
    if (!counts) return fail_msg(-3, "psk31: counts is required");
    if ((err || idx) && p->cfg.last != PSK31_TIMING) return fail_msg(-3, "psk31: error and index outputs need last_stage == timing recovery");
    const long long mo = csdr_amd_psk31_max_out(p, n_in);
    if (mo > 0 && (!out || out_pitch < (size_t)mo)) return fail_msg(-3, "psk31: out_pitch %zu below max_out %lld", out_pitch, mo);
    csdr_amd_ctx *c = p->c;
    int C = 0;
    if (p->ring && !p->force_generic) {
        C = bank_launch_lanes(p, "k_psk31_tiled", default_lanes(p->cus, p->n_ch, true), 16);      // (k_psk31_tiled holds one sample per channel ahead: 16 at most)
        while (C > 0 && tiled_lds(C, p->ring) > (size_t)TILED_LDS) C--;
    }
    if (C > 0) {
        hipLaunchKernelGGL(k_psk31_tiled, dim3(cdiv(p->n_ch, C)), dim3(64), tiled_lds(C, p->ring), c->stream, p->cfg, p->d_st.get(), p->d_tail.get(), p->tail_cap,
                           p->n_ch, C, p->ring, (const float2 *)in, n_in, in_pitch, out, out_pitch, counts, err, idx, p->d_dec.get());
    } else {
        const int lanes = bank_launch_lanes(p, "k_psk31", default_lanes(p->cus, p->n_ch, false));
        hipLaunchKernelGGL(k_psk31, dim3(cdiv(p->n_ch, lanes)), dim3(64), 0, c->stream, p->cfg, p->d_st.get(), p->d_tail.get(), p->tail_cap, p->n_ch, lanes,
                           in, n_in, in_pitch, out, out_pitch, counts, err, idx, p->d_dec.get());
    }
    CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_psk31_force_generic(csdr_amd_psk31 *p, int on) { return bank_force_generic(p, "psk31", on); }
int csdr_amd_psk31_lanes(const csdr_amd_psk31 *p) { return p ? bank_lanes(p, default_lanes(p->cus, p->n_ch, p->ring && !p->force_generic)) : 0; }
const char *csdr_amd_psk31_kernel_name(const csdr_amd_psk31 *p) { return bank_kernel_name(p); }

void csdr_amd_psk31_destroy(csdr_amd_psk31 *p) { destroy_on_stream(p); }

// simple_agc_cc libcsdr.c:2201-2217 over n_streams streams: the object's AGC-only form with the gain in and out through gain_io (device, n_streams floats)
int csdr_amd_simple_agc_cc(csdr_amd_ctx *c, const csdr_complexf *in, csdr_complexf *out, int n_streams, long long n, size_t in_pitch, size_t out_pitch,
                           float rate, float reference, float max_gain, float *gain_io)
{
    csdr_amd_psk31_params pr; memset(&pr, 0, sizeof pr);
    pr.rate = rate; pr.reference = reference; pr.max_gain = max_gain;
    Psk31Cfg cfg;
    if (!c || n_streams < 1 || !gain_io) return fail_msg(-3, "simple_agc_cc: need a context, n_streams >= 1 and gain_io");
    if (make_cfg(&pr, PSK31_AGC, PSK31_AGC, &cfg) < 0) return -3;
    if (n < 0 || n > (1LL << 30) || (n > 0 && (!in || !out || in_pitch < (size_t)n || out_pitch < (size_t)n))) return fail_msg(-3, "simple_agc_cc: need pitches >= n >= 0");
    if (!n) return 0;
    hipLaunchKernelGGL(k_simple_agc, dim3(cdiv(n_streams, 64)), dim3(64), 0, c->stream, cfg, (const float2 *)in, (float2 *)out, n_streams, n, in_pitch, out_pitch, gain_io);
    CSDR_LAUNCH_CHECK();
    return 0;
}

// CPU run of the kernel's walk for one channel, the stream cut into calls of cuts[0], cuts[1], ... samples (the rest of n in one more call).
// Outputs of all calls are concatenated; state_io (may be NULL: a fresh channel) carries the channel state in and out.  Returns the output count.
long long csdr_amd_debug_psk31_walk(const csdr_amd_psk31_params *params, int first_stage, int last_stage, const void *in, long long n, const long long *cuts,
                                    int n_cuts, void *out, float *err, unsigned *idx, csdr_amd_psk31_chan *state_io)
{
    Psk31Cfg cfg;
    if (make_cfg(params, first_stage, last_stage, &cfg) < 0) return -3;
    if (n < 0 || (n > 0 && (!in || !out)) || n_cuts < 0 || (n_cuts && !cuts)) return fail_msg(-3, "debug_psk31_walk: bad arguments");
    Psk31Chan s = fresh_chan();
    if (state_io) memcpy(&s, state_io, sizeof s);
    std::vector<float2> tail(3 * (size_t)cfg.hb + 2);
    if (s.tail_len < 0 || (size_t)s.tail_len >= tail.size()) return fail_msg(-3, "debug_psk31_walk: tail_len out of range");
    const size_t isz = first_stage == PSK31_VARICODE ? 1 : sizeof(float2), osz = last_stage <= PSK31_TIMING ? sizeof(float2) : 1;
    long long k = 0;
    for_each_call(n, cuts, n_cuts, [&](long long done, long long m) {
        const char *x = (const char *)in + done * isz;
        Psk31Out o{nullptr, nullptr, err ? err + k : nullptr, idx ? idx + k : nullptr};
        if (last_stage <= PSK31_TIMING) o.c = (float2 *)((char *)out + k * osz); else o.b = (uint8_t *)out + k;
        k += psk31_walk(cfg, s, tail.data(), first_stage <= PSK31_DBPSK ? (const float2 *)x : nullptr, first_stage == PSK31_VARICODE ? (const uint8_t *)x : nullptr,
                        m, o, varicode_dec().t);
    });
    if (state_io) memcpy(state_io, &s, sizeof s);
    return k;
}

// psk31_varicode_decoder_push (libcsdr.c:1536-1549) on the host, one bit per call
char csdr_amd_psk31_varicode_decoder_push(unsigned long long *status_shr, unsigned char symbol)
{
    return (char)psk31_varicode_push(status_shr, symbol, varicode_dec().t);
}

// the varicode table: out[2a] = code, out[2a + 1] = length of character a < 128
void csdr_amd_psk31_varicode_table(int *out)
{
    for (int a = 0; a < 128; a++) { out[2 * a] = VARICODE[a].code; out[2 * a + 1] = VARICODE[a].bits; }
}

} // extern "C"
