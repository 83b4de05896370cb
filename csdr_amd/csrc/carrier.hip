// carrier.hip -- carrier recovery for n_channels channels per call (MI355X / gfx950): bpsk_costas_loop_cc (libcsdr.c:2094-2142) and pll_cc (libcsdr.c:1856-1915).
//
// A loop is sample-serial within a channel (the NCO phase of sample k + 1 needs the error of sample k, and a double cos, sin and atan2 lie on that chain) and
// independent across channels; the loop coefficients are shared, the state (phase, dphase, freq) is per channel and stays on the device between calls.
//   k_carrier_tiled   C channels per one-wave workgroup.  Per tile of 64 samples all 64 lanes stage each channel's input row into LDS (one coalesced 512-byte
//                     load per channel, the next tile's loads already in flight), lane c walks channel c over the tile and leaves the requested outputs in LDS,
//                     and all lanes write every requested output tile back coalesced.  An output that was not asked for is neither stored to LDS nor written.
//   k_carrier         one lane per channel, straight from and to global memory, float by float: any pointer alignment.  force_generic(1) takes it always.
// Both run carrier_dev.hpp's step function on the same samples in the same order: the same bits, for every C, every batch position and every cut into calls.
#include "bank.hpp"
#include "carrier_dev.hpp"
#include <string.h>
#include <algorithm>
#include <vector>

using namespace csdr_amd;

namespace {

static_assert(sizeof(CarrierChan) == sizeof(csdr_amd_carrier_chan), "CarrierChan mirrors csdr_amd_carrier_chan");

struct CarrierArgs {
    CarrierCfg cfg; CarrierChan *st; int n_ch, lanes;
    const float *in; long long n; size_t in_pitch;
    float *out, *err, *dph, *nco; size_t out_pitch;
};

__global__ __launch_bounds__(64) void k_carrier(CarrierArgs a)
{
    if ((int)threadIdx.x >= a.lanes) return;
    const int ch = blockIdx.x * a.lanes + threadIdx.x;
    if (ch >= a.n_ch) return;
    CarrierChan s = a.st[ch];
    const float *x = a.in + 2 * (size_t)ch * a.in_pitch;
    const size_t oo = (size_t)ch * a.out_pitch;
    for (long long j = 0; j < a.n; j++) {
        CarrierSample o;
        carrier_step(a.cfg, s, x[2 * j], x[2 * j + 1], o);
        if (a.out) { a.out[2 * (oo + j)] = o.out.x; a.out[2 * (oo + j) + 1] = o.out.y; }
        if (a.err) a.err[oo + j] = o.error;
        if (a.dph) a.dph[oo + j] = o.dphase;
        if (a.nco) { a.nco[2 * (oo + j)] = o.nco.x; a.nco[2 * (oo + j) + 1] = o.nco.y; }
    }
    a.st[ch] = s;
}

constexpr int CT = 64;                                   // samples per tile (= lanes per wave: one coalesced row per load)
constexpr int CTP = CT + 1;                              // odd row stride: the chain lanes' same-column accesses fall in different banks
constexpr int CMAX = 64;                                 // channels per workgroup at most (one sample per channel is held ahead in registers)
constexpr size_t tiled_lds(int C) { return (size_t)C * CTP * (3 * sizeof(float2) + 2 * sizeof(float)); }

__global__ __launch_bounds__(64) void k_carrier_tiled(CarrierArgs a, int C)
{
    extern __shared__ float2 lds2[];
    float2 *xr = lds2, *orow = xr + (size_t)C * CTP, *nrow = orow + (size_t)C * CTP;
    float *erow = (float *)(nrow + (size_t)C * CTP), *drow = erow + (size_t)C * CTP;
    const int lane = threadIdx.x, ch0 = blockIdx.x * C;
    const int nc = min(C, a.n_ch - ch0);
    const bool chain = lane < nc;
    const float2 *in = (const float2 *)a.in;
    float2 *out = (float2 *)a.out, *nco = (float2 *)a.nco;
    CarrierChan s{0.f, 0.f, 0.f};
    if (chain) s = a.st[ch0 + lane];
    const int me = lane * CTP;

    float2 nx[CMAX];                                     // the next tile, loaded while the chain lanes walk this one
    auto fetch = [&](long long b) {
#pragma unroll
        for (int cc = 0; cc < CMAX; cc++)
            if (cc < nc) nx[cc] = b + lane < a.n ? in[(size_t)(ch0 + cc) * a.in_pitch + b + lane] : make_float2(0.f, 0.f);
    };
    fetch(0);
    for (long long base = 0; base < a.n; base += CT) {
#pragma unroll
        for (int cc = 0; cc < CMAX; cc++)                // 1. stage: lane j holds sample base + j of channel cc
            if (cc < nc) xr[cc * CTP + lane] = nx[cc];
        __syncthreads();                                 // (also: the write-back of the tile before has read its rows)
        if (base + CT < a.n) fetch(base + CT);
        if (chain) {                                     // 2. lane c walks channel c
            const int m = (int)min((long long)CT, a.n - base);
            for (int j0 = 0; j0 < m; j0 += 8) {
                float2 v[8];                             // 8 samples to registers first: the LDS latency stays off the chain
#pragma unroll
                for (int j = 0; j < 8; j++) v[j] = xr[me + j0 + j];       // (rows are CT long and zero-filled: in bounds beyond m)
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    if (j0 + j < m) {
                        CarrierSample o;
                        carrier_step(a.cfg, s, v[j].x, v[j].y, o);
                        if (out) orow[me + j0 + j] = o.out;
                        if (a.err) erow[me + j0 + j] = o.error;
                        if (a.dph) drow[me + j0 + j] = o.dphase;
                        if (nco) nrow[me + j0 + j] = o.nco;
                    }
                }
            }
        }
        __syncthreads();
        if (base + lane < a.n) {                         // 3. write back: lane j stores sample base + j of every channel
            for (int cc = 0; cc < nc; cc++) {
                const size_t g = (size_t)(ch0 + cc) * a.out_pitch + base + lane;
                if (out) out[g] = orow[cc * CTP + lane];
                if (a.err) a.err[g] = erow[cc * CTP + lane];
                if (a.dph) a.dph[g] = drow[cc * CTP + lane];
                if (nco) nco[g] = nrow[cc * CTP + lane];
            }
        }
    }
    if (chain) a.st[ch0 + lane] = s;
}

// channels per wave when the caller leaves it open.  A wave's walk takes the same time whatever the number of its lanes that walk, so more channels per wave
// is fewer waves for the same time each, until the tiled kernel's staging of many rows per tile shows (32, 64): DESIGN section 4l holds the sweeps on 4096 channels
int default_lanes(int n_ch, bool tiled) { return std::max(1, std::min(tiled ? 16 : 64, n_ch)); }

int check_params(const csdr_amd_carrier_params *p, CarrierCfg *c)
{
    if (!p) return fail_msg(-3, "carrier: null params");
    if (p->mode < CARRIER_COSTAS || p->mode > CARRIER_PLL_PI) return fail_msg(-3, "carrier: mode is 0 (COSTAS), 1 (COSTAS_DD), 2 (PLL_P) or 3 (PLL_PI)");
    // the bounds keep the phase wraps of one sample to a few turns
    if (!(fabsf(p->alpha) <= 64.f) || !(fabsf(p->beta) <= 64.f)) return fail_msg(-3, "carrier: need |alpha| <= 64 and |beta| <= 64");
    if (p->mode <= CARRIER_COSTAS_DD && !(p->dphase_max >= 0.f && p->dphase_max <= 64.f)) return fail_msg(-3, "carrier: need 0 <= dphase_max <= 64");
    c->mode = p->mode; c->alpha = p->alpha; c->beta = p->beta; c->dphase_max = p->dphase_max; c->reset_to_zero = p->dphase_max_reset_to_zero != 0;
    return 0;
}

int check_chan(const csdr_amd_carrier_chan *s)
{
    if (!(fabsf(s->phase) <= 1024.f) || !(fabsf(s->dphase) <= 1024.f) || !(fabsf(s->freq) <= 1024.f))
        return fail_msg(-3, "carrier: channel state should be finite, each of |phase|, |dphase|, |freq| <= 1024");
    return 0;
}

} // namespace

struct csdr_amd_carrier : ChanBank<CarrierChan> {
    CarrierCfg cfg;
};

extern "C" {

int csdr_amd_costas_params(float bandwidth, float damping, int decision_directed, csdr_amd_carrier_params *p)
{
    if (!p) return fail_msg(-3, "costas_params: null params");
    memset(p, 0, sizeof *p);
    p->mode = decision_directed ? CARRIER_COSTAS_DD : CARRIER_COSTAS;
    costas_coefficients(bandwidth, damping, &p->alpha, &p->beta, &p->dphase_max);
    return 0;
}

int csdr_amd_pll_params_p(float alpha, csdr_amd_carrier_params *p)
{
    if (!p) return fail_msg(-3, "pll_params_p: null params");
    memset(p, 0, sizeof *p);
    p->mode = CARRIER_PLL_P; p->alpha = alpha;
    return 0;
}

int csdr_amd_pll_params_pi(float bandwidth, float ko, float kd, float damping, csdr_amd_carrier_params *p)
{
    if (!p) return fail_msg(-3, "pll_params_pi: null params");
    memset(p, 0, sizeof *p);
    p->mode = CARRIER_PLL_PI;
    pll_pi_coefficients(bandwidth, ko, kd, damping, &p->alpha, &p->beta);
    return 0;
}

csdr_amd_carrier *csdr_amd_carrier_create(csdr_amd_ctx *c, const csdr_amd_carrier_params *params, int n_channels)
{
    CarrierCfg cfg;
    if (bank_create_check("carrier", c, n_channels) < 0 || check_params(params, &cfg) < 0) return nullptr;
    Owned<csdr_amd_carrier, csdr_amd_carrier_destroy> p(new csdr_amd_carrier());
    p->c = c; p->cfg = cfg; p->n_ch = n_channels;
    if (dev_alloc(p->d_st, sizeof(CarrierChan) * n_channels) != hipSuccess) { fail_msg(-2, "carrier: out of device memory"); return nullptr; }
    if (csdr_amd_carrier_reset(p.get()) < 0) return nullptr;
    return p.release();
}

// every channel back to phase = dphase = freq = 0 (what the reference's init functions leave): zero bytes, on the context's stream in order with the calls
int csdr_amd_carrier_reset(csdr_amd_carrier *p) { return bank_reset(p, "carrier", nullptr); }
int csdr_amd_carrier_reset_channel(csdr_amd_carrier *p, int ch) { return bank_reset_channel(p, "carrier", ch, CarrierChan{0.f, 0.f, 0.f}); }
int csdr_amd_carrier_get_channel(csdr_amd_carrier *p, int ch, csdr_amd_carrier_chan *out) { return bank_get_channel(p, "carrier", ch, out); }
int csdr_amd_carrier_set_channel(csdr_amd_carrier *p, int ch, const csdr_amd_carrier_chan *s)
{
    return bank_set_channel(p, "carrier", ch, s, [&] { return check_chan(s); });
}

int csdr_amd_carrier_set_lanes(csdr_amd_carrier *p, int lanes) { return bank_set_lanes(p, "carrier", lanes); }
int csdr_amd_carrier_lanes(const csdr_amd_carrier *p)
{
    if (!p) return 0;
    return p->force_generic ? bank_lanes(p, default_lanes(p->n_ch, false)) : bank_lanes(p, default_lanes(p->n_ch, true), CMAX);
}

int csdr_amd_carrier_force_generic(csdr_amd_carrier *p, int on) { return bank_force_generic(p, "carrier", on); }
const char *csdr_amd_carrier_kernel_name(const csdr_amd_carrier *p) { return bank_kernel_name(p); }

void csdr_amd_carrier_destroy(csdr_amd_carrier *p) { destroy_on_stream(p); }

int csdr_amd_carrier_process(csdr_amd_carrier *p, const csdr_complexf *in, long long n, size_t in_pitch, csdr_complexf *out, float *error, float *dphase,
                             csdr_complexf *nco, size_t out_pitch)
{
    if (!p) return fail_msg(-3, "carrier: null object");
    if (n < 0 || n > (1LL << 30)) return fail_msg(-3, "carrier: n should be 0 .. 2^30");
    if (!out && !error && !dphase && !nco) return fail_msg(-3, "carrier: at least one of out, error, dphase, nco is required");
    if (p->cfg.mode >= CARRIER_PLL_P && (out || error)) return fail_msg(-3, "carrier: the PLL modes give nco and dphase only");
    if (n > 0 && (!in || in_pitch < (size_t)n || out_pitch < (size_t)n)) return fail_msg(-3, "carrier: need in, in_pitch >= n and out_pitch >= n");
    if (!n) return 0;
    CarrierArgs a;
    a.cfg = p->cfg; a.st = p->d_st.get(); a.n_ch = p->n_ch;
    a.in = (const float *)in; a.n = n; a.in_pitch = in_pitch;
    a.out = (float *)out; a.err = error; a.dph = dphase; a.nco = (float *)nco; a.out_pitch = out_pitch;
    const bool aligned = !(((uintptr_t)in | (uintptr_t)out | (uintptr_t)nco) & 7);
    if (!p->force_generic && aligned) {
        const int C = a.lanes = bank_launch_lanes(p, "k_carrier_tiled", default_lanes(p->n_ch, true), CMAX);
        if (tiled_lds(C) > 64 * 1024 && lds_attr_once((const void *)k_carrier_tiled, tiled_lds(CMAX)) < 0) return -2;
        hipLaunchKernelGGL(k_carrier_tiled, dim3(cdiv(p->n_ch, C)), dim3(64), tiled_lds(C), p->c->stream, a, C);
    } else {
        a.lanes = bank_launch_lanes(p, "k_carrier", default_lanes(p->n_ch, false));
        hipLaunchKernelGGL(k_carrier, dim3(cdiv(p->n_ch, a.lanes)), dim3(64), 0, p->c->stream, a);
    }
    CSDR_LAUNCH_CHECK();
    return 0;
}

// CPU run of the kernels' step function for one channel, the stream cut into calls of cuts[0], cuts[1], ... samples (the rest of n in one more call); any of
// the outputs may be NULL.  state_io (may be NULL: a fresh channel) carries the channel state in and out.  Returns n.
long long csdr_amd_debug_carrier_walk(const csdr_amd_carrier_params *params, const csdr_complexf *in, long long n, const long long *cuts, int n_cuts,
                                      csdr_complexf *out, float *error, float *dphase, csdr_complexf *nco, csdr_amd_carrier_chan *state_io)
{
    CarrierCfg cfg;
    if (check_params(params, &cfg) < 0) return -3;
    if (n < 0 || (n > 0 && !in) || n_cuts < 0 || (n_cuts && !cuts)) return fail_msg(-3, "debug_carrier_walk: bad arguments");
    if (cfg.mode >= CARRIER_PLL_P && (out || error)) return fail_msg(-3, "carrier: the PLL modes give nco and dphase only");
    CarrierChan s{0.f, 0.f, 0.f};
    if (state_io) { if (check_chan(state_io) < 0) return -3; memcpy(&s, state_io, sizeof s); }
    for_each_call(n, cuts, n_cuts, [&](long long done, long long m) {
        CarrierChan t = s;                               // a call: state in, samples, state out
        for (long long j = done; j < done + m; j++) {
            CarrierSample o;
            carrier_step(cfg, t, in[j].i, in[j].q, o);
            if (out) { out[j].i = o.out.x; out[j].q = o.out.y; }
            if (error) error[j] = o.error;
            if (dphase) dphase[j] = o.dphase;
            if (nco) { nco[j].i = o.nco.x; nco[j].q = o.nco.y; }
        }
        s = t;
    });
    if (state_io) memcpy(state_io, &s, sizeof s);
    return n;
}

} // extern "C"
