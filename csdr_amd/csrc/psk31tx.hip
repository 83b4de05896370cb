// psk31tx.hip -- the BPSK31 transmit chain for n_channels channels per call (MI355X / gfx950):
//   psk31_varicode_encoder_u8_u8 | differential_encoder_u8_u8 | psk_modulator_u8_c n_psk | psk31_interpolate_sine_cc I     (psk31tx_dev.hpp: the step functions)
// and the flat helpers differential_decoder_u8_u8 and duplicate_samples_ntimes_u8_u8.
//
// k_psk31tx_generic is the definition: one lane per channel walks its items through the stage range with the step functions; it serves every stage range,
// n_psk and I.  The whole chain (VARICODE .. SHAPE) is serial in the reference only.  Character c starts at bit offset sum (len + 2) over the earlier
// characters, and the differential state in front of it is the starting state XOR the parity of the zero bits so far (len - popcount(code) + 2 per
// character), so the fused path is two kernels:
//   k_psk31tx_plan   one wave per channel scans the characters 64 at a time (an exclusive sum of lengths and an exclusive XOR of parities across the wave,
//                    both carried over chunks and, through the channel state, over calls) and writes the symbol states as packed bits, one per symbol,
//                    into a scratch row, the channel's output count and the symbol in front of the call's first;
//   k_psk31tx_shape  a grid over (channel, tile of TILE_S output samples): rate, 1 - rate and the tile's packed states in LDS, every lane computes two
//                    consecutive complex samples per step and writes them as one 16-byte store, a wave 1 KiB of a row at a time.  A row that starts on
//                    an odd complex sample (odd pitch) pairs its samples one further, its first and last sample then go out as 8-byte stores.
//                    Workgroups past a channel's count leave without storing.
// The fused path needs both tables and the states of a tile in LDS: 8 I + 4 (TILE_S / 32 + 8) bytes within 63 KiB, that is I <= FUSED_MAX_I = 7904; a
// larger I takes the generic path, as does a grid of more than 2^31 - 1 workgroups.  Both paths give the same bits.
#include "bank.hpp"
#include "psk31tx_dev.hpp"
#include <limits.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>

using namespace csdr_amd;

namespace {

static_assert(sizeof(Psk31TxChan) == sizeof(csdr_amd_psk31tx_chan), "Psk31TxChan mirrors csdr_amd_psk31tx_chan");

constexpr int SHAPE_THREADS = 256;
constexpr int SHAPE_STEPS = 16;                                   // 16-byte stores per lane
constexpr int TILE_P = SHAPE_THREADS * SHAPE_STEPS;               // pairs of samples per workgroup
constexpr int TILE_S = 2 * TILE_P;                                // 8192 output samples (64 KiB) per workgroup
constexpr int STATE_WORDS = TILE_S / 32 + 8;                      // packed states a tile can touch (I = 1: one symbol per sample), and the symbol in front
constexpr int FUSED_LDS = 63 * 1024;
constexpr int FUSED_MAX_I = (FUSED_LDS - 4 * STATE_WORDS) / 8;    // 7904

__global__ __launch_bounds__(64) void k_psk31tx_generic(Psk31TxCfg c, Psk31TxTab t, Psk31TxChan *__restrict__ st, int n_ch, const void *__restrict__ in,
                                                        long long n_in, const int *__restrict__ in_counts, size_t in_pitch, void *__restrict__ out,
                                                        size_t out_pitch, int *__restrict__ counts)
{
    const int ch = blockIdx.x * 64 + threadIdx.x;
    if (ch >= n_ch) return;
    long long n = in_counts ? in_counts[ch] : n_in;
    n = n < 0 ? 0 : n > n_in ? n_in : n;
    const size_t io = (size_t)ch * in_pitch, oo = (size_t)ch * out_pitch;
    Psk31TxChan s = st[ch];
    const uint8_t *xb = c.first <= PSK31TX_MOD ? (const uint8_t *)in + io : nullptr;
    const float2 *xc = c.first == PSK31TX_SHAPE ? (const float2 *)in + io : nullptr;
    uint8_t *ob = c.last <= PSK31TX_DIFF ? (uint8_t *)out + oo : nullptr;
    float2 *oc = c.last >= PSK31TX_MOD ? (float2 *)out + oo : nullptr;
    counts[ch] = (int)psk31tx_walk(c, s, t, xb, xc, n, ob, oc);
    st[ch] = s;
}

// One wave per channel.  bits[ch * bits_pitch ..]: the state of symbol k of this call in bit k & 31 of word k >> 5.  prev[ch]: the symbol in front of symbol 0.
__global__ __launch_bounds__(64) void k_psk31tx_plan(int I, Psk31TxTab t, Psk31TxChan *__restrict__ st, int n_ch, const uint8_t *__restrict__ in, long long n_in,
                                                     const int *__restrict__ in_counts, size_t in_pitch, uint32_t *__restrict__ bits, size_t bits_pitch,
                                                     float2 *__restrict__ prev, int *__restrict__ counts)
{
    __shared__ uint32_t w[32];                                    // a chunk's bits: at most 31 carried + 64 * 12 new
    const int ch = blockIdx.x, lane = threadIdx.x;
    if (ch >= n_ch) return;
    long long n = in_counts ? in_counts[ch] : n_in;
    n = n < 0 ? 0 : n > n_in ? n_in : n;
    const uint8_t *x = in + (size_t)ch * in_pitch;
    uint32_t *row = bits + (size_t)ch * bits_pitch;
    const Psk31TxChan s0 = st[ch];
    int state = s0.diff_state & 1;                                // the state in front of the chunk
    long long nbits = 0;                                          // bits in front of the chunk
    uint32_t part = 0;                                            // the bits of the row's unfinished word
    for (long long base = 0; base < n; base += 64) {
        const bool have = base + lane < n;
        const uint8_t c = have ? x[base + lane] : (uint8_t)255;
        int par;
        const int len = psk31tx_char_bits(t.vc, c, &par);
        int off = len, px = par;                                  // inclusive scans over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(off, d), p = __shfl_up(px, d);
            if (lane >= d) { off += o; px ^= p; }
        }
        const int total = __shfl(off, 63), ptotal = __shfl(px, 63);
        off -= len; px ^= par;                                    // exclusive
        const int lead = (int)(nbits & 31);
        if (lane < 32) w[lane] = lane == 0 ? part : 0u;
        __syncthreads();
        if (len) {
            const unsigned e = t.vc[c];
            int sc = state ^ px;
            uint32_t v = 0;
            for (int bi = 0; bi < len; bi++) { if (!psk31tx_code_bit(e, bi)) sc ^= 1; v |= (uint32_t)sc << bi; }
            const int at = lead + off;
            atomicOr(&w[at >> 5], v << (at & 31));
            if ((at & 31) + len > 32) atomicOr(&w[(at >> 5) + 1], v >> (32 - (at & 31)));
        }
        __syncthreads();
        const int full = (lead + total) >> 5;
        if (lane < full) row[(nbits >> 5) + lane] = w[lane];
        part = w[full];
        __syncthreads();
        nbits += total; state ^= ptotal;
    }
    if (lane == 0) {
        if (nbits & 31) row[nbits >> 5] = part;
        prev[ch] = make_float2(s0.last_i, s0.last_q);
        counts[ch] = (int)(nbits * I);
        if (nbits) {
            const float2 y = t.sym[state];
            Psk31TxChan s1; s1.diff_state = (uint8_t)state; s1.last_i = y.x; s1.last_q = y.y;
            st[ch] = s1;
        }
    }
}

// blockIdx.x = channel * n_tiles + tile.  Dynamic LDS: rate[I], rate1m[I], STATE_WORDS words of packed states.
__global__ __launch_bounds__(SHAPE_THREADS) void k_psk31tx_shape(int I, int step_k, int step_j, float2 sym0, float2 sym1, const float *__restrict__ rate,
                                                                 const float *__restrict__ rate1m, const uint32_t *__restrict__ bits, size_t bits_pitch,
                                                                 const float2 *__restrict__ prev, const int *__restrict__ counts, int n_tiles,
                                                                 float2 *__restrict__ out, size_t out_pitch)
{
    extern __shared__ float lds[];
    float *l_rate = lds, *l_rate1m = lds + I;
    uint32_t *l_bits = (uint32_t *)(lds + 2 * (size_t)I);
    const int ch = blockIdx.x / n_tiles, tile = blockIdx.x - ch * n_tiles, tid = threadIdx.x;
    const int count = counts[ch];
    float2 *row = out + (size_t)ch * out_pitch;
    const int a = (int)(((uintptr_t)row >> 3) & 1);               // 1: the row starts on an odd complex sample, so sample 2 p - 1 opens the 16-byte pair p
    const long long s_lo = 2LL * tile * TILE_P - a;               // the tile's samples: s_lo .. s_lo + TILE_S - 1
    if (s_lo >= count) return;
    const int s_first = s_lo < 0 ? 0 : (int)s_lo, s_last = (s_lo + TILE_S < count ? (int)(s_lo + TILE_S) : count) - 1;
    const int k_first = s_first / I - 1, k_last = s_last / I;     // symbols the tile reads (k_first may be -1: the carried symbol)
    const int w_lo = (k_first < 0 ? 0 : k_first) >> 5, n_w = (k_last >> 5) - w_lo + 1;
    for (int j = tid; j < I; j += SHAPE_THREADS) { l_rate[j] = rate[j]; l_rate1m[j] = rate1m[j]; }
    const uint32_t *brow = bits + (size_t)ch * bits_pitch;
    for (int j = tid; j < n_w; j += SHAPE_THREADS) l_bits[j] = brow[w_lo + j];
    __syncthreads();
    const float2 carried = prev[ch];
    auto sym = [&](int k) -> float2 {
        if (k < 0) return carried;
        return ((l_bits[(k >> 5) - w_lo] >> (k & 31)) & 1u) ? sym1 : sym0;
    };
    // this lane's first sample, s = s_lo + 2 tid = k I + j with 0 <= j < I (s = -1: k = -1, j = I - 1); every step moves on by 2 SHAPE_THREADS samples
    long long s = s_lo + 2 * tid;
    int k, j;
    if (s < 0) { k = -1; j = I - 1; } else { k = (int)(s / I); j = (int)(s - (long long)k * I); }
#pragma unroll 4
    for (int it = 0; it < SHAPE_STEPS; it++) {
        int k1 = k, j1 = j + 1;
        if (j1 == I) { j1 = 0; k1++; }
        const bool v0 = s >= 0 && s < count, v1 = s + 1 < count;
        if (v0 && v1) {
            const float2 x0 = sym(k), p0 = sym(k - 1);
            const float2 x1 = k1 == k ? x0 : sym(k1), p1 = k1 == k ? p0 : x0;
            const float2 y0 = psk31tx_shape(x0, p0, l_rate[j], l_rate1m[j]), y1 = psk31tx_shape(x1, p1, l_rate[j1], l_rate1m[j1]);
            *(float4 *)(row + s) = make_float4(y0.x, y0.y, y1.x, y1.y);
        } else if (v0) {
            row[s] = psk31tx_shape(sym(k), sym(k - 1), l_rate[j], l_rate1m[j]);
        } else if (v1) {
            row[s + 1] = psk31tx_shape(sym(k1), sym(k1 - 1), l_rate[j1], l_rate1m[j1]);
        }
        s += 2 * SHAPE_THREADS;
        k += step_k; j += step_j;
        if (j >= I) { j -= I; k++; }
    }
}

__global__ void k_differential_decoder(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, long long n, size_t in_pitch, size_t out_pitch,
                                       const uint8_t *__restrict__ state)
{
    const int s = blockIdx.y;
    const uint8_t *x = in + (size_t)s * in_pitch;
    uint8_t *y = out + (size_t)s * out_pitch;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        y[i] = x[i] == (i ? x[i - 1] : state[s]);
}
__global__ void k_differential_decoder_state(const uint8_t *__restrict__ in, long long n, size_t in_pitch, uint8_t *__restrict__ state, int n_streams)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n_streams) state[s] = in[(size_t)s * in_pitch + n - 1];
}

__global__ void k_duplicate_samples(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, long long n_out, size_t in_pitch, size_t out_pitch,
                                    int sample_size, int ntimes)
{
    const int s = blockIdx.y;
    const uint8_t *x = in + (size_t)s * in_pitch;
    uint8_t *y = out + (size_t)s * out_pitch;
    const long long group = (long long)sample_size * ntimes;
    for (long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x; l < n_out; l += (long long)gridDim.x * blockDim.x) {
        const long long smp = l / group;
        y[l] = x[smp * sample_size + (l - smp * group) % sample_size];
    }
}

// the 128 varicode entries as code | length << 10, from the one table of the library (psk31.hip)
void varicode_entries(uint16_t *vc)
{
    int t[256];
    csdr_amd_psk31_varicode_table(t);
    for (int a = 0; a < 128; a++) vc[a] = (uint16_t)(t[2 * a] | (t[2 * a + 1] << 10));
}

int check_cfg(int n_psk, int interpolation, int first, int last)
{
    if (first < PSK31TX_VARICODE || last > PSK31TX_SHAPE || first > last) return fail_msg(-3, "psk31tx: need 0 <= first_stage <= last_stage <= 3");
    if (n_psk <= 0 || n_psk > 256) return fail_msg(-3, "psk31tx: n_psk should be between 1 and 256");
    if (interpolation <= 0 || interpolation > (1 << 20)) return fail_msg(-3, "psk31tx: interpolation should be >0 (and <= 1048576)");
    return 0;
}

// The host copies of an object's tables.  sym: psk_modulator_u8_c's arithmetic (float increment, float product, libm cos / sin in double, rounded to float);
// rate: psk31_interpolate_sine_cc's (float quotient, the rest in double, rounded to float), and 1 - rate as a float difference.
struct HostTab {
    uint16_t vc[128]; float2 sym[256]; std::vector<float> rate, rate1m;
    HostTab(int n_psk, int I) : rate(I), rate1m(I)
    {
        varicode_entries(vc);
        const float phase_increment = (float)((2 * M_PI) / n_psk);
        for (int v = 0; v < 256; v++) { const float ph = phase_increment * (float)v; sym[v] = make_float2((float)cos((double)ph), (float)sin((double)ph)); }
        for (int j = 0; j < I; j++) {
            rate[j] = (float)((1 + sin(-(M_PI / 2) + M_PI * (double)((float)(j + 1) / (float)I))) / 2);
            rate1m[j] = 1.f - rate[j];
        }
    }
    Psk31TxTab tab() const { return Psk31TxTab{vc, sym, rate.data(), rate1m.data()}; }
};

const Psk31TxChan FRESH = {};      // state 0 (csdr.c:2823), last symbol 0 + 0i (csdr.c:2736-2738); static storage: the padding bytes are 0 too

long long max_out_of(int first, int last, int I, long long n_in)
{
    long long m = n_in;
    if (first == PSK31TX_VARICODE) m *= 12;
    if (last == PSK31TX_SHAPE) m *= I;
    return m;
}

} // namespace

struct csdr_amd_psk31tx : ChanBank<Psk31TxChan> {
    Psk31TxCfg cfg; int n_psk; bool fused; float2 sym0, sym1;
    DevBuf<uint16_t> d_vc; DevBuf<float2> d_sym; DevBuf<float> d_rate;                                // d_rate: rate[I] then rate1m[I]
    DevBuf<uint32_t> d_bits; size_t bits_pitch = 0; DevBuf<float2> d_prev;                            // the plan kernel's rows, grown on demand
    Psk31TxTab tab() const { return Psk31TxTab{d_vc.get(), d_sym.get(), d_rate.get(), d_rate.get() + cfg.I}; }
};

extern "C" {

csdr_amd_psk31tx *csdr_amd_psk31tx_create(csdr_amd_ctx *c, int n_channels, int n_psk, int interpolation, int first_stage, int last_stage)
{
    if (bank_create_check("psk31tx", c, n_channels) < 0 || check_cfg(n_psk, interpolation, first_stage, last_stage) < 0) return nullptr;
    Owned<csdr_amd_psk31tx, csdr_amd_psk31tx_destroy> p(new csdr_amd_psk31tx());
    p->c = c; p->cfg = Psk31TxCfg{first_stage, last_stage, interpolation}; p->n_ch = n_channels; p->n_psk = n_psk;
    p->fused = first_stage == PSK31TX_VARICODE && last_stage == PSK31TX_SHAPE && interpolation <= FUSED_MAX_I;
    const HostTab h(n_psk, interpolation);
    p->sym0 = h.sym[0]; p->sym1 = h.sym[1];
    const size_t I = (size_t)interpolation;
    if (dev_alloc(p->d_st, sizeof(Psk31TxChan) * n_channels) != hipSuccess || dev_alloc(p->d_vc, sizeof h.vc) != hipSuccess ||
        dev_alloc(p->d_sym, sizeof h.sym) != hipSuccess || dev_alloc(p->d_rate, sizeof(float) * 2 * I) != hipSuccess ||
        (p->fused && dev_alloc(p->d_prev, sizeof(float2) * n_channels) != hipSuccess)) { fail_msg(-2, "psk31tx: out of device memory"); return nullptr; }
    if (csdr_amd_h2d(c, p->d_vc.get(), h.vc, sizeof h.vc) < 0 || csdr_amd_h2d(c, p->d_sym.get(), h.sym, sizeof h.sym) < 0 ||
        csdr_amd_h2d(c, p->d_rate.get(), h.rate.data(), sizeof(float) * I) < 0 || csdr_amd_h2d(c, p->d_rate.get() + I, h.rate1m.data(), sizeof(float) * I) < 0 ||
        csdr_amd_psk31tx_reset(p.get()) < 0) return nullptr;
    return p.release();
}

int csdr_amd_psk31tx_reset(csdr_amd_psk31tx *p) { return bank_reset(p, "psk31tx", &FRESH); }
int csdr_amd_psk31tx_reset_channel(csdr_amd_psk31tx *p, int ch) { return bank_reset_channel(p, "psk31tx", ch, FRESH); }
int csdr_amd_psk31tx_get_channel(csdr_amd_psk31tx *p, int ch, csdr_amd_psk31tx_chan *out) { return bank_get_channel(p, "psk31tx", ch, out); }

int csdr_amd_psk31tx_set_channel(csdr_amd_psk31tx *p, int ch, const csdr_amd_psk31tx_chan *s)
{
    Psk31TxChan h; memset(&h, 0, sizeof h);                       // (what is uploaded: the caller's fields, padding bytes defined)
    return bank_set_channel(p, "psk31tx", ch, s, [&] {
        if (p->fused && s->diff_state > 1) return fail_msg(-3, "psk31tx: diff_state is 0 or 1 for the range VARICODE .. SHAPE");   // (its packed states hold one bit)
        h.diff_state = s->diff_state; h.last_i = s->last_i; h.last_q = s->last_q;
        return 0;
    }, &h);
}

long long csdr_amd_psk31tx_max_out(const csdr_amd_psk31tx *p, long long n_in)
{
    if (!p || n_in < 0) return 0;
    return max_out_of(p->cfg.first, p->cfg.last, p->cfg.I, n_in);
}

int csdr_amd_psk31tx_process(csdr_amd_psk31tx *p, const void *in, long long n_in, const int *in_counts, size_t in_pitch, void *out, size_t out_pitch, int *counts)
{
    if (!p) return fail_msg(-3, "psk31tx: null object");
    if (n_in < 0 || n_in > (1LL << 30) || (n_in > 0 && (!in || in_pitch < (size_t)n_in))) return fail_msg(-3, "psk31tx: need in_pitch >= n_in >= 0 (n_in <= 2^30)");
    if (!counts) return fail_msg(-3, "psk31tx: counts is required");
    const long long mo = csdr_amd_psk31tx_max_out(p, n_in);
    if (mo > INT_MAX) return fail_msg(-3, "psk31tx: max_out %lld of this call is above 2^31 - 1", mo);
    if (mo > 0 && (!out || out_pitch < (size_t)mo)) return fail_msg(-3, "psk31tx: out_pitch %zu below max_out %lld", out_pitch, mo);
    csdr_amd_ctx *c = p->c;
    const int I = p->cfg.I;
    const long long n_tiles = (mo + 1 + TILE_S - 1) / TILE_S;     // (+ 1: a row that starts on an odd sample is one sample further in its pairs)
    if (p->fused && !p->force_generic && n_tiles * p->n_ch <= INT_MAX) {
        const size_t words = (size_t)(12 * n_in + 31) / 32 + 1;
        if (words > p->bits_pitch) {
            if (csdr_amd_ctx_sync(c) < 0) return -5;                // an earlier call may still read the rows
            const size_t pitch = words + words / 2;
            if (dev_alloc(p->d_bits, sizeof(uint32_t) * pitch * p->n_ch) != hipSuccess) { p->bits_pitch = 0; return fail_msg(-2, "psk31tx: out of device memory"); }
            p->bits_pitch = pitch;
        }
        hipLaunchKernelGGL(k_psk31tx_plan, dim3(p->n_ch), dim3(64), 0, c->stream, I, p->tab(), p->d_st.get(), p->n_ch, (const uint8_t *)in, n_in, in_counts, in_pitch,
                           p->d_bits.get(), p->bits_pitch, p->d_prev.get(), counts);
        CSDR_LAUNCH_CHECK();
        if (n_in > 0) {
            const size_t lds = sizeof(float) * 2 * (size_t)I + sizeof(uint32_t) * STATE_WORDS;
            const Psk31TxTab t = p->tab();
            hipLaunchKernelGGL(k_psk31tx_shape, dim3((unsigned)(n_tiles * p->n_ch)), dim3(SHAPE_THREADS), lds, c->stream, I, (2 * SHAPE_THREADS) / I, (2 * SHAPE_THREADS) % I,
                               p->sym0, p->sym1, t.rate, t.rate1m, p->d_bits.get(), p->bits_pitch, p->d_prev.get(), counts, (int)n_tiles, (float2 *)out, out_pitch);
        }
        p->last_kernel = "k_psk31tx_plan+k_psk31tx_shape";
    } else {
        hipLaunchKernelGGL(k_psk31tx_generic, dim3(cdiv(p->n_ch, 64)), dim3(64), 0, c->stream, p->cfg, p->tab(), p->d_st.get(), p->n_ch, in, n_in, in_counts, in_pitch,
                           out, out_pitch, counts);
        p->last_kernel = "k_psk31tx_generic";
    }
    CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_psk31tx_force_generic(csdr_amd_psk31tx *p, int on) { return bank_force_generic(p, "psk31tx", on); }
const char *csdr_amd_psk31tx_kernel_name(const csdr_amd_psk31tx *p) { return bank_kernel_name(p); }

void csdr_amd_psk31tx_destroy(csdr_amd_psk31tx *p) { destroy_on_stream(p); }

// the host's tables of an object with these parameters: sym (256 complexf) and rate (interpolation floats); either may be NULL
int csdr_amd_psk31tx_tables(int n_psk, int interpolation, csdr_complexf *sym, float *rate)
{
    if (check_cfg(n_psk, interpolation, PSK31TX_VARICODE, PSK31TX_SHAPE) < 0) return -3;
    const HostTab h(n_psk, interpolation);
    if (sym) memcpy(sym, h.sym, sizeof h.sym);
    if (rate) memcpy(rate, h.rate.data(), sizeof(float) * (size_t)interpolation);
    return 0;
}

// differential_codec's decode branch (libcsdr.c:1830-1835) over n_streams streams: out = in == previous in, the previous byte carried in state_io
int csdr_amd_differential_decoder_u8_u8(csdr_amd_ctx *c, const unsigned char *in, unsigned char *out, int n_streams, long long n, size_t in_pitch, size_t out_pitch,
                                        unsigned char *state_io)
{
    if (!c || n_streams < 1 || n_streams > 65535 || !state_io) return fail_msg(-3, "differential_decoder_u8_u8: need a context, 1 <= n_streams <= 65535 and state_io");
    if (n < 0 || (n > 0 && (!in || !out || in == out || in_pitch < (size_t)n || out_pitch < (size_t)n)))
        return fail_msg(-3, "differential_decoder_u8_u8: need pitches >= n >= 0 and out apart from in");
    if (!n) return 0;
    const unsigned blocks = (unsigned)std::min<long long>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_differential_decoder, dim3(blocks, n_streams), dim3(256), 0, c->stream, in, out, n, in_pitch, out_pitch, state_io);
    hipLaunchKernelGGL(k_differential_decoder_state, dim3(cdiv(n_streams, 256)), dim3(256), 0, c->stream, in, n, in_pitch, state_io, n_streams);
    CSDR_LAUNCH_CHECK();
    return 0;
}

// duplicate_samples_ntimes_u8_u8 (libcsdr.c:1784-1791) over n_streams streams: the whole samples of n_bytes, each written ntimes
int csdr_amd_duplicate_samples_ntimes_u8_u8(csdr_amd_ctx *c, const unsigned char *in, unsigned char *out, int n_streams, long long n_bytes, size_t in_pitch,
                                            size_t out_pitch, int sample_size_bytes, int ntimes)
{
    if (!c || n_streams < 1 || n_streams > 65535) return fail_msg(-3, "duplicate_samples_ntimes_u8_u8: need a context and 1 <= n_streams <= 65535");
    if (sample_size_bytes <= 0) return fail_msg(-3, "duplicate_samples_ntimes_u8_u8: sample_size_bytes should be >0");
    if (ntimes <= 0) return fail_msg(-3, "duplicate_samples_ntimes_u8_u8: ntimes should be >0");
    if (n_bytes < 0) return fail_msg(-3, "duplicate_samples_ntimes_u8_u8: need n_bytes >= 0");
    const long long n_out = n_bytes / sample_size_bytes * sample_size_bytes * ntimes;
    if (n_out > 0 && (!in || !out || in_pitch < (size_t)n_bytes || out_pitch < (size_t)n_out))
        return fail_msg(-3, "duplicate_samples_ntimes_u8_u8: need in_pitch >= n_bytes and out_pitch >= n_bytes * ntimes");
    if (!n_out) return 0;
    const unsigned blocks = (unsigned)std::min<long long>((n_out + 255) / 256, 4096);
    hipLaunchKernelGGL(k_duplicate_samples, dim3(blocks, n_streams), dim3(256), 0, c->stream, in, out, n_out, in_pitch, out_pitch, sample_size_bytes, ntimes);
    CSDR_LAUNCH_CHECK();
    return 0;
}

// CPU run of k_psk31tx_generic's walk for one channel, the n items cut into calls of cuts[0], cuts[1], ... items (the rest in one more call).
// Outputs of all calls are concatenated; state_io (may be NULL: a fresh channel) carries the channel state in and out.  Returns the output count.
long long csdr_amd_debug_psk31tx_walk(int n_psk, int interpolation, int first_stage, int last_stage, const void *in, long long n, const long long *cuts, int n_cuts,
                                      void *out, csdr_amd_psk31tx_chan *state_io)
{
    if (check_cfg(n_psk, interpolation, first_stage, last_stage) < 0) return -3;
    if (n < 0 || (n > 0 && (!in || !out)) || n_cuts < 0 || (n_cuts && !cuts)) return fail_msg(-3, "debug_psk31tx_walk: bad arguments");
    const HostTab h(n_psk, interpolation);
    const Psk31TxCfg cfg{first_stage, last_stage, interpolation};
    const Psk31TxTab t = h.tab();
    Psk31TxChan s = FRESH;
    if (state_io) { s.diff_state = state_io->diff_state; s.last_i = state_io->last_i; s.last_q = state_io->last_q; }
    const size_t isz = first_stage == PSK31TX_SHAPE ? sizeof(float2) : 1, osz = last_stage >= PSK31TX_MOD ? sizeof(float2) : 1;
    long long k = 0;
    for_each_call(n, cuts, n_cuts, [&](long long done, long long m) {
        const char *x = (const char *)in + done * isz;
        char *y = (char *)out + k * osz;
        k += psk31tx_walk(cfg, s, t, (const uint8_t *)x, (const float2 *)x, m, (uint8_t *)y, (float2 *)y);
    });
    if (state_io) { state_io->diff_state = s.diff_state; state_io->last_i = s.last_i; state_io->last_q = s.last_q; }
    return k;
}

} // extern "C"
