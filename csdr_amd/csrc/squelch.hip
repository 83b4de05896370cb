// squelch.hip -- squelch_and_smeter_cc (csdr.c:2192-2243) and get_power_c / get_power_f (libcsdr.c:1144-1162) for n_channels channels per call (MI355X / gfx950).
//
// The stream of a channel is cut into blocks of B samples counted from its start.  A block's power has to be known before its first output byte, so a block is
// read completely first; the one-pass kernels keep it in registers between the read and the write, every input byte is fetched once and every output byte
// written once (8 + 8 bytes per sample, the operator's own traffic):
//   k_squelch_wave<R>   one wave per block, B <= 128 R samples (R = 4, 16: B <= 512, 2048): R float4 per lane, no barrier, the tree by lane shifts
//   k_squelch_wg<R>     one workgroup of 256 per block, B <= 512 R samples (R = 8, 16, 32: B <= 4096, 8192, 16384): R float4 per thread, the 512 chains
//                       meet in 2 KiB of LDS behind one barrier and every wave finishes the tree for itself
//   k_squelch_generic   two passes over global memory, any B, any pitch or alignment, blocks that begin in the samples held from earlier calls
// All of them evaluate squelch_dev.hpp's order (512 chains by sample index, then the tree): the same bits.  16-byte loads and stores in the one-pass kernels,
// zeros included.  What is left of a channel behind its last whole block (< B samples) stays in the object (k_squelch_carry).
#include "bank.hpp"
#include "squelch_dev.hpp"
#include <string.h>
#include <algorithm>
#include <vector>

using namespace csdr_amd;

namespace {

struct SqArgs {
    const float2 *in; size_t in_pitch; long long n_in;
    float2 *out; size_t out_pitch;
    float *power; uint8_t *flags; size_t power_pitch;
    const float *lv;                 // n_ch levels of the blocks this call starts, then n_ch levels of the blocks that earlier calls started
    const float2 *carry;             // [n_ch][B]: the held samples (generic kernel)
    const int *rem;                  // per-channel held counts, or null: rem0 for all
    int rem0, n_ch, B, d, nb;        // nb: the most blocks of any channel in this call
};

__device__ __forceinline__ void add_pair(float (&acc)[2], const float4 &v, int s, int d, float fB)
{
    if (d == 1) { acc[0] = acc[0] + squelch_term_c(v.x, v.y, fB); acc[1] = acc[1] + squelch_term_c(v.z, v.w, fB); return; }
    if (s % d == 0) acc[0] = acc[0] + squelch_term_c(v.x, v.y, fB);
    if ((s + 1) % d == 0) acc[1] = acc[1] + squelch_term_c(v.z, v.w, fB);
}

// one wave per block: lane l holds the samples 128 r + 2 l, + 1 of the rows r < R; needs rem == 0, B even, 16-byte aligned rows
template <int R> __global__ __launch_bounds__(256) void k_squelch_wave(SqArgs a)
{
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= (long long)a.n_ch * a.nb) return;
    const int ch = (int)(g / a.nb), k = (int)(g % a.nb), np = a.B / 2;
    const float4 *x = reinterpret_cast<const float4 *>(a.in + (size_t)ch * a.in_pitch + (size_t)k * a.B);
    float4 v[R];
#pragma unroll
    for (int r = 0; r < R; r++) { const int p = 64 * r + lane; v[r] = p < np ? x[p] : make_float4(0.f, 0.f, 0.f, 0.f); }
    float acc[4][2] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
    const float fB = (float)a.B;
#pragma unroll
    for (int r = 0; r < R; r++) { const int p = 64 * r + lane; if (p < np) add_pair(acc[r & 3], v[r], 2 * p, a.d, fB); }
    const float P = squelch_wave_tree(acc);
    const bool open = squelch_open(P, a.lv[ch]);
    float4 *y = reinterpret_cast<float4 *>(a.out + (size_t)ch * a.out_pitch + (size_t)k * a.B);
#pragma unroll
    for (int r = 0; r < R; r++) { const int p = 64 * r + lane; if (p < np) y[p] = open ? v[r] : make_float4(0.f, 0.f, 0.f, 0.f); }
    if (lane == 0) {
        if (a.power) a.power[(size_t)ch * a.power_pitch + k] = P;
        if (a.flags) a.flags[(size_t)ch * a.power_pitch + k] = open;
    }
}

// one workgroup per block: thread t holds the samples 512 r + 2 t, + 1 of the rows r < R; same preconditions as k_squelch_wave
template <int R> __global__ __launch_bounds__(256) void k_squelch_wg(SqArgs a)
{
    __shared__ float sh[SQ_CHAINS];
    const int t = threadIdx.x;
    const int ch = blockIdx.x / a.nb, k = blockIdx.x % a.nb, np = a.B / 2;
    const float4 *x = reinterpret_cast<const float4 *>(a.in + (size_t)ch * a.in_pitch + (size_t)k * a.B);
    float4 v[R];
#pragma unroll
    for (int r = 0; r < R; r++) { const int p = 256 * r + t; v[r] = p < np ? x[p] : make_float4(0.f, 0.f, 0.f, 0.f); }
    float acc[2] = {0.f, 0.f};
    const float fB = (float)a.B;
#pragma unroll
    for (int r = 0; r < R; r++) { const int p = 256 * r + t; if (p < np) add_pair(acc, v[r], 2 * p, a.d, fB); }
    const float P = squelch_wg_tree(acc, sh);
    const bool open = squelch_open(P, a.lv[ch]);
    float4 *y = reinterpret_cast<float4 *>(a.out + (size_t)ch * a.out_pitch + (size_t)k * a.B);
#pragma unroll
    for (int r = 0; r < R; r++) { const int p = 256 * r + t; if (p < np) y[p] = open ? v[r] : make_float4(0.f, 0.f, 0.f, 0.f); }
    if (t == 0) {
        if (a.power) a.power[(size_t)ch * a.power_pitch + k] = P;
        if (a.flags) a.flags[(size_t)ch * a.power_pitch + k] = open;
    }
}

// two passes, one workgroup per block; V = the channel's held samples then its input
__global__ __launch_bounds__(256) void k_squelch_generic(SqArgs a)
{
    __shared__ float sh[SQ_CHAINS];
    const int t = threadIdx.x;
    const int ch = blockIdx.x / a.nb, k = blockIdx.x % a.nb;
    const int rem = a.rem ? a.rem[ch] : a.rem0;
    if (k >= (rem + a.n_in) / a.B) return;                              // (the whole workgroup)
    const float2 *cr = a.carry + (size_t)ch * a.B, *x = a.in + (size_t)ch * a.in_pitch;
    const long long p0 = (long long)k * a.B;
    auto V = [&](long long p) { return p < rem ? cr[p] : x[p - rem]; };
    float acc[2] = {0.f, 0.f};
    const float fB = (float)a.B;
    for (int s0 = 2 * t; s0 < a.B; s0 += SQ_CHAINS)
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int s = s0 + e;
            if (s < a.B && s % a.d == 0) { const float2 u = V(p0 + s); acc[e] = acc[e] + squelch_term_c(u.x, u.y, fB); }
        }
    const float P = squelch_wg_tree(acc, sh);
    const bool open = squelch_open(P, a.lv[(k == 0 && rem > 0 ? a.n_ch : 0) + ch]);
    float2 *y = a.out + (size_t)ch * a.out_pitch + p0;
    for (int s = t; s < a.B; s += 256) y[s] = open ? V(p0 + s) : make_float2(0.f, 0.f);
    if (t == 0) {
        if (a.power) a.power[(size_t)ch * a.power_pitch + k] = P;
        if (a.flags) a.flags[(size_t)ch * a.power_pitch + k] = open;
    }
}

// behind the blocks: what is left of each channel (< B samples) moves to its row of `carry`.  With no whole block the input is appended to what is held;
// otherwise everything left lies in the input (the blocks have taken the held samples).
__global__ __launch_bounds__(256) void k_squelch_carry(const float2 *__restrict__ in, size_t in_pitch, long long n_in, float2 *__restrict__ carry, const int *__restrict__ remv,
                                                       int rem0, int B)
{
    const int ch = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const int rem = remv ? remv[ch] : rem0;
    const long long nb = (rem + n_in) / B, left = rem + n_in - nb * B;
    float2 *cr = carry + (size_t)ch * B;
    const float2 *x = in + (size_t)ch * in_pitch;
    if (nb == 0) { if (j < n_in) cr[rem + j] = x[j]; }
    else if (j < left) cr[j] = x[nb * B - rem + j];
}

__global__ void k_squelch_advance(int *__restrict__ rem, int n_ch, long long n_in, int B)
{
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch < n_ch) rem[ch] = (int)((rem[ch] + n_in) % B);
}

// get_power_c / get_power_f: one workgroup per (stream, block)
template <bool CPLX> __global__ __launch_bounds__(256) void k_get_power(const float *__restrict__ in, size_t in_pitch, int n_blocks, int B, int d, float *__restrict__ out)
{
    __shared__ float sh[SQ_CHAINS];
    const int t = threadIdx.x;
    const int st = blockIdx.x / n_blocks, k = blockIdx.x % n_blocks;
    const float *x = in + ((size_t)st * in_pitch + (size_t)k * B) * (CPLX ? 2 : 1);
    float acc[2] = {0.f, 0.f};
    const float fB = (float)B;
    for (int s0 = 2 * t; s0 < B; s0 += SQ_CHAINS)
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int s = s0 + e;
            if (s < B && s % d == 0) acc[e] = acc[e] + (CPLX ? squelch_term_c(x[2 * (size_t)s], x[2 * (size_t)s + 1], fB) : squelch_term_f(x[s], fB));
        }
    const float P = squelch_wg_tree(acc, sh);
    if (t == 0) out[(size_t)st * n_blocks + k] = P;
}

int get_power(csdr_amd_ctx *c, const void *in, int n_streams, int n_blocks, int B, int d, size_t in_pitch, float *out, bool cplx, const char *who)
{
    if (!c || n_streams < 1 || n_blocks < 0 || B < 1 || d < 1) return fail_msg(-3, "%s: need a context, n_streams >= 1, n_blocks >= 0, block_size >= 1, decimation >= 1", who);
    if (!n_blocks) return 0;
    if (!in || !out || in_pitch < (size_t)n_blocks * B) return fail_msg(-3, "%s: need in, power_out and in_pitch >= n_blocks * block_size", who);
    if ((long long)n_streams * n_blocks > 0x7fffffffLL) return fail_msg(-3, "%s: more than 2^31 - 1 blocks in one call", who);
    const dim3 grid((unsigned)((size_t)n_streams * n_blocks));
    if (cplx) hipLaunchKernelGGL(k_get_power<true>, grid, dim3(256), 0, c->stream, (const float *)in, in_pitch, n_blocks, B, d, out);
    else hipLaunchKernelGGL(k_get_power<false>, grid, dim3(256), 0, c->stream, (const float *)in, in_pitch, n_blocks, B, d, out);
    CSDR_LAUNCH_CHECK();
    return 0;
}

constexpr int SQ_ONE_PASS_MAX = 512 * 32;      // the largest block the registers of one workgroup hold (16384 samples, 128 KiB)
constexpr int SQ_WAVE_MAX = 128 * 16;          // the largest block of one wave

} // namespace

struct csdr_amd_squelch : Bank {
    int B, d; long long max_n; bool lv_dirty;
    std::vector<int> rem; std::vector<long long> blk; std::vector<float> lv, lv_started;
    bool uniform;                    // every channel holds rem[0] samples: the kernels need no per-channel counts
    DevBuf<float2> d_carry; DevBuf<float> d_lv; DevBuf<int> d_rem;
};

// common.hpp: the bank's state as csdr_amd_fmrx keeps it, for the calls it hands to this object
void *csdr_amd::squelch_adopt(csdr_amd_squelch *p, int held, long long block_index, const float *lv, const float *lv_started)
{
    const size_t bytes = sizeof(float) * p->n_ch;
    if (memcmp(p->lv.data(), lv, bytes) || memcmp(p->lv_started.data(), lv_started, bytes)) {
        p->lv.assign(lv, lv + p->n_ch); p->lv_started.assign(lv_started, lv_started + p->n_ch); p->lv_dirty = true;
    }
    p->rem.assign(p->n_ch, held); p->blk.assign(p->n_ch, block_index); p->uniform = true;
    return p->d_carry.get();
}

extern "C" {

csdr_amd_squelch *csdr_amd_squelch_create(csdr_amd_ctx *c, int n_channels, int block_size, int use_every_nth, const float *levels, long long max_samples_per_call)
{
    if (bank_create_check("squelch", c, n_channels) < 0) return nullptr;
    if (block_size < 1 || block_size > (1 << 24)) { fail_msg(-3, "squelch: block_size should be 1 .. 16777216"); return nullptr; }
    if (use_every_nth < 1) { fail_msg(-3, "squelch: use_every_nth <= 0 is invalid"); return nullptr; }
    if (max_samples_per_call < 1 || max_samples_per_call > (1LL << 30)) { fail_msg(-3, "squelch: max_samples_per_call should be 1 .. 2^30"); return nullptr; }
    Owned<csdr_amd_squelch, csdr_amd_squelch_destroy> p(new csdr_amd_squelch());
    p->c = c; p->n_ch = n_channels; p->B = block_size; p->d = use_every_nth; p->max_n = max_samples_per_call;
    p->lv.assign(n_channels, 0.f);
    if (levels) p->lv.assign(levels, levels + n_channels);
    if (dev_alloc(p->d_carry, sizeof(float2) * (size_t)block_size * n_channels) != hipSuccess || dev_alloc(p->d_lv, sizeof(float) * 2 * n_channels) != hipSuccess ||
        dev_alloc(p->d_rem, sizeof(int) * n_channels) != hipSuccess) { fail_msg(-2, "squelch: out of device memory"); return nullptr; }
    if (csdr_amd_squelch_reset(p.get()) < 0) return nullptr;
    return p.release();
}

// the held samples and the block count start over; the levels stay
int csdr_amd_squelch_reset(csdr_amd_squelch *p)
{
    if (!p) return fail_msg(-3, "squelch: null object");
    p->rem.assign(p->n_ch, 0); p->blk.assign(p->n_ch, 0); p->lv_started = p->lv; p->uniform = true; p->lv_dirty = true;
    return 0;
}

int csdr_amd_squelch_reset_channel(csdr_amd_squelch *p, int ch)
{
    if (!p || ch < 0 || ch >= p->n_ch) return fail_msg(-3, "squelch: channel out of range");
    p->rem[ch] = 0; p->blk[ch] = 0; p->lv_started[ch] = p->lv[ch]; p->lv_dirty = true;
    bool same = true;
    for (int k = 1; k < p->n_ch; k++) same = same && p->rem[k] == p->rem[0];
    if (!same && p->uniform) {                                          // from here on the kernels read the per-channel counts
        if (csdr_amd_ctx_sync(p->c) < 0) return -5;
        if (csdr_amd_h2d(p->c, p->d_rem.get(), p->rem.data(), sizeof(int) * p->n_ch) < 0) return -5;
    } else if (!p->uniform) {
        if (csdr_amd_ctx_sync(p->c) < 0) return -5;
        const int zero = 0;
        if (csdr_amd_h2d(p->c, p->d_rem.get() + ch, &zero, sizeof zero) < 0) return -5;
    }
    p->uniform = same;
    return 0;
}

int csdr_amd_squelch_set_level(csdr_amd_squelch *p, int ch, float level)
{
    if (!p || ch < -1 || ch >= p->n_ch) return fail_msg(-3, "squelch: channel out of range");
    for (int k = (ch < 0 ? 0 : ch); k < (ch < 0 ? p->n_ch : ch + 1); k++) {
        p->lv[k] = level;
        if (p->rem[k] == 0) p->lv_started[k] = level;
    }
    p->lv_dirty = true;
    return 0;
}

float csdr_amd_squelch_get_level(const csdr_amd_squelch *p, int ch) { return p && ch >= 0 && ch < p->n_ch ? p->lv[ch] : 0.f; }
long long csdr_amd_squelch_block_index(const csdr_amd_squelch *p, int ch) { return p && ch >= 0 && ch < p->n_ch ? p->blk[ch] : -1; }
int csdr_amd_squelch_max_blocks(const csdr_amd_squelch *p) { return p ? (int)((p->max_n + p->B - 1) / p->B) : 0; }
int csdr_amd_squelch_force_generic(csdr_amd_squelch *p, int on) { return bank_force_generic(p, "squelch", on); }
const char *csdr_amd_squelch_kernel_name(const csdr_amd_squelch *p) { return bank_kernel_name(p); }

void csdr_amd_squelch_destroy(csdr_amd_squelch *p) { destroy_on_stream(p); }

int csdr_amd_squelch_process(csdr_amd_squelch *p, const csdr_complexf *in, long long n_in, size_t in_pitch, csdr_complexf *out, size_t out_pitch, float *power,
                             size_t power_pitch, uint8_t *open_flags, int *n_blocks_out)
{
    if (!p) return fail_msg(-3, "squelch: null object");
    if (n_in < 0 || n_in > p->max_n) return fail_msg(-3, "squelch: n_in should be 0 .. max_samples_per_call (%lld)", p->max_n);
    if (n_in > 0 && (!in || in_pitch < (size_t)n_in)) return fail_msg(-3, "squelch: in_pitch below n_in");
    const int B = p->B, n_ch = p->n_ch;
    long long nbmax = 0;
    for (int k = 0; k < n_ch; k++) {
        const long long nb = (p->rem[k] + n_in) / B;
        nbmax = std::max(nbmax, nb);
        if (n_blocks_out) n_blocks_out[k] = (int)nb;
    }
    if (nbmax > 0 && (!out || out_pitch < (size_t)nbmax * B)) return fail_msg(-3, "squelch: out_pitch below the %lld samples of the complete blocks", nbmax * B);
    if (nbmax > 0 && (power || open_flags) && power_pitch < (size_t)nbmax) return fail_msg(-3, "squelch: power_pitch below the %lld complete blocks", nbmax);
    if (nbmax * n_ch > 0x7fffffffLL) return fail_msg(-3, "squelch: more than 2^31 - 1 blocks in one call");
    if (!n_in) return 0;
    csdr_amd_ctx *c = p->c;
    if (p->lv_dirty) {
        float *h = (float *)c->pinned_acquire(sizeof(float) * 2 * n_ch); if (!h) return -2;
        memcpy(h, p->lv.data(), sizeof(float) * n_ch); memcpy(h + n_ch, p->lv_started.data(), sizeof(float) * n_ch);
        const int rc = c->pinned_upload(p->d_lv.get(), sizeof(float) * 2 * n_ch); if (rc) return rc;
        p->lv_dirty = false;
    }
    SqArgs a;
    a.in = (const float2 *)in; a.in_pitch = in_pitch; a.n_in = n_in; a.out = (float2 *)out; a.out_pitch = out_pitch; a.power = power; a.flags = open_flags;
    a.power_pitch = power_pitch; a.lv = p->d_lv.get(); a.carry = p->d_carry.get(); a.rem = p->uniform ? nullptr : p->d_rem.get(); a.rem0 = p->rem[0];
    a.n_ch = n_ch; a.B = B; a.d = p->d; a.nb = (int)nbmax;
    if (nbmax > 0) {
        const bool aligned = !(((uintptr_t)in | (uintptr_t)out) & 15) && !((in_pitch | out_pitch | (size_t)B) & 1);
        const bool one_pass = !p->force_generic && p->uniform && p->rem[0] == 0 && aligned && B <= SQ_ONE_PASS_MAX;
        const unsigned blocks = (unsigned)(nbmax * n_ch);
        if (!one_pass) { hipLaunchKernelGGL(k_squelch_generic, dim3(blocks), dim3(256), 0, c->stream, a); p->last_kernel = "k_squelch_generic"; }
        else if (B <= 512) { hipLaunchKernelGGL(k_squelch_wave<4>, dim3(cdiv(blocks, 4)), dim3(256), 0, c->stream, a); p->last_kernel = "k_squelch_wave<4>"; }
        else if (B <= SQ_WAVE_MAX) { hipLaunchKernelGGL(k_squelch_wave<16>, dim3(cdiv(blocks, 4)), dim3(256), 0, c->stream, a); p->last_kernel = "k_squelch_wave<16>"; }
        else if (B <= 4096) { hipLaunchKernelGGL(k_squelch_wg<8>, dim3(blocks), dim3(256), 0, c->stream, a); p->last_kernel = "k_squelch_wg<8>"; }
        else if (B <= 8192) { hipLaunchKernelGGL(k_squelch_wg<16>, dim3(blocks), dim3(256), 0, c->stream, a); p->last_kernel = "k_squelch_wg<16>"; }
        else { hipLaunchKernelGGL(k_squelch_wg<32>, dim3(blocks), dim3(256), 0, c->stream, a); p->last_kernel = "k_squelch_wg<32>"; }
        CSDR_LAUNCH_CHECK();
    }
    // what is left of every channel
    bool any_left = !p->uniform;
    if (p->uniform) any_left = (p->rem[0] + n_in) % B != 0;
    if (any_left) {
        const long long most = std::min<long long>(n_in, B);
        hipLaunchKernelGGL(k_squelch_carry, dim3(cdiv((size_t)most, 256), n_ch), dim3(256), 0, c->stream, a.in, in_pitch, n_in, p->d_carry.get(), a.rem, a.rem0, B);
        CSDR_LAUNCH_CHECK();
    }
    if (!p->uniform) { hipLaunchKernelGGL(k_squelch_advance, dim3(cdiv(n_ch, 256)), dim3(256), 0, c->stream, p->d_rem.get(), n_ch, n_in, B); CSDR_LAUNCH_CHECK(); }
    for (int k = 0; k < n_ch; k++) {
        const long long tot = p->rem[k] + n_in, nb = tot / B;
        p->blk[k] += nb;
        p->rem[k] = (int)(tot % B);
        // a block that is still open behind this call's whole blocks was started by this call: its level is the one in force now
        if (nb > 0 && memcmp(&p->lv_started[k], &p->lv[k], sizeof(float))) { p->lv_started[k] = p->lv[k]; p->lv_dirty = true; }
    }
    return (int)nbmax;
}

int csdr_amd_get_power_c(csdr_amd_ctx *c, const csdr_complexf *in, int n_streams, int n_blocks, int block_size, int decimation, size_t in_pitch, float *power_out)
{
    return get_power(c, in, n_streams, n_blocks, block_size, decimation, in_pitch, power_out, true, "get_power_c");
}

int csdr_amd_get_power_f(csdr_amd_ctx *c, const float *in, int n_streams, int n_blocks, int block_size, int decimation, size_t in_pitch, float *power_out)
{
    return get_power(c, in, n_streams, n_blocks, block_size, decimation, in_pitch, power_out, false, "get_power_f");
}

int csdr_amd_squelch_report_due(int report_every_nth, long long block_index) { return squelch_report_due(report_every_nth, block_index) ? 1 : 0; }
int csdr_amd_squelch_gate_open(float power, float level) { return squelch_open(power, level) ? 1 : 0; }

// the step function on the host: the power of one block of block_size samples (complex: interleaved i, q)
float csdr_amd_debug_squelch_power(const float *in, int block_size, int decimation, int is_complex)
{
    if (!in || block_size < 1 || decimation < 1) { fail_msg(-3, "debug_squelch_power: need in, block_size >= 1, decimation >= 1"); return -1.f; }
    const float fB = (float)block_size;
    if (is_complex) return squelch_power_serial(block_size, decimation, [&](int s) { return squelch_term_c(in[2 * (size_t)s], in[2 * (size_t)s + 1], fB); });
    return squelch_power_serial(block_size, decimation, [&](int s) { return squelch_term_f(in[s], fB); });
}

} // extern "C"
