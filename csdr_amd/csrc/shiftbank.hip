// shiftbank.hip -- the frequency shifters for n_streams streams with a rate and a phase PER STREAM (MI355X / gfx950): shift_addition_cc / _fc
// (libcsdr_gpl.c:27-79), shift_math_cc (libcsdr.c:186-207), shift_table_cc (libcsdr.c:229-265) as one object whose state stays on the device.
//
// shift.hip serves one rate per call: a generator writes that rate's rotator table to HBM and a mixing kernel multiplies every stream by it.  N clients on one
// wideband stream, each with its own retunable rate (csdr.c:881-923, ddcd_old.h:51-61), are N such calls, N host phase scans and N tables.  Here a stream's
// rotator never leaves the registers:
//   k_shiftbank_open      ADDITION's pre-pass, one lane per stream: applies a pending retune, steps the chunk start phases of the call (seeds.hpp's plan: no
//                         wrap-loop iterations) into cph[stream][0 .. n / chunk + 1] and leaves the record at the call's end.
//   k_shiftbank_addition  one lane owns one (stream, chunk) and walks its phasor recurrence.  A one-wave workgroup stages 32 samples of each of its 64 chunks
//                         through LDS: coalesced 256-byte runs in (the next tile's loads in flight during the walk), each lane steps through its own row, the
//                         tile goes out coalesced.  The call's partial first chunk (pos, c, s of the record) and partial last chunk are ordinary lanes.
//   k_shiftbank_scan      MATH / TABLE: one lane per stream walks the call's n phase steps and keeps every SB_TILE-th value (4 B per 64 samples).  The scan of the
//                         NEXT call runs on a side stream from this call's end phases as soon as this call's scan is known (ShiftAheadSlot's idea on the device).
//   k_shiftbank_math / _table   a lane replays at most SB_TILE - 1 steps from its tile's phase and mixes two samples per 16-byte access in the same pass.
//   k_shiftbank_generic   the plain form: one lane per (stream, chunk) or (stream, tile) on global memory, sample by sample; any alignment, any chunk.
// All of them, and the CPU walk, run shiftbank_dev.hpp's step functions: the same bits for every kernel and every cut into calls.
#include "bank.hpp"
#include "shiftbank_dev.hpp"
#include <string.h>
#include <algorithm>
#include <vector>

using namespace csdr_amd;

namespace {

static_assert(sizeof(ShiftbankChan) == sizeof(csdr_amd_shiftbank_chan), "ShiftbankChan mirrors csdr_amd_shiftbank_chan");

struct SbCall { float c0, s0; int pos0, pad; };          // ADDITION: a stream's open chunk at the call's first sample

struct SbArgs {
    ShiftbankChan *st; const float2 *par;                // par[stream] = (sindelta, cosdelta) of the stream's rate (host libm, libcsdr_gpl.c:85-86)
    int n_streams, chunk;
    const void *in; size_t in_pitch; cf32 *out; size_t out_pitch; long long n;
    const float *cph; size_t cph_pitch; const SbCall *call;                   // ADDITION
    const float *tiles; size_t tiles_pitch; const float *endph, *incs;        // MATH / TABLE
    const float *table; int size;                                             // TABLE
};

__global__ void k_shiftbank_set_rate(ShiftbankChan *st, float2 *par, int stream, float rate, float sd, float cd)
{
    st[stream].rate = rate; st[stream].pending = 1;
    par[stream] = make_float2(sd, cd);
}

__global__ __launch_bounds__(256) void k_shiftbank_quarter(float *__restrict__ table, int size)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < size) table[k] = sb_quarter_entry(k, size);
}

// ---- ADDITION
__global__ __launch_bounds__(64) void k_shiftbank_open(ShiftbankChan *__restrict__ st, SbCall *__restrict__ call, float *__restrict__ cph, size_t cph_pitch,
                                                       int n_streams, int chunk, long long n)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_streams) return;
    ShiftbankChan t = st[s];
    sb_open_call_addition(t);
    call[s] = SbCall{t.c, t.s, t.pos, 0};
    ChunkStepper cs; sb_stepper_init(cs, t.rate, chunk);
    float *row = cph + (size_t)s * cph_pitch;
    const long long total = (long long)t.pos + n, K = total / chunk;          // K <= (chunk - 1 + n) / chunk < cph_pitch
    float p = t.phase;
    row[0] = p;
    for (long long k = 1; k <= K; k++) { p = sb_next_chunk_phase(cs, p); row[k] = p; }
    t.phase = p; t.pos = (int)(total - K * chunk);
    st[s] = t;                                           // (c, s: the lane that mixes the call's last sample writes them)
}

// what lane g of the data kernels owns: chunk k of the call for stream s = samples [start, start + len) of the call
struct SbSpan { int s; long long start; int len; Phasor r; float2 d; };
__device__ __forceinline__ SbSpan sb_span(const SbArgs &a, long long g, int nck)
{
    SbSpan sp; sp.s = (int)(g / nck); sp.start = 0; sp.len = 0; sp.r = Phasor{1.f, 0.f}; sp.d = make_float2(0.f, 0.f);
    if (sp.s >= a.n_streams) return sp;
    const int k = (int)(g - (long long)sp.s * nck);
    const SbCall cl = a.call[sp.s];
    sp.start = k ? (long long)k * a.chunk - cl.pos0 : 0;
    if (sp.start >= a.n) return sp;
    sp.len = (int)min((long long)(a.chunk - (k ? 0 : cl.pos0)), a.n - sp.start);
    sp.r = (k == 0 && cl.pos0 > 0) ? Phasor{cl.c0, cl.s0} : sb_chunk_start(a.cph[(size_t)sp.s * a.cph_pitch + k]);
    sp.d = a.par[sp.s];
    return sp;
}

constexpr int ST = 32;                                   // samples per row and tile: 256-byte runs in, 256-byte runs out
constexpr int STP = ST + 1;                              // odd row stride in float2: the walking lanes' same-column accesses fall in different banks

template <bool REAL>
__global__ __launch_bounds__(64) void k_shiftbank_addition(SbArgs a, int nck)
{
    __shared__ float2 tile[64 * STP];
    __shared__ long long rin[64], rout[64];
    __shared__ int rlen[64];
    const int lane = threadIdx.x;
    const SbSpan sp = sb_span(a, (long long)blockIdx.x * 64 + lane, nck);
    rin[lane] = (long long)sp.s * (long long)a.in_pitch + sp.start;
    rout[lane] = (long long)sp.s * (long long)a.out_pitch + sp.start;
    rlen[lane] = sp.len;
    __syncthreads();
    const float2 *in2 = (const float2 *)a.in; const float *in1 = (const float *)a.in;
    float2 *out2 = (float2 *)a.out;
    const int half = lane >> 5, col = lane & 31, me = lane * STP;
    Phasor r = sp.r;

    float2 nx[ST];                                       // the next tile: load i holds column `col` of rows 2 i and 2 i + 1 (one per half wave)
    auto fetch = [&](int t0) {
#pragma unroll
        for (int i = 0; i < ST; i++) {
            const int rr = 2 * i + half, j = t0 + col;
            float2 v = make_float2(0.f, 0.f);
            if (j < rlen[rr]) { if (REAL) v.x = in1[rin[rr] + j]; else v = in2[rin[rr] + j]; }
            nx[i] = v;
        }
    };
    fetch(0);
    for (int t0 = 0; __ballot(t0 < sp.len) != 0; t0 += ST) {
#pragma unroll
        for (int i = 0; i < ST; i++) tile[(2 * i + half) * STP + col] = nx[i];        // 1. stage
        __syncthreads();
        if (__ballot(t0 + ST < sp.len) != 0) fetch(t0 + ST);
        const int m = min(ST, sp.len - t0);                                          // 2. lane r walks row r
#pragma unroll 8
        for (int j = 0; j < m; j++) {
            const float2 x = tile[me + j];
            const cf32 y = REAL ? sb_mix_fc(r, x.x) : sb_mix_cc(r, cf32{x.x, x.y});
            tile[me + j] = make_float2(y.i, y.q);
            r = sb_phasor_step(r, sp.d.x, sp.d.y);
        }
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < ST; i++) {                                               // 3. write back
            const int rr = 2 * i + half, j = t0 + col;
            if (j < rlen[rr]) out2[rout[rr] + j] = tile[rr * STP + col];
        }
        __syncthreads();
    }
    if (sp.len > 0 && sp.start + sp.len == a.n) { a.st[sp.s].c = r.c; a.st[sp.s].s = r.s; }
}

// ---- MATH / TABLE
// start == nullptr: the call's own scan, from the records (and their rates, left in incs for the scans ahead and the data kernel); else from start[stream]
__global__ __launch_bounds__(64) void k_shiftbank_scan(const ShiftbankChan *__restrict__ st, const float *__restrict__ start, float *__restrict__ incs,
                                                       float *__restrict__ tiles, size_t tiles_pitch, float *__restrict__ endph, int n_streams, long long n)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_streams) return;
    float p, inc;
    if (start) { p = start[s]; inc = incs[s]; }
    else { p = st[s].phase; inc = sb_inc(st[s].rate); incs[s] = inc; }
    float *row = tiles + (size_t)s * tiles_pitch;
    for (long long t = 0; t * SB_TILE < n; t++) {
        row[t] = p;
        const int m = (int)min((long long)SB_TILE, n - t * SB_TILE);
        if (!sb_once_ok(p, inc)) { for (int j = 0; j < m; j++) p = sb_phase_step(p, inc); }      // (a rate beyond 1, or a start phase a caller set outside 0 .. 2 PI)
        else if (m == SB_TILE) {
#pragma unroll 16
            for (int j = 0; j < SB_TILE; j++) p = sb_phase_step_once(p, inc);
        } else for (int j = 0; j < m; j++) p = sb_phase_step_once(p, inc);
    }
    endph[s] = p;
}

__device__ __forceinline__ float sb_phase_of_sample(const float *__restrict__ row, long long k, float inc)
{
    float p = row[k / SB_TILE];
    const int steps = (int)(k % SB_TILE);
    if (sb_once_ok(p, inc)) { for (int j = 0; j < steps; j++) p = sb_phase_step_once(p, inc); }
    else for (int j = 0; j < steps; j++) p = sb_phase_step(p, inc);
    return p;
}
template <bool TABLE> __device__ __forceinline__ Phasor sb_rot(const SbArgs &a, float p) { return TABLE ? sb_rot_table(p, a.table, a.size) : sb_rot_math(p); }

// the record at the call's end (the phase the scan arrived at); one lane per stream does it
__device__ __forceinline__ void sb_close_phase_call(const SbArgs &a, int s)
{
    ShiftbankChan t = a.st[s];
    t.phase = a.endph[s]; t.c = 1.f; t.s = 0.f; t.pos = 0; t.pending = 0; t.old_rate = t.rate;
    a.st[s] = t;
}

template <bool TABLE, bool VEC>
__global__ __launch_bounds__(256) void k_shiftbank_phase(SbArgs a)
{
    const int s = blockIdx.y;
    const cf32 *src = (const cf32 *)a.in + (size_t)s * a.in_pitch;
    cf32 *dst = a.out + (size_t)s * a.out_pitch;
    const float *row = a.tiles + (size_t)s * a.tiles_pitch;
    const float inc = a.incs[s];
    const long long stride = (long long)gridDim.x * blockDim.x, first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (first == 0) sb_close_phase_call(a, s);
    if (VEC) {
        const long long npair = a.n / 2;
        for (long long v = first; v < npair; v += stride) {
            const float p0 = sb_phase_of_sample(row, 2 * v, inc), p1 = sb_phase_next(p0, inc);      // (2 v and 2 v + 1 share a tile)
            const Phasor r0 = sb_rot<TABLE>(a, p0), r1 = sb_rot<TABLE>(a, p1);
            const float4 x = reinterpret_cast<const float4 *>(src)[v];
            const cf32 y0 = sb_mix_cc(r0, cf32{x.x, x.y}), y1 = sb_mix_cc(r1, cf32{x.z, x.w});
            reinterpret_cast<float4 *>(dst)[v] = make_float4(y0.i, y0.q, y1.i, y1.q);
        }
        if ((a.n & 1) && first == 0) dst[a.n - 1] = sb_mix_cc(sb_rot<TABLE>(a, sb_phase_of_sample(row, a.n - 1, inc)), src[a.n - 1]);
    } else {
        for (long long k = first; k < a.n; k += stride) dst[k] = sb_mix_cc(sb_rot<TABLE>(a, sb_phase_of_sample(row, k, inc)), src[k]);
    }
}

// ---- every variant in the plain form: lane g owns chunk (ADDITION) or tile (MATH / TABLE) g % per_stream of stream g / per_stream
template <int VARIANT, bool REAL>
__global__ __launch_bounds__(64) void k_shiftbank_generic(SbArgs a, int per_stream)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (VARIANT == CSDR_SHIFT_ADDITION) {
        const SbSpan sp = sb_span(a, g, per_stream);
        if (sp.len <= 0) return;
        const size_t io = (size_t)sp.s * a.in_pitch + sp.start, oo = (size_t)sp.s * a.out_pitch + sp.start;
        Phasor r = sp.r;
        for (int j = 0; j < sp.len; j++) {
            a.out[oo + j] = REAL ? sb_mix_fc(r, ((const float *)a.in)[io + j]) : sb_mix_cc(r, ((const cf32 *)a.in)[io + j]);
            r = sb_phasor_step(r, sp.d.x, sp.d.y);
        }
        if (sp.start + sp.len == a.n) { a.st[sp.s].c = r.c; a.st[sp.s].s = r.s; }
    } else {
        const int s = (int)(g / per_stream);
        if (s >= a.n_streams) return;
        const long long k0 = (g - (long long)s * per_stream) * SB_TILE;
        if (k0 == 0) sb_close_phase_call(a, s);
        if (k0 >= a.n) return;
        const int len = (int)min((long long)SB_TILE, a.n - k0);
        const cf32 *src = (const cf32 *)a.in + (size_t)s * a.in_pitch + k0;
        cf32 *dst = a.out + (size_t)s * a.out_pitch + k0;
        const float inc = a.incs[s];
        float p = a.tiles[(size_t)s * a.tiles_pitch + k0 / SB_TILE];
        for (int j = 0; j < len; j++) {
            dst[j] = sb_mix_cc(sb_rot<VARIANT == CSDR_SHIFT_TABLE>(a, p), src[j]);
            p = sb_phase_next(p, inc);
        }
    }
}

float2 host_deltas(float rate)
{   // shift_addition_init, libcsdr_gpl.c:81-88 (the host's libm, like the reference and like csdr_amd_rotator_generate)
    const float inc = sb_inc(rate);
    return make_float2((float)sin((double)inc), (float)cos((double)inc));
}

ShiftbankChan fresh_chan(float rate) { return ShiftbankChan{rate, 0.f, 1.f, 0.f, 0, 0, rate, 0}; }

int check_variant(int variant, int chunk, int aux, int in_format)
{
    if (variant == CSDR_SHIFT_UNROLL || variant == CSDR_SHIFT_ADDFAST)
        return fail_msg(-3, "shiftbank: shift_unroll_cc and shift_addfast_cc keep one rate per call (csdr_amd_shift_cc); the bank has ADDITION, MATH and TABLE");
    if (variant != CSDR_SHIFT_ADDITION && variant != CSDR_SHIFT_MATH && variant != CSDR_SHIFT_TABLE) return fail_msg(-3, "shiftbank: unknown shifter variant %d", variant);
    if (in_format != CSDR_AMD_SHIFTBANK_IN_CF32 && in_format != CSDR_AMD_SHIFTBANK_IN_F32) return fail_msg(-3, "shiftbank: in_format is 0 (CF32) or 1 (F32)");
    if (in_format == CSDR_AMD_SHIFTBANK_IN_F32 && variant != CSDR_SHIFT_ADDITION) return fail_msg(-3, "shiftbank: real input (shift_addition_fc) goes with ADDITION only");
    if (variant == CSDR_SHIFT_ADDITION && (chunk < 1 || chunk > (1 << 24))) return fail_msg(-3, "shiftbank: chunk should be 1 .. 2^24");
    if (variant == CSDR_SHIFT_TABLE && (aux < 0 || aux > (1 << 24))) return fail_msg(-3, "shiftbank: the table size (aux) should be 0 (65536) .. 2^24");
    return 0;
}

int check_chan(const csdr_amd_shiftbank_chan *s, int variant, int chunk)
{
    if (!(fabsf(s->rate) <= 1024.f) || !(fabsf(s->old_rate) <= 1024.f) || !(fabsf(s->phase) <= 1024.f) || !(fabsf(s->c) <= 1024.f) || !(fabsf(s->s) <= 1024.f))
        return fail_msg(-3, "shiftbank: channel state should be finite, each of |rate|, |old_rate|, |phase|, |c|, |s| <= 1024");
    if (s->pos < 0 || s->pos >= (variant == CSDR_SHIFT_ADDITION ? chunk : 1)) return fail_msg(-3, "shiftbank: pos should be 0 .. chunk - 1 (0 for MATH and TABLE)");
    return 0;
}

} // namespace

struct csdr_amd_shiftbank : ChanBank<ShiftbankChan> {
    int variant = 0, chunk = 1024, size = 0, in_format = 0;
    size_t max_n = 0;
    std::vector<float> h_rate;                           // the rates as set_rate / set_channel left them (get_rate, reset)
    Stream side;                                         // MATH / TABLE: the scans ahead
    Event ev_main, ev_ahead;
    DevBuf<float2> d_par;
    DevBuf<SbCall> d_call;
    DevBuf<float> d_cph; size_t cph_pitch = 0;
    DevBuf<float> d_tiles[2], d_endph[2], d_incs, d_table; size_t tiles_pitch = 0;
    int cur = 0;                                         // the tile table of the last call
    bool ahead_queued = false, ahead_valid = false; size_t ahead_n = 0;     // a scan for a call of ahead_n samples into table cur ^ 1; valid until the state is touched
    long long hits = 0;
};

extern "C" {

csdr_amd_shiftbank *csdr_amd_shiftbank_create(csdr_amd_ctx *c, int variant, int n_streams, const float *rates, int chunk, int aux, int in_format, size_t max_samples_per_call)
{
    if (bank_create_check("shiftbank", c, n_streams, 65535, "n_streams") < 0 || check_variant(variant, chunk, aux, in_format) < 0) return nullptr;
    if (!rates) { fail_msg(-3, "shiftbank: null rates"); return nullptr; }
    for (int s = 0; s < n_streams; s++) if (!(fabsf(rates[s]) <= 1024.f)) { fail_msg(-3, "shiftbank: rate %d should be finite, |rate| <= 1024", s); return nullptr; }
    if (max_samples_per_call < 1 || max_samples_per_call > ((size_t)1 << 30)) { fail_msg(-3, "shiftbank: max_samples_per_call should be 1 .. 2^30"); return nullptr; }
    Owned<csdr_amd_shiftbank, csdr_amd_shiftbank_destroy> p(new csdr_amd_shiftbank());
    p->c = c; p->n_ch = n_streams; p->variant = variant; p->chunk = variant == CSDR_SHIFT_ADDITION ? chunk : 1; p->in_format = in_format; p->max_n = max_samples_per_call;
    p->size = variant == CSDR_SHIFT_TABLE ? (aux > 0 ? aux : 65536) : 0;      // csdr.c:731
    p->h_rate.assign(rates, rates + n_streams);
    bool ok = dev_alloc(p->d_st, sizeof(ShiftbankChan) * n_streams) == hipSuccess && dev_alloc(p->d_par, sizeof(float2) * n_streams) == hipSuccess;
    if (variant == CSDR_SHIFT_ADDITION) {
        p->cph_pitch = max_samples_per_call / chunk + 2;
        ok = ok && dev_alloc(p->d_call, sizeof(SbCall) * n_streams) == hipSuccess && dev_alloc(p->d_cph, sizeof(float) * p->cph_pitch * n_streams) == hipSuccess;
    } else {
        p->tiles_pitch = max_samples_per_call / SB_TILE + 1;
        for (int b = 0; b < 2; b++)
            ok = ok && dev_alloc(p->d_tiles[b], sizeof(float) * p->tiles_pitch * n_streams) == hipSuccess && dev_alloc(p->d_endph[b], sizeof(float) * n_streams) == hipSuccess;
        ok = ok && dev_alloc(p->d_incs, sizeof(float) * n_streams) == hipSuccess;
        if (p->size) ok = ok && dev_alloc(p->d_table, sizeof(float) * p->size) == hipSuccess;
        if (ok && (stream_create(p->side) != hipSuccess || event_create(p->ev_main, hipEventDisableTiming) != hipSuccess || event_create(p->ev_ahead, hipEventDisableTiming) != hipSuccess)) {
            fail_msg(-2, "shiftbank: cannot create the side stream"); return nullptr;
        }
    }
    if (!ok) { fail_msg(-2, "shiftbank: out of device memory"); return nullptr; }
    if (p->size) {
        hipLaunchKernelGGL(k_shiftbank_quarter, dim3(cdiv(p->size, 256)), dim3(256), 0, c->stream, p->d_table.get(), p->size);
        if (hipGetLastError() != hipSuccess) { fail_msg(-2, "shiftbank: table launch"); return nullptr; }
    }
    if (csdr_amd_shiftbank_reset(p.get()) < 0) return nullptr;
    return p.release();
}

// every stream back to the stream's start with its current rate; synchronises the context's stream
int csdr_amd_shiftbank_reset(csdr_amd_shiftbank *p)
{
    if (!p) return fail_msg(-3, "shiftbank: null object");
    std::vector<ShiftbankChan> h(p->n_ch); std::vector<float2> par(p->n_ch);
    for (int s = 0; s < p->n_ch; s++) { h[s] = fresh_chan(p->h_rate[s]); par[s] = host_deltas(p->h_rate[s]); }
    p->ahead_valid = false;
    if (const int rc = csdr_amd_h2d(p->c, p->d_st.get(), h.data(), sizeof(ShiftbankChan) * p->n_ch)) return rc;
    return csdr_amd_h2d(p->c, p->d_par.get(), par.data(), sizeof(float2) * p->n_ch);
}

int csdr_amd_shiftbank_reset_channel(csdr_amd_shiftbank *p, int ch)
{
    if (!p || ch < 0 || ch >= p->n_ch) return fail_msg(-3, "shiftbank: channel out of range");
    const csdr_amd_shiftbank_chan f{p->h_rate[ch], 0.f, 1.f, 0.f, 0, 0, p->h_rate[ch], 0};
    return csdr_amd_shiftbank_set_channel(p, ch, &f);
}

int csdr_amd_shiftbank_get_channel(csdr_amd_shiftbank *p, int ch, csdr_amd_shiftbank_chan *out) { return bank_get_channel(p, "shiftbank", ch, out); }

int csdr_amd_shiftbank_set_channel(csdr_amd_shiftbank *p, int ch, const csdr_amd_shiftbank_chan *s)
{
    const int rc = bank_set_channel(p, "shiftbank", ch, s, [&] { return check_chan(s, p->variant, p->chunk); });
    if (rc) return rc;
    p->h_rate[ch] = s->rate; p->ahead_valid = false;
    const float2 d = host_deltas(s->rate);
    return csdr_amd_h2d(p->c, p->d_par.get() + ch, &d, sizeof d);
}

int csdr_amd_shiftbank_set_rate(csdr_amd_shiftbank *p, int ch, float rate)
{
    if (!p || ch < 0 || ch >= p->n_ch) return fail_msg(-3, "shiftbank: stream out of range");
    if (!(fabsf(rate) <= 1024.f)) return fail_msg(-3, "shiftbank: rate should be finite, |rate| <= 1024");
    const float2 d = host_deltas(rate);
    hipLaunchKernelGGL(k_shiftbank_set_rate, dim3(1), dim3(1), 0, p->c->stream, p->d_st.get(), p->d_par.get(), ch, rate, d.x, d.y);
    CSDR_LAUNCH_CHECK();
    p->h_rate[ch] = rate; p->ahead_valid = false;
    return 0;
}

int csdr_amd_shiftbank_get_rate(csdr_amd_shiftbank *p, int ch, float *rate)
{
    if (!p || !rate || ch < 0 || ch >= p->n_ch) return fail_msg(-3, "shiftbank: stream out of range");
    *rate = p->h_rate[ch];
    return 0;
}

int csdr_amd_shiftbank_force_generic(csdr_amd_shiftbank *p, int on) { return bank_force_generic(p, "shiftbank", on); }
const char *csdr_amd_shiftbank_kernel_name(const csdr_amd_shiftbank *p) { return bank_kernel_name(p); }
long long csdr_amd_shiftbank_scans_ahead(csdr_amd_shiftbank *p) { return p ? p->hits : 0; }

void csdr_amd_shiftbank_destroy(csdr_amd_shiftbank *p)
{
    if (!p) return;
    (void)hipSetDevice(p->c->device);
    if (p->side) (void)hipStreamSynchronize(p->side.get());
    destroy_on_stream(p);
}

int csdr_amd_shiftbank_process(csdr_amd_shiftbank *p, const void *in, size_t in_pitch, csdr_complexf *out, size_t out_pitch, size_t n)
{
    if (!p) return fail_msg(-3, "shiftbank: null object");
    if (n > p->max_n) return fail_msg(-3, "shiftbank: n = %zu is more than max_samples_per_call = %zu", n, p->max_n);
    if (!n) return 0;
    if (!in || !out || (in_pitch && in_pitch < n) || out_pitch < n) return fail_msg(-3, "shiftbank: need in, out, in_pitch >= n (or 0: one shared row) and out_pitch >= n");
    const bool real = p->in_format == CSDR_AMD_SHIFTBANK_IN_F32;
    if (((uintptr_t)in & (real ? 3 : 7)) || ((uintptr_t)out & 7)) return fail_msg(-3, "shiftbank: rows should be aligned to their elements");
    hipStream_t st = p->c->stream;
    const int S = p->n_ch;
    SbArgs a{};
    a.st = p->d_st.get(); a.par = p->d_par.get(); a.n_streams = S; a.chunk = p->chunk;
    a.in = in; a.in_pitch = in_pitch; a.out = out; a.out_pitch = out_pitch; a.n = (long long)n;

    if (p->variant == CSDR_SHIFT_ADDITION) {
        a.cph = p->d_cph.get(); a.cph_pitch = p->cph_pitch; a.call = p->d_call.get();
        hipLaunchKernelGGL(k_shiftbank_open, dim3(cdiv(S, 64)), dim3(64), 0, st, p->d_st.get(), p->d_call.get(), p->d_cph.get(), p->cph_pitch, S, p->chunk, (long long)n);
        CSDR_LAUNCH_CHECK();
        const int nck = (int)((n + 2 * (size_t)p->chunk - 2) / p->chunk);            // the chunks a call can touch, whatever pos it starts at
        if ((size_t)S * nck / 64 >= 0x7fffffffu) return fail_msg(-3, "shiftbank: n_streams x chunks per call is beyond one launch");
        const dim3 grid(cdiv((size_t)S * nck, 64));
        if (!p->force_generic && p->chunk >= ST) {
            p->last_kernel = "k_shiftbank_addition";
            if (real) hipLaunchKernelGGL((k_shiftbank_addition<true>), grid, dim3(64), 0, st, a, nck);
            else      hipLaunchKernelGGL((k_shiftbank_addition<false>), grid, dim3(64), 0, st, a, nck);
        } else {
            p->last_kernel = "k_shiftbank_generic";
            if (real) hipLaunchKernelGGL((k_shiftbank_generic<CSDR_SHIFT_ADDITION, true>), grid, dim3(64), 0, st, a, nck);
            else      hipLaunchKernelGGL((k_shiftbank_generic<CSDR_SHIFT_ADDITION, false>), grid, dim3(64), 0, st, a, nck);
        }
        CSDR_LAUNCH_CHECK();
        return 0;
    }

    // MATH / TABLE.  The scan queued ahead (if any) wrote table cur ^ 1 on the side stream: the context's stream waits for it either way, so that the buffers
    // this call writes are free.
    if (p->ahead_queued) { CSDR_HIP(hipStreamWaitEvent(st, p->ev_ahead.get(), 0)); p->ahead_queued = false; }
    if (p->ahead_valid && p->ahead_n == n) { p->cur ^= 1; p->hits++; }
    else {
        hipLaunchKernelGGL(k_shiftbank_scan, dim3(cdiv(S, 64)), dim3(64), 0, st, p->d_st.get(), (const float *)nullptr, p->d_incs.get(),
                           p->d_tiles[p->cur].get(), p->tiles_pitch, p->d_endph[p->cur].get(), S, (long long)n);
        CSDR_LAUNCH_CHECK();
    }
    // the next call's scan, from this call's end phases: behind everything the context's stream holds so far (this call's scan; the data kernel that read the
    // other table last)
    CSDR_HIP(hipEventRecord(p->ev_main.get(), st));
    CSDR_HIP(hipStreamWaitEvent(p->side.get(), p->ev_main.get(), 0));
    hipLaunchKernelGGL(k_shiftbank_scan, dim3(cdiv(S, 64)), dim3(64), 0, p->side.get(), p->d_st.get(), (const float *)p->d_endph[p->cur].get(), p->d_incs.get(),
                       p->d_tiles[p->cur ^ 1].get(), p->tiles_pitch, p->d_endph[p->cur ^ 1].get(), S, (long long)n);
    CSDR_LAUNCH_CHECK();
    CSDR_HIP(hipEventRecord(p->ev_ahead.get(), p->side.get()));
    p->ahead_queued = true; p->ahead_valid = true; p->ahead_n = n;

    a.tiles = p->d_tiles[p->cur].get(); a.tiles_pitch = p->tiles_pitch; a.endph = p->d_endph[p->cur].get(); a.incs = p->d_incs.get();
    a.table = p->d_table.get(); a.size = p->size;
    const bool table = p->variant == CSDR_SHIFT_TABLE;
    if (p->force_generic) {
        p->last_kernel = "k_shiftbank_generic";
        const int per = (int)cdiv(n, SB_TILE);
        if ((size_t)S * per / 64 >= 0x7fffffffu) return fail_msg(-3, "shiftbank: n_streams x tiles per call is beyond one launch");
        const dim3 grid(cdiv((size_t)S * per, 64));
        if (table) hipLaunchKernelGGL((k_shiftbank_generic<CSDR_SHIFT_TABLE, false>), grid, dim3(64), 0, st, a, per);
        else       hipLaunchKernelGGL((k_shiftbank_generic<CSDR_SHIFT_MATH, false>), grid, dim3(64), 0, st, a, per);
    } else {
        p->last_kernel = table ? "k_shiftbank_table" : "k_shiftbank_math";
        const bool vec = !(((uintptr_t)in | (uintptr_t)out) & 15) && !(in_pitch & 1) && !(out_pitch & 1);
        const size_t per_lane = vec ? 2 : 1;
        const dim3 grid(std::max(1u, cdiv(n / per_lane, 256)), (unsigned)S);
        if (table) { if (vec) hipLaunchKernelGGL((k_shiftbank_phase<true, true>), grid, dim3(256), 0, st, a); else hipLaunchKernelGGL((k_shiftbank_phase<true, false>), grid, dim3(256), 0, st, a); }
        else       { if (vec) hipLaunchKernelGGL((k_shiftbank_phase<false, true>), grid, dim3(256), 0, st, a); else hipLaunchKernelGGL((k_shiftbank_phase<false, false>), grid, dim3(256), 0, st, a); }
    }
    CSDR_LAUNCH_CHECK();
    return 0;
}

long long csdr_amd_debug_shiftbank_walk(int variant, float rate, int chunk, int aux, int in_format, const void *in, long long n, const long long *cuts, int n_cuts,
                                        const float *call_rates, csdr_complexf *out, csdr_amd_shiftbank_chan *state_io)
{
    if (check_variant(variant, chunk, aux, in_format) < 0) return -3;
    if (n < 0 || (n > 0 && (!in || !out)) || n_cuts < 0 || (n_cuts && !cuts)) return fail_msg(-3, "debug_shiftbank_walk: bad arguments");
    if (variant != CSDR_SHIFT_ADDITION) chunk = 1;
    ShiftbankChan s = fresh_chan(rate);
    if (state_io) { if (check_chan(state_io, variant, chunk) < 0) return -3; memcpy(&s, state_io, sizeof s); }
    const bool real = in_format == CSDR_AMD_SHIFTBANK_IN_F32;
    const int size = variant == CSDR_SHIFT_TABLE ? (aux > 0 ? aux : 65536) : 0;
    std::vector<float> table(size);
    for (int k = 0; k < size; k++) table[k] = sb_quarter_entry(k, size);
    int call = 0;
    for_each_call(n, cuts, n_cuts, [&](long long done, long long m) {
        const float nr = call_rates ? call_rates[call] : NAN;
        call++;
        if (!isnan(nr)) { s.rate = nr; s.pending = 1; }                      // set_rate in front of the call
        if (!m) return;
        if (variant == CSDR_SHIFT_ADDITION) {
            sb_open_call_addition(s);
            const float2 d = host_deltas(s.rate);
            ChunkStepper cs; sb_stepper_init(cs, s.rate, chunk);
            Phasor r{s.c, s.s};
            for (long long j = done; j < done + m; j++) {
                if (s.pos == 0) r = sb_chunk_start(s.phase);
                out[j] = real ? sb_mix_fc(r, ((const float *)in)[j]) : sb_mix_cc(r, ((const cf32 *)in)[j]);
                r = sb_phasor_step(r, d.x, d.y);
                if (++s.pos == chunk) { s.phase = sb_next_chunk_phase(cs, s.phase); s.pos = 0; }
            }
            s.c = r.c; s.s = r.s;
        } else {
            const float inc = sb_inc(s.rate);
            float p = s.phase;
            for (long long j = done; j < done + m; j++) {
                const Phasor r = size ? sb_rot_table(p, table.data(), size) : sb_rot_math(p);
                out[j] = sb_mix_cc(r, ((const cf32 *)in)[j]);
                p = sb_phase_next(p, inc);
            }
            s.phase = p; s.c = 1.f; s.s = 0.f; s.pos = 0; s.pending = 0; s.old_rate = s.rate;
        }
    });
    if (state_io) memcpy(state_io, &s, sizeof s);
    return n;
}

void csdr_amd_debug_shiftbank_chunk_phases(float rate, float phase, int chunk, int n, float *out)
{
    ChunkStepper cs; sb_stepper_init(cs, rate, chunk);
    for (int k = 0; k < n; k++) { phase = sb_next_chunk_phase(cs, phase); out[k] = phase; }
}

} // extern "C"
