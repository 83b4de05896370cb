// compat.cpp -- the reference's own C API (include/libcsdr_amd_compat.h) on host pointers.
// Every function stages its block into device scratch, runs the batch API's kernels with n_streams = 1
// and copies the result back before returning.  The DSP runs on the device: if the device context cannot be
// created the process is terminated with the reason (there is no CPU fallback).  Host-side code here is limited
// to state bookkeeping, setup-time table generation and format plumbing around the copies.
#include "common.hpp"
#include "carrier_dev.hpp"
#include "modem_dev.hpp"
#include "noise_dev.hpp"
#include "../../include/libcsdr_amd_compat.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <unistd.h>
#include <sys/syscall.h>
#include <vector>

using namespace csdr_amd;

namespace {

// One device context PER HOST THREAD (own HIP stream, own scratch / staging buffers): the reference's functions are stateless and
// re-entrant (SURVEY.md section 8b "Threading"), so two threads may call any of them concurrently; with a context each they neither share
// staging buffers nor serialise on one stream.  A thread's context is destroyed when the thread ends; the main thread's lives until the
// process exits (the HIP runtime may already be unloading when its thread-local destructors run).
struct ThreadCtx {
    csdr_amd_ctx *c = nullptr;
    ~ThreadCtx() { if (c && (long)syscall(SYS_gettid) != (long)getpid()) csdr_amd_ctx_destroy(c); }
};
thread_local ThreadCtx t_ctx;

csdr_amd_ctx *ctx()
{
    if (t_ctx.c) return t_ctx.c;
    const char *dev = getenv("CSDR_AMD_DEVICE");
    t_ctx.c = csdr_amd_ctx_create(dev ? atoi(dev) : 0, nullptr);
    if (!t_ctx.c) { fprintf(stderr, "libcsdr_amd: cannot open the MI355X device: %s\n", csdr_amd_last_error()); abort(); }
    return t_ctx.c;
}

void die(const char *where, int rc)
{
    fprintf(stderr, "libcsdr_amd: %s failed (%d): %s\n", where, rc, csdr_amd_last_error());
    abort();
}
#define MUST(call) do { int rc__ = (call); if (rc__ < 0) die(#call, rc__); } while (0)

// staging buffers: slot 4 = input, 5 = output, 6 = aux, 7 = aux2
template <typename T> T *stage_in(int slot, const T *host, size_t n, size_t extra = 0)
{
    csdr_amd_ctx *c = ctx();
    T *d = (T *)c->get_scratch(slot, sizeof(T) * (n + extra) + 64);
    if (!d) die("scratch", -2);
    if (n) MUST(hipMemcpyAsync(d, host, sizeof(T) * n, hipMemcpyHostToDevice, c->stream) == hipSuccess ? 0 : -1);
    return d;
}
template <typename T> T *stage_out(int slot, size_t n)
{
    T *d = (T *)ctx()->get_scratch(slot, sizeof(T) * n + 64);
    if (!d) die("scratch", -2);
    return d;
}
template <typename T> void fetch(T *host, const T *dev, size_t n)
{
    csdr_amd_ctx *c = ctx();
    if (n) MUST(hipMemcpyAsync(host, dev, sizeof(T) * n, hipMemcpyDeviceToHost, c->stream) == hipSuccess ? 0 : -1);
    MUST(hipStreamSynchronize(c->stream) == hipSuccess ? 0 : -1);
}

float run_shifter(int variant, complexf *in, complexf *out, int n, float rate, float phase, int aux)
{
    if (n <= 0) return phase;
    csdr_amd_ctx *c = ctx();
    cf32 *din = stage_in<cf32>(4, (const cf32 *)in, n);
    cf32 *dout = stage_out<cf32>(5, n);
    MUST(csdr_amd_shift_cc(c, variant, rate, &phase, din, dout, 1, (size_t)n, (size_t)n, (size_t)n, n, aux));   // one library call = one chunk
    fetch((cf32 *)out, dout, n);
    return phase;
}

struct FftPlanImpl { int kind; int forward; };   // kind 0: c2c, 1: r2c, 2: c2r

// The device generators take the CLI's `rate` and form the per-sample increment (2*rate)*PI in float themselves.
// Callers of the library API hand over the increment; recover a rate that reproduces it bit for bit.
float rate_from_increment(float inc)
{
    const float guess = inc / (2 * PI_F);
    float cand[3] = { guess, nextafterf(guess, INFINITY), nextafterf(guess, -INFINITY) };
    for (float r : cand) if ((r * 2) * PI_F == inc) return r;
    return guess;
}

} // namespace

extern "C" {

// ------------------------------------------------------------------ design (host side, same code as the batch API)
void firdes_lowpass_f(float *output, int length, float cutoff_rate, window_t window) { csdr_amd_firdes_lowpass_f(output, length, cutoff_rate, (int)window); }
void firdes_bandpass_c(complexf *output, int length, float lowcut, float highcut, window_t window)
{ csdr_amd_firdes_bandpass_c((csdr_complexf *)output, length, lowcut, highcut, (int)window); }
float firdes_wkernel_blackman(float r) { r = (float)(0.5 + r / 2); return (float)(0.42 - 0.5 * cos((double)(2 * PI_F * r)) + 0.08 * cos((double)(4 * PI_F * r))); }  // libcsdr.c:76-82
float firdes_wkernel_hamming(float r) { r = (float)(0.5 + r / 2); return (float)(0.54 - 0.46 * cos((double)(2 * PI_F * r))); }                            // :84-90
float firdes_wkernel_boxcar(float) { return 1.0f; }                                                                                           // :93-96
window_t firdes_get_window_from_string(char *s)
{   // libcsdr.c:57-63
    if (!strcmp(s, "BOXCAR")) return WINDOW_BOXCAR;
    if (!strcmp(s, "BLACKMAN")) return WINDOW_BLACKMAN;
    if (!strcmp(s, "HAMMING")) return WINDOW_HAMMING;
    return WINDOW_DEFAULT;
}
char *firdes_get_string_from_window(window_t w)
{   // libcsdr.c:68-74
    return (char *)(w == WINDOW_BOXCAR ? "BOXCAR" : w == WINDOW_BLACKMAN ? "BLACKMAN" : w == WINDOW_HAMMING ? "HAMMING" : "INVALID");
}
int firdes_filter_len(float tbw) { return csdr_amd_firdes_filter_len(tbw); }
void normalize_fir_f(float *in, float *out, int length)
{   // libcsdr.c:117-125 (setup-time helper on a handful of taps)
    float sum = 0; for (int k = 0; k < length; k++) sum += in[k];
    for (int k = 0; k < length; k++) out[k] = in[k] / sum;
}
int log2n(int x) { return csdr_amd_log2n(x); }
int next_pow2(int x) { return csdr_amd_next_pow2(x); }
float fir_one_pass_ff(float *input, float *taps, int taps_length)
{   // libcsdr.c:675-680: a single dot product; served by the device FIR kernel with one output
    float *din = stage_in<float>(4, input, taps_length, 1), *dt = stage_in<float>(6, taps, taps_length);
    float *dout = stage_out<float>(5, 4);
    MUST(csdr_amd_fir_ff(ctx(), din, dout, 1, taps_length + 1, 0, 0, dt, taps_length));
    float r; fetch(&r, dout, 1); return r;
}

// ------------------------------------------------------------------ converters
#define CONVERT(name, IN_T, OUT_T, DIN_T, DOUT_T, in_count, out_count, call)                                   \
    void name(IN_T *input, OUT_T *output, int input_size) {                                                     \
        if (input_size <= 0) return;                                                                            \
        const size_t n = (size_t)input_size;                                                                    \
        DIN_T *din = stage_in<DIN_T>(4, (const DIN_T *)input, in_count);                                        \
        DOUT_T *dout = stage_out<DOUT_T>(5, out_count);                                                         \
        MUST(call(ctx(), din, dout, n));                                                                        \
        fetch((DOUT_T *)output, dout, out_count);                                                               \
    }
CONVERT(convert_u8_f, unsigned char, float, uint8_t, float, n, n, csdr_amd_convert_u8_f)
CONVERT(convert_s8_f, signed char, float, int8_t, float, n, n, csdr_amd_convert_s8_f)
CONVERT(convert_s16_f, short, float, int16_t, float, n, n, csdr_amd_convert_s16_f)
CONVERT(convert_f_u8, float, unsigned char, float, uint8_t, n, n, csdr_amd_convert_f_u8)
CONVERT(convert_f_s8, float, signed char, float, int8_t, n, n, csdr_amd_convert_f_s8)
CONVERT(convert_f_s16, float, short, float, int16_t, n, n, csdr_amd_convert_f_s16)
void convert_i16_f(short *i, float *o, int n) { convert_s16_f(i, o, n); }     // libcsdr.c:2400
void convert_f_i16(float *i, short *o, int n) { convert_f_s16(i, o, n); }     // libcsdr.c:2401
void convert_f_s24(float *input, unsigned char *output, int input_size, int bigendian)
{
    if (input_size <= 0) return;
    float *din = stage_in<float>(4, input, input_size); uint8_t *dout = stage_out<uint8_t>(5, 3 * (size_t)input_size + 16);
    MUST(csdr_amd_convert_f_s24(ctx(), din, dout, input_size, bigendian));
    fetch((uint8_t *)output, dout, 3 * (size_t)input_size);
}
void convert_s24_f(unsigned char *input, float *output, int input_size, int bigendian)
{
    if (input_size <= 0) return;
    uint8_t *din = stage_in<uint8_t>(4, input, 3 * (size_t)input_size, 16); float *dout = stage_out<float>(5, input_size);
    MUST(csdr_amd_convert_s24_f(ctx(), din, dout, input_size, bigendian));
    fetch(output, dout, input_size);
}

// ------------------------------------------------------------------ shifters
float shift_math_cc(complexf *in, complexf *out, int n, float rate, float phase) { return run_shifter(CSDR_SHIFT_MATH, in, out, n, rate, phase, 0); }

shift_table_data_t shift_table_init(int table_size)
{   // libcsdr.c:211-222; the device regenerates the same table, the host copy is kept for callers that read it
    shift_table_data_t t; t.table = (float *)malloc(sizeof(float) * table_size); t.table_size = table_size;
    for (int k = 0; k < table_size; k++) t.table[k] = (float)sin((double)(((float)k / table_size) * (PI_F / 2)));
    return t;
}
void shift_table_deinit(shift_table_data_t t) { free(t.table); }
float shift_table_cc(complexf *in, complexf *out, int n, float rate, shift_table_data_t t, float phase)
{ return run_shifter(CSDR_SHIFT_TABLE, in, out, n, rate, phase, t.table_size); }

shift_addfast_data_t shift_addfast_init(float rate)
{   // libcsdr.c:307-317
    shift_addfast_data_t d; d.phase_increment = 2 * rate * PI_F;
    for (int j = 0; j < 4; j++) { d.dsin[j] = (float)sin((double)(d.phase_increment * (j + 1))); d.dcos[j] = (float)cos((double)(d.phase_increment * (j + 1))); }
    return d;
}
float shift_addfast_cc(complexf *in, complexf *out, int n, shift_addfast_data_t *d, float phase)
{ return run_shifter(CSDR_SHIFT_ADDFAST, in, out, n, rate_from_increment(d->phase_increment), phase, 0); }

shift_unroll_data_t shift_unroll_init(float rate, int size)
{   // libcsdr.c:268-284
    shift_unroll_data_t d; d.phase_increment = 2 * rate * PI_F; d.size = size;
    d.dsin = (float *)malloc(sizeof(float) * size); d.dcos = (float *)malloc(sizeof(float) * size);
    float a = 0;
    for (int k = 0; k < size; k++) {
        a += d.phase_increment; while (a > PI_F) a -= 2 * PI_F; while (a < -PI_F) a += 2 * PI_F;
        d.dsin[k] = (float)sin((double)a); d.dcos[k] = (float)cos((double)a);
    }
    return d;
}
float shift_unroll_cc(complexf *in, complexf *out, int n, shift_unroll_data_t *d, float phase)
{ return run_shifter(CSDR_SHIFT_UNROLL, in, out, n, rate_from_increment(d->phase_increment), phase, d->size); }

shift_addition_data_t shift_addition_init(float rate)
{   // libcsdr_gpl.c:81-89
    rate *= 2; shift_addition_data_t o;
    o.sindelta = (float)sin((double)(rate * PI_F)); o.cosdelta = (float)cos((double)(rate * PI_F)); o.rate = rate;
    return o;
}
float shift_addition_cc(complexf *in, complexf *out, int n, shift_addition_data_t d, float phase)
{ return run_shifter(CSDR_SHIFT_ADDITION, in, out, n, d.rate / 2, phase, 0); }
float shift_addition_fc(float *in, complexf *out, int n, shift_addition_data_t d, float phase)
{
    if (n <= 0) return phase;
    csdr_amd_ctx *c = ctx();
    float *din = stage_in<float>(4, in, n); cf32 *dout = stage_out<cf32>(5, n);
    cf32 *rot = stage_out<cf32>(7, n);
    MUST(csdr_amd_rotator_generate(c, CSDR_SHIFT_ADDITION, d.rate / 2, &phase, rot, n, n, 0));
    MUST(csdr_amd_mix_fc(c, din, dout, rot, 1, n, n, n));
    fetch((cf32 *)out, dout, n);
    return phase;
}
shift_addition_data_t decimating_shift_addition_init(float rate, int decimation) { return shift_addition_init(rate * decimation); }
decimating_shift_addition_status_t decimating_shift_addition_cc(complexf *in, complexf *out, int n, shift_addition_data_t d, int decimation, decimating_shift_addition_status_t s)
{
    csdr_amd_ctx *c = ctx();
    cf32 *din = stage_in<cf32>(4, (const cf32 *)in, n); cf32 *dout = stage_out<cf32>(5, n / (decimation > 0 ? decimation : 1) + 2);
    shift_addition_data_t *dd = stage_in<shift_addition_data_t>(6, &d, 1);
    int32_t *dst = (int32_t *)stage_in<decimating_shift_addition_status_t>(7, &s, 1);
    MUST(csdr_amd_decimating_shift_addition_cc(c, din, dout, 1, n, n, n, dd, decimation, dst));
    fetch(&s, (decimating_shift_addition_status_t *)dst, 1);
    fetch((cf32 *)out, dout, s.output_size);
    return s;
}

// ------------------------------------------------------------------ filters / demod / audio
int fir_decimate_cc(complexf *in, complexf *out, int n, int decimation, float *taps, int taps_length)
{
    if (n < taps_length) return 0;
    cf32 *din = stage_in<cf32>(4, (const cf32 *)in, n); float *dt = stage_in<float>(6, taps, taps_length);
    cf32 *dout = stage_out<cf32>(5, n / decimation + 2);
    int produced = csdr_amd_fir_decimate_cc(ctx(), din, dout, 1, n, n, n / decimation + 2, decimation, dt, taps_length);
    if (produced < 0) die("fir_decimate_cc", produced);
    fetch((cf32 *)out, dout, produced);
    return produced;
}
int deemphasis_nfm_ff(float *in, float *out, int n, int sample_rate)
{
    const float *taps = nullptr; const int nt = csdr_amd_nfm_deemph_taps(sample_rate, &taps);
    if (!nt) return 0;                                                   // unsupported rate, libcsdr.c:1119
    if (n - nt <= 0) return (n - nt < 0) ? 0 : 0;
    float *din = stage_in<float>(4, in, n); float *dt = stage_in<float>(6, taps, nt); float *dout = stage_out<float>(5, n);
    int produced = csdr_amd_fir_ff(ctx(), din, dout, 1, n, n, n, dt, nt);
    if (produced < 0) die("deemphasis_nfm_ff", produced);
    fetch(out, dout, produced);
    return produced;
}
float deemphasis_wfm_ff(float *in, float *out, int n, float tau, int sample_rate, float last_output)
{
    if (n <= 0) return last_output;
    float *din = stage_in<float>(4, in, n); float *dout = stage_out<float>(5, n); float *dl = stage_in<float>(6, &last_output, 1);
    MUST(csdr_amd_deemphasis_wfm_ff(ctx(), din, dout, 1, n, n, n, tau, sample_rate, dl));
    fetch(out, dout, n);
    float l; fetch(&l, dl, 1); return l;
}
complexf fmdemod_quadri_cf(complexf *in, float *out, int n, float *temp, complexf last)
{
    (void)temp;                                                          // the reference's scratch (libcsdr.c:1042-1043) is not needed
    if (n <= 0) return last;
    cf32 *din = stage_in<cf32>(4, (const cf32 *)in, n); float *dout = stage_out<float>(5, n);
    cf32 *dl = stage_in<cf32>(6, (const cf32 *)&last, 1);
    MUST(csdr_amd_fmdemod_quadri_cf(ctx(), din, dout, 1, n, n, n, dl));
    fetch(out, dout, n);
    return in[n - 1];
}
complexf fmdemod_quadri_novect_cf(complexf *in, float *out, int n, complexf last) { return fmdemod_quadri_cf(in, out, n, nullptr, last); }
void limit_ff(float *in, float *out, int n, float m)
{
    if (n <= 0) return;
    float *din = stage_in<float>(4, in, n); float *dout = stage_out<float>(5, n);
    MUST(csdr_amd_limit_ff(ctx(), din, dout, n, m)); fetch(out, dout, n);
}
void gain_ff(float *in, float *out, int n, float g)
{
    if (n <= 0) return;
    float *din = stage_in<float>(4, in, n); float *dout = stage_out<float>(5, n);
    MUST(csdr_amd_gain_ff(ctx(), din, dout, n, g)); fetch(out, dout, n);
}
void fastagc_ff(fastagc_ff_t *st, float *output)
{   // libcsdr.c:946-991: device state layout [buffer_1 | buffer_2 | peak_1 peak_2 last_gain pad]
    const int n = st->input_size;
    if (n <= 0) return;
    std::vector<float> hs(2 * (size_t)n + 4);
    memcpy(hs.data(), st->buffer_1, sizeof(float) * n); memcpy(hs.data() + n, st->buffer_2, sizeof(float) * n);
    hs[2 * n] = st->peak_1; hs[2 * n + 1] = st->peak_2; hs[2 * n + 2] = st->last_gain; hs[2 * n + 3] = 0;
    float *dstate = stage_in<float>(6, hs.data(), hs.size());
    float *din = stage_in<float>(4, st->buffer_input, n); float *dout = stage_out<float>(5, n);
    MUST(csdr_amd_fastagc_ff(ctx(), din, dout, 1, 1, n, n, n, st->reference, dstate));
    fetch(output, dout, n);
    float tail[4]; fetch(tail, dstate + 2 * n, 4);
    float *recycled = st->buffer_1;                                      // pointer rotation, libcsdr.c:983-988
    st->buffer_1 = st->buffer_2; st->buffer_2 = st->buffer_input; st->buffer_input = recycled;
    st->peak_1 = tail[0]; st->peak_2 = tail[1]; st->last_gain = tail[2];
}

fractional_decimator_ff_t fractional_decimator_ff_init(float rate, int num_poly_points, float *taps, int taps_length)
{   // libcsdr.c:715-748 (host-side state block, same fields and allocations)
    fractional_decimator_ff_t d;
    d.num_poly_points = num_poly_points & ~1;
    d.poly_precalc_denomiator = (float *)malloc(d.num_poly_points * sizeof(float));
    d.xifirst = -(num_poly_points / 2) + 1; d.xilast = num_poly_points / 2;
    int id = 0;
    for (int a = d.xifirst; a <= d.xilast; a++, id++) {
        float prod = 1;
        for (int b = d.xifirst; b <= d.xilast; b++) if (a != b) prod *= (a - b);
        d.poly_precalc_denomiator[id] = prod;
    }
    d.where = -d.xifirst;
    d.coeffs_buf = (float *)malloc(d.num_poly_points * sizeof(float));
    d.filtered_buf = (float *)malloc(d.num_poly_points * sizeof(float));
    d.rate = rate; d.taps = taps; d.taps_length = taps_length; d.input_processed = 0; d.output_size = 0;
    return d;
}
void fractional_decimator_ff(float *in, float *out, int n, fractional_decimator_ff_t *d)
{
    csdr_amd_fracdec *fd = csdr_amd_fracdec_create(d->rate, d->num_poly_points, d->taps, d->taps ? d->taps_length : 0);
    if (!fd) die("fractional_decimator_ff", -3);
    csdr_amd_fracdec_set_where(fd, d->where);
    float *din = stage_in<float>(4, in, n); float *dout = stage_out<float>(5, n);
    int processed = 0;
    int produced = csdr_amd_fractional_decimator_ff(ctx(), fd, din, dout, 1, n, n, n, &processed);
    if (produced < 0) die("fractional_decimator_ff", produced);
    fetch(out, dout, produced);
    d->where = csdr_amd_fracdec_get_where(fd); d->input_processed = processed; d->output_size = produced;
    csdr_amd_fracdec_destroy(fd);
}

// ------------------------------------------------------------------ BPSK31 receive (psk31.hip)
void simple_agc_cc(complexf *in, complexf *out, int n, float rate, float reference, float max_gain, float *current_gain)
{   // libcsdr.c:2201-2217
    if (n <= 0) return;
    complexf *din = stage_in<complexf>(4, in, n); complexf *dout = stage_out<complexf>(5, n);
    float *dg = stage_in<float>(6, current_gain, 1);
    MUST(csdr_amd_simple_agc_cc(ctx(), (const csdr_complexf *)din, (csdr_complexf *)dout, 1, n, n, n, rate, reference, max_gain, dg));
    fetch(out, dout, n);
    fetch(current_gain, dg, 1);
}

timing_recovery_state_t timing_recovery_init(timing_recovery_algorithm_t algorithm, int decimation_rate, int use_q, float loop_gain, float max_error,
                                             int debug_every_nth, char *debug_writefiles_path)
{   // libcsdr.c:1955-1970
    timing_recovery_state_t t;
    memset(&t, 0, sizeof t);
    t.algorithm = algorithm; t.decimation_rate = decimation_rate; t.use_q = use_q; t.debug_phase = debug_every_nth; t.debug_every_nth = debug_every_nth;
    t.debug_writefiles_path = debug_writefiles_path; t.last_correction_offset = 0; t.earlylate_ratio = 0.25f; t.loop_gain = loop_gain; t.max_error = max_error;
    return t;
}

// One call = a fresh one-channel timing-only object whose correction_offset is the state's: it consumes up to the reference's input_processed and keeps the rest
void timing_recovery_cc(complexf *in, complexf *out, int n, float *timing_error, int *sampled_indexes, timing_recovery_state_t *state)
{   // libcsdr.c:1977-2075
    if (state->debug_every_nth >= 0) { fprintf(stderr, "libcsdr_amd: timing_recovery_cc: debug_every_nth >= 0 (Octave plots) is not supported\n"); abort(); }
    csdr_amd_psk31_params pr; memset(&pr, 0, sizeof pr);
    pr.algorithm = (int)state->algorithm; pr.decimation = state->decimation_rate; pr.loop_gain = state->loop_gain; pr.max_error = state->max_error; pr.use_q = state->use_q;
    // one object per thread, kept while the parameters stay the same: a client calls this once per buffer
    struct TrCache { csdr_amd_psk31 *p = nullptr; csdr_amd_psk31_params pr; ~TrCache() { if (p && (long)syscall(SYS_gettid) != (long)getpid()) csdr_amd_psk31_destroy(p); } };
    static thread_local TrCache cache;
    if (!cache.p || memcmp(&cache.pr, &pr, sizeof pr)) {
        if (cache.p) csdr_amd_psk31_destroy(cache.p);
        cache.p = csdr_amd_psk31_create(ctx(), &pr, 1, CSDR_AMD_PSK31_TIMING, CSDR_AMD_PSK31_TIMING);
        if (!cache.p) die("timing_recovery_cc", -3);
        cache.pr = pr;
    }
    csdr_amd_psk31 *p = cache.p;
    csdr_amd_psk31_chan st; memset(&st, 0, sizeof st);
    st.correction_offset = state->last_correction_offset;
    MUST(csdr_amd_psk31_set_channel(p, 0, &st));
    const long long mo = csdr_amd_psk31_max_out(p, n > 0 ? n : 0);
    complexf *din = stage_in<complexf>(4, in, n > 0 ? n : 0); complexf *dout = stage_out<complexf>(5, (size_t)mo);
    float *derr = stage_out<float>(6, (size_t)mo); unsigned *didx = stage_out<unsigned>(7, (size_t)mo + 16);
    int *dcnt = (int *)(didx + mo);
    MUST(csdr_amd_psk31_process(p, din, n > 0 ? n : 0, n > 0 ? n : 1, dout, (size_t)mo, dcnt, derr, didx));
    int k = 0; fetch(&k, dcnt, 1);
    MUST(csdr_amd_psk31_get_channel(p, 0, &st));
    if (k) {
        fetch(out, dout, (size_t)k);
        if (timing_error) fetch(timing_error, derr, (size_t)k);
        if (sampled_indexes) fetch((unsigned *)sampled_indexes, didx, (size_t)k);
    }
    state->input_processed = (int)st.base; state->output_size = k; state->last_correction_offset = st.correction_offset;
}

timing_recovery_algorithm_t timing_recovery_get_algorithm_from_string(char *input)
{   // libcsdr.c:2080-2086
    if (!strcmp(input, "GARDNER")) return TIMING_RECOVERY_ALGORITHM_GARDNER;
    if (!strcmp(input, "EARLYLATE")) return TIMING_RECOVERY_ALGORITHM_EARLYLATE;
    return TIMING_RECOVERY_ALGORITHM_DEFAULT;
}

char *timing_recovery_get_string_from_algorithm(timing_recovery_algorithm_t algorithm)
{   // libcsdr.c:2090-2096
    if (algorithm == TIMING_RECOVERY_ALGORITHM_GARDNER) return (char *)"GARDNER";
    if (algorithm == TIMING_RECOVERY_ALGORITHM_EARLYLATE) return (char *)"EARLYLATE";
    return (char *)"INVALID";
}

// the reference's function-level static last_input: one per process, its calls serialised
static std::mutex g_dbpsk_mu;
static csdr_amd_psk31_chan g_dbpsk_last;
void dbpsk_decoder_c_u8(complexf *in, unsigned char *out, int n)
{   // libcsdr.c:2319-2333
    if (n <= 0) return;
    std::lock_guard<std::mutex> lk(g_dbpsk_mu);
    // one object per thread (on that thread's context), kept between calls; last_input itself is the process-wide g_dbpsk_last
    struct DbCache { csdr_amd_psk31 *p = nullptr; ~DbCache() { if (p && (long)syscall(SYS_gettid) != (long)getpid()) csdr_amd_psk31_destroy(p); } };
    static thread_local DbCache cache;
    if (!cache.p) {
        csdr_amd_psk31_params pr; memset(&pr, 0, sizeof pr);
        cache.p = csdr_amd_psk31_create(ctx(), &pr, 1, CSDR_AMD_PSK31_DBPSK, CSDR_AMD_PSK31_DBPSK);
        if (!cache.p) die("dbpsk_decoder_c_u8", -3);
    }
    csdr_amd_psk31 *p = cache.p;
    csdr_amd_psk31_chan st; memset(&st, 0, sizeof st); st.last_i = g_dbpsk_last.last_i; st.last_q = g_dbpsk_last.last_q;
    MUST(csdr_amd_psk31_set_channel(p, 0, &st));
    complexf *din = stage_in<complexf>(4, in, n); unsigned char *dout = stage_out<unsigned char>(5, n); int *dcnt = stage_out<int>(6, 1);
    MUST(csdr_amd_psk31_process(p, din, n, n, dout, n, dcnt, nullptr, nullptr));
    fetch(out, dout, n);
    MUST(csdr_amd_psk31_get_channel(p, 0, &g_dbpsk_last));
}

char psk31_varicode_decoder_push(unsigned long long *status_shr, unsigned char symbol)
{   // libcsdr.c:1536-1549, on the host
    return csdr_amd_psk31_varicode_decoder_push(status_shr, symbol);
}

// ------------------------------------------------------------------ BPSK31 transmit (psk31tx.hip)
// one one-channel, one-stage object per thread and stage, kept while n_psk and the interpolation stay the same
static csdr_amd_psk31tx *tx_object(int stage, int n_psk, int interpolation, const char *who)
{
    struct TxCache { csdr_amd_psk31tx *p = nullptr; int n_psk = 0, I = 0; ~TxCache() { if (p && (long)syscall(SYS_gettid) != (long)getpid()) csdr_amd_psk31tx_destroy(p); } };
    static thread_local TxCache cache[4];
    TxCache &k = cache[stage];
    if (!k.p || k.n_psk != n_psk || k.I != interpolation) {
        if (k.p) csdr_amd_psk31tx_destroy(k.p);
        k.p = csdr_amd_psk31tx_create(ctx(), 1, n_psk, interpolation, stage, stage);
        if (!k.p) die(who, -3);
        k.n_psk = n_psk; k.I = interpolation;
    }
    return k.p;
}

void psk31_varicode_encoder_u8_u8(unsigned char *in, unsigned char *out, int n, int output_max_size, int *input_processed, int *output_size)
{   // libcsdr.c:1551-1575: how many characters fit is counted here from the code lengths, the bits come from the device
    int table[256];
    csdr_amd_psk31_varicode_table(table);
    int take = 0; long long room = output_max_size, bits = 0;
    for (; take < n; take++) {
        if (in[take] >= 128) continue;
        const int len = table[2 * in[take] + 1] + 2;
        if (room < len) break;
        room -= len; bits += len;
    }
    *input_processed = take; *output_size = (int)bits;
    if (!bits) return;
    csdr_amd_psk31tx *p = tx_object(CSDR_AMD_PSK31TX_VARICODE, 2, 1, "psk31_varicode_encoder_u8_u8");
    const size_t mo = (size_t)csdr_amd_psk31tx_max_out(p, take);
    unsigned char *din = stage_in<unsigned char>(4, in, take); unsigned char *dout = stage_out<unsigned char>(5, mo); int *dcnt = stage_out<int>(6, 1);
    MUST(csdr_amd_psk31tx_process(p, din, take, nullptr, take, dout, mo, dcnt));
    fetch(out, dout, (size_t)bits);
}

unsigned char differential_codec(unsigned char *in, unsigned char *out, int n, int encode, unsigned char state)
{   // libcsdr.c:1828-1843
    if (n <= 0) return state;
    unsigned char *din = stage_in<unsigned char>(4, in, n); unsigned char *dout = stage_out<unsigned char>(5, n);
    if (!encode) {
        unsigned char *dst = stage_in<unsigned char>(6, &state, 1);
        MUST(csdr_amd_differential_decoder_u8_u8(ctx(), din, dout, 1, n, n, n, dst));
        fetch(out, dout, n);
        fetch(&state, dst, 1);
        return state;
    }
    csdr_amd_psk31tx *p = tx_object(CSDR_AMD_PSK31TX_DIFF, 2, 1, "differential_codec");
    csdr_amd_psk31tx_chan st; memset(&st, 0, sizeof st); st.diff_state = state;
    MUST(csdr_amd_psk31tx_set_channel(p, 0, &st));
    int *dcnt = stage_out<int>(6, 1);
    MUST(csdr_amd_psk31tx_process(p, din, n, nullptr, n, dout, n, dcnt));
    fetch(out, dout, n);
    MUST(csdr_amd_psk31tx_get_channel(p, 0, &st));
    return st.diff_state;
}

void psk_modulator_u8_c(unsigned char *in, complexf *out, int n, int n_psk)
{   // libcsdr.c:1772-1782
    if (n <= 0) return;
    csdr_amd_psk31tx *p = tx_object(CSDR_AMD_PSK31TX_MOD, n_psk, 1, "psk_modulator_u8_c");
    unsigned char *din = stage_in<unsigned char>(4, in, n); complexf *dout = stage_out<complexf>(5, n); int *dcnt = stage_out<int>(6, 1);
    MUST(csdr_amd_psk31tx_process(p, din, n, nullptr, n, dout, n, dcnt));
    fetch(out, dout, n);
}

void duplicate_samples_ntimes_u8_u8(unsigned char *in, unsigned char *out, int input_size_bytes, int sample_size_bytes, int ntimes)
{   // libcsdr.c:1784-1791
    if (input_size_bytes <= 0 || sample_size_bytes <= 0 || ntimes <= 0) return;
    const size_t n = (size_t)input_size_bytes, m = n / sample_size_bytes * sample_size_bytes * ntimes;
    if (!m) return;
    unsigned char *din = stage_in<unsigned char>(4, in, n); unsigned char *dout = stage_out<unsigned char>(5, m);
    MUST(csdr_amd_duplicate_samples_ntimes_u8_u8(ctx(), din, dout, 1, (long long)n, n, m, sample_size_bytes, ntimes));
    fetch(out, dout, m);
}

complexf psk31_interpolate_sine_cc(complexf *in, complexf *out, int n, int interpolation, complexf last_input)
{   // libcsdr.c:1793-1808
    if (n <= 0) return last_input;
    csdr_amd_psk31tx *p = tx_object(CSDR_AMD_PSK31TX_SHAPE, 2, interpolation, "psk31_interpolate_sine_cc");
    csdr_amd_psk31tx_chan st; memset(&st, 0, sizeof st); st.last_i = last_input.i; st.last_q = last_input.q;
    MUST(csdr_amd_psk31tx_set_channel(p, 0, &st));
    const size_t mo = (size_t)csdr_amd_psk31tx_max_out(p, n);
    complexf *din = stage_in<complexf>(4, in, n); complexf *dout = stage_out<complexf>(5, mo); int *dcnt = stage_out<int>(6, 1);
    MUST(csdr_amd_psk31tx_process(p, din, n, nullptr, n, dout, mo, dcnt));
    fetch(out, dout, mo);
    return in[n - 1];
}

// ------------------------------------------------------------------ pulse-shaped symbol modem (modem.hip)
int firdes_rrc_f(float *taps, int taps_length, int samples_per_symbol, float beta)
{   // libcsdr.c:2482-2497, on the host; an even taps_length is designed as the reference does, without its write to taps[taps_length]
    if (taps_length >= 1) firdes_rrc_below(taps, taps_length, samples_per_symbol, beta);
    return 0;
}
int firdes_cosine_f(float *taps, int taps_length, int samples_per_symbol)
{   // libcsdr.c:2473-2480, on the host
    (void)csdr_amd_firdes_cosine_f(taps, taps_length, samples_per_symbol);
    return 0;
}
matched_filter_type_t matched_filter_get_type_from_string(char *input)
{   // libcsdr.c:2508-2516
    if (!strcmp("RRC", input)) return MATCHED_FILTER_RRC;
    if (!strcmp("COSINE", input)) return MATCHED_FILTER_COSINE;
    return MATCHED_FILTER_DEFAULT;
}
int apply_real_fir_cc(complexf *in, complexf *out, int n, float *taps, int taps_length)
{   // libcsdr.c:2276-2291
    if (taps_length < 1 || n < taps_length) return 0;
    cf32 *din = stage_in<cf32>(4, (const cf32 *)in, n); float *dt = stage_in<float>(6, taps, taps_length);
    cf32 *dout = stage_out<cf32>(5, n - taps_length + 1);
    const int produced = csdr_amd_apply_real_fir_cc(ctx(), din, dout, 1, n, n, n - taps_length + 1, dt, taps_length);
    if (produced < 0) die("apply_real_fir_cc", produced);
    fetch((cf32 *)out, dout, produced);
    return produced;
}
void generic_slicer_f_u8(float *input, unsigned char *output, int input_size, int n_symbols)
{   // libcsdr.c:1731-1765
    if (input_size <= 0 || n_symbols < 2 || n_symbols > 256) return;
    float *din = stage_in<float>(4, input, input_size); unsigned char *dout = stage_out<unsigned char>(5, input_size);
    MUST(csdr_amd_generic_slicer_f_u8(ctx(), din, dout, 1, input_size, input_size, input_size, n_symbols));
    fetch(output, dout, input_size);
}
void plain_interpolate_cc(complexf *in, complexf *out, int n, int interpolation)
{   // libcsdr.c:2499-2506
    if (n <= 0 || interpolation <= 0) return;
    const size_t m = (size_t)n * interpolation;
    cf32 *din = stage_in<cf32>(4, (const cf32 *)in, n); cf32 *dout = stage_out<cf32>(5, m);
    MUST(csdr_amd_plain_interpolate_cc(ctx(), din, dout, 1, n, n, m, interpolation));
    fetch((cf32 *)out, dout, m);
}
void pack_bits_1to8_u8_u8(unsigned char *in, unsigned char *out, int n)
{   // libcsdr.c:1810-1815
    if (n <= 0) return;
    unsigned char *din = stage_in<unsigned char>(4, in, n); unsigned char *dout = stage_out<unsigned char>(5, 8 * (size_t)n);
    MUST(csdr_amd_pack_bits_1to8_u8_u8(ctx(), din, dout, 1, n, n, 8 * (size_t)n));
    fetch(out, dout, 8 * (size_t)n);
}
unsigned char pack_bits_8to1_u8_u8(unsigned char *input) { return pack_bits_8to1_step(input); }   // libcsdr.c:1818-1827: eight bytes, on the host

// ------------------------------------------------------------------ RTTY receive (rtty.hip)
int bfsk_demod_cf(complexf *in, float *out, int n, complexf *mark_filter, complexf *space_filter, int taps_length)
{   // libcsdr.c:2335-2350
    const int no = n - taps_length + 1;
    if (no <= 0 || taps_length < 1) return no;
    cf32 *din = stage_in<cf32>(4, (const cf32 *)in, n); float *dout = stage_out<float>(5, no);
    cf32 *dt = stage_in<cf32>(6, (const cf32 *)mark_filter, taps_length, taps_length);
    MUST(hipMemcpyAsync(dt + taps_length, space_filter, sizeof(cf32) * taps_length, hipMemcpyHostToDevice, ctx()->stream) == hipSuccess ? 0 : -1);
    MUST(csdr_amd_bfsk_demod_cf(ctx(), din, dout, 1, n, n, no, dt, dt + taps_length, taps_length, 0));
    fetch(out, dout, no);
    return no;
}

int apply_fir_cc(complexf *in, complexf *out, int n, complexf *taps, int taps_length)
{   // libcsdr.c:2261-2273
    const int no = n - taps_length + 1;
    if (no <= 0 || taps_length < 1) return 0;
    cf32 *din = stage_in<cf32>(4, (const cf32 *)in, n); cf32 *dout = stage_out<cf32>(5, no);
    cf32 *dt = stage_in<cf32>(6, (const cf32 *)taps, taps_length);
    MUST(csdr_amd_apply_fir_cc(ctx(), din, dout, 1, n, n, no, dt, 0, taps_length, 0));
    fetch((cf32 *)out, dout, no);
    return no;
}

void firdes_add_peak_c(complexf *output, int length, float rate, window_t window, int add, int normalize)
{   // libcsdr.c:2219-2257, on the host
    csdr_amd_firdes_add_peak_c((cf32 *)output, length, rate, (int)window, add, normalize);
}

void serial_line_decoder_f_u8(serial_line_t *s, float *input, unsigned char *output, int input_size)
{   // libcsdr.c:1662-1728: one window per call; output elements of 1, 2 or 4 bytes by databits
    s->output_size = 0; s->input_used = 0;
    if (input_size <= 0) return;
    const size_t esz = s->databits <= 8 ? 1 : s->databits <= 16 ? 2 : 4;
    float *din = stage_in<float>(4, input, input_size); unsigned char *dout = stage_out<unsigned char>(5, esz * input_size);
    int *dcu = stage_out<int>(6, 2);
    MUST(csdr_amd_serial_line_decoder_f_u8(ctx(), din, dout, 1, input_size, input_size, input_size, s->samples_per_bits, s->databits, s->stopbits,
                                           s->bit_sampling_width_ratio, dcu, dcu + 1));
    int cu[2]; fetch(cu, dcu, 2);
    if (cu[0]) fetch(output, dout, esz * cu[0]);
    s->output_size = cu[0]; s->input_used = cu[1];
}

void binary_slicer_f_u8(float *input, unsigned char *output, int input_size)
{   // libcsdr.c:1767-1770
    if (input_size <= 0) return;
    float *din = stage_in<float>(4, input, input_size); unsigned char *dout = stage_out<unsigned char>(5, input_size);
    MUST(csdr_amd_binary_slicer_f_u8(ctx(), din, dout, 1, input_size, input_size, input_size));
    fetch(output, dout, input_size);
}

// ------------------------------------------------------------------ squelch and S-meter (squelch.hip)
float get_power_f(float *input, int input_size, int decimation)
{   // libcsdr.c:1144-1152
    if (input_size <= 0 || decimation <= 0) return 0.f;
    float *din = stage_in<float>(4, input, input_size); float *dout = stage_out<float>(5, 1);
    MUST(csdr_amd_get_power_f(ctx(), din, 1, 1, input_size, decimation, input_size, dout));
    float p = 0.f; fetch(&p, dout, 1);
    return p;
}

float get_power_c(complexf *input, int input_size, int decimation)
{   // libcsdr.c:1154-1162
    if (input_size <= 0 || decimation <= 0) return 0.f;
    cf32 *din = stage_in<cf32>(4, (const cf32 *)input, input_size); float *dout = stage_out<float>(5, 1);
    MUST(csdr_amd_get_power_c(ctx(), din, 1, 1, input_size, decimation, input_size, dout));
    float p = 0.f; fetch(&p, dout, 1);
    return p;
}

// ------------------------------------------------------------------ carrier recovery (carrier.hip)
// One call = the thread's one-channel object with the caller's coefficients and state: state in, n samples, state out.
static void run_carrier(const csdr_amd_carrier_params &pr, csdr_amd_carrier_chan *st, complexf *in, int n, complexf *out, float *error, float *dphase, complexf *nco)
{
    struct CrCache { csdr_amd_carrier *p = nullptr; csdr_amd_carrier_params pr; ~CrCache() { if (p && (long)syscall(SYS_gettid) != (long)getpid()) csdr_amd_carrier_destroy(p); } };
    static thread_local CrCache cache;
    if (!cache.p || memcmp(&cache.pr, &pr, sizeof pr)) {
        if (cache.p) csdr_amd_carrier_destroy(cache.p);
        cache.p = csdr_amd_carrier_create(ctx(), &pr, 1);
        if (!cache.p) die("carrier_create", -3);
        cache.pr = pr;
    }
    MUST(csdr_amd_carrier_set_channel(cache.p, 0, st));
    complexf *din = stage_in<complexf>(4, in, n);
    // one scratch slot for the four outputs: out, nco (8 bytes per sample), error, dphase (4 bytes)
    char *d = stage_out<char>(5, 24 * (size_t)n);
    complexf *dout = (complexf *)d, *dnco = dout + n; float *derr = (float *)(dnco + n), *ddph = derr + n;
    MUST(csdr_amd_carrier_process(cache.p, (const csdr_complexf *)din, n, n, out ? (csdr_complexf *)dout : nullptr, error ? derr : nullptr, dphase ? ddph : nullptr,
                                  nco ? (csdr_complexf *)dnco : nullptr, n));
    if (out) fetch(out, dout, n);
    if (error) fetch(error, derr, n);
    if (dphase) fetch(dphase, ddph, n);
    if (nco) fetch(nco, dnco, n);
    MUST(csdr_amd_carrier_get_channel(cache.p, 0, st));
}

void init_bpsk_costas_loop_cc(bpsk_costas_loop_state_t *s, int, float damping_factor, float bandwidth)
{   // libcsdr.c:2094-2106 (decision_directed is not stored there either)
    csdr_amd_carrier_params pr;
    csdr_amd_costas_params(bandwidth, damping_factor, 0, &pr);
    s->alpha = pr.alpha; s->beta = pr.beta;
    s->current_freq = s->dphase = s->nco_phase = 0;
    s->dphase_max = pr.dphase_max;
    s->dphase_max_reset_to_zero = 0;
}

void bpsk_costas_loop_cc(complexf *input, complexf *output, int input_size, float *output_error, float *output_dphase, complexf *output_nco, bpsk_costas_loop_state_t *s)
{   // libcsdr.c:2108-2142
    if (input_size <= 0) return;
    csdr_amd_carrier_params pr; memset(&pr, 0, sizeof pr);
    pr.mode = s->decision_directed ? CSDR_AMD_CARRIER_COSTAS_DD : CSDR_AMD_CARRIER_COSTAS;
    pr.alpha = s->alpha; pr.beta = s->beta; pr.dphase_max = s->dphase_max; pr.dphase_max_reset_to_zero = s->dphase_max_reset_to_zero != 0;
    csdr_amd_carrier_chan st = { s->nco_phase, s->dphase, s->current_freq };
    run_carrier(pr, &st, input, input_size, output, output_error, output_dphase, output_nco);
    s->nco_phase = st.phase; s->dphase = st.dphase; s->current_freq = st.freq;
}

void pll_cc_init_pi_controller(pll_t *p, float bandwidth, float ko, float kd, float damping_factor)
{   // libcsdr.c:1856-1865
    csdr_amd_carrier_params pr;
    csdr_amd_pll_params_pi(bandwidth, ko, kd, damping_factor, &pr);
    p->alpha = pr.alpha; p->beta = pr.beta;
    p->iir_temp = p->dphase = p->output_phase = 0;
}

void pll_cc_init_p_controller(pll_t *p, float alpha)
{   // libcsdr.c:1867-1871
    p->alpha = alpha;
    p->dphase = p->output_phase = 0;
}

void pll_cc(pll_t *p, complexf *input, float *output_dphase, complexf *output_nco, int input_size)
{   // libcsdr.c:1874-1915
    if (input_size <= 0) return;
    if (p->pll_type != PLL_PI_CONTROLLER && p->pll_type != PLL_P_CONTROLLER) {     // :1878-1884, 1911: the phase moves on, the first NCO sample is written
        p->output_phase = carrier_wrap_pm_pi(p->output_phase + p->dphase);
        if (output_nco) carrier_sincos(p->output_phase, &output_nco[0].i, &output_nco[0].q);
        return;
    }
    csdr_amd_carrier_params pr; memset(&pr, 0, sizeof pr);
    pr.mode = p->pll_type == PLL_PI_CONTROLLER ? CSDR_AMD_CARRIER_PLL_PI : CSDR_AMD_CARRIER_PLL_P;
    pr.alpha = p->alpha; pr.beta = pr.mode == CSDR_AMD_CARRIER_PLL_PI ? p->beta : 0.f;
    csdr_amd_carrier_chan st = { p->output_phase, p->dphase, pr.mode == CSDR_AMD_CARRIER_PLL_PI ? p->iir_temp : 0.f };
    float *dph = output_dphase;
    std::vector<float> unused;
    if (!output_dphase && !output_nco) { unused.resize(input_size); dph = unused.data(); }      // the state still has to move
    run_carrier(pr, &st, input, input_size, nullptr, nullptr, dph, output_nco);
    p->output_phase = st.phase; p->dphase = st.dphase;
    if (pr.mode == CSDR_AMD_CARRIER_PLL_PI) p->iir_temp = st.freq;
}

char rtty_baudot_decoder_lookup(unsigned char *fig_mode, unsigned char c) { return csdr_amd_rtty_baudot_decoder_lookup(fig_mode, c); }   // libcsdr.c:1606-1613

char rtty_baudot_decoder_push(rtty_baudot_decoder_t *s, unsigned char symbol)
{   // libcsdr.c:1615-1655, on the host
    csdr_amd_rtty_push_state p = {s->fig_mode, s->character_received, s->shr, s->bit_cntr, (int)s->state};
    const char r = csdr_amd_rtty_baudot_decoder_push(&p, symbol);
    s->fig_mode = (unsigned char)p.fig_mode; s->character_received = (unsigned char)p.character_received; s->shr = (unsigned short)p.shr;
    s->bit_cntr = (unsigned char)p.bit_cntr; s->state = (rtty_baudot_decoder_state_t)p.state;
    return r;
}

// One call of each FIR resampler = a fresh batch object fed the whole block once (resampler.hip).
rational_resampler_ff_t rational_resampler_ff(float *in, float *out, int n, int interpolation, int decimation, float *taps, int taps_length, int last_taps_delay)
{
    rational_resampler_ff_t d;
    int st[3];
    MUST(csdr_amd_resampler_window(interpolation, decimation, taps_length, n, last_taps_delay, st));
    d.input_processed = st[0]; d.output_size = st[1]; d.last_taps_delay = st[2];
    if (!d.output_size) return d;
    csdr_amd_resampler *r = csdr_amd_resampler_create(ctx(), interpolation, decimation, taps, taps_length, 1);
    if (!r) die("rational_resampler_ff", -3);
    MUST(csdr_amd_resampler_set_cli_bufsize(r, n));                      // one window of n samples: the reference's cap exit included
    MUST(csdr_amd_resampler_set_last_taps_delay(r, last_taps_delay));
    float *din = stage_in<float>(4, in, n); float *dout = stage_out<float>(5, (size_t)d.output_size + 2);
    long long produced = 0;
    MUST(csdr_amd_resampler_process(r, din, n, n, dout, (size_t)d.output_size + 2, &produced));
    if (produced != d.output_size) die("rational_resampler_ff", -5);
    fetch(out, dout, (size_t)produced);
    csdr_amd_resampler_destroy(r);
    return d;
}

void rational_resampler_get_lowpass_f(float *output, int output_size, int interpolation, int decimation, window_t window)
{
    csdr_amd_rational_resampler_get_lowpass_f(output, output_size, interpolation, decimation, (int)window);
}

int fir_interpolate_cc(complexf *in, complexf *out, int n, int interpolation, float *taps, int taps_length)
{
    if (n <= 0) return 0;
    csdr_amd_interp *p = csdr_amd_interp_create(ctx(), interpolation, taps, taps_length, 1);
    if (!p) die("fir_interpolate_cc", -3);
    cf32 *din = stage_in<cf32>(4, (const cf32 *)in, n);
    const size_t cap = (size_t)csdr_amd_interp_max_out(p, n);
    cf32 *dout = stage_out<cf32>(5, cap);
    long long produced = 0;
    MUST(csdr_amd_interp_process(p, din, n, n, dout, cap, &produced));
    fetch((cf32 *)out, dout, (size_t)produced);
    csdr_amd_interp_destroy(p);
    return (int)produced;
}

// ------------------------------------------------------------------ FFT plan layer (fft_fftw.c:6-45) on hipFFT
void *csdr_fft_malloc(size_t n) { void *p = nullptr; if (posix_memalign(&p, 64, n ? n : 64)) return nullptr; return p; }
void csdr_fft_free(void *p) { free(p); }
// The reference's own header maps fft_malloc / fft_free to fftwf_malloc / fftwf_free (fft_fftw.h:11-12): a client compiled against it asks the dynamic linker for
// these two FFTW symbols and nothing else of FFTW (plans go through make_fft_c2c / fft_execute, served here).  Exported so that such a client needs no -lfftw3f.
// (If the real libfftw3f is loaded as well, whichever comes first in the link order serves both calls: either pair is a plain aligned malloc / free.)
void *fftwf_malloc(size_t n) { return csdr_fft_malloc(n); }
void fftwf_free(void *p) { csdr_fft_free(p); }

static FFT_PLAN_T *make_plan(int size, void *in, void *out, int kind, int forward)
{
    FFT_PLAN_T *p = (FFT_PLAN_T *)malloc(sizeof(FFT_PLAN_T));
    FftPlanImpl *impl = (FftPlanImpl *)malloc(sizeof(FftPlanImpl));
    impl->kind = kind; impl->forward = forward;
    p->size = size; p->input = in; p->output = out; p->plan = impl;
    return p;
}
FFT_PLAN_T *make_fft_c2c(int size, complexf *input, complexf *output, int forward, int) { return make_plan(size, input, output, 0, forward); }
FFT_PLAN_T *make_fft_r2c(int size, float *input, complexf *output, int) { return make_plan(size, input, output, 1, 1); }
FFT_PLAN_T *make_fft_c2r(int size, complexf *input, float *output, int) { return make_plan(size, input, output, 2, 0); }
void fft_destroy(FFT_PLAN_T *p) { if (p) { free(p->plan); free(p); } }
void fft_execute(FFT_PLAN_T *p)
{
    const FftPlanImpl *impl = (const FftPlanImpl *)p->plan;
    const int n = p->size;
    csdr_amd_ctx *c = ctx();
    if (impl->kind == 0) {
        cf32 *din = stage_in<cf32>(4, (const cf32 *)p->input, n); cf32 *dout = stage_out<cf32>(5, n);
        MUST(csdr_amd_fft_c2c(c, din, dout, n, impl->forward));
        fetch((cf32 *)p->output, dout, n);
    } else if (impl->kind == 1) {      // real -> half spectrum: widen to complex on the host side of the copy (setup-rate path)
        std::vector<cf32> tmp(n); const float *x = (const float *)p->input;
        for (int k = 0; k < n; k++) tmp[k] = cf32{x[k], 0.f};
        cf32 *din = stage_in<cf32>(4, tmp.data(), n); cf32 *dout = stage_out<cf32>(5, n);
        MUST(csdr_amd_fft_c2c(c, din, dout, n, 1));
        fetch(tmp.data(), dout, n);
        memcpy(p->output, tmp.data(), sizeof(cf32) * (n / 2 + 1));
    } else {                           // half spectrum -> real
        std::vector<cf32> tmp(n); const cf32 *x = (const cf32 *)p->input;
        for (int k = 0; k <= n / 2; k++) tmp[k] = x[k];
        for (int k = n / 2 + 1; k < n; k++) tmp[k] = cf32{x[n - k].i, -x[n - k].q};
        cf32 *din = stage_in<cf32>(4, tmp.data(), n); cf32 *dout = stage_out<cf32>(5, n);
        MUST(csdr_amd_fft_c2c(c, din, dout, n, 0));
        fetch(tmp.data(), dout, n);
        float *y = (float *)p->output; for (int k = 0; k < n; k++) y[k] = tmp[k].i;
    }
}

void apply_fir_fft_cc(FFT_PLAN_T *plan, FFT_PLAN_T *plan_inverse, complexf *taps_fft, complexf *last_overlap, int overlap_size)
{   // libcsdr.c:814-849, all on the device between one upload and one download per buffer the reference exposes
    const int n = plan->size;
    csdr_amd_ctx *c = ctx();
    cf32 *din = stage_in<cf32>(4, (const cf32 *)plan->input, n);
    cf32 *dspec = stage_out<cf32>(5, n);
    cf32 *dtaps = stage_in<cf32>(6, (const cf32 *)taps_fft, n);
    MUST(csdr_amd_fft_c2c(c, din, dspec, n, 1));
    fetch((cf32 *)plan->output, dspec, n);                               // plan->output holds the spectrum in the reference too
    MUST(csdr_amd_bin_product(c, dspec, dtaps, din, n));
    fetch((cf32 *)plan_inverse->input, din, n);
    MUST(csdr_amd_fft_c2c(c, din, dspec, n, 0));
    cf32 *dov = stage_in<cf32>(7, (const cf32 *)last_overlap, overlap_size);
    MUST(csdr_amd_scale_add(c, dspec, n, 1.0f / (float)n, dov, overlap_size));
    fetch((cf32 *)plan_inverse->output, dspec, n);
}

// ------------------------------------------------------------------ fastddc
int fastddc_init(fastddc_t *ddc, float tbw, int decimation, float shift_rate)
{
    static_assert(sizeof(fastddc_t) == sizeof(csdr_fastddc_t), "fastddc_t layout");
    return csdr_amd_fastddc_init((csdr_fastddc_t *)ddc, tbw, decimation, shift_rate);
}
void fastddc_print(fastddc_t *ddc, char *source)
{   // fastddc.c:75-89 (same text)
    fprintf(stderr,
        "%s: fastddc_print_sizes(): (fft_size = %d) = (taps_length = %d) + (input_size = %d) - 1\n"
        "  overlap     ::  (overlap_length = %d) = taps_length - 1, taps_min_length = %d\n"
        "  decimation  ::  decimation = (pre_decimation = %d) * (post_decimation = %d), fft_inv_size = %d\n"
        "  shift       ::  startbin = %d, offsetbin = %d, v = %d, pre_shift = %g, post_shift = %g\n"
        "  o&s         ::  post_input_size = %d, scrap = %d\n",
        source, ddc->fft_size, ddc->taps_length, ddc->input_size, ddc->overlap_length, ddc->taps_min_length,
        ddc->pre_decimation, ddc->post_decimation, ddc->fft_inv_size, ddc->startbin, ddc->offsetbin, ddc->v,
        ddc->pre_shift, ddc->post_shift, ddc->post_input_size, ddc->scrap);
}
void fft_swap_sides(complexf *io, int fft_size)
{   // fastddc.c:91-104 -- an in-place permutation of a host buffer (setup helper; the batch path folds it into index math)
    const int h = fft_size / 2;
    for (int k = 0; k < h; k++) { complexf t = io[k]; io[k] = io[k + h]; io[k + h] = t; }
}
decimating_shift_addition_status_t fastddc_inv_cc(complexf *input, complexf *output, fastddc_t *ddc, FFT_PLAN_T *plan_inverse, complexf *taps_fft,
                                                  decimating_shift_addition_status_t st)
{
    csdr_amd_ctx *c = ctx();
    const int fft = ddc->fft_size, inv = ddc->fft_inv_size;
    cf32 *dspec = stage_in<cf32>(4, (const cf32 *)input, fft);
    cf32 *dtaps = stage_in<cf32>(6, (const cf32 *)taps_fft, fft);
    cf32 *dwork = stage_out<cf32>(5, 2 * (size_t)inv + ddc->post_input_size + 8);
    cf32 *dinv_in = dwork, *dtd = dwork + inv, *dout = dwork + 2 * inv;
    MUST(csdr_amd_fastddc_inv_block(c, dspec, dtaps, (const csdr_fastddc_t *)ddc, &st, dinv_in, dtd, dout));
    fetch((cf32 *)output, dout, st.output_size);
    if (plan_inverse) {                                                  // the reference leaves its work in the plan's buffers
        if (plan_inverse->input) fetch((cf32 *)plan_inverse->input, dinv_in, inv);
        if (plan_inverse->output) {
            fetch((cf32 *)plan_inverse->output, dtd, inv);
            cf32 *o = (cf32 *)plan_inverse->output; const float s = 1.0f / (float)inv;
            for (int k = 0; k < inv; k++) { o[k].i *= s; o[k].q *= s; }
        }
    }
    fft_swap_sides(input, fft);                                          // the reference swaps its input in place (fastddc.c:123)
    return st;
}


// ------------------------------------------------------------------ f2 blocks (libcsdr.c:861-941, 1004-1019, 1245-1303; libcsdr_gpl.c:163-260)
void amdemod_cf(complexf *in, float *out, int n)
{
    if (n <= 0) return;
    cf32 *din = stage_in<cf32>(4, (const cf32 *)in, n); float *dout = stage_out<float>(5, n);
    MUST(csdr_amd_amdemod_cf(ctx(), (const csdr_complexf *)din, dout, n)); fetch(out, dout, n);
}
void amdemod_estimator_cf(complexf *in, float *out, int n, float alpha, float beta)
{
    if (n <= 0) return;
    cf32 *din = stage_in<cf32>(4, (const cf32 *)in, n); float *dout = stage_out<float>(5, n);
    MUST(csdr_amd_amdemod_estimator_cf(ctx(), (const csdr_complexf *)din, dout, n, alpha, beta)); fetch(out, dout, n);
}
void logpower_cf(complexf *in, float *out, int n, float add_db)
{
    if (n <= 0) return;
    cf32 *din = stage_in<cf32>(4, (const cf32 *)in, n); float *dout = stage_out<float>(5, n);
    MUST(csdr_amd_logpower_cf(ctx(), (const csdr_complexf *)din, dout, n, add_db)); fetch(out, dout, n);
}
void accumulate_power_cf(complexf *in, float *out, int n)
{
    if (n <= 0) return;
    cf32 *din = stage_in<cf32>(4, (const cf32 *)in, n); float *dacc = stage_in<float>(5, out, n);
    MUST(csdr_amd_accumulate_power_cf(ctx(), (const csdr_complexf *)din, dacc, n)); fetch(out, dacc, n);
}
void log_ff(float *in, float *out, int n, float add_db)
{
    if (n <= 0) return;
    float *din = stage_in<float>(4, in, n); float *dout = stage_out<float>(5, n);
    MUST(csdr_amd_log_ff(ctx(), din, dout, n, add_db)); fetch(out, dout, n);
}
float fmdemod_atan_cf(complexf *in, float *out, int n, float last_phase)
{
    if (n <= 0) return last_phase;
    cf32 *din = stage_in<cf32>(4, (const cf32 *)in, n); float *dout = stage_out<float>(5, n); float *dl = stage_in<float>(6, &last_phase, 1);
    MUST(csdr_amd_fmdemod_atan_cf(ctx(), (const csdr_complexf *)din, dout, 1, n, n, n, dl));
    fetch(out, dout, n);
    float l; fetch(&l, dl, 1); return l;
}
dcblock_preserve_t dcblock_ff(float *in, float *out, int n, float a, dcblock_preserve_t preserved)
{
    if (n <= 0) return preserved;
    float *din = stage_in<float>(4, in, n); float *dout = stage_out<float>(5, n); float *ds = stage_in<float>(6, &preserved.last_input, 2);
    MUST(csdr_amd_dcblock_ff(ctx(), din, dout, 1, n, n, n, a, ds));
    fetch(out, dout, n);
    fetch(&preserved.last_input, ds, 2);
    return preserved;
}
float fastdcblock_ff(float *in, float *out, int n, float last_dc_level)
{
    if (n <= 0) return last_dc_level;
    float *din = stage_in<float>(4, in, n); float *dout = stage_out<float>(5, n); float *dl = stage_in<float>(6, &last_dc_level, 1);
    MUST(csdr_amd_fastdcblock_ff(ctx(), din, dout, 1, 1, n, n, n, dl));
    fetch(out, dout, n);                                                 // in == out is allowed by the reference: the device buffers are distinct
    float l; fetch(&l, dl, 1); return l;
}
float agc_ff(float *in, float *out, int n, float reference, float attack_rate, float decay_rate, float max_gain, short hang_time, short attack_wait_time,
             float gain_filter_alpha, float last_gain)
{
    if (n <= 0) return last_gain;
    float *din = stage_in<float>(4, in, n); float *dout = stage_out<float>(5, n); float *dl = stage_in<float>(6, &last_gain, 1);
    MUST(csdr_amd_agc_ff(ctx(), din, dout, 1, n, n, n, n, reference, attack_rate, decay_rate, max_gain, hang_time, attack_wait_time, gain_filter_alpha, dl));
    fetch(out, dout, n);
    float l; fetch(&l, dl, 1); return l;
}
float *precalculate_window(int size, window_t window)
{   // libcsdr.c:1256-1267: caller owns the malloc'ed table
    float *w = (float *)malloc(sizeof(float) * (size > 0 ? size : 1));
    if (w && size > 0) csdr_amd_precalculate_window(w, size, (int)window);
    return w;
}
void apply_precalculated_window_c(complexf *in, complexf *out, int size, float *windowt)
{   // libcsdr.c:1269-1276: one float product per component; a host loop is the whole job at this size, the device path is csdr_amd_fftcc
    for (int k = 0; k < size; k++) { out[k].i = in[k].i * windowt[k]; out[k].q = in[k].q * windowt[k]; }
}
void apply_window_c(complexf *in, complexf *out, int size, window_t window)
{   // libcsdr.c:1245-1254
    float *w = precalculate_window(size, window);
    apply_precalculated_window_c(in, out, size, w);
    free(w);
}

// ------------------------------------------------------------------ transmit-side modulators (txmod.hip), libcsdr.h:216-218
float fmmod_fc(float *in, complexf *out, int n, float last_phase)
{
    if (n <= 0) return last_phase;
    float *din = stage_in<float>(4, in, n); cf32 *dout = stage_out<cf32>(5, n); float *dl = stage_in<float>(6, &last_phase, 1);
    MUST(csdr_amd_fmmod_fc(ctx(), din, (csdr_complexf *)dout, 1, n, n, n, dl));
    fetch((cf32 *)out, dout, n);
    float l; fetch(&l, dl, 1); return l;
}
void add_dcoffset_cc(complexf *in, complexf *out, int n)
{
    if (n <= 0) return;
    cf32 *din = stage_in<cf32>(4, (const cf32 *)in, n); cf32 *dout = stage_out<cf32>(5, n);
    MUST(csdr_amd_add_dcoffset_cc(ctx(), (const csdr_complexf *)din, (csdr_complexf *)dout, n)); fetch((cf32 *)out, dout, n);
}
void fixed_amplitude_cc(complexf *in, complexf *out, int n, float amp)
{
    if (n <= 0) return;
    cf32 *din = stage_in<cf32>(4, (const cf32 *)in, n); cf32 *dout = stage_out<cf32>(5, n);
    MUST(csdr_amd_fixed_amplitude_cc(ctx(), (const csdr_complexf *)din, (csdr_complexf *)dout, n, amp)); fetch((cf32 *)out, dout, n);
}

// ------------------------------------------------------------------ f3: IMA ADPCM (ima_adpcm.h:5-11)
ima_adpcm_state_t encode_ima_adpcm_i16_u8(short *in, unsigned char *out, int n, ima_adpcm_state_t state)
{
    if (n < 2) return state;
    int16_t *din = stage_in<int16_t>(4, in, n); uint8_t *dout = stage_out<uint8_t>(5, n / 2 + 16); int *ds = stage_in<int>(6, &state.index, 2);
    MUST(csdr_amd_encode_ima_adpcm_i16_u8(ctx(), din, dout, 1, n, n, n / 2, ds));
    fetch(out, dout, n / 2); fetch(&state.index, ds, 2);
    return state;
}
ima_adpcm_state_t decode_ima_adpcm_u8_i16(unsigned char *in, short *out, int n, ima_adpcm_state_t state)
{
    if (n <= 0) return state;
    uint8_t *din = stage_in<uint8_t>(4, in, n); int16_t *dout = stage_out<int16_t>(5, 2 * (size_t)n + 16); int *ds = stage_in<int>(6, &state.index, 2);
    MUST(csdr_amd_decode_ima_adpcm_u8_i16(ctx(), din, dout, 1, n, n, 2 * (size_t)n, ds));
    fetch(out, dout, 2 * (size_t)n); fetch(&state.index, ds, 2);
    return state;
}

// ------------------------------------------------------------------ noise sources and link measurements (libcsdr.c:2444-2471, 2518-2521, 1316-1321, 2293-2317): host code
FILE *init_get_random_samples_f(void) { return fopen("/dev/urandom", "r"); }
void get_random_samples_f(float *output, int output_size, FILE *status)
{
    if (output_size <= 0) return;
    fread((unsigned char *)output, sizeof(float), output_size, status);
    for (int i = 0; i < output_size; i++) { uint32_t w; memcpy(&w, output + i, 4); output[i] = noise_uniform(w); }
}
void get_random_gaussian_samples_c(complexf *output, int output_size, FILE *status)
{
    if (output_size <= 0) return;
    fread((unsigned char *)output, sizeof(complexf), output_size, status);
    for (int i = 0; i < output_size; i++) {
        uint32_t w[2]; memcpy(w, output + i, 8);
        const float2 g = noise_gauss(w[0], w[1]);
        memcpy(output + i, &g, 8);
    }
}
int deinit_get_random_samples_f(FILE *status) { return fclose(status); }
float *add_ff(float *input1, float *input2, float *output, int input_size)
{
    for (int i = 0; i < input_size; i++) output[i] = input1[i] + input2[i];
    return output;
}
float total_logpower_cf(complexf *input, int input_size)
{
    const float *x = (const float *)input;
    float acc = 0;
    for (int i = 0; i < input_size; i++) acc += x[2 * i] * x[2 * i] + x[2 * i + 1] * x[2 * i + 1];
    return 10 * log10(acc / input_size);
}
float normalized_timing_variance_u32_f(unsigned *input, float *temp, int input_size, int samples_per_symbol, int initial_sample_offset, int debug_print)
{   // temp and debug_print: the reference's scratch and its stderr trace, neither needed here
    (void)temp; (void)debug_print;
    if (input_size <= 0 || samples_per_symbol < 1) return 0.f;
    return timing_variance([&](int i) { return input[i]; }, input_size, samples_per_symbol, initial_sample_offset);
}

} // extern "C"
