/* include/csdr_amd.h -- C ABI of the MI355X-native libcsdr hot path (libcsdr_amd.so).
 *
 * Two layers, both plain C (no torch / C++ types in any signature):
 *
 *  1. DEVICE BATCH API  (csdr_amd_*):  device pointers, N independent sample streams per call,
 *     stream-major layout  buf[stream * pitch + sample]  (pitch in ELEMENTS of the buffer's type),
 *     asynchronous on the context's HIP stream.  This is what bench.py and the parity tests drive.
 *     Cross-block state (phases, last samples, filter history) is explicit and caller-owned, exactly
 *     like the reference's by-value state, but held in device arrays of
 *     n_streams entries so that a call never synchronises with the host.
 *
 *  2. DROP-IN HOST API  (include/libcsdr_amd_compat.h): the reference's own symbols
 *     (libcsdr.h:85-229, libcsdr_gpl.h:26-46, fastddc.h:26-29, fft_fftw.h:24-27) with identical
 *     signatures and struct layouts, operating on host pointers (H2D -> kernels -> D2H).
 *
 * Every entry point cites the reference interface it replaces.  Return value: 0 on success,
 * negative on error (csdr_amd_last_error() gives the text) unless stated otherwise.
 * The library FAILS LOUDLY (error return, never a CPU fallback) when no gfx950 device is usable.
 */
#ifndef CSDR_AMD_H
#define CSDR_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* libcsdr.h:46 -- interleaved I/Q pair, 8 bytes */
typedef struct csdr_complexf_s { float i, q; } csdr_complexf;

/* libcsdr.h:70-73 */
typedef enum { CSDR_WINDOW_BOXCAR = 0, CSDR_WINDOW_BLACKMAN = 1, CSDR_WINDOW_HAMMING = 2 } csdr_window_t;

typedef struct csdr_amd_ctx csdr_amd_ctx;

/* ------------------------------------------------------------------ context / memory */
/* hip_stream: a hipStream_t owned by the caller (e.g. torch.cuda.current_stream().cuda_stream) or
 * NULL to let the context create its own non-blocking stream. */
csdr_amd_ctx *csdr_amd_ctx_create(int device, void *hip_stream);
void          csdr_amd_ctx_destroy(csdr_amd_ctx *ctx);
int           csdr_amd_ctx_sync(csdr_amd_ctx *ctx);
void         *csdr_amd_ctx_stream(csdr_amd_ctx *ctx);
const char   *csdr_amd_last_error(void);
int           csdr_amd_device_count(void);
/* "gfx950:sramecc+:xnack-" style architecture name of the context's device */
const char   *csdr_amd_device_arch(csdr_amd_ctx *ctx);

void *csdr_amd_malloc(csdr_amd_ctx *ctx, size_t bytes);
void  csdr_amd_free(csdr_amd_ctx *ctx, void *dptr);
int   csdr_amd_h2d(csdr_amd_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);   /* sync */
int   csdr_amd_d2h(csdr_amd_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);   /* sync */
int   csdr_amd_d2d(csdr_amd_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes);    /* async, regions must not overlap */
int   csdr_amd_memset(csdr_amd_ctx *ctx, void *dst_dev, int value, size_t bytes);           /* async */

/* HIP-event timing on the context's stream (bench.py: the kernel stream is not torch's stream) */
int   csdr_amd_timer_start(csdr_amd_ctx *ctx);
int   csdr_amd_timer_stop_ms(csdr_amd_ctx *ctx, float *ms);   /* records, synchronises, returns elapsed */

/* ------------------------------------------------------------------ host-side design helpers */
int  csdr_amd_firdes_filter_len(float transition_bw);                                        /* libcsdr.c:169-174 */
void csdr_amd_firdes_lowpass_f(float *taps, int length, float cutoff_rate, int window);      /* libcsdr.c:117-142 */
void csdr_amd_firdes_bandpass_c(csdr_complexf *taps, int length, float lowcut, float highcut, int window); /* :144-167 */
int  csdr_amd_next_pow2(int x);                                                              /* libcsdr.c:1235-1243 */
int  csdr_amd_log2n(int x);                                                                  /* libcsdr.c:1220-1233 */
/* fixed NFM de-emphasis FIR tables (predefined.h:56-68): returns tap count or 0 for an unsupported rate */
int  csdr_amd_nfm_deemph_taps(int sample_rate, const float **taps);

/* ------------------------------------------------------------------ sample-format converters (bit exact)
 * libcsdr.c:2363-2437 / libcsdr.h:220-229.  n = number of VALUES (not bytes). */
int csdr_amd_convert_u8_f (csdr_amd_ctx *ctx, const uint8_t *in, float *out, size_t n);
int csdr_amd_convert_s8_f (csdr_amd_ctx *ctx, const int8_t *in, float *out, size_t n);
int csdr_amd_convert_s16_f(csdr_amd_ctx *ctx, const int16_t *in, float *out, size_t n);
int csdr_amd_convert_f_u8 (csdr_amd_ctx *ctx, const float *in, uint8_t *out, size_t n);
int csdr_amd_convert_f_s8 (csdr_amd_ctx *ctx, const float *in, int8_t *out, size_t n);
int csdr_amd_convert_f_s16(csdr_amd_ctx *ctx, const float *in, int16_t *out, size_t n);
int csdr_amd_convert_f_s24(csdr_amd_ctx *ctx, const float *in, uint8_t *out, size_t n, int bigendian);
int csdr_amd_convert_s24_f(csdr_amd_ctx *ctx, const uint8_t *in, float *out, size_t n, int bigendian);

/* ------------------------------------------------------------------ frequency shifters
 * All shifter variants are "rotator generators" (the variant's own float32 phase bookkeeping replayed
 * exactly on the device) feeding one mixing kernel.  The rotator table rot[0..n) is shared by every
 * stream that has the same rate and starting phase.
 *
 * phase_io: HOST float; read as the starting phase, overwritten with the phase after n samples (the reference
 * returns it by value: libcsdr_gpl.c:48-51, libcsdr.c:206, 302-304).  The float32 phase recurrences are strictly
 * sequential and data independent; they run on the host (identical IEEE arithmetic) and are uploaded, the
 * device does the parallel part (sin/cos, per-chunk phasor replay, mixing).  Calls do not block on the GPU. */
enum {
    CSDR_SHIFT_ADDITION = 0,   /* shift_addition_cc  libcsdr_gpl.c:27-52, 1024-chunks per csdr.c:911-918 */
    CSDR_SHIFT_MATH     = 1,   /* shift_math_cc      libcsdr.c:186-207 */
    CSDR_SHIFT_TABLE    = 2,   /* shift_table_cc     libcsdr.c:229-265 (aux = table_size) */
    CSDR_SHIFT_UNROLL   = 3,   /* shift_unroll_cc    libcsdr.c:268-305 (aux = table size = chunk, csdr.c:821) */
    CSDR_SHIFT_ADDFAST  = 4    /* shift_addfast_cc   libcsdr.c:307-317, 406-434, 1024-chunks csdr.c:785 */
};
int csdr_amd_rotator_generate(csdr_amd_ctx *ctx, int variant, float rate, float *phase_io,
                              csdr_complexf *rot, size_t n, int chunk, int aux);
/* MATH / TABLE: the number of calls on this context that found their phase scan done by the call before (same rate, same n, the
 * phase that call handed back; either of the two variants); the twin of csdr_amd_shiftbank_scans_ahead */
long long csdr_amd_debug_shift_scans_ahead(csdr_amd_ctx *ctx);
/* out[s][k] = in[s][k] * rot[k]   (four float products, two sums, no FMA contraction).  csdr_amd_mix_cc, csdr_amd_mix_fc and
 * csdr_amd_shift_cc take at most 65535 streams a call (one grid row each): more is refused with -3 and nothing is launched */
int csdr_amd_mix_cc(csdr_amd_ctx *ctx, const csdr_complexf *in, csdr_complexf *out, const csdr_complexf *rot,
                    int n_streams, size_t n, size_t in_pitch, size_t out_pitch);
/* real input variant: shift_addition_fc libcsdr_gpl.c:54-79 */
int csdr_amd_mix_fc(csdr_amd_ctx *ctx, const float *in, csdr_complexf *out, const csdr_complexf *rot,
                    int n_streams, size_t n, size_t in_pitch, size_t out_pitch);
/* convenience: generate + mix with context scratch */
int csdr_amd_shift_cc(csdr_amd_ctx *ctx, int variant, float rate, float *phase_io,
                      const csdr_complexf *in, csdr_complexf *out, int n_streams, size_t n,
                      size_t in_pitch, size_t out_pitch, int chunk, int aux);

/* decimating_shift_addition_cc (libcsdr_gpl.c:131-160), one call per stream-block.
 * dsa_data: device array of n_streams {sindelta, cosdelta, rate} = shift_addition_data_t (libcsdr_gpl.h:26-31) as
 * returned by decimating_shift_addition_init (csdr_amd_shift_addition_init(rate*decimation) on the host).
 * status_io: device int32[3*n_streams] = {decimation_remain, float bits of starting_phase, output_size}
 * laid out exactly like decimating_shift_addition_status_t (libcsdr_gpl.h:39-44). */
int csdr_amd_decimating_shift_addition_cc(csdr_amd_ctx *ctx, const csdr_complexf *in, csdr_complexf *out,
                                          int n_streams, int input_size, size_t in_pitch, size_t out_pitch,
                                          const void *dsa_data, int decimation, void *status_io);
/* shift_addition_init libcsdr_gpl.c:81-89 (host): out3 = {sindelta, cosdelta, 2*rate} */
void csdr_amd_shift_addition_init(float rate, float *out3);

/* ------------------------------------------------------------------ FIR decimator
 * fir_decimate_cc libcsdr.c:528-549: out[s][o] = sum_t in[s][D*o+t]*taps[t] for all o with D*o+taps<=input_size.
 * Returns the number of outputs per stream (>=0) or a negative error.  taps: DEVICE pointer. */
/* the kernel the calling thread's last csdr_amd_fir_decimate_cc launched: k_fir_poly (short filters), k_fir_mfma3 / k_fir_mfma (long filters on the fp32 matrix cores),
 * k_fir_generic */
const char *csdr_amd_fir_last_kernel(void);
/* the template instance behind it: k_fir_poly<R4,U24> / <R4,U44> / <R2,U24> / <R2,U44>, k_fir_mfma<NT,NS>, k_fir_mfma3<MAXB>, k_fir_generic ("" before the first call) */
const char *csdr_amd_fir_last_instance(void);
/* the same for the calling thread's last csdr_amd_fir_ff: a k_fir_poly<R,U> instance or k_fir_generic */
const char *csdr_amd_fir_ff_last_instance(void);
int csdr_amd_fir_decimate_cc(csdr_amd_ctx *ctx, const csdr_complexf *in, csdr_complexf *out,
                             int n_streams, int input_size, size_t in_pitch, size_t out_pitch,
                             int decimation, const float *taps, int taps_length);
/* real FIR without decimation = deemphasis_nfm_ff libcsdr.c:1101-1128 (outputs for i < input_size-taps_length).
 * Returns outputs per stream. */
int csdr_amd_fir_ff(csdr_amd_ctx *ctx, const float *in, float *out, int n_streams, int input_size,
                    size_t in_pitch, size_t out_pitch, const float *taps, int taps_length);

/* ------------------------------------------------------------------ demod / audio
 * fmdemod_quadri_cf libcsdr.c:1040-1071.  last_io: device complexf[n_streams] (in: previous block's last
 * sample, out: this block's last sample). */
int csdr_amd_fmdemod_quadri_cf(csdr_amd_ctx *ctx, const csdr_complexf *in, float *out, int n_streams,
                               size_t n, size_t in_pitch, size_t out_pitch, csdr_complexf *last_io);
/* limit_ff / gain_ff libcsdr.c:1130-1142 (flat arrays) */
int csdr_amd_limit_ff(csdr_amd_ctx *ctx, const float *in, float *out, size_t n, float max_amplitude);
int csdr_amd_gain_ff(csdr_amd_ctx *ctx, const float *in, float *out, size_t n, float gain);
/* the kernel path the calling thread's last call of one of these three took ("" before the first): csdr_amd_deemphasis_wfm_ff: k_deemph_wfm, k_deemph_wfm_spec<1> /
 * <2> / <4> / <8>; csdr_amd_agc_ff: k_agc, k_agc_coop; csdr_amd_fractional_decimator_ff: fracdec:exact (plan on the device), fracdec:walked (host walk),
 * fracdec:cached (the previous call's plan reused) */
const char *csdr_amd_audio_last_path(void);
/* deemphasis_wfm_ff libcsdr.c:1081-1097.  last_io: device float[n_streams]. */
int csdr_amd_deemphasis_wfm_ff(csdr_amd_ctx *ctx, const float *in, float *out, int n_streams, size_t n,
                               size_t in_pitch, size_t out_pitch, float tau, int sample_rate, float *last_io);
/* fastagc_ff libcsdr.c:946-991 over n_blocks consecutive blocks per stream.
 * state_io: device float[n_streams * (2*block + 4)] = {buffer_1[block], buffer_2[block], peak_1, peak_2,
 * last_gain, pad}; zero-initialised = the CLI's calloc'ed state (csdr.c:1393-1394). */
int csdr_amd_fastagc_ff(csdr_amd_ctx *ctx, const float *in, float *out, int n_streams, int n_blocks, int block,
                        size_t in_pitch, size_t out_pitch, float reference, float *state_io);

/* fractional_decimator_ff libcsdr.c:715-793 (Lagrange, optional FIR prefilter).  The float `where`
 * bookkeeping is data independent, so the plan (sample indices + interpolation coefficients) is built on the
 * host with the reference's float arithmetic and applied to all streams by one kernel.
 * state: opaque host object carrying where/input_processed between calls. */
typedef struct csdr_amd_fracdec csdr_amd_fracdec;
csdr_amd_fracdec *csdr_amd_fracdec_create(float rate, int num_poly_points, const float *host_taps, int taps_length);
void csdr_amd_fracdec_destroy(csdr_amd_fracdec *d);
/* returns outputs per stream; *input_processed receives the reference's d->input_processed */
int csdr_amd_fractional_decimator_ff(csdr_amd_ctx *ctx, csdr_amd_fracdec *d, const float *in, float *out,
                                     int n_streams, int input_size, size_t in_pitch, size_t out_pitch,
                                     int *input_processed);
void  csdr_amd_fracdec_set_where(csdr_amd_fracdec *d, float where);   /* fractional_decimator_ff_t.where */
/* the_bufsize > 0: csdr_amd_fractional_decimator_ff replays the CLI's loop (csdr.c:1511-1524: the function is called on the_bufsize-sample windows,
 * the unprocessed tail is re-presented) over the given input instead of one call over the whole array; 0 (default) = one call = the library function */
void  csdr_amd_fracdec_set_cli_bufsize(csdr_amd_fracdec *d, int the_bufsize);
float csdr_amd_fracdec_get_where(const csdr_amd_fracdec *d);

/* ------------------------------------------------------------------ FIR resamplers (resampler.hip)
 * rational_resampler_ff libcsdr.c:607-640 (interpolation I, decimation D, taps T long, typically from csdr_amd_rational_resampler_get_lowpass_f) and
 * fir_interpolate_cc libcsdr.c:579-605, for n_streams streams in lockstep.  The objects keep each stream's recent input on the device, so a stream may be cut into
 * calls anywhere (also 0- and 1-sample calls) without changing a bit of the output.
 * Streaming (default): the output equals the reference function applied once to the whole stream seen since the last reset.
 * set_cli_bufsize(B > 0): the output equals the reference CLI's stream at that buffer size -- `csdr rational_resampler_ff` (csdr.c:1441-1459: B-sample windows,
 * the state of the last computed output carried when a window hits its output cap, whose output then repeats), `csdr fir_interpolate_cc` (csdr.c:1215-1231:
 * B zeros in front of the stream).  Setting it resets the object; 0 goes back to streaming.
 * process: n_in new samples per stream (device, in_pitch elements apart) -> *n_out outputs per stream (out_pitch elements apart; at most *_max_out(n_in)).
 * kernel_name: what the last call ran ("k_rr_poly" / "k_rr_generic", "k_interp_poly" / "k_interp_generic"); force_generic(1) takes the generic kernel always. */
typedef struct csdr_amd_resampler csdr_amd_resampler;
csdr_amd_resampler *csdr_amd_resampler_create(csdr_amd_ctx *ctx, int interpolation, int decimation, const float *host_taps, int taps_length, int n_streams);
int  csdr_amd_resampler_process(csdr_amd_resampler *r, const float *in, long long n_in, size_t in_pitch, float *out, size_t out_pitch, long long *n_out);
long long csdr_amd_resampler_max_out(const csdr_amd_resampler *r, long long n_in);
int  csdr_amd_resampler_reset(csdr_amd_resampler *r);
int  csdr_amd_resampler_set_cli_bufsize(csdr_amd_resampler *r, int the_bufsize);
int  csdr_amd_resampler_force_generic(csdr_amd_resampler *r, int on);
/* the incoming last_taps_delay (0 <= d < I) of the stream's first output (or first CLI window): call after create / reset / set_cli_bufsize */
int  csdr_amd_resampler_set_last_taps_delay(csdr_amd_resampler *r, int last_taps_delay);
/* what one rational_resampler_ff call over input_size samples returns, without the samples: state = {input_processed, output_size, last_taps_delay}
 * (libcsdr.c:616-639, both loop exits; the outputs themselves are those of a set_cli_bufsize(input_size) object fed input_size samples) */
int  csdr_amd_resampler_window(int interpolation, int decimation, int taps_length, int input_size, int last_taps_delay, int *state);
const char *csdr_amd_resampler_kernel_name(const csdr_amd_resampler *r);
void csdr_amd_resampler_destroy(csdr_amd_resampler *r);
typedef struct csdr_amd_interp csdr_amd_interp;
csdr_amd_interp *csdr_amd_interp_create(csdr_amd_ctx *ctx, int interpolation, const float *host_taps, int taps_length, int n_streams);
int  csdr_amd_interp_process(csdr_amd_interp *p, const csdr_complexf *in, long long n_in, size_t in_pitch, csdr_complexf *out, size_t out_pitch, long long *n_out);
long long csdr_amd_interp_max_out(const csdr_amd_interp *p, long long n_in);
int  csdr_amd_interp_reset(csdr_amd_interp *p);
int  csdr_amd_interp_set_cli_bufsize(csdr_amd_interp *p, int the_bufsize);
int  csdr_amd_interp_force_generic(csdr_amd_interp *p, int on);
const char *csdr_amd_interp_kernel_name(const csdr_amd_interp *p);
void csdr_amd_interp_destroy(csdr_amd_interp *p);
/* rational_resampler_get_lowpass_f libcsdr.c:665-673 (host) */
void csdr_amd_rational_resampler_get_lowpass_f(float *output, int output_size, int interpolation, int decimation, int window);
/* Host-side schedule of rational_resampler_ff from an incoming last_taps_delay: out[3k..3k+2] = (startingi, delayi, taps used) of output k, k < n
 * (libcsdr.c:621-626).  The kernels' tables are built from the same recurrence. */
int  csdr_amd_debug_resampler_schedule(int interpolation, int decimation, int taps_length, int last_taps_delay, int n, int *out);

/* ------------------------------------------------------------------ BPSK31 receive chain (psk31.hip)
 * simple_agc_cc libcsdr.c:2201-2217 | timing_recovery_cc libcsdr.c:1977-2075 | dbpsk_decoder_c_u8 libcsdr.c:2319-2333 | psk31_varicode_decoder_u8_u8 csdr.c:2418-2431,
 * for n_channels channels, all with the same parameters.  The object runs the stages first_stage .. last_stage (CSDR_AMD_PSK31_*) in one launch and keeps each
 * channel's state on the device: the gain (starting at 1, as the CLI), the samples timing recovery has not consumed yet (< 3 D/2 + 1), correction_offset,
 * the last symbol (starting at 0 + 0i) and the varicode shift register.  The output equals the reference functions applied once to the whole stream since the
 * last reset, however the stream is cut into calls (0- and 1-sample calls included) and whatever a channel's position in the batch.
 * params: rate, reference, max_gain > 0 (AGC); algorithm 0 = GARDNER, 1 = EARLYLATE; decimation > 4 and a multiple of 4; |loop_gain| * max_error <= 1
 * (OpenWebRX: 0.5 * 2); use_q = the CLI's --add_q.
 * process: n_in new items per channel (complexf, or one byte per bit when first_stage is VARICODE), in_pitch items apart; out: complexf (last_stage AGC or
 * TIMING) or bytes (DBPSK: one bit per byte; VARICODE: the decoded characters, NUL and "no character" left out), out_pitch items apart, at least
 * max_out(n_in); counts (device, n_channels ints) receives each channel's output count.  err / idx (device, may be NULL; last_stage TIMING only, out_pitch
 * apart): the unclamped timing error and the absolute sample index (unsigned, wrapping, as --output_error / --output_indexes) of each symbol.
 * Asynchronous on the context's stream.  kernel_name: "k_psk31_tiled" (the fused range: first_stage AGC, last_stage TIMING or later, the ring of
 * 3 D/2 + 66 samples per channel within 63 KiB of LDS) or "k_psk31" (every other case); force_generic(1) takes k_psk31 always.
 * set_lanes(n): channels per wave (0: automatic; k_psk31_tiled takes at most 16; every choice gives the same bits).
 * Timing recovery needs |loop_gain| * max_error <= 1, so that a symbol moves on by D/2 .. 3D/2 samples (the reference accepts more; its loop can then
 * step backwards and read before its buffer).
 * get_channel / set_channel: one channel's state (synchronous). */
enum { CSDR_AMD_PSK31_AGC = 0, CSDR_AMD_PSK31_TIMING = 1, CSDR_AMD_PSK31_DBPSK = 2, CSDR_AMD_PSK31_VARICODE = 3 };
typedef struct csdr_amd_psk31_params {
    float rate, reference, max_gain;     /* simple_agc_cc */
    int algorithm, decimation;           /* timing_recovery_cc */
    float loop_gain, max_error;
    int use_q;
} csdr_amd_psk31_params;
typedef struct csdr_amd_psk31_chan {
    float gain;                          /* first_stage AGC: the gain in front of the unconsumed tail (AGC alone: after the last sample) */
    int tail_len, correction_offset;
    unsigned base;                       /* absolute index of the tail's first sample */
    float last_i, last_q;                /* dbpsk_decoder_c_u8's last_input */
    unsigned long long varicode_shr;
} csdr_amd_psk31_chan;
typedef struct csdr_amd_psk31 csdr_amd_psk31;
csdr_amd_psk31 *csdr_amd_psk31_create(csdr_amd_ctx *ctx, const csdr_amd_psk31_params *params, int n_channels, int first_stage, int last_stage);
int  csdr_amd_psk31_process(csdr_amd_psk31 *p, const void *in, long long n_in, size_t in_pitch, void *out, size_t out_pitch, int *counts, float *err, unsigned *idx);
long long csdr_amd_psk31_max_out(const csdr_amd_psk31 *p, long long n_in);
int  csdr_amd_psk31_reset(csdr_amd_psk31 *p);
int  csdr_amd_psk31_reset_channel(csdr_amd_psk31 *p, int channel);
int  csdr_amd_psk31_get_channel(csdr_amd_psk31 *p, int channel, csdr_amd_psk31_chan *state);
int  csdr_amd_psk31_set_channel(csdr_amd_psk31 *p, int channel, const csdr_amd_psk31_chan *state);
int  csdr_amd_psk31_set_lanes(csdr_amd_psk31 *p, int lanes);
int  csdr_amd_psk31_force_generic(csdr_amd_psk31 *p, int on);
int  csdr_amd_psk31_lanes(const csdr_amd_psk31 *p);
const char *csdr_amd_psk31_kernel_name(const csdr_amd_psk31 *p);
void csdr_amd_psk31_destroy(csdr_amd_psk31 *p);
/* simple_agc_cc libcsdr.c:2201-2217 on n_streams streams of n samples; gain_io (device, n_streams floats) carries each stream's gain in and out */
int  csdr_amd_simple_agc_cc(csdr_amd_ctx *ctx, const csdr_complexf *in, csdr_complexf *out, int n_streams, long long n, size_t in_pitch, size_t out_pitch,
                            float rate, float reference, float max_gain, float *gain_io);
/* psk31_varicode_decoder_push libcsdr.c:1536-1549 (host, one bit per call) and the varicode table: out[2a], out[2a + 1] = code, length of character a < 128 */
char csdr_amd_psk31_varicode_decoder_push(unsigned long long *status_shr, unsigned char symbol);
void csdr_amd_psk31_varicode_table(int *out);
/* CPU run of k_psk31's walk (the same step functions) for one channel, the n items cut into calls of cuts[0..n_cuts) items and the rest; outputs concatenated.
 * state_io: the channel state in and out (NULL: a fresh channel).  Returns the output count. */
long long csdr_amd_debug_psk31_walk(const csdr_amd_psk31_params *params, int first_stage, int last_stage, const void *in, long long n, const long long *cuts,
                                    int n_cuts, void *out, float *err, unsigned *idx, csdr_amd_psk31_chan *state_io);

/* ------------------------------------------------------------------ BPSK31 transmit chain (psk31tx.hip)
 * psk31_varicode_encoder_u8_u8 libcsdr.c:1551-1575 | differential_encoder_u8_u8 libcsdr.c:1836-1841 | psk_modulator_u8_c libcsdr.c:1772-1782 |
 * psk31_interpolate_sine_cc libcsdr.c:1793-1808, for n_channels channels with the same n_psk (1..256) and interpolation (>= 1).  The object runs the stages
 * first_stage .. last_stage (CSDR_AMD_PSK31TX_*) and keeps each channel's state on the device: the differential state (0 after a reset, csdr.c:2823) and the
 * shaper's last symbol (0 + 0i after a reset, csdr.c:2736-2738).  The output equals the reference functions applied once to each channel's whole stream since
 * its last reset, however the stream is cut into calls (0- and 1-item calls included) and wherever the channel sits in the batch.
 * process: n_in items per channel, in_pitch items apart: bytes (characters for VARICODE, bits for DIFF, symbol indexes for MOD) or complexf (SHAPE).
 * in_counts (device, n_channels ints, may be NULL = n_in for every channel): each channel's item count of this call, 0 .. n_in (a value outside is clamped
 * on the device; a caller that holds the counts on the host checks them there).  out: bytes (last_stage VARICODE or DIFF) or complexf (MOD or SHAPE),
 * out_pitch items apart, at least max_out(n_in) = n_in (x 12 from VARICODE: a character is at most 12 bits) (x interpolation to SHAPE), at most 2^31 - 1:
 * a smaller out_pitch is an error, so input is never left unconsumed.  counts (device, n_channels ints) receives each channel's output count; nothing is
 * written at or beyond it.  Bytes 128..255 have no varicode and produce nothing.  Asynchronous on the context's stream.
 * kernel_name: "k_psk31tx_plan+k_psk31tx_shape" (the range VARICODE .. SHAPE with interpolation <= 7904, the tables' bound in 63 KiB of LDS) or
 * "k_psk31tx_generic" (every other case); force_generic(1) takes k_psk31tx_generic always.  Both give the same bits.
 * get_channel / set_channel: one channel's state (synchronous).  diff_state is any byte, as differential_codec takes it (a byte above 1 is output until
 * the first toggle makes it 0), except for the range VARICODE .. SHAPE, which takes 0 or 1. */
enum { CSDR_AMD_PSK31TX_VARICODE = 0, CSDR_AMD_PSK31TX_DIFF = 1, CSDR_AMD_PSK31TX_MOD = 2, CSDR_AMD_PSK31TX_SHAPE = 3 };
typedef struct csdr_amd_psk31tx_chan {
    unsigned char diff_state;            /* DIFF */
    float last_i, last_q;                /* SHAPE: the last symbol */
} csdr_amd_psk31tx_chan;
typedef struct csdr_amd_psk31tx csdr_amd_psk31tx;
csdr_amd_psk31tx *csdr_amd_psk31tx_create(csdr_amd_ctx *ctx, int n_channels, int n_psk, int interpolation, int first_stage, int last_stage);
int  csdr_amd_psk31tx_process(csdr_amd_psk31tx *p, const void *in, long long n_in, const int *in_counts, size_t in_pitch, void *out, size_t out_pitch, int *counts);
long long csdr_amd_psk31tx_max_out(const csdr_amd_psk31tx *p, long long n_in);
int  csdr_amd_psk31tx_reset(csdr_amd_psk31tx *p);
int  csdr_amd_psk31tx_reset_channel(csdr_amd_psk31tx *p, int channel);
int  csdr_amd_psk31tx_get_channel(csdr_amd_psk31tx *p, int channel, csdr_amd_psk31tx_chan *state);
int  csdr_amd_psk31tx_set_channel(csdr_amd_psk31tx *p, int channel, const csdr_amd_psk31tx_chan *state);
int  csdr_amd_psk31tx_force_generic(csdr_amd_psk31tx *p, int on);
const char *csdr_amd_psk31tx_kernel_name(const csdr_amd_psk31tx *p);
void csdr_amd_psk31tx_destroy(csdr_amd_psk31tx *p);
/* The tables an object with these parameters is created with (host): sym = the 256 symbols of psk_modulator_u8_c, (cos, sin) of float(2 pi / n_psk) * v by
 * libm in double, rounded to float; rate = the `interpolation` factors of psk31_interpolate_sine_cc.  Either may be NULL. */
int  csdr_amd_psk31tx_tables(int n_psk, int interpolation, csdr_complexf *sym, float *rate);
/* differential_codec's decode branch (libcsdr.c:1830-1835) on n_streams streams of n bytes: out = (in == the previous in); state_io (device, n_streams bytes)
 * carries each stream's previous byte in and out.  out must not be in. */
int  csdr_amd_differential_decoder_u8_u8(csdr_amd_ctx *ctx, const unsigned char *in, unsigned char *out, int n_streams, long long n, size_t in_pitch,
                                         size_t out_pitch, unsigned char *state_io);
/* duplicate_samples_ntimes_u8_u8 (libcsdr.c:1784-1791) on n_streams streams: every whole sample of sample_size_bytes within n_bytes, written ntimes */
int  csdr_amd_duplicate_samples_ntimes_u8_u8(csdr_amd_ctx *ctx, const unsigned char *in, unsigned char *out, int n_streams, long long n_bytes, size_t in_pitch,
                                             size_t out_pitch, int sample_size_bytes, int ntimes);
/* CPU run of k_psk31tx_generic's walk (the same step functions) for one channel, the n items cut into calls of cuts[0..n_cuts) items and the rest; outputs
 * concatenated.  state_io: the channel state in and out (NULL: a fresh channel).  Returns the output count. */
long long csdr_amd_debug_psk31tx_walk(int n_psk, int interpolation, int first_stage, int last_stage, const void *in, long long n, const long long *cuts,
                                      int n_cuts, void *out, csdr_amd_psk31tx_chan *state_io);

/* ------------------------------------------------------------------ pulse-shaped symbol modem (modem.hip)
 * Transmit: psk_modulator_u8_c n_psk libcsdr.c:1772-1782 | plain_interpolate_cc I libcsdr.c:2499-2506 | pulse_shaping_filter_cc = apply_real_fir_cc
 * libcsdr.c:2276-2291 (csdr.c:3159-3254), for n_channels channels with the same n_psk (1..256), interpolation I (>= 1) and T real taps (host pointer, copied).
 * With c[m] a channel's symbols since its last reset, x[j] = c[j / I] where I divides j and 0 elsewhere, the stream is y[i] = sum over t < T of x[i + t] *
 * taps[t]: after n symbols in total it holds exactly the outputs i = 0 .. n I - T (the zeros behind the last symbol are input), max(0, n I - T + 1) of them.
 * The nonzero products of an output (t = (-i) mod I, + I, ...) are accumulated in ascending t with fmaf; a phase without a tap (T < I) gives 0 + 0i.  The
 * output does not depend on how the stream is cut into calls (0- and 1-symbol calls included) nor on where a channel sits in the batch.
 * The object runs the stages first_stage .. last_stage: MOD .. MOD is psk_modulator_u8_c alone (taps may be NULL); SHAPE .. SHAPE takes complexf symbols (any
 * constellation).  Symbols: the table of csdr_amd_psk31tx_tables.  State: the number of symbols taken (the same for every channel) and, on the device, each
 * channel's last ceil((T - 1) / I) symbols.
 * process: n_in symbols per channel, in_pitch items apart (bytes from MOD, complexf from SHAPE); out: complexf, out_pitch apart, at least max_out(n_in) = n_in
 * (x I to SHAPE), at most 2^31 - 1: a smaller out_pitch is an error and consumes nothing.  *n_out (host) receives the outputs per channel of this call;
 * nothing is written at or beyond it.  Asynchronous on the context's stream.
 * kernel_name: "k_pulsetx_poly" (taps and a tile's symbols within 63 KiB of LDS: 4 K I + 8 (4096 / I + K + 4) bytes, K = ceil(T / I)) or "k_pulsetx_generic"
 * (every other shape, MOD .. MOD, and after force_generic(1)).  Both give the same bits.  tile: the symbols per tile of k_pulsetx_poly, max(1, 4096 / I). */
enum { CSDR_AMD_PULSETX_MOD = 0, CSDR_AMD_PULSETX_SHAPE = 1 };
typedef struct csdr_amd_pulsetx csdr_amd_pulsetx;
csdr_amd_pulsetx *csdr_amd_pulsetx_create(csdr_amd_ctx *ctx, int n_channels, int n_psk, int interpolation, const float *host_taps, int taps_length,
                                          int first_stage, int last_stage);
int  csdr_amd_pulsetx_process(csdr_amd_pulsetx *p, const void *in, long long n_in, size_t in_pitch, void *out, size_t out_pitch, long long *n_out);
long long csdr_amd_pulsetx_max_out(const csdr_amd_pulsetx *p, long long n_in);
int  csdr_amd_pulsetx_reset(csdr_amd_pulsetx *p);
int  csdr_amd_pulsetx_force_generic(csdr_amd_pulsetx *p, int on);
const char *csdr_amd_pulsetx_kernel_name(const csdr_amd_pulsetx *p);
int  csdr_amd_pulsetx_tile(const csdr_amd_pulsetx *p);
void csdr_amd_pulsetx_destroy(csdr_amd_pulsetx *p);
/* CPU run of the object's definition (the same step functions) for one channel, the n items cut into calls of cuts[0..n_cuts) items and the rest; outputs
 * concatenated.  Returns the output count. */
long long csdr_amd_debug_pulsetx_walk(int n_psk, int interpolation, const float *taps, int taps_length, int first_stage, int last_stage, const void *in,
                                      long long n, const long long *cuts, int n_cuts, void *out);
/* Receive: pulse_shaping_filter_cc as the matched filter (apply_real_fir_cc libcsdr.c:2276-2291) | timing_recovery_cc libcsdr.c:1977-2072 | [realpart_cf |]
 * gain_ff libcsdr.c:1139-1142 | generic_slicer_f_u8 libcsdr.c:1731-1765, for n_channels channels with the same parameters.  With x a channel's complexf input
 * since its last reset: FILTER gives f[i] = sum over t < T of x[i + t] taps[t], i = 0 .. n - T (no zeros in front); from first_stage TIMING on, f = x with its
 * bits kept and the taps are not read.  TIMING is timing_recovery_cc applied once to the whole of f (GARDNER 0 / EARLYLATE 1, use_q, loop_gain, max_error with
 * |loop_gain| max_error <= 1, decimation >= 2: the library function's range, wider than the command line's).  SLICE: slice_q 0 is realpart_cf |
 * gain_ff gain | generic_slicer_f_u8 n_symbols, one byte per symbol; slice_q 1 is gain_ff | generic_slicer_f_u8 on the complexf symbols read as interleaved floats, two bytes per symbol (I, Q).
 * f is never stored: it is evaluated only at the three positions the timing loop reads per symbol.  The order of the T products is part of the definition (a
 * float is truncated to an int in the loop): 16 partial sums over t = r (mod 16), each in ascending t with fmaf from 0, then p[r] += p[r + s] for r < s,
 * s = 8, 4, 2, 1.  Both kernels and the debug walk run that order and give the same bits.  The output does not depend on how the stream is cut into calls
 * (0- and 1-sample calls included) nor on where a channel sits in the batch.  State per channel: the raw unconsumed tail (from the current symbol start on,
 * at most 3 D/2 + T - 1 samples, kept on the device), its length, correction_offset, and base, the absolute index of the tail's first sample.
 * process: n_in complexf per channel, in_pitch items apart; out: complexf symbols (last_stage TIMING) or bytes (SLICE), out_pitch items apart, at least
 * max_out(n_in): a smaller out_pitch is an error and consumes nothing.  counts (device, n_channels ints) receives each channel's output count (bytes from
 * SLICE).  err / idx (device, optional, last_stage TIMING only): the unclamped timing error and the absolute sample index per symbol.  Asynchronous.
 * kernel_name: "k_pulserx_tiled" (a one-wave workgroup per 16, 8, 4, 2 or 1 channels with 4, 8 or 16 lanes per channel; per channel a ring of the next
 * power of two >= 3 D/2 + T + 127 samples, with the taps and the byte staging within 63 KiB of LDS) or "k_pulserx_generic" (one lane per channel; every
 * other shape and after force_generic(1)).  set_lanes(n): channels per wave, 0 automatic; k_pulserx_tiled takes the largest of 16, 8, 4, 2, 1 within n,
 * the next smaller of them where the rings do not fit.  Every choice gives the same bits. */
enum { CSDR_AMD_PULSERX_FILTER = 0, CSDR_AMD_PULSERX_TIMING = 1, CSDR_AMD_PULSERX_SLICE = 2 };
typedef struct csdr_amd_pulserx_params {
    const float *taps; int taps_length;                  /* host taps (copied); not read from first_stage TIMING on */
    int algorithm, decimation;
    float loop_gain, max_error;
    int use_q;
    float gain;                                          /* gain_ff's factor in front of the slicer */
    int n_symbols, slice_q;                              /* generic_slicer_f_u8's n_symbols (2..256); both needed to last_stage SLICE only */
} csdr_amd_pulserx_params;
typedef struct csdr_amd_pulserx_chan {
    int tail_len;
    int correction_offset;
    unsigned base;
} csdr_amd_pulserx_chan;
typedef struct csdr_amd_pulserx csdr_amd_pulserx;
csdr_amd_pulserx *csdr_amd_pulserx_create(csdr_amd_ctx *ctx, const csdr_amd_pulserx_params *params, int n_channels, int first_stage, int last_stage);
int  csdr_amd_pulserx_process(csdr_amd_pulserx *p, const csdr_complexf *in, long long n_in, size_t in_pitch, void *out, size_t out_pitch, int *counts, float *err,
                              unsigned *idx);
long long csdr_amd_pulserx_max_out(const csdr_amd_pulserx *p, long long n_in);
int  csdr_amd_pulserx_reset(csdr_amd_pulserx *p);
int  csdr_amd_pulserx_reset_channel(csdr_amd_pulserx *p, int channel);
int  csdr_amd_pulserx_get_channel(csdr_amd_pulserx *p, int channel, csdr_amd_pulserx_chan *state);
int  csdr_amd_pulserx_set_channel(csdr_amd_pulserx *p, int channel, const csdr_amd_pulserx_chan *state);
int  csdr_amd_pulserx_set_lanes(csdr_amd_pulserx *p, int lanes);
int  csdr_amd_pulserx_lanes(const csdr_amd_pulserx *p);
int  csdr_amd_pulserx_force_generic(csdr_amd_pulserx *p, int on);
const char *csdr_amd_pulserx_kernel_name(const csdr_amd_pulserx *p);
void csdr_amd_pulserx_destroy(csdr_amd_pulserx *p);
/* CPU run of the object's walk (the same step functions) for one channel, the n samples cut into calls of cuts[0..n_cuts) samples and the rest; outputs
 * concatenated.  state_io (may be NULL: a fresh channel) carries the channel state in and out; a state with a tail cannot be carried in (the tail is not
 * part of the record).  Returns the output count. */
long long csdr_amd_debug_pulserx_walk(const csdr_amd_pulserx_params *params, int first_stage, int last_stage, const csdr_complexf *in, long long n,
                                      const long long *cuts, int n_cuts, void *out, float *err, unsigned *idx, csdr_amd_pulserx_chan *state_io);
/* generic_slicer_f_u8 libcsdr.c:1731-1765 on n_streams streams of n floats, n_symbols 2..256: symbol j's centre is -1 + j d with d = (float)(2.0 / (n_symbols - 1)),
 * its limits centre -/+ d / 2, all in float as the reference computes them; the first symbol has no lower and the last no upper limit.  An input that no symbol
 * claims gives 0: NaN (the reference leaves that output byte unwritten), and a value in a rounding gap between two neighbours' limits. */
int  csdr_amd_generic_slicer_f_u8(csdr_amd_ctx *ctx, const float *in, unsigned char *out, int n_streams, long long n, size_t in_pitch, size_t out_pitch,
                                  int n_symbols);
/* plain_interpolate_cc libcsdr.c:2499-2506: out[i I] = in[i], zeros between; n inputs, n I outputs per stream.  out must not be in. */
int  csdr_amd_plain_interpolate_cc(csdr_amd_ctx *ctx, const csdr_complexf *in, csdr_complexf *out, int n_streams, long long n, size_t in_pitch, size_t out_pitch,
                                   int interpolation);
/* pack_bits_1to8_u8_u8 libcsdr.c:1810-1815: n bytes -> 8 n bytes per stream, a byte's bits LSB first.  pack_bits_8to1_u8_u8 libcsdr.c:1818-1827 applied to
 * every group of eight: n bytes (a multiple of 8) -> n / 8 bytes per stream, the first byte of a group the MSB, each byte taken as !!byte.  (They are not
 * inverses of each other.)  out must not be in. */
int  csdr_amd_pack_bits_1to8_u8_u8(csdr_amd_ctx *ctx, const unsigned char *in, unsigned char *out, int n_streams, long long n, size_t in_pitch, size_t out_pitch);
int  csdr_amd_pack_bits_8to1_u8_u8(csdr_amd_ctx *ctx, const unsigned char *in, unsigned char *out, int n_streams, long long n, size_t in_pitch, size_t out_pitch);
/* apply_real_fir_cc libcsdr.c:2276-2291: csdr_amd_fir_decimate_cc at decimation 1.  taps: DEVICE pointer.  Returns input_size - taps_length + 1 outputs per
 * stream (0 when input_size < taps_length) or a negative error. */
int  csdr_amd_apply_real_fir_cc(csdr_amd_ctx *ctx, const csdr_complexf *in, csdr_complexf *out, int n_streams, int input_size, size_t in_pitch, size_t out_pitch,
                                const float *taps, int taps_length);
/* firdes_rrc_f libcsdr.c:2482-2497 and firdes_cosine_f libcsdr.c:2473-2480 (host), normalize_fir_f included.  RRC: taps_length odd, otherwise an error (for an
 * even length the reference writes taps[taps_length]).  Cosine: meant for taps_length = 2 samples_per_symbol + 1; the taps the reference never writes (the two
 * end taps of that length) are 0. */
int  csdr_amd_firdes_rrc_f(float *taps, int taps_length, int samples_per_symbol, float beta);
int  csdr_amd_firdes_cosine_f(float *taps, int taps_length, int samples_per_symbol);

/* ------------------------------------------------------------------ the frame synchroniser (framesync.hip, framesync_dev.hpp)
 * pattern_search_u8_u8 <values_after> <pattern values> (csdr.c:3532-3597) for n_channels byte streams with the same pattern: behind every place where the last
 * pattern_length bytes equal the pattern, the next values_after bytes are output and the search starts over behind them.  It is the reference's loop byte by byte
 * (DESIGN section 4u): a ring of pattern_length bytes, a write index and a fill count; a match restarts the fill count and leaves the index where it stands,
 * so that the bytes which would land past the ring's end are dropped (one byte after a reset; the reference writes them beyond its buffer).  max_mismatch > 0
 * (not in the reference) accepts a window of which at most that many positions differ.  The result does not depend on how calls cut a stream, 0- and 1-byte
 * calls included, nor on the kernel.
 * create: pattern_length 1 .. 1024, values_after 0 .. 2^30, 0 <= max_mismatch < pattern_length, pattern values 0 .. 255 (a larger value cannot match a byte).
 * process: channel ch takes in_counts[ch] (DEVICE, clamped to 0 .. n_in; NULL: n_in) bytes from in + ch * in_pitch (device).  out (device, out_pitch >= max_out(n_in)
 * = n_in apart) receives the payload bytes of this call and out_counts[ch] (device) their number; frame_pos (device, may be NULL; frame_pitch >=
 * max_frames(n_in) = n_in / (pattern_length + 1) + 1 apart) receives per match of this call the absolute index, counted from the channel's last reset, of
 * the payload's first byte, and frame_counts[ch] (device, may be NULL) the matches.  A short pitch is an error that consumes nothing.  Asynchronous on the
 * context's stream.
 * kernel_name: "k_framesync_tiled" (one wave per channel, tiles of csdr_amd_framesync_tile() bytes staged in LDS) or "k_framesync_generic" (one lane per
 * channel on global memory; force_generic(1)).  set_lanes(n): channels per wave of k_framesync_generic (1 .. 64; 0: automatic); k_framesync_tiled always runs
 * one channel per wave, so lanes() is 1 for it.  get_channel / set_channel: one channel's record and, where `window` is not NULL, its pattern_length ring bytes (synchronous). */
typedef struct csdr_amd_framesync_chan {
    int fill;                            /* bytes since the (re)start, pattern_length at most */
    int index;                           /* where the next byte is stored: below pattern_length while checking, up to 2 pattern_length - 1 while filling */
    int remain;                          /* payload bytes left to copy */
    int reserved;
    long long base;                      /* bytes taken since the last reset */
    long long frames;                    /* matches since the last reset */
} csdr_amd_framesync_chan;
typedef struct csdr_amd_framesync csdr_amd_framesync;
int  csdr_amd_framesync_create(csdr_amd_ctx *ctx, int n_channels, const unsigned *pattern, int pattern_length, int values_after, int max_mismatch,
                               csdr_amd_framesync **out);
int  csdr_amd_framesync_process(csdr_amd_framesync *p, const unsigned char *in, size_t in_pitch, long long n_in, const int *in_counts, unsigned char *out,
                                size_t out_pitch, int *out_counts, long long *frame_pos, size_t frame_pitch, int *frame_counts);
long long csdr_amd_framesync_max_out(const csdr_amd_framesync *p, long long n_in);
long long csdr_amd_framesync_max_frames(const csdr_amd_framesync *p, long long n_in);
int  csdr_amd_framesync_tile(void);
int  csdr_amd_framesync_reset(csdr_amd_framesync *p);
int  csdr_amd_framesync_reset_channel(csdr_amd_framesync *p, int channel);
int  csdr_amd_framesync_get_channel(csdr_amd_framesync *p, int channel, csdr_amd_framesync_chan *state, unsigned char *window);
int  csdr_amd_framesync_set_channel(csdr_amd_framesync *p, int channel, const csdr_amd_framesync_chan *state, const unsigned char *window);
int  csdr_amd_framesync_set_lanes(csdr_amd_framesync *p, int lanes);
int  csdr_amd_framesync_lanes(const csdr_amd_framesync *p);
int  csdr_amd_framesync_force_generic(csdr_amd_framesync *p, int on);
const char *csdr_amd_framesync_kernel_name(const csdr_amd_framesync *p);
void csdr_amd_framesync_destroy(csdr_amd_framesync *p);
/* One stream with fresh state (all pointers device): *out_count (device) receives the payload bytes written to out (n at most). */
int  csdr_amd_pattern_search_u8_u8(csdr_amd_ctx *ctx, const unsigned char *in, long long n, const unsigned *pattern, int pattern_length, int values_after,
                                   unsigned char *out, int *out_count);
/* CPU run of the kernels' step function for one channel (host pointers), the n bytes cut into calls of cuts[0..n_cuts) bytes and the rest; payloads and
 * positions (may be NULL) concatenated.  state_io (may be NULL: a fresh channel) carries the record and window_io (pattern_length bytes, may be NULL with a
 * fresh channel) the ring in and out.  Returns the payload count; *n_frames (may be NULL) the matches. */
long long csdr_amd_debug_framesync_walk(const unsigned *pattern, int pattern_length, int values_after, int max_mismatch, const unsigned char *in, long long n,
                                        const long long *cuts, int n_cuts, unsigned char *out, long long *pos, long long *n_frames,
                                        csdr_amd_framesync_chan *state_io, unsigned char *window_io);

/* ------------------------------------------------------------------ RTTY receive chain (rtty.hip)
 * bfsk_demod_cf libcsdr.c:2335-2350 (csdr.c:3271-3300) | serial_line_decoder_f_u8 libcsdr.c:1662-1728 (csdr.c:2490-2528) | rtty_baudot2ascii_u8_u8 csdr.c:2461-2473,
 * for n_channels channels, all with the same parameters.  The object runs the stages first_stage .. last_stage (CSDR_AMD_RTTY_*) and keeps each channel's
 * state on the device: the last < L complex samples (the CLI keeps L - 1 between its windows, so its stream is the valid correlation over the whole input),
 * the < B discriminator samples the serial decoder has not consumed, and the letters / figures shift.  The serial decoder works in windows of cli_bufsize
 * (B) samples exactly as the CLI's bigbufs loop does: its output depends on B.  Only whole windows are decoded (no stale window at the end of a stream).
 * The output equals the stages applied once to the whole stream since the last reset, however the stream is cut into calls and whatever a channel's
 * position in the batch.
 * params: spacing and filter_length (> 0) for BFSK (mark filter at +spacing/2, space at -spacing/2, Hamming); samples_per_bits >= 1, databits 1 .. 8
 * (1 .. 32 when SERIAL is the last stage: 2- / 4-byte outputs above 8 and 16 bits, as the library function), stopbits >= 1, bit_sampling_width_ratio
 * 0 .. 1 (the CLI: 0.4), cli_bufsize B with 2 + samples_per_bits * (1 + databits + stopbits) < B (otherwise the reference CLI "gets stuck").
 * `window` is the bfsk_demod_cf CLI's buffer size; it changes no output.
 * process: n_in new items per channel (complexf for BFSK, float for SERIAL, bytes for BAUDOT), in_pitch items apart; out: float (last BFSK), the serial
 * decoder's characters (last SERIAL) or ASCII (last BAUDOT, NULs left out), out_pitch items apart, at least max_out(n_in); counts (device, n_channels
 * ints) receives each channel's output count.  Asynchronous on the context's stream.
 * kernel_name: the discriminator's kernel ("k_bfsk_mfma": the fp32 matrix cores, filters up to 256 taps; "k_bfsk_generic": one thread per output),
 * or, when the range starts behind it, "k_rtty_walk" (the serial decoder, one wave per channel) / "k_rtty_baudot" (Baudot alone).  force_generic(1) takes
 * k_bfsk_generic always: the same bits. */
enum { CSDR_AMD_RTTY_BFSK = 0, CSDR_AMD_RTTY_SERIAL = 1, CSDR_AMD_RTTY_BAUDOT = 2 };
typedef struct csdr_amd_rtty_params {
    float spacing;
    int filter_length;
    int window;                        /* bfsk_demod_cf */
    float samples_per_bits;
    int databits;
    float stopbits;
    float bit_sampling_width_ratio;    /* serial_line_decoder_f_u8; CLI defaults 8, 1, 0.4 */
    int cli_bufsize;                   /* B, default 16384 */
} csdr_amd_rtty_params;
typedef struct csdr_amd_rtty csdr_amd_rtty;
csdr_amd_rtty *csdr_amd_rtty_create(csdr_amd_ctx *ctx, const csdr_amd_rtty_params *params, int n_channels, int first_stage, int last_stage);
int  csdr_amd_rtty_process(csdr_amd_rtty *r, const void *in, long long n_in, size_t in_pitch, void *out, size_t out_pitch, int *counts);
long long csdr_amd_rtty_max_out(const csdr_amd_rtty *r, long long n_in);
int  csdr_amd_rtty_reset(csdr_amd_rtty *r);
int  csdr_amd_rtty_reset_channel(csdr_amd_rtty *r, int channel);
int  csdr_amd_rtty_force_generic(csdr_amd_rtty *r, int on);
const char *csdr_amd_rtty_kernel_name(const csdr_amd_rtty *r);
void csdr_amd_rtty_destroy(csdr_amd_rtty *r);
/* bfsk_demod_cf with caller taps (device, taps_length complexf each) on n_streams independent streams of n samples: n - taps_length + 1 outputs each
 * (none below that), stateless.  force_generic: k_bfsk_generic; csdr_amd_bfsk_last_kernel() names the kernel of the last call. */
int  csdr_amd_bfsk_demod_cf(csdr_amd_ctx *ctx, const csdr_complexf *in, float *out, int n_streams, long long n, size_t in_pitch, size_t out_pitch,
                            const csdr_complexf *mark_filter, const csdr_complexf *space_filter, int taps_length, int force_generic);
const char *csdr_amd_bfsk_last_kernel(void);
/* binary_slicer_f_u8 libcsdr.c:1767-1770: out = in > 0, on n_streams (<= 65535) rows */
int  csdr_amd_binary_slicer_f_u8(csdr_amd_ctx *ctx, const float *in, uint8_t *out, int n_streams, long long n, size_t in_pitch, size_t out_pitch);
/* rtty_line_decoder_u8_u8 csdr.c:2446-2458 (rtty_baudot_decoder_push libcsdr.c:1623-1655 per byte, NULs left out) on n_streams streams; state (device,
 * n_streams entries, zero = the CLI's fresh decoder) carries each stream's decoder; counts (device) receives each stream's output count */
typedef struct csdr_amd_rtty_push_state { int fig_mode, character_received, shr, bit_cntr, state; } csdr_amd_rtty_push_state;
int  csdr_amd_rtty_line_decoder_u8_u8(csdr_amd_ctx *ctx, const uint8_t *in, uint8_t *out, int n_streams, long long n, size_t in_pitch, size_t out_pitch,
                                      csdr_amd_rtty_push_state *state, int *counts);
/* serial_line_decoder_f_u8 libcsdr.c:1662-1728 as the library call: ONE window of n samples per stream (device arrays); out elements are 1, 2 or 4 bytes
 * (databits <= 8, <= 16, above); counts / used (device) receive output_size / input_used */
int  csdr_amd_serial_line_decoder_f_u8(csdr_amd_ctx *ctx, const float *in, void *out, int n_streams, int n, size_t in_pitch, size_t out_pitch,
                                       float samples_per_bits, int databits, float stopbits, float bit_sampling_width_ratio, int *counts, int *used);
/* rtty_baudot_decoder_lookup / _push libcsdr.c:1606-1655 on the host */
char csdr_amd_rtty_baudot_decoder_lookup(unsigned char *fig_mode, unsigned char c);
char csdr_amd_rtty_baudot_decoder_push(csdr_amd_rtty_push_state *s, unsigned char symbol);
/* firdes_add_peak_c libcsdr.c:2219-2257, and firdes_peak_c (csdr.c:2932-2972: add = 0, normalize = 1) */
void csdr_amd_firdes_add_peak_c(csdr_complexf *output, int length, float rate, int window, int add, int normalize);
void csdr_amd_firdes_peak_c(csdr_complexf *taps, int length, float rate, int window);
/* CPU run of the object's walk (the same step functions) for one channel, the n items cut into calls of cuts[0..n_cuts) items and the rest; outputs
 * concatenated.  Returns the output count (< 0: refused parameters, the reason in csdr_amd_last_error()). */
long long csdr_amd_debug_rtty_walk(const csdr_amd_rtty_params *params, int first_stage, int last_stage, const void *in, long long n, const long long *cuts,
                                   int n_cuts, void *out);

/* ------------------------------------------------------------------ complex-tap FIR (cfir.hip)
 * apply_fir_cc libcsdr.c:2261-2273: y[o] = sum_{t < T} x[o + t] h[t], complex x complex; n samples give n - T + 1 outputs (none below that, no zero
 * history).  Each part of an output is ONE fmaf chain over the 2 T interleaved tap floats, from 0 (cfir_dev.hpp): the matrix-core kernel, the generic
 * kernel and the CPU walk give the same bits for finite inputs, however a stream is cut into calls and whatever a channel's position in the batch.  (On
 * the matrix cores an Inf or NaN sample also reaches outputs of its group of 16 that do not use it: the tap band's zeros multiply it there.)
 * Stateless call: n_streams rows of n samples, in_pitch / out_pitch samples apart (rows 8-byte aligned); taps: DEVICE, taps_length complexf per row,
 * taps_pitch samples apart, taps_pitch == 0: one row for all streams.  taps_length 1 .. 65536.  Returns 0 or a negative error.
 * kernel names: "k_cfir_mfma" (the fp32 matrix cores, up to 256 taps), "k_cfir_generic" (one thread per output; force_generic takes it always). */
int  csdr_amd_apply_fir_cc(csdr_amd_ctx *ctx, const csdr_complexf *in, csdr_complexf *out, int n_streams, long long n, size_t in_pitch, size_t out_pitch,
                           const csdr_complexf *taps, size_t taps_pitch, int taps_length, int force_generic);
const char *csdr_amd_apply_fir_last_kernel(void);
/* The bank: n_channels channels, each with its own taps_length taps (all zero after create) and the last < taps_length samples of its stream on the
 * device, so the outputs of successive calls are the valid filter output of the whole stream since the last reset.  taps_length 1 .. 65536 and
 * n_channels x taps_length <= 2^27 (the taps and the history are device buffers of that many samples).
 * set_taps: taps_length HOST complexf for `channel` (-1: every channel).  set_peaks: the taps of peaks_fir_cc (csdr.c:2997-3002): firdes_add_peak_c of every
 * rate (n_rates >= 1) into zeroed taps, normalised with the last.  Both are ordered with the calls on the context's stream and keep the history: new taps
 * apply to every output of the calls that follow, the output stream has no gap and no repeat.
 * process: n_in new samples per channel -> held + n_in - taps_length + 1 outputs (0 if fewer), at most max_out(n_in) = n_in; counts (device, n_channels ints,
 * may be NULL) receives each channel's count.  Asynchronous.  reset / reset_channel drop the history and keep the taps. */
typedef struct csdr_amd_cfir csdr_amd_cfir;
csdr_amd_cfir *csdr_amd_cfir_create(csdr_amd_ctx *ctx, int n_channels, int taps_length);
int  csdr_amd_cfir_set_taps(csdr_amd_cfir *f, int channel, const csdr_complexf *host_taps);
int  csdr_amd_cfir_set_peaks(csdr_amd_cfir *f, int channel, const float *rates, int n_rates, int window);
int  csdr_amd_cfir_process(csdr_amd_cfir *f, const csdr_complexf *in, long long n_in, size_t in_pitch, csdr_complexf *out, size_t out_pitch, int *counts);
long long csdr_amd_cfir_max_out(const csdr_amd_cfir *f, long long n_in);
int  csdr_amd_cfir_reset(csdr_amd_cfir *f);
int  csdr_amd_cfir_reset_channel(csdr_amd_cfir *f, int channel);
int  csdr_amd_cfir_force_generic(csdr_amd_cfir *f, int on);
const char *csdr_amd_cfir_kernel_name(const csdr_amd_cfir *f);
void csdr_amd_cfir_destroy(csdr_amd_cfir *f);
/* the taps of peaks_fir_cc on the host: length complexf */
void csdr_amd_firdes_peaks_c(csdr_complexf *taps, int length, const float *rates, int n_rates, int window);
/* CPU run of the bank's walk (the same step functions) for one channel with HOST taps, the n samples cut into calls of cuts[0..n_cuts) samples and the
 * rest; outputs concatenated.  Returns the output count (< 0: refused, the reason in csdr_amd_last_error()). */
long long csdr_amd_debug_cfir_walk(const csdr_complexf *taps, int taps_length, const csdr_complexf *in, long long n, const long long *cuts, int n_cuts,
                                   csdr_complexf *out);

/* ------------------------------------------------------------------ noise sources, the AWGN channel and link measurements (noise.hip, noise_dev.hpp)
 * uniform_noise_f, gaussian_noise_c and awgn_cc (csdr.c:3035-3119; get_random_samples_f / get_random_gaussian_samples_c libcsdr.c:2444-2466) for
 * n_channels channels.  The reference turns 32-bit words from /dev/urandom into samples; here the words come from Philox4x32-10:
 *   block(kind, s, j) = philox(ctr = (j lo, j hi, s, kind), key = (seed lo, seed hi))      s: the channel's stream id, kind 0 Gaussian / 1 uniform
 *   Gaussian complex sample i takes words 2 (i & 1) and 2 (i & 1) + 1 of block(0, s, i >> 1), uniform float k word k & 3 of block(1, s, k >> 2)
 * and the words become samples as in the reference (noise_dev.hpp), with ln, sin and cos written out so that the kernels and the CPU entry give the same
 * bits.  A channel's stream is a function of (seed, stream id, sample index) alone: it does not depend on how calls cut it nor on the batch position.
 * create: stream_ids = n_channels HOST ids, or NULL for 0 .. n_channels - 1.  Every channel starts at position 0 with a_signal 1 and no noise.
 * generate: n samples per channel from its position on (float rows for a uniform object, complexf rows for a Gaussian one, out_pitch items apart).
 * awgn_cc (Gaussian objects): out = in * a_signal + noise * a_noise_scaled, two rounded products and one rounded sum per part (gain_ff, gain_ff, add_ff of
 * csdr.c:3078-3087), generated, scaled and added in one pass: the noise is not written anywhere.  out may be in.  snr_out (device, n_channels floats, may
 * be NULL): what --snrshow prints for this call, total_logpower_cf(in * a_signal) - total_logpower_cf(noise * a_noise_scaled), the powers summed in the
 * fixed order that noise.hip documents (float squares, double sums); a call of 0 samples leaves it alone.
 * Both advance every channel's position by n; any n from 0 on, any position, positions may differ per channel.  Asynchronous.
 * set_snr_db / set_snrs (HOST array): a_signal = spn / (spn + 1), a_noise = 1 / (spn + 1), a_noise_scaled = a_noise * 0.707 with spn = 10^(snr_db / 20)
 * in the reference's types (csdr_amd_awgn_gains).  get_gains returns a_signal and a_noise_scaled.  reset / reset_channel: back to position 0; ids
 * and gains stay.  kernel_name: "k_noise_gauss", "k_noise_uniform", "k_noise_gauss<awgn>", "k_noise_gauss<awgn+snr>". */
enum { CSDR_AMD_NOISE_GAUSSIAN = 0, CSDR_AMD_NOISE_UNIFORM = 1 };
typedef struct csdr_amd_noise_chan {
    unsigned long long position;
    unsigned stream_id;
    float a_signal, a_noise_scaled;
    unsigned reserved;
} csdr_amd_noise_chan;
typedef struct csdr_amd_noise csdr_amd_noise;
csdr_amd_noise *csdr_amd_noise_create(csdr_amd_ctx *ctx, int n_channels, int kind, unsigned long long seed, const unsigned *stream_ids);
int  csdr_amd_noise_generate(csdr_amd_noise *p, void *out, long long n, size_t out_pitch);
int  csdr_amd_noise_awgn_cc(csdr_amd_noise *p, const csdr_complexf *in, long long n, size_t in_pitch, csdr_complexf *out, size_t out_pitch, float *snr_out);
int  csdr_amd_noise_set_snr_db(csdr_amd_noise *p, int channel, float snr_db);
int  csdr_amd_noise_set_snrs(csdr_amd_noise *p, const float *snr_db);
int  csdr_amd_noise_get_gains(const csdr_amd_noise *p, int channel, float *a_signal, float *a_noise_scaled);
long long csdr_amd_noise_position(csdr_amd_noise *p, int channel);
int  csdr_amd_noise_set_position(csdr_amd_noise *p, int channel, long long position);
int  csdr_amd_noise_get_channel(csdr_amd_noise *p, int channel, csdr_amd_noise_chan *state);
int  csdr_amd_noise_reset(csdr_amd_noise *p);
int  csdr_amd_noise_reset_channel(csdr_amd_noise *p, int channel);
const char *csdr_amd_noise_kernel_name(const csdr_amd_noise *p);
void csdr_amd_noise_destroy(csdr_amd_noise *p);
/* the gains of awgn_cc <snr_db> on the host (either output may be NULL) */
void csdr_amd_awgn_gains(float snr_db, float *a_signal, float *a_noise_scaled);
/* awgn_cc on the caller's noise rows (the --awgnfile path): out = in * a_signal[ch] + noise * a_noise_scaled[ch] in the order above, bit-exact to the
 * reference.  Rows of n complexf, pitches in samples; a_signal / a_noise_scaled: DEVICE, n_channels floats each.  out may be in. */
int  csdr_amd_awgn_cc(csdr_amd_ctx *ctx, const csdr_complexf *in, const csdr_complexf *noise, csdr_complexf *out, int n_channels, long long n, size_t in_pitch,
                      size_t noise_pitch, size_t out_pitch, const float *a_signal, const float *a_noise_scaled);
/* total_logpower_cf libcsdr.c:1316-1321 for n_rows rows of n >= 1 samples: out (device, n_rows floats) = 10 log10(sum (i*i + q*q) / n), the squares in
 * float, the sum in double in the order of noise.hip. */
int  csdr_amd_total_logpower_cf(csdr_amd_ctx *ctx, const csdr_complexf *in, int n_rows, long long n, size_t in_pitch, float *out);
/* normalized_timing_variance_u32_f libcsdr.c:2293-2317 for n_rows rows of sample indexes (the idx output of csdr_amd_pulserx_process), pitch items apart:
 * row r has counts[r] of them (device ints, clamped to 0 .. n; NULL: n each).  The reference's unsigned arithmetic and running mean, one lane per row.
 * out: device, n_rows floats.  A row of one index divides 0 by 0 as the reference does and gives NaN; an empty row gives 0. */
int  csdr_amd_normalized_timing_variance_u32_f(csdr_amd_ctx *ctx, const unsigned *idx, size_t pitch, int n, const int *counts, int n_rows, int samples_per_symbol,
                                               int initial_sample_offset, float *out);
/* errors[c] (device ints) = the number of i < n_c with a[c][lag_c + i] != b[c][i], exact.  n_c = counts[c] (device; NULL: b_len) cut to b_len and to
 * a_len - lag_c, so that no read leaves a row; lag_c = lags[c] >= 0 (device; NULL: 0).  Rows a_pitch / b_pitch bytes apart. */
int  csdr_amd_count_errors_u8(csdr_amd_ctx *ctx, const unsigned char *a, size_t a_pitch, long long a_len, const unsigned char *b, size_t b_pitch, long long b_len,
                              int n_channels, const int *lags, const int *counts, int *errors);
/* CPU entries (noise_dev.hpp on the host).  philox: ctr[4], key[2] -> out[4].  noise_words: kind 0, n complexf from 2 n words; kind 1, n floats from n
 * words.  noise_walk: one channel's stream from `position`, cut into calls of cuts[0..n_cuts) samples and the rest; in == NULL: the noise, else (Gaussian)
 * awgn_cc of in at snr_db.  Returns n (< 0: refused). */
void csdr_amd_debug_philox(const unsigned *ctr, const unsigned *key, unsigned *out);
int  csdr_amd_debug_noise_words(int kind, const unsigned *words, long long n, void *out);
long long csdr_amd_debug_noise_walk(int kind, unsigned long long seed, unsigned stream_id, long long position, long long n, const long long *cuts, int n_cuts,
                                    const csdr_complexf *in, float snr_db, void *out);
int  csdr_amd_debug_awgn_cc(const csdr_complexf *in, const csdr_complexf *noise, long long n, float snr_db, csdr_complexf *out);   /* the flat awgn_cc on the host */
float csdr_amd_debug_timing_variance(const unsigned *idx, int n, int samples_per_symbol, int initial_sample_offset);

/* ------------------------------------------------------------------ squelch and S-meter (squelch.hip)
 * squelch_and_smeter_cc csdr.c:2192-2243 with get_power_c libcsdr.c:1154-1162, for n_channels channels.  Each channel's stream is cut into blocks of
 * block_size (B) samples counted from its start (the last reset).  A block's power is P = sum over its samples 0, d, 2d, .. of (i*i + q*q) / B with
 * d = use_every_nth (the divisor is B, as in the reference); the block is written unchanged if level == 0 or P >= level, else as B complex +0.0 (a NaN power
 * closes the gate unless the level is 0).  The sum runs in the library's own fixed order (squelch_dev.hpp): the power bits and the decision of a block do
 * not depend on the kernel that served it, on the channel's position in the batch or on how the calls cut the stream; against the float64 power it lies
 * within (ceil(B/d) + 8) 2^-24 P, as any float32 order does.
 * create: levels = n_channels floats, or NULL = 0 = always open; process accepts up to max_samples_per_call samples per channel and call.
 * process: any n_in per call (in: device, in_pitch samples apart).  The blocks that have become complete are emitted: out (device, out_pitch samples apart)
 * receives them back to back, power / open_flags (device, both [n_channels][power_pitch], either may be NULL) their power and 1 = passed / 0 = zeroed,
 * n_blocks_out (HOST, n_channels ints, may be NULL) each channel's count; the fewer than B samples behind a channel's last whole block stay in the object,
 * so the output lags the input by up to B - 1 samples at a call boundary.  Returns the largest count of any channel (all equal unless reset_channel was
 * used), or a negative code.  out_pitch >= that count * B; power_pitch >= that count: max_blocks() bounds it.  Asynchronous on the context's stream.
 * set_level: takes effect from the next block that a later call starts (a block already begun keeps the level it began under, as the reference reads a new
 * level behind a block's output); channel -1 sets all channels.  block_index: the number of blocks the channel has emitted since its reset = the index of
 * its next block, for the report schedule below.  reset / reset_channel drop the held samples and the block count and keep the levels.
 * kernel_name: "k_squelch_wave<4>" / "<16>" (one wave per block, B <= 512 / 2048), "k_squelch_wg<8>" / "<16>" / "<32>" (one workgroup per block, B <= 4096 /
 * 8192 / 16384), each holding the block in registers between its one read and one write, or "k_squelch_generic" (two passes: larger blocks, odd B or pitch,
 * unaligned pointers, calls that begin inside a block).  force_generic(1) takes k_squelch_generic always: the same bits. */
typedef struct csdr_amd_squelch csdr_amd_squelch;
csdr_amd_squelch *csdr_amd_squelch_create(csdr_amd_ctx *ctx, int n_channels, int block_size, int use_every_nth, const float *levels, long long max_samples_per_call);
int  csdr_amd_squelch_process(csdr_amd_squelch *s, const csdr_complexf *in, long long n_in, size_t in_pitch, csdr_complexf *out, size_t out_pitch, float *power,
                              size_t power_pitch, uint8_t *open_flags, int *n_blocks_out);
int  csdr_amd_squelch_set_level(csdr_amd_squelch *s, int channel, float level);
float csdr_amd_squelch_get_level(const csdr_amd_squelch *s, int channel);
long long csdr_amd_squelch_block_index(const csdr_amd_squelch *s, int channel);
int  csdr_amd_squelch_max_blocks(const csdr_amd_squelch *s);
int  csdr_amd_squelch_reset(csdr_amd_squelch *s);
int  csdr_amd_squelch_reset_channel(csdr_amd_squelch *s, int channel);
int  csdr_amd_squelch_force_generic(csdr_amd_squelch *s, int on);
const char *csdr_amd_squelch_kernel_name(const csdr_amd_squelch *s);
void csdr_amd_squelch_destroy(csdr_amd_squelch *s);
/* get_power_c / get_power_f libcsdr.c:1144-1162 on n_blocks consecutive blocks of block_size samples of each of n_streams rows (device, in_pitch samples apart):
 * power_out (device) [n_streams][n_blocks], the same order and bits as the object's powers.  Stateless. */
int  csdr_amd_get_power_c(csdr_amd_ctx *ctx, const csdr_complexf *in, int n_streams, int n_blocks, int block_size, int decimation, size_t in_pitch, float *power_out);
int  csdr_amd_get_power_f(csdr_amd_ctx *ctx, const float *in, int n_streams, int n_blocks, int block_size, int decimation, size_t in_pitch, float *power_out);
/* host: whether block block_index (0-based) reports its power, csdr.c:2224-2229 (`if (report_cntr++ > report_every_nth)`: the blocks with
 * block_index mod (report_every_nth + 2) == report_every_nth + 1); the gate decision csdr.c:2230 */
int  csdr_amd_squelch_report_due(int report_every_nth, long long block_index);
int  csdr_amd_squelch_gate_open(float power, float level);
/* the power step function on the host (the source the kernels run): one block of block_size samples at `in` (host; complex: interleaved i, q) */
float csdr_amd_debug_squelch_power(const float *in, int block_size, int decimation, int is_complex);

/* ------------------------------------------------------------------ carrier recovery (carrier.hip)
 * bpsk_costas_loop_cc libcsdr.c:2094-2142 and pll_cc libcsdr.c:1856-1915 for n_channels channels: the loop coefficients are shared, each channel has its
 * own state (phase, dphase, freq), kept on the device between calls.  Every float operation is the reference's, in its order; cos, sin and atan2 are taken
 * in double from the float argument and rounded (carrier_dev.hpp).  A call over a whole stream and any cut of it into calls, any batch position, any
 * set_lanes and either kernel give the same bits.
 * params: mode COSTAS (error = PI out.i out.q) / COSTAS_DD (the decision-directed atan2 error) / PLL_P / PLL_PI; alpha, beta; dphase_max and
 * dphase_max_reset_to_zero (Costas only).  |alpha|, |beta| <= 64 and 0 <= dphase_max <= 64 keep a sample's phase wraps to a few turns; a wrap ends after
 * 1024 turns in any case, where the reference is on its way to a hang.  The helpers compute what init_bpsk_costas_loop_cc, pll_cc_init_p_controller and
 * pll_cc_init_pi_controller store, to the bit.
 * process: in (device, in_pitch samples apart), n samples per channel; out, error, dphase, nco (device, each out_pitch of its own elements apart) receive n
 * items per channel; any may be NULL, not all.  Costas: out = in * nco, error, dphase (after the clamp), nco = (cos, sin) of the phase before the step.
 * PLL: nco = (sin, cos) of the advanced phase and dphase = -dphase, the reference's outputs; out and error must be NULL.  Asynchronous on the context's
 * stream.  n = 0 is a no-op.
 * set_lanes: channels per wave, 0 = automatic .. 64.  kernel_name: "k_carrier_tiled" (input and outputs staged through LDS in
 * coalesced tiles) or "k_carrier" (one lane per channel on global memory: pointers that are not 8-byte aligned, or force_generic(1)). */
enum { CSDR_AMD_CARRIER_COSTAS = 0, CSDR_AMD_CARRIER_COSTAS_DD = 1, CSDR_AMD_CARRIER_PLL_P = 2, CSDR_AMD_CARRIER_PLL_PI = 3 };
typedef struct csdr_amd_carrier_params { int mode; float alpha, beta, dphase_max; int dphase_max_reset_to_zero; } csdr_amd_carrier_params;
typedef struct csdr_amd_carrier_chan { float phase, dphase, freq; } csdr_amd_carrier_chan;   /* nco_phase / output_phase, dphase, current_freq / iir_temp */
typedef struct csdr_amd_carrier csdr_amd_carrier;
int  csdr_amd_costas_params(float bandwidth, float damping, int decision_directed, csdr_amd_carrier_params *p);
int  csdr_amd_pll_params_p(float alpha, csdr_amd_carrier_params *p);
int  csdr_amd_pll_params_pi(float bandwidth, float ko, float kd, float damping, csdr_amd_carrier_params *p);
csdr_amd_carrier *csdr_amd_carrier_create(csdr_amd_ctx *ctx, const csdr_amd_carrier_params *params, int n_channels);
int  csdr_amd_carrier_process(csdr_amd_carrier *p, const csdr_complexf *in, long long n, size_t in_pitch, csdr_complexf *out, float *error, float *dphase,
                              csdr_complexf *nco, size_t out_pitch);
int  csdr_amd_carrier_reset(csdr_amd_carrier *p);
int  csdr_amd_carrier_reset_channel(csdr_amd_carrier *p, int channel);
int  csdr_amd_carrier_get_channel(csdr_amd_carrier *p, int channel, csdr_amd_carrier_chan *out);
int  csdr_amd_carrier_set_channel(csdr_amd_carrier *p, int channel, const csdr_amd_carrier_chan *state);   /* finite, each magnitude <= 1024 */
int  csdr_amd_carrier_set_lanes(csdr_amd_carrier *p, int lanes);
int  csdr_amd_carrier_lanes(const csdr_amd_carrier *p);
int  csdr_amd_carrier_force_generic(csdr_amd_carrier *p, int on);
const char *csdr_amd_carrier_kernel_name(const csdr_amd_carrier *p);
void csdr_amd_carrier_destroy(csdr_amd_carrier *p);
/* the kernels' step function on the host for one channel, the stream cut into calls of cuts[0], cuts[1], ... samples and the rest; outputs may be NULL;
 * state_io (may be NULL: a fresh channel) carries the state in and out.  Returns n or a negative code. */
long long csdr_amd_debug_carrier_walk(const csdr_amd_carrier_params *params, const csdr_complexf *in, long long n, const long long *cuts, int n_cuts,
                                      csdr_complexf *out, float *error, float *dphase, csdr_complexf *nco, csdr_amd_carrier_chan *state_io);

/* ------------------------------------------------------------------ the shifter bank: a shift rate and a phase per stream (shiftbank.hip)
 * shift_addition_cc / shift_addition_fc (libcsdr_gpl.c:27-52, 54-79; the CLI's 1024-blocks csdr.c:896-923), shift_math_cc (libcsdr.c:186-207) and
 * shift_table_cc (libcsdr.c:229-265) for n_streams streams, each with its own rate and its own state on the device: one shifter per client on one wideband
 * stream (csdr.c:881-923, ddcd_old.h:51-61) is one object and one call.  csdr_amd_shift_cc keeps one rate per call; CSDR_SHIFT_UNROLL and CSDR_SHIFT_ADDFAST
 * exist there only and are refused here.
 * variant: CSDR_SHIFT_ADDITION (chunk: samples per phasor restart, 1024 in the CLI), CSDR_SHIFT_MATH or CSDR_SHIFT_TABLE (aux: table size, 0 = 65536).
 * in_format F32 (real input, shift_addition_fc) goes with ADDITION only.
 * Semantics: the reference's, independent of how calls cut the stream.  ADDITION: chunks count from the STREAM's start (reset), a call may end inside a chunk
 * and (pos, c, s) carry it on; chunk start c = (float)cos(phase), s = (float)sin(phase); chunk end phase = wrap(phase + (2 rate) PI chunk) in float.
 * MATH / TABLE: phase = wrap(phase + (2 rate) PI) per sample.
 * Retune: set_rate takes effect at the first sample of the next process call that has samples.  MATH / TABLE: the phase carries over.  ADDITION: the open
 * chunk ends where it stands -- pos > 0: phase = wrap(phase + (2 old_rate) PI pos), what the reference returns for a block of pos samples -- and a new chunk
 * starts at the call's first sample: the reference called on blocks that end at the retune (pos == 0: the CLI's own behaviour).
 * process: in (device; in_pitch elements apart, in_pitch == 0: ONE input row shared by every stream), out (device, out_pitch samples apart), n samples per
 * stream, 0 <= n <= max_samples_per_call.  Asynchronous on the context's stream.
 * MATH / TABLE scan each stream's n phase steps with one lane per stream, and the scan of the NEXT call (same n, from this call's end phases) is queued on
 * a side stream at once: a call that finds it ready (same n, no set_rate / set_channel / reset since) uses it; scans_ahead counts those calls.
 * kernel_name: "k_shiftbank_addition" / "k_shiftbank_math" / "k_shiftbank_table", or "k_shiftbank_generic" (force_generic(1), or a chunk below 32). */
typedef struct csdr_amd_shiftbank csdr_amd_shiftbank;
enum { CSDR_AMD_SHIFTBANK_IN_CF32 = 0, CSDR_AMD_SHIFTBANK_IN_F32 = 1 };
typedef struct csdr_amd_shiftbank_chan {   /* one stream's state */
    float rate;            /* as the caller gave it (the reference's argument, before its own *2) */
    float phase;           /* ADDITION: phase at the start of the current chunk; MATH / TABLE: phase of the next sample */
    float c, s;            /* ADDITION: the phasor of the next sample (cosphi, sinphi); MATH / TABLE: 1, 0 */
    int   pos;             /* ADDITION: samples of the current chunk already done, 0 .. chunk - 1; 0 otherwise */
    int   pending;         /* 1: `rate` changed since the last call with samples */
    float old_rate;        /* the rate the open chunk was started with (ADDITION: for the phase advance that closes it) */
    int   pad;
} csdr_amd_shiftbank_chan;
csdr_amd_shiftbank *csdr_amd_shiftbank_create(csdr_amd_ctx *ctx, int variant, int n_streams, const float *rates /* host, n_streams */, int chunk, int aux,
                                              int in_format, size_t max_samples_per_call);
int  csdr_amd_shiftbank_process(csdr_amd_shiftbank *p, const void *in, size_t in_pitch, csdr_complexf *out, size_t out_pitch, size_t n);
int  csdr_amd_shiftbank_set_rate(csdr_amd_shiftbank *p, int stream, float rate);      /* asynchronous, in order with the calls */
int  csdr_amd_shiftbank_get_rate(csdr_amd_shiftbank *p, int stream, float *rate);
int  csdr_amd_shiftbank_reset(csdr_amd_shiftbank *p);                                 /* every stream: phase 0, pos 0, its current rate */
int  csdr_amd_shiftbank_reset_channel(csdr_amd_shiftbank *p, int stream);
int  csdr_amd_shiftbank_get_channel(csdr_amd_shiftbank *p, int stream, csdr_amd_shiftbank_chan *out);
int  csdr_amd_shiftbank_set_channel(csdr_amd_shiftbank *p, int stream, const csdr_amd_shiftbank_chan *state);   /* finite, |phase| <= 1024, 0 <= pos < chunk */
int  csdr_amd_shiftbank_force_generic(csdr_amd_shiftbank *p, int on);
const char *csdr_amd_shiftbank_kernel_name(const csdr_amd_shiftbank *p);
long long csdr_amd_shiftbank_scans_ahead(csdr_amd_shiftbank *p);                      /* calls whose phase scan was found ready (MATH / TABLE) */
void csdr_amd_shiftbank_destroy(csdr_amd_shiftbank *p);
/* the kernels' step functions on the host for one stream, the stream cut into calls of cuts[0], cuts[1], ... samples and the rest.  call_rates (may be NULL):
 * n_cuts + 1 floats, a set_rate in front of call k where call_rates[k] is not NaN.  state_io (may be NULL: a fresh stream of rate `rate`) carries the state
 * in and out.  Returns n or a negative code. */
long long csdr_amd_debug_shiftbank_walk(int variant, float rate, int chunk, int aux, int in_format, const void *in, long long n, const long long *cuts, int n_cuts,
                                        const float *call_rates, csdr_complexf *out, csdr_amd_shiftbank_chan *state_io);
/* ADDITION's chunk start phases as the pre-pass kernel steps them (seeds.hpp's plan where it covers the step, the wrap loop beyond): out[k] = the phase
 * after k + 1 chunks from `phase`, host build */
void csdr_amd_debug_shiftbank_chunk_phases(float rate, float phase, int chunk, int n, float *out);

/* ------------------------------------------------------------------ the transmit side: analog modulators and the up-converter bank (txmod.hip)
 * fmmod_fc libcsdr.c:1180-1192 for n_streams rows.  phase_io: device float[n_streams], last_phase in and out.  Bit-equal phases for every cut into calls. */
int csdr_amd_fmmod_fc(csdr_amd_ctx *ctx, const float *in, csdr_complexf *out, int n_streams, size_t n, size_t in_pitch, size_t out_pitch, float *phase_io);
/* dsb_fc csdr.c:2084-2102, add_dcoffset_cc libcsdr.c:1174-1178, fixed_amplitude_cc libcsdr.c:1194-1208: flat arrays */
int csdr_amd_dsb_fc(csdr_amd_ctx *ctx, const float *in, csdr_complexf *out, size_t n, float q_value);
int csdr_amd_add_dcoffset_cc(csdr_amd_ctx *ctx, const csdr_complexf *in, csdr_complexf *out, size_t n);
int csdr_amd_fixed_amplitude_cc(csdr_amd_ctx *ctx, const csdr_complexf *in, csdr_complexf *out, size_t n, float new_amplitude);
/* convert_f_samplerf csdr.c:2104-2127: 16 bytes per sample = (double)x, wait_for_this_sample, (unsigned)0 */
int csdr_amd_convert_f_samplerf(csdr_amd_ctx *ctx, const float *in, void *out, size_t n, unsigned wait_for_this_sample);
/* the phase step function of fmmod_fc on the host for one stream, the samples cut into calls of cuts[0], cuts[1], ... and the rest; phases (the phase after
 * every sample) and out may be NULL; state_io (may be NULL: phase 0) carries last_phase in and out.  Returns n or a negative code. */
long long csdr_amd_debug_fmmod_walk(const float *in, long long n, const long long *cuts, int n_cuts, float *phases, csdr_complexf *out, float *state_io);

/* The fused transmit bank: for n_streams s16 audio streams the stream of
 *     convert_s16_f | gain_ff gain | <modulator> | fir_interpolate_cc interpolation (taps) | shift_addition_cc rate[s] | [convert_f_u8]
 * with <modulator> = fmmod_fc (CSDR_TX_FM), dsb_fc q_value | add_dcoffset_cc (CSDR_TX_AM) or dsb_fc q_value (CSDR_TX_DSB).
 * The object keeps each stream's FM phase, the interpolator's last ceil((taps_length - 1) / interpolation) modulated samples and the rotator's phase on the
 * device: a stream cut into calls anywhere (0-sample calls included) gives the bits of one call.  The output is fir_interpolate_cc (libcsdr.c:579-605) applied
 * once to the whole modulated stream since the last reset.  The rotator is shift_addition_cc as the CLI runs it, in 1024-sample chunks (csdr.c:911-918) laid on
 * the output stream from the first output after a reset or a retune, the float phase carried from chunk to chunk.  set_rate takes effect from the first output
 * of the next process call: the phase is carried and the chunk grid restarts there.  Rates are -0.5 .. 0.5.
 * process: in_s16 [n_streams][in_pitch] s16 samples, out [n_streams][out_pitch] complex samples (cf32, or u8 pairs), pitches in samples; *n_out <= max_out(n_in).
 * k_tx_up needs a 16-byte aligned out and row pitch; anything else takes k_tx_up_generic: the same bits. */
enum { CSDR_TX_FM = 0, CSDR_TX_AM = 1, CSDR_TX_DSB = 2 };
enum { CSDR_TX_OUT_CF32 = 0, CSDR_TX_OUT_U8 = 1 };
typedef struct csdr_amd_txbank csdr_amd_txbank;
csdr_amd_txbank *csdr_amd_txbank_create(csdr_amd_ctx *ctx, int n_streams, int mode, float gain, float q_value, int interpolation, const float *host_taps,
                                        int taps_length, const float *shift_rates, int out_format, size_t max_in_samples);
int  csdr_amd_txbank_process(csdr_amd_txbank *p, const int16_t *in_s16, size_t in_pitch, long long n_in, void *out, size_t out_pitch, long long *n_out);
int  csdr_amd_txbank_set_rate(csdr_amd_txbank *p, int stream, float rate);
float csdr_amd_txbank_get_rate(const csdr_amd_txbank *p, int stream);
int  csdr_amd_txbank_reset(csdr_amd_txbank *p);                        /* phases and history; the rates stay as last set */
long long csdr_amd_txbank_max_out(const csdr_amd_txbank *p, long long n_in);
int  csdr_amd_txbank_force_generic(csdr_amd_txbank *p, int on);
const char *csdr_amd_txbank_kernel_name(const csdr_amd_txbank *p);
void csdr_amd_txbank_destroy(csdr_amd_txbank *p);

/* ------------------------------------------------------------------ f2: the remaining simple blocks
 * amdemod_cf / amdemod_estimator_cf libcsdr.c:861-901, realpart_cf csdr.c:634-645, logpower_cf libcsdr.c:1296-1303: flat arrays */
int csdr_amd_amdemod_cf(csdr_amd_ctx *ctx, const csdr_complexf *in, float *out, size_t n);
int csdr_amd_amdemod_estimator_cf(csdr_amd_ctx *ctx, const csdr_complexf *in, float *out, size_t n, float alpha, float beta);
int csdr_amd_realpart_cf(csdr_amd_ctx *ctx, const csdr_complexf *in, float *out, size_t n);
int csdr_amd_logpower_cf(csdr_amd_ctx *ctx, const csdr_complexf *in, float *out, size_t n, float add_db);
/* fmdemod_atan_cf libcsdr.c:1004-1019.  last_phase_io: device float[n_streams] */
int csdr_amd_fmdemod_atan_cf(csdr_amd_ctx *ctx, const csdr_complexf *in, float *out, int n_streams, size_t n,
                             size_t in_pitch, size_t out_pitch, float *last_phase_io);
/* dcblock_ff libcsdr.c:903-918.  state_io: device float[2*n_streams] = {last_input, last_output} (dcblock_preserve_t, libcsdr.h:110-114) */
int csdr_amd_dcblock_ff(csdr_amd_ctx *ctx, const float *in, float *out, int n_streams, size_t n, size_t in_pitch, size_t out_pitch,
                        float a, float *state_io);
/* fastdcblock_ff libcsdr.c:920-941 over n_blocks consecutive blocks per stream.  last_dc_io: device float[n_streams] */
int csdr_amd_fastdcblock_ff(csdr_amd_ctx *ctx, const float *in, float *out, int n_streams, int n_blocks, int block,
                            size_t in_pitch, size_t out_pitch, float *last_dc_io);
/* agc_ff libcsdr_gpl.c:163-260: n samples per stream processed as consecutive calls of `block` samples (the CLI's the_bufsize,
 * csdr.c:1338-1375: the hang/attack counters restart with every call).  last_gain_io: device float[n_streams] */
int csdr_amd_agc_ff(csdr_amd_ctx *ctx, const float *in, float *out, int n_streams, size_t n, int block, size_t in_pitch, size_t out_pitch,
                    float reference, float attack_rate, float decay_rate, float max_gain, short hang_time, short attack_wait_time,
                    float gain_filter_alpha, float *last_gain_io);
/* precalculate_window libcsdr.c:1256-1267 (host) */
void csdr_amd_precalculate_window(float *host_windowt, int size, int window);
/* `csdr fft_cc <fft_size> <out_of_every_n_samples> [window]` (csdr.c:1569-1641): windowed FFT of the newest fft_size samples every
 * every_n_samples new samples; the sliding buffer is carried inside the object.  Returns the number of spectra written. */
typedef struct csdr_amd_fftcc csdr_amd_fftcc;
csdr_amd_fftcc *csdr_amd_fftcc_create(csdr_amd_ctx *ctx, int fft_size, int every_n_samples, int window, int max_frames);
void csdr_amd_fftcc_destroy(csdr_amd_fftcc *f);
int  csdr_amd_fftcc_process(csdr_amd_fftcc *f, const csdr_complexf *in, size_t n_in, csdr_complexf *out, size_t *consumed);
/* `csdr fft_fc <fft_out_size> <out_of_every_n_samples> [window]` (csdr.c:3414-3498): the spectrum of a real signal.  M = fft_out_size (a power of two >= 2)
 * is the number of complex bins written per spectrum, DC to M-1 (the Nyquist bin is not written); every transform takes 2M floats times
 * precalculate_window(2M, window).  Schedule in floats, E = every_n_samples: E <= 2M: spectrum k covers stream floats [k E + E - 2M, k E + E), positions
 * before 0 being the zeros of a fresh sliding buffer; E > 2M: the reference skips with complexf-sized reads on its float stream (csdr.c:3466-3469), i.e.
 * 2 (E - 2M) floats, so spectrum k covers [k P, k P + 2M) with P = 2 E - 2M -- reproduced, so that a stream frames as the reference's does.
 * The sliding buffer and the floats still to skip are carried inside the object: process consumes all n_in (<= max_samples_per_call) device floats and
 * writes the spectra they complete, at most ceil(n_in / min(E, P)) of M csdr_complexf each, to the device array out.  Returns their number, or < 0.
 * The reference's repeated last spectrum at end of stream is not produced. */
typedef struct csdr_amd_fftfc csdr_amd_fftfc;
csdr_amd_fftfc *csdr_amd_fftfc_create(csdr_amd_ctx *ctx, int fft_out_size, int every_n_samples, int window, size_t max_samples_per_call);
void csdr_amd_fftfc_destroy(csdr_amd_fftfc *f);
int  csdr_amd_fftfc_process(csdr_amd_fftfc *f, const float *in, size_t n_in, csdr_complexf *out);
/* `csdr fft_one_side_ff <fft_size>` (csdr.c:1717-1734): the first fft_size/2 floats of each of n_rows rows of fft_size (device arrays; fft_size even) */
int  csdr_amd_fft_one_side_ff(csdr_amd_ctx *ctx, const float *in, float *out, int n_rows, int fft_size);

/* ------------------------------------------------------------------ the waterfall: `[convert_u8_f |] fft_cc N E [window] | logaveragepower_cf A N AVG |
 * fft_exchange_sides_ff N [| compress_fft_adpcm_f_u8 N]` (csdr.c:1569-1641, 1663-1714, 1745-1768) for n_streams streams per call.
 * fft_size 1024 / 2048 / 4096 / 8192: one kernel per row that reads the input once (k_wf_onepass); any other power of two >= 2: framing + hipFFT + one
 * post-FFT kernel.  The frame schedule is fft_cc's; the overlap history, the samples still to skip and the partial row are carried per stream between calls,
 * and only complete rows are written: rows of fft_size float dB values (CSDR_AMD_WF_OUT_DB, halves exchanged) or of (fft_size+10)/2 ADPCM bytes
 * (CSDR_AMD_WF_OUT_ADPCM, compress_fft_adpcm_f_u8 of the dB row).  add_db' = (float)(add_db - 10 log10(avgnumber)) as csdr.c:1678 forms it.
 * Real input, CSDR_AMD_WF_IN_F32 (floats) / CSDR_AMD_WF_IN_S16 (shorts through convert_s16_f's arithmetic): the object is
 * `[convert_s16_f |] fft_fc M E [window] | logaveragepower_cf A M AVG [| compress_fft_adpcm_f_u8 M]`.  fft_size means M, the output bins, as in fft_fc;
 * every_n_samples, max_samples_per_call, n_in and in_pitch count real samples, with fft_fc's schedule (above, its E > 2M period P = 2 E - 2M included);
 * rows are M floats or (M+10)/2 bytes in display order (DC first, no exchange of halves).  M = 1024 / 2048 / 4096 / 8192: one kernel (k_wf_onepass_real:
 * the M-point transform of the packed frame plus one untangling exchange); any other power of two >= 2: framing + hipFFT + k_wf_post. */
typedef struct csdr_amd_waterfall csdr_amd_waterfall;
enum { CSDR_AMD_WF_IN_CF32 = 0, CSDR_AMD_WF_IN_U8 = 1, CSDR_AMD_WF_IN_F32 = 2, CSDR_AMD_WF_IN_S16 = 3 };
enum { CSDR_AMD_WF_OUT_DB = 0, CSDR_AMD_WF_OUT_ADPCM = 1 };
csdr_amd_waterfall *csdr_amd_waterfall_create(csdr_amd_ctx *ctx, int fft_size, int every_n_samples, int window, int avgnumber,
                                              float add_db, int in_format, int out_format, int n_streams, size_t max_samples_per_call);
/* n_in new samples for every stream (device, in_pitch samples apart); writes *rows_out rows per stream (out_pitch bytes apart).  Returns the rows or < 0. */
int  csdr_amd_waterfall_process(csdr_amd_waterfall *w, const void *in, size_t n_in, size_t in_pitch, void *out, size_t out_pitch, int *rows_out);
int  csdr_amd_waterfall_reset(csdr_amd_waterfall *w);
/* what the last call ran: "k_wf_onepass (u8)" / "k_wf_onepass (cf32)" or "k_wf_post (generic: framing + hipFFT)"; real input:
 * "k_wf_onepass_real (f32)" / "k_wf_onepass_real (s16)" or "k_wf_post (generic real: framing + hipFFT + untangle)" */
const char *csdr_amd_waterfall_kernel_name(const csdr_amd_waterfall *w);
/* on != 0: the one-pass sizes take the generic path too (A/B comparisons) */
int  csdr_amd_waterfall_force_generic(csdr_amd_waterfall *w, int on);
void csdr_amd_waterfall_destroy(csdr_amd_waterfall *w);
/* stand-alone stages (device, n_rows independent rows): logaveragepower_cf reads n_rows*avgnumber spectra, writes n_rows rows (csdr.c:1663-1695);
 * fft_exchange_sides_ff swaps the halves of every row (csdr.c:1697-1714) */
int  csdr_amd_logaveragepower_cf(csdr_amd_ctx *ctx, const csdr_complexf *in, float *out, int n_rows, int fft_size, int avgnumber, float add_db);
int  csdr_amd_fft_exchange_sides_ff(csdr_amd_ctx *ctx, const float *in, float *out, int n_rows, int fft_size);
/* accumulate_power_cf / log_ff (libcsdr.c:1305-1314), device arrays: acc_io[i] += |in[i]|^2; out[i] = 10 log10(in[i]) + add_db */
int  csdr_amd_accumulate_power_cf(csdr_amd_ctx *ctx, const csdr_complexf *in, float *acc_io, size_t n);
int  csdr_amd_log_ff(csdr_amd_ctx *ctx, const float *in, float *out, size_t n, float add_db);

/* ------------------------------------------------------------------ f3: IMA ADPCM (ima_adpcm.c:110-174), bit exact.
 * A serial state machine per stream: one lane per stream.  state_io: device int32[2*n_streams] = {index, previousValue} (ima_adpcm_state_t).
 * encode: n int16 samples per stream -> n/2 bytes (low nibble first; an odd last sample is dropped like the reference does);
 * decode: n bytes per stream -> 2n samples. */
int csdr_amd_encode_ima_adpcm_i16_u8(csdr_amd_ctx *ctx, const int16_t *in, uint8_t *out, int n_streams, size_t n,
                                     size_t in_pitch, size_t out_pitch, int *state_io);
int csdr_amd_decode_ima_adpcm_u8_i16(csdr_amd_ctx *ctx, const uint8_t *in, int16_t *out, int n_streams, size_t n,
                                     size_t in_pitch, size_t out_pitch, int *state_io);
/* `csdr compress_fft_adpcm_f_u8 <fft_size>` (csdr.c:1745-1768): n_blocks rows of fft_size dB values -> (fft_size+10)/2 bytes each; the
 * encoder restarts from the zero state for every row, so rows are independent (one lane per row). */
int csdr_amd_compress_fft_adpcm_f_u8(csdr_amd_ctx *ctx, const float *in, uint8_t *out, int n_blocks, int fft_size);

/* ------------------------------------------------------------------ FFT overlap-add filter
 * bandpass_fir_fft_cc (csdr.c:1810-1886) = apply_fir_fft_cc (libcsdr.c:814-849) per block.
 * One object per (fft_size, taps); processes n_blocks blocks of input_size = fft_size-taps_length+1 samples
 * for n_streams streams per call; the inter-block overlap is carried inside the object per stream. */
typedef struct csdr_amd_fftfilt csdr_amd_fftfilt;
csdr_amd_fftfilt *csdr_amd_fftfilt_create(csdr_amd_ctx *ctx, int fft_size, const csdr_complexf *host_taps,
                                          int taps_length, int n_streams, int max_blocks);
void csdr_amd_fftfilt_destroy(csdr_amd_fftfilt *f);
int  csdr_amd_fftfilt_set_taps(csdr_amd_fftfilt *f, const csdr_complexf *host_taps, int taps_length);
/* A passband per stream (one-pass path only, i.e. <= 4096 taps and the path not switched off; the full-size transforms keep one taps spectrum and refuse with a
 * negative status, staying usable).  The taps LENGTH, and with it input_size, the window and the carried history, is common to the object: streams differ in their
 * taps, not in their number.
 * create_per_stream: host_taps holds n_streams rows of taps_length; stream s is filtered with row s.
 * set_stream_taps: new taps for one stream, from the next process on, over the input history carried so far (what set_taps does for all streams).  The first call on
 * a filter created with shared taps gives every stream a spectrum table of its own (2 x window x 8 bytes per stream on the device), filled with the current one; the
 * history is not touched.  set_taps on a per-stream filter sets every stream.  per_stream: 0 / 1.
 * A wrong taps_length, a stream out of range or a filter on the full-size path: negative status, message in csdr_amd_last_error, the object unchanged. */
csdr_amd_fftfilt *csdr_amd_fftfilt_create_per_stream(csdr_amd_ctx *ctx, int fft_size, const csdr_complexf *host_taps,
                                                     int taps_length, int n_streams, int max_blocks);
int  csdr_amd_fftfilt_set_stream_taps(csdr_amd_fftfilt *f, int stream, const csdr_complexf *host_taps, int taps_length);
int  csdr_amd_fftfilt_per_stream(const csdr_amd_fftfilt *f);
int  csdr_amd_fftfilt_input_size(const csdr_amd_fftfilt *f);
/* Taps short enough for windows that fit a CU's LDS (<= 4096 taps) are served by ONE pass over HBM (fftfilt_lds.hip: overlap-save with 4096 / 8192 / 16384-point
 * transforms in LDS; same samples out, same framing at this interface): its kernel name and window size, or "" / 0 when the full-size transform path runs. */
const char *csdr_amd_fftfilt_kernel_name(const csdr_amd_fftfilt *f);
int  csdr_amd_fftfilt_window(const csdr_amd_fftfilt *f);
int  csdr_amd_fftfilt_reset(csdr_amd_fftfilt *f);
int  csdr_amd_fftfilt_process(csdr_amd_fftfilt *f, const csdr_complexf *in, csdr_complexf *out,
                              int n_blocks, size_t in_pitch, size_t out_pitch);

/* building blocks used by the drop-in apply_fir_fft_cc / make_fft_c2c (libcsdr.c:814-849, fft_fftw.c:6-45) */
int csdr_amd_fft_c2c(csdr_amd_ctx *ctx, const csdr_complexf *in, csdr_complexf *out, int n, int forward);  /* unnormalised, cached plan */
int csdr_amd_bin_product(csdr_amd_ctx *ctx, const csdr_complexf *a, const csdr_complexf *b, csdr_complexf *out, size_t n);
/* io[k] = io[k]*scale (+ add[k] for k < n_add) */
int csdr_amd_scale_add(csdr_amd_ctx *ctx, csdr_complexf *io, size_t n, float scale, const csdr_complexf *add, size_t n_add);

/* ------------------------------------------------------------------ fastddc channelizer
 * fastddc_init fastddc.c:38-72 (layout == fastddc_t fastddc.h:5-24, 76 bytes) */
typedef struct csdr_fastddc_s {
    int pre_decimation, post_decimation, taps_length, taps_min_length, overlap_length,
        fft_size, fft_inv_size, input_size, post_input_size;
    float pre_shift; int startbin, v, offsetbin; float post_shift; int output_scrape, scrap;
    struct { float sindelta, cosdelta, rate; } dsadata;
} csdr_fastddc_t;
int csdr_amd_fastddc_init(csdr_fastddc_t *ddc, float transition_bw, int decimation, float shift_rate);

/* forward half = `csdr fastddc_fwd_cc` (csdr.c:2255-2300): overlap-save framing + fft_size forward FFT.
 * in: n_blocks*input_size new samples; spectra: [n_blocks][fft_size].  The overlap tail is kept in the object. */
typedef struct csdr_amd_fastddc_fwd csdr_amd_fastddc_fwd;
csdr_amd_fastddc_fwd *csdr_amd_fastddc_fwd_create(csdr_amd_ctx *ctx, const csdr_fastddc_t *ddc, int max_blocks);
void csdr_amd_fastddc_fwd_destroy(csdr_amd_fastddc_fwd *f);
int  csdr_amd_fastddc_fwd_process(csdr_amd_fastddc_fwd *f, const csdr_complexf *in, csdr_complexf *spectra, int n_blocks);

/* inverse half = `csdr fastddc_inv_cc` x n_channels (csdr.c:2302-2378, fastddc.c:106-166): per channel
 * alias-fold X*H into fft_inv_size bins, small inverse FFT, scrap, residual shift + post-decimation.
 * All channels share decimation/transition_bw (hence geometry) and differ by shift_rate.
 * out: [n_channels][out_pitch]; out_counts (host int[n_channels], may be NULL) receives samples written. */
typedef struct csdr_amd_fastddc_inv csdr_amd_fastddc_inv;
csdr_amd_fastddc_inv *csdr_amd_fastddc_inv_create(csdr_amd_ctx *ctx, float transition_bw, int decimation,
                                                  const float *host_shift_rates, int n_channels, int window,
                                                  int max_blocks);
void csdr_amd_fastddc_inv_destroy(csdr_amd_fastddc_inv *f);
/* retune one channel between two process() calls: geometry, taps and shift status of that channel are rebuilt (csdr.c:2329-2376) */
int  csdr_amd_fastddc_inv_set_rate(csdr_amd_fastddc_inv *f, int channel, float shift_rate);
int  csdr_amd_fastddc_inv_geometry(const csdr_amd_fastddc_inv *f, int channel, csdr_fastddc_t *ddc);
int  csdr_amd_fastddc_inv_max_output(const csdr_amd_fastddc_inv *f, int n_blocks);
int  csdr_amd_fastddc_inv_process(csdr_amd_fastddc_inv *f, const csdr_complexf *spectra, int n_blocks,
                                  csdr_complexf *out, size_t out_pitch, int *out_counts);
/* name of the dominant kernel ("k_ddc_gemm": the alias fold as an fp32 matrix-core product, taken at fft_inv_size 512 = BASELINE config 4;
 * "k_ddc_fold_ct": the general kernel) and HIP-event timing of it on the context's stream (bench_fastddc.py's roofline leg) */
const char *csdr_amd_fastddc_inv_kernel_name(const csdr_amd_fastddc_inv *f);
/* every kernel instance of the object's last call, template arguments included and joined by '+': the transform in front of the fold where the object runs one
 * ("k_ddc_xt" for natural-order spectra, "k_ddc_fwd512<16,F>[+k_ddc_fwd128]" for a bank's fused forward transform), the fold, the inverse transforms -- e.g.
 * "k_ddc_xt+k_ddc_gemm<2,true>+k_ddc_ifft512_post<8>", "k_ddc_fwd512<16,0>+k_ddc_gemm3<1,true>+k_ddc_ifft256d_post<8>", "k_ddc_fold<16>+hipfft+k_ddc_post".
 * "" before the first call; the pointer is valid until the object's next call.  csdr_amd_fastddc_inv_kernel_name keeps its coarse names. */
const char *csdr_amd_fastddc_inv_kernels(const csdr_amd_fastddc_inv *f);
int  csdr_amd_fastddc_inv_set_profiling(csdr_amd_fastddc_inv *f, int on);
int  csdr_amd_fastddc_inv_kernel_time(csdr_amd_fastddc_inv *f, double *total_ms, long *launches);
/* the same for the kernels around it (csdr_amd_fastddc_inv_set_profiling(f, 2): two more event pairs per call): stage 1 = the forward transform's first pass (k_ddc_fwd512), stage 2 = the inverse transforms with scrap and residual
 * shift (k_ddc_ifft256d_post / k_ddc_ifft512_post) */
int  csdr_amd_fastddc_inv_stage_time(csdr_amd_fastddc_inv *f, int stage, double *total_ms, long *launches);
/* Both halves in one object = the ddcd topology (ddcd_old.cpp:238-252, 474-492: one `csdr fastddc_fwd_cc` feeding N `csdr fastddc_inv_cc --fd` clients)
 * as one call per batch of blocks: in = n_blocks * input_size NEW wideband samples (the overlap is kept inside), out / out_counts as for
 * csdr_amd_fastddc_inv_process.  At BASELINE config 4's geometry (fft_size 65536, fft_inv_size 512) the forward transform writes the fold's own layout
 * directly (no natural-order spectrum, no framing copy). */
typedef struct csdr_amd_fastddc_bank csdr_amd_fastddc_bank;
csdr_amd_fastddc_bank *csdr_amd_fastddc_bank_create(csdr_amd_ctx *ctx, float transition_bw, int decimation, const float *host_shift_rates, int n_channels,
                                                    int window, int max_blocks);
void csdr_amd_fastddc_bank_destroy(csdr_amd_fastddc_bank *b);
int  csdr_amd_fastddc_bank_set_rate(csdr_amd_fastddc_bank *b, int channel, float shift_rate);   /* csdr.c:2329-2376 for one client */
int  csdr_amd_fastddc_bank_input_size(const csdr_amd_fastddc_bank *b);
int  csdr_amd_fastddc_bank_max_output(const csdr_amd_fastddc_bank *b, int n_blocks);
int  csdr_amd_fastddc_bank_process(csdr_amd_fastddc_bank *b, const csdr_complexf *in, int n_blocks, csdr_complexf *out, size_t out_pitch, int *out_counts);
/* The same in two halves, so that consecutive batches overlap: submit() stages a batch (state chains, forward transform -- and, for a sharded bank, the
 * exchange -- on a side stream; `in` must stay untouched until the matching collect() has been queued); collect() folds / inverse-transforms the oldest staged
 * batch on the context's stream.  Two batches may be staged: submit(N + 1) runs under collect(N).  process() = submit() + collect(). */
int  csdr_amd_fastddc_bank_submit(csdr_amd_fastddc_bank *b, const csdr_complexf *in, int n_blocks);
int  csdr_amd_fastddc_bank_collect(csdr_amd_fastddc_bank *b, csdr_complexf *out, size_t out_pitch, int *out_counts);

/* ------------------------------------------------------------------ multi-GPU: one process per GPU, RCCL over xGMI
 * The communicator belongs to the library (RCCL is loaded on demand, librccl.so.1).  Rank 0 calls csdr_amd_comm_unique_id and ships the 128 bytes to
 * the other ranks by any means (torch.distributed / MPI / a file); every rank then calls csdr_amd_comm_create (collective, ncclCommInitRank). */
typedef struct csdr_amd_comm csdr_amd_comm;
int  csdr_amd_comm_unique_id(char id128[128]);
csdr_amd_comm *csdr_amd_comm_create(csdr_amd_ctx *ctx, const char id128[128], int rank, int world);
void csdr_amd_comm_destroy(csdr_amd_comm *c);
int  csdr_amd_comm_rank(const csdr_amd_comm *c);
int  csdr_amd_comm_world(const csdr_amd_comm *c);
int  csdr_amd_comm_broadcast(csdr_amd_comm *c, void *dev_buf, size_t bytes, int root);        /* on the context's stream (test / bench plumbing) */
/* A second communicator over the same ranks (collective; RCCL: a new unique id broadcast over the parent, then ncclCommInitRank).  The time-sliced bank makes one
 * for its output exchange, so that its two exchanges -- issued from two side streams -- never share an ncclComm.  Destroy with csdr_amd_comm_destroy. */
csdr_amd_comm *csdr_amd_comm_dup(csdr_amd_comm *c);
/* First contact with a transport / a box (collective): a send/recv ring, an all-gather, a broadcast and a two-communicator / two-stream ring of rank-stamped
 * buffers of n_floats floats each, every byte checked, timed.  report (may be NULL) receives one line per rank; CSDR_AMD_COMM_VERBOSE=1 also prints it on stderr.
 * 0 = every byte arrived as stamped; -6 otherwise (csdr_amd_last_error() holds the line). */
int  csdr_amd_comm_selftest(csdr_amd_comm *c, size_t n_floats, char *report, size_t report_cap);
/* Two more transports behind the same communicator type, for boxes with ONE GPU:
 * loopback -- the `world` ranks live in one process, one host thread + one context each (all on one device, or on several); every exchange is a
 *   stream-ordered device copy.  The multi-rank code of the channelizer runs unchanged (tests at world 2 / 4 / 8 on one MI355X).  Every rank thread
 *   must make the same exchange calls in the same order; a rank that never arrives fails the others after 60 s instead of hanging them.
 * null -- rank `rank` of a `world`-rank schedule with NO peers: every exchange call returns at once and moves nothing.  For timing one rank's own
 *   work of a world-N schedule on one GPU (bench_fastddc.py --emulate-world); the outputs are meaningless. */
typedef struct csdr_amd_loopback csdr_amd_loopback;
csdr_amd_loopback *csdr_amd_loopback_create(int world);
void csdr_amd_loopback_destroy(csdr_amd_loopback *g);
void csdr_amd_loopback_abort(csdr_amd_loopback *g);                 /* a rank thread gave up: fail the others' rendezvous at once */
csdr_amd_comm *csdr_amd_comm_create_loopback(csdr_amd_ctx *ctx, csdr_amd_loopback *g, int rank);
csdr_amd_comm *csdr_amd_comm_create_null(csdr_amd_ctx *ctx, int rank, int world);
/* The ranks as PROCESSES on one box (RCCL refuses two ranks per device; the loopback's ranks are threads): unix sockets named "<path_prefix>.<rank>" + HIP IPC mappings
 * of the peers' buffers (a name too long for a socket path goes to the abstract namespace, under a hash of it).  A test transport (every group is host synchronous)
 * for what only separate processes exercise: `csdr fastddc_bank_cc` started once per rank (CSDR_AMD_COMM=ipc with CSDR_AMD_RANK / _WORLD / _COMM_FILE).
 * Collective; 60 s for the peers to appear. */
csdr_amd_comm *csdr_amd_comm_create_ipc(csdr_amd_ctx *ctx, const char *path_prefix, int rank, int world);
/* test hook: one send/receive group with `peer` (n floats each way; n_sends = 2 provokes the local error whose handling comm.cpp's l_group_end documents) */
int csdr_amd_debug_comm_exchange(csdr_amd_comm *c, const float *send_buf, float *recv_buf, size_t n, int peer, int n_sends);
/* fastddc bank over the communicator (BASELINE config 4 at 2 / 4 / 8 GPUs): host_shift_rates_all = ALL channels on every rank; rank r DELIVERS the
 * block-distributed slice of the channels csdr_amd_fastddc_bank_channel_slice reports (out rows = that slice; a channel's client connects to that GPU).
 * Two ways of dividing the work (shard_mode):
 *   CSDR_AMD_SHARD_BLOCKS (what csdr_amd_fastddc_bank_create_sharded picks for more than two ranks): time slices.  The blocks of a batch are dealt to the ranks in runs of
 *     ceil(max_blocks / world); every rank runs the whole single-GPU pipeline -- forward transform, fold of ALL channels, inverse transforms -- on its run and
 *     only the decimated outputs cross the links (all-to-all: each rank sends every peer that peer's channels of its run; 8 B per input sample in total, 1/world
 *     of it per link).  Possible because the only state that crosses block boundaries, decimating_shift_addition_cc's (remain, phase) per channel
 *     (fastddc.c:152-164), is data independent: every rank walks it over the whole batch itself.  The spectra never leave the GPU that computed them.
 *   CSDR_AMD_SHARD_CHANNELS (BASELINE north_star's partitioning; what csdr_amd_fastddc_bank_create_sharded picks for one or two ranks): the compute is channel-sharded
 *     as well: forward transform split by blocks, transposed spectra all-gathered over the full mesh (9.1 B per input sample arrive at EVERY rank), every rank folds
 *     its own channels.  Link bound beyond two GPUs.
 * csdr_amd_fastddc_bank_default_shard_mode(world) tells which one csdr_amd_fastddc_bank_create_sharded picks; csdr_amd_fastddc_bank_create_sharded_by takes either.
 * Input: submit / process read `in` on rank 0 only (the wideband stream lives there, like ddcd's single fastddc_fwd_cc, ddcd_old.cpp:238-252) and send every
 * rank the samples of its blocks point to point; csdr_amd_fastddc_bank_submit_local (time slices only) takes each rank's OWN run instead -- overlap_length
 * samples of the stream in front of the run's first block (zeros at the start of the stream), then its blocks -- when the ingest already distributes the
 * stream (csdr_amd_fastddc_bank_local_blocks tells a rank which blocks of an n-block batch are its run).
 * Needs the geometry of the matrix-core path (fft_size 65536, fft_inv_size 512).  All ranks make the same calls in the same order.
 * A time-sliced bank finishes a batch on its exchange stream: `out` is complete once csdr_amd_fastddc_bank_finish has been called (it orders the
 * context's stream behind the exchange; with out_counts it also waits and returns the sample counts).  collect() with out_counts != NULL and process()
 * call it themselves. */
enum { CSDR_AMD_SHARD_CHANNELS = 0, CSDR_AMD_SHARD_BLOCKS = 1 };
csdr_amd_fastddc_bank *csdr_amd_fastddc_bank_create_sharded(csdr_amd_ctx *ctx, float transition_bw, int decimation, const float *host_shift_rates_all, int n_channels_total,
                                                            int window, int max_blocks, csdr_amd_comm *comm);
csdr_amd_fastddc_bank *csdr_amd_fastddc_bank_create_sharded_by(csdr_amd_ctx *ctx, float transition_bw, int decimation, const float *host_shift_rates_all, int n_channels_total,
                                                               int window, int max_blocks, csdr_amd_comm *comm, int shard_mode);
int  csdr_amd_fastddc_bank_channel_slice(const csdr_amd_fastddc_bank *b, int *first, int *count);
int  csdr_amd_fastddc_bank_shard_mode(const csdr_amd_fastddc_bank *b);                          /* -1: one GPU */
int  csdr_amd_fastddc_bank_default_shard_mode(int world);
int  csdr_amd_fastddc_bank_local_blocks(const csdr_amd_fastddc_bank *b, int n_blocks, int *first, int *count);
int  csdr_amd_fastddc_bank_overlap(const csdr_amd_fastddc_bank *b);
int  csdr_amd_fastddc_bank_submit_local(csdr_amd_fastddc_bank *b, const csdr_complexf *in_run, int n_blocks);
/* Integer ingest: the wideband stream as s16 or u8 IQ pairs (what an SDR delivers; the reference puts convert_s16_f / convert_u8_f in front of fastddc_fwd_cc,
 * README.md:66-87, libcsdr.c:2363-2437, csdr.c:2255-2300).  The conversion runs inside the forward transform with the converters' own arithmetic -- the outputs
 * are bit-equal to csdr_amd_convert_s16_f / _u8_f followed by the complexf entry points -- and the stream crosses PCIe (and, in a sharded bank, the root's xGMI
 * links) at 4 or 2 bytes per sample instead of 8.  Matrix-core geometry only (fft 65536 / inverse 512: BASELINE config 4); other geometries: convert first. */
int  csdr_amd_fastddc_bank_process_s16(csdr_amd_fastddc_bank *b, const int16_t *in_iq, int n_blocks, csdr_complexf *out, size_t out_pitch, int *out_counts);
int  csdr_amd_fastddc_bank_process_u8(csdr_amd_fastddc_bank *b, const uint8_t *in_iq, int n_blocks, csdr_complexf *out, size_t out_pitch, int *out_counts);
int  csdr_amd_fastddc_bank_submit_s16(csdr_amd_fastddc_bank *b, const int16_t *in_iq, int n_blocks);
int  csdr_amd_fastddc_bank_submit_u8(csdr_amd_fastddc_bank *b, const uint8_t *in_iq, int n_blocks);
int  csdr_amd_fastddc_bank_submit_local_s16(csdr_amd_fastddc_bank *b, const int16_t *in_run_iq, int n_blocks);
int  csdr_amd_fastddc_bank_submit_local_u8(csdr_amd_fastddc_bank *b, const uint8_t *in_run_iq, int n_blocks);
int  csdr_amd_fastddc_bank_finish(csdr_amd_fastddc_bank *b, int *out_counts);
/* retune by GLOBAL channel number; every rank makes the same call (csdr_amd_fastddc_bank_set_rate takes an index into the rank's own slice; in a time-sliced
 * bank, where every rank computes every channel, a call on one rank only changes that rank's contribution).  A retune takes effect from the next SUBMITTED batch on (csdr.c:2329-2376: the new rate
 * between two reads): a time-sliced bank holds a retune that arrives while batches are staged back until they are collected; every other bank REFUSES it then
 * (-3: collect first) -- part of a staged batch's tables is already fixed. */
int  csdr_amd_fastddc_bank_set_rate_global(csdr_amd_fastddc_bank *b, int channel, float shift_rate);
/* the bank's inverse half (kernel name / profiling: csdr_amd_fastddc_inv_kernel_name, _set_profiling, _kernel_time) */
csdr_amd_fastddc_inv *csdr_amd_fastddc_bank_inverse(csdr_amd_fastddc_bank *b);

/* one channel, one block, explicit taps_fft and status = fastddc_inv_cc itself (fastddc.c:106-166).
 * status_io: HOST {decimation_remain, float starting_phase, output_size} (decimating_shift_addition_status_t).
 * d_inv_in / d_td: device scratch of fft_inv_size complexf (folded bins after the second swap / IFFT output, unnormalised). */
int  csdr_amd_fastddc_inv_block(csdr_amd_ctx *ctx, const csdr_complexf *d_spectrum, const csdr_complexf *d_taps_fft,
                                const csdr_fastddc_t *ddc, void *status_io, csdr_complexf *d_inv_in, csdr_complexf *d_td,
                                csdr_complexf *d_out);

/* ------------------------------------------------------------------ fused WFM receive chain (BASELINE config 2)
 * README.md:66 / csdr-fm:41:  convert_u8_f | shift_addition_cc r | fir_decimate_cc D tbw HAMMING |
 * fmdemod_quadri_cf | fractional_decimator_ff R | deemphasis_wfm_ff fs tau | convert_f_s16
 * for n_streams independent u8 IQ streams in one pass: each input byte is read from HBM once, each
 * audio sample written once.  Streaming: call repeatedly with consecutive blocks; all cross-block state
 * (shift phase, FIR/demod history, de-emphasis state, decimator position) lives in the object.
 * Scope: an FM AUDIO chain.  Its matrix-core front end models the reference's float rotator as C_m D^k per 1024-sample chunk; for rates at which
 * the reference's recurrence (libcsdr_gpl.c:44-45) drifts from that model (1e-5 .. 4e-5 per chunk at e.g. 0.05, 0.25) the deviation is a slowly
 * varying complex factor common to y[k] and y[k-1], which fmdemod_quadri_cf cancels: the audio is within the stated tolerance at every rate
 * (tests/test_edges_gpu.py::test_wfm_other_shift_rates), but the object's INTERNAL complex samples are not a substitute for
 * `convert_u8_f | shift_addition_cc | fir_decimate_cc` at such rates.  The complex front end for that is csdr_amd_ddc_* below, which replays the
 * drift per chunk (k_ddc_corr) and is held to 1e-5 on the complex samples themselves.
 *
 * De-emphasis, tau and audio_rate.  The chain kernels cut a call's audio into time segments; every segment but the call's first starts its one-pole de-emphasis
 * from zero state W samples early, and W is fixed by the code: 48 in the matrix-core chain kernel (two steps of 24 samples; shared rate, rate per stream and the
 * resident ring alike; the ring also rebuilds the state behind a retune over 48), 48 in the fallback's k_wfm_back (csdr_amd_wfm_deemph_warm_samples).  A seam is
 * wrong by b^W of the true state, b = 1 - alpha, alpha = dt / (tau + dt), dt = (float)(1.0 / audio_rate), all in float (libcsdr.c:1090-1091).  The rule
 * csdr_amd_wfm_deemph_exact(tau, audio_rate, W) returns 1 when b^W > 2^-20 (2^-20 of a full-scale state is 0.03 LSB of the s16 audio: below it a seam leaves the
 * chain's +-1 LSB to the front end).  Where it says 1 an object of csdr_amd_wfm_create / _create_rates takes the EXACT route: the same kernels with alpha = 1 (their
 * de-emphasis is then the identity) write float rows owned by the object, and csdr_amd_deemphasis_wfm_ff with the object's carried state and
 * csdr_amd_convert_f_s16 follow: three more small launches and two copies per call, results the reference's at every tau and rate.  Where it says 0 -- the default
 * 50e-6 / 48000 (b^48 = 5.5e-8), 50e-6 / 44100, 5e-6 / 48000 -- nothing changes.  On the exact route at W = 48: 75e-6 / 48000 (7.8e-6), 50e-6 / 96000 (1.1e-4),
 * 75e-6 / 96000 (1.9e-3), 75e-6 / 192000 (4.0e-2), 1e-3 / 48000 (0.37).  csdr_amd_wfm_exact_deemphasis reports the route an object took;
 * csdr_amd_wfm_ring_create refuses the parameters of the exact route. */
int csdr_amd_wfm_deemph_exact(float tau, int audio_rate, int warm_samples);
/* the fewest audio samples a path warms up over.  path 0: the matrix-core chain kernel per call, 1: the fallback (k_wfm_back), 2: the resident ring */
int csdr_amd_wfm_deemph_warm_samples(int path);
typedef struct csdr_amd_wfm csdr_amd_wfm;
csdr_amd_wfm *csdr_amd_wfm_create(csdr_amd_ctx *ctx, int n_streams, float shift_rate, int decimation,
                                  const float *host_taps, int taps_length, int frac_rate,
                                  float tau, int audio_rate, size_t max_block_samples);
/* The same with a shift rate PER STREAM and its retune between calls (the reference's unit of work is one (stream, shift_rate) pair: `csdr shift_addition_cc --fifo`,
 * csdr.c:881-923; ddcd's per-client chains, ddcd_old.h:51-61) -- see csdr_amd_ddc_create_rates.  The chain kernel then gives a workgroup ONE stream and puts 16 time
 * segments of it into the 16 columns of the product; full rate needs blocks of >= 16 x lcm(4 D F, 1024) samples per stream and call (409 600 at D F = 50).
 * Needs the matrix-core kernel's shapes (csdr_amd_wfm_fallback == 0). */
csdr_amd_wfm *csdr_amd_wfm_create_rates(csdr_amd_ctx *ctx, int n_streams, const float *shift_rates, int decimation,
                                        const float *host_taps, int taps_length, int frac_rate,
                                        float tau, int audio_rate, size_t max_block_samples);
int   csdr_amd_wfm_set_rate(csdr_amd_wfm *w, int stream, float shift_rate);
float csdr_amd_wfm_get_rate(const csdr_amd_wfm *w, int stream);
void csdr_amd_wfm_destroy(csdr_amd_wfm *w);
int  csdr_amd_wfm_reset(csdr_amd_wfm *w);
/* in: u8 IQ, [n_streams][in_pitch bytes], block_samples complex samples per stream (multiple of 1024 except
 * for the last block of a stream).  audio_s16: [n_streams][out_pitch]; audio_f (optional, may be NULL)
 * receives the float audio before convert_f_s16 (parity tap).  Returns audio samples written per stream.
 * Any in_pitch that is a multiple of 16 bytes and any audio pointers / out_pitch are accepted; the streaming rate the benchmarks quote needs audio_f == NULL,
 * audio_s16 on a 16-byte boundary and out_pitch a multiple of 8 samples (the kernel then keeps the finished s16 lines in registers and stores 5.5 KiB per stream at
 * a time; other layouts are stored line by line or sample by sample: same values, 5-10 % slower). */
long csdr_amd_wfm_process(csdr_amd_wfm *w, const uint8_t *in, size_t in_pitch, size_t block_samples,
                          int16_t *audio_s16, float *audio_f, size_t out_pitch);
/* name and launch count of the dominant kernel of the last process() call (bench.py roofline leg) */
const char *csdr_amd_wfm_kernel_name(const csdr_amd_wfm *w);
/* 1 when the object runs outside the matrix-core chain kernel (k_wfm_front + k_wfm_back: decimation x audio decimation odd, filters beyond the 256-sample window;
 * CSDR_AMD_WFM_PATH=valu): same results at about a sixth of the rate.  The CLI prints a one-line note on stderr. */
int csdr_amd_wfm_fallback(const csdr_amd_wfm *w);
/* 1 when the object runs its de-emphasis as a pass of its own behind the chain kernel (the exact route above: csdr_amd_wfm_deemph_exact said 1 for its tau, audio
 * rate and the warm-up of the kernel it uses) */
int csdr_amd_wfm_exact_deemphasis(const csdr_amd_wfm *w);
/* sets the de-emphasis state the next call starts from (the reference's last_output, libcsdr.c:1081-1097; a NaN restarts from 0 as there): host float[n_streams] */
int csdr_amd_wfm_set_deemphasis_state(csdr_amd_wfm *w, const float *host_state);
/* as csdr_amd_ddc_seed_stats / csdr_amd_ddc_tables_built (the WFM chain has no drift corrections: out[4] stays 0) */
int  csdr_amd_wfm_seed_stats(const csdr_amd_wfm *w, long out[5]);
long csdr_amd_wfm_tables_built(const csdr_amd_wfm *w);
/* HIP-event timing of that kernel, on the context's stream: enable, run, then read the accumulated time. */
int csdr_amd_wfm_set_profiling(csdr_amd_wfm *w, int on);
int csdr_amd_wfm_kernel_time(csdr_amd_wfm *w, double *total_ms, long *launches);

/* ------------------------------------------------------------------ the RESIDENT form of the fused WFM chain: a persistent grid walking a ring of blocks
 * (north_star: "a persistent-kernel ring buffer so the stdin->stdout pipe never round-trips to host between stages").  The reference's unit of work is one
 * the_bufsize block -- 16384 samples -- per loop iteration of every stage (csdr.c:189-193, 232-247, 330-392); a kernel launch per such block spends most of its time
 * outside the data (launch gap, kernel entry, the de-emphasis warm-up of the time segments a short call is cut into).  A ring object owns
 *     an input ring   [n_slots][n_streams][pitch]  u8 IQ in device memory  -- block seq of every stream lies in slot seq mod n_slots,
 *     an output ring  [n_slots][n_streams][pitch]  s16 audio in device memory,
 * and ONE grid that stays on the GPU, polls block descriptors in host memory (no launch, no stream operation per block) and tells the host through a done word
 * per slot.  Same arithmetic and the same samples as csdr_amd_wfm_process on the same stream cut into the same blocks (tests/test_ring_gpu.py: >= 1000 consecutive
 * 16384-sample blocks with a retune in the middle against the oracle).  Protocol per block:
 *     seq = csdr_amd_wfm_ring_submitted(r);
 *     csdr_amd_wfm_ring_acquire(r, seq, 0);                      -- waits until slot seq mod n_slots may be overwritten (blocks seq - n_slots and seq - n_slots + 1 finished:
 *                                                                   a block's input stays the NEXT block's history)
 *     write [n_streams][2 block_samples] bytes to csdr_amd_wfm_ring_input(r, seq, &pitch)   (any producer: hipMemcpy, a kernel, a peer through HIP IPC) and complete it;
 *     csdr_amd_wfm_ring_submit(r);                               -- posts the block (a store to host memory; relaunches the grid if it has left)
 *     n = csdr_amd_wfm_ring_wait(r, seq, 0);                     -- audio samples per stream of that block, in csdr_amd_wfm_ring_output(r, seq, &pitch); valid until
 *                                                                   block seq + n_slots is posted.  Up to n_slots - 2 blocks may be in flight.
 * The grid never holds the GPU against a silent host: it leaves by itself when no block arrived for idle_us (default 200) or when it is older than life_ms (default
 * 250), and is relaunched by the next submit / wait; no state lives in it: every block warms its de-emphasis up from zero state over the 48 audio samples in front of
 * it, which leaves (1 - alpha)^48 of the true state at a block's first sample.  That is 5.5e-8 at tau = 50e-6 / 48000 and grows with tau and the audio rate, so
 * csdr_amd_wfm_ring_create returns NULL (-3, the message names tau and audio_rate) where csdr_amd_wfm_deemph_exact(tau, audio_rate, 48) is 1 -- e.g. 75e-6 / 48000,
 * 75e-6 / 96000, 1e-3 / 48000: the grid stores s16 straight into the output ring and has no place for a second pass; use csdr_amd_wfm_process there.  While it is
 * resident it occupies every CU it runs on (one workgroup per CU): other kernels of the process wait for it to leave.
 * block_samples: a multiple of 1024, 4096 .. 65536.  Retune: csdr.c:881-923 semantics (from the next posted block's first sample, phase carried). */
typedef struct csdr_amd_wfm_ring csdr_amd_wfm_ring;
csdr_amd_wfm_ring *csdr_amd_wfm_ring_create(csdr_amd_ctx *ctx, int n_streams, float shift_rate, int decimation, const float *host_taps, int taps_length, int frac_rate,
                                            float tau, int audio_rate, size_t block_samples, int n_slots);
void csdr_amd_wfm_ring_destroy(csdr_amd_wfm_ring *r);
int  csdr_amd_wfm_ring_reset(csdr_amd_wfm_ring *r);                                    /* stream start: block 0 next, phase 0 */
int  csdr_amd_wfm_ring_acquire(csdr_amd_wfm_ring *r, long long seq, double timeout_s);  /* timeout_s <= 0: 10 s */
uint8_t *csdr_amd_wfm_ring_input(csdr_amd_wfm_ring *r, long long seq, size_t *pitch_bytes);
long long csdr_amd_wfm_ring_submit(csdr_amd_wfm_ring *r);                              /* returns the block's sequence number, < 0 on error */
long csdr_amd_wfm_ring_wait(csdr_amd_wfm_ring *r, long long seq, double timeout_s);    /* audio samples per stream, < 0 on error / timeout */
const int16_t *csdr_amd_wfm_ring_output(csdr_amd_wfm_ring *r, long long seq, size_t *pitch_samples);
int  csdr_amd_wfm_ring_set_rate(csdr_amd_wfm_ring *r, float shift_rate);               /* drains the ring, rebuilds the weight set; from the next posted block on */
float csdr_amd_wfm_ring_get_rate(const csdr_amd_wfm_ring *r);
int  csdr_amd_wfm_ring_set_timeouts(csdr_amd_wfm_ring *r, double idle_us, double life_ms);
int  csdr_amd_wfm_ring_resident(csdr_amd_wfm_ring *r);                                 /* 1 while the grid is on the GPU */
int  csdr_amd_wfm_ring_stop(csdr_amd_wfm_ring *r);                                     /* asks the grid to leave and waits for it (posted blocks are finished first) */
int  csdr_amd_wfm_ring_slots(const csdr_amd_wfm_ring *r);
int  csdr_amd_wfm_ring_grid(const csdr_amd_wfm_ring *r);                               /* workgroups of the resident grid */
long csdr_amd_wfm_ring_launches(const csdr_amd_wfm_ring *r);                           /* launches of the grid so far */
long long csdr_amd_wfm_ring_submitted(const csdr_amd_wfm_ring *r);
/* where the grid's time went since the last reset (stops the grid): out[0..2] = microseconds per work item (block x 16-stream group) spent waiting for a block, in the
 * chain's body, in the completion; out[3] = items */
int  csdr_amd_wfm_ring_stats(csdr_amd_wfm_ring *r, double out[4]);
/* benchmark / soak aid: posts n_blocks blocks whose inputs are what lies in the ring's slots, as fast as the ring takes them, waits for the last one; t_first_us /
 * t_done_us (NULL or n_blocks doubles) receive every block's start / completion on the device clock */
int  csdr_amd_wfm_ring_replay(csdr_amd_wfm_ring *r, long n_blocks, double *t_first_us, double *t_done_us);
/* device clock (microseconds, arbitrary origin) at which the first workgroup took an item of block seq and at which its last item was finished */
int  csdr_amd_wfm_ring_block_times(csdr_amd_wfm_ring *r, long long seq, double *t_first_us, double *t_done_us);

/* ------------------------------------------------------------------ fused receiver front end (head of the NFM / AM / SSB chains, BASELINE config 5)
 * README.md:87, 95, 110:  convert_u8_f | shift_addition_cc r | fir_decimate_cc D tbw window
 * (libcsdr.c:2363-2368, libcsdr_gpl.c:27-52 in the CLI's 1024-sample chunks csdr.c:911-918, libcsdr.c:528-549 with the CLI's re-feed loop
 * csdr.c:1160-1176) for n_streams independent u8 IQ streams in one pass:  y[k] = sum_t taps[t] x'[D k + t].  Each input byte is read from HBM
 * once; the decimated complex stream is written once.  Streaming: consecutive blocks, all cross-block state (shift phase, FIR history,
 * output index) lives in the object.  taps_length <= 1025. */
typedef struct csdr_amd_ddc csdr_amd_ddc;
csdr_amd_ddc *csdr_amd_ddc_create(csdr_amd_ctx *ctx, int n_streams, float shift_rate, int decimation,
                                  const float *host_taps, int taps_length, size_t max_block_samples);
/* The same with a shift rate PER STREAM -- the reference's unit of work is one (stream, shift_rate) pair: `csdr shift_addition_cc --fifo` retunes a running stream
 * (csdr.c:881-923), ddcd starts one `csdr shift_unroll_cc --fd N | csdr fir_decimate_cc D bw` per client (ddcd_old.h:51-61).  shift_rates: n_streams floats.
 * The matrix-core kernel then gives a workgroup ONE stream and puts 16 time segments of it into the 16 columns of the product (the weights are the stream's own);
 * full rate needs blocks of >= 16 x lcm(8 D, 1024) samples per stream and call (409 600 at D = 50), shorter blocks fill fewer columns.
 * csdr_amd_ddc_set_rate: effective from the next call's first sample, the float phase carries over exactly as the reference's starting_phase does; the outputs of
 * that call whose window still reaches into samples rotated at the old rate are evaluated with both rates.  Returns 0 or a negative error. */
csdr_amd_ddc *csdr_amd_ddc_create_rates(csdr_amd_ctx *ctx, int n_streams, const float *shift_rates, int decimation,
                                        const float *host_taps, int taps_length, size_t max_block_samples);
int   csdr_amd_ddc_set_rate(csdr_amd_ddc *d, int stream, float shift_rate);
float csdr_amd_ddc_get_rate(const csdr_amd_ddc *d, int stream);
/* 1 when the last process() call ran outside the matrix-core kernel (k_ddc_direct: odd decimation, windows beyond 2304 bytes, input pitch not a multiple of 128 bytes,
 * ragged or very short blocks; a rate per stream with fewer than 100 taps while a stream's rate needs drift corrections: the matrix-core kernel applies those once per
 * 288-sample stretch of the window, too coarse for a few taps at its end): same results, a fraction of the rate */
int   csdr_amd_ddc_fallback(const csdr_amd_ddc *d);
/* Which path the per-stream seed tables took since create (read-only, no effect on the stream; a reset does not clear them): out[0] tables generated, out[1] takeovers of
 * a prepared table, out[2] regenerations because the prepared table did not fit the call, out[3] regenerations after a retune, out[4] regrowths of the drift-correction
 * rows in mid-stream.  A negative error on an object that shares one rate.  The NFM and AM/SSB chains: through their *_front_end.
 * csdr_amd_ddc_tables_built: chunk-seed tables built since create -- the host-built table of a shared-rate object (rebuilt 16 calls ahead), out[0] otherwise. */
int   csdr_amd_ddc_seed_stats(const csdr_amd_ddc *d, long out[5]);
long  csdr_amd_ddc_tables_built(const csdr_amd_ddc *d);
void csdr_amd_ddc_destroy(csdr_amd_ddc *d);
int  csdr_amd_ddc_reset(csdr_amd_ddc *d);
/* in: u8 IQ, [n_streams][in_pitch bytes], block_samples complex samples per stream (multiple of 1024 except for the last block of a
 * stream).  out: [n_streams][out_pitch] complexf.  Returns the number of outputs written per stream (all k with D k + taps <= samples so far). */
long csdr_amd_ddc_process(csdr_amd_ddc *d, const uint8_t *in, size_t in_pitch, size_t block_samples,
                          csdr_complexf *out, size_t out_pitch);
const char *csdr_amd_ddc_kernel_name(const csdr_amd_ddc *d);
/* what the last process() call launched: "k_ddc_mfma<13,NT,FUSE,PS> whole" (the matrix-core kernel took the whole call) or "... tiles" (its whole tiles inside the
 * block), followed by " + k_ddc_direct" when the plain kernel ran beside it (edge outputs, the first outputs of retuned streams); "k_ddc_direct" when it ran alone;
 * "" when the call produced no output.  NT: teams per workgroup, FUSE: the NFM chain's demodulating epilogue, PS: a rate per stream. */
const char *csdr_amd_ddc_last_instance(const csdr_amd_ddc *d);
int csdr_amd_ddc_set_profiling(csdr_amd_ddc *d, int on);
int csdr_amd_ddc_kernel_time(csdr_amd_ddc *d, double *total_ms, long *launches);
/* Test hook: CPU evaluation of one tile of the front end's matrix-core kernel with its own weight table, K-range split and chunk-boundary
 * handling (no GPU needed).  window: 2304 raw bytes from sample n0 (multiple of 16); ctab3: (cos, sin) of chunks n0>>10, +1, +2; out16: 8 x (Re, Im). */
int csdr_amd_debug_ddc_mfma_tile(int D, int L, float shift_rate, const float *taps, long long n0, const uint8_t *window,
                                 const float *ctab3, float *out16);

/* ------------------------------------------------------------------ NFM receive chain (BASELINE config 5)
 * README.md:87:  convert_u8_f | shift_addition_cc r | fir_decimate_cc D tbw HAMMING | fmdemod_quadri_cf | limit_ff [max] |
 *                deemphasis_nfm_ff fs | fastagc_ff [block [reference]] | convert_f_s16
 * for n_streams independent u8 IQ streams: front end = csdr_amd_ddc (one pass over the input), back end at the audio rate.  Streaming as the
 * CLI pipeline does it: the de-emphasis FIR re-feeds its unconsumed input (csdr.c:1083), fastagc_ff works on whole blocks with its two-block
 * latency and zero-initialised state (csdr.c:1393-1394); a call returns the whole AGC blocks that became available (a multiple of agc_block,
 * possibly 0).  audio_rate selects the de-emphasis table (48000, 44100, 8000, 11025; libcsdr.c:1115-1119). */
typedef struct csdr_amd_nfm csdr_amd_nfm;
csdr_amd_nfm *csdr_amd_nfm_create(csdr_amd_ctx *ctx, int n_streams, float shift_rate, int decimation, const float *host_taps, int taps_length,
                                  int audio_rate, int agc_block, float agc_reference, float limit_max, size_t max_block_samples);
/* a shift rate per channel, and its retune (csdr_amd_ddc_create_rates / csdr_amd_ddc_set_rate on the chain's front end) */
csdr_amd_nfm *csdr_amd_nfm_create_rates(csdr_amd_ctx *ctx, int n_streams, const float *shift_rates, int decimation, const float *host_taps, int taps_length,
                                        int audio_rate, int agc_block, float agc_reference, float limit_max, size_t max_block_samples);
int  csdr_amd_nfm_set_rate(csdr_amd_nfm *w, int stream, float shift_rate);
void csdr_amd_nfm_destroy(csdr_amd_nfm *w);
int  csdr_amd_nfm_reset(csdr_amd_nfm *w);
/* in: u8 IQ as for csdr_amd_ddc_process.  audio_s16: [n_streams][out_pitch]; audio_f (optional, may be NULL): the float audio before
 * convert_f_s16 (parity tap).  Returns audio samples written per stream. */
long csdr_amd_nfm_process(csdr_amd_nfm *w, const uint8_t *in, size_t in_pitch, size_t block_samples,
                          int16_t *audio_s16, float *audio_f, size_t out_pitch);
/* the chain's front end object (kernel name / profiling: csdr_amd_ddc_kernel_name, csdr_amd_ddc_set_profiling, csdr_amd_ddc_kernel_time) */
csdr_amd_ddc *csdr_amd_nfm_front_end(csdr_amd_nfm *w);

/* ------------------------------------------------------------------ the NFM receive bank on baseband (fmrx.hip)
 *   fmdemod_quadri_cf | limit_ff [max_amp] | deemphasis_nfm_ff <audio_rate> | fastagc_ff [block [reference]] | convert_f_s16
 * for n_channels rows of decimated complex baseband on the device (the output of csdr_amd_fastddc_bank, csdr_amd_ddc_process, csdr_amd_fir_decimate_cc): the tail of
 * csdr_amd_nfm without its u8 front end, in the same stream model and with the same arithmetic.  Per channel: the demodulator starts from the sample (0, 0) and a
 * zero denominator gives 0; the de-emphasis FIR runs over (1024 zeros ++ limited stream), as `csdr deemphasis_nfm_ff` does at the default buffer size, as an exact
 * integer product on three base-256 digits per sample; fastagc_ff works on whole blocks of agc_block samples from a zeroed state, so the first two blocks are 0.
 * The channels advance in lockstep: a call gives every channel n_in samples.  With `fill` the filter input the object holds (1024 after a reset) and Ld the taps of
 * csdr_amd_nfm_deemph_taps(audio_rate), a call writes ne = ((fill + n_in - Ld) / agc_block) * agc_block samples per channel (0 when that is not positive) and then
 * holds fill + n_in - ne: csdr_amd_fmrx_plan, a host function.  The audio has the same bits however the stream is cut into calls, on either kernel path, and fed with
 * the rows of csdr_amd_ddc_process it has the bits of csdr_amd_nfm on the same u8 input.  Inputs are finite; Inf and NaN behave as they do in csdr_amd_nfm.
 * create: NULL with a message when audio_rate has no table, the taps exceed the matrix-core tile (241), agc_block is not a multiple of 16 in 16 .. 1536, limit_max <= 0,
 * n_channels < 1 (or > 65535) or max_samples_per_call is not in 1 .. 2^30.
 * process: in (device) [n_channels][in_pitch complexf]; audio_s16 and audio_f (the float audio in front of convert_f_s16), both device, [n_channels][out_pitch], either
 * may be NULL.  Returns the samples written per channel; -3 when n_in > max_samples_per_call, or when out_pitch < ne with more than one channel (nothing has changed
 * then).  n_in = 0 does nothing.  Asynchronous on the context's stream.
 * max_output: the largest ne of a call of n_in samples whatever the object holds (max_out: the same, the name the other banks use).
 * reset_channel: one channel's held input, previous sample and AGC state to zero; `fill` is the bank's and stays, the other channels carry on.
 * kernel_name: the path of the last call: "k_fmrx_front" (agc_block 1024, 16-byte aligned rows, even in_pitch: the rows are read, demodulated and filtered in one
 * kernel) or "k_nfm_deemph_mfma" (csdr_amd_nfm's separate launches; every shape; force_generic(1)).  Both give the same bits, and a stream may change between them. */
typedef struct csdr_amd_fmrx csdr_amd_fmrx;
csdr_amd_fmrx *csdr_amd_fmrx_create(csdr_amd_ctx *ctx, int n_channels, int audio_rate, int agc_block, float agc_reference, float limit_max, size_t max_samples_per_call);
long long csdr_amd_fmrx_process(csdr_amd_fmrx *o, const csdr_complexf *in, size_t in_pitch, long long n_in, int16_t *audio_s16, float *audio_f, size_t out_pitch);
long long csdr_amd_fmrx_max_output(const csdr_amd_fmrx *o, long long n_in);
long long csdr_amd_fmrx_max_out(const csdr_amd_fmrx *o, long long n_in);
int  csdr_amd_fmrx_plan(int fill, long long n_in, int taps_length, int agc_block, long long *ne, int *new_fill);
int  csdr_amd_fmrx_fill(const csdr_amd_fmrx *o);
int  csdr_amd_fmrx_reset(csdr_amd_fmrx *o);
int  csdr_amd_fmrx_reset_channel(csdr_amd_fmrx *o, int channel);
int  csdr_amd_fmrx_force_generic(csdr_amd_fmrx *o, int on);
const char *csdr_amd_fmrx_kernel_name(const csdr_amd_fmrx *o);
void csdr_amd_fmrx_destroy(csdr_amd_fmrx *o);
/* The same bank with squelch_and_smeter_cc (csdr.c:2192-2243) in front of every channel's demodulator:
 *   squelch_and_smeter_cc | fmdemod_quadri_cf | limit_ff | deemphasis_nfm_ff | fastagc_ff | convert_f_s16
 * create_squelched: squelch_block B in 1 .. 65536, use_every_nth >= 1, levels: n_channels host floats or NULL (all 0: always open); else NULL with a message.
 * The squelch cuts a channel's input into blocks of B samples counted from the reset.  Only whole blocks go on to the demodulator, a closed block as B samples
 * (0, 0) (which demodulate to silence: the zero-denominator branch); what lies behind the last whole block, at most B - 1 complexf per channel, waits in the object.
 * With `held` waiting, a call of n_in samples advances the chain by m = (held + n_in) / B * B gated samples and then holds held + n_in - m
 * (csdr_amd_fmrx_squelch_plan, a host function); csdr_amd_fmrx_plan applies to m as it does to n_in without a squelch, and max_output counts B - 1 samples more.
 * The power of a block is csdr_amd_squelch's (the same bits), its gate level == 0 || power >= level, its level the one in force when its first sample
 * arrived: set_squelch_level (channel -1: all) reaches the block under way only when nothing of it is held yet.  squelch_held and squelch_block_index (the
 * blocks completed since the reset) are the bank's: the channels advance in lockstep.
 * process_squelched: as process; power (float) and open_flags (u8), both device, [n_channels][power_pitch], either may be NULL, get one entry per block the
 * call completed, *n_blocks (may be NULL) their number.  -3 and no change when power_pitch is below that number while one of the two is given.  process on a
 * squelched object is this call without the two rows.  The entry points of this paragraph return -3 on an object created without a squelch.
 * reset starts the block count and the held samples over and keeps the levels; reset_channel also zeroes the channel's held squelch samples, the block phase
 * is the bank's and stays.
 * kernel_name: "k_fmrx_front_sq" (the shapes of "k_fmrx_front", any n_in: k_fmrx_power reads the samples once for the block powers, the front kernel then gates
 * them as it loads them and skips closed blocks; the gated rows never exist in memory) or "k_nfm_deemph_mfma" (an internal csdr_amd_squelch writes gated rows,
 * the separate launches run over them; every shape; force_generic(1)).  Both give the bits of csdr_amd_squelch followed by csdr_amd_fmrx. */
csdr_amd_fmrx *csdr_amd_fmrx_create_squelched(csdr_amd_ctx *ctx, int n_channels, int audio_rate, int agc_block, float agc_reference, float limit_max,
                                              size_t max_samples_per_call, int squelch_block, int use_every_nth, const float *levels);
long long csdr_amd_fmrx_process_squelched(csdr_amd_fmrx *o, const csdr_complexf *in, size_t in_pitch, long long n_in, int16_t *audio_s16, float *audio_f, size_t out_pitch,
                                          float *power, size_t power_pitch, uint8_t *open_flags, int *n_blocks);
int  csdr_amd_fmrx_squelch_plan(int held, long long n_in, int block, long long *m, int *new_held);
int  csdr_amd_fmrx_set_squelch_level(csdr_amd_fmrx *o, int channel, float level);
int  csdr_amd_fmrx_get_squelch_level(const csdr_amd_fmrx *o, int channel, float *level);
int  csdr_amd_fmrx_squelch_held(const csdr_amd_fmrx *o);
long long csdr_amd_fmrx_squelch_block_index(const csdr_amd_fmrx *o);

/* ------------------------------------------------------------------ the WFM receive bank on baseband (wfmrx.hip)
 *   fmdemod_quadri_cf | fractional_decimator_ff <rate> [num_poly_points] [--prefilter] | deemphasis_wfm_ff <audio_rate> <tau> | convert_f_s16
 * for n_channels rows of decimated complex baseband on the device: the tail of the reference README's first receive line behind csdr_amd_fastddc_bank,
 * csdr_amd_ddc_process or csdr_amd_fir_decimate_cc.  The stream model is the four commands' at the default buffer size.  Per channel: the demodulator starts
 * from the sample (0, 0) and a zero denominator gives 0; the decimator is called on windows of `window` demodulated samples from the first unprocessed one
 * (csdr.c:1513-1524), the unprocessed tail is presented again and `where` is carried; the de-emphasis is the reference's recurrence from state 0 (a NaN state
 * restarts at 0); convert_f_s16 truncates.  The channels advance in lockstep: `where`, the count of held samples and the plan are the bank's; a channel has its
 * previous sample, its held floats (at most window - 1) and its de-emphasis state.  A window is processed once `window` samples from the first unprocessed one are
 * there, so a fresh object writes its first outputs in the call that completes sample number `window`.  What a call writes and keeps depends on
 * (rate, num_poly_points, taps_length, window, where, held, n_in) only: csdr_amd_wfmrx_plan, a host function (window 0: 1024).  The audio has the same bits
 * however the stream is cut into calls and on either kernel path.  Inputs are finite.
 * create: NULL with a message "wfmrx: ..." when rate <= 1, num_poly_points is odd or outside 2 .. 64, n_channels < 1 (or > 65535), max_samples_per_call is not in
 * 1 .. 2^30, tau <= 0, or the window and the rate do not fit: a window call advances by (ceilf(where) - 1) + xifirst samples, which is at least 1 and at most
 * `window` when   window >= 3 * num_poly_points / 2 + taps_length + 1   and   ceil(rate) <= 3 * num_poly_points / 2 + taps_length + 1   (sufficient; both are
 * checked, by plan as well).  host_prefilter_taps NULL: no prefilter (taps_length is not read).
 * process: in (device) [n_channels][in_pitch complexf]; audio_s16 and audio_f (the float audio in front of convert_f_s16), both device, [n_channels][out_pitch],
 * either may be NULL.  Returns the samples written per channel; -3 when n_in > max_samples_per_call, or when out_pitch is below that count with more than one
 * channel (nothing has changed then).  n_in = 0 does nothing.  Asynchronous on the context's stream, except that a rate which is not exact in float uploads its
 * positions synchronously, as csdr_amd_fractional_decimator_ff does.
 * max_output: a bound on what a call of n_in samples writes whatever the object holds (max_out: the same, the name the other banks use).
 * reset_channel: one channel's previous sample, held floats and de-emphasis state to zero, which is a fresh object's channel whose earlier input was all zeros;
 * `where` and `held` are the bank's and stay, the other channels carry on.
 * kernel_name: the path of the last call: "k_wfmrx_front" (no prefilter, num_poly_points <= 16, 16-byte aligned rows, even in_pitch: the rows
 * are read, demodulated and interpolated in one kernel, k_wfmrx_tail de-emphasises and converts) or "k_fracdec" (the stand-alone entry points composed; every shape;
 * force_generic(1)).  Both give the same bits, and a stream may change between them. */
typedef struct csdr_amd_wfmrx csdr_amd_wfmrx;
csdr_amd_wfmrx *csdr_amd_wfmrx_create(csdr_amd_ctx *ctx, int n_channels, float rate, int num_poly_points, const float *host_prefilter_taps, int taps_length, int window,
                                      float tau, int audio_rate, size_t max_samples_per_call);
long long csdr_amd_wfmrx_process(csdr_amd_wfmrx *o, const csdr_complexf *in, size_t in_pitch, long long n_in, int16_t *audio_s16, float *audio_f, size_t out_pitch);
long long csdr_amd_wfmrx_max_output(const csdr_amd_wfmrx *o, long long n_in);
long long csdr_amd_wfmrx_max_out(const csdr_amd_wfmrx *o, long long n_in);
int  csdr_amd_wfmrx_plan(float rate, int num_poly_points, int taps_length, int window, float where, int held, long long n_in, long long *n_out, float *new_where, int *new_held);
int  csdr_amd_wfmrx_held(const csdr_amd_wfmrx *o);
float csdr_amd_wfmrx_where(const csdr_amd_wfmrx *o);
int  csdr_amd_wfmrx_reset(csdr_amd_wfmrx *o);
int  csdr_amd_wfmrx_reset_channel(csdr_amd_wfmrx *o, int channel);
int  csdr_amd_wfmrx_force_generic(csdr_amd_wfmrx *o, int on);
const char *csdr_amd_wfmrx_kernel_name(const csdr_amd_wfmrx *o);
void csdr_amd_wfmrx_destroy(csdr_amd_wfmrx *o);
/* The same bank with squelch_and_smeter_cc (csdr.c:2192-2243) in front of every channel's demodulator:
 *   squelch_and_smeter_cc | fmdemod_quadri_cf | fractional_decimator_ff | deemphasis_wfm_ff | convert_f_s16
 * The interface is csdr_amd_fmrx's squelched one, name for name, and so are the rules.  create_squelched: squelch_block B in 1 .. 65536, use_every_nth >= 1,
 * levels: n_channels host floats or NULL (all 0: always open); else NULL with a message "wfmrx: ...", as for everything create refuses.
 * The squelch cuts a channel's input into blocks of B samples counted from the reset.  Only whole blocks go on to the demodulator, a closed block as B samples
 * (0, 0); what lies behind the last whole block, at most B - 1 complexf per channel, waits in the object.  With `held` waiting, a call of n_in samples advances
 * the chain by m = (held + n_in) / B * B gated samples and then holds held + n_in - m (csdr_amd_wfmrx_squelch_plan, a host function); csdr_amd_wfmrx_plan
 * applies to m as it does to n_in without a squelch, and max_output counts B - 1 samples more.  Behind the gate the model above applies to the gated stream: the
 * demodulator's previous sample is the last gated one, (0, 0) behind a closed block; a zero sample demodulates to 0; the de-emphasis runs on through closed
 * stretches (it decays, it is not reset).
 * The power of a block is csdr_amd_squelch's (the same bits), its gate level == 0 || power >= level, its level the one in force when its first sample
 * arrived: set_squelch_level (channel -1: all) reaches the block under way only when nothing of it is held yet.  squelch_held and squelch_block_index (the
 * blocks completed since the reset) are the bank's: the channels advance in lockstep.
 * process_squelched: as process; power (float) and open_flags (u8), both device, [n_channels][power_pitch], either may be NULL, get one entry per block the
 * call completed, *n_blocks (may be NULL) their number.  -3 and no change when power_pitch is below that number while one of the two is given, when out_pitch
 * is too small or n_in > max_samples_per_call.  process on a squelched object is this call without the two rows.  The entry points of this paragraph return
 * -3 on an object created without a squelch.
 * reset starts the block count and the held samples over and keeps the levels; reset_channel also zeroes the channel's held squelch samples, the block phase
 * is the bank's and stays.
 * kernel_name: "k_wfmrx_front_sq" (the shapes of "k_wfmrx_front", any n_in and any B: k_fmrx_power reads the samples once for the block powers, the front
 * kernel then gates them as it loads them and does not fetch closed blocks; the gated rows never exist in memory) or "k_fracdec" (an internal csdr_amd_squelch
 * writes gated rows, the generic path runs over them; every shape; force_generic(1)).  Both give the bits of csdr_amd_squelch followed by csdr_amd_wfmrx, and a
 * stream may change between them. */
csdr_amd_wfmrx *csdr_amd_wfmrx_create_squelched(csdr_amd_ctx *ctx, int n_channels, float rate, int num_poly_points, const float *host_prefilter_taps, int taps_length,
                                                int window, float tau, int audio_rate, size_t max_samples_per_call, int squelch_block, int use_every_nth,
                                                const float *levels);
long long csdr_amd_wfmrx_process_squelched(csdr_amd_wfmrx *o, const csdr_complexf *in, size_t in_pitch, long long n_in, int16_t *audio_s16, float *audio_f, size_t out_pitch,
                                           float *power, size_t power_pitch, uint8_t *open_flags, int *n_blocks);
int  csdr_amd_wfmrx_squelch_plan(int held, long long n_in, int block, long long *m, int *new_held);
int  csdr_amd_wfmrx_set_squelch_level(csdr_amd_wfmrx *o, int channel, float level);
int  csdr_amd_wfmrx_get_squelch_level(const csdr_amd_wfmrx *o, int channel, float *level);
int  csdr_amd_wfmrx_squelch_held(const csdr_amd_wfmrx *o);
long long csdr_amd_wfmrx_squelch_block_index(const csdr_amd_wfmrx *o);

/* ------------------------------------------------------------------ the AM and SSB receive chains (amssb.hip)
 * README.md:95   ... | amdemod_cf | fastdcblock_ff | agc_ff | limit_ff | convert_f_s16
 * README.md:110  ... | bandpass_fir_fft_cc lo hi tbw | realpart_cf | agc_ff | limit_ff | convert_f_s16
 * for n_channels channels: the parameters are shared, each channel has its own state {last_dc, last_gain}, kept on the device between calls.  The tail works on
 * whole blocks of `block` samples, 2 .. 16384: fastdcblock_ff's buffer and agc_ff's call length, the CLI's situation when fastdcblock_ff announces its buffer size and
 * agc_ff adopts it (in SSB only the AGC's call length).  Every float operation is the reference's, in its order (amssb_dev.hpp); only the order of fastdcblock_ff's
 * block sum, which the reference leaves to its compiler, is fixed here.  A stream in one call and any cut of it into calls (0 samples included), any pitch,
 * any set_lanes and either kernel give the same bits as csdr_amd_debug_amssb_walk.
 * params_default: mode, block 1024, agc_ff's CLI defaults (csdr.c:1342-1361: hang_time 200, reference 0.2, attack_rate 0.01, decay_rate 0.0001, max_gain 65536,
 * attack_wait_time 0, gain_filter_alpha 0.999) and limit_max 1.
 * create_cf32: the input is decimated complex baseband (the output of csdr_amd_fastddc_bank, csdr_amd_ddc_process, csdr_amd_fir_decimate_cc), in_pitch in complex
 * samples.  create / create_rates: the input is wideband u8 IQ per channel through an owned csdr_amd_ddc (one shift rate, or one per channel; ddc_taps: the real
 * decimation filter), in_pitch in bytes, n_in in complex samples with that object's rules; set_rate / get_rate forward to it, front_end returns it.
 * taps, taps_length, fft_size (SSB only; taps_length 0: no filter): host complex taps of an owned csdr_amd_fftfilt in front of realpart_cf, the passband of every
 * channel until one is given its own.
 * set_passband: channel's taps become firdes_bandpass_c(taps_length, low, high, window), as bandpass_fir_fft_cc designs them (the length is the object's: one
 * transition bandwidth for the bank).  set_channel_taps: any taps of that length.  get_passband: the edges last set for the channel; NaN after set_channel_taps and
 * before any set_passband (the object does not know what its creation taps pass).  All three need an SSB object with a filter (AM has none: negative status).
 * A change lands at the first sample the owned filter has not consumed yet: the object holds back input short of one input_size = fft_size - taps_length + 1, and
 * those samples, like all later ones, are filtered with the new taps (over the history of the old input, as a retuned bandpass_fir_fft_cc --fifo does).
 * reset and reset_channel keep every channel's passband.
 * max_samples_per_call: the most n_in of a call.
 * process: in (device), n_in new samples per channel.  Carried per channel between calls: the state, the complex samples short of a whole block and the filter's
 * input short of one input_size.  Writes the whole blocks that became available to audio_s16 and, when it is not NULL, the float samples in front of agc_ff to
 * pre_agc_f (both device, out_pitch elements apart) and returns their count per channel: a multiple of block, possibly 0.  Nothing is written beyond the count.
 * Asynchronous on the context's stream.  reset_channel / set_channel touch the two state words only.
 * set_lanes: channels per wave, 0 = automatic .. 64.  kernel_name: "k_amssb_tiled<AM>" / "k_amssb_tiled<SSB>" (staged through LDS in coalesced tiles; block a
 * multiple of 64 and 8-byte aligned input) or "k_amssb_generic<AM>" / "k_amssb_generic<SSB>" (one lane per channel on global memory; force_generic(1)). */
enum { CSDR_AMD_AMSSB_AM = 0, CSDR_AMD_AMSSB_SSB = 1 };
typedef struct csdr_amd_amssb_params {
    int mode, block;
    float reference, attack_rate, decay_rate, max_gain;
    short hang_time, attack_wait_time;
    float gain_filter_alpha, limit_max;
} csdr_amd_amssb_params;
typedef struct csdr_amd_amssb_chan { float last_dc, last_gain; } csdr_amd_amssb_chan;
typedef struct csdr_amd_amssb csdr_amd_amssb;
int  csdr_amd_amssb_params_default(csdr_amd_amssb_params *p, int mode);
csdr_amd_amssb *csdr_amd_amssb_create_cf32(csdr_amd_ctx *ctx, const csdr_amd_amssb_params *params, int n_channels, const csdr_complexf *taps, int taps_length,
                                           int fft_size, size_t max_samples_per_call);
csdr_amd_amssb *csdr_amd_amssb_create(csdr_amd_ctx *ctx, const csdr_amd_amssb_params *params, int n_channels, float shift_rate, int decimation,
                                      const float *ddc_taps, int ddc_taps_length, const csdr_complexf *taps, int taps_length, int fft_size,
                                      size_t max_samples_per_call);
csdr_amd_amssb *csdr_amd_amssb_create_rates(csdr_amd_ctx *ctx, const csdr_amd_amssb_params *params, int n_channels, const float *shift_rates, int decimation,
                                            const float *ddc_taps, int ddc_taps_length, const csdr_complexf *taps, int taps_length, int fft_size,
                                            size_t max_samples_per_call);
long long csdr_amd_amssb_process(csdr_amd_amssb *p, const void *in, size_t in_pitch, long long n_in, int16_t *audio_s16, float *pre_agc_f, size_t out_pitch);
long long csdr_amd_amssb_max_out(const csdr_amd_amssb *p, long long n_in);
int  csdr_amd_amssb_set_rate(csdr_amd_amssb *p, int channel, float shift_rate);
float csdr_amd_amssb_get_rate(const csdr_amd_amssb *p, int channel);
csdr_amd_ddc *csdr_amd_amssb_front_end(csdr_amd_amssb *p);
int  csdr_amd_amssb_set_passband(csdr_amd_amssb *p, int channel, float low, float high, int window);
int  csdr_amd_amssb_set_channel_taps(csdr_amd_amssb *p, int channel, const csdr_complexf *taps, int taps_length);
int  csdr_amd_amssb_get_passband(const csdr_amd_amssb *p, int channel, float *low, float *high);
int  csdr_amd_amssb_reset(csdr_amd_amssb *p);
int  csdr_amd_amssb_reset_channel(csdr_amd_amssb *p, int channel);
int  csdr_amd_amssb_get_channel(csdr_amd_amssb *p, int channel, csdr_amd_amssb_chan *out);
int  csdr_amd_amssb_set_channel(csdr_amd_amssb *p, int channel, const csdr_amd_amssb_chan *state);
int  csdr_amd_amssb_set_lanes(csdr_amd_amssb *p, int lanes);
int  csdr_amd_amssb_lanes(const csdr_amd_amssb *p);
int  csdr_amd_amssb_force_generic(csdr_amd_amssb *p, int on);
const char *csdr_amd_amssb_kernel_name(const csdr_amd_amssb *p);
void csdr_amd_amssb_destroy(csdr_amd_amssb *p);
/* the kernels' functions on the host for one channel (params->mode: which chain): in holds n_blocks * params->block complex samples; state_io (may be NULL: a fresh
 * channel) carries the state in and out; either output may be NULL.  Returns n_blocks * block or a negative code. */
long long csdr_amd_debug_amssb_walk(const csdr_amd_amssb_params *params, const csdr_complexf *in, int n_blocks, csdr_amd_amssb_chan *state_io, int16_t *s16_out,
                                    float *pre_agc_out);
/* The squelch and S-meter inside the object: squelch_and_smeter_cc at the tail's input (behind the owned front end and filter), per channel
 *   squelch_and_smeter_cc | amdemod_cf | fastdcblock_ff | agc_ff | limit_ff | convert_f_s16          (realpart_cf for amdemod_cf | fastdcblock_ff in SSB)
 * The squelch block is the object's block and is counted from the reset, for all channels in lockstep; the samples short of a block that the object carries
 * serve both.  The power of a block is csdr_amd_squelch's, bit for bit (use_every_nth: every n-th sample enters, the divisor is the block); a block passes if
 * its level is 0 or its power >= the level, else it goes on as (0, 0) samples.  A block's level is the one in force when its first sample reached the tail's
 * input, so set_squelch_level between calls gives the flags csdr_amd_squelch_set_level gives at the same call boundaries.  The outputs are, in every bit, those
 * of a csdr_amd_squelch in front of an unsquelched object; closed blocks are not loaded, and once fastdcblock_ff's level has reached 0 they are not walked either.
 * enable_squelch: levels holds n_channels floats (NULL: 0, open), on any creation form; only while the object has taken no sample since its creation or its last
 * reset, and only with limit_max >= 0 (-3 otherwise, nothing changed).  There is no way back.  reset clears the block index and the held samples and keeps the
 * levels; reset_channel and set_channel stay the two state words.
 * process_squelched: as process; power and open_flags (device, [n_channels][power_pitch], either may be NULL) receive one entry per block the call completed,
 * *n_blocks_out (may be NULL) their count.  power_pitch must hold the blocks the call can complete: exactly those of this call for CF32 input, max_out(n_in) /
 * block behind an owned front end (-3 otherwise, nothing changed).  process on such an object is process_squelched without the rows.
 * set_squelch_level: channel -1 = all.  squelch_block_index: the blocks completed since the reset.  Every squelch call on an object without one returns -3.
 * kernel_name: "k_amssb_tiled_sq<AM>" / "k_amssb_tiled_sq<SSB>" / "k_amssb_generic_sq<AM>" / "k_amssb_generic_sq<SSB>". */
int  csdr_amd_amssb_enable_squelch(csdr_amd_amssb *p, int use_every_nth, const float *levels);
long long csdr_amd_amssb_process_squelched(csdr_amd_amssb *p, const void *in, size_t in_pitch, long long n_in, int16_t *audio_s16, float *pre_agc_f, size_t out_pitch,
                                           float *power, size_t power_pitch, uint8_t *open_flags, int *n_blocks_out);
int  csdr_amd_amssb_set_squelch_level(csdr_amd_amssb *p, int channel, float level);
int  csdr_amd_amssb_get_squelch_level(const csdr_amd_amssb *p, int channel, float *level);
long long csdr_amd_amssb_squelch_block_index(const csdr_amd_amssb *p);
/* agc_ff over n zero samples, as the kernels take it (amssb_dev.hpp's amssb_agc_zero_run): the gain behind them; *steps_iterated (may be NULL): how many
 * of the n steps were taken one by one before a cycle of the gain (period <= 4) was found.  NaN and a message on bad arguments. */
float csdr_amd_debug_amssb_zero_run(const csdr_amd_amssb_params *params, float gain, long long n, long long *steps_iterated);

/* Test hook: one tile of the WFM chain kernel (k_wfm_mfma_seq: phase-independent weight set, post factors, chunk-boundary handling) on the CPU.
 * n0: window base sample (multiple of 8); window: 512 raw bytes; ctab2: (cos, sin) of chunks n0>>10, +1; out16: 16 rows. */
int csdr_amd_debug_wfm_seq_tile(int D, int L, int F, float shift_rate, const float *taps, long long n0, const uint8_t *window,
                                const float *ctab2, float *out16);
/* Test hook: the register-level 16-point butterfly of the three-pass 65536-point transform (fft64k.hip) on the CPU; 16 interleaved complex floats */
void csdr_amd_debug_dft16(const float *in32, float *out32, int inverse);
/* Test hook: the 8-point butterfly of the channelizer's 512-point inverse transforms (fastddc_mfma.hip) on the CPU; 8 interleaved complex floats */
int  csdr_amd_debug_fftfilt_lds(int n, const float *taps_iq, int taps_len, const float *x_iq, long m_new, float *y_iq);   /* CPU run of the one-pass filter kernel's stages */
void csdr_amd_debug_dft8(const float *in16, float *out16, int inverse);
/* Test hook: the channelizer's residual-shift bookkeeping (decimating_shift_addition_cc's (remain, phase) per block, libcsdr_gpl.c:153-158) over n_blocks blocks on the
 * CPU; mode 0 = the general step, mode 1 = the constant-step fast path of the kernels (-1 when it does not apply).  phases_out[b] = phase in front of block b. */
int  csdr_amd_debug_ddc_chain(int mode, float rate2, int post_in, int post_dec, int n_blocks, int *remain_io, float *phase_io, float *phases_out, int *count_out);
/* Test hook: how the channelizer's matrix-core fold tiles a call of n_blocks blocks at `pre_decimation` (32-block accumulator tiles per workgroup, bytes of LDS of one
 * spectra buffer); -1 when the path declines the geometry because not even one tile fits a workgroup's 160 KiB (the general kernels serve it). */
int  csdr_amd_debug_ddc_fold_plan(int pre_decimation, int n_blocks, int *tiles, long *lds_bytes);
/* Test hook: one tile (16 outputs from 256 limited samples) of the NFM chain's matrix-core de-emphasis FIR on the CPU: digit planes,
 * Toeplitz digit table and accumulator classes as k_nfm_deemph_mfma combines them. */
int csdr_amd_debug_nfm_deemph_tile(int audio_rate, float max_amp, const float *x, float *out16);
/* Test hook: the one-pass waterfall kernel's stages (k_wf_onepass) on the CPU for the first row of a fresh stream (fft_size 1024 / 2048 / 4096 / 8192):
 * in holds n_in samples (cf32 or u8 IQ pairs; floats or shorts for the real formats, fft_size then being the output bins) from the stream's start.
 * db_row: the row as the object writes it (halves exchanged; a real format's row is one-sided, DC first); power_row (may be null):
 * the summed |X|^2 in the same order.  Returns 0, or -3 when the row's frames are not all within n_in. */
int csdr_amd_debug_waterfall_row(int fft_size, int every_n_samples, int window, int avgnumber, float add_db, int in_format, const void *in, long long n_in,
                                 float *db_row, float *power_row);
/* the same for row `row` (0 = the first) of the stream that in holds from its start */
int csdr_amd_debug_waterfall_row_at(int fft_size, int every_n_samples, int window, int avgnumber, float add_db, int in_format, const void *in, long long n_in,
                                    int row, float *db_row, float *power_row);
#ifdef __cplusplus
}
#endif
#endif
