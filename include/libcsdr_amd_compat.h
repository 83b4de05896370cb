/* include/libcsdr_amd_compat.h -- the reference's own C API, served by libcsdr_amd.so.
 *
 * Same symbol names, argument order, by-value state conventions and struct layouts as
 *   libcsdr.h:46-229, libcsdr_gpl.h:26-46, fastddc.h:5-29, fft_fftw.h:14-27
 * (layouts checked against the compiled reference in tests/test_abi.py), so a program
 * written against the reference headers links against libcsdr_amd.so unchanged.
 *
 * All pointers are HOST pointers: each call copies its block to the MI355X, runs the same HIP kernels as
 * the device batch API (include/csdr_amd.h) and copies the result back before returning, i.e. it appears
 * synchronous like the reference.  Per-call PCIe + launch latency makes this the compatibility path, not the
 * fast path; throughput work goes through the batch API / the csdr CLI shim.
 * Threads: like the reference's functions these keep no hidden state and may be called from several host threads at once; the library keeps one
 * device context (stream + staging) per calling thread, released when that thread exits.
 * There is NO CPU fallback: without a gfx950 device the first call prints the reason and aborts.
 */
#ifndef LIBCSDR_AMD_COMPAT_H
#define LIBCSDR_AMD_COMPAT_H
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct complexf_s { float i; float q; } complexf;                          /* libcsdr.h:46 */
typedef enum window_s { WINDOW_BOXCAR, WINDOW_BLACKMAN, WINDOW_HAMMING } window_t;   /* libcsdr.h:70-73 */
#define WINDOW_DEFAULT WINDOW_HAMMING

/* FFT plan layer, fft_fftw.h:14-27 */
#define FFT_PLAN_T struct fft_plan_s
struct fft_plan_s { int size; void *input; void *output; void *plan; };
FFT_PLAN_T *make_fft_c2c(int size, complexf *input, complexf *output, int forward, int benchmark);
FFT_PLAN_T *make_fft_r2c(int size, float *input, complexf *output, int benchmark);
FFT_PLAN_T *make_fft_c2r(int size, complexf *input, float *output, int benchmark);
void fft_execute(FFT_PLAN_T *plan);
void fft_destroy(FFT_PLAN_T *plan);
void *csdr_fft_malloc(size_t n);      /* the reference's fft_malloc/fft_free are FFTW macros (fft_fftw.h:11-12) */
void csdr_fft_free(void *p);
#define fft_malloc csdr_fft_malloc
#define fft_free csdr_fft_free
void *fftwf_malloc(size_t n);          /* what the REFERENCE's fft_fftw.h:11-12 expands fft_malloc / fft_free to: exported too, so a client built against */
void fftwf_free(void *p);              /* the reference headers links without -lfftw3f */

/* filter design, libcsdr.h:85-92 */
void firdes_lowpass_f(float *output, int length, float cutoff_rate, window_t window);
void firdes_bandpass_c(complexf *output, int length, float lowcut, float highcut, window_t window);
float firdes_wkernel_blackman(float input);
float firdes_wkernel_hamming(float input);
float firdes_wkernel_boxcar(float input);
window_t firdes_get_window_from_string(char *input);
char *firdes_get_string_from_window(window_t window);
int firdes_filter_len(float transition_bw);
void normalize_fir_f(float *input, float *output, int length);

/* demodulators, libcsdr.h:95-100 */
complexf fmdemod_quadri_cf(complexf *input, float *output, int input_size, float *temp, complexf last_sample);
complexf fmdemod_quadri_novect_cf(complexf *input, float *output, int input_size, complexf last_sample);
void limit_ff(float *input, float *output, int input_size, float max_amplitude);

/* filters, decimators, shift, libcsdr.h:103-108 */
float fir_one_pass_ff(float *input, float *taps, int taps_length);
int fir_decimate_cc(complexf *input, complexf *output, int input_size, int decimation, float *taps, int taps_length);
int deemphasis_nfm_ff(float *input, float *output, int input_size, int sample_rate);
float deemphasis_wfm_ff(float *input, float *output, int input_size, float tau, int sample_rate, float last_output);
float shift_math_cc(complexf *input, complexf *output, int input_size, float rate, float starting_phase);

typedef struct fastagc_ff_s {                                                       /* libcsdr.h:118-128 */
    float *buffer_1; float *buffer_2; float *buffer_input;
    float peak_1; float peak_2; int input_size; float reference; float last_gain;
} fastagc_ff_t;
void fastagc_ff(fastagc_ff_t *input, float *output);

typedef struct fractional_decimator_ff_s {                                          /* libcsdr.h:151-168 */
    float where; int input_processed; int output_size; int num_poly_points;
    float *poly_precalc_denomiator; float *coeffs_buf; float *filtered_buf;
    int xifirst; int xilast; float rate; float *taps; int taps_length;
} fractional_decimator_ff_t;
fractional_decimator_ff_t fractional_decimator_ff_init(float rate, int num_poly_points, float *taps, int taps_length);
void fractional_decimator_ff(float *input, float *output, int input_size, fractional_decimator_ff_t *d);

int fir_interpolate_cc(complexf *input, complexf *output, int input_size, int interpolation, float *taps, int taps_length);   /* libcsdr.h:105 */
typedef struct rational_resampler_ff_s { int input_processed; int output_size; int last_taps_delay; } rational_resampler_ff_t;   /* libcsdr.h:132-137 */
rational_resampler_ff_t rational_resampler_ff(float *input, float *output, int input_size, int interpolation, int decimation, float *taps, int taps_length, int last_taps_delay);
/* BPSK31 receive, libcsdr.h:314-336 and libcsdr.c:1536-1549, 1977-2075, 2201-2217, 2319-2333.  debug_every_nth >= 0 (the Octave plots) is not supported:
 * timing_recovery_cc aborts on it.  dbpsk_decoder_c_u8 keeps ONE process-wide last_input, like the reference's function-level static: concurrent callers
 * share it (calls are serialised).  psk31_varicode_decoder_push runs on the host (one bit per call).
 * timing_recovery_cc needs |loop_gain| * max_error <= 1 (a symbol then moves on by D/2 .. 3D/2 samples; beyond that the reference's loop can step
 * backwards and read before its buffer): outside it the call prints the reason and aborts, like debug_every_nth >= 0. */
typedef enum timing_recovery_algorithm_e { TIMING_RECOVERY_ALGORITHM_GARDNER, TIMING_RECOVERY_ALGORITHM_EARLYLATE } timing_recovery_algorithm_t;
#define TIMING_RECOVERY_ALGORITHM_DEFAULT TIMING_RECOVERY_ALGORITHM_GARDNER
typedef struct timing_recovery_state_s {
    timing_recovery_algorithm_t algorithm;
    int decimation_rate;
    int output_size;
    int input_processed;
    int use_q;
    int debug_phase;
    int debug_every_nth;
    char *debug_writefiles_path;
    int last_correction_offset;
    float earlylate_ratio;
    float loop_gain;
    float max_error;
} timing_recovery_state_t;
timing_recovery_state_t timing_recovery_init(timing_recovery_algorithm_t algorithm, int decimation_rate, int use_q, float loop_gain, float max_error, int debug_every_nth, char *debug_writefiles_path);
void timing_recovery_cc(complexf *input, complexf *output, int input_size, float *timing_error, int *sampled_indexes, timing_recovery_state_t *state);
timing_recovery_algorithm_t timing_recovery_get_algorithm_from_string(char *input);
char *timing_recovery_get_string_from_algorithm(timing_recovery_algorithm_t algorithm);
void simple_agc_cc(complexf *input, complexf *output, int input_size, float rate, float reference, float max_gain, float *current_gain);
void dbpsk_decoder_c_u8(complexf *input, unsigned char *output, int input_size);
char psk31_varicode_decoder_push(unsigned long long *status_shr, unsigned char symbol);
/* BPSK31 transmit, libcsdr.h:343-347 and libcsdr.c:1551-1575, 1772-1808, 1828-1843, on the device (one library call = one block).
 * psk31_varicode_encoder_u8_u8 keeps the output_max_size contract: it stops in front of the first character whose code and two separators do not fit and
 * reports input_processed and output_size.  duplicate_samples_ntimes_u8_u8 writes the whole samples of input_size_bytes (the reference reads past its
 * input for a partial one).  psk31_interpolate_sine_cc returns the last input by value, to be passed to the next call. */
void psk_modulator_u8_c(unsigned char *input, complexf *output, int input_size, int n_psk);
void duplicate_samples_ntimes_u8_u8(unsigned char *input, unsigned char *output, int input_size_bytes, int sample_size_bytes, int ntimes);
complexf psk31_interpolate_sine_cc(complexf *input, complexf *output, int input_size, int interpolation, complexf last_input);
void psk31_varicode_encoder_u8_u8(unsigned char *input, unsigned char *output, int input_size, int output_max_size, int *input_processed, int *output_size);
unsigned char differential_codec(unsigned char *input, unsigned char *output, int input_size, int encode, unsigned char state);
/* The pulse-shaped symbol modem, libcsdr.h:393-411 and libcsdr.c:1731-1765, 1810-1827, 2276-2291, 2473-2516.  The designs and pack_bits_8to1_u8_u8 (eight
 * bytes) run on the host, the others on the device.  firdes_rrc_f writes only indexes below taps_length (the reference writes taps[taps_length] for an even
 * length); firdes_cosine_f writes 0 into the taps the reference leaves unwritten; both return 0.  generic_slicer_f_u8 writes 0 for an input that no symbol
 * claims (NaN: the reference leaves that byte unwritten) and does nothing for n_symbols outside 2..256. */
typedef enum matched_filter_type_e { MATCHED_FILTER_RRC, MATCHED_FILTER_COSINE } matched_filter_type_t;
#define MATCHED_FILTER_DEFAULT MATCHED_FILTER_RRC
int firdes_cosine_f(float *taps, int taps_length, int samples_per_symbol);
int firdes_rrc_f(float *taps, int taps_length, int samples_per_symbol, float beta);
matched_filter_type_t matched_filter_get_type_from_string(char *input);
int apply_real_fir_cc(complexf *input, complexf *output, int input_size, float *taps, int taps_length);
void generic_slicer_f_u8(float *input, unsigned char *output, int input_size, int n_symbols);
void plain_interpolate_cc(complexf *input, complexf *output, int input_size, int interpolation);
void pack_bits_1to8_u8_u8(unsigned char *input, unsigned char *output, int input_size);
unsigned char pack_bits_8to1_u8_u8(unsigned char *input);
/* RTTY receive, libcsdr.h:236-289, 412.  bfsk_demod_cf and serial_line_decoder_f_u8 run on the device (one library call = one window, as the reference);
 * serial_line_decoder_f_u8 writes unsigned char, short or unsigned outputs for databits <= 8, <= 16, above.  The Baudot functions run on the host. */
typedef struct rtty_baudot_item_s { unsigned long long code; unsigned char ascii_letter; unsigned char ascii_figure; } rtty_baudot_item_t;
typedef enum rtty_baudot_decoder_state_e { RTTY_BAUDOT_WAITING_STOP_PULSE = 0, RTTY_BAUDOT_WAITING_START_PULSE, RTTY_BAUDOT_RECEIVING_DATA } rtty_baudot_decoder_state_t;
typedef struct rtty_baudot_decoder_s {
    unsigned char fig_mode;
    unsigned char character_received;
    unsigned short shr;
    unsigned char bit_cntr;
    rtty_baudot_decoder_state_t state;
} rtty_baudot_decoder_t;
#define RTTY_FIGURE_MODE_SELECT_CODE 0b11011
#define RTTY_LETTER_MODE_SELECT_CODE 0b11111
char rtty_baudot_decoder_lookup(unsigned char *fig_mode, unsigned char c);
char rtty_baudot_decoder_push(rtty_baudot_decoder_t *s, unsigned char symbol);
typedef struct serial_line_s {
    float samples_per_bits;
    int databits; /* including parity */
    float stopbits;
    int output_size;
    int input_used;
    float bit_sampling_width_ratio;
} serial_line_t;
void serial_line_decoder_f_u8(serial_line_t *s, float *input, unsigned char *output, int input_size);
void binary_slicer_f_u8(float *input, unsigned char *output, int input_size);
int bfsk_demod_cf(complexf *input, float *output, int input_size, complexf *mark_filter, complexf *space_filter, int taps_length);
void firdes_add_peak_c(complexf *output, int length, float rate, window_t window, int add, int normalize);
int apply_fir_cc(complexf *input, complexf *output, int input_size, complexf *taps, int taps_length);      /* libcsdr.h:382: the complex-tap FIR, on the device */
void rational_resampler_get_lowpass_f(float *output, int output_size, int interpolation, int decimation, window_t window);

typedef struct shift_table_data_s { float *table; int table_size; } shift_table_data_t;     /* libcsdr.h:180-184 */
void shift_table_deinit(shift_table_data_t table_data);
shift_table_data_t shift_table_init(int table_size);
float shift_table_cc(complexf *input, complexf *output, int input_size, float rate, shift_table_data_t table_data, float starting_phase);

typedef struct shift_addfast_data_s { float dsin[4]; float dcos[4]; float phase_increment; } shift_addfast_data_t;  /* :189-194 */
shift_addfast_data_t shift_addfast_init(float rate);
float shift_addfast_cc(complexf *input, complexf *output, int input_size, shift_addfast_data_t *d, float starting_phase);

typedef struct shift_unroll_data_s { float *dsin; float *dcos; float phase_increment; int size; } shift_unroll_data_t; /* :199-205 */
float shift_unroll_cc(complexf *input, complexf *output, int input_size, shift_unroll_data_t *d, float starting_phase);
shift_unroll_data_t shift_unroll_init(float rate, int size);

int log2n(int x);
int next_pow2(int x);
void apply_fir_fft_cc(FFT_PLAN_T *plan, FFT_PLAN_T *plan_inverse, complexf *taps_fft, complexf *last_overlap, int overlap_size);
void gain_ff(float *input, float *output, int input_size, float gain);
/* libcsdr.h: the power behind squelch_and_smeter_cc and every S-meter (the sum over samples 0, decimation, .. divided by input_size), on the device */
float get_power_f(float *input, int input_size, int decimation);
float get_power_c(complexf *input, int input_size, int decimation);

/* carrier recovery, libcsdr.h:292-312, 364-378: the loop runs on the device, its state goes in and comes out through the caller's struct.
 * init_bpsk_costas_loop_cc does not store decision_directed and pll_cc_init_p_controller leaves iir_temp and pll_type alone, as in the reference;
 * pll_cc with any other pll_type advances the phase, writes output_nco[0] and returns. */
typedef enum pll_type_e { PLL_P_CONTROLLER = 1, PLL_PI_CONTROLLER = 2 } pll_type_t;
typedef struct pll_s { pll_type_t pll_type; float output_phase; float dphase; float frequency; float alpha; float beta; float iir_temp; } pll_t;
void pll_cc_init_pi_controller(pll_t *p, float bandwidth, float ko, float kd, float damping_factor);
void pll_cc_init_p_controller(pll_t *p, float alpha);
void pll_cc(pll_t *p, complexf *input, float *output_dphase, complexf *output_nco, int input_size);
typedef struct bpsk_costas_loop_state_s {
    float alpha; float beta; int decision_directed; float current_freq; float dphase; float nco_phase; float dphase_max; int dphase_max_reset_to_zero;
} bpsk_costas_loop_state_t;
void bpsk_costas_loop_cc(complexf *input, complexf *output, int input_size, float *output_error, float *output_dphase, complexf *output_nco, bpsk_costas_loop_state_t *s);
void init_bpsk_costas_loop_cc(bpsk_costas_loop_state_t *s, int decision_directed, float damping_factor, float bandwidth);

/* transmit-side modulators, libcsdr.h:216-218: fmmod_fc returns the phase to hand to the next call */
void add_dcoffset_cc(complexf *input, complexf *output, int input_size);
float fmmod_fc(float *input, complexf *output, int input_size, float last_phase);
void fixed_amplitude_cc(complexf *input, complexf *output, int input_size, float amp);

/* f2 blocks: libcsdr.h:97-99, 110-116, 142-147; libcsdr_gpl.h:37 */
float fmdemod_atan_cf(complexf *input, float *output, int input_size, float last_phase);
void amdemod_cf(complexf *input, float *output, int input_size);
void amdemod_estimator_cf(complexf *input, float *output, int input_size, float alpha, float beta);
typedef struct dcblock_preserve_s { float last_input; float last_output; } dcblock_preserve_t;             /* libcsdr.h:110-114 */
dcblock_preserve_t dcblock_ff(float *input, float *output, int input_size, float a, dcblock_preserve_t preserved);
float fastdcblock_ff(float *input, float *output, int input_size, float last_dc_level);
float *precalculate_window(int size, window_t window);
void apply_window_c(complexf *input, complexf *output, int size, window_t window);
void apply_precalculated_window_c(complexf *input, complexf *output, int size, float *windowt);
void logpower_cf(complexf *input, float *output, int size, float add_db);
void accumulate_power_cf(complexf *input, float *output, int size);
void log_ff(float *input, float *output, int size, float add_db);
float agc_ff(float *input, float *output, int input_size, float reference, float attack_rate, float decay_rate, float max_gain,
             short hang_time, short attack_wait_time, float gain_filter_alpha, float last_gain);

/* IMA ADPCM, ima_adpcm.h:5-11 */
typedef struct ImaState { int index; int previousValue; } ima_adpcm_state_t;
ima_adpcm_state_t encode_ima_adpcm_i16_u8(short *input, unsigned char *output, int input_length, ima_adpcm_state_t state);
ima_adpcm_state_t decode_ima_adpcm_u8_i16(unsigned char *input, short *output, int input_length, ima_adpcm_state_t state);

/* converters, libcsdr.h:220-229 */
void convert_u8_f(unsigned char *input, float *output, int input_size);
void convert_f_u8(float *input, unsigned char *output, int input_size);
void convert_s8_f(signed char *input, float *output, int input_size);
void convert_f_s8(float *input, signed char *output, int input_size);
void convert_f_s16(float *input, short *output, int input_size);
void convert_s16_f(short *input, float *output, int input_size);
void convert_f_i16(float *input, short *output, int input_size);
void convert_i16_f(short *input, float *output, int input_size);
void convert_f_s24(float *input, unsigned char *output, int input_size, int bigendian);
void convert_s24_f(unsigned char *input, float *output, int input_size, int bigendian);

/* libcsdr_gpl.h:26-46 */
typedef struct shift_addition_data_s { float sindelta; float cosdelta; float rate; } shift_addition_data_t;
shift_addition_data_t shift_addition_init(float rate);
float shift_addition_cc(complexf *input, complexf *output, int input_size, shift_addition_data_t d, float starting_phase);
float shift_addition_fc(float *input, complexf *output, int input_size, shift_addition_data_t d, float starting_phase);
typedef struct decimating_shift_addition_status_s { int decimation_remain; float starting_phase; int output_size; } decimating_shift_addition_status_t;
decimating_shift_addition_status_t decimating_shift_addition_cc(complexf *input, complexf *output, int input_size, shift_addition_data_t d, int decimation, decimating_shift_addition_status_t s);
shift_addition_data_t decimating_shift_addition_init(float rate, int decimation);

/* fastddc.h:5-29 */
typedef struct fastddc_s {
    int pre_decimation; int post_decimation; int taps_length; int taps_min_length; int overlap_length;
    int fft_size; int fft_inv_size; int input_size; int post_input_size;
    float pre_shift; int startbin; int v; int offsetbin; float post_shift; int output_scrape; int scrap;
    shift_addition_data_t dsadata;
} fastddc_t;
int fastddc_init(fastddc_t *ddc, float transition_bw, int decimation, float shift_rate);
decimating_shift_addition_status_t fastddc_inv_cc(complexf *input, complexf *output, fastddc_t *ddc, FFT_PLAN_T *plan_inverse, complexf *taps_fft, decimating_shift_addition_status_t shift_stat);
void fastddc_print(fastddc_t *ddc, char *source);
void fft_swap_sides(complexf *io, int fft_size);

/* noise sources and link measurements, libcsdr.h:385-391, all on the host.  The random samples are functions of the 32-bit words read from `status`:
 * any file of recorded words in place of /dev/urandom reproduces the reference (the Gaussian ones within the float32 gate of DESIGN.md 4s).
 * add_ff returns output (the reference's has no return statement). */
FILE *init_get_random_samples_f(void);
void get_random_samples_f(float *output, int output_size, FILE *status);
void get_random_gaussian_samples_c(complexf *output, int output_size, FILE *status);
int deinit_get_random_samples_f(FILE *status);
float *add_ff(float *input1, float *input2, float *output, int input_size);
float total_logpower_cf(complexf *input, int input_size);
float normalized_timing_variance_u32_f(unsigned *input, float *temp, int input_size, int samples_per_symbol, int initial_sample_offset, int debug_print);

#ifdef __cplusplus
}
#endif
#endif
