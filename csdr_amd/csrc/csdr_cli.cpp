// csdr_cli.cpp -- `csdr <function> <args>` for the hot-path commands, served by libcsdr_amd.so (SURVEY.md section 8b "CLI", f1).
//
// Same argv grammar, same raw native-endian sample streams on stdin/stdout as the reference CLI (csdr.c:56-181 usage string;
// per-command loops cited below), so a shell pipeline keeps working when `csdr` is replaced by this binary.  What differs, on purpose:
//   * each process moves whatever has arrived -- at least the reference's the_bufsize (1024 / 16384 samples, csdr.c:189-193, 332), at most
//     CSDR_AMD_BLOCK elements (default 4194304; 65536 when a control channel is open) -- through the GPU per iteration: a live stream sees the
//     reference's latency, a file or a fast producer large blocks (CSDR_AMD_MIN_READ overrides the minimum); the sample VALUES follow the reference's block semantics
//     exactly where they are observable (shift_* re-seed every 1024 samples like csdr.c:785,836,911-918; fastagc_ff works on its own
//     block size; decimating_shift_addition_cc restarts its recurrence every the_bufsize samples) and the stream models verified against
//     the reference (fir_decimate_cc refeed, fractional_decimator_ff refeed, overlap-add, fastddc);
//   * EOF is clean: every complete input sample is processed once; the reference's stale extra block at EOF is not emitted.
// Wire protocol either side of every command (csdr.c:325-419): CSDR_FIXED_BUFSIZE and CSDR_PRINT_BUFSIZES are honoured,
// CSDR_DYNAMIC_BUFSIZE_ON=1 makes every command consume the 8-byte "csdr"+int preamble from stdin and send its own (with the per-command
// size rule of the reference: /decimation, /rate, fft_size, ...) before its data; `setbuf N` starts such a chain.
// Live retune (csdr.c:252-323): `--fifo <path>` / `--fd <n>` in place of the rate arguments of shift_addition_cc, bandpass_fir_fft_cc and
// fastddc_inv_cc; the newest complete line is applied between two blocks.
// Fusion (the part of f1 that a process-per-command shell pipeline cannot give): `csdr chain "<cmd> <args> | <cmd> <args> | ..."` runs
// the listed hot-path commands in ONE process with every intermediate stream resident in HBM (PCIe carries only the first input and the
// last output), and replaces the README.md:66 WFM pattern by the fused matrix-core kernel.
// Device hand-off between ADJACENT csdr processes of an unchanged shell pipeline (`csdr a | csdr b`): see "device hand-off" in cli_run.hpp -- the samples stay in
// HBM, the pipe between the two processes carries nothing but the preamble.  Negotiated out of band, so a peer that is not this binary sees plain bytes.
// There is no CPU fallback: without a gfx950 device the process exits with status 3 and the reason on stderr.
#include "../../include/csdr_amd.h"
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <errno.h>
#include <fcntl.h>
#include <signal.h>
#include <stdarg.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <poll.h>
#include <pthread.h>
#include <sys/socket.h>
#include <sys/stat.h>
#include <sys/un.h>
#include <time.h>
#include <algorithm>
#include <string>
#include <vector>
#include <atomic>
#include <functional>
#include <memory>

namespace {

#include "cli_io.hpp"         // messages, descriptor and buffer helpers, wire protocol, control channel
#include "cli_stages.hpp"     // the streaming operators and make_stage()
#include "cli_run.hpp"        // device hand-off, I/O threads, the streaming loop run()
#include "cli_banks.hpp"      // fastddc_bank_cc, fastddc_nfm_bank_s16, fastddc_wfm_bank_s16, shift_bank_cc, wfm/nfm/am/ssb_bank_u8_s16, waterfall_bank_u8

// shift_addition_cc <rate> | shift_addition_cc --fifo <path> | shift_addition_cc --fd <n>: the tokens that stand for the rate (kept as they are in the fused command)
bool shift_rate_args(const std::vector<std::string> &cmd, std::vector<std::string> *rate_args)
{
    if (cmd.size() < 3 || cmd[1] != "shift_addition_cc") return false;
    if (cmd.size() == 4 && (cmd[2] == "--fifo" || cmd[2] == "--fd")) { rate_args->assign(cmd.begin() + 2, cmd.end()); return true; }
    float r;
    if (cmd.size() == 3 && sscanf(cmd[2].c_str(), "%g", &r) == 1) { char sh[64]; snprintf(sh, sizeof sh, "%.9g", r); rate_args->assign(1, sh); return true; }
    return false;
}

// one command of a chain against the words it must consist of ("*": any word)
bool is(const std::vector<std::string> &cmd, std::initializer_list<const char *> want)
{
    if (cmd.size() != want.size() + 1) return false;
    size_t j = 1; for (const char *w : want) { if (w[0] != '*' && cmd[j] != w) return false; j++; }
    return true;
}

bool is_wfm_pattern(const std::vector<std::vector<std::string>> &cmds, std::vector<std::string> *rate_args)
{   // README.md:66 exactly: the shape the fused matrix-core kernel implements
    if (cmds.size() != 7) return false;
    if (!is(cmds[0], {"convert_u8_f"}) || !is(cmds[2], {"fir_decimate_cc", "10", "0.05", "HAMMING"}) || !is(cmds[3], {"fmdemod_quadri_cf"}) ||
        !is(cmds[4], {"fractional_decimator_ff", "5"}) || !is(cmds[5], {"deemphasis_wfm_ff", "48000", "50e-6"}) || !is(cmds[6], {"convert_f_s16"})) return false;
    return shift_rate_args(cmds[1], rate_args);
}

bool is_nfm_pattern(const std::vector<std::vector<std::string>> &cmds, std::vector<std::string> *rate_args)
{   // README.md:87 exactly: the shape csdr_amd_nfm implements
    if (cmds.size() != 8) return false;
    if (!is(cmds[0], {"convert_u8_f"}) || !is(cmds[2], {"fir_decimate_cc", "50", "0.005", "HAMMING"}) || !is(cmds[3], {"fmdemod_quadri_cf"}) ||
        !is(cmds[4], {"limit_ff"}) || !is(cmds[5], {"deemphasis_nfm_ff", "48000"}) || !is(cmds[6], {"fastagc_ff"}) || !is(cmds[7], {"convert_f_s16"})) return false;
    return shift_rate_args(cmds[1], rate_args);
}

// [convert_u8_f |] fft_cc N E [window] | logaveragepower_cf A N AVG | fft_exchange_sides_ff N [| compress_fft_adpcm_f_u8 N], one N throughout -> waterfall_u8 / waterfall_cc
bool is_waterfall_pattern(const std::vector<std::vector<std::string>> &cmds, std::vector<std::string> *fused)
{
    size_t k = 0;
    const bool u8 = !cmds.empty() && cmds[0].size() == 2 && cmds[0][1] == "convert_u8_f";
    if (u8) k = 1;
    if (cmds.size() < k + 3 || cmds.size() > k + 4) return false;
    const auto &f = cmds[k], &l = cmds[k + 1], &x = cmds[k + 2];
    if (f.size() < 4 || f.size() > 5 || f[1] != "fft_cc" || l.size() != 5 || l[1] != "logaveragepower_cf" || x.size() != 3 || x[1] != "fft_exchange_sides_ff") return false;
    const std::string &N = f[2];
    if (l[3] != N || x[2] != N) return false;
    bool adpcm = false;
    if (cmds.size() == k + 4) {
        const auto &a = cmds[k + 3];
        if (a.size() != 3 || a[1] != "compress_fft_adpcm_f_u8" || a[2] != N) return false;
        adpcm = true;
    }
    int n = 0, e = 0, avg = 0; float db = 0;
    if (sscanf(N.c_str(), "%d", &n) != 1 || csdr_amd_log2n(n) < 1 || sscanf(f[3].c_str(), "%d", &e) != 1 || e <= 0 ||
        sscanf(l[2].c_str(), "%g", &db) != 1 || sscanf(l[4].c_str(), "%d", &avg) != 1 || avg <= 0) return false;
    *fused = {"csdr", u8 ? "waterfall_u8" : "waterfall_cc", N, f[3], f.size() == 5 ? f[4] : "HAMMING", l[2], l[4], adpcm ? "adpcm" : "db"};
    return true;
}

// a consecutive run (two or more) of the commands names[0 .. n-1], in this order and starting at any of them, becomes ONE command `fused_command` whose arguments are the
// run's commands, one per argument ("<cmd> <args>"); make_stage() builds one object that walks them in one launch.  `message`: what the chain says about it (two %s: the
// run's first and last command)
bool fuse_run(std::vector<std::vector<std::string>> &cmds, const char *const *names, int n, const char *fused_command, const char *message)
{
    auto stage_of = [&](const std::vector<std::string> &c) { for (int k = 0; k < n; k++) if (c.size() > 1 && c[1] == names[k]) return k; return -1; };
    bool any = false;
    for (size_t a = 0; a < cmds.size(); a++) {
        int s = stage_of(cmds[a]);
        if (s < 0) continue;
        size_t b = a + 1;
        while (b < cmds.size() && stage_of(cmds[b]) == s + (int)(b - a)) b++;
        if (b - a < 2) continue;
        std::vector<std::string> fused = {"csdr", fused_command};
        for (size_t k = a; k < b; k++) { std::string w; for (size_t t = 1; t < cmds[k].size(); t++) w += (t > 1 ? " " : "") + cmds[k][t]; fused.push_back(w); }
        fprintf(stderr, message, names[s], names[s + (int)(b - a) - 1]);
        cmds.erase(cmds.begin() + a, cmds.begin() + b);
        cmds.insert(cmds.begin() + a, fused);
        any = true;
    }
    return any;
}
// simple_agc_cc -> timing_recovery_cc -> dbpsk_decoder_c_u8 -> psk31_varicode_decoder_u8_u8 -> `psk31_rx`;  bfsk_demod_cf -> serial_line_decoder_f_u8 ->
// rtty_baudot2ascii_u8_u8 -> `rtty_rx`;  psk31_varicode_encoder_u8_u8 -> differential_encoder_u8_u8 -> psk_modulator_u8_c -> psk31_interpolate_sine_cc -> `psk31_tx`
const char *const PSK31_RUN[4] = {"simple_agc_cc", "timing_recovery_cc", "dbpsk_decoder_c_u8", "psk31_varicode_decoder_u8_u8"};
const char *const RTTY_RUN[3] = {"bfsk_demod_cf", "serial_line_decoder_f_u8", "rtty_baudot2ascii_u8_u8"};
const char *const PSK31TX_RUN[4] = {"psk31_varicode_encoder_u8_u8", "differential_encoder_u8_u8", "psk_modulator_u8_c", "psk31_interpolate_sine_cc"};

// [psk_modulator_u8_c n |] plain_interpolate_cc I | pulse_shaping_filter_cc ... -> one `pulse_tx` command (arguments: the run's commands, one per argument)
bool fuse_pulsetx(std::vector<std::vector<std::string>> &cmds)
{
    auto is = [&](size_t k, const char *name) { return k < cmds.size() && cmds[k].size() > 1 && cmds[k][1] == name; };
    bool any = false;
    for (size_t m = 0; m + 1 < cmds.size(); m++) {
        if (!is(m, "plain_interpolate_cc") || !is(m + 1, "pulse_shaping_filter_cc")) continue;
        const size_t a = m > 0 && is(m - 1, "psk_modulator_u8_c") ? m - 1 : m, b = m + 2;
        std::vector<std::string> fused = {"csdr", "pulse_tx"};
        for (size_t k = a; k < b; k++) { std::string w; for (size_t t = 1; t < cmds[k].size(); t++) w += (t > 1 ? " " : "") + cmds[k][t]; fused.push_back(w); }
        fprintf(stderr, "csdr chain: %s .. %s recognised -> one fused pulse-shaping transmit object (pulse_tx: k_pulsetx_poly)\n", cmds[a][1].c_str(), cmds[b - 1][1].c_str());
        cmds.erase(cmds.begin() + a, cmds.begin() + b);
        cmds.insert(cmds.begin() + a, fused);
        m = a; any = true;
    }
    return any;
}

// pulse_shaping_filter_cc ... | timing_recovery_cc ... [[| realpart_cf] | gain_ff g | generic_slicer_f_u8 n] -> one `pulse_rx` command (arguments: the run's commands, one
// per argument).  A timing_recovery_cc with an option behind --add_q (--output_error, --output_indexes, the Octave plots) writes something else: the run stays as it is.
bool fuse_pulserx(std::vector<std::vector<std::string>> &cmds)
{
    auto is = [&](size_t k, const char *name) { return k < cmds.size() && cmds[k].size() > 1 && cmds[k][1] == name; };
    bool any = false;
    for (size_t a = 0; a + 1 < cmds.size(); a++) {
        if (!is(a, "pulse_shaping_filter_cc") || !is(a + 1, "timing_recovery_cc")) continue;
        const std::vector<std::string> &t = cmds[a + 1];                // csdr timing_recovery_cc <algorithm> <decimation> [loop_gain [max_error [--add_q [option]]]]
        const size_t plain = 6 + (t.size() > 6 && t[6] == "--add_q");
        if (t.size() > plain) continue;
        size_t b = a + 2;
        if (is(b, "realpart_cf") && is(b + 1, "gain_ff") && is(b + 2, "generic_slicer_f_u8")) b += 3;
        else if (is(b, "gain_ff") && is(b + 1, "generic_slicer_f_u8")) b += 2;
        std::vector<std::string> fused = {"csdr", "pulse_rx"};
        for (size_t k = a; k < b; k++) { std::string w; for (size_t u = 1; u < cmds[k].size(); u++) w += (u > 1 ? " " : "") + cmds[k][u]; fused.push_back(w); }
        fprintf(stderr, "csdr chain: %s .. %s recognised -> one fused pulse-shaped receive object (pulse_rx)\n", cmds[a][1].c_str(), cmds[b - 1][1].c_str());
        cmds.erase(cmds.begin() + a, cmds.begin() + b);
        cmds.insert(cmds.begin() + a, fused);
        any = true;
    }
    return any;
}

// convert_u8_f | shift_addition_cc r | fir_decimate_cc D [tbw [window]] at the head of a chain -> one ddc_u8_cc command
bool fuse_front_end(std::vector<std::vector<std::string>> &cmds)
{
    if (cmds.size() < 3 || cmds[0].size() != 2 || cmds[0][1] != "convert_u8_f") return false;
    std::vector<std::string> rate_args;
    if (!shift_rate_args(cmds[1], &rate_args)) return false;
    if (cmds[2].size() < 3 || cmds[2].size() > 5 || cmds[2][1] != "fir_decimate_cc") return false;
    int d;
    if (sscanf(cmds[2][2].c_str(), "%d", &d) != 1 || d < 1) return false;
    std::vector<std::string> fused = {"csdr", "ddc_u8_cc"};
    fused.insert(fused.end(), rate_args.begin(), rate_args.end());
    fused.push_back(cmds[2][2]);
    for (size_t k = 3; k < cmds[2].size(); k++) fused.push_back(cmds[2][k]);
    cmds.erase(cmds.begin(), cmds.begin() + 3);
    cmds.insert(cmds.begin(), fused);
    return true;
}

} // namespace

int main(int argc, char **argv)
{
    parse_env();
    if (argc <= 1 || !strcmp(argv[1], "--help")) {
        fprintf(stderr, "csdr (MI355X back end): convert_u8_f convert_f_u8 convert_s8_f convert_f_s8 convert_f_s16 convert_s16_f convert_f_i16 convert_i16_f "
                        "convert_f_s24 convert_s24_f shift_math_cc shift_addition_cc shift_addition_fc shift_table_cc shift_addfast_cc shift_unroll_cc "
                        "decimating_shift_addition_cc fir_decimate_cc fmdemod_quadri_cf fmdemod_quadri_novect_cf fractional_decimator_ff rational_resampler_ff suboptimal_rational_resampler_ff fir_interpolate_cc deemphasis_wfm_ff "
                        "deemphasis_nfm_ff limit_ff fastagc_ff bandpass_fir_fft_cc fastddc_fwd_cc fastddc_inv_cc firdes_lowpass_f firdes_bandpass_c "
                        "simple_agc_cc timing_recovery_cc (needs |mu| * max_error <= 1) dbpsk_decoder_c_u8 psk31_varicode_decoder_u8_u8 "
                        "psk31_varicode_encoder_u8_u8 differential_encoder_u8_u8 differential_decoder_u8_u8 psk_modulator_u8_c (<n_psk>) psk31_interpolate_sine_cc (<interpolation>) "
                        "duplicate_samples_ntimes_u8_u8 (<sample_size_bytes> <ntimes>) "
                        "plain_interpolate_cc (<interpolation>) pulse_shaping_filter_cc / firdes_pulse_shaping_filter_f (RRC <samples_per_symbol> <num_taps> <beta> | COSINE <samples_per_symbol>) "
                        "generic_slicer_f_u8 (<n_symbols>) pack_bits_1to8_u8_u8 pack_bits_8to1_u8_u8 pattern_search_u8_u8 ([--mismatch <m>] <values_after> <pattern_values x N>) "
                        "bfsk_demod_cf serial_line_decoder_f_u8 rtty_baudot2ascii_u8_u8 rtty_line_decoder_u8_u8 binary_slicer_f_u8 firdes_peak_c peaks_fir_cc (<taps_length> <peak_rate> [<peak_rate> ...]) "
                        "squelch_and_smeter_cc (--fifo <ctl> --outfifo <path> <use_every_nth> <report_every_nth>) bpsk_costas_loop_cc (<loop_bandwidth> <damping_factor> [--dd | --decision_directed] [--output_error | --output_dphase | --output_nco | --output_combined <error_file> <dphase_file> <nco_file>]) pll_cc (1 [alpha] | 2 [bandwidth [damping_factor [ko [kd]]]]) amdemod_cf amdemod_estimator_cf fmdemod_atan_cf dcblock_ff fastdcblock_ff agc_ff gain_ff realpart_cf logpower_cf dsb_fc ([q_value]) fmmod_fc add_dcoffset_cc fixed_amplitude_cc (<new_amplitude>) convert_f_samplerf (<wait_for_this_sample>) fft_cc fft_fc (<fft_out_size> <out_of_every_n_samples> [window]) fft_one_side_ff logaveragepower_cf fft_exchange_sides_ff encode_ima_adpcm_i16_u8 decode_ima_adpcm_u8_i16 compress_fft_adpcm_f_u8 "
                        "awgn_cc (<snr_db> [--awgnfile <file>] [--snrshow] [--seed <seed>]) uniform_noise_f ([--seed <seed>]) gaussian_noise_c ([--seed <seed>]) normalized_timing_variance_u32_f (<samples_per_symbol> <initial_sample_offset>) "
                        "setbuf clone through | extensions: wfm_chain_u8_s16 <shift_rate>, nfm_chain_u8_s16 <shift_rate> [decimation [transition_bw]], ddc_u8_cc <shift_rate> <decimation> [transition_bw [window]], fastddc_bank_cc <decimation> <tbw> <window> <ctl|-> <out_0> <rate_0> ..., fastddc_nfm_bank_s16 [--squelch <block> <use_every_nth> <report_every_nth> <smeter_out>] <decimation> <tbw> <window> <audio_rate> <ctl|-> <out_0> <rate_0> ... (the bank with an NFM demodulator per channel: s16 audio; --squelch: squelch_and_smeter_cc in front of each, control line \"<channel> squelch <level>\", report lines \"<channel> <power>\"), nfm_rx_cc_s16 [audio_rate] [--squelch --fifo <ctl> --outfifo <path> <use_every_nth> <report_every_nth>] (fmdemod_quadri_cf | limit_ff | deemphasis_nfm_ff | fastagc_ff | convert_f_s16 on one complexf stream; --squelch: squelch_and_smeter_cc in front, its arguments), fastddc_wfm_bank_s16 [--squelch <block> <use_every_nth> <report_every_nth> <smeter_out>] <decimation> <tbw> <window> <frac_rate> <audio_rate> <tau> <ctl|-> <out_0> <rate_0> ... (the bank with a WFM demodulator per channel: s16 audio), wfm_rx_cc_s16 <rate> [audio_rate [tau [num_poly_points [--prefilter [transition_bw [window]]]]]] [--squelch --fifo <ctl> --outfifo <path> <use_every_nth> <report_every_nth>] (fmdemod_quadri_cf | fractional_decimator_ff | deemphasis_wfm_ff | convert_f_s16 on one complexf stream), shift_bank_cc <addition|math|table[:size]> <ctl|-> <out_0> <rate_0> ..., wfm_bank_u8_s16 / nfm_bank_u8_s16 / am_bank_u8_s16 <shift_rate> <in_0> <out_0> [<in_k> <out_k> ...], ssb_bank_u8_s16 [--lsb | --passbands lo:hi[,lo:hi,...]] <shift_rate> <in_0> <out_0> [<in_k> <out_k> ...], "
                        "waterfall_u8 / waterfall_cc <fft_size> <every_n> <window> <add_db> <avgnumber> <db|adpcm>, "
                        "waterfall_ff / waterfall_s16 <fft_out_size> <every_n> <window> <add_db> <avgnumber> <db|adpcm> (real input, one-sided rows), "
                        "waterfall_bank_u8 <fft_size> <every_n> <window> <add_db> <avgnumber> <db|adpcm> <in_0> <out_0> [<in_k> <out_k> ...], chain \"<cmd> <args> | <cmd> <args> ...\"\n");
        return -1;
    }
    g_cmd = argv[1];
    const std::string cmd = argv[1];
    if (cmd == "setbuf") {   // csdr.c:429-438
        if (argc <= 2) return badsyntax("need required parameter (buffer size)");
        int b = 0; sscanf(argv[2], "%d", &b);
        if (b <= 0) return badsyntax("buffer size <= 0 is invalid");
        return passthrough(false, b);
    }
    if (cmd == "clone" || cmd == "REM" || cmd == "through") return passthrough(true, 0);
    if (cmd == "firdes_peak_c") {                                     // csdr.c:2932-2972: print the designed taps, "(%g)+(%g)*i " each
        if (argc <= 3) return badsyntax("need required parameters (rate, length)");
        float rate = 0; int length = 0;
        sscanf(argv[2], "%g", &rate);
        sscanf(argv[3], "%d", &length);
        if (length % 2 == 0) return badsyntax("number of symmetric FIR filter taps should be odd");
        if (length < 1) return badsyntax("length should be at least 1");
        const int window = window_arg(argc, argv, 4, g_cmd);
        if (argc >= 6 && !strcmp(argv[5], "--octave")) return badsyntax("--octave (debug plot) is not supported");
        std::vector<csdr_complexf> t(length); csdr_amd_firdes_peak_c(t.data(), length, rate, window);
        for (int i = 0; i < length; i++) printf("(%g)+(%g)*i ", t[i].i, t[i].q);
        fflush(stdout);
        return 0;
    }
    if (cmd == "firdes_lowpass_f" || cmd == "firdes_bandpass_c") {   // csdr.c:1251-1335: print the designed taps ("%g " each), --octave wraps them in a plot script
        const bool bp = cmd == "firdes_bandpass_c";
        const int a0 = bp ? 5 : 4;                                    // argv index of the optional window
        if (argc < a0) return badsyntax(bp ? "need required parameters (low_cut, high_cut, length)" : "need required parameters (cutoff_rate, length)");
        float f1 = 0, f2 = 0; int length = 0;
        sscanf(argv[2], "%g", &f1);
        if (bp) sscanf(argv[3], "%g", &f2);
        sscanf(argv[a0 - 1], "%d", &length);
        if (length <= 0 || length % 2 == 0) return badsyntax("number of symmetric FIR filter taps should be odd");
        const int window = window_arg(argc, argv, a0, g_cmd);
        const bool octave = argc > a0 + 1 && !strcmp(argv[a0 + 1], "--octave");
        if (octave) printf("taps=[");
        if (bp) {
            std::vector<csdr_complexf> t(length); csdr_amd_firdes_bandpass_c(t.data(), length, f1, f2, window);
            for (int i = 0; i < length; i++) printf("(%g)+(%g)*i ", t[i].i, t[i].q);
            if (octave) printf("];spec=fftshift(abs(fft([taps,zeros(1,%d)])).^2);subplot(2,1,1);plot(spec);subplot(2,1,2);plot(arg(fft(taps)));\n", 4 * csdr_amd_next_pow2(length) - length);
        } else {
            std::vector<float> t(length); csdr_amd_firdes_lowpass_f(t.data(), length, f1, window);
            for (int i = 0; i < length; i++) printf("%g ", t[i]);
            if (octave) printf("];plot(taps);figure(2);freqz(taps);\n");
        }
        if (octave) { fflush(stdout); getchar(); }                   // keep octave's window open until the user closes the pipe
        return 0;
    }
    if (cmd == "firdes_pulse_shaping_filter_f") {                     // csdr.c:3159-3205: print the designed taps, "%f " each
        std::vector<float> t;
        if (!parse_pulse_filter(argc, argv, &t)) return -1;
        for (float v : t) printf("%f ", v);
        fflush(stdout);
        return 0;
    }
    if ((cmd == "rational_resampler_ff" || cmd == "suboptimal_rational_resampler_ff") && argc > 3) {   // csdr.c:1427: 1/1 copies input to output
        int I = 0, D = 0; sscanf(argv[2], "%d", &I); sscanf(argv[3], "%d", &D); if (I == 1 && D == 1) return passthrough(true, 0);
    }
    if (cmd == "fractional_decimator_ff" && argc > 2) { float r = 0; sscanf(argv[2], "%g", &r); if (r == 1) return passthrough(true, 0); }   // csdr.c:1494
    // device hand-off from the previous process of the shell pipeline (the streaming commands only): listen before anything slow -- the producer looks for this
    // socket when its first block is ready
    if (cmd != "fastddc_bank_cc" && cmd != "fastddc_nfm_bank_s16" && cmd != "fastddc_wfm_bank_s16" && cmd != "wfm_bank_u8_s16" && cmd != "nfm_bank_u8_s16" && cmd != "am_bank_u8_s16" && cmd != "ssb_bank_u8_s16" && cmd != "waterfall_bank_u8" && cmd != "shift_bank_cc" &&
        cmd != "uniform_noise_f" && cmd != "gaussian_noise_c") ipc_listen_on_stdin();
    const char *dev = getenv("CSDR_AMD_DEVICE");
    csdr_amd_ctx *c = csdr_amd_ctx_create(dev ? atoi(dev) : 0, nullptr);
    if (!c) { fprintf(stderr, "csdr %s: %s\n", g_cmd, csdr_amd_last_error()); return 3; }
    size_t block = block_elems();
    if (cmd == "uniform_noise_f" || cmd == "gaussian_noise_c") return run_noise_source(c, argc, argv, cmd[0] == 'g');
    if (cmd == "fastddc_bank_cc") return run_bank(c, argc, argv, block);
    if (cmd == "fastddc_nfm_bank_s16" || cmd == "fastddc_wfm_bank_s16") return run_fm_bank(c, argc, argv, block, cmd[8] == 'w');
    if (cmd == "wfm_bank_u8_s16" || cmd == "nfm_bank_u8_s16") return run_stream_bank(c, argc, argv, cmd[0] == 'n' ? BANK_NFM : BANK_WFM);
    if (cmd == "am_bank_u8_s16" || cmd == "ssb_bank_u8_s16") return run_stream_bank(c, argc, argv, cmd[0] == 'a' ? BANK_AM : BANK_SSB);
    if (cmd == "waterfall_bank_u8") return run_waterfall_bank(c, argc, argv);
    if (cmd == "shift_bank_cc") return run_shift_bank(c, argc, argv);
    std::vector<Stage *> stages; std::vector<size_t> caps;
    std::vector<std::vector<std::string>> cmds;
    if (cmd == "chain") {
        if (argc <= 2) return badsyntax("need the pipeline as one argument: \"<cmd> <args> | <cmd> <args> ...\"");
        cmds = split_chain(argv[2]);
        std::vector<std::string> rate_args;                            // the shift rate, or --fifo <path> / --fd <n> in its place: fusion AND retune
        if (is_wfm_pattern(cmds, &rate_args)) {
            fprintf(stderr, "csdr chain: WFM receive pattern recognised -> fused matrix-core kernel\n");
            std::vector<std::string> fused = {"csdr", "wfm_chain_u8_s16"}; fused.insert(fused.end(), rate_args.begin(), rate_args.end());
            cmds.assign(1, fused);
        } else if (is_nfm_pattern(cmds, &rate_args) && !g_dynamic && unitround(g_fixed) == 1024) {    // (the chain object models the pipeline at the default buffer size)
            fprintf(stderr, "csdr chain: NFM receive pattern recognised -> fused chain (matrix-core front end and de-emphasis)\n");
            std::vector<std::string> fused = {"csdr", "nfm_chain_u8_s16"}; fused.insert(fused.end(), rate_args.begin(), rate_args.end());
            cmds.assign(1, fused);
        } else if (std::vector<std::string> wf; !g_dynamic && is_waterfall_pattern(cmds, &wf)) {   // (the unfused pipeline's preambles are not modelled)
            fprintf(stderr, "csdr chain: waterfall pattern recognised -> %s (one-pass spectrum rows)\n", wf[1].c_str());
            cmds.assign(1, wf);
        } else if (fuse_front_end(cmds)) {
            fprintf(stderr, "csdr chain: convert_u8_f | shift_addition_cc | fir_decimate_cc recognised -> fused matrix-core front end\n");
        }
        fuse_run(cmds, PSK31_RUN, 4, "psk31_rx", "csdr chain: %s .. %s recognised -> one fused BPSK31 object (k_psk31)\n");
        fuse_pulsetx(cmds);                                             // (in front of the BPSK31 transmit run: psk_modulator_u8_c belongs to both)
        fuse_pulserx(cmds);                                             // (behind both: a filter that shapes a transmit run, or a timing loop a BPSK31 run took, is theirs)
        fuse_run(cmds, PSK31TX_RUN, 4, "psk31_tx", "csdr chain: %s .. %s recognised -> one fused BPSK31 transmit object (psk31_tx)\n");
        fuse_run(cmds, RTTY_RUN, 3, "rtty_rx", "csdr chain: %s .. %s recognised -> one fused RTTY object (rtty_rx: k_bfsk_mfma + k_rtty_walk)\n");
    } else {
        cmds.assign(1, std::vector<std::string>(argv, argv + argc));
    }
    if (g_dynamic) ipc_source_decide(dev ? atoi(dev) : 0);           // (before the preamble is read: a producer of ours connects first, then writes it)
    // (logaveragepower_cf reads no preamble: csdr.c:1663-1695 never calls getbufsize())
    const int in_bufsize = cmds[0].size() > 1 && cmds[0][1] == "logaveragepower_cf" ? unitround(g_dynamic ? 1024 : g_fixed)
                         : get_bufsize(cmds[0].size() > 1 && (cmds[0][1] == "shift_addition_cc" || cmds[0][1] == "decimating_shift_addition_cc" || cmds[0][1] == "shift_addition_fc" ||
                                                              cmds[0][1] == "serial_line_decoder_f_u8"));
    int out_bufsize = in_bufsize;
    // every command may have its control channel, also inside `chain` (fusion and retune together): the newest complete line is applied in front of a pass
    std::vector<Control> ctls(cmds.size());
    bool any_ctl = false;
    for (auto &cm : cmds) for (auto &t : cm) if (t == "--fifo" || t == "--fd") any_ctl = true;
    if (any_ctl && block > 65536 && !getenv("CSDR_AMD_BLOCK")) block = 65536;                               // retune latency
    size_t cap = block; bool cap_is_bytes = false;
    for (size_t k = 0; k < cmds.size(); k++) {
        std::vector<char *> av = argv_of(cmds[k]);
        if (av.size() < 2) return badsyntax("empty command in chain");
        // element size of the next command is only known once it is built; size its block for the worst case (1-byte elements) first
        Stage *s = make_stage(c, (int)av.size(), av.data(), cap, &ctls[k], out_bufsize);
        if (!s) return -1;
        if (ctls[k].fd) s->ctl = &ctls[k];
        if (cap_is_bytes) cap = cap / s->in_elem;
        if (cap < 4 * s->min_block) cap = 4 * s->min_block;
        if (cap < 2 * s->granule) cap = 2 * s->granule;
        if (k == 0 && s->max_block && cap > s->max_block) cap = std::max(s->max_block - s->max_block % s->granule, 2 * s->granule);
        if (k == 0) { cap -= cap % s->granule; block = cap; }
        stages.push_back(s); caps.push_back(cap + (k ? 64 : 0));
        out_bufsize = s->next_bufsize(out_bufsize);
        cap = s->out_capacity(caps.back()) * s->out_elem + 8 * (size_t)65536 * 8;    // BYTES the next stage may be handed: this stage's output plus its own carry
        cap_is_bytes = true;
    }
    g_cmd = argv[1];
    const int rc = run(c, stages, caps, in_bufsize, out_bufsize, dev ? atoi(dev) : 0);      // (sends the preamble: behind the hand-off offer to the next process)
    (void)csdr_amd_ctx_sync(c);
    return rc;
}
