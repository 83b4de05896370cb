"""csdr_amd -- Python harness over libcsdr_amd.so (the MI355X-native libcsdr hot path).

The product is the C-ABI shared library (include/csdr_amd.h, include/libcsdr_amd_compat.h) built from
csdr_amd/csrc/*.hip for gfx950.  This module only loads it with ctypes and offers numpy-in/numpy-out
conveniences for the tests and bench.py; it contains no DSP and NO fallback: if the library or the GPU is
missing, everything raises.
"""
import ctypes as C
import os
import sys
import subprocess
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CSDR_AMD_LIB") or os.path.join(HERE, "libcsdr_amd.so")     # override: A/B builds on one GPU box
ROOT = os.path.dirname(HERE)

c64 = np.complex64
f32 = np.float32

SHIFT = {"addition": 0, "math": 1, "table": 2, "unroll": 3, "addfast": 4}
WINDOWS = {"BOXCAR": 0, "BLACKMAN": 1, "HAMMING": 2}


class CsdrAmdError(RuntimeError):
    pass


def build(verbose=False):
    """Compile every HIP source for gfx950 into csdr_amd/libcsdr_amd.so (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", os.path.join(HERE, "csrc"), "-j8"], capture_output=True, text=True)
    if r.returncode != 0:
        raise CsdrAmdError("libcsdr_amd build failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    if verbose:
        print(r.stdout)
    return LIB_PATH


class FastDDC(C.Structure):       # csdr_fastddc_t == fastddc_t (fastddc.h:5-24)
    _fields_ = [(n, C.c_int) for n in ("pre_decimation", "post_decimation", "taps_length", "taps_min_length",
                                       "overlap_length", "fft_size", "fft_inv_size", "input_size", "post_input_size")] + \
               [("pre_shift", C.c_float), ("startbin", C.c_int), ("v", C.c_int), ("offsetbin", C.c_int),
                ("post_shift", C.c_float), ("output_scrape", C.c_int), ("scrap", C.c_int),
                ("sindelta", C.c_float), ("cosdelta", C.c_float), ("rate", C.c_float)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n not in ("sindelta", "cosdelta", "rate")}
        d["dsadata"] = (self.sindelta, self.cosdelta, self.rate)
        return d


_lib = None


def lib():
    """The loaded shared library (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CsdrAmdError("%s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` first" % LIB_PATH)
    # One HIP runtime per process: libcsdr_amd.so links the system libamdhip64, torch ships its own copy.  Loaded torch-first, the library
    # resolves to the copy torch brought (both share devices and streams); loaded the other way round, torch's runtime finds the devices taken
    # ("no ROCm-capable device").  So if torch is going to be used in this process at all, it has to come first.
    if "torch" not in sys.modules and not os.environ.get("CSDR_AMD_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(LIB_PATH)
    vp, sz, i, fl = C.c_void_p, C.c_size_t, C.c_int, C.c_float
    L.csdr_amd_ctx_create.restype = vp; L.csdr_amd_ctx_create.argtypes = [i, vp]
    L.csdr_amd_ctx_destroy.argtypes = [vp]
    L.csdr_amd_ctx_sync.argtypes = [vp]
    L.csdr_amd_ctx_stream.restype = vp; L.csdr_amd_ctx_stream.argtypes = [vp]
    L.csdr_amd_last_error.restype = C.c_char_p
    L.csdr_amd_device_arch.restype = C.c_char_p; L.csdr_amd_device_arch.argtypes = [vp]
    L.csdr_amd_malloc.restype = vp; L.csdr_amd_malloc.argtypes = [vp, sz]
    L.csdr_amd_free.argtypes = [vp, vp]
    L.csdr_amd_h2d.argtypes = [vp, vp, vp, sz]
    L.csdr_amd_d2h.argtypes = [vp, vp, vp, sz]
    L.csdr_amd_memset.argtypes = [vp, vp, i, sz]
    sh = C.c_short
    L.csdr_amd_d2d.argtypes = [vp, vp, vp, sz]
    L.csdr_amd_amdemod_cf.argtypes = [vp, vp, vp, sz]
    L.csdr_amd_amdemod_estimator_cf.argtypes = [vp, vp, vp, sz, fl, fl]
    L.csdr_amd_realpart_cf.argtypes = [vp, vp, vp, sz]
    L.csdr_amd_logpower_cf.argtypes = [vp, vp, vp, sz, fl]
    L.csdr_amd_fmdemod_atan_cf.argtypes = [vp, vp, vp, i, sz, sz, sz, vp]
    L.csdr_amd_dcblock_ff.argtypes = [vp, vp, vp, i, sz, sz, sz, fl, vp]
    L.csdr_amd_fastdcblock_ff.argtypes = [vp, vp, vp, i, i, i, sz, sz, vp]
    L.csdr_amd_agc_ff.argtypes = [vp, vp, vp, i, sz, i, sz, sz, fl, fl, fl, fl, sh, sh, fl, vp]
    L.csdr_amd_precalculate_window.argtypes = [vp, i, i]; L.csdr_amd_precalculate_window.restype = None
    L.csdr_amd_fftcc_create.restype = vp; L.csdr_amd_fftcc_create.argtypes = [vp, i, i, i, i]
    L.csdr_amd_fftcc_destroy.argtypes = [vp]; L.csdr_amd_fftcc_destroy.restype = None
    L.csdr_amd_fftcc_process.argtypes = [vp, vp, sz, vp, C.POINTER(sz)]
    L.csdr_amd_fftfc_create.restype = vp; L.csdr_amd_fftfc_create.argtypes = [vp, i, i, i, sz]
    L.csdr_amd_fftfc_destroy.argtypes = [vp]; L.csdr_amd_fftfc_destroy.restype = None
    L.csdr_amd_fftfc_process.argtypes = [vp, vp, sz, vp]
    L.csdr_amd_fft_one_side_ff.argtypes = [vp, vp, vp, i, i]
    L.csdr_amd_encode_ima_adpcm_i16_u8.argtypes = [vp, vp, vp, i, sz, sz, sz, vp]
    L.csdr_amd_decode_ima_adpcm_u8_i16.argtypes = [vp, vp, vp, i, sz, sz, sz, vp]
    L.csdr_amd_compress_fft_adpcm_f_u8.argtypes = [vp, vp, vp, i, i]
    L.csdr_amd_waterfall_create.restype = vp; L.csdr_amd_waterfall_create.argtypes = [vp, i, i, i, i, fl, i, i, i, sz]
    L.csdr_amd_waterfall_process.argtypes = [vp, vp, sz, sz, vp, sz, C.POINTER(i)]
    ll = C.c_longlong
    # csdr_amd_<pre>_<member>, the entry points the stateful objects share (what _Handle and its mixins below call; on the C side csrc/bank.hpp holds the
    # bodies): every object has `common`, the table lists which of the others
    members = {"reset": (i, [vp]), "force_generic": (i, [vp, i]), "kernel_name": (C.c_char_p, [vp]), "destroy": (None, [vp]), "max_out": (ll, [vp, ll]),
               "reset_channel": (i, [vp, i]), "get_channel": (i, [vp, i, vp]), "set_channel": (i, [vp, i, vp]), "set_lanes": (i, [vp, i]), "lanes": (i, [vp])}
    common, max_out, chan, lanes = ("reset", "force_generic", "kernel_name", "destroy"), ("max_out",), ("reset_channel", "get_channel", "set_channel"), ("set_lanes", "lanes")
    for pre, extra in (("waterfall", ()), ("resampler", max_out), ("interp", max_out), ("psk31", max_out + chan + lanes), ("psk31tx", max_out + chan),
                       ("pulsetx", max_out), ("pulserx", max_out + chan + lanes), ("rtty", max_out + chan[:1]), ("cfir", max_out + chan[:1]), ("squelch", chan[:1]), ("carrier", chan + lanes), ("shiftbank", chan), ("framesync", max_out + chan[:1] + lanes), ("amssb", max_out + chan + lanes),
                       ("txbank", max_out), ("fmrx", max_out + chan[:1]), ("wfmrx", max_out + chan[:1])):
        for m in common + extra:
            f = getattr(L, "csdr_amd_%s_%s" % (pre, m))
            f.restype, f.argtypes = members[m]
    L.csdr_amd_resampler_create.restype = vp; L.csdr_amd_resampler_create.argtypes = [vp, i, i, vp, i, i]
    L.csdr_amd_resampler_process.argtypes = [vp, vp, ll, sz, vp, sz, C.POINTER(ll)]
    L.csdr_amd_resampler_set_cli_bufsize.argtypes = [vp, i]
    L.csdr_amd_resampler_set_last_taps_delay.argtypes = [vp, i]
    L.csdr_amd_resampler_window.argtypes = [i, i, i, i, i, vp]
    L.csdr_amd_interp_create.restype = vp; L.csdr_amd_interp_create.argtypes = [vp, i, vp, i, i]
    L.csdr_amd_interp_process.argtypes = [vp, vp, ll, sz, vp, sz, C.POINTER(ll)]
    L.csdr_amd_interp_set_cli_bufsize.argtypes = [vp, i]
    L.csdr_amd_psk31_create.restype = vp; L.csdr_amd_psk31_create.argtypes = [vp, vp, i, i, i]
    L.csdr_amd_psk31_process.argtypes = [vp, vp, ll, sz, vp, sz, vp, vp, vp]
    L.csdr_amd_simple_agc_cc.argtypes = [vp, vp, vp, i, ll, sz, sz, C.c_float, C.c_float, C.c_float, vp]
    L.csdr_amd_psk31_varicode_decoder_push.restype = C.c_char; L.csdr_amd_psk31_varicode_decoder_push.argtypes = [vp, C.c_ubyte]
    L.csdr_amd_psk31_varicode_table.restype = None; L.csdr_amd_psk31_varicode_table.argtypes = [vp]
    L.csdr_amd_debug_psk31_walk.restype = ll; L.csdr_amd_debug_psk31_walk.argtypes = [vp, i, i, vp, ll, vp, i, vp, vp, vp, vp]
    L.csdr_amd_psk31tx_create.restype = vp; L.csdr_amd_psk31tx_create.argtypes = [vp, i, i, i, i, i]
    L.csdr_amd_psk31tx_process.argtypes = [vp, vp, ll, vp, sz, vp, sz, vp]
    L.csdr_amd_psk31tx_tables.argtypes = [i, i, vp, vp]
    L.csdr_amd_differential_decoder_u8_u8.argtypes = [vp, vp, vp, i, ll, sz, sz, vp]
    L.csdr_amd_duplicate_samples_ntimes_u8_u8.argtypes = [vp, vp, vp, i, ll, sz, sz, i, i]
    L.csdr_amd_debug_psk31tx_walk.restype = ll; L.csdr_amd_debug_psk31tx_walk.argtypes = [i, i, i, i, vp, ll, vp, i, vp, vp]
    L.csdr_amd_pulsetx_create.restype = vp; L.csdr_amd_pulsetx_create.argtypes = [vp, i, i, i, vp, i, i, i]
    L.csdr_amd_pulsetx_process.argtypes = [vp, vp, ll, sz, vp, sz, C.POINTER(ll)]
    L.csdr_amd_pulsetx_tile.argtypes = [vp]
    L.csdr_amd_debug_pulsetx_walk.restype = ll; L.csdr_amd_debug_pulsetx_walk.argtypes = [i, i, vp, i, i, i, vp, ll, vp, i, vp]
    L.csdr_amd_pulserx_create.restype = vp; L.csdr_amd_pulserx_create.argtypes = [vp, vp, i, i, i]
    L.csdr_amd_pulserx_process.argtypes = [vp, vp, ll, sz, vp, sz, vp, vp, vp]
    L.csdr_amd_debug_pulserx_walk.restype = ll; L.csdr_amd_debug_pulserx_walk.argtypes = [vp, i, i, vp, ll, vp, i, vp, vp, vp, vp]
    L.csdr_amd_framesync_create.argtypes = [vp, i, vp, i, i, i, vp]
    L.csdr_amd_framesync_process.argtypes = [vp, vp, sz, ll, vp, vp, sz, vp, vp, sz, vp]
    L.csdr_amd_framesync_max_frames.restype = ll; L.csdr_amd_framesync_max_frames.argtypes = [vp, ll]
    L.csdr_amd_framesync_tile.argtypes = []
    L.csdr_amd_framesync_get_channel.argtypes = [vp, i, vp, vp]
    L.csdr_amd_framesync_set_channel.argtypes = [vp, i, vp, vp]
    L.csdr_amd_pattern_search_u8_u8.argtypes = [vp, vp, ll, vp, i, i, vp, vp]
    L.csdr_amd_debug_framesync_walk.restype = ll; L.csdr_amd_debug_framesync_walk.argtypes = [vp, i, i, i, vp, ll, vp, i, vp, vp, vp, vp, vp]
    L.csdr_amd_generic_slicer_f_u8.argtypes = [vp, vp, vp, i, ll, sz, sz, i]
    L.csdr_amd_plain_interpolate_cc.argtypes = [vp, vp, vp, i, ll, sz, sz, i]
    L.csdr_amd_pack_bits_1to8_u8_u8.argtypes = [vp, vp, vp, i, ll, sz, sz]
    L.csdr_amd_pack_bits_8to1_u8_u8.argtypes = [vp, vp, vp, i, ll, sz, sz]
    L.csdr_amd_apply_real_fir_cc.argtypes = [vp, vp, vp, i, i, sz, sz, vp, i]
    L.csdr_amd_firdes_rrc_f.argtypes = [vp, i, i, fl]
    L.csdr_amd_firdes_cosine_f.argtypes = [vp, i, i]
    L.csdr_amd_rtty_create.restype = vp; L.csdr_amd_rtty_create.argtypes = [vp, vp, i, i, i]
    L.csdr_amd_rtty_process.argtypes = [vp, vp, ll, sz, vp, sz, vp]
    L.csdr_amd_bfsk_demod_cf.argtypes = [vp, vp, vp, i, ll, sz, sz, vp, vp, i, i]
    L.csdr_amd_bfsk_last_kernel.restype = C.c_char_p; L.csdr_amd_bfsk_last_kernel.argtypes = []
    L.csdr_amd_binary_slicer_f_u8.argtypes = [vp, vp, vp, i, ll, sz, sz]
    L.csdr_amd_rtty_line_decoder_u8_u8.argtypes = [vp, vp, vp, i, ll, sz, sz, vp, vp]
    L.csdr_amd_serial_line_decoder_f_u8.argtypes = [vp, vp, vp, i, i, sz, sz, C.c_float, i, C.c_float, C.c_float, vp, vp]
    L.csdr_amd_rtty_baudot_decoder_lookup.restype = C.c_char; L.csdr_amd_rtty_baudot_decoder_lookup.argtypes = [vp, C.c_ubyte]
    L.csdr_amd_rtty_baudot_decoder_push.restype = C.c_char; L.csdr_amd_rtty_baudot_decoder_push.argtypes = [vp, C.c_ubyte]
    L.csdr_amd_firdes_add_peak_c.restype = None; L.csdr_amd_firdes_add_peak_c.argtypes = [vp, i, C.c_float, i, i, i]
    L.csdr_amd_firdes_peak_c.restype = None; L.csdr_amd_firdes_peak_c.argtypes = [vp, i, C.c_float, i]
    L.csdr_amd_debug_rtty_walk.restype = ll; L.csdr_amd_debug_rtty_walk.argtypes = [vp, i, i, vp, ll, vp, i, vp]
    L.csdr_amd_cfir_create.restype = vp; L.csdr_amd_cfir_create.argtypes = [vp, i, i]
    L.csdr_amd_cfir_set_taps.argtypes = [vp, i, vp]
    L.csdr_amd_cfir_set_peaks.argtypes = [vp, i, vp, i, i]
    L.csdr_amd_cfir_process.argtypes = [vp, vp, ll, sz, vp, sz, vp]
    L.csdr_amd_apply_fir_cc.argtypes = [vp, vp, vp, i, ll, sz, sz, vp, sz, i, i]
    L.csdr_amd_apply_fir_last_kernel.restype = C.c_char_p; L.csdr_amd_apply_fir_last_kernel.argtypes = []
    L.csdr_amd_firdes_peaks_c.restype = None; L.csdr_amd_firdes_peaks_c.argtypes = [vp, i, vp, i, i]
    L.csdr_amd_debug_cfir_walk.restype = ll; L.csdr_amd_debug_cfir_walk.argtypes = [vp, i, vp, ll, vp, i, vp]
    ull = C.c_ulonglong
    L.csdr_amd_noise_create.restype = vp; L.csdr_amd_noise_create.argtypes = [vp, i, i, ull, vp]
    L.csdr_amd_noise_generate.argtypes = [vp, vp, ll, sz]
    L.csdr_amd_noise_awgn_cc.argtypes = [vp, vp, ll, sz, vp, sz, vp]
    L.csdr_amd_noise_set_snr_db.argtypes = [vp, i, fl]
    L.csdr_amd_noise_set_snrs.argtypes = [vp, vp]
    L.csdr_amd_noise_get_gains.argtypes = [vp, i, C.POINTER(fl), C.POINTER(fl)]
    L.csdr_amd_noise_position.restype = ll; L.csdr_amd_noise_position.argtypes = [vp, i]
    L.csdr_amd_noise_set_position.argtypes = [vp, i, ll]
    L.csdr_amd_noise_get_channel.argtypes = [vp, i, vp]
    L.csdr_amd_noise_reset.argtypes = [vp]
    L.csdr_amd_noise_reset_channel.argtypes = [vp, i]
    L.csdr_amd_noise_kernel_name.restype = C.c_char_p; L.csdr_amd_noise_kernel_name.argtypes = [vp]
    L.csdr_amd_noise_destroy.restype = None; L.csdr_amd_noise_destroy.argtypes = [vp]
    L.csdr_amd_awgn_gains.restype = None; L.csdr_amd_awgn_gains.argtypes = [fl, C.POINTER(fl), C.POINTER(fl)]
    L.csdr_amd_awgn_cc.argtypes = [vp, vp, vp, vp, i, ll, sz, sz, sz, vp, vp]
    L.csdr_amd_total_logpower_cf.argtypes = [vp, vp, i, ll, sz, vp]
    L.csdr_amd_normalized_timing_variance_u32_f.argtypes = [vp, vp, sz, i, vp, i, i, i, vp]
    L.csdr_amd_count_errors_u8.argtypes = [vp, vp, sz, ll, vp, sz, ll, i, vp, vp, vp]
    L.csdr_amd_debug_philox.restype = None; L.csdr_amd_debug_philox.argtypes = [vp, vp, vp]
    L.csdr_amd_debug_noise_words.argtypes = [i, vp, ll, vp]
    L.csdr_amd_debug_noise_walk.restype = ll; L.csdr_amd_debug_noise_walk.argtypes = [i, ull, C.c_uint, ll, ll, vp, i, vp, fl, vp]
    L.csdr_amd_debug_awgn_cc.argtypes = [vp, vp, ll, fl, vp]
    L.csdr_amd_debug_timing_variance.restype = fl; L.csdr_amd_debug_timing_variance.argtypes = [vp, i, i, i]
    L.csdr_amd_squelch_create.restype = vp; L.csdr_amd_squelch_create.argtypes = [vp, i, i, i, vp, ll]
    L.csdr_amd_squelch_process.argtypes = [vp, vp, ll, sz, vp, sz, vp, sz, vp, vp]
    L.csdr_amd_squelch_set_level.argtypes = [vp, i, fl]
    L.csdr_amd_squelch_get_level.restype = fl; L.csdr_amd_squelch_get_level.argtypes = [vp, i]
    L.csdr_amd_squelch_block_index.restype = ll; L.csdr_amd_squelch_block_index.argtypes = [vp, i]
    L.csdr_amd_squelch_max_blocks.argtypes = [vp]
    L.csdr_amd_get_power_c.argtypes = [vp, vp, i, i, i, i, sz, vp]
    L.csdr_amd_get_power_f.argtypes = [vp, vp, i, i, i, i, sz, vp]
    L.csdr_amd_squelch_report_due.argtypes = [i, ll]
    L.csdr_amd_squelch_gate_open.argtypes = [fl, fl]
    L.csdr_amd_debug_squelch_power.restype = fl; L.csdr_amd_debug_squelch_power.argtypes = [vp, i, i, i]
    L.csdr_amd_costas_params.argtypes = [fl, fl, i, vp]
    L.csdr_amd_pll_params_p.argtypes = [fl, vp]
    L.csdr_amd_pll_params_pi.argtypes = [fl, fl, fl, fl, vp]
    L.csdr_amd_carrier_create.restype = vp; L.csdr_amd_carrier_create.argtypes = [vp, vp, i]
    L.csdr_amd_carrier_process.argtypes = [vp, vp, ll, sz, vp, vp, vp, vp, sz]
    L.csdr_amd_debug_carrier_walk.restype = ll; L.csdr_amd_debug_carrier_walk.argtypes = [vp, vp, ll, vp, i, vp, vp, vp, vp, vp]
    L.csdr_amd_shiftbank_create.restype = vp; L.csdr_amd_shiftbank_create.argtypes = [vp, i, i, vp, i, i, i, sz]
    L.csdr_amd_shiftbank_process.argtypes = [vp, vp, sz, vp, sz, sz]
    L.csdr_amd_shiftbank_set_rate.argtypes = [vp, i, fl]
    L.csdr_amd_shiftbank_get_rate.argtypes = [vp, i, C.POINTER(fl)]
    L.csdr_amd_shiftbank_scans_ahead.restype = ll; L.csdr_amd_shiftbank_scans_ahead.argtypes = [vp]
    L.csdr_amd_debug_shiftbank_walk.restype = ll; L.csdr_amd_debug_shiftbank_walk.argtypes = [i, fl, i, i, i, vp, ll, vp, i, vp, vp, vp]
    L.csdr_amd_debug_shiftbank_chunk_phases.restype = None; L.csdr_amd_debug_shiftbank_chunk_phases.argtypes = [fl, fl, i, i, vp]
    L.csdr_amd_amssb_params_default.argtypes = [vp, i]
    L.csdr_amd_amssb_create_cf32.restype = vp; L.csdr_amd_amssb_create_cf32.argtypes = [vp, vp, i, vp, i, i, sz]
    L.csdr_amd_amssb_create.restype = vp; L.csdr_amd_amssb_create.argtypes = [vp, vp, i, fl, i, vp, i, vp, i, i, sz]
    L.csdr_amd_amssb_create_rates.restype = vp; L.csdr_amd_amssb_create_rates.argtypes = [vp, vp, i, vp, i, vp, i, vp, i, i, sz]
    L.csdr_amd_amssb_process.restype = ll; L.csdr_amd_amssb_process.argtypes = [vp, vp, sz, ll, vp, vp, sz]
    L.csdr_amd_amssb_set_rate.argtypes = [vp, i, fl]
    L.csdr_amd_amssb_get_rate.restype = fl; L.csdr_amd_amssb_get_rate.argtypes = [vp, i]
    L.csdr_amd_amssb_front_end.restype = vp; L.csdr_amd_amssb_front_end.argtypes = [vp]
    if hasattr(L, "csdr_amd_amssb_set_passband"):         # (absent from older builds selected with CSDR_AMD_LIB for A/B runs, like the per-stream filter below)
        L.csdr_amd_amssb_set_passband.argtypes = [vp, i, fl, fl, i]
        L.csdr_amd_amssb_set_channel_taps.argtypes = [vp, i, vp, i]
        L.csdr_amd_amssb_get_passband.argtypes = [vp, i, vp, vp]
    if hasattr(L, "csdr_amd_amssb_enable_squelch"):
        L.csdr_amd_amssb_enable_squelch.argtypes = [vp, i, vp]
        L.csdr_amd_amssb_process_squelched.restype = ll; L.csdr_amd_amssb_process_squelched.argtypes = [vp, vp, sz, ll, vp, vp, sz, vp, sz, vp, C.POINTER(i)]
        L.csdr_amd_amssb_set_squelch_level.argtypes = [vp, i, fl]
        L.csdr_amd_amssb_get_squelch_level.argtypes = [vp, i, C.POINTER(fl)]
        L.csdr_amd_amssb_squelch_block_index.restype = ll; L.csdr_amd_amssb_squelch_block_index.argtypes = [vp]
        L.csdr_amd_debug_amssb_zero_run.restype = fl; L.csdr_amd_debug_amssb_zero_run.argtypes = [vp, fl, ll, C.POINTER(ll)]
    L.csdr_amd_debug_amssb_walk.restype = ll; L.csdr_amd_debug_amssb_walk.argtypes = [vp, vp, i, vp, vp, vp]
    L.csdr_amd_fmmod_fc.argtypes = [vp, vp, vp, i, sz, sz, sz, vp]
    L.csdr_amd_dsb_fc.argtypes = [vp, vp, vp, sz, fl]
    L.csdr_amd_add_dcoffset_cc.argtypes = [vp, vp, vp, sz]
    L.csdr_amd_fixed_amplitude_cc.argtypes = [vp, vp, vp, sz, fl]
    L.csdr_amd_convert_f_samplerf.argtypes = [vp, vp, vp, sz, C.c_uint]
    L.csdr_amd_debug_fmmod_walk.restype = ll; L.csdr_amd_debug_fmmod_walk.argtypes = [vp, ll, vp, i, vp, vp, vp]
    L.csdr_amd_txbank_create.restype = vp; L.csdr_amd_txbank_create.argtypes = [vp, i, i, fl, fl, i, vp, i, vp, i, sz]
    L.csdr_amd_txbank_process.argtypes = [vp, vp, sz, ll, vp, sz, C.POINTER(ll)]
    L.csdr_amd_txbank_set_rate.argtypes = [vp, i, fl]
    L.csdr_amd_txbank_get_rate.restype = fl; L.csdr_amd_txbank_get_rate.argtypes = [vp, i]
    L.csdr_amd_rational_resampler_get_lowpass_f.restype = None; L.csdr_amd_rational_resampler_get_lowpass_f.argtypes = [vp, i, i, i, i]
    L.csdr_amd_debug_resampler_schedule.argtypes = [i, i, i, i, i, vp]
    L.csdr_amd_logaveragepower_cf.argtypes = [vp, vp, vp, i, i, i, fl]
    L.csdr_amd_fft_exchange_sides_ff.argtypes = [vp, vp, vp, i, i]
    L.csdr_amd_accumulate_power_cf.argtypes = [vp, vp, vp, sz]
    L.csdr_amd_log_ff.argtypes = [vp, vp, vp, sz, fl]
    L.csdr_amd_timer_start.argtypes = [vp]
    L.csdr_amd_timer_stop_ms.argtypes = [vp, C.POINTER(fl)]
    L.csdr_amd_firdes_filter_len.argtypes = [fl]
    L.csdr_amd_firdes_lowpass_f.argtypes = [vp, i, fl, i]
    L.csdr_amd_firdes_bandpass_c.argtypes = [vp, i, fl, fl, i]
    L.csdr_amd_nfm_deemph_taps.argtypes = [i, C.POINTER(vp)]
    L.csdr_amd_shift_addition_init.argtypes = [fl, vp]
    for nm in ("u8_f", "s8_f", "s16_f", "f_u8", "f_s8", "f_s16"):
        getattr(L, "csdr_amd_convert_" + nm).argtypes = [vp, vp, vp, sz]
    L.csdr_amd_convert_f_s24.argtypes = [vp, vp, vp, sz, i]
    L.csdr_amd_convert_s24_f.argtypes = [vp, vp, vp, sz, i]
    L.csdr_amd_rotator_generate.argtypes = [vp, i, fl, C.POINTER(fl), vp, sz, i, i]
    L.csdr_amd_debug_shift_scans_ahead.restype = ll; L.csdr_amd_debug_shift_scans_ahead.argtypes = [vp]
    L.csdr_amd_mix_cc.argtypes = [vp, vp, vp, vp, i, sz, sz, sz]
    L.csdr_amd_mix_fc.argtypes = [vp, vp, vp, vp, i, sz, sz, sz]
    L.csdr_amd_shift_cc.argtypes = [vp, i, fl, C.POINTER(fl), vp, vp, i, sz, sz, sz, i, i]
    L.csdr_amd_decimating_shift_addition_cc.argtypes = [vp, vp, vp, i, i, sz, sz, vp, i, vp]
    L.csdr_amd_fir_decimate_cc.argtypes = [vp, vp, vp, i, i, sz, sz, i, vp, i]
    L.csdr_amd_fir_last_kernel.restype = C.c_char_p; L.csdr_amd_fir_last_kernel.argtypes = []
    L.csdr_amd_fir_last_instance.restype = C.c_char_p; L.csdr_amd_fir_last_instance.argtypes = []
    L.csdr_amd_audio_last_path.restype = C.c_char_p; L.csdr_amd_audio_last_path.argtypes = []
    L.csdr_amd_fir_ff_last_instance.restype = C.c_char_p; L.csdr_amd_fir_ff_last_instance.argtypes = []
    L.csdr_amd_fir_ff.argtypes = [vp, vp, vp, i, i, sz, sz, vp, i]
    L.csdr_amd_fmdemod_quadri_cf.argtypes = [vp, vp, vp, i, sz, sz, sz, vp]
    L.csdr_amd_limit_ff.argtypes = [vp, vp, vp, sz, fl]
    L.csdr_amd_gain_ff.argtypes = [vp, vp, vp, sz, fl]
    L.csdr_amd_deemphasis_wfm_ff.argtypes = [vp, vp, vp, i, sz, sz, sz, fl, i, vp]
    L.csdr_amd_fastagc_ff.argtypes = [vp, vp, vp, i, i, i, sz, sz, fl, vp]
    L.csdr_amd_fracdec_create.restype = vp; L.csdr_amd_fracdec_create.argtypes = [fl, i, vp, i]
    L.csdr_amd_fracdec_destroy.argtypes = [vp]
    L.csdr_amd_fractional_decimator_ff.argtypes = [vp, vp, vp, vp, i, i, sz, sz, C.POINTER(i)]
    L.csdr_amd_fracdec_set_cli_bufsize.restype = None; L.csdr_amd_fracdec_set_cli_bufsize.argtypes = [vp, i]
    L.csdr_amd_fracdec_set_where.restype = None; L.csdr_amd_fracdec_set_where.argtypes = [vp, fl]
    L.csdr_amd_fracdec_get_where.restype = fl; L.csdr_amd_fracdec_get_where.argtypes = [vp]
    L.csdr_amd_fftfilt_create.restype = vp; L.csdr_amd_fftfilt_create.argtypes = [vp, i, vp, i, i, i]
    L.csdr_amd_fftfilt_set_taps.argtypes = [vp, vp, i]
    if hasattr(L, "csdr_amd_fftfilt_create_per_stream"):
        L.csdr_amd_fftfilt_create_per_stream.restype = vp; L.csdr_amd_fftfilt_create_per_stream.argtypes = [vp, i, vp, i, i, i]
        L.csdr_amd_fftfilt_set_stream_taps.argtypes = [vp, i, vp, i]
        L.csdr_amd_fftfilt_per_stream.argtypes = [vp]
    L.csdr_amd_fftfilt_destroy.argtypes = [vp]
    L.csdr_amd_fftfilt_input_size.argtypes = [vp]
    L.csdr_amd_fftfilt_reset.argtypes = [vp]
    L.csdr_amd_fftfilt_kernel_name.restype = C.c_char_p; L.csdr_amd_fftfilt_kernel_name.argtypes = [vp]
    L.csdr_amd_fftfilt_window.argtypes = [vp]
    L.csdr_amd_fftfilt_process.argtypes = [vp, vp, vp, i, sz, sz]
    L.csdr_amd_fft_c2c.argtypes = [vp, vp, vp, i, i]
    L.csdr_amd_fastddc_init.argtypes = [vp, fl, i, fl]
    L.csdr_amd_fastddc_fwd_create.restype = vp; L.csdr_amd_fastddc_fwd_create.argtypes = [vp, vp, i]
    L.csdr_amd_fastddc_fwd_destroy.argtypes = [vp]
    L.csdr_amd_fastddc_fwd_process.argtypes = [vp, vp, vp, i]
    L.csdr_amd_fastddc_inv_create.restype = vp; L.csdr_amd_fastddc_inv_create.argtypes = [vp, fl, i, vp, i, i, i]
    L.csdr_amd_fastddc_inv_destroy.argtypes = [vp]
    L.csdr_amd_fastddc_inv_geometry.argtypes = [vp, i, vp]
    L.csdr_amd_fastddc_inv_max_output.argtypes = [vp, i]
    L.csdr_amd_fastddc_inv_process.argtypes = [vp, vp, i, vp, sz, vp]
    L.csdr_amd_fastddc_bank_create.restype = vp; L.csdr_amd_fastddc_bank_create.argtypes = [vp, fl, i, vp, i, i, i]
    L.csdr_amd_fastddc_bank_destroy.argtypes = [vp]; L.csdr_amd_fastddc_bank_destroy.restype = None
    L.csdr_amd_fastddc_bank_set_rate.argtypes = [vp, i, fl]
    L.csdr_amd_fastddc_bank_input_size.argtypes = [vp]
    L.csdr_amd_fastddc_bank_max_output.argtypes = [vp, i]
    L.csdr_amd_fastddc_bank_process.argtypes = [vp, vp, i, vp, sz, vp]
    L.csdr_amd_fastddc_bank_inverse.restype = vp; L.csdr_amd_fastddc_bank_inverse.argtypes = [vp]
    L.csdr_amd_fastddc_bank_submit.argtypes = [vp, vp, i]
    L.csdr_amd_fastddc_bank_collect.argtypes = [vp, vp, sz, vp]
    L.csdr_amd_comm_unique_id.argtypes = [vp]
    L.csdr_amd_comm_create.restype = vp; L.csdr_amd_comm_create.argtypes = [vp, vp, i, i]
    L.csdr_amd_comm_destroy.argtypes = [vp]; L.csdr_amd_comm_destroy.restype = None
    L.csdr_amd_comm_rank.argtypes = [vp]; L.csdr_amd_comm_world.argtypes = [vp]
    L.csdr_amd_comm_broadcast.argtypes = [vp, vp, sz, i]
    L.csdr_amd_comm_dup.restype = vp; L.csdr_amd_comm_dup.argtypes = [vp]
    L.csdr_amd_comm_selftest.argtypes = [vp, sz, C.c_char_p, sz]
    L.csdr_amd_fastddc_bank_create_sharded.restype = vp; L.csdr_amd_fastddc_bank_create_sharded.argtypes = [vp, fl, i, vp, i, i, i, vp]
    L.csdr_amd_fastddc_bank_channel_slice.argtypes = [vp, C.POINTER(i), C.POINTER(i)]
    L.csdr_amd_fastddc_bank_create_sharded_by.restype = vp; L.csdr_amd_fastddc_bank_create_sharded_by.argtypes = [vp, fl, i, vp, i, i, i, vp, i]
    L.csdr_amd_fastddc_bank_shard_mode.argtypes = [vp]
    L.csdr_amd_fastddc_bank_default_shard_mode.argtypes = [i]
    L.csdr_amd_fastddc_bank_local_blocks.argtypes = [vp, i, C.POINTER(i), C.POINTER(i)]
    L.csdr_amd_fastddc_bank_overlap.argtypes = [vp]
    L.csdr_amd_fastddc_bank_submit_local.argtypes = [vp, vp, i]
    if hasattr(L, "csdr_amd_fastddc_bank_process_s16"):
        for nm in ("s16", "u8"):
            getattr(L, "csdr_amd_fastddc_bank_process_" + nm).argtypes = [vp, vp, i, vp, sz, vp]
            getattr(L, "csdr_amd_fastddc_bank_submit_" + nm).argtypes = [vp, vp, i]
            getattr(L, "csdr_amd_fastddc_bank_submit_local_" + nm).argtypes = [vp, vp, i]
    L.csdr_amd_fastddc_bank_finish.argtypes = [vp, vp]
    L.csdr_amd_fastddc_bank_set_rate_global.argtypes = [vp, i, fl]
    L.csdr_amd_loopback_create.restype = vp; L.csdr_amd_loopback_create.argtypes = [i]
    L.csdr_amd_loopback_destroy.argtypes = [vp]; L.csdr_amd_loopback_destroy.restype = None
    L.csdr_amd_loopback_abort.argtypes = [vp]; L.csdr_amd_loopback_abort.restype = None
    L.csdr_amd_comm_create_loopback.restype = vp; L.csdr_amd_comm_create_loopback.argtypes = [vp, vp, i]
    L.csdr_amd_comm_create_null.restype = vp; L.csdr_amd_comm_create_null.argtypes = [vp, i, i]
    L.csdr_amd_comm_create_ipc.restype = vp; L.csdr_amd_comm_create_ipc.argtypes = [vp, C.c_char_p, i, i]
    L.csdr_amd_fastddc_inv_kernel_name.restype = C.c_char_p; L.csdr_amd_fastddc_inv_kernel_name.argtypes = [vp]
    L.csdr_amd_fastddc_inv_kernels.restype = C.c_char_p; L.csdr_amd_fastddc_inv_kernels.argtypes = [vp]
    L.csdr_amd_fastddc_inv_set_profiling.argtypes = [vp, i]
    L.csdr_amd_fastddc_inv_kernel_time.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.csdr_amd_fastddc_inv_stage_time.argtypes = [vp, i, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.csdr_amd_wfm_create.restype = vp; L.csdr_amd_wfm_create.argtypes = [vp, i, fl, i, vp, i, i, fl, i, sz]
    L.csdr_amd_wfm_destroy.argtypes = [vp]
    L.csdr_amd_wfm_reset.argtypes = [vp]
    L.csdr_amd_wfm_process.restype = C.c_long; L.csdr_amd_wfm_process.argtypes = [vp, vp, sz, sz, vp, vp, sz]
    L.csdr_amd_wfm_kernel_name.restype = C.c_char_p; L.csdr_amd_wfm_kernel_name.argtypes = [vp]
    if hasattr(L, "csdr_amd_wfm_deemph_exact"):          # (absent from older builds selected with CSDR_AMD_LIB for A/B runs)
        L.csdr_amd_wfm_deemph_exact.argtypes = [fl, i, i]
        L.csdr_amd_wfm_deemph_warm_samples.argtypes = [i]
        L.csdr_amd_wfm_exact_deemphasis.argtypes = [vp]
        L.csdr_amd_wfm_set_deemphasis_state.argtypes = [vp, vp]
    ll = C.c_longlong; db = C.c_double
    L.csdr_amd_wfm_ring_create.restype = vp; L.csdr_amd_wfm_ring_create.argtypes = [vp, i, fl, i, vp, i, i, fl, i, sz, i]
    L.csdr_amd_wfm_ring_destroy.argtypes = [vp]; L.csdr_amd_wfm_ring_destroy.restype = None
    L.csdr_amd_wfm_ring_reset.argtypes = [vp]
    L.csdr_amd_wfm_ring_acquire.argtypes = [vp, ll, db]
    L.csdr_amd_wfm_ring_input.restype = vp; L.csdr_amd_wfm_ring_input.argtypes = [vp, ll, C.POINTER(sz)]
    L.csdr_amd_wfm_ring_submit.restype = ll; L.csdr_amd_wfm_ring_submit.argtypes = [vp]
    L.csdr_amd_wfm_ring_wait.restype = C.c_long; L.csdr_amd_wfm_ring_wait.argtypes = [vp, ll, db]
    L.csdr_amd_wfm_ring_output.restype = vp; L.csdr_amd_wfm_ring_output.argtypes = [vp, ll, C.POINTER(sz)]
    L.csdr_amd_wfm_ring_set_rate.argtypes = [vp, fl]
    L.csdr_amd_wfm_ring_get_rate.restype = fl; L.csdr_amd_wfm_ring_get_rate.argtypes = [vp]
    L.csdr_amd_wfm_ring_set_timeouts.argtypes = [vp, db, db]
    L.csdr_amd_wfm_ring_resident.argtypes = [vp]
    L.csdr_amd_wfm_ring_stop.argtypes = [vp]
    L.csdr_amd_wfm_ring_slots.argtypes = [vp]
    L.csdr_amd_wfm_ring_grid.argtypes = [vp]
    L.csdr_amd_wfm_ring_launches.restype = C.c_long; L.csdr_amd_wfm_ring_launches.argtypes = [vp]
    L.csdr_amd_wfm_ring_submitted.restype = ll; L.csdr_amd_wfm_ring_submitted.argtypes = [vp]
    L.csdr_amd_wfm_ring_block_times.argtypes = [vp, ll, C.POINTER(db), C.POINTER(db)]
    L.csdr_amd_wfm_ring_replay.argtypes = [vp, C.c_long, vp, vp]
    L.csdr_amd_wfm_ring_stats.argtypes = [vp, vp]
    L.csdr_amd_wfm_set_profiling.argtypes = [vp, i]
    L.csdr_amd_wfm_kernel_time.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.csdr_amd_ddc_create.restype = vp; L.csdr_amd_ddc_create.argtypes = [vp, i, fl, i, vp, i, sz]
    if hasattr(L, "csdr_amd_ddc_create_rates"):          # (absent from older builds selected with CSDR_AMD_LIB for A/B runs)
        L.csdr_amd_ddc_create_rates.restype = vp; L.csdr_amd_ddc_create_rates.argtypes = [vp, i, vp, i, vp, i, sz]
        L.csdr_amd_ddc_set_rate.argtypes = [vp, i, fl]
        L.csdr_amd_ddc_get_rate.restype = fl; L.csdr_amd_ddc_get_rate.argtypes = [vp, i]
        L.csdr_amd_ddc_fallback.argtypes = [vp]
        L.csdr_amd_wfm_fallback.argtypes = [vp]
        L.csdr_amd_wfm_create_rates.restype = vp; L.csdr_amd_wfm_create_rates.argtypes = [vp, i, vp, i, vp, i, i, fl, i, sz]
        L.csdr_amd_wfm_set_rate.argtypes = [vp, i, fl]
        L.csdr_amd_wfm_get_rate.restype = fl; L.csdr_amd_wfm_get_rate.argtypes = [vp, i]
        L.csdr_amd_nfm_create_rates.restype = vp; L.csdr_amd_nfm_create_rates.argtypes = [vp, i, vp, i, vp, i, i, i, fl, fl, sz]
        L.csdr_amd_nfm_set_rate.argtypes = [vp, i, fl]
    L.csdr_amd_ddc_destroy.argtypes = [vp]
    L.csdr_amd_ddc_reset.argtypes = [vp]
    L.csdr_amd_ddc_process.restype = C.c_long; L.csdr_amd_ddc_process.argtypes = [vp, vp, sz, sz, vp, sz]
    L.csdr_amd_ddc_kernel_name.restype = C.c_char_p; L.csdr_amd_ddc_kernel_name.argtypes = [vp]
    if hasattr(L, "csdr_amd_ddc_last_instance"):         # (absent from older builds selected with CSDR_AMD_LIB for A/B runs)
        L.csdr_amd_ddc_last_instance.restype = C.c_char_p; L.csdr_amd_ddc_last_instance.argtypes = [vp]
    if hasattr(L, "csdr_amd_ddc_seed_stats"):            # (absent from older builds selected with CSDR_AMD_LIB for A/B runs)
        L.csdr_amd_ddc_seed_stats.argtypes = [vp, C.POINTER(C.c_long)]; L.csdr_amd_wfm_seed_stats.argtypes = [vp, C.POINTER(C.c_long)]
        L.csdr_amd_ddc_tables_built.restype = C.c_long; L.csdr_amd_ddc_tables_built.argtypes = [vp]
        L.csdr_amd_wfm_tables_built.restype = C.c_long; L.csdr_amd_wfm_tables_built.argtypes = [vp]
    L.csdr_amd_ddc_set_profiling.argtypes = [vp, i]
    L.csdr_amd_ddc_kernel_time.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.csdr_amd_nfm_create.restype = vp; L.csdr_amd_nfm_create.argtypes = [vp, i, fl, i, vp, i, i, i, fl, fl, sz]
    L.csdr_amd_nfm_destroy.argtypes = [vp]
    L.csdr_amd_nfm_reset.argtypes = [vp]
    L.csdr_amd_nfm_process.restype = C.c_long; L.csdr_amd_nfm_process.argtypes = [vp, vp, sz, sz, vp, vp, sz]
    L.csdr_amd_nfm_front_end.restype = vp; L.csdr_amd_nfm_front_end.argtypes = [vp]
    L.csdr_amd_fmrx_create.restype = vp; L.csdr_amd_fmrx_create.argtypes = [vp, i, i, i, fl, fl, sz]
    L.csdr_amd_fmrx_process.restype = ll; L.csdr_amd_fmrx_process.argtypes = [vp, vp, sz, ll, vp, vp, sz]
    L.csdr_amd_fmrx_max_output.restype = ll; L.csdr_amd_fmrx_max_output.argtypes = [vp, ll]
    L.csdr_amd_fmrx_plan.argtypes = [i, ll, i, i, C.POINTER(ll), C.POINTER(i)]
    L.csdr_amd_fmrx_fill.argtypes = [vp]
    L.csdr_amd_fmrx_create_squelched.restype = vp; L.csdr_amd_fmrx_create_squelched.argtypes = [vp, i, i, i, fl, fl, sz, i, i, vp]
    L.csdr_amd_fmrx_process_squelched.restype = ll; L.csdr_amd_fmrx_process_squelched.argtypes = [vp, vp, sz, ll, vp, vp, sz, vp, sz, vp, C.POINTER(i)]
    L.csdr_amd_fmrx_squelch_plan.argtypes = [i, ll, i, C.POINTER(ll), C.POINTER(i)]
    L.csdr_amd_fmrx_set_squelch_level.argtypes = [vp, i, fl]
    L.csdr_amd_fmrx_get_squelch_level.argtypes = [vp, i, C.POINTER(fl)]
    L.csdr_amd_fmrx_squelch_held.argtypes = [vp]
    L.csdr_amd_fmrx_squelch_block_index.restype = ll; L.csdr_amd_fmrx_squelch_block_index.argtypes = [vp]
    L.csdr_amd_wfmrx_create.restype = vp; L.csdr_amd_wfmrx_create.argtypes = [vp, i, fl, i, vp, i, i, fl, i, sz]
    L.csdr_amd_wfmrx_process.restype = ll; L.csdr_amd_wfmrx_process.argtypes = [vp, vp, sz, ll, vp, vp, sz]
    L.csdr_amd_wfmrx_max_output.restype = ll; L.csdr_amd_wfmrx_max_output.argtypes = [vp, ll]
    L.csdr_amd_wfmrx_plan.argtypes = [fl, i, i, i, fl, i, ll, C.POINTER(ll), C.POINTER(fl), C.POINTER(i)]
    L.csdr_amd_wfmrx_held.argtypes = [vp]
    L.csdr_amd_wfmrx_where.restype = fl; L.csdr_amd_wfmrx_where.argtypes = [vp]
    L.csdr_amd_wfmrx_create_squelched.restype = vp; L.csdr_amd_wfmrx_create_squelched.argtypes = [vp, i, fl, i, vp, i, i, fl, i, sz, i, i, vp]
    L.csdr_amd_wfmrx_process_squelched.restype = ll; L.csdr_amd_wfmrx_process_squelched.argtypes = [vp, vp, sz, ll, vp, vp, sz, vp, sz, vp, C.POINTER(i)]
    L.csdr_amd_wfmrx_squelch_plan.argtypes = [i, ll, i, C.POINTER(ll), C.POINTER(i)]
    L.csdr_amd_wfmrx_set_squelch_level.argtypes = [vp, i, fl]
    L.csdr_amd_wfmrx_get_squelch_level.argtypes = [vp, i, C.POINTER(fl)]
    L.csdr_amd_wfmrx_squelch_held.argtypes = [vp]
    L.csdr_amd_wfmrx_squelch_block_index.restype = ll; L.csdr_amd_wfmrx_squelch_block_index.argtypes = [vp]
    _lib = L
    return L


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


class DevBuf:
    """A device allocation owned by a Context."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        self.ptr = lib().csdr_amd_malloc(ctx.h, max(self.nbytes, 16))
        if not self.ptr:
            raise CsdrAmdError(ctx.err())

    def free(self):
        if self.ptr and self.ctx.h:                  # a buffer that outlives its (closed) context is gone with the process
            lib().csdr_amd_free(self.ctx.h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def at(self, byte_offset):
        return C.c_void_p(self.ptr + int(byte_offset))


class _Handle:
    """A C object of the library: `h` is what csdr_amd_<pre>_create returned, the other entry points are csdr_amd_<pre>_<name>(h, ...).
    ctx is the Context the object was created on, or None for an object whose create takes no context.  Usable as `with`: closed on every path."""
    h = None                                             # (a constructor that raised in front of _Handle.__init__ leaves nothing to close)

    def __init__(self, ctx, pre, h):
        self.ctx, self._pre, self._L = ctx, pre, ctx.L if ctx is not None else lib()
        if not h:
            raise CsdrAmdError(ctx.err() if ctx is not None else self._L.csdr_amd_last_error().decode())
        self.h = h

    def _fn(self, name):
        return getattr(self._L, "csdr_amd_%s_%s" % (self._pre, name))

    def _call(self, name, *args):
        return self.ctx.check(self._fn(name)(self.h, *args), "%s_%s" % (self._pre, name))

    def reset(self):
        self._call("reset")

    def force_generic(self, on=True):
        self._call("force_generic", int(on))

    def kernel_name(self):
        return self._fn("kernel_name")(self.h).decode()

    def close(self):
        """Destroys the object once.  After Context.close the object's context is gone and destroy would read it: the handle is dropped and the
        object goes with the process."""
        h, self.h = self.h, None
        if h and (self.ctx is None or self.ctx.h):
            self._fn("destroy")(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# The members below exist for some objects only; a class lists the mixins of the entry points its C object has.
class _MaxOut:
    """csdr_amd_<pre>_max_out: the most outputs per stream that a call of n_in inputs can write"""

    def max_out(self, n_in):
        return int(self._fn("max_out")(self.h, int(n_in)))


class _PerChannel:
    """csdr_amd_<pre>_reset_channel: one channel back to its start state, the others untouched"""

    def reset_channel(self, ch):
        self._call("reset_channel", int(ch))


class _ChannelState(_PerChannel):
    """csdr_amd_<pre>_get_channel / _set_channel: one channel's state as the class's `_chan` structure"""

    def get_channel(self, ch):
        st = self._chan()
        self._call("get_channel", int(ch), C.byref(st))
        return st

    def set_channel(self, ch, st):
        self._call("set_channel", int(ch), C.byref(st))


class _Lanes:
    """csdr_amd_<pre>_set_lanes / _lanes: channels per wave of the tiled kernel (0: the library chooses)"""

    def set_lanes(self, lanes):
        self._call("set_lanes", int(lanes))

    def lanes(self):
        return int(self._fn("lanes")(self.h))


def _counted_calls(obj, x, calls, extras=(), **inputs):
    """The call loop of the objects whose process_dev reports one output count per channel: x [n_channels, n] host items, cut into calls of `calls` items
    -> per channel, the tuple of its concatenated outputs: the "d_out" row (obj.out_dtype) and one row per (process_dev keyword, dtype) in `extras`.
    inputs: further process_dev keywords, passed on as they are."""
    ctx, (s, n) = obj.ctx, x.shape
    rows = [("d_out", obj.out_dtype)] + list(extras)
    di = ctx.upload(x) if n else ctx.alloc(256)
    opitch = max(obj.max_out(max(calls) if calls else 0), 1)
    bufs = [ctx.alloc(np.dtype(dt).itemsize * opitch * s + 256) for _, dt in rows]
    dc = ctx.alloc(4 * s + 256)
    parts = [[[] for _ in rows] for _ in range(s)]
    at = 0
    for k in calls:
        obj.process_dev(d_in=di.at(x.itemsize * at), n_in=k, in_pitch=max(n, 1), out_pitch=opitch, d_counts=dc.ptr,
                        **{nm: b.ptr for (nm, _), b in zip(rows, bufs)}, **inputs)
        cnt = ctx.download(dc, np.int32, s)
        for j, ((_, dt), b) in enumerate(zip(rows, bufs)):
            y = ctx.download(b, dt, opitch * s).reshape(s, opitch)
            for c in range(s):
                parts[c][j].append(y[c, :cnt[c]].copy())
        at += k
    return [tuple(np.concatenate(p) if p else np.zeros(0, dt) for p, (_, dt) in zip(parts[c], rows)) for c in range(s)]


class Waterfall(_Handle):
    """csdr_amd_waterfall: n_streams streams in lockstep -> rows of fft_size float dB values (out_format "db") or (fft_size+10)/2 ADPCM bytes ("adpcm").
    in_format "cf32" / "u8": complex samples, rows with the halves exchanged; "f32" / "s16": real samples, fft_size is the number of output bins (fft_fc's
    fft_out_size), every_n and the sample counts are in real samples, rows are one-sided (DC first)."""
    # in_format -> (CSDR_AMD_WF_IN_*, host dtype, host elements per sample, bytes per sample)
    FORMATS = {"cf32": (0, c64, 1, 8), "u8": (1, np.uint8, 2, 2), "f32": (2, f32, 1, 4), "s16": (3, np.int16, 1, 2)}

    def __init__(self, ctx, fft_size, every_n, avgnumber, add_db, window, in_format, out_format, n_streams, max_samples_per_call):
        self.fft, self.every, self.avg, self.n_streams, self.max_in = fft_size, every_n, avgnumber, n_streams, int(max_samples_per_call)
        self.in_format, self.out_format = in_format, out_format
        self._code, self._dtype, self._per, self._eb = self.FORMATS.get(in_format, self.FORMATS["cf32"])
        _Handle.__init__(self, ctx, "waterfall", ctx.L.csdr_amd_waterfall_create(ctx.h, fft_size, every_n, WINDOWS[window], avgnumber, add_db,
                                                                                  self._code, 1 if out_format == "adpcm" else 0, n_streams, self.max_in))
        self.row_bytes = 4 * fft_size if out_format == "db" else (fft_size + 10) // 2

    def max_rows(self, n_in):
        return (n_in + self.fft) // self.every + 2

    def process_dev(self, d_in, n_in, in_pitch, d_out, out_pitch):
        """device pointers: n_in new samples per stream (in_pitch samples apart) -> rows per stream written at d_out (out_pitch bytes apart)"""
        rows = C.c_int(0)
        self._call("process", d_in, n_in, in_pitch, d_out, out_pitch, C.byref(rows))
        return rows.value

    def process(self, x, calls=None):
        """x: [n_streams, ...] host samples (u8 IQ bytes, complex64, float32 or int16 by in_format); calls: list of per-call sample counts (default one
        call) -> [n_streams, rows, ...]"""
        x = np.ascontiguousarray(x, self._dtype)
        if x.ndim == 1:
            x = x[None]
        n = x.shape[1] // self._per
        eb = self._eb
        calls = [n] if calls is None else list(calls)
        di = self.ctx.upload(x)
        opitch = (self.max_rows(max(calls)) * self.row_bytes + 255) // 256 * 256
        do = self.ctx.alloc(opitch * self.n_streams + 256)
        out = [[] for _ in range(self.n_streams)]
        at = 0
        for k in calls:
            r = self.process_dev(di.at(eb * at), k, n, do.ptr, opitch)
            if r:
                y = self.ctx.download(do, np.uint8, opitch * self.n_streams).reshape(self.n_streams, opitch)[:, :r * self.row_bytes]
                for s in range(self.n_streams):
                    out[s].append(y[s].copy())
            at += k
        dt = f32 if self.out_format == "db" else np.uint8
        per = self.fft if self.out_format == "db" else self.row_bytes
        return np.stack([np.concatenate(o).view(dt).reshape(-1, per) if o else np.zeros((0, per), dt) for o in out])


def rational_resampler_get_lowpass_f(taps_length, interpolation, decimation, window="HAMMING"):
    """rational_resampler_get_lowpass_f (libcsdr.c:665-673), on the host"""
    t = np.zeros(taps_length, f32)
    lib().csdr_amd_rational_resampler_get_lowpass_f(_hp(t), taps_length, interpolation, decimation, WINDOWS[window])
    return t


def fir_interpolate_lowpass_f(taps_length, interpolation, window="HAMMING"):
    """the taps `csdr fir_interpolate_cc` designs (csdr.c:1212): firdes_lowpass_f(taps_length, 0.5 / interpolation, window), on the host"""
    t = np.zeros(taps_length, f32)
    lib().csdr_amd_firdes_lowpass_f(_hp(t), taps_length, C.c_float(np.float32(0.5) / np.float32(interpolation)), WINDOWS[window])
    return t


def resampler_schedule(interpolation, decimation, taps_length, n, last_taps_delay=0):
    """[n, 3] int32: (startingi, delayi, taps used) of rational_resampler_ff's first n outputs from last_taps_delay (host)"""
    out = np.zeros((n, 3), np.int32)
    if lib().csdr_amd_debug_resampler_schedule(interpolation, decimation, taps_length, last_taps_delay, n, _hp(out)) < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return out


def resampler_window(interpolation, decimation, taps_length, input_size, last_taps_delay=0):
    """what one rational_resampler_ff call returns: (input_processed, output_size, last_taps_delay)"""
    st = np.zeros(3, np.int32)
    if lib().csdr_amd_resampler_window(interpolation, decimation, taps_length, input_size, last_taps_delay, _hp(st)) < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return tuple(int(v) for v in st)


class _Resampling(_Handle, _MaxOut):
    """Shared driver of csdr_amd_resampler (real, "resampler") and csdr_amd_interp (complex, "interp"): n_streams streams in lockstep."""
    _dt, _eb = f32, 4

    def process_dev(self, d_in, n_in, in_pitch, d_out, out_pitch):
        """device pointers: n_in new samples per stream (in_pitch apart) -> outputs per stream written at d_out (out_pitch elements apart)"""
        n = C.c_longlong(0)
        self._call("process", d_in, n_in, in_pitch, d_out, out_pitch, C.byref(n))
        return n.value

    def process(self, x, calls=None):
        """x: [n_streams, n] (or [n]) host samples; calls: per-call sample counts (default one call) -> [n_streams, outputs] (or [outputs])"""
        x = np.ascontiguousarray(x, self._dt)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None]
        s, n = x.shape
        calls = [n] if calls is None else list(calls)
        di = self.ctx.upload(x)
        opitch = max(self.max_out(max(calls) if calls else 0), 1)
        do = self.ctx.alloc(self._eb * opitch * s + 256)
        out, at = [], 0
        for k in calls:
            r = self.process_dev(di.at(self._eb * at), k, n, do.ptr, opitch)
            if r:
                out.append(self.ctx.download(do, self._dt, opitch * s).reshape(s, opitch)[:, :r].copy())
            at += k
        y = np.concatenate(out, axis=1) if out else np.zeros((s, 0), self._dt)
        return y[0] if squeeze else y

    def set_cli_bufsize(self, the_bufsize):
        self._call("set_cli_bufsize", int(the_bufsize))


class Resampler(_Resampling):
    """csdr_amd_resampler: rational_resampler_ff (libcsdr.c:607-640) by interpolation/decimation for n_streams float streams."""

    def __init__(self, ctx, interpolation, decimation, taps, n_streams=1, bufsize=None, last_taps_delay=0):
        self.I, self.D, self.n_streams = interpolation, decimation, n_streams
        self.taps = np.ascontiguousarray(taps, f32)
        _Handle.__init__(self, ctx, "resampler", ctx.L.csdr_amd_resampler_create(ctx.h, interpolation, decimation, _hp(self.taps), self.taps.size, n_streams))
        if bufsize:
            self.set_cli_bufsize(bufsize)
        if last_taps_delay:
            self.set_last_taps_delay(last_taps_delay)

    def set_last_taps_delay(self, d):
        self._call("set_last_taps_delay", int(d))


class Psk31Params(C.Structure):
    """csdr_amd_psk31_params"""
    _fields_ = [("rate", C.c_float), ("reference", C.c_float), ("max_gain", C.c_float), ("algorithm", C.c_int), ("decimation", C.c_int),
                ("loop_gain", C.c_float), ("max_error", C.c_float), ("use_q", C.c_int)]


class Psk31Chan(C.Structure):
    """csdr_amd_psk31_chan: one channel's state"""
    _fields_ = [("gain", C.c_float), ("tail_len", C.c_int), ("correction_offset", C.c_int), ("base", C.c_uint), ("last_i", C.c_float),
                ("last_q", C.c_float), ("varicode_shr", C.c_ulonglong)]


PSK31_STAGES = {"agc": 0, "timing": 1, "dbpsk": 2, "varicode": 3}
TIMING_ALGORITHMS = {"GARDNER": 0, "EARLYLATE": 1}


def psk31_params(rate=0.001, reference=0.5, max_gain=65535.0, algorithm="GARDNER", decimation=256, loop_gain=0.5, max_error=2.0, use_q=True):
    """the chain's parameters; the defaults are OpenWebRX's `simple_agc_cc 0.001 0.5 | timing_recovery_cc GARDNER 256 0.5 2 --add_q`"""
    alg = TIMING_ALGORITHMS[algorithm] if isinstance(algorithm, str) else int(algorithm)
    return Psk31Params(rate, reference, max_gain, alg, decimation, loop_gain, max_error, int(bool(use_q)))


def _psk31_stage(s):
    return PSK31_STAGES[s] if isinstance(s, str) else int(s)


def _psk31_types(first, last):
    return (np.uint8 if first == 3 else c64), (c64 if last <= 1 else np.uint8)


def psk31_debug_walk(params, first="agc", last="varicode", x=None, cuts=(), state=None, with_extras=False):
    """CPU run of k_psk31's walk for one channel (csdr_amd_debug_psk31_walk): x cut into calls of `cuts` items and the rest -> outputs
    (and, with_extras, the timing errors and indexes).  state: a Psk31Chan carried in and out."""
    f, l = _psk31_stage(first), _psk31_stage(last)
    ti, to = _psk31_types(f, l)
    x = np.ascontiguousarray(x, ti)
    n = x.size
    cap = n + 16 if (f >= 2 or l == 0) else 2 * n // max(params.decimation, 1) + 3 * len(cuts) + 16
    out = np.zeros(cap, to)
    err = np.zeros(cap, f32) if with_extras else None
    idx = np.zeros(cap, np.uint32) if with_extras else None
    cu = np.ascontiguousarray(cuts, np.int64)
    k = lib().csdr_amd_debug_psk31_walk(C.byref(params), f, l, _hp(x), n, _hp(cu) if cu.size else None, cu.size, _hp(out),
                                        _hp(err) if with_extras else None, _hp(idx) if with_extras else None, C.byref(state) if state is not None else None)
    if k < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return (out[:k], err[:k], idx[:k]) if with_extras else out[:k]


def psk31_varicode_table():
    """[128, 2] int32: (code, length) of each character, as the library holds it"""
    t = np.zeros(256, np.int32)
    lib().csdr_amd_psk31_varicode_table(_hp(t))
    return t.reshape(128, 2)


class Psk31(_Handle, _MaxOut, _ChannelState, _Lanes):
    """csdr_amd_psk31: the BPSK31 receive chain (simple_agc_cc | timing_recovery_cc | dbpsk_decoder_c_u8 | psk31_varicode_decoder_u8_u8) for
    n_channels channels, stages first..last ("agc", "timing", "dbpsk", "varicode"), state kept on the device between calls."""
    _chan = Psk31Chan

    def __init__(self, ctx, params=None, n_channels=1, first="agc", last="varicode"):
        self.n_channels = n_channels
        self.params = params if params is not None else psk31_params()
        self.first, self.last = _psk31_stage(first), _psk31_stage(last)
        self.in_dtype, self.out_dtype = _psk31_types(self.first, self.last)
        _Handle.__init__(self, ctx, "psk31", ctx.L.csdr_amd_psk31_create(ctx.h, C.byref(self.params), n_channels, self.first, self.last))

    def process_dev(self, d_in, n_in, in_pitch, d_out, out_pitch, d_counts, d_err=None, d_idx=None):
        """device pointers; counts (n_channels int32) receives each channel's output count.  Asynchronous."""
        self._call("process", d_in, n_in, in_pitch, d_out, out_pitch, d_counts, d_err, d_idx)

    def process(self, x, calls=None, with_extras=False):
        """x: [n_channels, n] (or [n]) host items; calls: per-call item counts (default one call) -> a list of per-channel output arrays
        (or one array for 1-D x); with_extras (last == "timing"): (symbols, errors, indexes) per channel."""
        x = np.ascontiguousarray(x, self.in_dtype)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None]
        s, n = x.shape
        if s != self.n_channels:
            raise ValueError("x has %d rows for %d channels" % (s, self.n_channels))
        calls = [n] if calls is None else list(calls)
        if with_extras:
            res = _counted_calls(self, x, calls, (("d_err", f32), ("d_idx", np.uint32)))
        else:
            res = [r[0] for r in _counted_calls(self, x, calls)]
        return res[0] if squeeze else res


class Psk31TxChan(C.Structure):
    """csdr_amd_psk31tx_chan: one channel's state"""
    _fields_ = [("diff_state", C.c_ubyte), ("last_i", C.c_float), ("last_q", C.c_float)]


PSK31TX_STAGES = {"varicode": 0, "diff": 1, "mod": 2, "shape": 3}


def _psk31tx_stage(s):
    return PSK31TX_STAGES[s] if isinstance(s, str) else int(s)


def _psk31tx_types(first, last):
    return (c64 if first == 3 else np.uint8), (c64 if last >= 2 else np.uint8)


def _psk31tx_max_out(first, last, interpolation, n):
    return n * (12 if first == 0 else 1) * (interpolation if last == 3 else 1)


def psk31tx_tables(n_psk=2, interpolation=256):
    """The host tables of a transmit object (csdr_amd_psk31tx_tables) -> (256 symbols complex64, `interpolation` shaping factors float32)"""
    sym = np.zeros(256, c64); rate = np.zeros(interpolation, f32)
    if lib().csdr_amd_psk31tx_tables(n_psk, interpolation, _hp(sym), _hp(rate)) < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return sym, rate


def psk31tx_debug_walk(x, n_psk=2, interpolation=256, first="varicode", last="shape", cuts=(), state=None):
    """CPU run of k_psk31tx_generic's walk for one channel (csdr_amd_debug_psk31tx_walk): x cut into calls of `cuts` items and the rest -> outputs.
    state: a Psk31TxChan carried in and out."""
    f, l = _psk31tx_stage(first), _psk31tx_stage(last)
    ti, to = _psk31tx_types(f, l)
    x = np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, ti)
    out = np.zeros(_psk31tx_max_out(f, l, interpolation, x.size) + 16, to)
    cu = np.ascontiguousarray(cuts, np.int64)
    k = lib().csdr_amd_debug_psk31tx_walk(n_psk, interpolation, f, l, _hp(x), x.size, _hp(cu) if cu.size else None, cu.size, _hp(out),
                                          C.byref(state) if state is not None else None)
    if k < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return out[:k]


class Psk31Tx(_Handle, _MaxOut, _ChannelState):
    """csdr_amd_psk31tx: the BPSK31 transmit chain (psk31_varicode_encoder_u8_u8 | differential_encoder_u8_u8 | psk_modulator_u8_c n_psk |
    psk31_interpolate_sine_cc interpolation) for n_channels channels, stages first..last ("varicode", "diff", "mod", "shape"), state kept on the
    device between calls."""
    _chan = Psk31TxChan

    def __init__(self, ctx, n_channels=1, n_psk=2, interpolation=256, first="varicode", last="shape"):
        self.n_channels, self.n_psk, self.interpolation = n_channels, n_psk, interpolation
        self.first, self.last = _psk31tx_stage(first), _psk31tx_stage(last)
        self.in_dtype, self.out_dtype = _psk31tx_types(self.first, self.last)
        _Handle.__init__(self, ctx, "psk31tx", ctx.L.csdr_amd_psk31tx_create(ctx.h, n_channels, n_psk, interpolation, self.first, self.last))

    def process_dev(self, d_in, n_in, d_in_counts, in_pitch, d_out, out_pitch, d_counts):
        """device pointers; in_counts (n_channels int32, or None) gives each channel's item count, counts receives its output count.  Asynchronous."""
        self._call("process", d_in, n_in, d_in_counts, in_pitch, d_out, out_pitch, d_counts)

    def process(self, x, in_counts=None, calls=None):
        """x: [n_channels, n] (or [n]) host items; in_counts: per-channel item counts of the (single) call, each 0..n; calls: per-call item counts
        (default one call) -> a list of per-channel output arrays (or one array for 1-D x)"""
        x = np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, self.in_dtype)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None]
        s, n = x.shape
        if s != self.n_channels:
            raise ValueError("x has %d rows for %d channels" % (s, self.n_channels))
        calls = [n] if calls is None else list(calls)
        dn = None
        if in_counts is not None:
            ic = np.ascontiguousarray(in_counts, np.int32)
            if ic.shape != (s,) or len(calls) != 1 or ic.min() < 0 or ic.max() > calls[0]:
                raise CsdrAmdError("psk31tx: in_counts holds one count of 0 .. n_in per channel, for one call")
            dn = self.ctx.upload(ic)
        res = [r[0] for r in _counted_calls(self, x, calls, d_in_counts=dn.ptr if dn else None)]
        return res[0] if squeeze else res


PULSETX_STAGES = {"mod": 0, "shape": 1}


def _pulsetx_stage(s):
    return PULSETX_STAGES[s] if isinstance(s, str) else int(s)


def firdes_rrc_f(taps_length, samples_per_symbol, beta):
    """firdes_rrc_f (libcsdr.c:2482-2497, csdr_amd_firdes_rrc_f): root raised cosine taps, taps_length odd -> float32"""
    t = np.zeros(taps_length, f32)
    if lib().csdr_amd_firdes_rrc_f(_hp(t), int(taps_length), int(samples_per_symbol), float(beta)) < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return t


def firdes_cosine_f(samples_per_symbol, taps_length=None):
    """firdes_cosine_f (libcsdr.c:2473-2480, csdr_amd_firdes_cosine_f): raised cosine pulse of 2 samples_per_symbol + 1 taps (the end taps 0) -> float32"""
    n = 2 * int(samples_per_symbol) + 1 if taps_length is None else int(taps_length)
    t = np.zeros(max(n, 1), f32)
    if lib().csdr_amd_firdes_cosine_f(_hp(t), n, int(samples_per_symbol)) < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return t


def pulsetx_debug_walk(x, taps, n_psk=4, interpolation=8, first="mod", last="shape", cuts=()):
    """CPU run of the pulse-shaping transmit object's definition for one channel (csdr_amd_debug_pulsetx_walk): x cut into calls of `cuts` items and the
    rest -> the outputs of all calls, concatenated"""
    f, l = _pulsetx_stage(first), _pulsetx_stage(last)
    x = np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, c64 if f == 1 else np.uint8)
    t = None if taps is None else np.ascontiguousarray(taps, f32)
    out = np.zeros(x.size * (max(int(interpolation), 1) if l == 1 else 1) + 16, c64)
    cu = np.ascontiguousarray(cuts, np.int64)
    k = lib().csdr_amd_debug_pulsetx_walk(n_psk, interpolation, _hp(t) if t is not None else None, t.size if t is not None else 0, f, l, _hp(x), x.size,
                                          _hp(cu) if cu.size else None, cu.size, _hp(out))
    if k < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return out[:k]


class PulseTx(_Handle, _MaxOut):
    """csdr_amd_pulsetx: psk_modulator_u8_c n_psk | plain_interpolate_cc interpolation | pulse_shaping_filter_cc (taps) for n_channels channels, stages
    first..last ("mod", "shape"); the symbols behind the last call are kept on the device."""

    def __init__(self, ctx, n_channels=1, n_psk=4, interpolation=8, taps=None, first="mod", last="shape"):
        self.n_channels, self.n_psk, self.interpolation = n_channels, n_psk, interpolation
        self.first, self.last = _pulsetx_stage(first), _pulsetx_stage(last)
        self.in_dtype = c64 if self.first == 1 else np.uint8
        t = None if taps is None else np.ascontiguousarray(taps, f32)
        _Handle.__init__(self, ctx, "pulsetx", ctx.L.csdr_amd_pulsetx_create(ctx.h, n_channels, n_psk, interpolation, _hp(t) if t is not None else None,
                                                                             t.size if t is not None else 0, self.first, self.last))

    def tile(self):
        """symbols per tile of k_pulsetx_poly"""
        return int(self._fn("tile")(self.h))

    def process_dev(self, d_in, n_in, in_pitch, d_out, out_pitch):
        """device pointers -> the outputs per channel of this call.  Asynchronous."""
        k = C.c_longlong(0)
        self._call("process", d_in, n_in, in_pitch, d_out, out_pitch, C.byref(k))
        return k.value

    def process(self, x, calls=None):
        """x: [n_channels, n] (or [n]) host symbols (bytes, or complex64 from "shape"); calls: per-call symbol counts (default one call) ->
        [n_channels, n_out] complex64, the outputs of all calls concatenated"""
        x = np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, self.in_dtype)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None]
        s, n = x.shape
        if s != self.n_channels:
            raise ValueError("x has %d rows for %d channels" % (s, self.n_channels))
        calls = [n] if calls is None else list(calls)
        if sum(calls) != n or min(calls, default=0) < 0:
            raise ValueError("calls do not add up to the %d symbols" % n)
        isz = x.dtype.itemsize
        di = self.ctx.upload(x) if n else self.ctx.alloc(256)
        pitch = max(self.max_out(max(calls, default=0)), 1)
        do = self.ctx.alloc(8 * pitch * s + 256)
        parts, pos = [], 0
        for m in calls:
            k = self.process_dev(di.at(pos * isz), m, max(n, 1), do.ptr, pitch)
            if k:
                parts.append(self.ctx.download(do, c64, pitch * s).reshape(s, pitch)[:, :k].copy())
            pos += m
        y = np.concatenate(parts, axis=1) if parts else np.zeros((s, 0), c64)
        return y[0] if squeeze else y


class PulseRxParams(C.Structure):
    """csdr_amd_pulserx_params; `taps` points into the array kept as `_taps`"""
    _fields_ = [("taps", C.c_void_p), ("taps_length", C.c_int), ("algorithm", C.c_int), ("decimation", C.c_int), ("loop_gain", C.c_float),
                ("max_error", C.c_float), ("use_q", C.c_int), ("gain", C.c_float), ("n_symbols", C.c_int), ("slice_q", C.c_int)]


class PulseRxChan(C.Structure):
    """csdr_amd_pulserx_chan: one channel's state (its raw tail stays on the device)"""
    _fields_ = [("tail_len", C.c_int), ("correction_offset", C.c_int), ("base", C.c_uint)]


PULSERX_STAGES = {"filter": 0, "timing": 1, "slice": 2}


def _pulserx_stage(s):
    return PULSERX_STAGES[s] if isinstance(s, str) else int(s)


def pulserx_params(taps=None, algorithm="GARDNER", decimation=8, loop_gain=0.5, max_error=2.0, use_q=True, gain=1.0, n_symbols=2, slice_q=False):
    """the receive object's parameters: `pulse_shaping_filter_cc` taps | `timing_recovery_cc algorithm decimation loop_gain max_error [--add_q]` |
    [`realpart_cf` |] `gain_ff gain | generic_slicer_f_u8 n_symbols` (slice_q: no realpart_cf, two bytes per symbol)"""
    alg = TIMING_ALGORITHMS[algorithm] if isinstance(algorithm, str) else int(algorithm)
    t = None if taps is None else np.ascontiguousarray(taps, f32)
    p = PulseRxParams(t.ctypes.data if t is not None and t.size else None, t.size if t is not None else 0, alg, decimation, loop_gain, max_error,
                      int(bool(use_q)), gain, n_symbols, int(bool(slice_q)))
    p._taps = t
    return p


def pulserx_debug_walk(params, first="filter", last="slice", x=None, cuts=(), state=None, with_extras=False):
    """CPU run of the receive object's walk for one channel (csdr_amd_debug_pulserx_walk): x cut into calls of `cuts` samples and the rest -> outputs
    (and, with_extras, the timing errors and indexes).  state: a PulseRxChan carried in and out (without a tail on the way in)."""
    f, l = _pulserx_stage(first), _pulserx_stage(last)
    x = np.ascontiguousarray(x, c64)
    n = x.size
    cap = (2 * n // max(params.decimation, 1) + 3 * len(cuts) + 16) * 2
    out = np.zeros(cap, c64 if l == 1 else np.uint8)
    err = np.zeros(cap, f32) if with_extras else None
    idx = np.zeros(cap, np.uint32) if with_extras else None
    cu = np.ascontiguousarray(cuts, np.int64)
    k = lib().csdr_amd_debug_pulserx_walk(C.byref(params), f, l, _hp(x), n, _hp(cu) if cu.size else None, cu.size, _hp(out),
                                          _hp(err) if with_extras else None, _hp(idx) if with_extras else None, C.byref(state) if state is not None else None)
    if k < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return (out[:k], err[:k], idx[:k]) if with_extras else out[:k]


class PulseRx(_Handle, _MaxOut, _ChannelState, _Lanes):
    """csdr_amd_pulserx: pulse_shaping_filter_cc (matched filter) | timing_recovery_cc | [realpart_cf |] gain_ff | generic_slicer_f_u8 for n_channels
    channels, stages first ("filter", "timing") .. last ("timing", "slice"), state kept on the device between calls."""
    _chan = PulseRxChan

    def __init__(self, ctx, params, n_channels=1, first="filter", last="slice"):
        self.n_channels, self.params = n_channels, params
        self.first, self.last = _pulserx_stage(first), _pulserx_stage(last)
        self.in_dtype, self.out_dtype = c64, (c64 if self.last == 1 else np.uint8)
        _Handle.__init__(self, ctx, "pulserx", ctx.L.csdr_amd_pulserx_create(ctx.h, C.byref(params), n_channels, self.first, self.last))

    def process_dev(self, d_in, n_in, in_pitch, d_out, out_pitch, d_counts, d_err=None, d_idx=None):
        """device pointers; counts (n_channels int32) receives each channel's output count.  Asynchronous."""
        self._call("process", d_in, n_in, in_pitch, d_out, out_pitch, d_counts, d_err, d_idx)

    def process(self, x, calls=None, with_extras=False):
        """x: [n_channels, n] (or [n]) host samples; calls: per-call sample counts (default one call) -> a list of per-channel output arrays
        (or one array for 1-D x); with_extras (last == "timing"): (symbols, errors, indexes) per channel."""
        x = np.ascontiguousarray(x, c64)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None]
        s, n = x.shape
        if s != self.n_channels:
            raise ValueError("x has %d rows for %d channels" % (s, self.n_channels))
        calls = [n] if calls is None else list(calls)
        if with_extras:
            res = _counted_calls(self, x, calls, (("d_err", f32), ("d_idx", np.uint32)))
        else:
            res = [r[0] for r in _counted_calls(self, x, calls)]
        return res[0] if squeeze else res


class FrameSyncChan(C.Structure):
    """csdr_amd_framesync_chan: one channel's record (its ring of pattern_length bytes travels beside it)"""
    _fields_ = [("fill", C.c_int), ("index", C.c_int), ("remain", C.c_int), ("reserved", C.c_int), ("base", C.c_longlong), ("frames", C.c_longlong)]

    def astuple(self):
        return (self.fill, self.index, self.remain, self.base, self.frames)


def framesync_debug_walk(pattern, values_after, x, max_mismatch=0, cuts=(), state=None, window=None):
    """CPU run of the frame synchroniser's step function for one channel (csdr_amd_debug_framesync_walk): x cut into calls of `cuts` bytes and the rest ->
    (payload bytes, the index of each payload's first byte).  state: a FrameSyncChan carried in and out, with `window` (pattern_length bytes, updated in
    place) holding its ring."""
    pat = np.ascontiguousarray(pattern, np.uint32)
    x = np.ascontiguousarray(x, np.uint8)
    out = np.zeros(max(x.size, 1), np.uint8)
    pos = np.zeros(x.size + 1, np.int64)
    nf = C.c_longlong(0)
    cu = np.ascontiguousarray(cuts, np.int64)
    if window is not None and (window.dtype != np.uint8 or window.size != pat.size or not window.flags.c_contiguous):
        raise ValueError("window: a contiguous uint8 array of pattern_length bytes")
    k = lib().csdr_amd_debug_framesync_walk(_hp(pat), pat.size, int(values_after), int(max_mismatch), _hp(x), x.size, _hp(cu) if cu.size else None, cu.size,
                                            _hp(out), _hp(pos), C.byref(nf), C.byref(state) if state is not None else None,
                                            _hp(window) if window is not None else None)
    if k < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return out[:k], pos[:nf.value]


def framesync_tile():
    """bytes of a row that k_framesync_tiled stages per step"""
    return int(lib().csdr_amd_framesync_tile())


class FrameSync(_Handle, _MaxOut, _PerChannel, _Lanes):
    """csdr_amd_framesync: pattern_search_u8_u8 (csdr.c:3532-3597) for n_channels byte streams: behind every match of `pattern` (at most max_mismatch
    positions differing) the next values_after bytes come out; state kept on the device between calls."""
    in_dtype = out_dtype = np.uint8

    def __init__(self, ctx, pattern, values_after, n_channels=1, max_mismatch=0):
        self.pattern = np.ascontiguousarray(pattern, np.int64)
        if self.pattern.size and (self.pattern.min() < 0 or self.pattern.max() > 0xffffffff):
            raise ValueError("pattern values are unsigned")
        self.n_channels, self.values_after, self.max_mismatch = int(n_channels), int(values_after), int(max_mismatch)
        pat, h = self.pattern.astype(np.uint32), C.c_void_p(None)
        rc = ctx.L.csdr_amd_framesync_create(ctx.h, self.n_channels, _hp(pat), pat.size, self.values_after, self.max_mismatch, C.byref(h))
        _Handle.__init__(self, ctx, "framesync", h.value if rc == 0 else None)

    def max_frames(self, n_in):
        return int(self._fn("max_frames")(self.h, int(n_in)))

    def get_channel(self, ch):
        """-> (FrameSyncChan, the channel's ring bytes)"""
        st, w = FrameSyncChan(), np.zeros(self.pattern.size, np.uint8)
        self._call("get_channel", int(ch), C.byref(st), _hp(w))
        return st, w

    def set_channel(self, ch, st, window=None):
        w = None if window is None else np.ascontiguousarray(window, np.uint8)
        if w is not None and w.size != self.pattern.size:
            raise ValueError("window holds pattern_length bytes")
        self._call("set_channel", int(ch), C.byref(st), _hp(w) if w is not None else None)

    def process_dev(self, d_in, n_in, in_pitch, d_out, out_pitch, d_counts, d_in_counts=None, d_pos=None, pos_pitch=0, d_frame_counts=None):
        """device pointers; d_counts (n_channels int32) receives each channel's payload bytes of this call, d_in_counts (or None: n_in) gives each
        channel's input bytes, d_pos (int64 rows, pos_pitch apart) and d_frame_counts receive the matches.  Asynchronous."""
        self._call("process", d_in, in_pitch, n_in, d_in_counts, d_out, out_pitch, d_counts, d_pos, pos_pitch, d_frame_counts)

    def process(self, x, counts=None, with_positions=False, calls=None, pitch=None):
        """x: [n_channels, n] (or [n]) host bytes of which channel c takes counts[c] (default n); calls: per-call byte counts (default one call; with counts a
        channel takes what is left of its bytes in each call); pitch: bytes between the rows on the device (default n) -> a list of per-channel payload arrays
        (or one array for 1-D x); with_positions: (payload, positions) per channel."""
        x = np.ascontiguousarray(x, np.uint8)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None]
        s, n = x.shape
        if s != self.n_channels:
            raise ValueError("x has %d rows for %d channels" % (s, self.n_channels))
        ctx = self.ctx
        left = np.full(s, n, np.int64) if counts is None else np.clip(np.asarray(counts, np.int64), 0, n)
        calls = [n] if calls is None else list(calls)
        pitch = max(n, 1) if pitch is None else int(pitch)
        if pitch < n:
            raise ValueError("pitch below the row length")
        rows = np.zeros((s, pitch), np.uint8); rows[:, :n] = x
        di = ctx.upload(rows)
        most = max(calls) if calls else 0
        opitch, fpitch = max(most, 1), self.max_frames(most)
        do, dp = ctx.alloc(opitch * s + 256), ctx.alloc(8 * fpitch * s + 256)
        dc, dfc, dn = ctx.alloc(4 * s + 256), ctx.alloc(4 * s + 256), ctx.alloc(4 * s + 256)
        outs, poss, at = [[] for _ in range(s)], [[] for _ in range(s)], 0
        for k in calls:
            take = np.clip(left - at, 0, k).astype(np.int32)
            self.ctx.check(ctx.L.csdr_amd_h2d(ctx.h, dn.ptr, _hp(take), take.nbytes), "h2d")
            self.process_dev(di.at(at), k, pitch, do.ptr, opitch, dc.ptr, dn.ptr, dp.ptr, fpitch, dfc.ptr)
            cnt, fc = ctx.download(dc, np.int32, s), ctx.download(dfc, np.int32, s)
            y = ctx.download(do, np.uint8, opitch * s).reshape(s, opitch)
            q = ctx.download(dp, np.int64, fpitch * s).reshape(s, fpitch)
            for c in range(s):
                outs[c].append(y[c, :cnt[c]].copy()); poss[c].append(q[c, :fc[c]].copy())
            at += k
        res = [(np.concatenate(o) if o else np.zeros(0, np.uint8), np.concatenate(p) if p else np.zeros(0, np.int64)) for o, p in zip(outs, poss)]
        if not with_positions:
            res = [r[0] for r in res]
        return res[0] if squeeze else res


class RttyParams(C.Structure):
    """csdr_amd_rtty_params"""
    _fields_ = [("spacing", C.c_float), ("filter_length", C.c_int), ("window", C.c_int), ("samples_per_bits", C.c_float), ("databits", C.c_int),
                ("stopbits", C.c_float), ("bit_sampling_width_ratio", C.c_float), ("cli_bufsize", C.c_int)]


class RttyPushState(C.Structure):
    """csdr_amd_rtty_push_state: rtty_baudot_decoder_push's state (zeros: a fresh decoder)"""
    _fields_ = [("fig_mode", C.c_int), ("character_received", C.c_int), ("shr", C.c_int), ("bit_cntr", C.c_int), ("state", C.c_int)]


RTTY_STAGES = {"bfsk": 0, "serial": 1, "baudot": 2}


def rtty_params(spacing=0.02125, filter_length=101, window=1024, samples_per_bits=176.0176, databits=5, stopbits=1.5, bit_sampling_width_ratio=0.4,
                cli_bufsize=16384):
    """the chain's parameters; the defaults are 45.45 Bd at 170 Hz shift and 8 kS/s: `bfsk_demod_cf 0.02125 101 | serial_line_decoder_f_u8 176.0176 5 1.5`"""
    return RttyParams(spacing, filter_length, window, samples_per_bits, databits, stopbits, bit_sampling_width_ratio, cli_bufsize)


def _rtty_stage(s):
    return RTTY_STAGES[s] if isinstance(s, str) else int(s)


def _rtty_types(params, first, last):
    ti = c64 if first == 0 else (f32 if first == 1 else np.uint8)
    if last == 0:
        to = f32
    elif last == 1:
        to = np.uint8 if params.databits <= 8 else (np.uint16 if params.databits <= 16 else np.uint32)
    else:
        to = np.uint8
    return ti, to


def firdes_peak_c(length, rate, window="HAMMING"):
    """firdes_peak_c (csdr.c:2932-2972 / firdes_add_peak_c libcsdr.c:2219-2257, add 0, normalize 1) -> complex64 taps"""
    t = np.zeros(length, c64)
    lib().csdr_amd_firdes_peak_c(_hp(t), int(length), float(rate), WINDOWS[window] if isinstance(window, str) else int(window))
    return t


def rtty_debug_walk(params, first="bfsk", last="baudot", x=None, cuts=()):
    """CPU run of the object's walk for one channel (csdr_amd_debug_rtty_walk): x cut into calls of `cuts` items and the rest -> outputs"""
    f, l = _rtty_stage(first), _rtty_stage(last)
    ti, to = _rtty_types(params, f, l)
    x = np.ascontiguousarray(x, ti)
    n = x.size
    out = np.zeros(n + 16, to)
    cu = np.ascontiguousarray(cuts, np.int64)
    k = lib().csdr_amd_debug_rtty_walk(C.byref(params), f, l, _hp(x), n, _hp(cu) if cu.size else None, cu.size, _hp(out))
    if k < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return out[:k]


def rtty_baudot_decoder_push(state, symbol):
    """rtty_baudot_decoder_push (libcsdr.c:1615-1655) on the host: state (RttyPushState) in and out -> the character or 0"""
    return lib().csdr_amd_rtty_baudot_decoder_push(C.byref(state), int(symbol) & 255)[0]


def rtty_baudot_decoder_lookup(fig_mode, c):
    """rtty_baudot_decoder_lookup (libcsdr.c:1606-1613) -> (character or 0, new fig_mode)"""
    f = C.c_ubyte(fig_mode)
    r = lib().csdr_amd_rtty_baudot_decoder_lookup(C.byref(f), int(c) & 255)[0]
    return r, f.value


class Rtty(_Handle, _MaxOut, _PerChannel):
    """csdr_amd_rtty: the RTTY receive chain (bfsk_demod_cf | serial_line_decoder_f_u8 | rtty_baudot2ascii_u8_u8) for n_channels channels, stages
    first..last ("bfsk", "serial", "baudot"), state kept on the device between calls."""

    def __init__(self, ctx, params=None, n_channels=1, first="bfsk", last="baudot"):
        self.n_channels = n_channels
        self.params = params if params is not None else rtty_params()
        self.first, self.last = _rtty_stage(first), _rtty_stage(last)
        self.in_dtype, self.out_dtype = _rtty_types(self.params, self.first, self.last)
        _Handle.__init__(self, ctx, "rtty", ctx.L.csdr_amd_rtty_create(ctx.h, C.byref(self.params), n_channels, self.first, self.last))

    def process_dev(self, d_in, n_in, in_pitch, d_out, out_pitch, d_counts):
        """device pointers; counts (n_channels int32) receives each channel's output count.  Asynchronous."""
        self._call("process", d_in, n_in, in_pitch, d_out, out_pitch, d_counts)

    def process(self, x, calls=None):
        """x: [n_channels, n] (or [n]) host items; calls: per-call item counts (default one call) -> a list of per-channel output arrays
        (or one array for 1-D x)"""
        x = np.ascontiguousarray(x, self.in_dtype)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None]
        s, n = x.shape
        if s != self.n_channels:
            raise ValueError("x has %d rows for %d channels" % (s, self.n_channels))
        calls = [n] if calls is None else list(calls)
        res = [r[0] for r in _counted_calls(self, x, calls)]
        return res[0] if squeeze else res


def _window(window):
    return WINDOWS[window] if isinstance(window, str) else int(window)


def firdes_peaks_c(length, rates, window="HAMMING"):
    """the taps of peaks_fir_cc (csdr.c:2997-3002): firdes_add_peak_c of every rate into zeroed taps, normalised with the last -> complex64 taps"""
    r = np.ascontiguousarray(np.atleast_1d(rates), f32)
    if int(length) < 1 or r.size < 1:
        raise ValueError("firdes_peaks_c needs length >= 1 and at least one rate")
    t = np.zeros(int(length), c64)
    lib().csdr_amd_firdes_peaks_c(_hp(t), int(length), _hp(r), r.size, _window(window))
    return t


def cfir_debug_walk(taps, x, cuts=()):
    """CPU run of the CFir walk for one channel (csdr_amd_debug_cfir_walk): x cut into calls of `cuts` samples and the rest -> the concatenated outputs"""
    taps = np.ascontiguousarray(taps, c64); x = np.ascontiguousarray(x, c64)
    out = np.zeros(x.size + 16, c64)
    cu = np.ascontiguousarray(cuts, np.int64)
    k = lib().csdr_amd_debug_cfir_walk(_hp(taps) if taps.size else None, taps.size, _hp(x), x.size, _hp(cu) if cu.size else None, cu.size, _hp(out))
    if k < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return out[:k]


def apply_fir_cc(x, taps, ctx=None, force_generic=False):
    """apply_fir_cc (libcsdr.c:2261-2273) on the device: Context.apply_fir_cc on `ctx`, or on a context of device 0 opened for the call"""
    if ctx is not None:
        return ctx.apply_fir_cc(x, taps, force_generic)
    own = Context(0)
    try:
        return own.apply_fir_cc(x, taps, force_generic)
    finally:
        own.close()


class CFir(_Handle, _MaxOut, _PerChannel):
    """csdr_amd_cfir: the complex-tap FIR (apply_fir_cc) for n_channels channels, each with its own taps_length taps (zero until set) and its history on the
    device: the calls' outputs are the valid filter output of each channel's whole stream."""
    in_dtype = out_dtype = c64

    def __init__(self, ctx, n_channels=1, taps_length=101):
        self.n_channels, self.taps_length = n_channels, taps_length
        _Handle.__init__(self, ctx, "cfir", ctx.L.csdr_amd_cfir_create(ctx.h, n_channels, taps_length))

    def set_taps(self, taps, channel=-1):
        """taps: taps_length complex taps for `channel` (-1: every channel), or [n_channels, taps_length] for all of them"""
        taps = np.ascontiguousarray(taps, c64)
        if taps.ndim == 2 and channel == -1:
            if taps.shape != (self.n_channels, self.taps_length):
                raise ValueError("taps should be [%d, %d]" % (self.n_channels, self.taps_length))
            for ch in range(self.n_channels):
                self._call("set_taps", ch, _hp(taps[ch]))
            return
        if taps.shape != (self.taps_length,):
            raise ValueError("taps should be %d complex values" % self.taps_length)
        self._call("set_taps", int(channel), _hp(taps))

    def set_peaks(self, rates, channel=-1, window="HAMMING"):
        """the taps of peaks_fir_cc at `rates` (one or more) for `channel` (-1: every channel)"""
        r = np.ascontiguousarray(np.atleast_1d(rates), f32)
        self._call("set_peaks", int(channel), _hp(r) if r.size else None, r.size, _window(window))

    def process_dev(self, d_in, n_in, in_pitch, d_out, out_pitch, d_counts):
        """device pointers; counts (n_channels int32) receives each channel's output count.  Asynchronous."""
        self._call("process", d_in, n_in, in_pitch, d_out, out_pitch, d_counts)

    def process(self, x, calls=None):
        """x: [n_channels, n] (or [n]) complex samples; calls: per-call sample counts (default one call) -> a list of per-channel output arrays
        (or one array for 1-D x)"""
        x = np.ascontiguousarray(x, c64)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None]
        s, n = x.shape
        if s != self.n_channels:
            raise ValueError("x has %d rows for %d channels" % (s, self.n_channels))
        calls = [n] if calls is None else list(calls)
        res = [r[0] for r in _counted_calls(self, x, calls)]
        return res[0] if squeeze else res


NOISE_KINDS = {"gaussian": 0, "uniform": 1}


def _noise_kind(kind):
    return NOISE_KINDS[kind] if isinstance(kind, str) else int(kind)


def philox4x32_10(ctr, key):
    """Philox4x32-10 of the library (csdr_amd_debug_philox): 4 counter words, 2 key words -> 4 uint32"""
    c = np.ascontiguousarray(ctr, np.uint32); k = np.ascontiguousarray(key, np.uint32); o = np.zeros(4, np.uint32)
    if c.shape != (4,) or k.shape != (2,):
        raise ValueError("philox4x32_10 takes 4 counter words and 2 key words")
    lib().csdr_amd_debug_philox(_hp(c), _hp(k), _hp(o))
    return o


def noise_from_words(kind, words):
    """CPU run of the words-to-samples transform (csdr_amd_debug_noise_words): 2 n words -> n complex Gaussian samples, or n words -> n uniform floats"""
    kind = _noise_kind(kind); w = np.ascontiguousarray(words, np.uint32).reshape(-1)
    n = w.size // 2 if kind == 0 else w.size
    out = np.zeros(n, c64 if kind == 0 else f32)
    if lib().csdr_amd_debug_noise_words(kind, _hp(w), n, _hp(out)) < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return out


def noise_debug_walk(kind, seed, stream_id=0, position=0, n=0, cuts=(), x=None, snr_db=0.0):
    """CPU run of one channel of a Noise object (csdr_amd_debug_noise_walk): samples position .. position + n - 1 of stream `stream_id`, cut into calls of
    `cuts` samples and the rest; with x (Gaussian): awgn_cc of x at snr_db, n = len(x)"""
    kind = _noise_kind(kind)
    if x is not None:
        x = np.ascontiguousarray(x, c64); n = x.size
    out = np.zeros(int(n), c64 if kind == 0 else f32)
    cu = np.ascontiguousarray(cuts, np.int64)
    k = lib().csdr_amd_debug_noise_walk(kind, int(seed), int(stream_id), int(position), int(n), _hp(cu) if cu.size else None, cu.size,
                                        _hp(x) if x is not None else None, float(snr_db), _hp(out))
    if k < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return out


def awgn_gains(snr_db):
    """(a_signal, a_noise * 0.707) of awgn_cc <snr_db> as float32 (csdr.c:3050-3052, :3079)"""
    a, g = C.c_float(0), C.c_float(0)
    lib().csdr_amd_awgn_gains(float(snr_db), C.byref(a), C.byref(g))
    return f32(a.value), f32(g.value)


def awgn_debug_mix(x, noise, snr_db):
    """CPU run of the flat awgn_cc (csdr_amd_debug_awgn_cc): x and the caller's noise at snr_db"""
    x = np.ascontiguousarray(x, c64); noise = np.ascontiguousarray(noise, c64)
    if x.shape != noise.shape or x.ndim != 1:
        raise ValueError("x and noise should be two rows of one length")
    out = np.zeros(x.size, c64)
    if lib().csdr_amd_debug_awgn_cc(_hp(x), _hp(noise), x.size, float(snr_db), _hp(out)) < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return out


def debug_timing_variance(idx, samples_per_symbol, initial_sample_offset):
    """CPU run of normalized_timing_variance_u32_f on one row of sample indexes"""
    idx = np.ascontiguousarray(idx, np.uint32)
    return f32(lib().csdr_amd_debug_timing_variance(_hp(idx) if idx.size else None, idx.size, int(samples_per_symbol), int(initial_sample_offset)))


class Noise(_Handle, _PerChannel):
    """csdr_amd_noise: uniform_noise_f / gaussian_noise_c for n_channels channels and, on a Gaussian object, the fused awgn_cc.  A channel's stream is a
    function of (seed, its stream id, sample index): positions are 64-bit sample indexes, settable per channel."""

    def __init__(self, ctx, n_channels=1, kind="gaussian", seed=0, stream_ids=None, snr_db=None):
        self.n_channels, self.kind, self.seed = int(n_channels), _noise_kind(kind), int(seed)
        self.dtype = c64 if self.kind == 0 else f32
        ids = None if stream_ids is None else np.ascontiguousarray(stream_ids, np.uint32)
        if ids is not None and ids.shape != (self.n_channels,):
            raise ValueError("stream_ids should be %d ids" % self.n_channels)
        _Handle.__init__(self, ctx, "noise", ctx.L.csdr_amd_noise_create(ctx.h, self.n_channels, self.kind, self.seed, _hp(ids) if ids is not None else None))
        if snr_db is not None:
            self.set_snrs(snr_db)

    def force_generic(self, on=True):
        raise CsdrAmdError("noise: one kernel per call form, nothing to force")

    def set_snr_db(self, ch, snr_db):
        self._call("set_snr_db", int(ch), float(snr_db))

    def set_snrs(self, snr_db):
        """one SNR for all channels or n_channels of them, in dB"""
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(snr_db, f32), (self.n_channels,)), f32)
        self._call("set_snrs", _hp(v))

    def get_gains(self, ch):
        a, g = C.c_float(0), C.c_float(0)
        self._call("get_gains", int(ch), C.byref(a), C.byref(g))
        return f32(a.value), f32(g.value)

    def position(self, ch=0):
        p = int(self._fn("position")(self.h, int(ch)))
        if p < 0:
            raise CsdrAmdError(self.ctx.err())
        return p

    def set_position(self, ch, pos):
        self._call("set_position", int(ch), int(pos))

    def generate_dev(self, d_out, n, out_pitch):
        """device pointer; n samples per channel, rows out_pitch items apart.  Asynchronous."""
        self._call("generate", d_out, int(n), int(out_pitch))

    def awgn_cc_dev(self, d_in, n, in_pitch, d_out, out_pitch, d_snr=None):
        self._call("awgn_cc", d_in, int(n), int(in_pitch), d_out, int(out_pitch), d_snr)

    def generate(self, n, out_pitch=None):
        """n samples per channel -> [n_channels, n] (float32 or complex64)"""
        n = int(n); pitch = max(n, 1) if out_pitch is None else int(out_pitch)
        size = self.n_channels * pitch
        do = self.ctx.upload(np.zeros(size, self.dtype))
        self.generate_dev(do.ptr, n, pitch)
        return self.ctx.download(do, self.dtype, size).reshape(self.n_channels, pitch)[:, :n].copy()

    def awgn_cc(self, x, with_snr=False, in_place=False, in_pitch=None, out_pitch=None):
        """x: [n_channels, n] (or [n]) complex samples -> the same shape with each channel's noise added at its SNR; with_snr: also the n_channels SNRs in dB
        that --snrshow would print for this call"""
        x = np.ascontiguousarray(x, c64)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None]
        s, n = x.shape
        if s != self.n_channels:
            raise ValueError("x has %d rows for %d channels" % (s, self.n_channels))
        ip = max(n, 1) if in_pitch is None else int(in_pitch); op = ip if in_place else (max(n, 1) if out_pitch is None else int(out_pitch))
        xi = np.zeros((s, ip), c64); xi[:, :n] = x
        di = self.ctx.upload(xi)
        do = di if in_place else self.ctx.upload(np.zeros(s * op, c64))
        ds = self.ctx.upload(np.zeros(s, f32)) if with_snr else None
        self.awgn_cc_dev(di.ptr, n, ip, do.ptr, op, ds.ptr if ds else None)
        y = self.ctx.download(do, c64, s * op).reshape(s, op)[:, :n].copy()
        y = y[0] if squeeze else y
        return (y, self.ctx.download(ds, f32, s)) if with_snr else y


def squelch_report_due(report_every_nth, block_index):
    """whether block `block_index` (0-based) of squelch_and_smeter_cc reports its power (csdr.c:2224-2229)"""
    return bool(lib().csdr_amd_squelch_report_due(int(report_every_nth), int(block_index)))


def squelch_gate_open(power, level):
    """the gate decision of one block (csdr.c:2230)"""
    return bool(lib().csdr_amd_squelch_gate_open(float(power), float(level)))


def squelch_debug_power(x, decimation=1):
    """the library's power step function on the host (csdr_amd_debug_squelch_power): one block = all of x (complex or real)"""
    cplx = np.iscomplexobj(x)
    x = np.ascontiguousarray(x, c64 if cplx else f32)
    return f32(lib().csdr_amd_debug_squelch_power(_hp(x), x.size, int(decimation), int(cplx)))


class Squelch(_Handle, _PerChannel):
    """csdr_amd_squelch: squelch_and_smeter_cc for n_channels channels in blocks of block_size samples; the samples behind a channel's last whole block
    stay on the device between calls."""

    def __init__(self, ctx, n_channels=1, block_size=1024, use_every_nth=1, levels=None, max_samples_per_call=1 << 22):
        self.n_channels, self.B = n_channels, block_size
        lv = None if levels is None else np.ascontiguousarray(np.broadcast_to(np.asarray(levels, f32), (n_channels,)))
        _Handle.__init__(self, ctx, "squelch", ctx.L.csdr_amd_squelch_create(ctx.h, n_channels, block_size, use_every_nth, None if lv is None else _hp(lv),
                                                                              max_samples_per_call))

    def max_blocks(self):
        return int(self._fn("max_blocks")(self.h))

    def process_dev(self, d_in, n_in, in_pitch, d_out, out_pitch, d_power=None, power_pitch=0, d_flags=None, counts=None):
        """device pointers (power / flags may be None); counts: a host int32 array of n_channels, or None -> the largest block count.  Asynchronous."""
        return self._call("process", d_in, n_in, in_pitch, d_out, out_pitch, d_power, power_pitch, d_flags, None if counts is None else _hp(counts))

    def process(self, x, calls=None, in_pitch=None, out_pitch=None, levels_between=None):
        """x: [n_channels, n] (or [n]) complex samples; calls: per-call sample counts (default one call); in_pitch / out_pitch: row pitches in samples
        (default: the row); levels_between: {call index: [(channel, level), ...]} applied in front of that call
        -> (out, power, flags): per-channel lists of the concatenated blocks, their powers and their open flags (arrays for 1-D x)"""
        x = np.ascontiguousarray(x, c64)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None]
        s, n = x.shape
        if s != self.n_channels:
            raise ValueError("x has %d rows for %d channels" % (s, self.n_channels))
        calls = [n] if calls is None else [int(k) for k in calls]
        ip = n if in_pitch is None else int(in_pitch)
        xin = np.zeros((s, ip), c64)
        xin[:, :n] = x
        di = self.ctx.upload(xin)
        mb = max((max(calls) if calls else 0) // self.B + 1, 1)
        op = mb * self.B if out_pitch is None else int(out_pitch)
        do = self.ctx.alloc(8 * op * s + 256)
        dp = self.ctx.alloc(4 * mb * s + 256)
        df = self.ctx.alloc(mb * s + 256)
        cnt = np.zeros(s, np.int32)
        outs, pws, fls = [[] for _ in range(s)], [[] for _ in range(s)], [[] for _ in range(s)]
        at = 0
        for ci, k in enumerate(calls):
            for ch, lv in (levels_between or {}).get(ci, ()):
                self.set_level(ch, lv)
            self.process_dev(di.at(8 * at), k, ip, do.ptr, op, dp.ptr, mb, df.ptr, cnt)
            y = self.ctx.download(do, c64, op * s).reshape(s, op)
            pw = self.ctx.download(dp, f32, mb * s).reshape(s, mb)
            fl = self.ctx.download(df, np.uint8, mb * s).reshape(s, mb)
            for c in range(s):
                outs[c].append(y[c, :cnt[c] * self.B].copy()); pws[c].append(pw[c, :cnt[c]].copy()); fls[c].append(fl[c, :cnt[c]].copy())
            at += k
        cat = lambda v, dt: [np.concatenate(o) if o else np.zeros(0, dt) for o in v]
        o, p, f = cat(outs, c64), cat(pws, f32), cat(fls, np.uint8)
        return (o[0], p[0], f[0]) if squeeze else (o, p, f)

    def set_level(self, ch, level):
        """takes effect from the next block that a later call starts; ch = -1: all channels"""
        self._call("set_level", int(ch), float(level))

    def get_level(self, ch):
        return float(self._fn("get_level")(self.h, int(ch)))

    def block_index(self, ch=0):
        return int(self._fn("block_index")(self.h, int(ch)))


class CarrierParams(C.Structure):
    """csdr_amd_carrier_params"""
    _fields_ = [("mode", C.c_int), ("alpha", C.c_float), ("beta", C.c_float), ("dphase_max", C.c_float), ("dphase_max_reset_to_zero", C.c_int)]


class CarrierChan(C.Structure):
    """csdr_amd_carrier_chan: one channel's state (nco_phase / output_phase, dphase, current_freq / iir_temp)"""
    _fields_ = [("phase", C.c_float), ("dphase", C.c_float), ("freq", C.c_float)]


CARRIER_MODES = {"costas": 0, "costas_dd": 1, "pll_p": 2, "pll_pi": 3}
CARRIER_OUTPUTS = ("out", "error", "dphase", "nco")


def costas_params(bandwidth, damping=0.707, decision_directed=False, dphase_max_reset_to_zero=False):
    """what init_bpsk_costas_loop_cc (libcsdr.c:2094-2106) stores, as csdr_amd_carrier_params"""
    p = CarrierParams()
    lib().csdr_amd_costas_params(float(bandwidth), float(damping), int(bool(decision_directed)), C.byref(p))
    p.dphase_max_reset_to_zero = int(bool(dphase_max_reset_to_zero))
    return p


def pll_params(pll_type, alpha=0.01, bandwidth=0.01, ko=10.0, kd=0.1, damping=0.707):
    """pll_type 1 / "P": pll_cc_init_p_controller(alpha); 2 / "PI": pll_cc_init_pi_controller(bandwidth, ko, kd, damping) (libcsdr.c:1856-1871)"""
    p = CarrierParams()
    if pll_type in (1, "P", "p"):
        lib().csdr_amd_pll_params_p(float(alpha), C.byref(p))
    elif pll_type in (2, "PI", "pi"):
        lib().csdr_amd_pll_params_pi(float(bandwidth), float(ko), float(kd), float(damping), C.byref(p))
    else:
        raise ValueError("pll_type is 1 (P) or 2 (PI)")
    return p


def _carrier_dtype(name):
    return c64 if name in ("out", "nco") else f32


def carrier_debug_walk(params, x, outputs=CARRIER_OUTPUTS, cuts=(), state=None):
    """CPU run of the kernels' step function for one channel (csdr_amd_debug_carrier_walk): x cut into calls of `cuts` samples and the rest
    -> {name: array} for the names in `outputs`.  state: a CarrierChan carried in and out."""
    x = np.ascontiguousarray(x, c64)
    res = {k: np.zeros(x.size, _carrier_dtype(k)) for k in outputs}
    cu = np.ascontiguousarray(cuts, np.int64)
    ptr = [_hp(res[k]) if k in res else None for k in CARRIER_OUTPUTS]
    rc = lib().csdr_amd_debug_carrier_walk(C.byref(params), _hp(x), x.size, _hp(cu) if cu.size else None, cu.size, *ptr,
                                           C.byref(state) if state is not None else None)
    if rc < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return res


class Carrier(_Handle, _ChannelState, _Lanes):
    """csdr_amd_carrier: bpsk_costas_loop_cc / pll_cc for n_channels channels with shared loop coefficients; each channel's phase, dphase and freq stay
    on the device between calls."""

    _chan = CarrierChan

    def __init__(self, ctx, params, n_channels=1):
        self.n_channels, self.params = n_channels, params
        _Handle.__init__(self, ctx, "carrier", ctx.L.csdr_amd_carrier_create(ctx.h, C.byref(params), n_channels))

    def process_dev(self, d_in, n, in_pitch, d_out=None, d_error=None, d_dphase=None, d_nco=None, out_pitch=0):
        """device pointers, any output may be None but not all.  Asynchronous."""
        self._call("process", d_in, n, in_pitch, d_out, d_error, d_dphase, d_nco, out_pitch)

    def process(self, x, outputs=("out",), calls=None, in_pitch=None, out_pitch=None):
        """x: [n_channels, n] (or [n]) complex samples; outputs: names out of "out", "error", "dphase", "nco"; calls: per-call sample counts (default one
        call); in_pitch / out_pitch: row pitches in samples (default: the row) -> {name: [n_channels, n] array} (1-D arrays for 1-D x)"""
        x = np.ascontiguousarray(x, c64)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None]
        s, n = x.shape
        if s != self.n_channels:
            raise ValueError("x has %d rows for %d channels" % (s, self.n_channels))
        for k in outputs:
            if k not in CARRIER_OUTPUTS:
                raise ValueError("unknown output %r" % (k,))
        calls = [n] if calls is None else [int(k) for k in calls]
        ip = max(n, 1) if in_pitch is None else int(in_pitch)
        op = max(max(calls) if calls else 0, 1) if out_pitch is None else int(out_pitch)
        xin = np.zeros((s, ip), c64)
        xin[:, :n] = x
        di = self.ctx.upload(xin)
        bufs = {k: self.ctx.alloc(np.dtype(_carrier_dtype(k)).itemsize * op * s + 256) for k in outputs}
        res = {k: np.zeros((s, n), _carrier_dtype(k)) for k in outputs}
        at = 0
        for k in calls:
            self.process_dev(di.at(8 * at), k, ip, *[bufs[nm].ptr if nm in bufs else None for nm in CARRIER_OUTPUTS], op)
            for nm in outputs:
                y = self.ctx.download(bufs[nm], _carrier_dtype(nm), op * s).reshape(s, op)
                res[nm][:, at:at + k] = y[:, :k]
            at += k
        return {k: v[0] for k, v in res.items()} if squeeze else res


class ShiftBankChan(C.Structure):
    """csdr_amd_shiftbank_chan: one stream's state"""
    _fields_ = [("rate", C.c_float), ("phase", C.c_float), ("c", C.c_float), ("s", C.c_float), ("pos", C.c_int), ("pending", C.c_int),
                ("old_rate", C.c_float), ("pad", C.c_int)]


SHIFTBANK_FORMATS = {"cf32": 0, "f32": 1}


def shiftbank_debug_walk(variant, rate, x, chunk=1024, aux=0, in_format="cf32", cuts=(), call_rates=None, state=None):
    """CPU run of the shifter bank's step functions for one stream (csdr_amd_debug_shiftbank_walk): x cut into calls of `cuts` samples and the rest -> the
    shifted samples.  call_rates: one entry per call (len(cuts) + 1), a set_rate in front of that call where it is not None / NaN.  state: a ShiftBankChan
    carried in and out."""
    real = SHIFTBANK_FORMATS[in_format] == 1
    x = np.ascontiguousarray(x, f32 if real else c64)
    y = np.zeros(x.size, c64)
    cu = np.ascontiguousarray(cuts, np.int64)
    cr = None
    if call_rates is not None:
        cr = np.array([np.nan if r is None else r for r in call_rates], f32)
        if cr.size != cu.size + 1:
            raise ValueError("call_rates has one entry per call: len(cuts) + 1")
    rc = lib().csdr_amd_debug_shiftbank_walk(SHIFT[variant], float(rate), int(chunk), int(aux), SHIFTBANK_FORMATS[in_format], _hp(x), x.size,
                                             _hp(cu) if cu.size else None, cu.size, _hp(cr) if cr is not None else None, _hp(y),
                                             C.byref(state) if state is not None else None)
    if rc < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return y


def shiftbank_chunk_phases(rate, phase, chunk, n):
    """ADDITION's chunk start phases as the bank's pre-pass steps them, host build (csdr_amd_debug_shiftbank_chunk_phases): the phases after 1 .. n chunks"""
    out = np.zeros(n, f32)
    lib().csdr_amd_debug_shiftbank_chunk_phases(float(rate), float(phase), int(chunk), int(n), _hp(out))
    return out


class ShiftBank(_Handle, _ChannelState):
    """csdr_amd_shiftbank: shift_addition_cc / _fc, shift_math_cc or shift_table_cc for len(rates) streams, each with its own rate; every stream's phase
    state stays on the device between calls and set_rate retunes one stream from the next call on."""

    _chan = ShiftBankChan

    def __init__(self, ctx, variant, rates, chunk=1024, aux=0, in_format="cf32", max_samples_per_call=1 << 20):
        r = np.ascontiguousarray(np.atleast_1d(rates), f32)
        self.n_streams, self.variant, self.real = r.size, variant, SHIFTBANK_FORMATS[in_format] == 1
        _Handle.__init__(self, ctx, "shiftbank", ctx.L.csdr_amd_shiftbank_create(ctx.h, SHIFT[variant], r.size, _hp(r), int(chunk), int(aux),
                                                                                  SHIFTBANK_FORMATS[in_format], int(max_samples_per_call)))

    def process_dev(self, d_in, in_pitch, d_out, out_pitch, n):
        """device pointers; in_pitch in elements, 0: one input row for every stream.  Asynchronous."""
        self._call("process", d_in, in_pitch, d_out, out_pitch, n)

    def process(self, x, calls=None):
        """x: [n_streams, n], or [n]: one row shared by every stream; calls: per-call sample counts (default one call) -> [n_streams, n] complex64"""
        x = np.ascontiguousarray(x, f32 if self.real else c64)
        shared = x.ndim == 1
        n = x.shape[-1]
        if not shared and x.shape[0] != self.n_streams:
            raise ValueError("x has %d rows for %d streams" % (x.shape[0], self.n_streams))
        calls = [n] if calls is None else [int(k) for k in calls]
        s, pitch = self.n_streams, max(n, 1)
        di = self.ctx.upload(x) if n else self.ctx.alloc(256)
        do = self.ctx.alloc(8 * pitch * s + 256)
        at = 0
        for k in calls:
            self.process_dev(di.at(x.itemsize * at), 0 if shared else pitch, do.at(8 * at), pitch, k)
            at += k
        return self.ctx.download(do, c64, pitch * s).reshape(s, pitch)[:, :n]

    def set_rate(self, stream, rate):
        self._call("set_rate", int(stream), float(rate))

    def get_rate(self, stream):
        r = C.c_float(0)
        self._call("get_rate", int(stream), C.byref(r))
        return r.value

    def scans_ahead(self):
        return int(self._fn("scans_ahead")(self.h))


AMSSB_MODES = {"am": 0, "ssb": 1}


def _fftfilt_taps(taps, n_streams):
    """complex64 taps, [taps_length] or [n_streams, taps_length]; ValueError on any other shape (before a device is touched)"""
    taps = np.ascontiguousarray(taps, c64)
    if taps.ndim == 2 and taps.shape[0] != n_streams:
        raise ValueError("taps: %d rows for %d streams" % (taps.shape[0], n_streams))
    if taps.ndim not in (1, 2) or taps.shape[-1] < 1:
        raise ValueError("taps: need [taps_length] or [n_streams, taps_length], got shape %s" % (taps.shape,))
    return taps


class FftFilt(_Handle):
    """csdr_amd_fftfilt: bandpass_fir_fft_cc for n_streams streams, the overlap carried between calls.  taps 1-D: one passband for all streams; 2-D: a passband per
    stream (one-pass path only).  set_stream_taps turns a shared filter per-stream in place."""

    def __init__(self, ctx, fft_size, taps, n_streams=1, max_blocks=1):
        self.taps = _fftfilt_taps(taps, n_streams)
        self.n_streams, self.taps_length = n_streams, self.taps.shape[-1]
        create = ctx.L.csdr_amd_fftfilt_create if self.taps.ndim == 1 else ctx.L.csdr_amd_fftfilt_create_per_stream
        _Handle.__init__(self, ctx, "fftfilt", create(ctx.h, fft_size, _hp(self.taps), self.taps_length, n_streams, max_blocks))
        self.input_size = self._fn("input_size")(self.h)

    def per_stream(self):
        return bool(self._fn("per_stream")(self.h))

    def window(self):
        return self._fn("window")(self.h)

    def _row(self, taps):
        taps = np.ascontiguousarray(taps, c64)
        if taps.ndim != 1:
            raise ValueError("taps: need one row, got shape %s" % (taps.shape,))
        return taps

    def set_taps(self, taps):
        taps = self._row(taps)
        self._call("set_taps", _hp(taps), taps.size)

    def set_stream_taps(self, stream, taps):
        taps = self._row(taps)
        self._call("set_stream_taps", int(stream), _hp(taps), taps.size)

    def process(self, x, calls=None):
        """x: [n_streams, n] complex samples; calls: blocks per call (default: all whole blocks in one call) -> the filtered whole blocks [n_streams, m]"""
        x = np.ascontiguousarray(x, c64)
        s, n = x.shape
        if s != self.n_streams:
            raise ValueError("x has %d rows for %d streams" % (s, self.n_streams))
        inp = self.input_size
        calls = [n // inp] if calls is None else [int(k) for k in calls]
        if sum(calls) * inp > n:
            raise ValueError("%d blocks of %d samples from %d samples" % (sum(calls), inp, n))
        di = self.ctx.upload(x); do = self.ctx.alloc(x.nbytes + 64)
        b = 0
        self.kernels = []                                # the one-pass kernel every call ran ("": the full-size path)
        for k in calls:
            self._call("process", di.at(8 * b * inp), do.at(8 * b * inp), k, n, n)
            self.kernels.append(self.kernel_name())
            b += k
        return self.ctx.download(do, c64, s * n).reshape(s, n)[:, :b * inp].copy()


class AmSsbParams(C.Structure):
    """csdr_amd_amssb_params"""
    _fields_ = [("mode", C.c_int), ("block", C.c_int), ("reference", C.c_float), ("attack_rate", C.c_float), ("decay_rate", C.c_float), ("max_gain", C.c_float),
                ("hang_time", C.c_short), ("attack_wait_time", C.c_short), ("gain_filter_alpha", C.c_float), ("limit_max", C.c_float)]


class AmSsbChan(C.Structure):
    """csdr_amd_amssb_chan: one channel's state (fastdcblock_ff's last_dc_level, agc_ff's last_gain)"""
    _fields_ = [("last_dc", C.c_float), ("last_gain", C.c_float)]


def amssb_params(mode, block=1024, agc=None, limit_max=None):
    """csdr_amd_amssb_params_default for mode "am" / "ssb", then block, agc = (hang_time, reference, attack_rate, decay_rate, max_gain, attack_wait,
    filter_alpha) in `csdr agc_ff`'s argument order, and limit_max where given"""
    p = AmSsbParams()
    if lib().csdr_amd_amssb_params_default(C.byref(p), AMSSB_MODES[mode] if isinstance(mode, str) else int(mode)) < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    p.block = int(block)
    if agc is not None:
        p.hang_time, p.reference, p.attack_rate, p.decay_rate, p.max_gain, p.attack_wait_time, p.gain_filter_alpha = agc
    if limit_max is not None:
        p.limit_max = limit_max
    return p


def amssb_debug_walk(params, x, state=None):
    """CPU run of the kernels' functions for one channel (csdr_amd_debug_amssb_walk): the whole blocks of x -> (s16, pre_agc).  state: an AmSsbChan
    carried in and out."""
    x = np.ascontiguousarray(x, c64)
    nb = x.size // params.block
    s16 = np.zeros(nb * params.block, np.int16); pre = np.zeros(nb * params.block, f32)
    rc = lib().csdr_amd_debug_amssb_walk(C.byref(params), _hp(x), nb, C.byref(state) if state is not None else None, _hp(s16), _hp(pre))
    if rc < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return s16, pre


def amssb_zero_run(params, gain, n):
    """csdr_amd_debug_amssb_zero_run: agc_ff's gain behind n zero samples as the kernels take it -> (gain as float32, the steps taken one by one)"""
    it = C.c_longlong()
    g = lib().csdr_amd_debug_amssb_zero_run(C.byref(params), float(gain), int(n), C.byref(it))
    if n < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return f32(g), it.value


def _passband_list(passbands, n_channels):
    """[(low, high)] * n_channels as floats; ValueError on any other shape (before a device is touched)"""
    pb = np.asarray(passbands, np.float64)
    if pb.ndim != 2 or pb.shape != (n_channels, 2):
        raise ValueError("passbands: need %d (low, high) pairs, got shape %s" % (n_channels, pb.shape))
    return [(float(lo), float(hi)) for lo, hi in pb]


class AmSsb(_Handle, _MaxOut, _ChannelState, _Lanes):
    """csdr_amd_amssb: the AM / SSB receive chain's demodulator and audio tail for n_channels channels; input "cf32" (decimated complex baseband) or "u8"
    (wideband u8 IQ through an owned front end: shift_rate one float or one per channel, decimation, ddc_taps); taps / fft_size: SSB's band-pass filter.
    squelch=True: squelch_and_smeter_cc at the tail's input in blocks of params.block (csdr_amd_amssb_enable_squelch); levels: one level or n_channels (None: 0,
    always open)."""
    _chan = AmSsbChan

    def __init__(self, ctx, params, n_channels=1, in_format="cf32", taps=None, fft_size=0, max_samples_per_call=1 << 20, shift_rate=0.0, decimation=50,
                 ddc_taps=None, passbands=None, window=WINDOWS["HAMMING"], squelch=False, use_every_nth=1, levels=None):
        """passbands: [(low, high), ...], one pair per channel, set (set_passband) on the fresh object; taps still give the length and the channels' start"""
        if passbands is not None:
            passbands = _passband_list(passbands, n_channels)
        self.n_channels, self.params, self.in_format = n_channels, params, in_format
        self.taps = np.ascontiguousarray(taps, c64) if taps is not None else np.zeros(0, c64)
        tp, tn = (_hp(self.taps), self.taps.size) if self.taps.size else (None, 0)
        if in_format == "cf32":
            h = ctx.L.csdr_amd_amssb_create_cf32(ctx.h, C.byref(params), n_channels, tp, tn, fft_size, max_samples_per_call)
        else:
            self.ddc_taps = np.ascontiguousarray(ddc_taps, f32)
            if np.ndim(shift_rate) == 0:
                h = ctx.L.csdr_amd_amssb_create(ctx.h, C.byref(params), n_channels, shift_rate, decimation, _hp(self.ddc_taps), self.ddc_taps.size, tp, tn,
                                                fft_size, max_samples_per_call)
            else:
                rates = np.ascontiguousarray(shift_rate, f32); assert rates.size == n_channels
                h = ctx.L.csdr_amd_amssb_create_rates(ctx.h, C.byref(params), n_channels, _hp(rates), decimation, _hp(self.ddc_taps), self.ddc_taps.size, tp,
                                                      tn, fft_size, max_samples_per_call)
        _Handle.__init__(self, ctx, "amssb", h)
        for ch, (lo, hi) in enumerate(passbands or []):
            self.set_passband(ch, lo, hi, window)
        self.squelch = bool(squelch)
        if squelch:
            lv = None if levels is None else np.ascontiguousarray(np.broadcast_to(np.asarray(levels, f32), (n_channels,)))
            self._call("enable_squelch", int(use_every_nth), None if lv is None else _hp(lv))

    def set_passband(self, ch, low, high, window=WINDOWS["HAMMING"]):
        """channel ch's filter becomes firdes_bandpass_c(low, high) at the object's taps length, from the first sample the filter has not consumed yet"""
        self._call("set_passband", int(ch), float(low), float(high), int(window))

    def get_passband(self, ch):
        """(low, high) as set_passband gave them last; (nan, nan) when the channel's taps came from create or set_channel_taps"""
        lo, hi = C.c_float(), C.c_float()
        self._call("get_passband", int(ch), C.byref(lo), C.byref(hi))
        return lo.value, hi.value

    def set_channel_taps(self, ch, taps):
        taps = np.ascontiguousarray(taps, c64)
        if taps.ndim != 1 or taps.size != self.taps.size:
            raise ValueError("a channel's taps have the object's length (%d), got shape %s" % (self.taps.size, taps.shape))
        self._call("set_channel_taps", int(ch), _hp(taps), taps.size)

    def set_rate(self, ch, rate):
        self._call("set_rate", int(ch), rate)

    def get_rate(self, ch):
        return float(self._fn("get_rate")(self.h, int(ch)))

    def front_end_kernel(self):
        return self._L.csdr_amd_ddc_kernel_name(self._fn("front_end")(self.h)).decode()

    def process_dev(self, d_in, in_pitch, n_in, d_s16, d_pre, out_pitch):
        """device pointers (d_pre may be None) -> the audio samples written per channel.  Asynchronous."""
        return self._call("process", d_in, in_pitch, n_in, d_s16, d_pre, out_pitch)

    # ---- the gate at the tail's input (squelch=True)
    def set_squelch_level(self, ch, level):
        """takes effect from the next block that starts; ch = -1: all channels"""
        self._call("set_squelch_level", int(ch), float(level))

    def get_squelch_level(self, ch):
        v = C.c_float()
        self._call("get_squelch_level", int(ch), C.byref(v))
        return float(v.value)

    def squelch_block_index(self):
        """the blocks completed since the reset"""
        return int(self._call("squelch_block_index"))

    def process_squelched_dev(self, d_in, in_pitch, n_in, d_s16, d_pre, out_pitch, d_power=None, power_pitch=0, d_flags=None):
        """device pointers (d_pre / d_power / d_flags may be None) -> (audio samples written per channel, blocks completed).  Asynchronous."""
        nb = C.c_int()
        got = self._call("process_squelched", d_in, in_pitch, n_in, d_s16, d_pre, out_pitch, d_power, power_pitch, d_flags, C.byref(nb))
        return got, nb.value

    def process_squelched(self, x, calls=None, with_pre=True, in_pitch=None, out_pitch=None, in_offset=0, retunes=None, levels_between=None, generic_calls=None):
        """process on an object with a squelch; levels_between: {call index: [(channel, level), ...]} applied in front of that call; generic_calls: the call
        indices that run under force_generic(True) (None: the object's setting stays) -> (s16, pre_agc or None, counts, power [n_channels, blocks],
        flags [n_channels, blocks], the kernel names of the calls that wrote blocks)"""
        return self.process(x, calls, with_pre, in_pitch, out_pitch, in_offset, retunes, levels_between, generic_calls, True)

    def process(self, x, calls=None, with_pre=True, in_pitch=None, out_pitch=None, in_offset=0, retunes=None, levels_between=None, generic_calls=None, _squelched=False):
        """x: [n_channels, n] complex samples (or [n_channels, 2n] u8 IQ bytes); calls: per-call sample counts (default one call); in_pitch: row pitch in
        samples (bytes for u8); out_pitch in samples; in_offset: bytes by which the input's base is moved off its allocation; retunes: {call index:
        [(channel, rate) or (channel, "bp", low, high) or (channel, "taps", taps), ...]} -> (s16 [n_channels, na], pre_agc [n_channels, na] or None, the counts of the calls)"""
        u8 = self.in_format == "u8"
        x = np.ascontiguousarray(x, np.uint8 if u8 else c64)
        if x.ndim == 1:
            x = x[None]
        s, w = x.shape
        n = w // 2 if u8 else w
        if s != self.n_channels:
            raise ValueError("x has %d rows for %d channels" % (s, self.n_channels))
        calls = [n] if calls is None else [int(k) for k in calls]
        ip = (((w + 127) // 128 * 128) if u8 else max(n, 1)) if in_pitch is None else int(in_pitch)
        xin = np.full((s, ip), 0x80, np.uint8) if u8 else np.zeros((s, ip), c64)
        xin[:, :w] = x
        raw = np.zeros(xin.nbytes + in_offset + 16, np.uint8)
        raw[in_offset:in_offset + xin.nbytes] = xin.view(np.uint8).ravel()
        di = self.ctx.upload(raw)
        op = max(self.max_out(max(calls) if calls else 0), 1) if out_pitch is None else int(out_pitch)
        ds = self.ctx.alloc(2 * op * s + 256); dp = self.ctx.alloc(4 * op * s + 256) if with_pre else None
        outs, pres, counts = [], [], []
        pws, fls, names = [], [], []
        if _squelched:
            pp = op // self.params.block + 1
            dw, dg = self.ctx.alloc(4 * pp * s + 256), self.ctx.alloc(pp * s + 256)
        at = 0
        for ci, k in enumerate(calls):
            self.ctx.check(self.ctx.L.csdr_amd_memset(self.ctx.h, ds.ptr, 0x55, 2 * op * s + 256), "memset")      # (what a call leaves alone is checked below)
            for ch, lv in (levels_between or {}).get(ci, []):
                self.set_squelch_level(ch, lv)
            if generic_calls is not None:
                self.force_generic(ci in generic_calls)
            for ch, r, *more in (retunes or {}).get(ci, []):
                if isinstance(r, str):
                    self.set_passband(ch, *more) if r == "bp" else self.set_channel_taps(ch, *more)
                else:
                    self.set_rate(ch, r)
            if _squelched:
                got, nb = self.process_squelched_dev(di.at(in_offset + (2 if u8 else 8) * at), ip, k, ds.ptr, dp.ptr if with_pre else None, op, dw.ptr, pp, dg.ptr)
                assert nb * self.params.block == got
                pws.append(self.ctx.download(dw, f32, pp * s).reshape(s, pp)[:, :nb].copy())
                fls.append(self.ctx.download(dg, np.uint8, pp * s).reshape(s, pp)[:, :nb].copy())
                if nb:
                    names.append(self.kernel_name())
            else:
                got = self.process_dev(di.at(in_offset + (2 if u8 else 8) * at), ip, k, ds.ptr, dp.ptr if with_pre else None, op)
            counts.append(got)
            y = self.ctx.download(ds, np.int16, op * s).reshape(s, op)
            if np.any(y[:, got:] != 0x5555):
                raise CsdrAmdError("amssb: wrote beyond the %d samples it reported" % got)
            outs.append(y[:, :got].copy())
            if with_pre:
                pres.append(self.ctx.download(dp, f32, op * s).reshape(s, op)[:, :got].copy())
            at += k
        cat = lambda parts, dt: np.concatenate(parts, axis=1) if parts else np.zeros((s, 0), dt)
        if _squelched:
            return cat(outs, np.int16), (cat(pres, f32) if with_pre else None), counts, cat(pws, f32), cat(fls, np.uint8), names
        return cat(outs, np.int16), (cat(pres, f32) if with_pre else None), counts


def fmrx_plan(fill, n_in, taps_length, agc_block):
    """csdr_amd_fmrx_plan (a host function): a call of n_in samples on an object that holds `fill` -> (samples written per channel, samples held afterwards)"""
    ne, nf = C.c_longlong(), C.c_int()
    if lib().csdr_amd_fmrx_plan(int(fill), int(n_in), int(taps_length), int(agc_block), C.byref(ne), C.byref(nf)) < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return ne.value, nf.value


def fmrx_squelch_plan(held, n_in, block):
    """csdr_amd_fmrx_squelch_plan (a host function): a call of n_in samples on a squelched object that holds `held` -> (gated samples handed to the demodulator,
    samples held afterwards)"""
    m, nh = C.c_longlong(), C.c_int()
    if lib().csdr_amd_fmrx_squelch_plan(int(held), int(n_in), int(block), C.byref(m), C.byref(nh)) < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return m.value, nh.value


class FmRx(_Handle, _MaxOut, _PerChannel):
    """csdr_amd_fmrx: fmdemod_quadri_cf | limit_ff | deemphasis_nfm_ff | fastagc_ff | convert_f_s16 for n_channels rows of complex baseband on the device;
    the filter's unconsumed input, the previous sample and the AGC's two blocks stay in the object between calls.  squelch_block > 0: squelch_and_smeter_cc
    in blocks of squelch_block samples in front of every channel (csdr_amd_fmrx_create_squelched); levels: one level or n_channels (None: 0, always open)."""

    def __init__(self, ctx, n_channels, audio_rate=48000, agc_block=1024, reference=1.0, limit=1.0, max_samples_per_call=1 << 16, squelch_block=0, use_every_nth=1,
                 levels=None):
        self.n_channels, self.agc_block, self.taps_length, self.squelch_block = n_channels, agc_block, ctx.nfm_taps(audio_rate).size, squelch_block
        if squelch_block == 0 and use_every_nth == 1 and levels is None:
            h = ctx.L.csdr_amd_fmrx_create(ctx.h, n_channels, audio_rate, agc_block, reference, limit, max_samples_per_call)
        else:
            lv = None if levels is None else np.ascontiguousarray(np.broadcast_to(np.asarray(levels, f32), (max(n_channels, 0),)))
            h = ctx.L.csdr_amd_fmrx_create_squelched(ctx.h, n_channels, audio_rate, agc_block, reference, limit, max_samples_per_call, squelch_block, use_every_nth,
                                                     None if lv is None else _hp(lv))
        _Handle.__init__(self, ctx, "fmrx", h)

    def max_output(self, n_in):
        return int(self._fn("max_output")(self.h, int(n_in)))

    def fill(self):
        """the filter input the object holds, per channel"""
        return int(self._fn("fill")(self.h))

    def process_dev(self, d_in, in_pitch, n_in, d_s16, d_f, out_pitch):
        """device pointers (d_s16 / d_f may be None), pitches in elements -> the audio samples written per channel.  Asynchronous."""
        return self._call("process", d_in, in_pitch, n_in, d_s16, d_f, out_pitch)

    def process(self, x, with_float=False, in_pitch=None, out_pitch=None, in_offset=0, with_s16=True):
        """One call.  x: [n_channels, n] (or [n]) complex samples; in_pitch / out_pitch: row pitches in samples (default: the row, the input's rounded up to even); in_offset: bytes by which the input's base is
        moved off its allocation -> (s16 [n_channels, count], count), with the float audio [n_channels, count] in between when with_float; with_s16=False:
        no s16 row is asked for and the first entry is None."""
        x = np.ascontiguousarray(x, c64)
        if x.ndim == 1:
            x = x[None]
        s, n = x.shape
        if s != self.n_channels:
            raise ValueError("x has %d rows for %d channels" % (s, self.n_channels))
        ip = max((n + 1) & ~1, 2) if in_pitch is None else int(in_pitch)      # (default: the row, rounded up to the even pitch the one-kernel path needs)
        xin = np.zeros((s, ip), c64)
        xin[:, :n] = x
        raw = np.zeros(xin.nbytes + in_offset + 16, np.uint8)
        raw[in_offset:in_offset + xin.nbytes] = xin.view(np.uint8).ravel()
        di = self.ctx.upload(raw)
        op = max(self.max_output(n), 1) if out_pitch is None else int(out_pitch)
        ds = self.ctx.alloc(2 * op * s + 256) if with_s16 else None
        df = self.ctx.alloc(4 * op * s + 256) if with_float else None
        got = self.process_dev(di.at(in_offset), ip, n, ds.ptr if ds else None, df.ptr if df else None, op)
        pcm = self.ctx.download(ds, np.int16, op * s).reshape(s, op)[:, :got].copy() if ds else None
        if with_float:
            return pcm, self.ctx.download(df, f32, op * s).reshape(s, op)[:, :got].copy(), got
        return pcm, got

    # ---- the squelch in front (squelch_block > 0)
    def set_squelch_level(self, ch, level):
        """takes effect from the next block that starts; ch = -1: all channels"""
        self._call("set_squelch_level", int(ch), float(level))

    def get_squelch_level(self, ch):
        v = C.c_float()
        self._call("get_squelch_level", int(ch), C.byref(v))
        return float(v.value)

    def squelch_held(self):
        """the samples per channel that wait for their squelch block to complete"""
        return self._call("squelch_held")

    def squelch_block_index(self):
        """the squelch blocks completed since the reset"""
        return int(self._call("squelch_block_index"))

    def process_squelched_dev(self, d_in, in_pitch, n_in, d_s16, d_f, out_pitch, d_power=None, power_pitch=0, d_flags=None):
        """device pointers (d_s16 / d_f / d_power / d_flags may be None), pitches in elements -> (audio samples written per channel, squelch blocks completed).
        Asynchronous."""
        nb = C.c_int()
        got = self._call("process_squelched", d_in, in_pitch, n_in, d_s16, d_f, out_pitch, d_power, power_pitch, d_flags, C.byref(nb))
        return got, nb.value

    def process_squelched(self, x, with_float=False, in_pitch=None, out_pitch=None, in_offset=0, with_s16=True, power_pitch=None):
        """One call, as process -> (s16 [n_channels, count], [float audio,] count, power [n_channels, blocks], flags [n_channels, blocks]): the powers and the open
        flags of the squelch blocks the call completed."""
        x = np.ascontiguousarray(x, c64)
        if x.ndim == 1:
            x = x[None]
        s, n = x.shape
        if s != self.n_channels:
            raise ValueError("x has %d rows for %d channels" % (s, self.n_channels))
        ip = max((n + 1) & ~1, 2) if in_pitch is None else int(in_pitch)
        xin = np.zeros((s, ip), c64)
        xin[:, :n] = x
        raw = np.zeros(xin.nbytes + in_offset + 16, np.uint8)
        raw[in_offset:in_offset + xin.nbytes] = xin.view(np.uint8).ravel()
        di = self.ctx.upload(raw)
        op = max(self.max_output(n), 1) if out_pitch is None else int(out_pitch)
        pp = n // max(self.squelch_block, 1) + 1 if power_pitch is None else int(power_pitch)
        ds = self.ctx.alloc(2 * op * s + 256) if with_s16 else None
        df = self.ctx.alloc(4 * op * s + 256) if with_float else None
        dp, dg = self.ctx.alloc(4 * pp * s + 256), self.ctx.alloc(pp * s + 256)
        got, nb = self.process_squelched_dev(di.at(in_offset), ip, n, ds.ptr if ds else None, df.ptr if df else None, op, dp.ptr, pp, dg.ptr)
        pcm = self.ctx.download(ds, np.int16, op * s).reshape(s, op)[:, :got].copy() if ds else None
        power = self.ctx.download(dp, f32, pp * s).reshape(s, pp)[:, :nb].copy()
        flags = self.ctx.download(dg, np.uint8, pp * s).reshape(s, pp)[:, :nb].copy()
        if with_float:
            return pcm, self.ctx.download(df, f32, op * s).reshape(s, op)[:, :got].copy(), got, power, flags
        return pcm, got, power, flags


def wfmrx_plan(rate, num_poly_points, taps_length, window, where, held, n_in):
    """csdr_amd_wfmrx_plan (a host function): a call of n_in samples on an object that holds `held` demodulated samples at position `where`
    -> (samples written per channel, where afterwards, samples held afterwards)"""
    no, nw, nh = C.c_longlong(), C.c_float(), C.c_int()
    if lib().csdr_amd_wfmrx_plan(float(rate), int(num_poly_points), int(taps_length), int(window), float(where), int(held), int(n_in), C.byref(no), C.byref(nw), C.byref(nh)) < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return no.value, nw.value, nh.value


def wfmrx_squelch_plan(held, n_in, block):
    """csdr_amd_wfmrx_squelch_plan (a host function): a call of n_in samples on a squelched object that holds `held` -> (gated samples handed to the demodulator,
    samples held afterwards)"""
    m, nh = C.c_longlong(), C.c_int()
    if lib().csdr_amd_wfmrx_squelch_plan(int(held), int(n_in), int(block), C.byref(m), C.byref(nh)) < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return m.value, nh.value


class WfmRx(_Handle, _MaxOut, _PerChannel):
    """csdr_amd_wfmrx: fmdemod_quadri_cf | fractional_decimator_ff | deemphasis_wfm_ff | convert_f_s16 for n_channels rows of complex baseband on the device;
    the decimator's unprocessed samples and position, the previous sample and the de-emphasis state stay in the object between calls.  squelch_block > 0:
    squelch_and_smeter_cc in blocks of squelch_block samples in front of every channel (csdr_amd_wfmrx_create_squelched); levels: one level or n_channels
    (None: 0, always open).  plan() then applies to the gated samples wfmrx_squelch_plan hands on."""

    def __init__(self, ctx, n_channels, rate=5, num_poly_points=12, prefilter_taps=None, window=1024, tau=50e-6, audio_rate=48000, max_samples_per_call=1 << 16,
                 squelch_block=0, use_every_nth=1, levels=None):
        taps = None if prefilter_taps is None else np.ascontiguousarray(prefilter_taps, f32)
        self.n_channels, self.rate, self.num_poly_points, self.window = n_channels, float(f32(rate)), num_poly_points, window or 1024
        self.taps_length, self.squelch_block = 0 if taps is None else taps.size, squelch_block
        tp = taps.ctypes.data if taps is not None else None
        if squelch_block == 0 and use_every_nth == 1 and levels is None:
            h = ctx.L.csdr_amd_wfmrx_create(ctx.h, n_channels, rate, num_poly_points, tp, self.taps_length, window, tau, audio_rate, max_samples_per_call)
        else:
            lv = None if levels is None else np.ascontiguousarray(np.broadcast_to(np.asarray(levels, f32), (max(n_channels, 0),)))
            h = ctx.L.csdr_amd_wfmrx_create_squelched(ctx.h, n_channels, rate, num_poly_points, tp, self.taps_length, window, tau, audio_rate, max_samples_per_call,
                                                      squelch_block, use_every_nth, None if lv is None else _hp(lv))
        _Handle.__init__(self, ctx, "wfmrx", h)

    # ---- the squelch in front (squelch_block > 0): FmRx's methods, which reach the library through the object's own prefix
    set_squelch_level, get_squelch_level = FmRx.set_squelch_level, FmRx.get_squelch_level
    squelch_held, squelch_block_index = FmRx.squelch_held, FmRx.squelch_block_index
    process_squelched_dev, process_squelched = FmRx.process_squelched_dev, FmRx.process_squelched

    def max_output(self, n_in):
        return int(self._fn("max_output")(self.h, int(n_in)))

    def held(self):
        """the demodulated samples the object holds, per channel"""
        return int(self._fn("held")(self.h))

    def where(self):
        """the decimator's position in front of the first held sample"""
        return float(self._fn("where")(self.h))

    def plan(self, n_in):
        """wfmrx_plan for the next call of n_in samples"""
        return wfmrx_plan(self.rate, self.num_poly_points, self.taps_length, self.window, self.where(), self.held(), n_in)

    def process_dev(self, d_in, in_pitch, n_in, d_s16, d_f, out_pitch):
        """device pointers (d_s16 / d_f may be None), pitches in elements -> the audio samples written per channel.  Asynchronous."""
        return self._call("process", d_in, in_pitch, n_in, d_s16, d_f, out_pitch)

    def process(self, x, with_float=False, in_pitch=None, out_pitch=None, in_offset=0, with_s16=True):
        """One call.  x: [n_channels, n] (or [n]) complex samples; in_pitch / out_pitch: row pitches in samples (default: the row, the input's rounded up to even);
        in_offset: bytes by which the input's base is moved off its allocation -> (s16 [n_channels, count], count), with the float audio [n_channels, count] in
        between when with_float; with_s16=False: no s16 row is asked for and the first entry is None."""
        x = np.ascontiguousarray(x, c64)
        if x.ndim == 1:
            x = x[None]
        s, n = x.shape
        if s != self.n_channels:
            raise ValueError("x has %d rows for %d channels" % (s, self.n_channels))
        ip = max((n + 1) & ~1, 2) if in_pitch is None else int(in_pitch)
        xin = np.zeros((s, ip), c64)
        xin[:, :n] = x
        raw = np.zeros(xin.nbytes + in_offset + 16, np.uint8)
        raw[in_offset:in_offset + xin.nbytes] = xin.view(np.uint8).ravel()
        di = self.ctx.upload(raw)
        op = max(self.max_output(n), 1) if out_pitch is None else int(out_pitch)
        ds = self.ctx.alloc(2 * op * s + 256) if with_s16 else None
        df = self.ctx.alloc(4 * op * s + 256) if with_float else None
        got = self.process_dev(di.at(in_offset), ip, n, ds.ptr if ds else None, df.ptr if df else None, op)
        pcm = self.ctx.download(ds, np.int16, op * s).reshape(s, op)[:, :got].copy() if ds else None
        if with_float:
            return pcm, self.ctx.download(df, f32, op * s).reshape(s, op)[:, :got].copy(), got
        return pcm, got


TX_MODES = {"fm": 0, "am": 1, "dsb": 2}
TX_FORMATS = {"cf32": 0, "u8": 1}


def fmmod_debug_walk(x, cuts=(), state=0.0, want_out=False):
    """CPU run of fmmod_fc's phase step function for one stream (csdr_amd_debug_fmmod_walk): x cut into calls of `cuts` samples and the rest
    -> (phase after every sample, last_phase[, outputs])"""
    x = np.ascontiguousarray(x, f32)
    ph = np.zeros(x.size, f32)
    out = np.zeros(x.size, c64) if want_out else None
    cu = np.ascontiguousarray(cuts, np.int64)
    st = C.c_float(state)
    rc = lib().csdr_amd_debug_fmmod_walk(_hp(x), x.size, _hp(cu) if cu.size else None, cu.size, _hp(ph), _hp(out) if want_out else None, C.byref(st))
    if rc < 0:
        raise CsdrAmdError(lib().csdr_amd_last_error().decode())
    return (ph, np.float32(st.value), out) if want_out else (ph, np.float32(st.value))


class TxBank(_Handle, _MaxOut):
    """csdr_amd_txbank: convert_s16_f | gain_ff | fmmod_fc or dsb_fc [| add_dcoffset_cc] | fir_interpolate_cc | shift_addition_cc [| convert_f_u8] for
    n_streams s16 audio streams, each with its own shift rate; FM phase, interpolator history and rotator phase stay on the device between calls."""

    def __init__(self, ctx, n_streams, mode, interpolation, taps, rates, gain=1.0, q_value=0.0, out_format="cf32", max_in_samples=1 << 16):
        self.n_streams, self.I, self.fmt = n_streams, interpolation, out_format
        self.taps = np.ascontiguousarray(taps, f32)
        rates = np.ascontiguousarray(rates, f32)
        if rates.size != n_streams:
            raise ValueError("%d rates for %d streams" % (rates.size, n_streams))
        self.max_in = int(max_in_samples)
        _Handle.__init__(self, ctx, "txbank", ctx.L.csdr_amd_txbank_create(ctx.h, n_streams, TX_MODES[mode], gain, q_value, interpolation, _hp(self.taps),
                                                                            self.taps.size, _hp(rates), TX_FORMATS[out_format], self.max_in))

    def process_dev(self, d_in, in_pitch, n_in, d_out, out_pitch):
        """device pointers, pitches in samples -> outputs per stream.  Asynchronous."""
        no = C.c_longlong(0)
        self._call("process", d_in, in_pitch, n_in, d_out, out_pitch, C.byref(no))
        return no.value

    def process(self, x, calls=None, out_pitch=None, out_byte_offset=0):
        """x: [n_streams, n] (or [n]) int16; calls: per-call sample counts (default one call); out_pitch: the output row pitch in samples (default: a
        multiple of 8 that holds the largest call); out_byte_offset shifts the output pointer -> [n_streams, n_out] complex64, or [n_streams, n_out, 2] uint8"""
        x = np.ascontiguousarray(x, np.int16)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None]
        s, n = x.shape
        if s != self.n_streams:
            raise ValueError("x has %d rows for %d streams" % (s, self.n_streams))
        calls = [n] if calls is None else [int(k) for k in calls]
        esz, dt = (2, np.uint8) if self.fmt == "u8" else (8, f32)
        op = ((max(self.max_out(max(calls)) if calls else 0, 1) + 7) & ~7) if out_pitch is None else int(out_pitch)
        di = self.ctx.upload(np.concatenate([x.ravel(), np.zeros(8, np.int16)]))
        do = self.ctx.alloc(esz * op * s + 256)
        parts, at = [], 0
        for k in calls:
            no = self.process_dev(di.at(2 * at), n, k, do.at(out_byte_offset), op)
            y = self.ctx.download(do, dt, (esz // dt().itemsize) * op * s, out_byte_offset).reshape(s, op, -1)
            parts.append(y[:, :no].copy())
            at += k
        y = np.concatenate(parts, axis=1) if parts else np.zeros((s, 0, 2), dt)
        if self.fmt != "u8":
            y = np.ascontiguousarray(y).view(c64)[:, :, 0]
        return y[0] if squeeze else y

    def set_rate(self, stream, rate):
        self._call("set_rate", int(stream), float(rate))

    def get_rate(self, stream):
        return float(self._fn("get_rate")(self.h, int(stream)))


class Interpolator(_Resampling):
    """csdr_amd_interp: fir_interpolate_cc (libcsdr.c:579-605) by `interpolation` for n_streams complex streams."""
    _dt, _eb = c64, 8

    def __init__(self, ctx, interpolation, taps, n_streams=1, bufsize=None):
        self.I, self.n_streams = interpolation, n_streams
        self.taps = np.ascontiguousarray(taps, f32)
        _Handle.__init__(self, ctx, "interp", ctx.L.csdr_amd_interp_create(ctx.h, interpolation, _hp(self.taps), self.taps.size, n_streams))
        if bufsize:
            self.set_cli_bufsize(bufsize)


class Context:
    """csdr_amd_ctx: one GPU, one HIP stream."""

    def __init__(self, device=0, hip_stream=None):
        self.L = lib()
        self.h = self.L.csdr_amd_ctx_create(device, hip_stream)
        if not self.h:
            raise CsdrAmdError("csdr_amd_ctx_create failed: " + self.L.csdr_amd_last_error().decode())
        self.last_ddc_kernels = ""; self.ddc_kernels_seen = set()      # fastddc_inv_cc / fastddc_bank: _note_ddc_call

    def err(self):
        return self.L.csdr_amd_last_error().decode()

    def check(self, rc, what=""):
        if rc < 0:
            raise CsdrAmdError("%s failed (%d): %s" % (what, rc, self.err()))
        return rc

    def close(self):
        if self.h:
            self.L.csdr_amd_ctx_destroy(self.h)
            self.h = None

    def sync(self):
        self.check(self.L.csdr_amd_ctx_sync(self.h), "sync")

    def arch(self):
        return self.L.csdr_amd_device_arch(self.h).decode()

    def alloc(self, nbytes):
        return DevBuf(self, nbytes)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        b = DevBuf(self, arr.nbytes)
        if arr.nbytes:
            self.check(self.L.csdr_amd_h2d(self.h, b.ptr, _hp(arr), arr.nbytes), "h2d")
        return b

    def download(self, buf, dtype, count, byte_offset=0):
        out = np.empty(count, dtype=dtype)
        if out.nbytes:
            self.check(self.L.csdr_amd_d2h(self.h, _hp(out), buf.at(byte_offset), out.nbytes), "d2h")
        return out

    def timer_start(self):
        self.check(self.L.csdr_amd_timer_start(self.h), "timer_start")

    def timer_stop_ms(self):
        ms = C.c_float(0)
        self.check(self.L.csdr_amd_timer_stop_ms(self.h, C.byref(ms)), "timer_stop")
        return ms.value

    # ------------------------------------------------------------------ host-side design
    def firdes_filter_len(self, tbw):
        return self.L.csdr_amd_firdes_filter_len(tbw)

    def firdes_lowpass_f(self, length, cutoff, window="HAMMING"):
        t = np.zeros(length, f32); self.L.csdr_amd_firdes_lowpass_f(_hp(t), length, cutoff, WINDOWS[window]); return t

    def firdes_bandpass_c(self, length, lo, hi, window="HAMMING"):
        t = np.zeros(length, c64); self.L.csdr_amd_firdes_bandpass_c(_hp(t), length, lo, hi, WINDOWS[window]); return t

    def nfm_taps(self, sample_rate):
        p = C.c_void_p()
        n = self.L.csdr_amd_nfm_deemph_taps(sample_rate, C.byref(p))
        if not n:
            return np.zeros(0, f32)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), (n,)).copy()

    # ------------------------------------------------------------------ numpy conveniences (single call, 2-D batches)
    def _conv(self, name, x, in_dt, out_dt, n_out=None, extra=()):
        x = np.ascontiguousarray(x, in_dt)
        n = x.size if in_dt != np.uint8 or name != "csdr_amd_convert_s24_f" else x.size // 3
        n_out = n if n_out is None else n_out
        di = self.upload(np.concatenate([x.ravel(), np.zeros(16, in_dt)]))
        do = self.alloc(np.dtype(out_dt).itemsize * (n_out + 16))
        self.check(getattr(self.L, name)(self.h, di.ptr, do.ptr, n, *extra), name)
        return self.download(do, out_dt, n_out)

    def convert_u8_f(self, x): return self._conv("csdr_amd_convert_u8_f", x, np.uint8, f32)
    def convert_s8_f(self, x): return self._conv("csdr_amd_convert_s8_f", x, np.int8, f32)
    def convert_s16_f(self, x): return self._conv("csdr_amd_convert_s16_f", x, np.int16, f32)
    def convert_f_u8(self, x): return self._conv("csdr_amd_convert_f_u8", x, f32, np.uint8)
    def convert_f_s8(self, x): return self._conv("csdr_amd_convert_f_s8", x, f32, np.int8)
    def convert_f_s16(self, x): return self._conv("csdr_amd_convert_f_s16", x, f32, np.int16)

    def convert_f_s24(self, x, bigendian=0):
        x = np.ascontiguousarray(x, f32)
        return self._conv("csdr_amd_convert_f_s24", x, f32, np.uint8, n_out=3 * x.size, extra=(int(bigendian),))

    def convert_s24_f(self, x, bigendian=0):
        x = np.ascontiguousarray(x, np.uint8)
        return self._conv("csdr_amd_convert_s24_f", x, np.uint8, f32, n_out=x.size // 3, extra=(int(bigendian),))

    @staticmethod
    def _2d(x, dt):
        x = np.ascontiguousarray(x, dt)
        return (x[None, :], True) if x.ndim == 1 else (x, False)

    PAD = -7.5                                           # what _rows writes between and around the rows: a call must leave it alone

    def _rows(self, x2, pitch, offset, dt):
        """x2 [streams, n] as rows of `pitch` elements that start `offset` elements into a buffer filled with PAD -> (DevBuf, elements)"""
        s, n = x2.shape
        assert pitch >= n and offset >= 0
        flat = np.full(offset + s * pitch + 8, self.PAD, dt)
        flat[offset:offset + s * pitch].reshape(s, pitch)[:, :n] = x2
        return self.upload(flat), flat.size

    def shift_cc(self, x, rate, variant="addition", phase=0.0, chunk=1024, aux=0, in_pitch=None, out_pitch=None, in_offset=0, out_offset=0,
                 in_place=False, full=False):
        """x: [n] or [streams, n] complex64 -> (shifted, new_phase).  in_pitch / out_pitch: elements from row to row (default n); in_offset / out_offset:
        elements the first row starts into its buffer (an odd one takes the pointer off 16 bytes); in_place: the output over the input, at its pitch and
        offset.  full: returns the whole output buffer instead, flat, PAD wherever the call wrote nothing."""
        x2, squeeze = self._2d(x, c64)
        s, n = x2.shape
        ip = n if in_pitch is None else int(in_pitch)
        op, oo = (ip, in_offset) if in_place else (n if out_pitch is None else int(out_pitch), out_offset)
        di = self._rows(x2, ip, in_offset, c64)[0]
        total =oo + s * op + 8
        do = di if in_place else self.upload(np.full(total, self.PAD, c64)) if full else self.alloc(8 * total)
        ph = C.c_float(phase)
        self.check(self.L.csdr_amd_shift_cc(self.h, SHIFT[variant], rate, C.byref(ph), di.at(8 * in_offset), do.at(8 * oo), s, n, ip, op, chunk, aux), "shift_cc")
        flat = self.download(do, c64, total)
        if full:
            return flat, ph.value
        y = flat[oo:oo + s * op].reshape(s, op)[:, :n].copy()
        return (y[0] if squeeze else y), ph.value

    def rotator(self, variant, rate, phase, n, chunk=1024, aux=0):
        """csdr_amd_rotator_generate -> (rot [n] complex64 as the device wrote it, the phase after n samples)"""
        rot = self.upload(np.full(n + 8, self.PAD, c64))
        ph = C.c_float(phase)
        self.check(self.L.csdr_amd_rotator_generate(self.h, SHIFT[variant], rate, C.byref(ph), rot.ptr, n, chunk, aux), "rotator")
        got = self.download(rot, c64, n + 8)
        assert np.all(got[n:] == c64(self.PAD)), "rotator_generate wrote past n"
        return got[:n].copy(), ph.value

    def shift_scans_ahead(self):
        """the calls of shift_math_cc / shift_table_cc on this context that found their phase scan done (csdr_amd_debug_shift_scans_ahead)"""
        return int(self.L.csdr_amd_debug_shift_scans_ahead(self.h))

    def mix_fc(self, x, rot, in_pitch=None, out_pitch=None, full=False):
        """csdr_amd_mix_fc: x [n] or [streams, n] float32 times rot [n] complex64 -> [streams, n] complex64 (full: the whole output buffer, flat)"""
        x2, squeeze = self._2d(x, f32); rot = np.ascontiguousarray(rot, c64)
        s, n = x2.shape; assert rot.size == n
        ip, op = n if in_pitch is None else int(in_pitch), n if out_pitch is None else int(out_pitch)
        total = s * op + 8
        di = self._rows(x2, ip, 0, f32)[0]; do = self.upload(np.full(total, self.PAD, c64)); dr = self.upload(rot)
        self.check(self.L.csdr_amd_mix_fc(self.h, di.ptr, do.ptr, dr.ptr, s, n, ip, op), "mix_fc")
        flat = self.download(do, c64, total)
        if full:
            return flat
        y = flat[:s * op].reshape(s, op)[:, :n].copy()
        return y[0] if squeeze else y

    # the reference's own names for the five shifter variants (libcsdr.h:108, 185-207; libcsdr_gpl.h:32-35), CLI chunking included
    def shift_addition_cc(self, x, rate, chunk=1024, phase=0.0): return self.shift_cc(x, rate, "addition", phase, chunk)
    def shift_math_cc(self, x, rate, phase=0.0): return self.shift_cc(x, rate, "math", phase)
    def shift_addfast_cc(self, x, rate, chunk=1024, phase=0.0): return self.shift_cc(x, rate, "addfast", phase, chunk)
    def shift_unroll_cc(self, x, rate, size=1024, phase=0.0): return self.shift_cc(x, rate, "unroll", phase, size, size)
    def shift_table_cc(self, x, rate, table_size=65536, phase=0.0): return self.shift_cc(x, rate, "table", phase, 1024, table_size)

    def shift_addition_fc(self, x, rate, phase=0.0, chunk=1024):
        x = np.ascontiguousarray(x, f32); n = x.size
        di = self.upload(x); do = self.alloc(8 * n + 64); rot = self.alloc(8 * n + 64)
        ph = C.c_float(phase)
        self.check(self.L.csdr_amd_rotator_generate(self.h, 0, rate, C.byref(ph), rot.ptr, n, chunk, 0), "rotator")
        self.check(self.L.csdr_amd_mix_fc(self.h, di.ptr, do.ptr, rot.ptr, 1, n, n, n), "mix_fc")
        return self.download(do, c64, n), ph.value

    def decimating_shift_addition_cc(self, x, rate, decimation, status=(0, 0.0, 0), in_pitch=None, out_pitch=None, full=False):
        """x [n] complex64, one rate, one status (remain, phase, produced) -> (y, status); or x [streams, n], a rate and a status per stream ->
        ([streams] arrays, [streams] statuses), with in_pitch / out_pitch elements from row to row (full: the whole output buffer as well, flat)"""
        if np.ndim(x) == 2:
            x2 = np.ascontiguousarray(x, c64); s, n = x2.shape
            rates = np.ascontiguousarray(rate, f32); assert rates.size == s and len(status) == s
            ip, op = n if in_pitch is None else int(in_pitch), n // decimation + 4 if out_pitch is None else int(out_pitch)
            assert op >= (n + decimation - 1) // decimation
            dsa = np.zeros((s, 3), f32); st = np.zeros((s, 3), np.int32)
            for k in range(s):
                self.L.csdr_amd_shift_addition_init(rates[k] * f32(decimation), _hp(dsa[k]))
                st[k] = (status[k][0], np.array([status[k][1]], f32).view(np.int32)[0], status[k][2])
            total = s * op + 8
            di = self._rows(x2, ip, 0, c64)[0]; do = self.upload(np.full(total, self.PAD, c64)); dd = self.upload(dsa); ds = self.upload(st)
            self.check(self.L.csdr_amd_decimating_shift_addition_cc(self.h, di.ptr, do.ptr, s, n, ip, op, dd.ptr, decimation, ds.ptr), "dsa")
            st = self.download(ds, np.int32, 3 * s).reshape(s, 3); flat = self.download(do, c64, total)
            ys = [flat[k * op:k * op + int(st[k, 2])].copy() for k in range(s)]
            sts = [(int(st[k, 0]), float(st[k, 1:2].view(f32)[0]), int(st[k, 2])) for k in range(s)]
            return (ys, sts, flat) if full else (ys, sts)
        x = np.ascontiguousarray(x, c64); n = x.size
        dsa = np.zeros(3, f32); self.L.csdr_amd_shift_addition_init(np.float32(rate) * np.float32(decimation), _hp(dsa))
        st = np.zeros(3, np.int32); st[0] = status[0]; st[1] = np.array([status[1]], f32).view(np.int32)[0]; st[2] = status[2]
        di = self.upload(x); do = self.alloc(8 * (n // decimation + 4)); dd = self.upload(dsa); ds = self.upload(st)
        self.check(self.L.csdr_amd_decimating_shift_addition_cc(self.h, di.ptr, do.ptr, 1, n, n, n // decimation + 4, dd.ptr, decimation, ds.ptr), "dsa")
        st = self.download(ds, np.int32, 3)
        y = self.download(do, c64, int(st[2]))
        return y, (int(st[0]), float(st[1:2].view(f32)[0]), int(st[2]))

    def fir_decimate_cc(self, x, decimation, taps):
        x2, squeeze = self._2d(x, c64); taps = np.ascontiguousarray(taps, f32)
        s, n = x2.shape
        opitch = n // max(int(decimation), 1) + 2
        di = self.upload(x2); dt = self.upload(taps); do = self.alloc(8 * s * opitch + 64)
        no = self.check(self.L.csdr_amd_fir_decimate_cc(self.h, di.ptr, do.ptr, s, n, n, opitch, decimation, dt.ptr, taps.size), "fir_decimate_cc")
        y = self.download(do, c64, s * opitch).reshape(s, opitch)[:, :no]
        return y[0].copy() if squeeze else y.copy()

    def fir_ff(self, x, taps):
        x2, squeeze = self._2d(x, f32); taps = np.ascontiguousarray(taps, f32)
        s, n = x2.shape
        di = self.upload(x2); dt = self.upload(taps); do = self.alloc(4 * s * n + 64)
        no = self.check(self.L.csdr_amd_fir_ff(self.h, di.ptr, do.ptr, s, n, n, n, dt.ptr, taps.size), "fir_ff")
        y = self.download(do, f32, s * n).reshape(s, n)[:, :no]
        return y[0].copy() if squeeze else y.copy()


    # ---- f2 blocks
    def _cf_to_f(self, fn, x, *extra):
        x = np.ascontiguousarray(x, c64).ravel()
        di = self.upload(x); do = self.alloc(4 * x.size + 64)
        self.check(fn(self.h, di.ptr, do.ptr, x.size, *extra), fn.__name__)
        return self.download(do, f32, x.size)

    def amdemod_cf(self, x): return self._cf_to_f(self.L.csdr_amd_amdemod_cf, x)
    def amdemod_estimator_cf(self, x, alpha=0.0, beta=0.0): return self._cf_to_f(self.L.csdr_amd_amdemod_estimator_cf, x, alpha, beta)
    def realpart_cf(self, x): return self._cf_to_f(self.L.csdr_amd_realpart_cf, x)
    def logpower_cf(self, x, add_db=0.0): return self._cf_to_f(self.L.csdr_amd_logpower_cf, x, add_db)

    # ---- transmit-side modulators (txmod.hip)
    def fmmod_fc(self, x, phase=None, calls=None, in_pitch=None, out_pitch=None):
        """x: [n] or [streams, n] float32; phase: last_phase per stream; calls: per-call sample counts -> (complex [streams, n], last_phase [streams])"""
        x2, squeeze = self._2d(x, f32)
        s, n = x2.shape
        ph = np.zeros(s, f32) if phase is None else np.ascontiguousarray(phase, f32).reshape(s).copy()
        calls = [n] if calls is None else [int(k) for k in calls]
        ip = max(n, 1) if in_pitch is None else int(in_pitch)
        op = max(n, 1) if out_pitch is None else int(out_pitch)
        xin = np.zeros((s, ip), f32); xin[:, :n] = x2
        di = self.upload(xin); do = self.alloc(8 * s * op + 64); dl = self.upload(ph)
        at = 0
        for k in calls:
            self.check(self.L.csdr_amd_fmmod_fc(self.h, di.at(4 * at), do.at(8 * at), s, k, ip, op, dl.ptr), "fmmod_fc"); at += k
        y = self.download(do, c64, s * op).reshape(s, op)[:, :n].copy(); lo = self.download(dl, f32, s)
        return (y[0], lo[0]) if squeeze else (y, lo)

    def _flat(self, fn, x, in_dt, out_dt, out_per_in, *extra):
        x = np.ascontiguousarray(x, in_dt).ravel()
        di = self.upload(x); do = self.alloc(np.dtype(out_dt).itemsize * out_per_in * x.size + 64)
        self.check(fn(self.h, di.ptr, do.ptr, x.size, *extra), fn.__name__)
        return self.download(do, out_dt, out_per_in * x.size)

    def dsb_fc(self, x, q_value=0.0): return self._flat(self.L.csdr_amd_dsb_fc, x, f32, c64, 1, q_value)
    def add_dcoffset_cc(self, x): return self._flat(self.L.csdr_amd_add_dcoffset_cc, x, c64, c64, 1)
    def fixed_amplitude_cc(self, x, amp): return self._flat(self.L.csdr_amd_fixed_amplitude_cc, x, c64, c64, 1, amp)
    def convert_f_samplerf(self, x, wait): return self._flat(self.L.csdr_amd_convert_f_samplerf, x, f32, np.uint8, 16, int(wait))

    def fmdemod_atan_cf(self, x, last_phase=None, calls=1):
        x2, squeeze = self._2d(x, c64)
        s, n = x2.shape
        lp = np.zeros(s, f32) if last_phase is None else np.ascontiguousarray(last_phase, f32).reshape(s)
        di = self.upload(x2); do = self.alloc(4 * s * n + 64); dl = self.upload(lp)
        per = (n + calls - 1) // calls; at = 0
        while at < n:
            k = min(per, n - at)
            self.check(self.L.csdr_amd_fmdemod_atan_cf(self.h, di.at(8 * at), do.at(4 * at), s, k, n, n, dl.ptr), "fmdemod_atan"); at += k
        y = self.download(do, f32, s * n).reshape(s, n); lo = self.download(dl, f32, s)
        return (y[0], lo[0]) if squeeze else (y, lo)

    def dcblock_ff(self, x, a=0.0, state=None, calls=1):
        x2, squeeze = self._2d(x, f32)
        s, n = x2.shape
        st = np.zeros(2 * s, f32) if state is None else np.ascontiguousarray(state, f32).reshape(2 * s)
        di = self.upload(x2); do = self.alloc(4 * s * n + 64); ds = self.upload(st)
        per = (n + calls - 1) // calls; at = 0
        while at < n:
            k = min(per, n - at)
            self.check(self.L.csdr_amd_dcblock_ff(self.h, di.at(4 * at), do.at(4 * at), s, k, n, n, a, ds.ptr), "dcblock"); at += k
        y = self.download(do, f32, s * n).reshape(s, n); so = self.download(ds, f32, 2 * s).reshape(s, 2)
        return (y[0], so[0]) if squeeze else (y, so)

    def fastdcblock_ff(self, x, block=1024, last_dc=None, calls=1):
        x2, squeeze = self._2d(x, f32)
        s, n = x2.shape; nb = n // block
        ld = np.zeros(s, f32) if last_dc is None else np.ascontiguousarray(last_dc, f32).reshape(s)
        di = self.upload(x2); do = self.alloc(4 * s * n + 64); dl = self.upload(ld)
        per = max(1, (nb + calls - 1) // calls); b = 0
        while b < nb:
            k = min(per, nb - b)
            self.check(self.L.csdr_amd_fastdcblock_ff(self.h, di.at(4 * b * block), do.at(4 * b * block), s, k, block, n, n, dl.ptr), "fastdcblock"); b += k
        y = self.download(do, f32, s * n).reshape(s, n)[:, :nb * block]; lo = self.download(dl, f32, s)
        return (y[0].copy(), lo[0]) if squeeze else (y.copy(), lo)

    def agc_ff(self, x, block=1024, hang_time=200, reference=0.2, attack_rate=0.01, decay_rate=0.0001, max_gain=65536.0,
               attack_wait=0, filter_alpha=0.999, last_gain=None):
        x2, squeeze = self._2d(x, f32)
        s, n = x2.shape
        lg = np.ones(s, f32) if last_gain is None else np.ascontiguousarray(last_gain, f32).reshape(s)
        di = self.upload(x2); do = self.alloc(4 * s * n + 64); dl = self.upload(lg)
        self.check(self.L.csdr_amd_agc_ff(self.h, di.ptr, do.ptr, s, n, block, n, n, reference, attack_rate, decay_rate, max_gain, hang_time, attack_wait,
                                          filter_alpha, dl.ptr), "agc_ff")
        y = self.download(do, f32, s * n).reshape(s, n); lo = self.download(dl, f32, s)
        return (y[0], lo[0]) if squeeze else (y, lo)

    def precalculate_window(self, size, window="HAMMING"):
        w = np.zeros(size, f32); self.L.csdr_amd_precalculate_window(_hp(w), size, WINDOWS[window]); return w

    def fft_cc(self, x, fft_size, every_n, window="HAMMING", calls=1):
        x = np.ascontiguousarray(x, c64).ravel()
        frames_max = x.size // every_n + 1
        with _Handle(self, "fftcc", self.L.csdr_amd_fftcc_create(self.h, fft_size, every_n, WINDOWS[window], frames_max)) as f:
            di = self.upload(x); do = self.alloc(8 * fft_size * frames_max + 64)
            per = (x.size + calls - 1) // calls; at = 0; total = 0; left = 0
            while at < x.size or left:
                take = min(per, x.size - at) + left
                start = at - left
                cons = C.c_size_t(0)
                nf = self.check(f._fn("process")(f.h, di.at(8 * start), take, do.at(8 * fft_size * total), C.byref(cons)), "fft_cc")
                total += nf
                at = start + take; left = take - cons.value
                if at >= x.size and (nf == 0 or left < every_n):
                    break
            return self.download(do, c64, fft_size * total)


    # ---- the waterfall (waterfall.hip)
    def waterfall(self, fft_size, every_n, avgnumber, add_db=0.0, window="HAMMING", in_format="u8", out_format="db", n_streams=1, max_samples_per_call=1 << 20):
        """A batched `[convert_u8_f |] fft_cc | logaveragepower_cf | fft_exchange_sides_ff [| compress_fft_adpcm_f_u8]` object (csdr_amd_waterfall);
        in_format "f32" / "s16": `[convert_s16_f |] fft_fc | logaveragepower_cf [| compress_fft_adpcm_f_u8]` on real samples, fft_size = output bins."""
        return Waterfall(self, fft_size, every_n, avgnumber, add_db, window, in_format, out_format, n_streams, max_samples_per_call)

    def fft_fc(self, x, fft_out_size, every_n, window="HAMMING", calls=1):
        """`csdr fft_fc` (csdr.c:3414-3498) on one stream of floats, cut into `calls` calls -> [spectra, fft_out_size] complex64"""
        x = np.ascontiguousarray(x, f32).ravel()
        per = max(1, (x.size + calls - 1) // calls)
        frames_max = x.size // min(every_n, 2 * fft_out_size) + calls + 1
        with _Handle(self, "fftfc", self.L.csdr_amd_fftfc_create(self.h, fft_out_size, every_n, WINDOWS[window], per)) as f:
            di = self.upload(x); do = self.alloc(8 * fft_out_size * frames_max + 64)
            total = 0
            for at in range(0, x.size, per):
                total += self.check(f._fn("process")(f.h, di.at(4 * at), min(per, x.size - at), do.at(8 * fft_out_size * total)), "fft_fc")
            return self.download(do, c64, fft_out_size * total).reshape(total, fft_out_size)

    def fft_one_side_ff(self, x, fft_size):
        """`csdr fft_one_side_ff` (csdr.c:1717-1734): the first fft_size/2 floats of every row of fft_size -> [n_rows, fft_size/2]"""
        x = np.ascontiguousarray(x, f32).ravel(); rows = x.size // fft_size
        di = self.upload(x); do = self.alloc(4 * rows * (fft_size // 2) + 64)
        self.check(self.L.csdr_amd_fft_one_side_ff(self.h, di.ptr, do.ptr, rows, fft_size), "fft_one_side_ff")
        return self.download(do, f32, rows * (fft_size // 2)).reshape(rows, fft_size // 2)

    def logaveragepower_cf(self, x, fft_size, avgnumber, add_db=0.0):
        """x: n_rows*avgnumber spectra of fft_size bins -> [n_rows, fft_size] dB rows (csdr.c:1663-1695)"""
        x = np.ascontiguousarray(x, c64).ravel(); rows = x.size // (fft_size * avgnumber)
        di = self.upload(x); do = self.alloc(4 * rows * fft_size + 64)
        self.check(self.L.csdr_amd_logaveragepower_cf(self.h, di.ptr, do.ptr, rows, fft_size, avgnumber, add_db), "logaveragepower_cf")
        return self.download(do, f32, rows * fft_size).reshape(rows, fft_size)

    def fft_exchange_sides_ff(self, x, fft_size):
        x = np.ascontiguousarray(x, f32).ravel(); rows = x.size // fft_size
        di = self.upload(x); do = self.alloc(4 * rows * fft_size + 64)
        self.check(self.L.csdr_amd_fft_exchange_sides_ff(self.h, di.ptr, do.ptr, rows, fft_size), "fft_exchange_sides_ff")
        return self.download(do, f32, rows * fft_size).reshape(rows, fft_size)

    # ---- f3: IMA ADPCM
    def encode_ima_adpcm_i16_u8(self, x, state=None, calls=1):
        x2, squeeze = self._2d(x, np.int16)
        s, n = x2.shape
        st = np.zeros(2 * s, np.int32) if state is None else np.ascontiguousarray(state, np.int32).reshape(2 * s)
        di = self.upload(x2); do = self.alloc(s * (n // 2) + 64); ds = self.upload(st)
        per = ((n + calls - 1) // calls + 1) & ~1; at = 0
        while at < n:
            k = min(per, n - at)
            self.check(self.L.csdr_amd_encode_ima_adpcm_i16_u8(self.h, di.at(2 * at), do.at(at // 2), s, k, n, n // 2, ds.ptr), "adpcm encode"); at += k
        y = self.download(do, np.uint8, s * (n // 2)).reshape(s, n // 2); so = self.download(ds, np.int32, 2 * s).reshape(s, 2)
        return (y[0], so[0]) if squeeze else (y, so)

    def decode_ima_adpcm_u8_i16(self, x, state=None, calls=1):
        x2, squeeze = self._2d(x, np.uint8)
        s, n = x2.shape
        st = np.zeros(2 * s, np.int32) if state is None else np.ascontiguousarray(state, np.int32).reshape(2 * s)
        di = self.upload(x2); do = self.alloc(4 * s * n + 64); ds = self.upload(st)
        per = (n + calls - 1) // calls; at = 0
        while at < n:
            k = min(per, n - at)
            self.check(self.L.csdr_amd_decode_ima_adpcm_u8_i16(self.h, di.at(at), do.at(4 * at), s, k, n, 2 * n, ds.ptr), "adpcm decode"); at += k
        y = self.download(do, np.int16, 2 * s * n).reshape(s, 2 * n); so = self.download(ds, np.int32, 2 * s).reshape(s, 2)
        return (y[0], so[0]) if squeeze else (y, so)

    def compress_fft_adpcm_f_u8(self, x, fft_size):
        x = np.ascontiguousarray(x, f32).ravel(); nb = x.size // fft_size; ob = (fft_size + 10) // 2
        di = self.upload(x); do = self.alloc(nb * ob + 64)
        self.check(self.L.csdr_amd_compress_fft_adpcm_f_u8(self.h, di.ptr, do.ptr, nb, fft_size), "compress_fft")
        return self.download(do, np.uint8, nb * ob)

    def fmdemod_quadri_cf(self, x, last=None):
        x2, squeeze = self._2d(x, c64)
        s, n = x2.shape
        lst = np.zeros(s, c64) if last is None else np.ascontiguousarray(last, c64).reshape(s)
        di = self.upload(x2); do = self.alloc(4 * s * n + 64); dl = self.upload(lst)
        self.check(self.L.csdr_amd_fmdemod_quadri_cf(self.h, di.ptr, do.ptr, s, n, n, n, dl.ptr), "fmdemod")
        y = self.download(do, f32, s * n).reshape(s, n); lo = self.download(dl, c64, s)
        return (y[0], lo[0]) if squeeze else (y, lo)

    def limit_ff(self, x, m=1.0):
        x = np.ascontiguousarray(x, f32); di = self.upload(x); do = self.alloc(x.nbytes + 64)
        self.check(self.L.csdr_amd_limit_ff(self.h, di.ptr, do.ptr, x.size, m), "limit"); return self.download(do, f32, x.size).reshape(x.shape)

    def gain_ff(self, x, g):
        x = np.ascontiguousarray(x, f32); di = self.upload(x); do = self.alloc(x.nbytes + 64)
        self.check(self.L.csdr_amd_gain_ff(self.h, di.ptr, do.ptr, x.size, g), "gain"); return self.download(do, f32, x.size).reshape(x.shape)

    def deemphasis_wfm_ff(self, x, tau, sample_rate, last=None):
        x2, squeeze = self._2d(x, f32)
        s, n = x2.shape
        lst = np.zeros(s, f32) if last is None else np.ascontiguousarray(last, f32).reshape(s)
        di = self.upload(x2); do = self.alloc(4 * s * n + 64); dl = self.upload(lst)
        self.check(self.L.csdr_amd_deemphasis_wfm_ff(self.h, di.ptr, do.ptr, s, n, n, n, tau, int(sample_rate), dl.ptr), "deemph")
        y = self.download(do, f32, s * n).reshape(s, n); lo = self.download(dl, f32, s)
        return (y[0], lo[0]) if squeeze else (y, lo)

    def fastagc_ff(self, x, block=1024, reference=1.0, calls=1):
        """x: [n] or [streams, n]; whole blocks only; `calls` splits the blocks over several API calls (state carry)."""
        x2, squeeze = self._2d(x, f32)
        s, n = x2.shape; nb = n // block
        di = self.upload(x2); do = self.alloc(4 * s * n + 64)
        dst = self.upload(np.zeros(s * (2 * block + 4), f32))
        per = max(1, (nb + calls - 1) // calls); b = 0
        while b < nb:
            k = min(per, nb - b)
            self.check(self.L.csdr_amd_fastagc_ff(self.h, di.at(4 * b * block), do.at(4 * b * block), s, k, block, n, n, reference, dst.ptr), "fastagc")
            b += k
        y = self.download(do, f32, s * n).reshape(s, n)[:, :nb * block]
        return y[0].copy() if squeeze else y.copy()

    def fractional_decimator_ff(self, x, rate, num_poly_points=12, taps=None, bufsize=None):
        x2, squeeze = self._2d(x, f32)
        s, n = x2.shape
        tp = None if taps is None else np.ascontiguousarray(taps, f32)
        with _Handle(None, "fracdec", self.L.csdr_amd_fracdec_create(rate, num_poly_points, None if tp is None else _hp(tp), 0 if tp is None else tp.size)) as d:
            if bufsize:                               # the CLI's window loop (csdr.c:1511-1524) instead of one call over the whole array
                d._fn("set_cli_bufsize")(d.h, bufsize)
            di = self.upload(x2); do = self.alloc(4 * s * n + 64); proc = C.c_int(0)
            no = self.check(self.L.csdr_amd_fractional_decimator_ff(self.h, d.h, di.ptr, do.ptr, s, n, n, n, C.byref(proc)), "fracdec")
            self.sync()                               # (the kernels read the object's tables: they finish in front of its destroy)
        y = self.download(do, f32, s * n).reshape(s, n)[:, :no]
        return y[0].copy() if squeeze else y.copy()

    # ---- FIR resamplers (resampler.hip)
    def resampler(self, interpolation, decimation, taps=None, n_streams=1, transition_bw=0.05, window="HAMMING", bufsize=None):
        """A batched rational_resampler_ff object; taps default to rational_resampler_get_lowpass_f(firdes_filter_len(transition_bw), I, D, window)."""
        if taps is None:
            taps = rational_resampler_get_lowpass_f(self.firdes_filter_len(transition_bw), interpolation, decimation, window)
        return Resampler(self, interpolation, decimation, taps, n_streams, bufsize)

    # ---- BPSK31 receive chain (psk31.hip)
    def psk31(self, params=None, n_channels=1, first="agc", last="varicode"):
        """A batched BPSK31 receive chain object (Psk31); params from psk31_params()"""
        return Psk31(self, params, n_channels, first, last)

    def simple_agc_cc(self, x, rate, reference=1.0, max_gain=65535.0, gain=None):
        """simple_agc_cc (libcsdr.c:2201-2217) on [n_streams, n] (or [n]) complex samples; gain: per-stream starting gain (default 1, as the CLI)
        -> (output, gain after the last sample)"""
        x = np.ascontiguousarray(x, c64)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None]
        s, n = x.shape
        g = np.ascontiguousarray(np.ones(s, f32) if gain is None else np.broadcast_to(np.asarray(gain, f32), (s,)), f32)
        di = self.upload(x); dg = self.upload(g)
        do = self.alloc(8 * max(n, 1) * s + 256)
        self.check(self.L.csdr_amd_simple_agc_cc(self.h, di.ptr, do.ptr, s, n, n, n, rate, reference, max_gain, dg.ptr), "simple_agc_cc")
        y = self.download(do, c64, n * s).reshape(s, n)
        g = self.download(dg, f32, s)
        return (y[0].copy(), float(g[0])) if squeeze else (y.copy(), g.copy())

    # ---- BPSK31 transmit chain (psk31tx.hip)
    def psk31_tx(self, n_channels=1, n_psk=2, interpolation=256, first="varicode", last="shape"):
        """A batched BPSK31 transmit chain object (Psk31Tx)"""
        return Psk31Tx(self, n_channels, n_psk, interpolation, first, last)

    def differential_decoder_u8_u8(self, x, state=None):
        """differential_codec's decode branch (libcsdr.c:1830-1835) on [n_streams, n] (or [n]) bytes; state: per-stream previous byte (default 0, as
        the CLI) -> (output, the last byte of each stream)"""
        x = np.ascontiguousarray(x, np.uint8)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None]
        s, n = x.shape
        st = np.ascontiguousarray(np.zeros(s, np.uint8) if state is None else np.broadcast_to(np.asarray(state, np.uint8), (s,)), np.uint8)
        di = self.upload(x) if n else self.alloc(256)
        ds = self.upload(st)
        do = self.alloc(max(n, 1) * s + 256)
        self.check(self.L.csdr_amd_differential_decoder_u8_u8(self.h, di.ptr, do.ptr, s, n, max(n, 1), max(n, 1), ds.ptr), "differential_decoder_u8_u8")
        y = self.download(do, np.uint8, max(n, 1) * s).reshape(s, max(n, 1))[:, :n]
        st = self.download(ds, np.uint8, s)
        return (y[0].copy(), int(st[0])) if squeeze else (y.copy(), st.copy())

    def duplicate_samples_ntimes_u8_u8(self, x, sample_size_bytes, ntimes):
        """duplicate_samples_ntimes_u8_u8 (libcsdr.c:1784-1791) on [n_streams, n_bytes] (or [n_bytes]) bytes -> every whole sample ntimes"""
        x = np.ascontiguousarray(x, np.uint8)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None]
        s, n = x.shape
        m = n // max(sample_size_bytes, 1) * max(sample_size_bytes, 1) * max(ntimes, 0)
        di = self.upload(x) if n else self.alloc(256)
        do = self.alloc(max(m, 1) * s + 256)
        self.check(self.L.csdr_amd_duplicate_samples_ntimes_u8_u8(self.h, di.ptr, do.ptr, s, n, max(n, 1), max(m, 1), sample_size_bytes, ntimes),
                   "duplicate_samples_ntimes_u8_u8")
        y = self.download(do, np.uint8, max(m, 1) * s).reshape(s, max(m, 1))[:, :m]
        return y[0].copy() if squeeze else y.copy()

    # ---- pulse-shaped symbol modem (modem.hip)
    def pulse_tx(self, n_channels=1, n_psk=4, interpolation=8, taps=None, first="mod", last="shape"):
        """A batched pulse-shaping transmit object (PulseTx)"""
        return PulseTx(self, n_channels, n_psk, interpolation, taps, first, last)

    def pulse_rx(self, params, n_channels=1, first="filter", last="slice"):
        """A batched pulse-shaped receive object (PulseRx); params from pulserx_params()"""
        return PulseRx(self, params, n_channels, first, last)

    def frame_sync(self, pattern, values_after, n_channels=1, max_mismatch=0):
        """A batched frame synchroniser (FrameSync): `pattern_search_u8_u8 values_after pattern...` for n_channels byte streams"""
        return FrameSync(self, pattern, values_after, n_channels, max_mismatch)

    def pattern_search(self, x, pattern, values_after):
        """pattern_search_u8_u8 (csdr.c:3532-3597) on one stream of bytes with fresh state -> the payload bytes"""
        x, pat = np.ascontiguousarray(x, np.uint8).ravel(), np.ascontiguousarray(pattern, np.uint32)
        di, do, dc = self.upload(x), self.alloc(x.size + 256), self.alloc(256)
        self.check(self.L.csdr_amd_pattern_search_u8_u8(self.h, di.ptr, x.size, _hp(pat), pat.size, int(values_after), do.ptr, dc.ptr), "pattern_search_u8_u8")
        return self.download(do, np.uint8, int(self.download(dc, np.int32, 1)[0]))

    @staticmethod
    def framesync_debug_walk(pattern, values_after, x, max_mismatch=0, cuts=(), state=None, window=None):
        """framesync_debug_walk: the CPU run of the frame synchroniser's step function for one channel"""
        return framesync_debug_walk(pattern, values_after, x, max_mismatch, cuts, state, window)

    @staticmethod
    def pulserx_debug_walk(params, first="filter", last="slice", x=None, cuts=(), state=None, with_extras=False):
        """pulserx_debug_walk: the CPU run of the receive object's walk for one channel"""
        return pulserx_debug_walk(params, first, last, x, cuts, state, with_extras)

    def _flat_rows(self, fn, name, x, dtype_in, dtype_out, n_out, *extra):
        x = np.ascontiguousarray(x, dtype_in)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None]
        s, n = x.shape
        m = n_out(n)
        di = self.upload(x) if n else self.alloc(256)
        do = self.alloc(np.dtype(dtype_out).itemsize * max(m, 1) * s + 256)
        self.check(fn(self.h, di.ptr, do.ptr, s, n, max(n, 1), max(m, 1), *extra), name)
        y = self.download(do, dtype_out, max(m, 1) * s).reshape(s, max(m, 1))[:, :m]
        return y[0].copy() if squeeze else y.copy()

    def generic_slicer_f_u8(self, x, n_symbols):
        """generic_slicer_f_u8 (libcsdr.c:1731-1765) on [n_streams, n] (or [n]) floats; NaN gives 0"""
        return self._flat_rows(self.L.csdr_amd_generic_slicer_f_u8, "generic_slicer_f_u8", x, f32, np.uint8, lambda n: n, int(n_symbols))

    def plain_interpolate_cc(self, x, interpolation):
        """plain_interpolate_cc (libcsdr.c:2499-2506) on [n_streams, n] (or [n]) complex samples -> n * interpolation each"""
        return self._flat_rows(self.L.csdr_amd_plain_interpolate_cc, "plain_interpolate_cc", x, c64, c64, lambda n: n * max(int(interpolation), 0), int(interpolation))

    def pack_bits_1to8(self, x):
        """pack_bits_1to8_u8_u8 (libcsdr.c:1810-1815) on [n_streams, n] (or [n]) bytes -> 8 n bytes each, LSB first"""
        return self._flat_rows(self.L.csdr_amd_pack_bits_1to8_u8_u8, "pack_bits_1to8_u8_u8", x, np.uint8, np.uint8, lambda n: 8 * n)

    def pack_bits_8to1(self, x):
        """pack_bits_8to1_u8_u8 (libcsdr.c:1818-1827) on every group of eight of [n_streams, n] (or [n]) bytes, n a multiple of 8 -> n / 8 bytes each, MSB first"""
        return self._flat_rows(self.L.csdr_amd_pack_bits_8to1_u8_u8, "pack_bits_8to1_u8_u8", x, np.uint8, np.uint8, lambda n: n // 8)

    def apply_real_fir_cc(self, x, taps):
        """apply_real_fir_cc (libcsdr.c:2276-2291) on [n_streams, n] (or [n]) complex samples -> n - len(taps) + 1 each"""
        x2, squeeze = self._2d(x, c64); taps = np.ascontiguousarray(taps, f32)
        s, n = x2.shape
        di = self.upload(x2) if n else self.alloc(256); dt = self.upload(taps); do = self.alloc(8 * s * max(n, 1) + 64)
        no = self.check(self.L.csdr_amd_apply_real_fir_cc(self.h, di.ptr, do.ptr, s, n, max(n, 1), max(n, 1), dt.ptr, taps.size), "apply_real_fir_cc")
        y = self.download(do, c64, s * max(n, 1)).reshape(s, max(n, 1))[:, :no]
        return y[0].copy() if squeeze else y.copy()

    # ---- RTTY receive chain (rtty.hip)
    def rtty(self, params=None, n_channels=1, first="bfsk", last="baudot"):
        """A batched RTTY receive chain object (Rtty); params from rtty_params()"""
        return Rtty(self, params, n_channels, first, last)

    def bfsk_demod_cf(self, x, mark, space, force_generic=False):
        """bfsk_demod_cf (libcsdr.c:2335-2350) with caller taps on [n_streams, n] (or [n]) complex samples -> [n_streams, n - L + 1] float32"""
        x = np.ascontiguousarray(x, c64)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None]
        s, n = x.shape
        mark = np.ascontiguousarray(mark, c64); space = np.ascontiguousarray(space, c64)
        L = mark.size
        no = max(n - L + 1, 0)
        di = self.upload(x); dt = self.upload(np.concatenate([mark, space]))
        do = self.alloc(4 * max(no, 1) * s + 256)
        self.check(self.L.csdr_amd_bfsk_demod_cf(self.h, di.ptr, do.ptr, s, n, n, max(no, 1), dt.ptr, dt.at(8 * L), L, int(force_generic)), "bfsk_demod_cf")
        y = self.download(do, f32, max(no, 1) * s).reshape(s, max(no, 1))[:, :no].copy()
        self.last_bfsk_kernel = self.L.csdr_amd_bfsk_last_kernel().decode()
        return y[0] if squeeze else y

    # ---- complex-tap FIR (cfir.hip)
    def cfir(self, n_channels=1, taps_length=101):
        """A batched complex-tap FIR object (CFir)"""
        return CFir(self, n_channels, taps_length)

    def apply_fir_cc(self, x, taps, force_generic=False):
        """apply_fir_cc (libcsdr.c:2261-2273) on [n_streams, n] (or [n]) complex samples; taps [T] for all streams or [n_streams, T] -> [n_streams, n - T + 1]"""
        x2, squeeze = self._2d(x, c64); taps = np.ascontiguousarray(taps, c64)
        s, n = x2.shape
        if taps.ndim not in (1, 2) or (taps.ndim == 2 and taps.shape[0] != s):
            raise ValueError("taps should be [T] or [%d, T]" % s)
        T = taps.shape[-1]
        no = max(n - T + 1, 0)
        di = self.upload(x2) if n else self.alloc(256); dt = self.upload(taps) if taps.size else self.alloc(256); do = self.alloc(8 * s * max(no, 1) + 64)
        self.check(self.L.csdr_amd_apply_fir_cc(self.h, di.ptr, do.ptr, s, n, max(n, 1), max(no, 1), dt.ptr, T if taps.ndim == 2 else 0, T, int(force_generic)), "apply_fir_cc")
        y = self.download(do, c64, s * max(no, 1)).reshape(s, max(no, 1))[:, :no].copy()
        self.last_apply_fir_kernel = self.L.csdr_amd_apply_fir_last_kernel().decode()
        return y[0] if squeeze else y

    # ---- noise sources, AWGN channel and link measurements (noise.hip)
    def noise(self, n_channels=1, kind="gaussian", seed=0, stream_ids=None, snr_db=None):
        """A batched noise source / AWGN channel (Noise)"""
        return Noise(self, n_channels, kind, seed, stream_ids, snr_db)

    def awgn_cc(self, x, noise, a_signal, a_noise_scaled):
        """the flat awgn_cc on the caller's noise rows: x, noise [n_channels, n] (or [n]); gains per channel or one for all -> x * a_signal + noise * a_noise_scaled"""
        x2, squeeze = self._2d(x, c64); nz, _ = self._2d(noise, c64)
        s, n = x2.shape
        if nz.shape != x2.shape:
            raise ValueError("x and noise should have one shape")
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(a_signal, f32), (s,)), f32); g = np.ascontiguousarray(np.broadcast_to(np.asarray(a_noise_scaled, f32), (s,)), f32)
        di = self.upload(x2) if n else self.alloc(256); dn = self.upload(nz) if n else self.alloc(256); do = self.alloc(8 * s * max(n, 1)); da = self.upload(a); dg = self.upload(g)
        self.check(self.L.csdr_amd_awgn_cc(self.h, di.ptr, dn.ptr, do.ptr, s, n, max(n, 1), max(n, 1), max(n, 1), da.ptr, dg.ptr), "awgn_cc")
        y = self.download(do, c64, s * max(n, 1)).reshape(s, max(n, 1))[:, :n].copy()
        return y[0] if squeeze else y

    def total_logpower_cf(self, x):
        """total_logpower_cf of each row of [n_rows, n] (or [n]) complex samples, in dB"""
        x2, squeeze = self._2d(x, c64)
        s, n = x2.shape
        di = self.upload(x2); do = self.alloc(4 * s)
        self.check(self.L.csdr_amd_total_logpower_cf(self.h, di.ptr, s, n, n, do.ptr), "total_logpower_cf")
        y = self.download(do, f32, s)
        return y[0] if squeeze else y

    def normalized_timing_variance_u32_f(self, idx, samples_per_symbol, initial_sample_offset, counts=None):
        """normalized_timing_variance_u32_f of each row of [n_rows, n] sample indexes (row r: its first counts[r]) -> n_rows floats"""
        idx = np.ascontiguousarray(idx, np.uint32)
        if idx.ndim == 1:
            idx = idx[None]
        s, n = idx.shape
        di = self.upload(idx) if n else self.alloc(256); do = self.alloc(4 * s)
        dc = self.upload(np.ascontiguousarray(counts, np.int32)) if counts is not None else None
        self.check(self.L.csdr_amd_normalized_timing_variance_u32_f(self.h, di.ptr, max(n, 1), n, dc.ptr if dc else None, s, int(samples_per_symbol),
                                                                    int(initial_sample_offset), do.ptr), "normalized_timing_variance_u32_f")
        return self.download(do, f32, s)

    def count_errors_u8(self, a, b, lags=None, counts=None):
        """per row c the number of i < counts[c] with a[c][lags[c] + i] != b[c][i] (a, b: [n_channels, len] bytes) -> n_channels ints"""
        a = np.ascontiguousarray(a, np.uint8); b = np.ascontiguousarray(b, np.uint8)
        if a.ndim != 2 or b.ndim != 2 or a.shape[0] != b.shape[0]:
            raise ValueError("a and b should be [n_channels, len] with one n_channels")
        s = a.shape[0]
        da = self.upload(a) if a.size else self.alloc(256); db_ = self.upload(b) if b.size else self.alloc(256); de = self.alloc(4 * s)
        dl = self.upload(np.ascontiguousarray(lags, np.int32)) if lags is not None else None
        dc = self.upload(np.ascontiguousarray(counts, np.int32)) if counts is not None else None
        self.check(self.L.csdr_amd_count_errors_u8(self.h, da.ptr, max(a.shape[1], 1), a.shape[1], db_.ptr, max(b.shape[1], 1), b.shape[1], s,
                                                   dl.ptr if dl else None, dc.ptr if dc else None, de.ptr), "count_errors_u8")
        return self.download(de, np.int32, s)

    # ---- squelch and S-meter (squelch.hip)
    def squelch(self, n_channels=1, block_size=1024, use_every_nth=1, levels=None, max_samples_per_call=1 << 22):
        """A batched squelch_and_smeter_cc object (Squelch)"""
        return Squelch(self, n_channels, block_size, use_every_nth, levels, max_samples_per_call)

    # ---- the NFM receive bank on baseband (fmrx.hip)
    def fm_rx(self, n_channels=1, audio_rate=48000, agc_block=1024, reference=1.0, limit=1.0, max_samples_per_call=1 << 16, squelch_block=0, use_every_nth=1, levels=None):
        """A batched fmdemod_quadri_cf | limit_ff | deemphasis_nfm_ff | fastagc_ff | convert_f_s16 object on complex baseband (FmRx), behind a squelch when
        squelch_block > 0"""
        return FmRx(self, n_channels, audio_rate, agc_block, reference, limit, max_samples_per_call, squelch_block, use_every_nth, levels)

    # ---- the WFM receive bank on baseband (wfmrx.hip)
    def wfm_rx(self, n_channels=1, rate=5, num_poly_points=12, prefilter_taps=None, window=1024, tau=50e-6, audio_rate=48000, max_samples_per_call=1 << 16,
               squelch_block=0, use_every_nth=1, levels=None):
        """A batched fmdemod_quadri_cf | fractional_decimator_ff | deemphasis_wfm_ff | convert_f_s16 object on complex baseband (WfmRx), behind a squelch when
        squelch_block > 0"""
        return WfmRx(self, n_channels, rate, num_poly_points, prefilter_taps, window, tau, audio_rate, max_samples_per_call, squelch_block, use_every_nth, levels)

    # ---- the AM and SSB receive chains (amssb.hip)
    def am_bank(self, n_channels=1, block=1024, agc=None, limit_max=None, **kw):
        """csdr_amd_amssb in AM mode (README.md:95's amdemod_cf | fastdcblock_ff | agc_ff | limit_ff | convert_f_s16); kw: AmSsb's squelch, use_every_nth, levels, in_format, max_samples_per_call
        and, for "u8", shift_rate, decimation, ddc_taps"""
        return AmSsb(self, amssb_params("am", block, agc, limit_max), n_channels, **kw)

    def ssb_bank(self, n_channels=1, block=1024, taps=None, fft_size=0, agc=None, limit_max=None, **kw):
        """csdr_amd_amssb in SSB mode (README.md:110's bandpass_fir_fft_cc | realpart_cf | agc_ff | limit_ff | convert_f_s16); taps: firdes_bandpass_c's, or
        None for no filter; passbands=[(low, high), ...]: a passband per channel (designed at the taps' length), window: their window"""
        if kw.get("passbands") is not None:
            kw["passbands"] = _passband_list(kw["passbands"], n_channels)
            if taps is None:
                raise ValueError("passbands need taps: their length is the passbands' length")
        return AmSsb(self, amssb_params("ssb", block, agc, limit_max), n_channels, taps=taps, fft_size=fft_size, **kw)

    # ---- carrier recovery (carrier.hip)
    def carrier(self, params, n_channels=1):
        """A batched bpsk_costas_loop_cc / pll_cc object (Carrier); params from costas_params() or pll_params()"""
        return Carrier(self, params, n_channels)

    def shiftbank(self, variant, rates, **kw):
        """A shifter bank with a rate per stream (ShiftBank)"""
        return ShiftBank(self, variant, rates, **kw)

    def txbank(self, n_streams, mode, interpolation, taps, rates, **kw):
        """The fused transmit bank (TxBank): mode "fm", "am" or "dsb"; kw: gain, q_value, out_format ("cf32" / "u8"), max_in_samples"""
        return TxBank(self, n_streams, mode, interpolation, taps, rates, **kw)

    def _get_power(self, x, block_size, decimation, dt, fn):
        x = np.ascontiguousarray(x, dt)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None]
        s, n = x.shape
        B = n if block_size is None else int(block_size)
        nb = n // B if B > 0 else 0
        di = self.upload(x); do = self.alloc(4 * max(nb, 1) * s + 256)
        self.check(fn(self.h, di.ptr, s, nb, B, int(decimation), n, do.ptr), "get_power")
        y = self.download(do, f32, nb * s).reshape(s, nb)
        return y[0].copy() if squeeze else y.copy()

    def get_power_c(self, x, block_size=None, decimation=1):
        """get_power_c (libcsdr.c:1154-1162) of the whole blocks of block_size samples (default: one block = the row) of [n_streams, n] (or [n])
        complex samples -> [n_streams, n_blocks] float32"""
        return self._get_power(x, block_size, decimation, c64, self.L.csdr_amd_get_power_c)

    def get_power_f(self, x, block_size=None, decimation=1):
        """get_power_f (libcsdr.c:1144-1152), as get_power_c on real samples"""
        return self._get_power(x, block_size, decimation, f32, self.L.csdr_amd_get_power_f)

    def binary_slicer_f_u8(self, x):
        """binary_slicer_f_u8 (libcsdr.c:1767-1770) on [n_streams, n] (or [n]) floats"""
        x = np.ascontiguousarray(x, f32)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None]
        s, n = x.shape
        di = self.upload(x); do = self.alloc(max(n, 1) * s + 256)
        self.check(self.L.csdr_amd_binary_slicer_f_u8(self.h, di.ptr, do.ptr, s, n, n, n), "binary_slicer_f_u8")
        y = self.download(do, np.uint8, n * s).reshape(s, n)
        return y[0].copy() if squeeze else y.copy()

    def rtty_line_decoder_u8_u8(self, x, calls=None):
        """rtty_line_decoder_u8_u8 (csdr.c:2446-2458) on [n_streams, n] (or [n]) bytes, fresh decoders, cut into `calls` -> per-stream text"""
        x = np.ascontiguousarray(x, np.uint8)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None]
        s, n = x.shape
        calls = [n] if calls is None else list(calls)
        di = self.upload(x)
        mx = max(max(calls) if calls else 0, 1)
        do = self.alloc(mx * s + 256); dc = self.alloc(4 * s + 256)
        dst = self.upload(np.zeros(5 * s, np.int32))
        outs = [[] for _ in range(s)]
        at = 0
        for k in calls:
            self.check(self.L.csdr_amd_rtty_line_decoder_u8_u8(self.h, di.at(at), do.ptr, s, k, n, mx, dst.ptr, dc.ptr), "rtty_line_decoder_u8_u8")
            cnt = self.download(dc, np.int32, s)
            y = self.download(do, np.uint8, mx * s).reshape(s, mx)
            for c in range(s):
                outs[c].append(y[c, :cnt[c]].copy())
            at += k
        res = [np.concatenate(o) for o in outs]
        return res[0] if squeeze else res

    def interpolator(self, interpolation, taps=None, n_streams=1, transition_bw=0.05, window="HAMMING", bufsize=None):
        """A batched fir_interpolate_cc object; taps default to firdes_lowpass_f(firdes_filter_len(transition_bw), 0.5 / I, window) as csdr.c:1212 designs them."""
        if taps is None:
            taps = fir_interpolate_lowpass_f(self.firdes_filter_len(transition_bw), interpolation, window)
        return Interpolator(self, interpolation, taps, n_streams, bufsize)

    def rational_resampler_ff(self, x, interpolation, decimation, taps=None, transition_bw=0.05, window="HAMMING", bufsize=None, calls=None):
        """x: [n] or [n_streams, n] float.  Default: the reference function over the whole stream; bufsize=B: the `csdr rational_resampler_ff` stream at that buffer size."""
        x2 = np.ascontiguousarray(x, f32)
        r = self.resampler(interpolation, decimation, taps, 1 if x2.ndim == 1 else x2.shape[0], transition_bw, window, bufsize)
        try:
            return r.process(x2, calls)
        finally:
            r.close()

    def fir_interpolate_cc(self, x, interpolation, taps=None, transition_bw=0.05, window="HAMMING", bufsize=None, calls=None):
        """x: [n] or [n_streams, n] complex.  Default: the reference function over the whole stream; bufsize=B: the `csdr fir_interpolate_cc` stream (B zeros first)."""
        x2 = np.ascontiguousarray(x, c64)
        p = self.interpolator(interpolation, taps, 1 if x2.ndim == 1 else x2.shape[0], transition_bw, window, bufsize)
        try:
            return p.process(x2, calls)
        finally:
            p.close()

    def fft_c2c(self, x, forward=True):
        x = np.ascontiguousarray(x, c64); di = self.upload(x); do = self.alloc(x.nbytes + 64)
        self.check(self.L.csdr_amd_fft_c2c(self.h, di.ptr, do.ptr, x.size, int(forward)), "fft"); return self.download(do, c64, x.size)

    def fftfilt(self, fft_size, taps, n_streams=1, max_blocks=1):
        """A csdr_amd_fftfilt object (FftFilt); taps 1-D: shared by the streams, 2-D [n_streams, taps_length]: a passband per stream"""
        return FftFilt(self, fft_size, taps, n_streams, max_blocks)

    def bandpass_fir_fft_cc(self, x, taps, fft_size, blocks_per_call=None):
        """taps: 1-D for every stream of x, or 2-D with one row per stream"""
        x2, squeeze = self._2d(x, c64)
        s, n = x2.shape
        taps = _fftfilt_taps(taps, s)
        inp = fft_size - taps.shape[-1] + 1; nb = n // inp
        per = nb if not blocks_per_call else blocks_per_call
        with FftFilt(self, fft_size, taps, s, max(per, 1)) as f:
            y = f.process(x2, [per] * (nb // per) + ([nb % per] if nb % per else [])) if nb else np.zeros((s, 0), c64)
        return y[0].copy() if squeeze else y

    def fastddc_init(self, tbw, decimation, shift_rate):
        d = FastDDC(); err = self.L.csdr_amd_fastddc_init(C.byref(d), tbw, decimation, shift_rate); return d, err

    def fastddc_fwd_cc(self, x, ddc, blocks_per_call=None):
        x = np.ascontiguousarray(x, c64); nb = x.size // ddc.input_size
        per = nb if not blocks_per_call else blocks_per_call
        with _Handle(self, "fastddc_fwd", self.L.csdr_amd_fastddc_fwd_create(self.h, C.byref(ddc), max(per, 1))) as f:
            di = self.upload(x); do = self.alloc(8 * nb * ddc.fft_size + 64)
            b = 0
            while b < nb:
                k = min(per, nb - b)
                self.check(f._fn("process")(f.h, di.at(8 * b * ddc.input_size), do.at(8 * b * ddc.fft_size), k), "fastddc_fwd")
                b += k
            return self.download(do, c64, nb * ddc.fft_size).reshape(nb, ddc.fft_size)

    def _note_ddc_call(self, inv, counts):
        """what a fastddc call ran and wrote: `last_ddc_kernels` (csdr_amd_fastddc_inv_kernels of the call), `ddc_kernels_seen` (the set over all calls of this
        context), and per call of the current fastddc_inv_cc / fastddc_bank run `ddc_call_kernels` / `ddc_call_counts` (samples written per channel)."""
        self.last_ddc_kernels = self.L.csdr_amd_fastddc_inv_kernels(inv).decode()
        self.ddc_kernels_seen.add(self.last_ddc_kernels)
        self.ddc_call_kernels.append(self.last_ddc_kernels); self.ddc_call_counts.append(counts.copy())

    def fastddc_inv_cc(self, spectra, tbw, decimation, shift_rates, window="HAMMING", blocks_per_call=None):
        """spectra [n_blocks, fft] -> list of per-channel outputs."""
        self.ddc_call_kernels = []; self.ddc_call_counts = []
        spectra = np.ascontiguousarray(spectra, c64); nb = spectra.shape[0]
        rates = np.ascontiguousarray(shift_rates, f32); nc = rates.size
        per = nb if not blocks_per_call else blocks_per_call
        with _Handle(self, "fastddc_inv", self.L.csdr_amd_fastddc_inv_create(self.h, tbw, decimation, _hp(rates), nc, WINDOWS[window], max(per, 1))) as f:
            fft = spectra.shape[1]
            di = self.upload(spectra)
            outs = [[] for _ in range(nc)]
            b = 0
            while b < nb:
                k = min(per, nb - b)
                pitch = f._fn("max_output")(f.h, k) + 8
                do = self.alloc(8 * nc * pitch)
                counts = np.zeros(nc, np.int32)
                self.check(f._fn("process")(f.h, di.at(8 * b * fft), k, do.ptr, pitch, _hp(counts)), "fastddc_inv")
                self._note_ddc_call(f.h, counts)
                y = self.download(do, c64, nc * pitch).reshape(nc, pitch)
                for c in range(nc):
                    outs[c].append(y[c, :counts[c]].copy())
                b += k
        return [np.concatenate(o) for o in outs]

    def fastddc_bank(self, x, tbw, decimation, shift_rates, window="HAMMING", blocks_per_call=None, retune=None, schedule=None, retunes=None):
        """forward + inverse in one object (csdr_amd_fastddc_bank_*): x = wideband samples -> list of per-channel outputs.
        retune = (call_index, channel, rate): applied before that call.  schedule = explicit list of blocks per call (instead of blocks_per_call);
        retunes = {call_index: [(channel, rate), ...]}.  x: complex64, or interleaved IQ as int16 / uint8 (csdr_amd_fastddc_bank_process_s16 / _u8)."""
        x, sfx, es = _bank_input(x)
        self.ddc_call_kernels = []; self.ddc_call_counts = []
        rates = np.ascontiguousarray(shift_rates, f32); nc = rates.size
        ddc, _ = self.fastddc_init(tbw, decimation, 0.0)
        nb = (x.size if es == 8 else x.size // 2) // ddc.input_size
        process = getattr(self.L, "csdr_amd_fastddc_bank_process" + sfx)
        per = nb if not blocks_per_call else blocks_per_call
        if schedule:
            per = max(schedule)
        with _Handle(self, "fastddc_bank", self.L.csdr_amd_fastddc_bank_create(self.h, tbw, decimation, _hp(rates), nc, WINDOWS[window], max(per, 1))) as bk:
            di = self.upload(x)
            outs = [[] for _ in range(nc)]
            b = 0; call = 0
            while b < nb:
                k = min(per, nb - b) if not schedule else min(schedule[call % len(schedule)], nb - b)
                if retune and retune[0] == call:
                    self.check(bk._fn("set_rate")(bk.h, retune[1], retune[2]), "bank_set_rate")
                for ch, rt in (retunes or {}).get(call, []):
                    self.check(bk._fn("set_rate")(bk.h, ch, rt), "bank_set_rate")
                pitch = bk._fn("max_output")(bk.h, k) + 8
                do = self.alloc(8 * nc * pitch)
                counts = np.zeros(nc, np.int32)
                self.check(process(bk.h, di.at(es * b * ddc.input_size), k, do.ptr, pitch, _hp(counts)), "fastddc_bank")
                self._note_ddc_call(bk._fn("inverse")(bk.h), counts)
                y = self.download(do, c64, nc * pitch).reshape(nc, pitch)
                for c in range(nc):
                    outs[c].append(y[c, :counts[c]].copy())
                b += k; call += 1
            self.last_ddc_kernel = self.L.csdr_amd_fastddc_inv_kernel_name(bk._fn("inverse")(bk.h)).decode()
        return [np.concatenate(o) for o in outs]

    # (the multi-rank form of the bank on ONE GPU: sharded_bank_loopback below, module level -- one Context per rank thread)

    def _seed_stats(self, pre, h, per_stream, seen=None, call=0):
        """csdr_amd_<pre>_seed_stats (pre: "ddc" / "wfm") of object h as a dict: a rate per stream -> generated, takeovers, refits, dirty, regrowths (seeds.hip's
        counters) and takeover_calls / refit_calls, the indexes of the calls in front of which those counters moved (`seen`: the dict of the call before);
        a shared rate -> tables_built alone.  None with an older build selected with CSDR_AMD_LIB."""
        if not hasattr(self.L, "csdr_amd_%s_seed_stats" % pre):
            return None
        if not per_stream:
            return {"tables_built": int(getattr(self.L, "csdr_amd_%s_tables_built" % pre)(h))}
        out = (C.c_long * 5)()
        self.check(getattr(self.L, "csdr_amd_%s_seed_stats" % pre)(h, out), "%s_seed_stats" % pre)
        st = dict(zip(("generated", "takeovers", "refits", "dirty", "regrowths"), (int(v) for v in out)))
        st["tables_built"] = st["generated"]
        for key, calls in (("takeovers", "takeover_calls"), ("refits", "refit_calls")):
            st[calls] = list(seen[calls]) if seen else []
            if st[key] > (seen[key] if seen else 0):
                st[calls].append(call)
        return st

    def wfm_chain(self, iq_u8, shift_rate, decimation, taps, frac_rate=5, tau=50e-6, audio_rate=48000, block=None, pitch_pad=0, retunes=None, want_float=True,
                  out_per_call=False, max_block=None, deemph_state=None, repeat_after_reset=False):
        """iq_u8: [2n] or [streams, 2n] uint8 -> (s16 [streams, na], float audio [streams, na]); `block` = samples per call (or a list of call sizes);
        `pitch_pad` = extra bytes of row pitch (multiple of 16).  shift_rate: one float, or one per stream (csdr_amd_wfm_create_rates);
        retunes: {call index: [(stream, rate), ...]} applied in front of that call.  want_float=False: s16 only (the kernel's line-collecting store path).
        out_per_call: every call writes at the START of the (16-byte aligned) output rows, as a streaming caller with one output buffer does -- the kernel's
        aligned store path on every call (otherwise call k's audio follows call k - 1's in one row: aligned only by chance).
        max_block: the object's max_block_samples (default: the largest call) -- it sizes the chunk-seed tables, nothing else of the matrix-core chain.
        deemph_state: float per stream, the de-emphasis state in front of the first call (csdr_amd_wfm_set_deemphasis_state).  repeat_after_reset: the whole
        schedule runs a second time behind csdr_amd_wfm_reset (rates and state put back as at the start); that run's (s16, float) are left in `self.wfm_repeat`.
        The front-end kernel of the last call is left in `self.last_wfm_kernel`, the seed tables' counters (_seed_stats) in `self.wfm_seed_stats`, the route of the
        de-emphasis (csdr_amd_wfm_exact_deemphasis) in `self.last_wfm_exact`."""
        x2, squeeze = self._2d(iq_u8, np.uint8)
        s, nbytes = x2.shape; n = nbytes // 2
        pitch = (nbytes + 15) // 16 * 16 + pitch_pad
        xx = np.zeros((s, pitch), np.uint8); xx[:, :nbytes] = x2
        taps = np.ascontiguousarray(taps, f32)
        sched = list(block) if isinstance(block, (list, tuple)) else None
        block = n if block is None else (max(sched) if sched else block)
        cap = max(block, 1024) if max_block is None else int(max_block)
        ps = np.ndim(shift_rate) != 0
        if not ps:
            w = self.L.csdr_amd_wfm_create(self.h, s, shift_rate, decimation, _hp(taps), taps.size, frac_rate, tau, audio_rate, cap)
        else:
            rates = np.ascontiguousarray(shift_rate, f32); assert rates.size == s
            w = self.L.csdr_amd_wfm_create_rates(self.h, s, _hp(rates), decimation, _hp(taps), taps.size, frac_rate, tau, audio_rate, cap)
        with _Handle(self, "wfm", w) as w:
            di = self.upload(xx)
            apitch = (n // (decimation * frac_rate) + 64 + 63) // 64 * 64
            ds = self.alloc(2 * s * apitch); df = self.alloc(4 * s * apitch) if want_float else None
            stats = None

            def run():
                nonlocal stats
                pos = 0; na = 0; call = 0; parts_s = []; parts_f = []
                if deemph_state is not None:
                    st0 = np.ascontiguousarray(deemph_state, f32); assert st0.size == s
                    w._call("set_deemphasis_state", _hp(st0))
                while pos < n:
                    for st, r in (retunes or {}).get(call, []):
                        w._call("set_rate", st, r)
                    k = min(sched[call] if (sched and call < len(sched)) else block, n - pos); call += 1
                    if out_per_call:
                        got = w._call("process", di.at(2 * pos), pitch, k, ds.ptr, df.ptr if want_float else None, apitch)
                        parts_s.append(self.download(ds, np.int16, s * apitch).reshape(s, apitch)[:, :got].copy())
                        if want_float: parts_f.append(self.download(df, f32, s * apitch).reshape(s, apitch)[:, :got].copy())
                    else:
                        got = w._call("process", di.at(2 * pos), pitch, k, ds.at(2 * na), df.at(4 * na) if want_float else None, apitch)
                    stats = self._seed_stats("wfm", w.h, ps, stats, call - 1)
                    pos += k; na += got
                if out_per_call:
                    s16 = np.concatenate(parts_s, axis=1) if parts_s else np.zeros((s, 0), np.int16)
                    af = np.concatenate(parts_f, axis=1) if parts_f else np.zeros((s, 0), f32)
                else:
                    s16 = self.download(ds, np.int16, s * apitch).reshape(s, apitch)[:, :na].copy()
                    af = self.download(df, f32, s * apitch).reshape(s, apitch)[:, :na].copy() if want_float else np.zeros((s, 0), f32)
                return s16, af
            s16, af = run()
            if repeat_after_reset:
                w.reset()
                if ps:
                    for st in range(s):
                        w._call("set_rate", st, float(rates[st]))
                self.wfm_repeat = run()
            if hasattr(self.L, "csdr_amd_wfm_exact_deemphasis"):
                self.last_wfm_exact = int(self.L.csdr_amd_wfm_exact_deemphasis(w.h))
            self.last_wfm_kernel = w.kernel_name(); self.wfm_seed_stats = stats
        return (s16[0].copy(), af[0].copy()) if squeeze else (s16.copy(), af.copy())

    def ddc_u8(self, iq_u8, shift_rate, decimation, taps, block=None, pitch_pad=0, retunes=None, max_block=None, reset_at=None):
        """Fused front end convert_u8_f | shift_addition_cc | fir_decimate_cc (csdr_amd_ddc_*): iq_u8 [2n] or [streams, 2n] uint8 ->
        complex64 [streams, n_out].  `block` = samples per call; `pitch_pad` = extra bytes of row pitch (a pitch that is not a multiple of
        128 selects the plain kernel).  The kernel of the last call is left in `self.last_ddc_kernel`, all kernels used in `self.ddc_kernels`, the set of the
        calls' dispatch reports (csdr_amd_ddc_last_instance) in `self.ddc_instances`.
        shift_rate: one float, or one per stream (csdr_amd_ddc_create_rates); retunes: {call index: [(stream, rate), ...]} applied in front of that call.
        max_block: the object's max_block_samples (default: the largest call) -- it sizes the chunk-seed tables, nothing else.  reset_at: csdr_amd_ddc_reset in front of
        that call (the outputs of the stream that starts there follow the others; their first index is left in `self.ddc_reset_out`).
        The seed tables' counters (_seed_stats) are left in `self.ddc_seed_stats`, the position of every call's first output in `self.ddc_call_out`."""
        x2, squeeze = self._2d(iq_u8, np.uint8)
        s, nbytes = x2.shape; n = nbytes // 2
        pitch = (nbytes + 127) // 128 * 128 + pitch_pad
        xx = np.full((s, pitch), 0x80, np.uint8); xx[:, :nbytes] = x2
        taps = np.ascontiguousarray(taps, f32)
        sched = list(block) if isinstance(block, (list, tuple)) else None          # `block` may be a list of call sizes (the rest of the stream follows in one call)
        block = n if block is None else (max(sched) if sched else block)
        cap = max(block, 1024) if max_block is None else int(max_block)
        ps = np.ndim(shift_rate) != 0
        if not ps:
            d = self.L.csdr_amd_ddc_create(self.h, s, shift_rate, decimation, _hp(taps), taps.size, cap)
        else:
            rates = np.ascontiguousarray(shift_rate, f32); assert rates.size == s
            d = self.L.csdr_amd_ddc_create_rates(self.h, s, _hp(rates), decimation, _hp(taps), taps.size, cap)
        with _Handle(self, "ddc", d) as d:
            di = self.upload(xx)
            opitch = n // decimation + 64
            do = self.alloc(8 * s * opitch)
            pos = 0; no = 0; self.ddc_kernels = set(); self.ddc_instances = set(); call = 0; stats = None; self.ddc_call_out = []; self.ddc_reset_out = None
            while pos < n:
                if reset_at is not None and call == reset_at:
                    d.reset(); self.ddc_reset_out = no
                for st, r in (retunes or {}).get(call, []):
                    d._call("set_rate", st, r)
                k = min(sched[call] if (sched and call < len(sched)) else block, n - pos); call += 1
                got = d._call("process", di.at(2 * pos), pitch, k, do.at(8 * no), opitch)
                self.ddc_kernels.add(d.kernel_name())
                self.ddc_instances.add(self.L.csdr_amd_ddc_last_instance(d.h).decode())
                stats = self._seed_stats("ddc", d.h, ps, stats, call - 1)
                self.ddc_call_out.append(no)
                pos += k; no += got
            y = self.download(do, c64, s * opitch).reshape(s, opitch)[:, :no]
            self.last_ddc_kernel = d.kernel_name(); self.ddc_seed_stats = stats
        return y[0].copy() if squeeze else y.copy()

    def wfm_ring_chain(self, iq_u8, shift_rate, decimation, taps, block=16384, n_slots=8, frac_rate=5, tau=50e-6, audio_rate=48000, retunes=None, in_flight=None,
                       idle_us=None, life_ms=None, pause_every=None, pause_s=0.0):
        """The resident form (csdr_amd_wfm_ring_*): iq_u8 [streams, 2n] uint8, n a multiple of `block` -> s16 [streams, na] (all blocks' audio in stream order).
        Blocks are copied into the input ring slot by slot (hipMemcpy H2D), posted, and collected `in_flight` (default n_slots - 2) blocks later.
        retunes: {block index: rate} applied in front of that block.  pause_every / pause_s: sleep so long every so many blocks (the grid leaves and is relaunched).
        Leaves (launches, grid) in self.last_ring."""
        import time
        x2, squeeze = self._2d(iq_u8, np.uint8)
        s, nbytes = x2.shape; n = nbytes // 2
        assert n % block == 0
        nb = n // block
        taps = np.ascontiguousarray(taps, f32)
        with _Handle(self, "wfm_ring", self.L.csdr_amd_wfm_ring_create(self.h, s, shift_rate, decimation, _hp(taps), taps.size, frac_rate, tau, audio_rate, block,
                                                                       n_slots)) as ring:
            r = ring.h
            if idle_us is not None or life_ms is not None:
                self.check(self.L.csdr_amd_wfm_ring_set_timeouts(r, 200.0 if idle_us is None else idle_us, 250.0 if life_ms is None else life_ms), "ring_set_timeouts")
            depth = (n_slots - 2) if in_flight is None else in_flight
            outs = []; pitch = C.c_size_t(0); opitch = C.c_size_t(0)

            def collect(k):
                na = self.check(self.L.csdr_amd_wfm_ring_wait(r, k, 0.0), "ring_wait")
                po = self.L.csdr_amd_wfm_ring_output(r, k, C.byref(opitch))
                buf = np.empty((s, opitch.value), np.int16)
                self.check(self.L.csdr_amd_d2h(self.h, _hp(buf), po, buf.nbytes), "d2h")
                outs.append(buf[:, :na].copy())
            for k in range(nb):
                if retunes and k in retunes:
                    while len(outs) < k:
                        collect(len(outs))
                    self.check(self.L.csdr_amd_wfm_ring_set_rate(r, retunes[k]), "ring_set_rate")
                if pause_every and k and k % pause_every == 0:
                    time.sleep(pause_s)
                self.check(self.L.csdr_amd_wfm_ring_acquire(r, k, 0.0), "ring_acquire")
                pi = self.L.csdr_amd_wfm_ring_input(r, k, C.byref(pitch))
                blk = np.zeros((s, pitch.value), np.uint8); blk[:, :2 * block] = x2[:, 2 * k * block:2 * (k + 1) * block]
                self.check(self.L.csdr_amd_h2d(self.h, pi, _hp(blk), blk.nbytes), "h2d")
                got = self.L.csdr_amd_wfm_ring_submit(r)
                if got != k:
                    raise CsdrAmdError("ring_submit: %d (%s)" % (got, self.err()))
                while len(outs) + depth <= k:
                    collect(len(outs))
            while len(outs) < nb:
                collect(len(outs))
            self.last_ring = {"launches": self.L.csdr_amd_wfm_ring_launches(r), "grid": self.L.csdr_amd_wfm_ring_grid(r)}
        y = np.concatenate(outs, axis=1)
        return y[0].copy() if squeeze else y

    def nfm_chain(self, iq_u8, shift_rate, decimation=50, tbw=0.005, audio_rate=48000, agc_block=1024, block=None, retunes=None, max_block=None):
        """BASELINE config 5 / README.md:87 through the chain object csdr_amd_nfm_* (matrix-core front end + audio-rate back end):
        iq_u8 [streams, 2n] uint8 -> (s16 [streams, na], float audio [streams, na]); `block` = samples per call.
        shift_rate: one float, or one per stream (csdr_amd_nfm_create_rates); retunes: {call index: [(stream, rate), ...]}.  The set of the front end's
        dispatch reports (csdr_amd_ddc_last_instance) is left in `self.ddc_instances`, its seed tables' counters (_seed_stats) in `self.ddc_seed_stats`.
        max_block: the object's max_block_samples (default: the largest call) -- it sizes the chunk-seed tables and the back end's buffers."""
        x2, squeeze = self._2d(iq_u8, np.uint8)
        S, nbytes = x2.shape; n = nbytes // 2
        pitch = (nbytes + 127) // 128 * 128
        xx = np.full((S, pitch), 0x80, np.uint8); xx[:, :nbytes] = x2
        nt = self.firdes_filter_len(tbw)
        taps = np.ascontiguousarray(self.firdes_lowpass_f(nt, 0.5 / decimation), f32)
        sched = list(block) if isinstance(block, (list, tuple)) else None
        block = n if block is None else (max(sched) if sched else block)
        cap = max(block, 1024) if max_block is None else int(max_block)
        ps = np.ndim(shift_rate) != 0
        if not ps:
            w = self.L.csdr_amd_nfm_create(self.h, S, shift_rate, decimation, _hp(taps), taps.size, audio_rate, agc_block, 1.0, 1.0, cap)
        else:
            rates = np.ascontiguousarray(shift_rate, f32); assert rates.size == S
            w = self.L.csdr_amd_nfm_create_rates(self.h, S, _hp(rates), decimation, _hp(taps), taps.size, audio_rate, agc_block, 1.0, 1.0, cap)
        with _Handle(self, "nfm", w) as w:
            di = self.upload(xx)
            apitch = n // decimation + 1024 + 64
            ds = self.alloc(2 * S * apitch); df = self.alloc(4 * S * apitch)
            pos = 0; na = 0; call = 0; self.ddc_instances = set(); stats = None
            while pos < n:
                for st, r in (retunes or {}).get(call, []):
                    w._call("set_rate", st, r)
                k = min(sched[call] if (sched and call < len(sched)) else block, n - pos); call += 1
                got = w._call("process", di.at(2 * pos), pitch, k, ds.at(2 * na), df.at(4 * na), apitch)
                self.ddc_instances.add(self.L.csdr_amd_ddc_last_instance(w._fn("front_end")(w.h)).decode())
                stats = self._seed_stats("ddc", w._fn("front_end")(w.h), ps, stats, call - 1)
                pos += k; na += got
            pcm = self.download(ds, np.int16, S * apitch).reshape(S, apitch)[:, :na]
            af = self.download(df, f32, S * apitch).reshape(S, apitch)[:, :na]
            self.last_ddc_kernel = self.L.csdr_amd_ddc_kernel_name(w._fn("front_end")(w.h)).decode(); self.ddc_seed_stats = stats
        return (pcm[0].copy(), af[0].copy()) if squeeze else (pcm.copy(), af.copy())

    def nfm_chain_unfused(self, iq_u8, shift_rate, decimation=50, tbw=0.005, audio_rate=48000, agc_block=1024):
        """BASELINE config 5 / README.md:87, stage by stage through the device batch API with the data resident on the GPU between
        stages: convert_u8_f | shift_addition_cc | fir_decimate_cc D tbw HAMMING | fmdemod_quadri_cf | limit_ff | deemphasis_nfm_ff |
        fastagc_ff | convert_f_s16.   iq_u8: [streams, 2n] uint8  ->  (s16 [streams, na], float audio [streams, na])."""
        x2, squeeze = self._2d(iq_u8, np.uint8)
        S, nbytes = x2.shape; n = nbytes // 2
        L = self.L
        d_u8 = self.upload(x2)
        d_f = self.alloc(4 * S * nbytes + 64)
        self.check(L.csdr_amd_convert_u8_f(self.h, d_u8.ptr, d_f.ptr, S * nbytes), "convert_u8_f")
        d_sh = self.alloc(8 * S * n + 64)
        ph = C.c_float(0.0)
        self.check(L.csdr_amd_shift_cc(self.h, SHIFT["addition"], shift_rate, C.byref(ph), d_f.ptr, d_sh.ptr, S, n, n, n, 1024, 0), "shift")
        nt = self.firdes_filter_len(tbw)
        taps = self.upload(self.firdes_lowpass_f(nt, 0.5 / decimation))
        pd = n // decimation + 2
        d_dec = self.alloc(8 * S * pd + 64)
        nd = self.check(L.csdr_amd_fir_decimate_cc(self.h, d_sh.ptr, d_dec.ptr, S, n, n, pd, decimation, taps.ptr, nt), "fir_decimate_cc")
        d_dem = self.alloc(4 * S * pd + 64); d_last = self.upload(np.zeros(S, c64))
        self.check(L.csdr_amd_fmdemod_quadri_cf(self.h, d_dec.ptr, d_dem.ptr, S, nd, pd, pd, d_last.ptr), "fmdemod")
        pre = 1024                         # `csdr deemphasis_nfm_ff` filters  the_bufsize zeros ++ stream  (csdr.c:1076-1081)
        pd2 = pd + pre
        d_lim0 = self.alloc(4 * S * pd + 64)
        self.check(L.csdr_amd_limit_ff(self.h, d_dem.ptr, d_lim0.ptr, S * pd, 1.0), "limit")
        lim = np.zeros((S, pd2), f32); lim[:, pre:] = self.download(d_lim0, f32, S * pd).reshape(S, pd)
        d_lim = self.upload(lim)
        dtaps_h = self.nfm_taps(audio_rate)
        d_dt = self.upload(dtaps_h)
        d_de = self.alloc(4 * S * pd2 + 64)
        ne = self.check(L.csdr_amd_fir_ff(self.h, d_lim.ptr, d_de.ptr, S, nd + pre, pd2, pd2, d_dt.ptr, dtaps_h.size), "deemphasis_nfm")
        nb = ne // agc_block
        d_agc = self.alloc(4 * S * pd2 + 64)
        d_st = self.upload(np.zeros(S * (2 * agc_block + 4), f32))
        self.check(L.csdr_amd_fastagc_ff(self.h, d_de.ptr, d_agc.ptr, S, nb, agc_block, pd2, pd2, 1.0, d_st.ptr), "fastagc")
        na = nb * agc_block
        d_pcm = self.alloc(2 * S * pd2 + 64)
        self.check(L.csdr_amd_convert_f_s16(self.h, d_agc.ptr, d_pcm.ptr, S * pd2), "convert_f_s16")
        af = self.download(d_agc, f32, S * pd2).reshape(S, pd2)[:, :na]
        pcm = self.download(d_pcm, np.int16, S * pd2).reshape(S, pd2)[:, :na]
        return (pcm[0].copy(), af[0].copy()) if squeeze else (pcm.copy(), af.copy())


SHARD = {"channels": 0, "blocks": 1}


def _bank_input(x):
    """the wideband stream as the bank takes it: (array, entry-point suffix, bytes per complex sample)"""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return np.ascontiguousarray(x), "_s16", 4
    if x.dtype == np.uint8:
        return np.ascontiguousarray(x), "_u8", 2
    return np.ascontiguousarray(x, c64), "", 8


def sharded_bank_loopback(world, x, tbw, decimation, shift_rates, schedule, mode="blocks", window="HAMMING", retunes=None, pipelined=True,
                          local_input=False, device=0, retune_while_staged=False, superseded_retune=False):
    """The multi-rank fastddc bank (csdr_amd_fastddc_bank_create_sharded_by) run for real on ONE GPU: `world` rank threads, one Context each, joined by the
    library's loopback communicator (every exchange = stream-ordered device copies).  x = the wideband stream (on rank 0; local_input: every rank is handed
    its own run of each batch instead), schedule = blocks per batch, retunes = {batch index: [(global channel, rate), ...]} applied before that batch.
    pipelined: submit(k + 1) is queued before collect(k) wherever no retune sits in between -- or, with retune_while_staged, everywhere: batch k + 1's retunes are
    then issued while batch k is still staged (they must leave batch k alone and apply from batch k + 1 on, in both sharding modes).  superseded_retune (with
    retune_while_staged, unpipelined): the retune issued while batch k is staged goes to a DECOY rate and the real one follows after collect(k), when nothing is
    staged -- the held-back decoy must not be replayed on top of it at collect(k + 1).  Returns the per-channel outputs (all channels, gathered from the ranks' slices)."""
    import threading
    L = lib()
    x, sfx, es = _bank_input(x)                          # complex64, or interleaved IQ as int16 / uint8 (the _s16 / _u8 entry points: the raw integers are scattered)
    spc = 1 if es == 8 else 2                            # array elements per complex sample
    rates = np.ascontiguousarray(shift_rates, f32); nc = rates.size
    retunes = retunes or {}
    outs = [None] * nc
    errors = []

    def rank_main(rank):
        ctx = None
        try:
            ctx = Context(device)
            with _Handle(ctx, "comm", L.csdr_amd_comm_create_loopback(ctx.h, grp.h, rank)) as comm, \
                 _Handle(ctx, "fastddc_bank", L.csdr_amd_fastddc_bank_create_sharded_by(ctx.h, tbw, decimation, _hp(rates), nc, WINDOWS[window], max(schedule),
                                                                                        comm.h, SHARD[mode])) as bank:      # (left bank first, then comm)
                first = C.c_int(); count = C.c_int()
                L.csdr_amd_fastddc_bank_channel_slice(bank.h, C.byref(first), C.byref(count))
                first, count = first.value, count.value
                inp = L.csdr_amd_fastddc_bank_input_size(bank.h); ovl = L.csdr_amd_fastddc_bank_overlap(bank.h)
                starts = np.concatenate([[0], np.cumsum(schedule)])
                di = ctx.upload(x) if (rank == 0 and not local_input) else None
                mine = [[] for _ in range(count)]
                held = {}

                def submit(k):
                    nb = schedule[k]
                    if local_input:
                        f0 = C.c_int(); n0 = C.c_int()
                        L.csdr_amd_fastddc_bank_local_blocks(bank.h, nb, C.byref(f0), C.byref(n0))
                        a = (starts[k] + f0.value) * inp
                        run = np.zeros((ovl + n0.value * inp) * spc, x.dtype)          # (zeros in front of the stream: exact for complexf and s16)
                        lo = max(0, a - ovl)
                        run[(ovl - (a - lo)) * spc:] = x[lo * spc:(a + n0.value * inp) * spc]
                        held[k] = ctx.upload(run)
                        ctx.check(getattr(L, "csdr_amd_fastddc_bank_submit_local" + sfx)(bank.h, held[k].ptr, nb), "bank_submit_local")
                    else:
                        ctx.check(getattr(L, "csdr_amd_fastddc_bank_submit" + sfx)(bank.h, di.at(es * starts[k] * inp) if di is not None else None, nb), "bank_submit")

                submitted = -1
                for k in range(len(schedule)):
                    if not (retune_while_staged and k > 0):
                        for ch, rt in retunes.get(k, []):
                            ctx.check(L.csdr_amd_fastddc_bank_set_rate_global(bank.h, ch, rt), "bank_set_rate_global")
                    if submitted < k:
                        submit(k); submitted = k
                    if retune_while_staged:                               # batch k is staged, not collected: the next batch's retunes arrive now
                        for ch, rt in retunes.get(k + 1, []):
                            ctx.check(L.csdr_amd_fastddc_bank_set_rate_global(bank.h, ch, rt + 0.0517 if superseded_retune else rt), "bank_set_rate_global")
                    if pipelined and k + 1 < len(schedule) and (retune_while_staged or (k + 1) not in retunes):
                        submit(k + 1); submitted = k + 1
                    pitch = L.csdr_amd_fastddc_bank_max_output(bank.h, schedule[k]) + 8
                    do = ctx.alloc(8 * count * pitch)
                    ctx.check(L.csdr_amd_fastddc_bank_collect(bank.h, do.ptr, pitch, None), "bank_collect")
                    counts = np.zeros(count, np.int32)
                    ctx.check(L.csdr_amd_fastddc_bank_finish(bank.h, _hp(counts)), "bank_finish")
                    if superseded_retune:                                 # nothing is staged now: the real rate, applied at once
                        for ch, rt in retunes.get(k + 1, []):
                            ctx.check(L.csdr_amd_fastddc_bank_set_rate_global(bank.h, ch, rt), "bank_set_rate_global")
                    y = ctx.download(do, c64, count * pitch).reshape(count, pitch)
                    for c in range(count):
                        mine[c].append(y[c, :counts[c]].copy())
                    held.pop(k, None)
                for c in range(count):
                    outs[first + c] = np.concatenate(mine[c])
        except BaseException as e:      # a dead rank must not leave the others waiting at a rendezvous
            errors.append((rank, e))
            L.csdr_amd_loopback_abort(grp.h)
        finally:
            if ctx is not None:
                ctx.close()

    with _Handle(None, "loopback", L.csdr_amd_loopback_create(world)) as grp:
        threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    if errors:
        raise CsdrAmdError("rank %d: %r" % errors[0])
    return outs
