// nfm.hip -- the NFM receive chain (BASELINE config 5, README.md:87) for N independent u8 IQ streams, streaming:
//
//   convert_u8_f | shift_addition_cc r | fir_decimate_cc D tbw HAMMING | fmdemod_quadri_cf | limit_ff | deemphasis_nfm_ff fs | fastagc_ff | convert_f_s16
//
//   front end (2.4 MS/s -> 48 kS/s): csdr_amd_ddc (ddc_mfma.hip), one pass over the input on the matrix cores;
//   back end  (48 kS/s, 1/50 of the input rate): k_nfm_demod_limit (fmdemod_quadri_cf libcsdr.c:1040-1071 + limit_ff :1130-1137 in one
//   pass, appended behind the de-emphasis filter's unconsumed input), the fixed de-emphasis FIR (libcsdr.c:1101-1128, the CLI's re-feed
//   loop csdr.c:1083), fastagc_ff (libcsdr.c:946-991) over whole blocks and convert_f_s16 (:2397).  The de-emphasis filter is run for whole
//   AGC blocks only (its remaining input waits in the carry buffer), so nothing else needs a carry.
//
//   The 201-tap de-emphasis FIR was 80 % of the back end as a float VALU kernel (0.53 ms of 0.66 ms for 512 channels x 1 s: 18 TFLOP/s).  Its
//   input is the LIMITED demodulator output, |x| <= max_amplitude, so 24-bit fixed point represents it to 6e-8 of full scale: the demodulator
//   kernel writes three int8 digit planes instead of floats, and the FIR becomes a banded int8 product on v_mfma_i32_16x16x64_i8 (16 consecutive
//   outputs x 16 channels x 256 inputs per tile, band 93 % dense, one resident weight set): k_nfm_deemph_mfma.  Digit pairs of equal weight
//   share an accumulator; only the (low x low) pair is dropped (2^-31 of full scale).
//   The back end's kernels live in nfm_dev.hpp, which csdr_amd_fmrx (fmrx.hip: the same tail on complexf baseband) includes as well.
#include "nfm_dev.hpp"
#include <string.h>
#include <string>
using namespace csdr_amd;

namespace {

// k_nfm_demod_limit for the outputs the fused front end left over (DdcFuseInfo): the leading outputs [0, n_lead) (plain kernel), the first output of every segment of the
// matrix-core kernel (its predecessor belongs to another workgroup) and the trailing outputs; y holds these samples and their predecessors.
// Thread 0 of a stream also keeps the call's last sample as the next call's predecessor (two `last` buffers: k_nfm_store_last's work).
__global__ __launch_bounds__(64) void k_nfm_demod_boundary(const cf32 *__restrict__ y, size_t y_pitch, const cf32 *__restrict__ last, cf32 *__restrict__ last_out, int n_y,
                                                           DdcFuseInfo info, DdcFuse f)
{
    const int s = blockIdx.y, j = blockIdx.x * 64 + threadIdx.x;
    if (j == 0) last_out[s] = y[(size_t)s * y_pitch + n_y - 1];
    long k;
    if (j < info.n_lead) k = j;
    else if (j < info.n_lead + info.n_seg) { k = info.seg_first + (long)(j - info.n_lead) * info.seg_outputs; if (k < info.n_lead) return; }      // (a partial first tile: the lead covers output 0)
    else if (j < info.n_lead + info.n_seg + info.n_trail) k = info.trail_first + (j - info.n_lead - info.n_seg);
    else return;
    const cf32 *src = y + (size_t)s * y_pitch;
    const cf32 x = src[k];
    const cf32 p = k ? src[k - 1] : last[s];
    int d[3]; nfm_demod_digits(make_float2(x.i, x.q), make_float2(p.i, p.q), f.max_amp, f.q_per_amp, d);
    int8_t *dst = f.planes + (size_t)s * f.dl_pitch + f.dl_fill + k;
    dst[0] = (int8_t)d[0]; dst[f.plane_bytes] = (int8_t)d[1]; dst[2 * f.plane_bytes] = (int8_t)d[2];
}

} // namespace

namespace csdr_amd { long ddc_process_fused(csdr_amd_ddc *d, const uint8_t *in, size_t in_pitch, size_t block_samples, csdr_complexf *out, size_t out_pitch, const DdcFuse *fuse, DdcFuseInfo *info); }

struct csdr_amd_nfm {
    csdr_amd_ctx *ctx;
    int n_streams, D, Ld, agc_block, cli_prefix;
    float limit, agc_ref;
    DevBuf<cf32> d_y; size_t y_pitch; DevBuf<cf32> d_last, d_last2; int lflip;
    DevBuf<int8_t> d_planes; size_t plane_bytes; size_t dl_pitch; int dl_fill;   // limited demodulator output (three digit planes) waiting for the de-emphasis filter
    DevBuf<> d_fir_frags; float fir_scale;            // de-emphasis taps as int8 digit fragments; scale of the recombined product
    DevBuf<float> d_de; size_t a_pitch;             // de-emphasised blocks
    DevBuf<float> d_agc_state;
    size_t max_y;
    bool fuse_off;                                  // CSDR_AMD_NFM_FUSE=0 (A/B: separate demodulator / AGC-peak passes), read when the object is created
    Owned<csdr_amd_ddc, csdr_amd_ddc_destroy> ddc;  // the receiver front end
};

extern "C" {

static csdr_amd_nfm *nfm_create_impl(csdr_amd_ctx *ctx, int n_streams, const float *rates, bool per_stream, int decimation, const float *host_taps, int taps_length,
                                     int audio_rate, int agc_block, float agc_reference, float limit_max, size_t max_block_samples)
{
    if (!ctx || n_streams < 1 || agc_block < 1 || agc_block > 2048 - 512 || (agc_block % 16) || !(limit_max > 0)) { fail_msg(-3, "nfm_create: bad arguments (agc_block: multiple of 16 up to 1536; limit > 0)"); return nullptr; }
    const float *dt = nullptr;
    const int Ld = csdr_amd_nfm_deemph_taps(audio_rate, &dt);
    if (!Ld) { fail_msg(-3, "nfm_create: no de-emphasis table for sample rate %d (libcsdr.c:1115-1119)", audio_rate); return nullptr; }
    if (Ld + 15 > 64 * NFM_FIR_NK) { fail_msg(-3, "nfm_create: %d de-emphasis taps exceed the matrix-core tile", Ld); return nullptr; }
    if (max_block_samples < 1024) max_block_samples = 1024;
    Owned<csdr_amd_nfm, csdr_amd_nfm_destroy> w(new csdr_amd_nfm());
    w->ctx = ctx; w->n_streams = n_streams; w->D = decimation; w->Ld = Ld; w->agc_block = agc_block; w->limit = limit_max; w->agc_ref = agc_reference;
    w->ddc.reset(per_stream ? csdr_amd_ddc_create_rates(ctx, n_streams, rates, decimation, host_taps, taps_length, max_block_samples)
                            : csdr_amd_ddc_create(ctx, n_streams, rates[0], decimation, host_taps, taps_length, max_block_samples));
    if (!w->ddc) return nullptr;
    { const char *fe = getenv("CSDR_AMD_NFM_FUSE"); w->fuse_off = fe && atoi(fe) == 0; }
    w->max_y = max_block_samples / decimation + 2;
    w->y_pitch = (w->max_y + 15) & ~(size_t)15;
    // The reference's `csdr deemphasis_nfm_ff` runs its FIR over its freshly allocated buffer before it reads anything (csdr.c:1076-1081: `processed`
    // starts at 0, the first fread is empty): its output is the FIR of  the_bufsize zeros ++ stream.  The chain object reproduces the pipeline
    // at the default buffer size (1024, csdr.c:189).
    w->cli_prefix = 1024;
    w->dl_pitch = (w->max_y + Ld + agc_block + w->cli_prefix + NFM_FIR_ROW + 63) & ~(size_t)63;        // + the last workgroup's staged span beyond the valid samples (zero weights)
    w->a_pitch = (w->max_y + Ld + agc_block + 1024 + 15) & ~(size_t)15;
    hipError_t e = hipSuccess;
    auto alloc = [&](auto &p, size_t bytes) { if (e == hipSuccess) e = dev_alloc(p, bytes); };
    alloc(w->d_y, sizeof(cf32) * w->y_pitch * n_streams);
    alloc(w->d_last, sizeof(cf32) * n_streams);
    alloc(w->d_last2, sizeof(cf32) * n_streams);
    w->plane_bytes = w->dl_pitch * n_streams;
    alloc(w->d_planes, 3 * w->plane_bytes);
    alloc(w->d_fir_frags, (size_t)NFM_FIR_NK * 3 * 64 * 16);
    alloc(w->d_de, sizeof(float) * w->a_pitch * n_streams);
    alloc(w->d_agc_state, sizeof(float) * (size_t)n_streams * (2 * agc_block + 4));
    {
        std::vector<int8_t> fr;
        w->fir_scale = nfm_fir_table(dt, Ld, limit_max, fr);
        if (e == hipSuccess) e = hipMemcpy(w->d_fir_frags.get(), fr.data(), fr.size(), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) { fail(e, "hipMalloc/hipMemcpy(nfm state)", __FILE__, __LINE__); return nullptr; }
    if (csdr_amd_nfm_reset(w.get())) return nullptr;
    return w.release();
}

csdr_amd_nfm *csdr_amd_nfm_create(csdr_amd_ctx *ctx, int n_streams, float shift_rate, int decimation, const float *host_taps, int taps_length,
                                  int audio_rate, int agc_block, float agc_reference, float limit_max, size_t max_block_samples)
{
    return nfm_create_impl(ctx, n_streams, &shift_rate, false, decimation, host_taps, taps_length, audio_rate, agc_block, agc_reference, limit_max, max_block_samples);
}

csdr_amd_nfm *csdr_amd_nfm_create_rates(csdr_amd_ctx *ctx, int n_streams, const float *shift_rates, int decimation, const float *host_taps, int taps_length,
                                        int audio_rate, int agc_block, float agc_reference, float limit_max, size_t max_block_samples)
{
    if (!shift_rates) { fail_msg(-3, "nfm_create_rates: no rates"); return nullptr; }
    return nfm_create_impl(ctx, n_streams, shift_rates, true, decimation, host_taps, taps_length, audio_rate, agc_block, agc_reference, limit_max, max_block_samples);
}

int csdr_amd_nfm_set_rate(csdr_amd_nfm *w, int stream, float shift_rate) { return csdr_amd_ddc_set_rate(w->ddc.get(), stream, shift_rate); }

void csdr_amd_nfm_destroy(csdr_amd_nfm *w)
{
    if (!w) return;
    (void)hipStreamSynchronize(w->ctx->stream);
    delete w;
}

int csdr_amd_nfm_reset(csdr_amd_nfm *w)
{
    hipStream_t st = w->ctx->stream;
    w->dl_fill = w->cli_prefix;                                                                                // zeros (the planes are cleared below): see csdr_amd_nfm_create
    CSDR_HIP(hipMemsetAsync(w->d_planes.get(), 0, 3 * w->plane_bytes, st));                                          // bytes behind the valid samples meet zero weights, but must be initialised
    CSDR_HIP(hipMemsetAsync(w->d_last.get(), 0, sizeof(cf32) * w->n_streams, st));                                   // the CLI starts fmdemod from (0, 0) (csdr.c:1044)
    CSDR_HIP(hipMemsetAsync(w->d_last2.get(), 0, sizeof(cf32) * w->n_streams, st)); w->lflip = 0;
    CSDR_HIP(hipMemsetAsync(w->d_agc_state.get(), 0, sizeof(float) * (size_t)w->n_streams * (2 * w->agc_block + 4), st));   // calloc'ed fastagc state (csdr.c:1393-1394)
    return csdr_amd_ddc_reset(w->ddc.get());
}

csdr_amd_ddc *csdr_amd_nfm_front_end(csdr_amd_nfm *w) { return w->ddc.get(); }

long csdr_amd_nfm_process(csdr_amd_nfm *w, const uint8_t *in, size_t in_pitch, size_t block_samples, int16_t *audio_s16, float *audio_f, size_t out_pitch)
{
    csdr_amd_ctx *c = w->ctx; hipStream_t st = c->stream;
    const int S = w->n_streams;
    // front end; on its matrix-core path the reducer epilogue demodulates, limits and writes the digit planes itself (the decimated complex stream never goes
    // to HBM: only the samples at workgroup / kernel boundaries do, for k_nfm_demod_boundary).  CSDR_AMD_NFM_FUSE=0: the separate pass over y.
    const bool fuse_off = w->fuse_off;
    DdcFuse fz; fz.planes = w->d_planes.get(); fz.plane_bytes = w->plane_bytes; fz.dl_pitch = w->dl_pitch; fz.dl_fill = w->dl_fill; fz.max_amp = w->limit; fz.q_per_amp = NFM_XQ / w->limit;
    DdcFuseInfo fi; memset(&fi, 0, sizeof fi);
    const long n_y = ddc_process_fused(w->ddc.get(), in, in_pitch, block_samples, w->d_y.get(), w->y_pitch, fuse_off ? nullptr : &fz, &fi);
    if (n_y < 0) return n_y;
    if (n_y == 0) return 0;
    if ((size_t)n_y > w->max_y) return fail_msg(-3, "nfm: front end produced more than the planned %zu samples", w->max_y);
    cf32 *last_in = w->lflip ? w->d_last2.get() : w->d_last.get(), *last_out = w->lflip ? w->d_last.get() : w->d_last2.get();
    if (fi.fused) {
        const long nb_out = fi.n_lead + fi.n_seg + fi.n_trail;
        hipLaunchKernelGGL(k_nfm_demod_boundary, dim3(cdiv(nb_out > 0 ? nb_out : 1, 64), S), dim3(64), 0, st, w->d_y.get(), w->y_pitch, last_in, last_out, (int)n_y, fi, fz);
        CSDR_LAUNCH_CHECK();
    } else {
        // fmdemod_quadri_cf | limit_ff, appended behind the filter's unconsumed input
        hipLaunchKernelGGL(k_nfm_demod_limit, dim3(cdiv(n_y, 256), S), dim3(256), 0, st, w->d_y.get(), w->y_pitch, (int)n_y, last_in, w->d_planes.get(), w->plane_bytes, w->dl_pitch, w->dl_fill, w->limit, NFM_XQ / w->limit);
        CSDR_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_nfm_store_last, dim3(cdiv(S, 64)), dim3(64), 0, st, w->d_y.get(), w->y_pitch, (int)n_y, last_out, S);
        CSDR_LAUNCH_CHECK();
    }
    w->lflip ^= 1;
    const int n_in = w->dl_fill + (int)n_y;
    // deemphasis_nfm_ff produces input - taps outputs (libcsdr.c:1121); run it for whole AGC blocks only
    const int ne_all = n_in - w->Ld;
    const int nb = ne_all > 0 ? ne_all / w->agc_block : 0;
    const int ne = nb * w->agc_block;
    if (nb > 0) {
        if ((size_t)ne > out_pitch && S > 1) return fail_msg(-3, "nfm: out_pitch %zu smaller than the %d audio samples of this block", out_pitch, ne);
        {
            const int n_tiles = ne / 16, n_sb = (S + 15) / 16;
            const int gx = (n_tiles + NFM_FIR_SPAN - 1) / NFM_FIR_SPAN;
            // fastagc's peak pass rides in the de-emphasis kernel when an AGC block is exactly a workgroup's span
            const bool fuse_peaks = w->agc_block == 16 * NFM_FIR_SPAN && !fuse_off;
            float *peaks = fuse_peaks ? fastagc_peaks_buffer(c, S, nb) : nullptr;
            if (fuse_peaks && !peaks) return -2;
            hipLaunchKernelGGL(k_nfm_deemph_mfma, dim3(gx, n_sb), dim3(256), 0, st, w->d_planes.get(), w->plane_bytes, w->dl_pitch, (const v4i *)w->d_fir_frags.get(), w->fir_scale,
                               w->d_de.get(), w->a_pitch, n_tiles, S, peaks, nb + 2);
            CSDR_LAUNCH_CHECK();
            // fastagc_ff | convert_f_s16 in one pass (the float audio is written only when the caller wants the parity tap)
            int rc = fastagc_ff_s16(c, w->d_de.get(), audio_f, audio_s16, S, nb, w->agc_block, w->a_pitch, out_pitch, out_pitch, w->agc_ref, w->d_agc_state.get(), fuse_peaks);
            if (rc) return rc;
        }
    }
    // keep the unconsumed filter input in front
    const int rem = n_in - ne;
    if (ne > 0 && rem > 0) {
        if (rem > 2048) return fail_msg(-3, "nfm: internal carry of %d samples", rem);
        hipLaunchKernelGGL(k_nfm_move_front_planes, dim3(S, 3), dim3(256), 0, st, w->d_planes.get(), w->plane_bytes, w->dl_pitch, ne, rem);
        CSDR_LAUNCH_CHECK();
    }
    w->dl_fill = rem;
    return ne;
}

} // extern "C"

// Test hook (tests/test_abi_cpu.py): ONE tile of k_nfm_deemph_mfma on the CPU -- the digit planes of 256 limited samples (as k_nfm_demod_limit
// stores them), the Toeplitz digit table and the four accumulator classes, exactly as the kernel combines them.  x: 256 floats, |x| <= max_amp;
// out16: the 16 outputs out[i] = sum_t taps[t] x[i + t].
extern "C" int csdr_amd_debug_nfm_deemph_tile(int audio_rate, float max_amp, const float *x, float *out16)
{
    const float *dt = nullptr;
    const int Ld = csdr_amd_nfm_deemph_taps(audio_rate, &dt);
    if (!Ld || Ld + 15 > 64 * NFM_FIR_NK || !(max_amp > 0)) return -1;
    std::vector<int8_t> fr;
    const float scale = nfm_fir_table(dt, Ld, max_amp, fr);
    const float q_per_amp = NFM_XQ / max_amp;
    int xd[256][3];
    for (int t = 0; t < 256; t++) nfm_sample_digits(x[t], q_per_amp, xd[t]);
    for (int o = 0; o < 16; o++) {
        long acc[4] = {0, 0, 0, 0};
        for (int ks = 0; ks < NFM_FIR_NK; ks++) for (int b = 0; b < 64; b++) {
            const int t = 64 * ks + b;
            int w[3];
            for (int l = 0; l < 3; l++) w[l] = fr[((size_t)(ks * 3 + l) * 64 + (16 * (b / 16) + o)) * 16 + b % 16];
            acc[0] += (long)w[0] * xd[t][0];
            acc[1] += (long)w[0] * xd[t][1] + (long)w[1] * xd[t][0];
            acc[2] += (long)w[0] * xd[t][2] + (long)w[1] * xd[t][1] + (long)w[2] * xd[t][0];
            acc[3] += (long)w[1] * xd[t][2] + (long)w[2] * xd[t][1];
        }
        float v = fmaf((float)acc[0], 256.0f, (float)acc[1]);
        v = fmaf(v, 256.0f, (float)acc[2]);
        v = fmaf(v, 256.0f, (float)acc[3]);
        out16[o] = v * scale;
    }
    return 0;
}

