// nfm_dev.hpp -- the audio-rate back end of the NFM receive chain as kernels: fmdemod_quadri_cf | limit_ff into three int8 digit planes, the de-emphasis FIR as a
// banded int8 product on v_mfma_i32_16x16x64_i8, the carry of the filter's unconsumed input, and the host's digit table.  Shared by the two objects that launch
// them: csdr_amd_nfm (nfm.hip, behind its own u8 front end) and csdr_amd_fmrx (fmrx.hip, on complexf baseband): one definition, so both compute the same bits.
#pragma once
#include "common.hpp"
#include "nfm_demod.hpp"
#include <math.h>
#include <vector>

namespace csdr_amd {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
constexpr float NFM_XQ = 8355711.0f;       // 127*65536 + 127*256 + 127: full scale of three balanced base-256 digits
constexpr int NFM_FIR_NK = 4;              // 64-input K-steps per tile of 16 outputs: taps <= 241

// planes: [3][n_streams][dl_pitch] int8 -- digit j of round(v / max_amp * NFM_XQ) = d0 * 65536 + d1 * 256 + d2
__global__ __launch_bounds__(256) void k_nfm_demod_limit(const cf32 *__restrict__ y, size_t y_pitch, int n, const cf32 *__restrict__ last,
                                                         int8_t *__restrict__ planes, size_t plane_bytes, size_t dl_pitch, int dl_fill, float max_amp, float q_per_amp)
{
    const int s = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const cf32 *src = y + (size_t)s * y_pitch;
    const cf32 x = src[k];
    const cf32 p = k ? src[k - 1] : last[s];
    int d[3]; nfm_demod_digits(make_float2(x.i, x.q), make_float2(p.i, p.q), max_amp, q_per_amp, d);
    int8_t *dst = planes + (size_t)s * dl_pitch + dl_fill + k;
    dst[0] = (int8_t)d[0]; dst[plane_bytes] = (int8_t)d[1]; dst[2 * plane_bytes] = (int8_t)d[2];
}

// out[s][i] = sum_t taps[t] x[s][i + t] for i < n_tiles * 16, x given as digit planes.  One workgroup = 16 channels x NFM_FIR_SPAN consecutive
// tiles: the three planes' bytes of that span (+ the 240-sample window tail) are staged in LDS once (consecutive tiles overlap by 240 of
// their 256 inputs; reading the B operands straight from global memory made this kernel L2-bandwidth bound: 1.2 GB of L2 reads for 74 MB of
// planes, 0.16 ms); the 12 weight fragments (4 K-steps x 3 digits of the Toeplitz band) stay in registers; each wave takes every fourth tile.
// MFMA result layout: lane (col, q) holds outputs 4q .. 4q+3 of channel col.
constexpr int NFM_FIR_SPAN = 64;                                   // tiles per workgroup (1024 outputs)
#ifndef NFM_FIR_SUB_N
#define NFM_FIR_SUB_N 32
#endif
constexpr int NFM_FIR_SUB = NFM_FIR_SUB_N;                         // tiles staged at a time: the span in SPAN / SUB passes (64: 61 KiB of LDS, two workgroups per CU; 32: 37 KiB, four)
constexpr int NFM_FIR_ROW = 16 * NFM_FIR_SUB + 64 * NFM_FIR_NK;    // staged bytes per channel and plane
constexpr int NFM_FIR_RP = NFM_FIR_ROW + 16;                       // LDS pitch: odd multiple of 16 bytes (the 16 channels of a B read hit different banks)

// peaks != nullptr (fastagc block = the workgroup's span of 1024 outputs): the workgroup also leaves max |out| of its span per channel at
// peaks[stream * peak_pitch + 2 + blockIdx.x].
__global__ __launch_bounds__(256) void k_nfm_deemph_mfma(const int8_t *__restrict__ planes, size_t plane_bytes, size_t dl_pitch, const v4i *__restrict__ frags,
                                                         float scale, float *__restrict__ out, size_t out_pitch, int n_tiles, int n_streams,
                                                         float *__restrict__ peaks, int peak_pitch)
{
    __shared__ __attribute__((aligned(16))) int8_t lds[3 * 16 * NFM_FIR_RP];
    __shared__ float wpeak[4][16];
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, q = lane >> 4, wv = tid >> 6;
    v4i A[NFM_FIR_NK * 3];
#pragma unroll
    for (int i = 0; i < NFM_FIR_NK * 3; i++) A[i] = frags[i * 64 + lane];
    const int last = n_streams - 1;
    const int stream = (int)blockIdx.y * 16 + col;
    const int8_t *row = lds + col * NFM_FIR_RP + 16 * q;
    float pmax = 0.f;
    for (int sub = 0; sub < NFM_FIR_SPAN / NFM_FIR_SUB; sub++) {
        const int tile0 = blockIdx.x * NFM_FIR_SPAN + sub * NFM_FIR_SUB;
        const int nt = min(NFM_FIR_SUB, n_tiles - tile0);
        if (nt <= 0) break;                                           // (uniform)
        if (sub) __syncthreads();                                     // everyone has read the previous pass's rows
        // stage [3 planes][16 channels][NFM_FIR_ROW] (rows of channels past the last one re-read it; bytes behind the valid samples meet zero weights)
        for (int i = tid; i < 3 * 16 * (NFM_FIR_ROW / 16); i += 256) {
            const int piece = i % (NFM_FIR_ROW / 16), r = (i / (NFM_FIR_ROW / 16)) % 16, pl = i / (16 * (NFM_FIR_ROW / 16));
            const int st = min((int)blockIdx.y * 16 + r, last);
            *reinterpret_cast<v4i *>(lds + (pl * 16 + r) * NFM_FIR_RP + 16 * piece) =
                *reinterpret_cast<const v4i *>(planes + (size_t)pl * plane_bytes + (size_t)st * dl_pitch + (size_t)tile0 * 16 + 16 * piece);
        }
        __syncthreads();
        for (int t = wv; t < nt; t += 4) {
            const int8_t *src = row + 16 * t;
            v4i acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
            for (int ks = 0; ks < NFM_FIR_NK; ks++) {
                const v4i x0 = *reinterpret_cast<const v4i *>(src + 64 * ks), x1 = *reinterpret_cast<const v4i *>(src + 64 * ks + 16 * NFM_FIR_RP),
                          x2 = *reinterpret_cast<const v4i *>(src + 64 * ks + 32 * NFM_FIR_RP);
                const v4i w0 = A[ks * 3], w1 = A[ks * 3 + 1], w2 = A[ks * 3 + 2];
                acc[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w0, x0, acc[0], 0, 0, 0);          // 2^32
                acc[1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w0, x1, acc[1], 0, 0, 0);          // 2^24
                acc[1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w1, x0, acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w0, x2, acc[2], 0, 0, 0);          // 2^16
                acc[2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w1, x1, acc[2], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w2, x0, acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w1, x2, acc[3], 0, 0, 0);          // 2^8
                acc[3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w2, x1, acc[3], 0, 0, 0);
            }
            float4 r;
            float *rv = reinterpret_cast<float *>(&r);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float v = fmaf((float)acc[0][j], 256.0f, (float)acc[1][j]);
                v = fmaf(v, 256.0f, (float)acc[2][j]);
                v = fmaf(v, 256.0f, (float)acc[3][j]);
                rv[j] = v * scale;
            }
            if (stream < n_streams)
                *reinterpret_cast<float4 *>(out + (size_t)stream * out_pitch + 16 * (size_t)(tile0 + t) + 4 * q) = r;
            pmax = fmaxf(fmaxf(pmax, fmaxf(fabsf(r.x), fabsf(r.y))), fmaxf(fabsf(r.z), fabsf(r.w)));
        }
    }
    if (peaks) {                                                      // uniform
        pmax = fmaxf(pmax, __shfl_xor(pmax, 16)); pmax = fmaxf(pmax, __shfl_xor(pmax, 32));      // over q: the channel's outputs of this wave's tiles
        if (q == 0) wpeak[wv][col] = pmax;
        __syncthreads();
        if (tid < 16 && (int)blockIdx.y * 16 + tid < n_streams)
            peaks[(size_t)((int)blockIdx.y * 16 + tid) * peak_pitch + 2 + blockIdx.x] = fmaxf(fmaxf(wpeak[0][tid], wpeak[1][tid]), fmaxf(wpeak[2][tid], wpeak[3][tid]));
    }
}

// k_nfm_deemph_mfma's tile loop and its peak epilogue, statement for statement, as functions for a kernel that stages the rows itself (k_fmrx_front, fmrx.hip).
// k_nfm_deemph_mfma keeps its own body: routed through these functions the compiler schedules it differently, and its machine code is to stay what it was.
// The tiles t = wv, wv + 4, ... < nt of one staged pass (row: this lane's channel and quarter in [3 planes][16 channels][NFM_FIR_RP]): the band product with the
// resident weight fragments A, the recombination of the four accumulator classes, the store of 4 outputs per lane and the running peak |out|.
__device__ __forceinline__ void nfm_deemph_tiles(const int8_t *row, const v4i (&A)[NFM_FIR_NK * 3], float scale, float *out, size_t out_pitch, int stream, int n_streams,
                                                 int tile0, int nt, int wv, int q, float &pmax)
{
    for (int t = wv; t < nt; t += 4) {
        const int8_t *src = row + 16 * t;
        v4i acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
        for (int ks = 0; ks < NFM_FIR_NK; ks++) {
            const v4i x0 = *reinterpret_cast<const v4i *>(src + 64 * ks), x1 = *reinterpret_cast<const v4i *>(src + 64 * ks + 16 * NFM_FIR_RP),
                      x2 = *reinterpret_cast<const v4i *>(src + 64 * ks + 32 * NFM_FIR_RP);
            const v4i w0 = A[ks * 3], w1 = A[ks * 3 + 1], w2 = A[ks * 3 + 2];
            acc[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w0, x0, acc[0], 0, 0, 0);          // 2^32
            acc[1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w0, x1, acc[1], 0, 0, 0);          // 2^24
            acc[1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w1, x0, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w0, x2, acc[2], 0, 0, 0);          // 2^16
            acc[2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w1, x1, acc[2], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w2, x0, acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w1, x2, acc[3], 0, 0, 0);          // 2^8
            acc[3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w2, x1, acc[3], 0, 0, 0);
        }
        float4 r;
        float *rv = reinterpret_cast<float *>(&r);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            float v = fmaf((float)acc[0][j], 256.0f, (float)acc[1][j]);
            v = fmaf(v, 256.0f, (float)acc[2][j]);
            v = fmaf(v, 256.0f, (float)acc[3][j]);
            rv[j] = v * scale;
        }
        if (stream < n_streams)
            *reinterpret_cast<float4 *>(out + (size_t)stream * out_pitch + 16 * (size_t)(tile0 + t) + 4 * q) = r;
        pmax = fmaxf(fmaxf(pmax, fmaxf(fabsf(r.x), fabsf(r.y))), fmaxf(fabsf(r.z), fabsf(r.w)));
    }
}

// max over a workgroup's four waves of the per-lane peaks: the span's peak |out| per channel -> peaks[stream * peak_pitch + 2 + span] (fastagc_ff's first pass,
// libcsdr.c:957-962, without reading the audio back).  wpeak: [4][16] floats of LDS.  Called by every thread.
__device__ __forceinline__ void nfm_store_span_peaks(float pmax, float (*wpeak)[16], int n_streams, float *__restrict__ peaks, int peak_pitch)
{
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, q = lane >> 4, wv = tid >> 6;
    pmax = fmaxf(pmax, __shfl_xor(pmax, 16)); pmax = fmaxf(pmax, __shfl_xor(pmax, 32));      // over q: the channel's outputs of this wave's tiles
    if (q == 0) wpeak[wv][col] = pmax;
    __syncthreads();
    if (tid < 16 && (int)blockIdx.y * 16 + tid < n_streams)
        peaks[(size_t)((int)blockIdx.y * 16 + tid) * peak_pitch + 2 + blockIdx.x] = fmaxf(fmaxf(wpeak[0][tid], wpeak[1][tid]), fmaxf(wpeak[2][tid], wpeak[3][tid]));
}

// Toeplitz band of the de-emphasis taps as three base-256 digits: row o (output), column t (input): taps[t - o]; lane / byte layout of the A
// operand of v_mfma_i32_16x16x64_i8.  Returns the scale of the recombined product:
//   value = (a0 2^24 + a1 2^16 + a2 2^8 + a3) * 2^8 * (gmax / 2^22) * (max_amp / NFM_XQ)
inline float nfm_fir_table(const float *taps, int Ld, float limit_max, std::vector<int8_t> &fr)
{
    fr.assign((size_t)NFM_FIR_NK * 3 * 64 * 16, 0);
    double gmax = 0;
    for (int k = 0; k < Ld; k++) gmax = fmax(gmax, fabs((double)taps[k]));
    gmax *= 1.0001; if (gmax == 0) gmax = 1;
    const double qscale = 4194304.0 / gmax;
    for (int o = 0; o < 16; o++) for (int tp = 0; tp < Ld; tp++) {
        const int t = o + tp, ks = t / 64, b = t % 64;
        long qv = lrint((double)taps[tp] * qscale);
        const int w2 = (int)(((qv + 128) % 256 + 256) % 256) - 128; qv = (qv - w2) / 256;
        const int w1 = (int)(((qv + 128) % 256 + 256) % 256) - 128; qv = (qv - w1) / 256;
        const int dig[3] = {(int)qv, w1, w2};
        for (int l = 0; l < 3; l++) fr[((size_t)(ks * 3 + l) * 64 + (16 * (b / 16) + o)) * 16 + b % 16] = (int8_t)dig[l];
    }
    return (float)(256.0 * (gmax / 4194304.0) * ((double)limit_max / (double)NFM_XQ));
}

// the digits k_nfm_demod_limit stores for a limited sample v (|v| <= max_amp)
inline void nfm_sample_digits(float v, float q_per_amp, int (&d)[3])
{
    int qv = (int)lrintf(v * q_per_amp);
    d[2] = ((qv + 128) & 255) - 128; qv = (qv - d[2]) >> 8;
    d[1] = ((qv + 128) & 255) - 128; qv = (qv - d[1]) >> 8;
    d[0] = qv;
}

// bytes: buf[s][0 .. count) = buf[s][src_off .. src_off + count) on each of the three planes (ranges may overlap; count <= 2048)
__global__ __launch_bounds__(256) void k_nfm_move_front_planes(int8_t *__restrict__ planes, size_t plane_bytes, size_t pitch, int src_off, int count)
{
    int8_t *row = planes + (size_t)blockIdx.y * plane_bytes + (size_t)blockIdx.x * pitch;
    int8_t v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) { const int i = threadIdx.x + 256 * j; v[j] = i < count ? row[src_off + i] : (int8_t)0; }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; j++) { const int i = threadIdx.x + 256 * j; if (i < count) row[i] = v[j]; }
}

__global__ void k_nfm_store_last(const cf32 *__restrict__ y, size_t y_pitch, int n, cf32 *__restrict__ last, int n_streams)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n_streams) last[s] = y[(size_t)s * y_pitch + n - 1];
}

} // namespace
} // namespace csdr_amd
