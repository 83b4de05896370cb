// txmod_dev.hpp -- step functions of the transmit-side modulators, shared by the kernels of txmod.hip, the CPU hook and the drop-in.
//
//   fmmod_fc              libcsdr.c:1180-1192   phase += x PI; while (phase > PI) phase -= 2 PI; while (phase <= -PI) phase += 2 PI; out = (cos, sin)(phase)
//   dsb_fc                csdr.c:2084-2102      out = (x, q_value)
//   add_dcoffset_cc       libcsdr.c:1174-1178   out = (0.5 + i / 2, q / 2)
//   fixed_amplitude_cc    libcsdr.c:1194-1208   gain = |in| > 0 ? amp / |in| : 0; out = in gain
//   convert_f_samplerf    csdr.c:2104-2127      16 bytes per sample: (double)x, wait_for_this_sample, 0
//
// PI is the reference's float constant (libcsdr.h:65), so the phase chain is float32 throughout: one rounded product, one rounded sum, rounded wrap steps.  The
// sources build with -ffp-contract=off: no operation below is fused unless it says fmaf().  The wraps are loops, as in the reference (|x| > 2 takes more than one
// turn), but end after TXMOD_WRAP_MAX turns: a kernel has to end on an infinite or NaN sample, on which the reference never returns.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "carrier_dev.hpp"      // carrier_sincos: (float)sin((double)w), (float)cos((double)w) for a phase within a turn, the same bits on host and device

namespace csdr_amd {

#define TXMOD_PI ((float)3.14159265358979323846)
constexpr int TXMOD_WRAP_MAX = 4096;

// phase increment of one sample: the rounded product x PI
__host__ __device__ inline float fmmod_delta(float x) { return x * TXMOD_PI; }

// one step of the phase chain from the increment
__host__ __device__ inline float fmmod_phase_step(float p, float d)
{
    p = p + d;
    for (int k = 0; k < TXMOD_WRAP_MAX && p > TXMOD_PI; k++) p -= 2 * TXMOD_PI;
    for (int k = 0; k < TXMOD_WRAP_MAX && p <= -TXMOD_PI; k++) p += 2 * TXMOD_PI;
    return p;
}

__host__ __device__ inline float2 fmmod_output(float p)
{
    float sn, cs;
    carrier_sincos(p, &sn, &cs);
    return make_float2(cs, sn);
}

__host__ __device__ inline float2 dsb_value(float x, float q) { return make_float2(x, q); }

// 0.5 is a double in the reference: the sum is taken in double and stored to float
__host__ __device__ inline float2 add_dcoffset_value(float2 v) { return make_float2((float)(0.5 + (double)(v.x / 2)), v.y / 2); }

__host__ __device__ inline float2 fixed_amplitude_value(float2 v, float amp)
{
#ifdef __HIP_DEVICE_COMPILE__
    const float now = __fsqrt_rn(v.x * v.x + v.y * v.y);
    const float gain = now > 0 ? __fdiv_rn(amp, now) : 0.f;
#else
    const float now = sqrtf(v.x * v.x + v.y * v.y);
    const float gain = now > 0 ? amp / now : 0.f;
#endif
    return make_float2(v.x * gain, v.y * gain);
}

// convert_s16_f | gain_ff g  (libcsdr.c:2375 under the reference's -ffast-math: a product with the rounded reciprocal; libcsdr.c:1139-1142)
__host__ __device__ inline float tx_audio(int raw, float gain) { return gain * ((float)raw * (1.0f / 32767.0f)); }

// shift_addition_cc's phase after n samples of a chunk (libcsdr_gpl.c:48-51): wrap(phase + rate2 PI n), rate2 the doubled rate the reference stores
__host__ __device__ inline float tx_rot_advance(float phase, float rate2, int n)
{
    float p = phase + rate2 * TXMOD_PI * (float)n;
    for (int k = 0; k < TXMOD_WRAP_MAX && p > TXMOD_PI; k++) p -= 2 * TXMOD_PI;
    for (int k = 0; k < TXMOD_WRAP_MAX && p < -TXMOD_PI; k++) p += 2 * TXMOD_PI;
    return p;
}

#ifdef __HIPCC__
// convert_f_u8 (libcsdr.c:2380) as convert.hip computes it: x 255 in float, 0.5 x + 128 in double, truncated as cvttsd2si does, narrowed modulo 256
__device__ __forceinline__ int tx_to_u8(float x)
{
    const double y = (double)__fmul_rn(x, 255.0f) * 0.5 + 128.0;
    return ((y > -2147483649.0 && y < 2147483648.0) ? (int)y : (int)0x80000000) & 0xff;
}
#endif

} // namespace csdr_amd
