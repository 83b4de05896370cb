// shiftbank_dev.hpp -- the step functions of the shifter bank (shiftbank.hip): chunk start, phasor step, phase steps, quadrant-table lookup and the mix product of
// shift_addition_cc / _fc (libcsdr_gpl.c:27-79), shift_math_cc (libcsdr.c:186-207) and shift_table_cc (libcsdr.c:209-265) with ONE STREAM'S state carried across calls.
// __host__ __device__: the tiled kernels, the generic kernel and the CPU walk (csdr_amd_debug_shiftbank_walk) run this text.  The arithmetic is that of shift.hip's
// generator and mixing kernels -- the same operations in the same order, no contraction (-ffp-contract=off) -- so a stream of the bank and the shared-rate call agree
// to the bit on one device.
#pragma once
#include "seeds.hpp"
#include <math.h>

namespace csdr_amd {

constexpr int SB_TILE = 64;                              // MATH / TABLE: one kept phase per SB_TILE samples (shift.hip's SHIFT_TILE)

// csdr_amd_shiftbank_chan
struct ShiftbankChan {
    float rate, phase, c, s;
    int pos, pending;
    float old_rate;
    int pad;
};

__host__ __device__ inline float sb_wrap_pm_pi(float p)
{
    const float pi = (float)3.14159265358979323846;
    while (p > pi) p -= 2 * pi;
    while (p < -pi) p += 2 * pi;
    return p;
}
__host__ __device__ inline float sb_wrap_0_2pi(float p)
{
    const float pi = (float)3.14159265358979323846;
    while (p > 2 * pi) p -= 2 * pi;
    while (p < 0) p += 2 * pi;
    return p;
}
// (float)cos((double)x): the reference calls libm's double cos on a float phase and stores a float
__host__ __device__ inline float sb_cos(float x) { return (float)cos((double)x); }
__host__ __device__ inline float sb_sin(float x) { return (float)sin((double)x); }

// the phase increment per sample: "rate*=2" (libcsdr_gpl.c:83, libcsdr.c:188), then the float product with the float PI
__host__ __device__ inline float sb_inc(float rate) { return (rate * 2) * (float)3.14159265358979323846; }

// ---- ADDITION
// the phase advance over `len` samples: phase + rate*PI*len, wrapped (libcsdr_gpl.c:48-51); len = chunk at a chunk's end, = pos where a retune closes an open chunk
__host__ __device__ inline float sb_advance(float phase, float rate, int len) { return sb_wrap_pm_pi(phase + sb_inc(rate) * (float)len); }

// The same for whole chunks, one after the other, without the wrap loop's iterations where seeds.hpp's plan covers the step: |step| + PI below 4096, every rate of
// the band at chunk 1024 (|rate| <= 0.5: 3217).  Beyond it (rate 1.7 at chunk 1024: a step of 10938 rad) the loop itself runs.  The same bits either way.
struct ChunkStepper {
    WrapPlan w; float step; bool planned;
};
__host__ __device__ inline void sb_stepper_init(ChunkStepper &cs, float rate, int chunk)
{
    cs.step = sb_inc(rate) * (float)chunk;
    cs.planned = fabsf(cs.step) < 4000.f;
    wrap_plan_init(cs.w, cs.planned ? cs.step : 0.f);
}
__host__ __device__ inline float sb_next_chunk_phase(const ChunkStepper &cs, float phase)
{
    const float x = phase + cs.step;
    // (the plan takes |phase| <= PI: a phase a caller set from outside that range goes through the loop once)
    return (cs.planned && fabsf(phase) <= (float)3.14159265358979323846) ? wrap_plan_apply(cs.w, x) : sb_wrap_pm_pi(x);
}

// a retune closes the open chunk where it stands and the next sample starts a chunk with the new rate; a call's first sample sees the record after this
__host__ __device__ inline void sb_open_call_addition(ShiftbankChan &st)
{
    if (st.pending) {
        if (st.pos > 0) st.phase = sb_advance(st.phase, st.old_rate, st.pos);      // what the reference returns for a block of pos samples
        st.pos = 0; st.pending = 0;
    }
    st.old_rate = st.rate;
}

struct Phasor { float c, s; };
__host__ __device__ inline Phasor sb_chunk_start(float phase) { return Phasor{sb_cos(phase), sb_sin(phase)}; }           // libcsdr_gpl.c:33-34
__host__ __device__ inline Phasor sb_phasor_step(Phasor p, float sindelta, float cosdelta)                              // libcsdr_gpl.c:43-46
{
    Phasor q;
    q.c = p.c * cosdelta - p.s * sindelta;
    q.s = p.s * cosdelta + p.c * sindelta;
    return q;
}
__host__ __device__ inline cf32 sb_mix_cc(Phasor r, cf32 x) { return cf32{r.c * x.i - r.s * x.q, r.s * x.i + r.c * x.q}; }   // libcsdr_gpl.c:39-40
__host__ __device__ inline cf32 sb_mix_fc(Phasor r, float x) { return cf32{r.c * x, r.s * x}; }                               // libcsdr_gpl.c:65-66

// ---- MATH / TABLE
__host__ __device__ inline float sb_phase_step(float phase, float inc) { return sb_wrap_0_2pi(phase + inc); }          // libcsdr.c:202-204, 260-262
// The same step without the loops where each of them runs once at most: 0 <= phase <= 2 PI (what every step leaves) and |inc| <= 2 PI (|rate| <= 1) give
// -2 PI <= phase + inc <= 4 PI, one subtraction brings the sum to 2 PI or below and one addition to 0 or above, and neither result re-enters the other loop.
// The same operations on the same values: the same bits (tests/test_shiftbank_cpu.py holds the walk, which takes this path, to the loop model).  It is what
// makes the one-lane-per-stream scan affordable: a divergent loop costs a wave some 40 instructions per step, this form seven.
__host__ __device__ inline bool sb_once_ok(float phase, float inc)
{
    const float c = 2 * (float)3.14159265358979323846;
    return phase >= 0.f && phase <= c && fabsf(inc) <= c;
}
__host__ __device__ inline float sb_phase_step_once(float phase, float inc)
{
    const float c = 2 * (float)3.14159265358979323846;
    const float t = phase + inc, hi = t - c, lo = t + c;
    return t > c ? hi : (t < 0 ? lo : t);
}
__host__ __device__ inline float sb_phase_next(float phase, float inc) { return sb_once_ok(phase, inc) ? sb_phase_step_once(phase, inc) : sb_phase_step(phase, inc); }
__host__ __device__ inline Phasor sb_rot_math(float p) { return Phasor{sb_cos(p), sb_sin(p)}; }                          // libcsdr.c:199-200
__host__ __device__ inline float sb_quarter_entry(int k, int size) { return sb_sin(((float)k / (float)size) * ((float)3.14159265358979323846 / 2)); }   // libcsdr.c:211-222
__host__ __device__ inline Phasor sb_rot_table(float p, const float *table, int size)
{   // libcsdr.c:236-253: quadrant folding, truncated index, clamped where the reference would index out of bounds
    const float q90 = (float)3.14159265358979323846 / 2;
    const int quadrant = (int)(p / q90);
    const float within = p - (float)quadrant * q90;
    int si = (int)((within / q90) * (float)size), ci = size - 1 - si;
    if (quadrant & 1) { const int t = si; si = ci; ci = t; }
    si = si < 0 ? 0 : (si >= size ? size - 1 : si);
    ci = ci < 0 ? 0 : (ci >= size ? size - 1 : ci);
    Phasor r;
    r.s = (quadrant > 1 ? -1.0f : 1.0f) * table[si];
    r.c = ((quadrant && quadrant < 3) ? -1.0f : 1.0f) * table[ci];
    return r;
}

} // namespace csdr_amd
