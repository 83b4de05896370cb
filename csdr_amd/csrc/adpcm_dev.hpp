// adpcm_dev.hpp -- the IMA ADPCM encoder step (ima_adpcm.c:110-152) and the dB -> short conversion of compress_fft_adpcm_f_u8 (csdr.c:1763) as device
// functions: one definition for the codec kernels (adpcm.hip) and for the waterfall kernels that compress their rows in place (waterfall.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__constant__ int c_step[89] = { 7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143,
    157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707, 1878, 2066,
    2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500,
    20350, 22385, 24623, 27086, 29794, 32767 };                     // the standard IMA step table (ima_adpcm.c:98-108)

struct St { int index, prev; };

__device__ __forceinline__ int dec_one(unsigned code, St &s)
{   // ima_adpcm.c:110-134
    const int step = c_step[s.index];
    int diff = step >> 3;
    if (code & 1) diff += step >> 2;
    if (code & 2) diff += step >> 1;
    if (code & 4) diff += step;
    if (code & 8) diff = -diff;
    s.prev += diff;
    s.prev = s.prev > 32767 ? 32767 : (s.prev < -32768 ? -32768 : s.prev);
    s.index += (code & 4) ? 2 * (int)(code & 3) + 2 : -1;           // indexAdjustTable {-1,-1,-1,-1,2,4,6,8} twice (ima_adpcm.c:90-95)
    s.index = s.index < 0 ? 0 : (s.index > 88 ? 88 : s.index);
    return s.prev;
}
__device__ __forceinline__ unsigned enc_one(int sample, St &s)
{   // ima_adpcm.c:136-152
    int diff = sample - s.prev, step = c_step[s.index];
    unsigned code = 0;
    if (diff < 0) { code = 8; diff = -diff; }
    if (diff >= step) { code |= 4; diff -= step; }
    step >>= 1;
    if (diff >= step) { code |= 2; diff -= step; }
    step >>= 1;
    if (diff >= step) code |= 1;
    dec_one(code, s);
    return code;
}

__device__ __forceinline__ int db_to_short(float v)
{   // temp = input*100 stored to a short (csdr.c:1763): float product, truncation towards zero (x86 cvttss2si: 0x80000000 when out of range), low 16 bits
    const float p = v * 100;
    const int i = (p >= -2147483648.0f && p < 2147483648.0f) ? (int)p : (int)0x80000000;
    return (int)(int16_t)(i & 0xffff);
}

} // namespace
