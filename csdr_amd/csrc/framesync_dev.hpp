// framesync_dev.hpp -- the step function of the frame synchroniser (framesync.hip): pattern_search_u8_u8 (csdr.c:3532-3597) with ONE STREAM'S state carried
// across calls.  __host__ __device__: k_framesync_generic and the CPU walk (csdr_amd_debug_framesync_walk) run this text; k_framesync_tiled evaluates the same
// definition on the stream of stored bytes (framesync.hip says how) and is tested against it byte for byte.
//
// It is the reference's loop: a ring of L bytes, a write index and a fill count.  A byte is stored at the index, which moves on (csdr.c:3555).  While fewer than
// L bytes have come since the (re)start nothing else happens (:3556).  Otherwise the index wraps to 0 at L and the ring, read from the index on, is compared with
// the pattern (:3557-3585).  A match emits the next V bytes and restarts the fill count ALONE (:3590): the index stays, so the ring fills from k = the index at
// the match, and the k + 1 bytes that would land at ring[L .. L+k] are dropped (the reference writes them past its buffer and never reads them), while
// ring[0 .. k) still holds the last k bytes of the window that matched.  After a reset k = 0: one dropped byte, behind the first L.
#pragma once
#include <stdint.h>

namespace csdr_amd {

constexpr int FS_MAX_L = 1024;                           // the longest pattern
constexpr int FS_TILE = 2048;                            // k_framesync_tiled: bytes of a row staged per step (csdr_amd_framesync_tile())

struct FsCfg { int L, V, m; };

// csdr_amd_framesync_chan
struct FsChan {
    int fill, index, remain, reserved;
    long long base, frames;
};

enum { FS_NONE = 0, FS_EMIT = 1, FS_MATCH = 2 };

// how many of the window's L positions differ from the pattern, counted up to m + 1; the window is the ring read from `from` on
__host__ __device__ inline int framesync_misses(const FsCfg &c, const uint8_t *ring, int from, const uint8_t *pat)
{
    int miss = 0, r = from;
    for (int i = 0; i < c.L; i++) {
        miss += ring[r] != pat[i];
        if (miss > c.m) break;
        if (++r == c.L) r = 0;
    }
    return miss;
}

// one byte: FS_EMIT: b is payload; FS_MATCH: the window that b completed matches, the payload starts at the stream's byte s.base (as it is on return)
__host__ __device__ inline int framesync_step(const FsCfg &c, FsChan &s, uint8_t *ring, const uint8_t *pat, uint8_t b)
{
    s.base++;
    if (s.remain > 0) { s.remain--; return FS_EMIT; }
    if (s.index < c.L) ring[s.index] = b;
    s.index++;
    if (s.fill < c.L) { s.fill++; return FS_NONE; }
    if (s.index >= c.L) s.index = 0;
    if (framesync_misses(c, ring, s.index, pat) > c.m) return FS_NONE;
    s.fill = 0; s.remain = c.V; s.frames++;
    return FS_MATCH;
}

// n bytes of one channel: payload bytes to out, each match's payload index to pos[*n_pos ..] (pos may be null; pos_cap entries at most).  Returns the payload count.
__host__ __device__ inline int framesync_walk(const FsCfg &c, FsChan &s, uint8_t *ring, const uint8_t *pat, const uint8_t *x, int n, uint8_t *out, long long *pos,
                                              int pos_cap, int *n_pos)
{
    int k = 0, f = 0;
    for (int j = 0; j < n; j++) {
        const uint8_t b = x[j];
        const int ev = framesync_step(c, s, ring, pat, b);
        if (ev == FS_EMIT) out[k++] = b;
        else if (ev == FS_MATCH) { if (pos && f < pos_cap) pos[f] = s.base; f++; }
    }
    *n_pos = f;
    return k;
}

} // namespace csdr_amd
