// framesync.hip -- the frame synchroniser: pattern_search_u8_u8 (csdr.c:3532-3597) for n_channels byte streams per call (MI355X / gfx950).  The definition and
// the per-channel record are framesync_dev.hpp's; both kernels give its bytes, counts, positions and state.
//   k_framesync_generic  one lane per channel runs framesync_dev.hpp's walk on global memory: the channel's ring of L bytes lives in its row of `rings`.
//   k_framesync_tiled    one wave (one workgroup) per channel.  A tile of FS_TILE bytes of the row is staged in LDS with 16-byte loads from the row's aligned
//                        base (the bytes in front of a misaligned row and behind its end are not read; the ragged first and last 16 are fetched bytewise); the
//                        next tile's loads are in flight while this one is searched.  The kernel works on the stream of STORED bytes, P: every byte the
//                        definition stores inside the ring, in order.  The ring is at all times the last L bytes of P, so a check is "P's last L bytes against
//                        the pattern", the bytes dropped behind a restart are simply not appended and the k bytes a restart inherits are P's tail.  In LDS:
//                        the last L bytes of P from earlier tiles, then what this tile appends.  While the searcher checks, up to FS_GROUP bytes are appended and
//                        every lane evaluates the four windows that end in its aligned word of P (a word at a time from the newest back, the wave out as soon as
//                        none of its windows is within m); __ballot's first set bit is the match, what was appended behind it is discarded.  A payload is copied from
//                        LDS to the output row in runs of up to 64 bytes per instruction.  Each input byte is read from HBM once, each output byte written once.
// At a call's end k_framesync_tiled turns P's tail back into the ring, so calls may alternate between the kernels.
#include "bank.hpp"
#include "framesync_dev.hpp"
#include <string.h>
#include <vector>

using namespace csdr_amd;

namespace {

constexpr int FS_PCAP = FS_MAX_L + FS_TILE;

struct FsArgs {
    FsCfg c; FsChan *st; uint8_t *rings; const uint8_t *pat; int n_ch, lanes;
    const uint8_t *in; size_t in_pitch; int n_in; const int *in_counts;
    uint8_t *out; size_t out_pitch; int *out_counts;
    long long *pos; size_t pos_pitch; int pos_cap; int *frame_counts;
};

__device__ __forceinline__ int fs_count(const FsArgs &a, int ch) { return a.in_counts ? min(max(a.in_counts[ch], 0), a.n_in) : a.n_in; }

__global__ __launch_bounds__(64) void k_framesync_generic(FsArgs a)
{
    if ((int)threadIdx.x >= a.lanes) return;
    const int ch = blockIdx.x * a.lanes + threadIdx.x;
    if (ch >= a.n_ch) return;
    FsChan s = a.st[ch];
    int f = 0;
    const int k = framesync_walk(a.c, s, a.rings + (size_t)ch * a.c.L, a.pat, a.in + (size_t)ch * a.in_pitch, fs_count(a, ch), a.out + (size_t)ch * a.out_pitch,
                                 a.pos ? a.pos + (size_t)ch * a.pos_pitch : nullptr, a.pos_cap, &f);
    a.st[ch] = s;
    a.out_counts[ch] = k;
    if (a.frame_counts) a.frame_counts[ch] = f;
}

constexpr int FS_GROUP = 256;                            // k_framesync_tiled: windows a wave evaluates at once, four a lane

// how many of a word's four bytes are not 0
__device__ __forceinline__ int fs_bytes_set(uint32_t x)
{
    x |= x >> 4; x |= x >> 2; x |= x >> 1;
    return __popc(x & 0x01010101u);
}

// the window P[e - L + 1 .. e] against the pattern, from the newest byte back: four bytes, then out as soon as more than m differ
__device__ __forceinline__ bool fs_window_matches(const uint8_t *P, int e, const uint8_t *pat, int L, int m)
{
    const uint8_t *w = P + (e - (L - 1));
    int miss = 0, i = L - 1;
    for (; i >= 3; i -= 4) {
        miss += (w[i] != pat[i]) + (w[i - 1] != pat[i - 1]) + (w[i - 2] != pat[i - 2]) + (w[i - 3] != pat[i - 3]);
        if (miss > m) return false;
    }
    for (; i >= 0; i--) miss += w[i] != pat[i];
    return miss <= m;
}

__global__ __launch_bounds__(64) void k_framesync_tiled(FsArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t raw[FS_TILE];
    __shared__ __attribute__((aligned(16))) uint8_t Pbuf[16 + FS_PCAP + FS_GROUP];      // a guard word in front (the oldest chunk of a window may begin 3 bytes early)
    __shared__ uint8_t pat[FS_MAX_L];
    __shared__ uint32_t patw[FS_MAX_L / 4], patm[FS_MAX_L / 4];                          // the pattern in words from its end back, and which of their bytes count
    uint8_t *P = Pbuf + 16;
    const uint32_t *PW = reinterpret_cast<const uint32_t *>(P);
    const int lane = threadIdx.x, ch = blockIdx.x, L = a.c.L, m = a.c.m;
    const int n = fs_count(a, ch);
    if (n == 0) {
        if (lane == 0) { a.out_counts[ch] = 0; if (a.frame_counts) a.frame_counts[ch] = 0; }
        return;
    }
    const FsChan s = a.st[ch];
    int fill = s.fill, index = s.index, remain = s.remain;
    uint8_t *ring = a.rings + (size_t)ch * L;
    for (int i = lane; i < L; i += 64) pat[i] = a.pat[i];
    if (lane < 4) reinterpret_cast<uint32_t *>(Pbuf)[lane] = 0;
    __syncthreads();
    const int n_words = (L + 3) / 4;
    for (int w = lane; w < n_words; w += 64) {
        uint32_t v = 0, k = 0;
        for (int b = 0; b < 4; b++) { const int i = L - 4 - 4 * w + b; if (i >= 0) { v |= (uint32_t)pat[i] << (8 * b); k |= 0xffu << (8 * b); } }
        patw[w] = v; patm[w] = k;
    }
    // P's last L bytes out of the ring: while the searcher checks, the ring read from the index on; otherwise the k bytes a restart inherited, then what it stored
    if (fill == L && index < L) {
        for (int d = lane; d < L; d += 64) { int r = index + d; if (r >= L) r -= L; P[d] = ring[r]; }
    } else {
        const int k = index - fill, have = k + min(fill, L - k);
        for (int i = lane; i < L; i += 64) P[i] = i >= L - have ? ring[i - (L - have)] : (uint8_t)0;
    }
    int plen = L;

    const uint8_t *row = a.in + (size_t)ch * a.in_pitch;
    const int al = (int)((uintptr_t)row & 15);
    const uint8_t *gb = row - al;                        // 16-byte aligned; offsets al .. al + n - 1 from it are the row
    const int span = al + n, n_tiles = (span + FS_TILE - 1) / FS_TILE;
    uint8_t *orow = a.out + (size_t)ch * a.out_pitch;
    long long *prow = a.pos ? a.pos + (size_t)ch * a.pos_pitch : nullptr;
    int ocount = 0, fcount = 0;

    uint4 nx[FS_TILE / 1024];
    auto whole = [&](int o) { return o >= al && o + 16 <= span; };
    auto fetch = [&](int t) {
#pragma unroll
        for (int c = 0; c < FS_TILE / 1024; c++) {
            const int o = t * FS_TILE + 16 * (lane + 64 * c);
            nx[c] = whole(o) ? *reinterpret_cast<const uint4 *>(gb + o) : make_uint4(0, 0, 0, 0);
        }
    };
    auto commit = [&](int t) {
#pragma unroll
        for (int c = 0; c < FS_TILE / 1024; c++) {
            const int q = 16 * (lane + 64 * c), o = t * FS_TILE + q;
            if (whole(o)) *reinterpret_cast<uint4 *>(raw + q) = nx[c];
            else for (int b = 0; b < 16; b++) if (o + b >= al && o + b < span) raw[q + b] = gb[o + b];
        }
    };
    auto matched = [&](int j_next) {                     // the payload starts at the call's byte j_next
        if (lane == 0 && prow && fcount < a.pos_cap) prow[fcount] = s.base + j_next;
        fcount++; remain = a.c.V; fill = 0;
    };

    fetch(0);
    for (int t = 0; t < n_tiles; t++) {
        __syncthreads();
        commit(t);
        if (t + 1 < n_tiles) fetch(t + 1);
        __syncthreads();
        const int o0 = t * FS_TILE - al;                 // the call's byte index of raw[0]
        int j = max(o0, 0);
        const int jend = min(o0 + FS_TILE, n);
        while (j < jend) {
            const uint8_t *x = raw + (j - o0);
            if (remain > 0) {                            // payload
                const int r = min(remain, jend - j);
                for (int i = lane; i < r; i += 64) orow[ocount + i] = x[i];
                ocount += r; remain -= r; j += r;
            } else if (fill < L) {                       // the ring fills: what lands inside it is appended
                const int r = min(L - fill, jend - j), push = min(max(L - index, 0), r);
                for (int i = lane; i < push; i += 64) P[plen + i] = x[i];
                plen += push; index += r; fill += r; j += r;
            } else if (index >= L) {                     // the byte behind the fill: dropped, and the first check
                __syncthreads();
                index = 0; j += 1;
                if (__ballot(fs_window_matches(P, plen - 1, pat, L, m)) != 0) matched(j);
            } else {                                     // checking: every byte is stored, then the window behind it compared
                const int q0 = plen & ~3, r = min(jend - j, FS_GROUP - (plen - q0));
                for (int i = lane; i < r; i += 64) P[plen + i] = x[i];
                __syncthreads();
                // a lane takes the four windows that end in P's word d0.  Word by word from the newest back: one aligned LDS word per step, shifted against the
                // one before into the four unaligned words of the windows; the walk ends when no window of the wave is within m any more.
                const int d0 = (q0 >> 2) + lane;
                int miss[4];
#pragma unroll
                for (int k = 0; k < 4; k++) { const int e = 4 * d0 + k; miss[k] = e >= plen && e < plen + r ? 0 : m + 1; }
                uint32_t hi = PW[d0];
                for (int w = 0; w < n_words; w++) {
                    const uint32_t lo = PW[d0 - w - 1], pw = patw[w], pm = patm[w];
                    const uint64_t both = ((uint64_t)hi << 32) | lo;
#pragma unroll
                    for (int k = 0; k < 4; k++) miss[k] += fs_bytes_set(((uint32_t)(both >> (8 * (k + 1))) ^ pw) & pm);
                    hi = lo;
                    if (__ballot(min(min(miss[0], miss[1]), min(miss[2], miss[3])) <= m) == 0) break;
                }
                const int kf = miss[0] <= m ? 0 : miss[1] <= m ? 1 : miss[2] <= m ? 2 : miss[3] <= m ? 3 : 4;
                const unsigned long long mask = __ballot(kf < 4);
                int found = -1;
                if (mask) { const int fl = __ffsll((long long)mask) - 1; found = 4 * ((q0 >> 2) + fl) + __shfl(kf, fl) - plen; }
                found = __builtin_amdgcn_readfirstlane(found);
                const int adv = found < 0 ? r : found + 1;
                plen += adv; index = (index + adv) % L; j += adv;
                if (found >= 0) matched(j);
                __syncthreads();
            }
        }
        if (plen > L) {                                  // keep P's last L bytes for the next tile
            __syncthreads();
            uint8_t keep[FS_MAX_L / 64];
#pragma unroll
            for (int i = 0; i < FS_MAX_L / 64; i++) if (lane + 64 * i < L) keep[i] = P[plen - L + lane + 64 * i];
            __syncthreads();
#pragma unroll
            for (int i = 0; i < FS_MAX_L / 64; i++) if (lane + 64 * i < L) P[lane + 64 * i] = keep[i];
            plen = L;
        }
    }
    __syncthreads();
    // P's tail back into the ring (the inverse of the start)
    if (fill == L && index < L) {
        for (int d = lane; d < L; d += 64) { int r = index - 1 - d; if (r < 0) r += L; ring[r] = P[plen - 1 - d]; }
    } else {
        const int k = index - fill, have = k + min(fill, L - k);
        for (int i = lane; i < have; i += 64) ring[i] = P[plen - have + i];
    }
    if (lane == 0) {
        FsChan e = s;
        e.fill = fill; e.index = index; e.remain = remain; e.base += n; e.frames += fcount;
        a.st[ch] = e;
        a.out_counts[ch] = ocount;
        if (a.frame_counts) a.frame_counts[ch] = fcount;
    }
}

static_assert(sizeof(FsChan) == sizeof(csdr_amd_framesync_chan), "FsChan mirrors csdr_amd_framesync_chan");

int make_fs_cfg(const char *tag, const unsigned *pattern, int L, int V, int m, FsCfg *c, std::vector<uint8_t> *pat)
{
    if (L < 1 || L > FS_MAX_L || !pattern) return fail_msg(-3, "%s: need 1 .. %d pattern values", tag, FS_MAX_L);
    if (V < 0 || V > (1 << 30)) return fail_msg(-3, "%s: values_after should be 0 .. 2^30", tag);
    if (m < 0 || m >= L) return fail_msg(-3, "%s: max_mismatch should be 0 .. pattern length - 1", tag);
    pat->resize(L);
    for (int i = 0; i < L; i++) {
        if (pattern[i] > 255) return fail_msg(-3, "%s: pattern value %u is above 255 and cannot match a byte", tag, pattern[i]);
        (*pat)[i] = (uint8_t)pattern[i];
    }
    c->L = L; c->V = V; c->m = m;
    return 0;
}

// what a record may hold: the states the step function reaches
int fs_chan_valid(const FsCfg &c, const FsChan &s)
{
    const bool checking = s.fill == c.L && s.index >= 0 && s.index < c.L;
    const int k = s.index - s.fill;
    const bool ok = s.fill >= 0 && s.fill <= c.L && s.remain >= 0 && s.remain <= c.V && (s.remain == 0 || s.fill == 0) && (checking || (k >= 0 && k < c.L)) && s.base >= 0;
    return ok ? 0 : fail_msg(-3, "framesync: a record the searcher cannot reach (fill, index or remain out of range)");
}

// channels per wave of k_framesync_generic when the caller leaves it open: one wave per CU first, as k_pulserx_generic
int default_fs_lanes(int cus, int n_ch) { return std::max(1, std::min(64, (int)cdiv(n_ch, (size_t)cus))); }

} // namespace

struct csdr_amd_framesync : ChanBank<FsChan> {
    FsCfg cfg; int cus;
    DevBuf<uint8_t> d_rings, d_pat;
};

extern "C" {

int csdr_amd_framesync_create(csdr_amd_ctx *c, int n_channels, const unsigned *pattern, int pattern_length, int values_after, int max_mismatch, csdr_amd_framesync **out)
{
    if (!out) return fail_msg(-3, "framesync: null result pointer");
    *out = nullptr;
    FsCfg cfg; std::vector<uint8_t> pat;
    if (const int rc = bank_create_check("framesync", c, n_channels)) return rc;
    if (const int rc = make_fs_cfg("framesync", pattern, pattern_length, values_after, max_mismatch, &cfg, &pat)) return rc;
    Owned<csdr_amd_framesync, csdr_amd_framesync_destroy> p(new csdr_amd_framesync());
    p->c = c; p->n_ch = n_channels; p->cfg = cfg; p->cus = current_device_cu_count();
    if (dev_alloc(p->d_st, sizeof(FsChan) * n_channels) != hipSuccess || dev_alloc(p->d_rings, (size_t)cfg.L * n_channels) != hipSuccess ||
        dev_alloc(p->d_pat, cfg.L) != hipSuccess) return fail_msg(-2, "framesync: out of device memory");
    if (csdr_amd_memset(c, p->d_rings.get(), 0, (size_t)cfg.L * n_channels) < 0 || csdr_amd_h2d(c, p->d_pat.get(), pat.data(), cfg.L) < 0) return -5;
    if (const int rc = csdr_amd_framesync_reset(p.get())) return rc;
    *out = p.release();
    return 0;
}

int csdr_amd_framesync_reset(csdr_amd_framesync *p) { return bank_reset(p, "framesync", (const FsChan *)nullptr); }
int csdr_amd_framesync_reset_channel(csdr_amd_framesync *p, int ch) { return bank_reset_channel(p, "framesync", ch, FsChan{0, 0, 0, 0, 0, 0}); }

int csdr_amd_framesync_get_channel(csdr_amd_framesync *p, int ch, csdr_amd_framesync_chan *out, unsigned char *window)
{
    if (const int rc = bank_get_channel(p, "framesync", ch, out)) return rc;
    return window ? csdr_amd_d2h(p->c, window, p->d_rings.get() + (size_t)ch * p->cfg.L, p->cfg.L) : 0;
}

int csdr_amd_framesync_set_channel(csdr_amd_framesync *p, int ch, const csdr_amd_framesync_chan *s, const unsigned char *window)
{
    const int rc = bank_set_channel(p, "framesync", ch, s, [&] { FsChan r; memcpy(&r, s, sizeof r); return fs_chan_valid(p->cfg, r); });
    if (rc || !window) return rc;
    return csdr_amd_h2d(p->c, p->d_rings.get() + (size_t)ch * p->cfg.L, window, p->cfg.L);
}

int csdr_amd_framesync_set_lanes(csdr_amd_framesync *p, int lanes) { return bank_set_lanes(p, "framesync", lanes); }
int csdr_amd_framesync_lanes(const csdr_amd_framesync *p) { return !p ? 0 : p->force_generic ? bank_lanes(p, default_fs_lanes(p->cus, p->n_ch)) : 1; }
int csdr_amd_framesync_force_generic(csdr_amd_framesync *p, int on) { return bank_force_generic(p, "framesync", on); }
const char *csdr_amd_framesync_kernel_name(const csdr_amd_framesync *p) { return bank_kernel_name(p); }
void csdr_amd_framesync_destroy(csdr_amd_framesync *p) { destroy_on_stream(p); }

long long csdr_amd_framesync_max_out(const csdr_amd_framesync *p, long long n_in) { return p && n_in > 0 ? n_in : 0; }
long long csdr_amd_framesync_max_frames(const csdr_amd_framesync *p, long long n_in) { return p && n_in >= 0 ? n_in / (p->cfg.L + 1) + 1 : 0; }
int csdr_amd_framesync_tile(void) { return FS_TILE; }

int csdr_amd_framesync_process(csdr_amd_framesync *p, const unsigned char *in, size_t in_pitch, long long n_in, const int *in_counts, unsigned char *out,
                               size_t out_pitch, int *out_counts, long long *frame_pos, size_t frame_pitch, int *frame_counts)
{
    if (!p) return fail_msg(-3, "framesync: null object");
    if (n_in < 0 || n_in > (1LL << 30) || (n_in > 0 && (!in || in_pitch < (size_t)n_in))) return fail_msg(-3, "framesync: need in_pitch >= n_in >= 0 (n_in <= 2^30)");
    if (!out_counts) return fail_msg(-3, "framesync: out_counts is required");
    if (n_in > 0 && (!out || out_pitch < (size_t)n_in)) return fail_msg(-3, "framesync: out_pitch %zu below max_out %lld", out_pitch, n_in);
    const long long mf = csdr_amd_framesync_max_frames(p, n_in);
    if (frame_pos && frame_pitch < (size_t)mf) return fail_msg(-3, "framesync: frame_pitch %zu below max_frames %lld", frame_pitch, mf);
    csdr_amd_ctx *c = p->c;
    FsArgs a;
    a.c = p->cfg; a.st = p->d_st.get(); a.rings = p->d_rings.get(); a.pat = p->d_pat.get(); a.n_ch = p->n_ch; a.lanes = 1;
    a.in = in; a.in_pitch = in_pitch; a.n_in = (int)n_in; a.in_counts = in_counts; a.out = out; a.out_pitch = out_pitch; a.out_counts = out_counts;
    a.pos = frame_pos; a.pos_pitch = frame_pitch; a.pos_cap = (int)std::min<long long>(mf, 0x7fffffff); a.frame_counts = frame_counts;
    if (!p->force_generic) {
        p->last_kernel = "k_framesync_tiled";
        hipLaunchKernelGGL(k_framesync_tiled, dim3(p->n_ch), dim3(64), 0, c->stream, a);
    } else {
        a.lanes = bank_launch_lanes(p, "k_framesync_generic", default_fs_lanes(p->cus, p->n_ch));
        hipLaunchKernelGGL(k_framesync_generic, dim3(cdiv(p->n_ch, a.lanes)), dim3(64), 0, c->stream, a);
    }
    CSDR_LAUNCH_CHECK();
    return 0;
}

int csdr_amd_pattern_search_u8_u8(csdr_amd_ctx *c, const unsigned char *in, long long n, const unsigned *pattern, int pattern_length, int values_after,
                                  unsigned char *out, int *out_count)
{
    csdr_amd_framesync *raw = nullptr;
    if (const int rc = csdr_amd_framesync_create(c, 1, pattern, pattern_length, values_after, 0, &raw)) return rc;
    Owned<csdr_amd_framesync, csdr_amd_framesync_destroy> p(raw);
    return csdr_amd_framesync_process(p.get(), in, (size_t)std::max(n, 0LL), n, nullptr, out, (size_t)std::max(n, 0LL), out_count, nullptr, 0, nullptr);
}

long long csdr_amd_debug_framesync_walk(const unsigned *pattern, int pattern_length, int values_after, int max_mismatch, const unsigned char *in, long long n,
                                        const long long *cuts, int n_cuts, unsigned char *out, long long *pos, long long *n_frames,
                                        csdr_amd_framesync_chan *state_io, unsigned char *window_io)
{
    FsCfg cfg; std::vector<uint8_t> pat;
    if (const int rc = make_fs_cfg("debug_framesync_walk", pattern, pattern_length, values_after, max_mismatch, &cfg, &pat)) return rc;
    if (n < 0 || n > (1LL << 30) || (n > 0 && (!in || !out)) || n_cuts < 0 || (n_cuts && !cuts)) return fail_msg(-3, "debug_framesync_walk: bad arguments");
    FsChan s{0, 0, 0, 0, 0, 0};
    std::vector<uint8_t> ring(cfg.L, 0);
    if (state_io) {
        memcpy(&s, state_io, sizeof s);
        if (const int rc = fs_chan_valid(cfg, s)) return rc;
        if ((s.fill || s.index) && !window_io) return fail_msg(-3, "debug_framesync_walk: a state that holds bytes needs its window");
    }
    if (window_io) memcpy(ring.data(), window_io, cfg.L);
    long long k = 0, f = 0;
    for_each_call(n, cuts, n_cuts, [&](long long done, long long cnt) {
        int nf = 0;
        k += framesync_walk(cfg, s, ring.data(), pat.data(), in + done, (int)cnt, out + k, pos ? pos + f : nullptr, 0x7fffffff, &nf);
        f += nf;
    });
    if (state_io) memcpy(state_io, &s, sizeof s);
    if (window_io) memcpy(window_io, ring.data(), cfg.L);
    if (n_frames) *n_frames = f;
    return k;
}

} // extern "C"
