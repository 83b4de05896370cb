// common.hpp -- shared host-side plumbing for libcsdr_amd.so (MI355X / gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>
#include <stdint.h>
#include <stddef.h>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include "../../include/csdr_amd.h"

namespace csdr_amd {

typedef csdr_complexf cf32;

int fail(hipError_t e, const char *what, const char *file, int line);
int fail_msg(int code, const char *fmt, ...);

#define CSDR_HIP(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return ::csdr_amd::fail(e__, #expr, __FILE__, __LINE__); } while (0)
#define CSDR_LAUNCH_CHECK() CSDR_HIP(hipGetLastError())

// float constant PI exactly as the reference defines it (libcsdr.h:65): a float, not a double
static const float PI_F = (float)3.14159265358979323846;

static inline unsigned cdiv(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

// ---- owners of HIP resources.  A member frees its resource when its object goes; members go in reverse declaration order, so a resource
// is declared in front of everything that uses it (a stream in front of its events, buffers and hipFFT plans).
template <auto Release> struct Del { template <class P> void operator()(P p) const { (void)Release(p); } };
template <class T = void> using DevBuf = std::unique_ptr<T, Del<hipFree>>;        // hipMalloc
template <class T = void> using HostBuf = std::unique_ptr<T, Del<hipHostFree>>;   // hipHostMalloc (pinned)
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, Del<hipEventDestroy>>;
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, Del<hipStreamDestroy>>;
using FftPlan = std::unique_ptr<std::remove_pointer_t<hipfftHandle>, Del<hipfftDestroy>>;
template <class T, auto Destroy> using Owned = std::unique_ptr<T, Del<Destroy>>;      // a library object, released by its destroy function

// (re)allocate: an owner that holds a buffer frees it first
template <class T> hipError_t dev_alloc(DevBuf<T> &p, size_t bytes)
{
    p.reset(); void *q = nullptr; const hipError_t e = hipMalloc(&q, bytes); p.reset(static_cast<T *>(q)); return e;
}
template <class T> hipError_t host_alloc(HostBuf<T> &p, size_t bytes, unsigned flags = hipHostMallocDefault)
{
    p.reset(); void *q = nullptr; const hipError_t e = hipHostMalloc(&q, bytes, flags); p.reset(static_cast<T *>(q)); return e;
}
static inline hipError_t event_create(Event &ev, unsigned flags = hipEventDefault)
{
    hipEvent_t e = nullptr; const hipError_t r = hipEventCreateWithFlags(&e, flags); ev.reset(e); return r;
}
static inline hipError_t stream_create(Stream &st, unsigned flags = hipStreamNonBlocking)
{
    hipStream_t s = nullptr; const hipError_t r = hipStreamCreateWithFlags(&s, flags); st.reset(s); return r;
}

// HIP-event timing of chosen kernels: a pool of (start, end) event pairs that grows on demand.  resolve() synchronises each end event recorded since the
// last resolve(), adds the pairs' elapsed times to *ms and their count to *launches, and starts over.
class KernelTimer {
    std::vector<std::pair<Event, Event>> pool_;
    size_t used_ = 0;
public:
    // the next pair, for the caller to record (e.g. as a launch's own start and completion signals)
    int take(hipEvent_t *start, hipEvent_t *end)
    {
        if (used_ == pool_.size()) {
            Event a, b; CSDR_HIP(event_create(a)); CSDR_HIP(event_create(b));
            pool_.emplace_back(std::move(a), std::move(b));
        }
        *start = pool_[used_].first.get(); *end = pool_[used_].second.get(); used_++;
        return 0;
    }
    // the next pair, its start recorded on st; end() records its end
    int begin(hipStream_t st) { hipEvent_t a, b; const int rc = take(&a, &b); if (rc) return rc; CSDR_HIP(hipEventRecord(a, st)); return 0; }
    int end(hipStream_t st) { CSDR_HIP(hipEventRecord(pool_[used_ - 1].second.get(), st)); return 0; }
    int resolve(double *ms, long *launches)
    {
        for (size_t k = 0; k < used_; k++) {
            CSDR_HIP(hipEventSynchronize(pool_[k].second.get()));
            float t = 0; CSDR_HIP(hipEventElapsedTime(&t, pool_[k].first.get(), pool_[k].second.get()));
            *ms += t; ++*launches;
        }
        used_ = 0;
        return 0;
    }
    void reset() { used_ = 0; }
};

enum { SCRATCH_SLOTS = 8 };

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (current device, kernel): the attribute is per device, contexts may live on several
// devices and be created from several threads (thread safe).  Returns 0 or a negative error.
int lds_attr_once(const void *kernel, size_t lds_bytes);
// multiProcessorCount of the CURRENT device (cached per device)
int current_device_cu_count();
void drop_fft_plans(hipStream_t st);      // fftpath.hip

// fastagc_ff (audio.hip) with an optional convert_f_s16 output written in the same pass; `out` may be null
int fastagc_ff_s16(struct ::csdr_amd_ctx *c, const float *in, float *out, int16_t *out_s16, int n_streams, int n_blocks, int block,
                   size_t in_pitch, size_t out_pitch, size_t s16_pitch, float reference, float *state_io, bool have_peaks = false);
float *fastagc_peaks_buffer(struct ::csdr_amd_ctx *c, int n_streams, int n_blocks);      // [n_streams][n_blocks + 2]; entries 2.. = peak |x| of the call's new blocks
void set_audio_last_path(const char *path);                          // audio.hip: what csdr_amd_audio_last_path() reports for the calling thread
void firdes_rrc_below(float *taps, int taps_length, int samples_per_symbol, float beta);   // modem.hip: firdes_rrc_f for any taps_length >= 1, writing indexes < taps_length only
// squelch.hip, for csdr_amd_fmrx, which serves some calls of a stream itself: every channel of `s` takes the bank's held count, block index and levels
// (lv, lv_started: n_channels each) -> the object's held samples [n_channels][block_size], which the caller may read and write between calls
void *squelch_adopt(struct ::csdr_amd_squelch *s, int held, long long block_index, const float *lv, const float *lv_started);
struct ShiftAhead;                                                   // shift.hip
struct ShiftAheadDel { void operator()(ShiftAhead *a) const; };

} // namespace csdr_amd

struct csdr_amd_ctx {
    int device;
    hipStream_t stream;
    csdr_amd::Stream own_stream;      // set when the context created `stream`
    std::string arch;
    // pinned host staging for small host-computed tables (phase sequences, plans): acquire() waits until the
    // previous upload from the buffer has completed, upload() queues the async copy on the context's stream
    csdr_amd::HostBuf<> pinned; size_t pinned_bytes; csdr_amd::Event pinned_ev; bool pinned_in_flight;
    void *pinned_acquire(size_t bytes);
    int pinned_upload(void *dst_dev, size_t bytes);
    csdr_amd::Event ev0, ev1;
    csdr_amd::DevBuf<> scratch[csdr_amd::SCRATCH_SLOTS];
    size_t scratch_bytes[csdr_amd::SCRATCH_SLOTS];
    // returns a device buffer of at least `bytes` that stays valid until the next request on the same slot
    void *get_scratch(int slot, size_t bytes);
    // shift_math_cc / shift_table_cc: the per-sample phase scan of the NEXT call, running on a helper thread while this call's kernels run (shift.hip: ShiftAhead)
    std::unique_ptr<csdr_amd::ShiftAhead, csdr_amd::ShiftAheadDel> shift_ahead;
};

namespace csdr_amd {
// the teardown of an object (its context: member `c`) whose work all runs on the context's stream: wait for it on the context's device, then let the
// members free what they own
template <class T> void destroy_on_stream(T *p)
{
    if (!p) return;
    (void)hipSetDevice(p->c->device);
    (void)hipStreamSynchronize(p->c->stream);
    delete p;
}
} // namespace csdr_amd

// ---- LDS-DMA row-step shared by the ring kernels (wfm_mfma.hip, ddc_mfma.hip).  Device code only.
#ifdef __HIPCC__
namespace csdr_amd {
// One row-step of a fetching wave as one piece of code: R rows, 1 KiB each (lane l: bytes 16 l .. 16 l + 15 of the run at sbase + vo[r]), LDS destinations RP bytes
// apart from la0 on.  M0 (the LDS destination) is saved once and stepped by s_add_u32, no branch between the pieces, `nt`: every byte is read once.  (Hand-written:
// the builtin form makes the compiler serialise the DMA with the LDS reads of other ring positions; vmcnt is counted by the callers.)
template <int R, int RP>
__device__ __forceinline__ void dma_rows(const uint32_t (&vo)[R], const uint8_t *sbase, uint32_t la0)
{
    uint32_t keep;
    static_assert(R == 2 || R == 4 || R == 8, "rows per fetching wave");
#define DMA_NEXT(k) "s_add_u32 m0, m0, %[rp]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %[v" #k "], %[sb] nt\n\t"
    if constexpr (R == 2)
        asm volatile("s_mov_b32 %[keep], m0\n\ts_mov_b32 m0, %[la]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %[v0], %[sb] nt\n\t" DMA_NEXT(1) "s_mov_b32 m0, %[keep]"
                     : [keep] "=&s"(keep) : [v0] "v"(vo[0]), [v1] "v"(vo[1]), [sb] "s"(sbase), [la] "s"(la0), [rp] "n"(RP) : "memory", "scc");
    else if constexpr (R == 4)
        asm volatile("s_mov_b32 %[keep], m0\n\ts_mov_b32 m0, %[la]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %[v0], %[sb] nt\n\t" DMA_NEXT(1) DMA_NEXT(2) DMA_NEXT(3) "s_mov_b32 m0, %[keep]"
                     : [keep] "=&s"(keep) : [v0] "v"(vo[0]), [v1] "v"(vo[1]), [v2] "v"(vo[2]), [v3] "v"(vo[3]), [sb] "s"(sbase), [la] "s"(la0), [rp] "n"(RP) : "memory", "scc");
    else
        asm volatile("s_mov_b32 %[keep], m0\n\ts_mov_b32 m0, %[la]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %[v0], %[sb] nt\n\t"
                     DMA_NEXT(1) DMA_NEXT(2) DMA_NEXT(3) DMA_NEXT(4) DMA_NEXT(5) DMA_NEXT(6) DMA_NEXT(7) "s_mov_b32 m0, %[keep]"
                     : [keep] "=&s"(keep) : [v0] "v"(vo[0]), [v1] "v"(vo[1]), [v2] "v"(vo[2]), [v3] "v"(vo[3]), [v4] "v"(vo[4]), [v5] "v"(vo[5]), [v6] "v"(vo[6]), [v7] "v"(vo[7]),
                       [sb] "s"(sbase), [la] "s"(la0), [rp] "n"(RP) : "memory", "scc");
#undef DMA_NEXT
}

} // namespace csdr_amd
#endif
