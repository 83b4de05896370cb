// bank.hpp -- what the per-channel bank objects share on the host (the C twin of the Python wrapper's _Handle, _ChannelState and _Lanes): the base
// fields, the create preamble, the bodies of the recurring entry points and the cut of a debug walk's stream into calls.  Host code only; an object's
// extern "C" entry points stay in its own file under their own names and call these with the object's tag, which leads every message ("carrier: ...").
#pragma once
#include "common.hpp"
#include <string.h>
#include <algorithm>

namespace csdr_amd {

struct Bank {
    csdr_amd_ctx *c = nullptr;
    int n_ch = 0, lanes = 0;                             // lanes: channels per wave as the caller set it (0: the object's default)
    bool force_generic = false;
    const char *last_kernel = "";
};
// a bank with one state record per channel on the device
template <class C> struct ChanBank : Bank {
    using Chan = C;
    DevBuf<C> d_st;
};

// in front of an object's construction: 0, or the error with its message
inline int bank_create_check(const char *tag, csdr_amd_ctx *c, int n_channels, int most = 1 << 22, const char *what = "n_channels")
{
    if (!c) return fail_msg(-3, "%s: null context", tag);
    if (n_channels < 1 || n_channels > most) return fail_msg(-3, "%s: %s should be 1 .. %d", tag, what, most);
    if (hipSetDevice(c->device) != hipSuccess) return fail_msg(-2, "%s: hipSetDevice", tag);
    return 0;
}

// every channel back to *fresh, uploaded from the host (its bytes as they are, padding included); fresh == nullptr: to all-zero bytes on the context's
// stream, in order with the calls
template <class B> int bank_reset(B *p, const char *tag, const typename B::Chan *fresh)
{
    if (!p) return fail_msg(-3, "%s: null object", tag);
    const size_t bytes = sizeof(typename B::Chan) * p->n_ch;
    if (!fresh) return csdr_amd_memset(p->c, p->d_st.get(), 0, bytes);
    std::vector<typename B::Chan> h(p->n_ch);
    for (auto &s : h) memcpy(&s, fresh, sizeof s);
    return csdr_amd_h2d(p->c, p->d_st.get(), h.data(), bytes);
}

template <class B, class Pub> int bank_get_channel(B *p, const char *tag, int ch, Pub *out)
{
    static_assert(sizeof(Pub) == sizeof(typename B::Chan), "the public record mirrors the device's");
    if (!p || !out || ch < 0 || ch >= p->n_ch) return fail_msg(-3, "%s: channel out of range", tag);
    if (csdr_amd_ctx_sync(p->c) < 0) return -5;
    return csdr_amd_d2h(p->c, out, p->d_st.get() + ch, sizeof(Pub));
}

// valid(): the object's own check of *s behind the range check, 0 or its error.  What is uploaded is *s, or *record where the check builds one.
template <class B, class Pub, class Valid> int bank_set_channel(B *p, const char *tag, int ch, const Pub *s, Valid valid, const typename B::Chan *record = nullptr)
{
    static_assert(sizeof(Pub) == sizeof(typename B::Chan), "the public record mirrors the device's");
    if (!p || !s || ch < 0 || ch >= p->n_ch) return fail_msg(-3, "%s: channel out of range", tag);
    if (const int rc = valid()) return rc;
    if (csdr_amd_ctx_sync(p->c) < 0) return -5;
    return csdr_amd_h2d(p->c, p->d_st.get() + ch, record ? (const void *)record : (const void *)s, sizeof(Pub));
}
template <class B> int bank_reset_channel(B *p, const char *tag, int ch, const typename B::Chan &fresh)
{
    return bank_set_channel(p, tag, ch, &fresh, [] { return 0; });
}

inline int bank_set_lanes(Bank *p, const char *tag, int lanes)
{
    if (!p || lanes < 0 || lanes > 64) return fail_msg(-3, "%s: channels per wave is 0 (automatic) .. 64", tag);
    p->lanes = lanes;
    return 0;
}
// channels per wave: the caller's value or the object's default `dflt` for the kernel in question, `cap` at most
inline int bank_lanes(const Bank *p, int dflt, int cap = 64) { return std::min(p->lanes ? p->lanes : dflt, cap); }
// the same in front of a launch, which it records as the object's last kernel
inline int bank_launch_lanes(Bank *p, const char *kernel, int dflt, int cap = 64) { p->last_kernel = kernel; return bank_lanes(p, dflt, cap); }

inline int bank_force_generic(Bank *p, const char *tag, int on)
{
    if (!p) return fail_msg(-3, "%s: null object", tag);
    p->force_generic = on != 0;
    return 0;
}
inline const char *bank_kernel_name(const Bank *p) { return p ? p->last_kernel : ""; }

// A debug walk's stream of n items cut into calls of cuts[0], cuts[1], ... items (a negative cut is 0, a cut beyond the end takes what is left) and the rest
// in one more call: fn(done, m) once per call, m = 0 included, with `done` items in the calls before it.
template <class Fn> void for_each_call(long long n, const long long *cuts, int n_cuts, Fn fn)
{
    long long done = 0;
    for (int ci = 0; ci <= n_cuts; ci++) {
        const long long m = ci < n_cuts ? std::min(std::max(cuts[ci], 0LL), n - done) : n - done;
        fn(done, m);
        done += m;
    }
}

} // namespace csdr_amd
