"""CPU checks of the pulse-shaped receive chain (matched filter | timing_recovery_cc | [realpart_cf |] gain_ff | generic_slicer_f_u8):
  1. the model's summation order (pulserx_model.dot32) against exact rational arithmetic;
  2. the step functions the kernels run (csdr_amd_debug_pulserx_walk) against the float32 model, bit for bit: symbols, errors, indexes, bytes, counts
     and the final state, for every shape, algorithm, use_q, stage range, slice_q and n_symbols, cut into calls of 0, 1, 7, T - 1, T, 3 D/2 + T and the rest;
  3. the walk against the compiled reference's apply_real_fir_cc | timing_recovery_cc | generic_slicer_f_u8 and float64, on the prefix of every channel in
     which the timing loop's truncation cannot depend on the order of a float32 sum;
  4. the new entry points at the boundary: exported, declared, and a C client that calls them links.
Measured figures: profiles/pulserx_gates.md."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import pulse_model as pm
import pulserx_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libcsdr_ref.so")

SHAPES = [(8, 65), (4, 33), (12, 65), (16, 129), (2, 7), (256, 513)]          # (samples per symbol = decimation, taps); the last one is the COSINE pulse
GRID = [(s, alg, q) for s in SHAPES for alg in (rm.GARDNER, rm.EARLYLATE) for q in (1, 0)]
LOOP_GAIN, MAX_ERROR = 0.5, 2.0
N_SYM = 300
SLICES = [(0, 2), (1, 2), (0, 4), (1, 4), (0, 3), (1, 3)]                       # (slice_q, n_symbols)


def taps_of(shape):
    import csdr_amd
    sps, T = shape
    return csdr_amd.firdes_cosine_f(sps) if T == 2 * sps + 1 else csdr_amd.firdes_rrc_f(T, sps, 0.35)


# The scale of a case's signal (RMS behind the matched filter).  A correction needs |error| loop_gain D/2 >= 1 and the error grows with the square of the
# amplitude, so the share of correcting symbols rises steeply with the scale; too large a scale clips nearly every error and, at a long symbol, lets
# v = error loop_gain D/2 sweep over many integers, near one of which a float32 sum's rounding may decide the truncation.  Each entry is the smallest
# step of a sqrt(2) grid at which the float32 model corrects on 3 % of the symbols or more, on every channel of the signals the tests use.
RMS = {(8, 65): (1.4, 1.0, 2.0, 1.0), (4, 33): (2.0, 1.4, 2.8, 1.4), (12, 65): (1.4, 0.7, 1.0, 1.0), (16, 129): (1.0, 0.7, 1.4, 0.7),
       (2, 7): (2.8, 2.0, 2.8, 2.0), (256, 513): (0.18, 0.18, 0.5, 0.35)}     # (GARDNER with Q, GARDNER, EARLYLATE with Q, EARLYLATE)


def rms_of(shape, alg, q):
    return RMS[shape][2 * alg + (0 if q else 1)]


def can_correct(shape, alg):
    """EARLYLATE at D = 2 has a wing of (int)(2 * 0.25) = 0 samples: its left and right point are the same sample, the error is 0 by construction"""
    return not (alg == rm.EARLYLATE and shape[0] < 4)


def cuts_of(shape):
    D, T = shape
    return (0, 1, 7, T - 1, T, 3 * D // 2 + T)


def case_signal(shape, alg, q, n_psk, n_channels=2, seed=1):
    return rm.signal(n_psk, shape[0], taps_of(shape), N_SYM, n_channels, rms=rms_of(shape, alg, q), seed=seed)[0]


def filtered32(x, taps):
    """a stream for the stage range that starts at TIMING: the filtered signal, rounded to float32"""
    return np.stack([rm.filter64(r, taps)[0] for r in np.atleast_2d(x)]).astype(np.complex64)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def params_of(shape, alg, q, taps, gain=1.0, n_symbols=2, slice_q=0):
    import csdr_amd
    return csdr_amd.pulserx_params(taps, alg, shape[0], LOOP_GAIN, MAX_ERROR, q, gain, n_symbols, slice_q)


def model_kw(shape, alg, q):
    return dict(decimation=shape[0], algorithm=alg, use_q=bool(q), loop_gain=LOOP_GAIN, max_error=MAX_ERROR)


def variants(model, gain):
    """what the object writes for every `last`, from one model run of the timing loop: [(last, slice_q, n_symbols, expected output)]"""
    out = [("timing", 0, 2, model["sym"])]
    for sq, ns in SLICES:
        soft = (np.float32(gain) * (model["sym"].view(np.float32) if sq else np.ascontiguousarray(model["sym"].real))).astype(np.float32)
        out.append(("slice", sq, ns, pm.slicer(soft, ns)))
    return out


# ------------------------------------------------------------------ 1. the order
def _round32(q):
    """the float32 nearest to the rational q, ties to even"""
    near = np.float32(float(q))
    cands = [near, np.nextafter(near, np.float32(np.inf)), np.nextafter(near, np.float32(-np.inf))]
    dist = [abs(Fraction(float(v)) - q) for v in cands]
    win = [v for v, d in zip(cands, dist) if d == min(dist)]
    if len(win) == 2:
        win = [v for v in win if (np.float32(v).view(np.uint32) & 1) == 0]
    return win[0]


def _exact_dot(x, w):
    """the defined order in rational arithmetic with one rounding per fused multiply-add and per sum"""
    p = [np.float32(0)] * 16
    for t in range(len(w)):
        p[t & 15] = _round32(Fraction(float(x[t])) * Fraction(float(w[t])) + Fraction(float(p[t & 15])))
    for s in (8, 4, 2, 1):
        for r in range(s):
            p[r] = _round32(Fraction(float(p[r])) + Fraction(float(p[r + s])))
    return p[0]


@pytest.mark.parametrize("T", [1, 7, 16, 17, 33, 65])
def test_model_order_is_the_defined_one(T):
    """dot32 against rational arithmetic, on operands of far apart exponents so that every rounding and the order of the sums show"""
    rng = np.random.default_rng(100 + T)
    n = T + 5
    x = ((rng.uniform(-2, 2, n) + 1j * rng.uniform(-2, 2, n)) * 2.0 ** rng.integers(-12, 12, n)).astype(np.complex64)
    w = (rng.uniform(-1, 1, T) * 2.0 ** rng.integers(-8, 8, T)).astype(np.float32)
    pos = np.array([[0, 3, 5]])
    re, im = rm.dot32(x[None], pos, w)
    for j, p in enumerate(pos[0]):
        assert re[0, j].view(np.uint32) == np.float32(_exact_dot(x.real[p:p + T], w)).view(np.uint32)
        assert im[0, j].view(np.uint32) == np.float32(_exact_dot(x.imag[p:p + T], w)).view(np.uint32)
    assert rm.fold16(np.arange(16, dtype=np.float32)) == 120


# ------------------------------------------------------------------ 2. the walk equals the model
def _check_walk(shape, alg, q, first, x, taps, model, gain):
    import csdr_amd
    cuts = cuts_of(shape)
    want_state = model["state"]
    for last, sq, ns, want in variants(model, gain):
        p = params_of(shape, alg, q, taps, gain, ns, sq)
        for cu in (cuts, ()):
            st = csdr_amd.PulseRxChan()
            if last == "timing":
                y, e, i = csdr_amd.pulserx_debug_walk(p, first, last, x, cuts=cu, state=st, with_extras=True)
                assert e.size == model["err"].size and np.array_equal(u32(e), u32(model["err"])), (first, last, "errors")
                assert np.array_equal(i, model["idx"]), (first, last, "indexes")
                assert y.dtype == np.complex64 and y.size == want.size and np.array_equal(u32(y), u32(want)), (first, last, "symbols")
            else:
                y = csdr_amd.pulserx_debug_walk(p, first, last, x, cuts=cu, state=st)
                assert y.dtype == np.uint8 and y.size == want.size and np.array_equal(y, want), (first, last, sq, ns, "bytes")
            assert (st.tail_len, st.correction_offset, st.base) == want_state, (first, last, "state")


@pytest.mark.parametrize("shape,alg,q", GRID)
def test_debug_walk_equals_model(shape, alg, q):
    taps = taps_of(shape)
    gain = 1.0 / rms_of(shape, alg, q)
    share = []
    for n_psk, firsts in ((4, ("filter", "timing")), (2, ("filter",))):
        x = case_signal(shape, alg, q, n_psk)
        for first in firsts:
            xs = x if first == "filter" else filtered32(x, taps)
            models = rm.receive(xs, taps, first=rm.FILTER if first == "filter" else rm.TIMING, last=rm.TIMING, **model_kw(shape, alg, q))
            for ch, m in enumerate(models):
                assert N_SYM // 2 <= m["sym"].size <= 2 * N_SYM
                share.append(np.mean(m["corr"] != 0))
                _check_walk(shape, alg, q, first, xs[ch], taps, m, gain)
    if can_correct(shape, alg):
        assert min(share) >= 0.01, share                   # the case exercises the correction path


def test_debug_walk_short_and_empty_streams():
    """no symbol until 3 D/2 + T samples are there; everything stays in the tail"""
    import csdr_amd
    shape = (8, 65)
    taps = taps_of(shape)
    p = params_of(shape, 0, 1, taps)
    x = case_signal(shape, 0, 1, 4)[0]
    for n in (0, 1, 64, 3 * 4 + 64):
        st = csdr_amd.PulseRxChan()
        y = csdr_amd.pulserx_debug_walk(p, "filter", "timing", x[:n], cuts=(0, 1), state=st)
        assert y.size == 0 and (st.tail_len, st.correction_offset, st.base) == (n, 0, 0)
    st = csdr_amd.PulseRxChan()
    y = csdr_amd.pulserx_debug_walk(p, "filter", "timing", x[:3 * 4 + 66], state=st)
    assert y.size == 1 and st.base == 8 + st.correction_offset and st.tail_len == 3 * 4 + 66 - st.base


def test_debug_walk_nan_and_inf_samples():
    """a NaN timing error corrects by 0 (the conversion of a NaN to int is not defined: it would be INT_MIN on this host and the symbol start would
    walk backwards out of the tail): the loop walks on, positions and state equal the model's, the symbols too wherever they are numbers"""
    import csdr_amd
    for shape, alg, q in (((8, 65), rm.GARDNER, 1), ((16, 129), rm.EARLYLATE, 0)):
        taps = taps_of(shape)
        x = np.array(case_signal(shape, alg, q, 4))
        x[0, 700] = np.inf; x[1, 900] = np.nan; x[1, 1500] = complex(0, -np.inf)
        for first in ("filter", "timing"):
            models = rm.receive(x, taps, first=rm.FILTER if first == "filter" else rm.TIMING, last=rm.TIMING, **model_kw(shape, alg, q))
            for ch, m in enumerate(models):
                st = csdr_amd.PulseRxChan()
                y, e, i = csdr_amd.pulserx_debug_walk(params_of(shape, alg, q, taps), first, "timing", x[ch], cuts=cuts_of(shape), state=st, with_extras=True)
                assert np.array_equal(i, m["idx"]) and (st.tail_len, st.correction_offset, st.base) == m["state"]
                num = ~np.isnan(m["sym"].view(np.float32))
                assert np.isnan(m["err"]).any() or first == "timing"           # (the filter spreads the sample over T positions: the loop meets it)
                assert np.array_equal(np.isnan(y.view(np.float32)), ~num) and np.array_equal(np.isnan(e), np.isnan(m["err"]))
                assert np.array_equal(u32(y.view(np.float32)[num]), u32(m["sym"].view(np.float32)[num]))


def test_debug_walk_argument_errors():
    import csdr_amd
    taps = taps_of((8, 65)); x = np.zeros(200, np.complex64)
    good = dict(taps=taps, algorithm=0, decimation=8, loop_gain=0.5, max_error=2.0, use_q=1, gain=1.0, n_symbols=4, slice_q=0)
    for kw, stages in [(dict(decimation=1), ("filter", "slice")), (dict(algorithm=2), ("filter", "slice")), (dict(loop_gain=0.6), ("filter", "slice")),
                       (dict(max_error=-1.0), ("filter", "slice")), (dict(n_symbols=1), ("filter", "slice")), (dict(n_symbols=257), ("filter", "slice")),
                       (dict(taps=None), ("filter", "timing")), (dict(), ("timing", "filter")), (dict(), (2, 2)), (dict(), (-1, 1))]:
        with pytest.raises(csdr_amd.CsdrAmdError):
            csdr_amd.pulserx_debug_walk(csdr_amd.pulserx_params(**dict(good, **kw)), stages[0], stages[1], x)
    # what a range does not use is not checked: no taps from TIMING on, no n_symbols to TIMING
    assert csdr_amd.pulserx_debug_walk(csdr_amd.pulserx_params(**dict(good, taps=None, n_symbols=0)), "timing", "timing", x).size > 0
    st = csdr_amd.PulseRxChan(5, 0, 0)
    with pytest.raises(csdr_amd.CsdrAmdError):
        csdr_amd.pulserx_debug_walk(csdr_amd.pulserx_params(**good), "filter", "slice", x, state=st)


# ------------------------------------------------------------------ 3. against the compiled reference and float64
@pytest.fixture(scope="module")
def ref():
    if not os.path.exists(REF_LIB):
        pytest.skip("reference library not built (oracle/_ref/libcsdr_ref.so)")
    import test_pulse_cpu as tp
    L = tp.bind_modem(C.CDLL(REF_LIB))
    import test_psk31_cpu as tk
    L.timing_recovery_init.restype = tk.TRState
    L.timing_recovery_init.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_char_p]
    L.timing_recovery_cc.restype = None
    L.timing_recovery_cc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(tk.TRState)]
    return L


def reference_prefix(shape, alg, q, x, taps, ridx):
    """From the reference's own sampled indexes: the float64 filtered samples at every symbol's three positions, v = clip(e) loop_gain (D/2 sign) in
    float64, and delta, the bound of |v - what a float32 path computes|: each filtered sample is within dot_gate(T, sum |x taps|) of the exact one
    whatever the order of its sum; through e = (r - l) m that is |m| (g_r + g_l) + (|r - l| + g_r + g_l) g_m per component, plus the three float32
    roundings of the expression itself (4 2^-24 of the magnitudes), halved with Q; the two products behind it scale by |loop_gain| D/2 and add
    2 2^-24 |v|.  -> (number of leading symbols in front of the first one whose v is within delta of a nonzero integer, gates of the sampled point)"""
    D = shape[0]; hb, qb = D // 2, D // 4
    wing = int(np.float32(D) * np.float32(0.25))
    f, mr, mi = rm.filter64(x, taps)
    T = np.asarray(taps).size
    gr, gi = pm.dot_gate(T, mr), pm.dot_gate(T, mi)
    ridx = np.asarray(ridx, np.int64)
    if alg == rm.GARDNER:
        pl, pmid, pr = ridx, ridx + hb, ridx + 2 * hb
    else:
        cbi = ridx - hb
        prev = np.concatenate([[0], np.diff(ridx) - D])                       # the correction in front of each symbol, as the reference took it
        prev = np.where((prev <= -qb * 0.9) | (prev >= 0.9 * qb), 0, prev)
        pl, pmid, pr = cbi + wing - prev, ridx, cbi + 3 * wing

    def part(v, g):
        e = (v[pr] - v[pl]) * v[pmid]
        gs = g[pr] + g[pl]
        d = np.abs(v[pmid]) * gs + (np.abs(v[pr] - v[pl]) + gs) * g[pmid] + 4 * pm.EPS * (np.abs(v[pr]) + np.abs(v[pl])) * np.abs(v[pmid])
        return e, d
    e, d = part(f.real, gr)
    if q:
        e2, d2 = part(f.imag, gi)
        e, d = (e + e2) / 2, (d + d2) / 2 + 2 * pm.EPS * (np.abs(e) + np.abs(e2))
    sign = -1 if alg == rm.GARDNER else 1
    v = np.clip(e, -MAX_ERROR, MAX_ERROR) * LOOP_GAIN * (hb * sign)
    delta = d * abs(LOOP_GAIN) * hb + 2 * pm.EPS * np.abs(v)
    m = np.rint(v)
    # a symbol whose error is beyond the clip by more than its bound is clipped in every path: the correction then comes from the constant max_error
    # alone and no sum enters it (at D = 2 every correction is of this kind: it needs |e| loop_gain >= 1, which is the clip)
    clipped = np.abs(e) > MAX_ERROR + d
    risky = (m != 0) & (np.abs(v - m) <= delta) & ~clipped
    k = int(np.argmax(risky)) if risky.any() else ridx.size
    po = pmid if alg == rm.EARLYLATE else pl
    return k, f[po], gr[po], gi[po], v


def near_a_limit(f64, gr, gi, gain, slice_q, n_symbols):
    """per output byte: gain * soft is within gain * gate (and the rounding of the product and of the slicer's own limits) of a slicer limit, where a
    float32 sum of another order may land on the other side"""
    g = np.stack([gr, gi], 1).reshape(-1) if slice_q else gr
    soft64 = gain * (np.stack([f64.real, f64.imag], 1).reshape(-1) if slice_q else f64.real)
    lo, hi = pm.slicer_limits(n_symbols)
    lim = np.unique(np.concatenate([lo, hi]).astype(np.float64))
    return np.min(np.abs(soft64[:, None] - lim[None, :]), 1) <= gain * g + 4 * pm.EPS * (np.abs(soft64) + 1)


@pytest.mark.parametrize("shape,alg,q", GRID)
def test_walk_vs_reference(ref, shape, alg, q):
    import csdr_amd
    import test_pulse_cpu as tp
    import test_psk31_cpu as tk
    taps = taps_of(shape)
    gain = 1.0 / rms_of(shape, alg, q)
    # twelve channels: a near-integer v is a matter of chance (about one symbol in some thousands), and one channel cut short then costs a twelfth at most
    x = case_signal(shape, alg, q, 4, n_channels=12, seed=2)
    total = kept = n_bytes = excepted = corrected = 0
    for ch in range(x.shape[0]):
        rf = tp.lib_fir(ref, x[ch], taps)
        rs, rerr, ridx, _ = tk.ref_timing(ref, rf, alg, shape[0], LOOP_GAIN, MAX_ERROR, bool(q))
        corrected += int(np.count_nonzero(np.diff(ridx) != shape[0]))
        k, f64, gr, gi, v = reference_prefix(shape, alg, q, x[ch], taps, ridx)
        total += ridx.size; kept += k
        y, e, i = csdr_amd.pulserx_debug_walk(params_of(shape, alg, q, taps), "filter", "timing", x[ch], with_extras=True)
        assert y.size >= k
        assert np.array_equal(i[:k].astype(np.int64), ridx[:k]), "indexes inside the prefix"
        for got in (y[:k], rs[:k]):
            assert np.all(np.abs(got.real.astype(np.float64) - f64.real[:k]) <= gr[:k]) and np.all(np.abs(got.imag.astype(np.float64) - f64.imag[:k]) <= gi[:k])
        for sq, ns in SLICES:
            b = csdr_amd.pulserx_debug_walk(params_of(shape, alg, q, taps, gain, ns, sq), "filter", "slice", x[ch])
            rsoft = (np.float32(gain) * (rs.view(np.float32) if sq else np.ascontiguousarray(rs.real))).astype(np.float32)
            rb = tp.lib_slicer(ref, rsoft, ns)
            kb = k * (2 if sq else 1)
            near = near_a_limit(f64[:k], gr[:k], gi[:k], gain, sq, ns)
            differs = b[:kb] != rb[:kb]
            assert not np.any(differs & ~near), "a byte differs away from every limit"
            n_bytes += kb; excepted += int(np.count_nonzero(near))
    print("shape %s alg %d q %d: prefix %d of %d symbols, %d of %d bytes near a limit, corrections on %.1f %%"
          % (shape, alg, q, kept, total, excepted, n_bytes, 100.0 * corrected / max(total, 1)))
    if can_correct(shape, alg):
        assert corrected >= 0.01 * total, "the reference alone corrects on at least 1 % of the symbols"
    assert kept >= 0.9 * total, "the compared prefix holds %d of %d symbols" % (kept, total)
    assert excepted <= 0.02 * n_bytes, "%d of %d bytes excepted" % (excepted, n_bytes)


# ------------------------------------------------------------------ 4. the boundary
DEVICE = ["csdr_amd_pulserx_create", "csdr_amd_pulserx_process", "csdr_amd_pulserx_max_out", "csdr_amd_pulserx_reset", "csdr_amd_pulserx_reset_channel",
          "csdr_amd_pulserx_get_channel", "csdr_amd_pulserx_set_channel", "csdr_amd_pulserx_set_lanes", "csdr_amd_pulserx_lanes",
          "csdr_amd_pulserx_force_generic", "csdr_amd_pulserx_kernel_name", "csdr_amd_pulserx_destroy", "csdr_amd_debug_pulserx_walk"]

CLIENT = r'''
#include "csdr_amd.h"
#include <stdio.h>
int main(void)
{
    static csdr_complexf x[400];
    static unsigned char out[400];
    float taps[9] = {0.05f, 0.1f, 0.15f, 0.2f, 0.2f, 0.15f, 0.1f, 0.05f, 0.f};
    csdr_amd_pulserx_params p = {taps, 9, 0, 8, 0.5f, 2.f, 1, 1.f, 4, 1};
    csdr_amd_pulserx_chan st = {0, 0, 0};
    long long cuts[2] = {3, 100};
    for (int i = 0; i < 400; i++) { x[i].i = (float)((i / 8) & 1 ? 1 : -1); x[i].q = (float)((i / 16) & 1 ? 1 : -1); }
    long long k = csdr_amd_debug_pulserx_walk(&p, CSDR_AMD_PULSERX_FILTER, CSDR_AMD_PULSERX_SLICE, x, 400, cuts, 2, out, NULL, NULL, &st);
    printf("%lld %d %u\n", k, st.tail_len, st.base);
    /* the device entry points: referenced, and refused without an object */
    void *fns[] = {(void *)csdr_amd_pulserx_create, (void *)csdr_amd_pulserx_process, (void *)csdr_amd_pulserx_reset, (void *)csdr_amd_pulserx_reset_channel,
                   (void *)csdr_amd_pulserx_get_channel, (void *)csdr_amd_pulserx_set_channel, (void *)csdr_amd_pulserx_set_lanes, (void *)csdr_amd_pulserx_destroy};
    if (csdr_amd_pulserx_max_out(NULL, 5) != 0 || csdr_amd_pulserx_lanes(NULL) != 0 || csdr_amd_pulserx_force_generic(NULL, 1) >= 0) return 2;
    if (csdr_amd_pulserx_kernel_name(NULL)[0] != 0) return 3;
    return k > 0 && fns[0] ? 0 : 1;
}
'''


@pytest.fixture(scope="module")
def libpath():
    import csdr_amd
    if not os.path.exists(csdr_amd.LIB_PATH):
        csdr_amd.build()
    return csdr_amd.LIB_PATH


def test_new_symbols_are_exported_and_declared(libpath):
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not sorted(set(DEVICE) - exported)
    txt = open(os.path.join(ROOT, "include", "csdr_amd.h")).read()
    for n in DEVICE:
        assert n + "(" in txt, n


def test_c_client_links_and_runs(libpath, tmp_path):
    src = tmp_path / "c.c"
    src.write_text(CLIENT)
    exe = str(tmp_path / "c")
    r = subprocess.run(["gcc", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", os.path.dirname(libpath),
                        "-l:libcsdr_amd.so", "-Wl,-rpath," + os.path.dirname(libpath), "-o", exe, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr)
    k, tail_len, base = (int(v) for v in r.stdout.split())
    assert k > 60 and k % 2 == 0 and tail_len + base == 400          # two bytes per symbol, about 400 / 8 symbols; every sample is consumed or held
