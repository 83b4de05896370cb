"""The fused WFM chain's de-emphasis at other tau / audio_rate than 50e-6 / 48000, on every path that cuts a call's audio into segments: k_wfm_mfma_seq at a shared
rate (segments of 120 samples at this shape) and at a rate per stream (columns of 512), the VALU fallback's k_wfm_back (a seam every 16 samples) and the resident
ring (a seam at every block start).  Every segment but a call's first warms up from zero state over 48 samples, which leaves b^48 of the true state at the seam
(wfm_deemph_model.py; tests/test_wfm_deemph_cpu.py shows that the cases below with b^48 >= 1.2e-4 break +-1 LSB under that warm-up).  Where b^48 > 2^-20 the
object has to take the exact route (csdr_amd_wfm_exact_deemphasis), and the ring has to refuse.

Gates, the project's own, against the oracle's stages with the same tau and audio_rate: every s16 sample within +-1 LSB, float audio relative RMS <= 1e-5, sample
counts within 2 of the oracle's.  Shape: D 10, 79 taps, F 5, 1024 * 60 samples per stream (1224 audio samples), 3 streams with different seeds."""
import numpy as np
import pytest
from oracle import relrms
from tests_helpers import wfm_signal_u8
import verify_configs as vc
import wfm_deemph_model as m

pytestmark = pytest.mark.gpu
c64, f32 = np.complex64, np.float32
TOL = 1e-5


@pytest.fixture(scope="module")
def gpu():
    import torch  # noqa: F401
    import csdr_amd
    ctx = csdr_amd.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def taps(port):
    return port.firdes_lowpass_f(m.L, 0.05)


def figures(s16, af, want, want_float=True):
    """per stream: (worst s16 difference, relative RMS of the float audio or None, samples got, samples wanted)"""
    out = []
    for s, (ps, pf) in enumerate(want):
        k = min(ps.size, s16.shape[1])
        out.append((int(vc.s16_diff(s16[s, :k], ps[:k]).max()), relrms(af[s, :k], pf[:k]) if want_float else None, s16.shape[1], ps.size))
    return out


def check(s16, af, want, what, want_float=True):
    fig = figures(s16, af, want, want_float)
    print("FIG %s: worst LSB %s, relrms %s, samples %s" % (what, [f[0] for f in fig], ["%.2e" % f[1] if f[1] is not None else "-" for f in fig], [f[2:] for f in fig]))
    for s, (lsb, rr, got, wanted) in enumerate(fig):
        assert 0 <= wanted - got <= 2 or 0 <= got - wanted <= 2, "%s stream %d: %d samples, oracle %d" % (what, s, got, wanted)
        assert lsb <= 1, "%s stream %d: %d LSB" % (what, s, lsb)
        if want_float:
            assert rr <= TOL, "%s stream %d: relrms %g" % (what, s, rr)


def warm(gpu, path):
    return gpu.L.csdr_amd_wfm_deemph_warm_samples(path)


@pytest.mark.parametrize("tau,ar", m.TR)
def test_shared_rate_one_call(gpu, port, taps, tau, ar):
    """a. one call cut into time segments (wfm_mfma_launch), every (tau, audio_rate): the gates; the route is the rule's at the chain kernel's warm-up; still the
    matrix-core chain kernel"""
    s16, af = gpu.wfm_chain(m.shared_inputs(), m.SHIFT, m.D, taps, frac_rate=m.F, tau=tau, audio_rate=ar)
    assert gpu.last_wfm_kernel == "k_wfm_mfma_seq"
    assert gpu.last_wfm_exact == m.rule(tau, ar, warm(gpu, 0)) == gpu.L.csdr_amd_wfm_deemph_exact(tau, ar, warm(gpu, 0))
    check(s16, af, m.oracle_audio(port, "shared", tau, ar), "shared %g/%d" % (tau, ar))


@pytest.mark.parametrize("want_float", [True, False])
@pytest.mark.parametrize("tau,ar", m.TR)
def test_rate_per_stream_one_call(gpu, port, taps, tau, ar, want_float):
    """b. a rate per stream: one workgroup = one stream x columns of 512 audio samples, every column but the first warmed up; with the float tap and without
    (the loaders' line-collecting store path)"""
    s16, af = gpu.wfm_chain(m.ps_inputs(), np.array(m.WRATES3, f32), m.D, taps, frac_rate=m.F, tau=tau, audio_rate=ar, want_float=want_float)
    assert gpu.last_wfm_kernel == "k_wfm_mfma_seq"
    assert gpu.last_wfm_exact == m.rule(tau, ar, warm(gpu, 0))
    check(s16, af, m.oracle_audio(port, "ps", tau, ar), "per stream %g/%d float %d" % (tau, ar, want_float), want_float)


@pytest.mark.parametrize("tau,ar", m.TR_FALLBACK)
def test_fallback(gpu, port, taps, tau, ar, monkeypatch):
    """c. k_wfm_front + k_wfm_back (forced: the variable is read when the object is created): a seam every 16 samples; the rule at k_wfm_back's warm-up"""
    monkeypatch.setenv("CSDR_AMD_WFM_PATH", "valu")
    s16, af = gpu.wfm_chain(m.shared_inputs(), m.SHIFT, m.D, taps, frac_rate=m.F, tau=tau, audio_rate=ar)
    assert gpu.last_wfm_kernel == "k_wfm_front"
    assert gpu.last_wfm_exact == m.rule(tau, ar, warm(gpu, 1))
    check(s16, af, m.oracle_audio(port, "shared", tau, ar), "fallback %g/%d" % (tau, ar))


SIZES = [1024 * 20, 1024 * 7, 1024 * 33]
RAGGED = 700
_calls = {}


def call_streams(port, taps, which):
    """the streams of the cases that come in several calls (the three sizes and a ragged last call of 700 samples) and their audio in front of the de-emphasis"""
    if which not in _calls:
        n = sum(SIZES) + RAGGED
        rates = [m.SHIFT] * m.S if which == "shared" else m.WRATES3
        u8 = np.stack([wfm_signal_u8(300 + s + (50 if which == "ps" else 0), n, offset=-rates[s]) for s in range(m.S)])
        pre = []
        for s in range(m.S):
            sh, _ = port.shift_addition_cc(port.convert_u8_f(u8[s]).view(c64), rates[s])
            dem, _ = port.fmdemod_quadri_cf(port.fir_decimate_cc(sh, m.D, taps))
            pre.append(port.fractional_decimator_ff(dem, float(m.F)))
        _calls[which] = (u8, pre)
    return _calls[which]


def want_of(port, pre, tau, ar, last=0.0):
    out = []
    for a in pre:
        de, _ = port.deemphasis_wfm_ff(a, tau, ar, last=last)
        out.append((port.convert_f_s16(de), de))
    return out


@pytest.mark.parametrize("out_per_call", [False, True])
@pytest.mark.parametrize("which", ["shared", "ps"])
@pytest.mark.parametrize("tau,ar", [(1e-3, 48000), (75e-6, 192000)])
def test_exact_route_calls_and_reset(gpu, port, taps, tau, ar, which, out_per_call):
    """d. the exact route's carried state: calls of 20, 7 and 33 chunks and a ragged last one of 700 samples (its state crosses every call boundary: b^48 = 0.37 at
    1 ms), both output layouts; then reset and the same stream again: the same bytes"""
    u8, pre = call_streams(port, taps, which)
    rates = m.SHIFT if which == "shared" else np.array(m.WRATES3, f32)
    s16, af = gpu.wfm_chain(u8, rates, m.D, taps, frac_rate=m.F, tau=tau, audio_rate=ar, block=SIZES + [RAGGED], out_per_call=out_per_call, repeat_after_reset=True)
    assert gpu.last_wfm_exact == 1 and gpu.last_wfm_kernel == "k_wfm_mfma_seq"
    check(s16, af, want_of(port, pre, tau, ar), "calls %s %g/%d per call %d" % (which, tau, ar, out_per_call))
    s16b, afb = gpu.wfm_repeat
    assert s16b.tobytes() == s16.tobytes() and afb.tobytes() == af.tobytes()


@pytest.mark.parametrize("start", [float("nan"), 0.37])
@pytest.mark.parametrize("which", ["shared", "ps", "valu"])
@pytest.mark.parametrize("tau,ar", [(1e-3, 48000), (50e-6, 48000)])
def test_start_state(gpu, port, taps, tau, ar, which, start, monkeypatch):
    """d. csdr_amd_wfm_set_deemphasis_state on the exact route (1 ms) and on the kernels' own (50 us), per kernel path: a start state of NaN restarts from 0 as the
    oracle's (libcsdr.c:1092); 0.37 shows that the state is used at all"""
    if which == "valu":
        monkeypatch.setenv("CSDR_AMD_WFM_PATH", "valu")
        which = "shared"
    rates = m.SHIFT if which == "shared" else np.array(m.WRATES3, f32)
    u8 = m.shared_inputs() if which == "shared" else m.ps_inputs()
    s16, af = gpu.wfm_chain(u8, rates, m.D, taps, frac_rate=m.F, tau=tau, audio_rate=ar, deemph_state=np.full(m.S, start, f32))
    assert gpu.last_wfm_exact == m.rule(tau, ar, 48)
    want = m.oracle_audio(port, which, tau, ar, last=start)
    if start == start:
        assert vc.s16_diff(want[0][0][:8], m.oracle_audio(port, which, tau, ar)[0][0][:8]).max() > 1000      # (the case means something)
    check(s16, af, want, "start state %s %g" % (which, start))


def test_exact_route_retune(gpu, port, taps):
    """e. csdr_amd_wfm_set_rate on the exact route: stream 1 retuned in front of the third call (the lead samples straddle two rates, k_wfm_lead) against the oracle
    composed stage by stage, its shift stage retuned at that sample"""
    tau, ar = 1e-3, 48000
    n = sum(SIZES)
    pos = SIZES[0] + SIZES[1]
    u8 = m.ps_inputs().copy()
    u8[1] = np.concatenate([wfm_signal_u8(2200, pos, offset=-0.11), wfm_signal_u8(2201, n - pos, offset=0.3)])
    s16, af = gpu.wfm_chain(u8, np.array(m.WRATES3, f32), m.D, taps, frac_rate=m.F, tau=tau, audio_rate=ar, block=SIZES, retunes={2: [(1, -0.3)]})
    assert gpu.last_wfm_exact == 1
    xf = port.convert_u8_f(u8[1]).view(c64)
    s1, ph = port.shift_addition_cc(xf[:pos], 0.11)
    s2, _ = port.shift_addition_cc(xf[pos:], -0.3, phase=ph)
    dem, _ = port.fmdemod_quadri_cf(port.fir_decimate_cc(np.concatenate([s1, s2]), m.D, taps))
    de, _ = port.deemphasis_wfm_ff(dem[10::5], tau, ar)          # fractional_decimator_ff 5 == x[5 k + 10] (exact at an integer rate)
    want = m.oracle_audio(port, "ps", tau, ar)
    check(s16, af, [want[0], (port.convert_f_s16(de), de), want[2]], "retune")


@pytest.mark.parametrize("tau,ar", [(75e-6, 96000), (1e-3, 48000)])
def test_ring_refuses(gpu, taps, tau, ar):
    """f. the resident grid stores s16 straight into its output ring: no second pass, so the parameters of the exact route are refused, by name"""
    import csdr_amd
    assert m.rule(tau, ar, warm(gpu, 2)) == 1
    with pytest.raises(csdr_amd.CsdrAmdError) as e:
        gpu.wfm_ring_chain(m.shared_inputs()[:2, :2 * 4096 * 12], m.SHIFT, m.D, taps, block=4096, n_slots=8, frac_rate=m.F, tau=tau, audio_rate=ar)
    msg = str(e.value)
    assert "%g" % tau in msg and str(ar) in msg and "csdr_amd_wfm_process" in msg, msg


def test_ring_accepts_44100(gpu, port, taps):
    """f. 50e-6 / 44100 (b^48 = 1.6e-8) through 12 blocks of 4096 samples, 2 streams: every block start is a seam 48 samples of warm-up in front of it"""
    tau, ar, nb = 50e-6, 44100, 12
    assert m.rule(tau, ar, warm(gpu, 2)) == 0
    u8 = m.shared_inputs()[:2, :2 * 4096 * nb]
    y = gpu.wfm_ring_chain(u8, m.SHIFT, m.D, taps, block=4096, n_slots=8, frac_rate=m.F, tau=tau, audio_rate=ar)
    want = [port.wfm_chain(u8[s], m.SHIFT, m.D, taps, frac_rate=m.F, tau=tau, audio_rate=ar) for s in range(2)]
    check(y, None, want, "ring 44100", want_float=False)
