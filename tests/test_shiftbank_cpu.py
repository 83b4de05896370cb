"""The shifter bank without a GPU: csdr_amd_debug_shiftbank_walk runs the kernels' step functions (shiftbank_dev.hpp) on the host for one stream, cut into
calls.  Checked against the CPU oracle and the compiled reference at the gates the shared-rate shifters have in tests/test_gpu_parity.py (ADDITION: relative
RMS < 1e-6, end phase within 1e-6; MATH / TABLE: TOL and 1e-5), for invariance under the cuts, for the retune rule and for the chunk-phase pre-pass."""
import numpy as np
import pytest
from oracle import relrms
import shiftbank_model as M

c64, f32 = np.complex64, np.float32
TOL = 1e-5
CUTS = (1, 63, 1000, 0, 961)
RATES = M.RATES
# (variant, chunk, aux, samples)
SHAPES = [("addition", 1024, 0, 2 * 1024 + 17), ("addition", 100, 0, 3 * 100 + 7), ("math", 1024, 0, 2 * 1024 + 17),
          ("table", 1024, 65536, 2 * 1024 + 17), ("table", 1024, 16, 3 * 100 + 7)]


@pytest.fixture(scope="module")
def ca():
    import csdr_amd
    csdr_amd.lib()
    return csdr_amd


def crand(rng, n):
    return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(c64)


def start_phase(variant, k):
    """every stream its own start phase, inside the variant's wrap range"""
    return f32(-3.0 + 0.77 * k) if variant == "addition" else f32(0.1 + 0.77 * k)


def chan(ca, rate, phase):
    return ca.ShiftBankChan(rate=rate, phase=phase, c=1.0, s=0.0, pos=0, pending=0, old_rate=rate, pad=0)


def fields(st):
    return tuple(np.array([getattr(st, n)]).view(np.uint32)[0] for n, _ in st._fields_)


def oracle_call(o, variant, x, rate, chunk, aux, phase):
    if variant == "addition":
        return o.shift_addition_cc(x, rate, chunk=chunk, phase=phase)
    if variant == "math":
        return o.shift_math_cc(x, rate, phase=phase)
    return o.shift_table_cc(x, rate, table_size=aux, phase=phase)


def against(ca, o, variant, chunk, aux, n):
    rng = np.random.default_rng(21)
    for k, rate in enumerate(RATES):
        x = crand(rng, n)
        ph = start_phase(variant, k)
        st = chan(ca, rate, ph)
        y = ca.shiftbank_debug_walk(variant, rate, x, chunk=chunk, aux=aux, state=st)
        b, pb = oracle_call(o, variant, x, rate, chunk, aux, float(ph))
        e, dp = relrms(y, b), abs(float(M.end_phase(variant, st)) - float(pb))
        print(variant, chunk, aux, rate, "relrms", e, "end phase off by", dp)
        assert e < (1e-6 if variant == "addition" else TOL), (variant, rate)
        assert dp < (1e-6 if variant == "addition" else 1e-5), (variant, rate)


@pytest.mark.parametrize("variant,chunk,aux,n", SHAPES)
def test_walk_matches_oracle(ca, port, variant, chunk, aux, n):
    against(ca, port, variant, chunk, aux, n)


@pytest.mark.parametrize("variant,chunk,aux,n", SHAPES)
def test_walk_matches_compiled_reference(ca, ref, variant, chunk, aux, n):
    against(ca, ref, variant, chunk, aux, n)


def test_real_input_walk_matches_oracle(ca, port):
    rng = np.random.default_rng(22)
    for k, rate in enumerate(RATES):
        x = rng.uniform(-1, 1, 2 * 1024 + 17).astype(f32)
        st = chan(ca, rate, start_phase("addition", k))
        y = ca.shiftbank_debug_walk("addition", rate, x, in_format="f32", state=st)
        b, pb = port.shift_addition_fc(x, rate, phase=float(start_phase("addition", k)))
        assert relrms(y, b) < 1e-6 and abs(float(M.end_phase("addition", st)) - float(pb)) < 1e-6, rate


@pytest.mark.parametrize("variant,chunk,aux,in_format", [("addition", 1024, 0, "cf32"), ("addition", 100, 0, "cf32"), ("addition", 1024, 0, "f32"),
                                                         ("math", 1024, 0, "cf32"), ("table", 1024, 4096, "cf32")])
def test_cut_invariance(ca, variant, chunk, aux, in_format):
    """the stream in calls of 1, 63, 1000, 0, 961 samples and the rest equals one call, by bits: outputs and the final channel record"""
    rng = np.random.default_rng(23)
    n = 2 * 1024 + 17
    for k, rate in enumerate(RATES):
        x = rng.uniform(-1, 1, n).astype(f32) if in_format == "f32" else crand(rng, n)
        one, cut = chan(ca, rate, start_phase(variant, k)), chan(ca, rate, start_phase(variant, k))
        a = ca.shiftbank_debug_walk(variant, rate, x, chunk=chunk, aux=aux, in_format=in_format, state=one)
        b = ca.shiftbank_debug_walk(variant, rate, x, chunk=chunk, aux=aux, in_format=in_format, cuts=CUTS, state=cut)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), rate
        assert fields(one) == fields(cut), rate
        assert one.pos == (n % chunk if variant == "addition" else 0) and one.pending == 0


@pytest.mark.parametrize("variant,chunk,aux", [("addition", 64, 0), ("math", 1024, 0), ("table", 1024, 64)])
def test_walk_is_the_model(ca, variant, chunk, aux):
    """the float32 numpy model (tests/shiftbank_model.py), cuts and a retune included, by bits"""
    rng = np.random.default_rng(24)
    x = crand(rng, 2 * 64 + 41)
    for k, rate in enumerate(RATES):
        new = RATES[(k + 3) % len(RATES)]
        st = chan(ca, rate, start_phase(variant, k))
        y = ca.shiftbank_debug_walk(variant, rate, x, chunk=chunk, aux=aux, cuts=(70, 0), call_rates=(None, new, None), state=st)
        m = M.ShiftModel(variant, rate, chunk=chunk, table_size=aux or 65536, phase=start_phase(variant, k))
        parts = [m.process(x[:70])]
        m.set_rate(new)
        parts += [m.process(x[70:70]), m.process(x[70:])]
        assert np.array_equal(y.view(np.uint32), np.concatenate(parts).view(np.uint32)), rate
        got = (f32(st.rate), f32(st.phase), f32(st.c), f32(st.s), st.pos, st.pending, f32(st.old_rate))
        assert [np.array([v]).view(np.uint32)[0] if isinstance(v, f32) else v for v in got] == \
               [np.array([v]).view(np.uint32)[0] if isinstance(v, f32) else v for v in m.record()], rate


@pytest.mark.parametrize("at", [1024 + 300, 2048])
@pytest.mark.parametrize("variant", ["addition", "math", "table"])
def test_retune(ca, port, variant, at):
    """a rate change mid-chunk (after 1024 + 300 samples) and on a chunk boundary (after 2048) equals the oracle called piecewise on the blocks the rule
    implies: the block in front of the retune ends there (the reference's own phase for a short block), the next one starts with the new rate"""
    rng = np.random.default_rng(25)
    n = 3 * 1024 + 100
    for k, rate in enumerate(RATES):
        new = RATES[(k + 5) % len(RATES)]
        x = crand(rng, n)
        ph = start_phase(variant, k)
        st = chan(ca, rate, ph)
        y = ca.shiftbank_debug_walk(variant, rate, x, aux=65536 if variant == "table" else 0, cuts=(at,), call_rates=(None, new), state=st)
        b1, p1 = oracle_call(port, variant, x[:at], rate, 1024, 65536, float(ph))
        b2, p2 = oracle_call(port, variant, x[at:], new, 1024, 65536, float(p1))
        assert relrms(y, np.concatenate([b1, b2])) < (1e-6 if variant == "addition" else TOL), (rate, new)
        assert abs(float(M.end_phase(variant, st)) - float(p2)) < (1e-6 if variant == "addition" else 1e-5), (rate, new)
        assert st.pending == 0 and f32(st.rate) == f32(new) and f32(st.old_rate) == f32(new)
        assert st.pos == ((n - at) % 1024 if variant == "addition" else 0)
        # the state right behind the retune's first call of one sample: a new chunk began at that sample, from the closed chunk's phase
        if variant == "addition":
            s2 = chan(ca, rate, ph)
            ca.shiftbank_debug_walk(variant, rate, x[:at + 1], cuts=(at,), call_rates=(None, new), state=s2)
            closed = M.advance(M.advance(ph, rate, 1024), rate, at - 1024) if at % 1024 else M.advance(M.advance(ph, rate, 1024), rate, 1024)
            assert s2.pos == 1 and f32(s2.phase).view(np.uint32) == f32(closed).view(np.uint32), (rate, new)


@pytest.mark.parametrize("chunk", [1024, 100])
def test_chunk_phase_prepass_is_the_wrap_loop(ca, chunk):
    """the pre-pass's chunk step (seeds.hpp's wrap_plan_apply where the plan covers the step, the loop beyond) against the wrap loop, by bits, over 4096
    consecutive chunks for each rate"""
    for k, rate in enumerate(RATES):
        ph = start_phase("addition", k)
        got = ca.shiftbank_chunk_phases(rate, ph, chunk, 4096)
        for j in range(4096):
            ph = M.advance(ph, rate, chunk)
            assert got[j].view(np.uint32) == ph.view(np.uint32), (rate, j)


def test_refusals(ca):
    x = np.zeros(8, c64)
    for variant in ("unroll", "addfast"):
        with pytest.raises(ca.CsdrAmdError, match="one rate per call"):
            ca.shiftbank_debug_walk(variant, 0.1, x)
    with pytest.raises(ca.CsdrAmdError, match="chunk"):
        ca.shiftbank_debug_walk("addition", 0.1, x, chunk=0)
    with pytest.raises(ca.CsdrAmdError, match="ADDITION only"):
        ca.shiftbank_debug_walk("math", 0.1, np.zeros(8, f32), in_format="f32")
    assert ca.lib().csdr_amd_shiftbank_create(None, 0, 1, None, 1024, 0, 0, 1024) is None
    assert b"null context" in ca.lib().csdr_amd_last_error()
