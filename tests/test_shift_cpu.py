"""The shared-rate shifters without a GPU: tests/shift_model.py -- what tests/test_shift_gpu.py holds the device to, by bits -- against the C oracle, by
bits, end phase and status included, over every (variant, rate, phase, chunk, aux) the GPU file uses; the conditions the GPU file's inputs have to meet
(no sin / cos evaluation next to a rounding tie in a chunked case, at most n / 10^4 such samples in a MATH / TABLE case); and the model's invariance under
the cuts into calls."""
import ctypes as C
import numpy as np
import pytest
import shift_model as S

c64, f32 = np.complex64, np.float32


def bits(a): return np.ascontiguousarray(a).view(np.uint32)
def word(v): return np.array([v], f32).view(np.uint32)[0]


def crand(seed, *shape):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)).astype(c64)


def oracle_unroll(port, x, rate, chunk, size, phase):
    """shift_unroll_cc with a table of `size` >= chunk entries, called in chunks of `chunk` (Port.shift_unroll_cc has size == chunk only)"""
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    y, ds, dc = np.zeros_like(x), np.zeros(size, f32), np.zeros(size, f32)
    inc = port.L.orc_shift_unroll_init(C.c_float(rate), size, p(ds), p(dc))
    for pos in range(0, x.size, chunk):
        phase = port.L.orc_shift_unroll_cc(p(x[pos:]), p(y[pos:]), min(chunk, x.size - pos), p(ds), p(dc), C.c_float(inc), C.c_float(phase))
    return y, phase


def oracle_call(port, x, variant, rate, phase, chunk, aux):
    phase = float(phase)
    if variant == "addition": return port.shift_addition_cc(x, rate, chunk=chunk, phase=phase)
    if variant == "addfast": return port.shift_addfast_cc(x, rate, chunk=chunk, phase=phase)
    if variant == "unroll": return oracle_unroll(port, x, rate, chunk, S.unroll_size(chunk, aux), phase)
    if variant == "math": return port.shift_math_cc(x, rate, phase=phase)
    return port.shift_table_cc(x, rate, table_size=S.table_size(aux), phase=phase)


ALL_ROTATOR_CASES = S.CASES + S.TAIL_CASES + S.ahead_cases("math", "table") + S.ahead_cases("table", "math")


@pytest.mark.parametrize("case", ALL_ROTATOR_CASES, ids=S.case_id)
def test_model_is_the_oracle(port, case):
    variant, rate, phase, n, chunk, aux = case
    x = crand(41, n)
    r, end = S.rot(*case)
    y = S.mix_cc(x, r)
    o, po = oracle_call(port, x, variant, rate, phase, chunk, aux)
    w = S.addfast_written(n, chunk) if variant == "addfast" else np.ones(n, bool)      # ADDFAST leaves a chunk's len % 4 tail unwritten
    assert np.array_equal(bits(y[w]), bits(o[w]))
    assert word(end) == word(po)
    if variant == "addfast":
        assert np.array_equal(bits(r[~w]), bits(np.full(int((~w).sum()), 1 + 0j, c64)))


@pytest.mark.parametrize("n", S.MIX_LENGTHS)
def test_mix_models_are_the_oracle(port, n):
    """the mixing cases' rotator: complex input against shift_addition_cc, real input against shift_addition_fc"""
    variant, rate, phase, chunk, aux = S.MIX_ROT
    r, end = S.mix_rot(n)
    x = crand(42, n)
    o, po = port.shift_addition_cc(x, rate, chunk=chunk, phase=float(phase))
    assert np.array_equal(bits(S.mix_cc(x, r)), bits(o)) and word(end) == word(po)
    o, po = port.shift_addition_fc(x.real.copy(), rate, chunk=chunk, phase=float(phase))
    assert np.array_equal(bits(S.mix_fc(x.real, r)), bits(o)) and word(end) == word(po)
    assert np.array_equal(bits(S.mix_cc(np.stack([x, x[::-1]]), r)[1]), bits(S.mix_cc(x[::-1], r)))


@pytest.mark.parametrize("streams,decimation,n,calls", S.DSA)
def test_dsa_model_is_the_oracle(port, streams, decimation, n, calls):
    rates = [S.dsa_rate(s) for s in range(streams)]
    st_m = [(0, S.dsa_phase(s), 0) for s in range(streams)]
    st_o = list(st_m)
    silent = 0
    for call in range(calls):
        x = crand(43 + call, streams, n)
        one, st1 = S.dsa(x[0], rates[0], decimation, st_m[0])      # the one-stream form is row 0 of the vectorised one
        ys, st_m = S.dsa(x, rates, decimation, st_m)
        assert np.array_equal(bits(one), bits(ys[0])) and st1 == st_m[0]
        silent += st_m[0][2] == 0
        for s in range(streams):
            o, so = port.decimating_shift_addition_cc(x[s], float(rates[s]), decimation, (st_o[s][0], float(st_o[s][1]), st_o[s][2]))
            st_o[s] = so
            assert np.array_equal(bits(ys[s]), bits(o)), (call, s)
            assert (st_m[s][0], word(st_m[s][1]), st_m[s][2]) == (so[0], word(so[1]), so[2]), (call, s)
    if decimation > n:
        assert silent >= 2 and silent < calls            # some calls give no output, `remain` carries across them


def test_exempt_sets_of_the_gpu_cases():
    """the cap on the GPU file's inputs: nothing exempt in a chunked case (one flipped start phasor would change a whole chunk) or where a whole test
    hangs on one evaluation, at most n / 10^4 samples in a MATH / TABLE case"""
    total = 0
    for case in ALL_ROTATOR_CASES:
        variant, n = case[0], case[3]
        e = int(S.exempt(*case).sum())
        total += e
        if e: print(S.case_id(case), "exempt", e, "of", n)
        assert e <= (0 if variant in S.CHUNKED else n / 1e4), S.case_id(case)
    print("exempt samples over the rotator cases:", total)
    variant, rate, phase, chunk, aux = S.MIX_ROT
    for n in S.MIX_LENGTHS:
        assert not S.exempt(variant, rate, phase, n, chunk, aux).any(), n
    for streams, decimation, n, calls in S.DSA:            # the decimating shifter seeds its phasor from the status phase at every call
        rates, st = [S.dsa_rate(s) for s in range(streams)], [(0, S.dsa_phase(s), 0) for s in range(streams)]
        for call in range(calls):
            assert not S.near_tie_any([v[1] for v in st]).any(), (streams, decimation, call)
            _, st = S.dsa(np.zeros((streams, n), c64), rates, decimation, st)


def test_near_tie_marks_what_it_should():
    """the band is 1024 double ulps on either side of a midpoint, 2^-18 of the floats' spacing: evaluations next to a tie are rare, and widening the band
    to half a float ulp marks everything.  The count over 200 000 consecutive phases at rate -0.085 from 0.1 is printed."""
    ph = S.scan(-0.085, 0.1, 200000)[0]
    marked = int(S.near_tie(ph, np.sin).sum() + S.near_tie(ph, np.cos).sum())
    print("evaluations next to a tie among 400 000:", marked)
    assert marked <= 12                                    # 400 000 * 2^-18 = 1.5 expected
    old = S.BAND
    try:
        S.BAND = 2 ** 28                                   # half a float ulp in double ulps, and a little: every value is that close to a midpoint
        assert S.near_tie(ph[:1000], np.sin).all()
    finally:
        S.BAND = old
    # the distance near_tie measures, recomputed here: no value lies further from the nearer midpoint than half a float ulp
    x = ph[:4096]
    v = np.sin(x.astype(np.longdouble)); f = v.astype(f32)
    d = np.minimum(np.abs(v - (f.astype(np.longdouble) + np.nextafter(f, f32(np.inf)).astype(np.longdouble)) / 2),
                   np.abs(v - (f.astype(np.longdouble) + np.nextafter(f, f32(-np.inf)).astype(np.longdouble)) / 2))
    assert np.all(d <= np.spacing(np.abs(f)).astype(np.longdouble) / 2 * (1 + 1e-6))     # no value is further from a midpoint than half a float ulp


@pytest.mark.parametrize("variant,aux", [("math", 0), ("table", 65536), ("table", 16)])
def test_model_cut_invariance_per_sample(variant, aux):
    """MATH / TABLE: any cut into calls, the phase carried, gives the one call's rotator and end phase"""
    n = 2 * 1024 + 17
    for k, rate in enumerate(S.RATES):
        phase = f32(0.1 + 0.77 * k)
        whole, end = S.rot(variant, rate, phase, n, 1024, aux)
        parts, p = [], phase
        for ln in (1, 63, 1000, 0, 961, n - 2025):
            r, p = (np.zeros(0, c64), p) if not ln else S.rot(variant, rate, p, ln, 1024, aux)
            parts.append(r)
        assert np.array_equal(bits(np.concatenate(parts)), bits(whole)) and word(p) == word(end), rate


@pytest.mark.parametrize("variant,chunk,aux", [("addition", 1024, 0), ("addition", 100, 0), ("addition", 7, 0), ("addfast", 1000, 0), ("addfast", 7, 0),
                                               ("unroll", 100, 100), ("unroll", 1000, 1024)])
def test_model_cut_invariance_at_chunk_boundaries(variant, chunk, aux):
    """the chunked variants: calls that end on chunk boundaries, the phase carried, give the one call's rotator and end phase"""
    n = 2 * 1024 + 17
    for k, rate in enumerate(S.RATES):
        phase = f32(-3.0 + 0.77 * k)
        whole, end = S.rot(variant, rate, phase, n, chunk, aux)
        parts, p, pos = [], phase, 0
        for chunks in (1, 2, 1, 10 ** 6):
            ln = min(chunks * chunk, n - pos)
            if ln:
                r, p = S.rot(variant, rate, p, ln, chunk, aux)
                parts.append(r); pos += ln
        assert pos == n and np.array_equal(bits(np.concatenate(parts)), bits(whole)) and word(p) == word(end), rate
