"""ddc_reference.py checked against itself, without a GPU: the reference's phasor is what the float64 model multiplies with, the rates sit in the class the
gate assumes, the oracle's own three float32 stages pass the per-sample gate at every shape test_ddc_shapes_gpu.py runs (the gate is no tighter than honest
float32 arithmetic), mutations of the model fail it (the gate is not vacuous), and the schedules and the dispatch model reach what the GPU tests claim."""
import numpy as np
import pytest

import ddc_reference as dr
import fir_reference as fr

f32, c64 = np.float32, np.complex64
ROWS = (0, 3, 4, 5, 6)          # the distinct kinds of byte rows: random, all 0, all 255, I = 0 / Q = 255, clipped FM


def _stream_case(port, D, L, rate, taps, rows=ROWS):
    sizes, n = dr.schedule(D, L)
    u8 = dr.byte_rows(n, rate, 100 * D + L)
    R = dr.phasor_sequence(port, n, [(0, rate)])
    q = dr.weight_step(D, L, taps, rate)
    out = []
    for s in rows:
        y64, c, s1, s2 = dr.reference(port, u8[s], R, D, taps)
        out.append((s, u8[s], y64, c, s1, s2))
    return R, q, out


def _oracle_front(port, u8, rate, D, taps):
    sh, _ = port.shift_addition_cc(port.convert_u8_f(u8).view(c64), rate)
    return port.fir_decimate_cc(sh, D, taps)


@pytest.mark.parametrize("rate", dr.RATES_CHUNK + dr.RATES_DRIFT)
def test_reference_phasor_is_the_recurrence(port, rate):
    """R = shift_addition_cc(ones): (1 + 0j) (c + js) is exact, so R is the recurrence's float32 phasor itself -- replayed here in numpy float32 from every
    chunk's own seed, bit for bit; the seeds follow the float phase bookkeeping; and rotating a signal multiplies it with this R."""
    n = 1024 * 3 + 100
    R = dr.phasor_sequence(port, n, [(0, rate)])
    inc = f32(f32(f32(rate) * f32(2)) * dr.PI_F)
    cd, sd = f32(np.cos(np.float64(inc))), f32(np.sin(np.float64(inc)))
    ph, two_pi = f32(0), f32(2) * dr.PI_F
    for m in range(0, n, 1024):
        c, s = f32(R[m].real), f32(R[m].imag)
        assert c == f32(np.cos(np.float64(ph))) and s == f32(np.sin(np.float64(ph)))            # the seed: libm's (cos, sin) of the float starting phase
        ph = f32(ph + f32(inc * f32(min(1024, n - m))))                                         # libcsdr_gpl.c:48-51
        while ph > dr.PI_F:
            ph = f32(ph - two_pi)
        while ph < -dr.PI_F:
            ph = f32(ph + two_pi)
        for k in range(min(1024, n - m)):
            assert R[m + k].real == c and R[m + k].imag == s, (m, k)
            c, s = f32(f32(c * cd) - f32(s * sd)), f32(f32(s * cd) + f32(c * sd))
    x = fr.crand(np.random.default_rng(3), n)
    y, _ = port.shift_addition_cc(x, rate)
    want = x.astype(np.complex128) * R.astype(np.complex128)
    assert np.abs(y - want).max() <= 4 * dr.U * 2.0                                               # three roundings per component of |x| <= sqrt(2)


def test_rate_classes(port):
    """Every rate the GPU tests use is in the table, and sits in its class, clear of the library's switch (2e-6 RMS deviation of the recurrence from C_m d^k
    over a chunk): measured on 96 chunks of the reference's phasor."""
    used = {r for _, _, _, r in dr.SHAPES} | {r for _, _, rr in dr.RATE_SHAPES for r in rr}
    assert used <= set(dr.RATES_CHUNK + dr.RATES_DRIFT)
    assert {0.05, 0.25} & {r for D, _, _, r in dr.SHAPES if D <= 80} and {0.05, 0.25} & {r for D, _, _, r in dr.SHAPES if D > 80}
    n = 1024 * 96
    k = np.arange(n)
    for rate in dr.RATES_CHUNK + dr.RATES_DRIFT:
        R = dr.phasor_sequence(port, n, [(0, rate)])
        rho, chunk, gran = dr.rotator_rho(R, rate)
        Rd = R.astype(np.complex128)
        dev = np.abs(Rd / (Rd[(k >> 10) << 10] * dr.step_phasor(rate) ** (k & 1023)) - 1.0)
        rms = float(np.sqrt((dev[(k & 1023) >= 256] ** 2).mean()))
        print("RHO rate %8.4f  rho %.3g  chunk peak %.3g  chunk rms %.3g  granule peak %.3g" % (rate, rho, chunk, rms, gran))
        if rate in dr.RATES_CHUNK:
            assert chunk <= dr.RHO_SWITCH and rms < 1.5e-6 and rho == chunk
        else:
            assert chunk > 1.5 * dr.RHO_SWITCH and rms > 2.5e-6 and rho == gran + 2 * dr.U and rho < 1e-6


@pytest.mark.parametrize("D,L,Lo,rate", dr.SHAPES)
def test_oracle_stages_pass_the_gate(port, D, L, Lo, rate):
    """the reference measured against the reference: convert_u8_f | shift_addition_cc | fir_decimate_cc in float32 (a sequential sum) under the gate"""
    for kind, taps in [("random", fr.random_taps(L, D + L))] + ([("lowpass", port.firdes_lowpass_f(Lo, 0.5 / D))] if Lo else []):
        Lt = taps.size
        R, q, cases = _stream_case(port, D, Lt, rate, taps)
        rho = dr.rotator_rho(R, rate)[0]
        worst = 0.0
        for s, u8, y64, c, s1, s2 in cases:
            y = _oracle_front(port, u8, rate, D, taps)
            assert y.size == y64.size and np.all(c > 0)
            g = dr.gate_ratio(y, y64, dr.bound(c, s1, s2, Lt, q, rho))
            assert g <= 1.0, "row %d: %.3g x the gate" % (s, g)
            worst = max(worst, g)
        print("RATIO oracle D=%d L=%d %s rate=%g worst %.4f" % (D, Lt, kind, rate, worst))


@pytest.mark.parametrize("D,L,Lo,rate", dr.SHAPES)
def test_mutations_fail_the_gate(port, D, L, Lo, rate):
    """Subtly wrong models of the front end on random bytes and random taps: each exceeds the gate."""
    taps = fr.random_taps(L, D + L)
    sizes, n = dr.schedule(D, L)
    u8 = dr.byte_rows(n, rate, 100 * D + L)[0]
    R = dr.phasor_sequence(port, n, [(0, rate)])
    y64, c, s1, s2 = dr.reference(port, u8, R, D, taps)
    bnd = dr.bound(c, s1, s2, L, dr.weight_step(D, L, taps, rate), dr.rotator_rho(R, rate)[0])
    assert dr.gate_ratio(y64, y64, bnd) == 0.0
    d = dr.step_phasor(rate)
    k = np.arange(n)

    def model(taps=taps, R=R, u8=u8, offset=0.5):
        h = np.asarray(taps, f32).astype(np.float64)
        v = u8.astype(np.float64) - 128.0 + offset
        z = np.asarray(R).astype(np.complex128) * (v[0::2] + 1j * v[1::2]) * (2.0 / 255.0)
        return fr._corr(z.real, h, D, y64.size) + 1j * fr._corr(z.imag, h, D, y64.size)

    assert dr.gate_ratio(model(), y64, bnd) <= 0.05                 # the mutated model's own form agrees with the reference (u8 -> float in double)
    muts = {"reversed taps": model(taps=taps[::-1].copy())}
    for name, t in (("first", 0), ("middle", L // 2), ("last", L - 1)):
        z = taps.copy(); z[t] = 0
        muts["zeroed %s tap" % name] = model(taps=z)
    m = (n // 1024) // 2                                             # one chunk seeded like its neighbour
    Rm = R.astype(np.complex128).copy()
    Rm[1024 * m:1024 * (m + 1)] = Rm[1024 * (m + 1)] * d ** np.arange(1024)
    muts["neighbouring chunk's seed"] = model(R=Rm)
    muts["no +0.5 byte offset"] = model(offset=0.0)
    sw = u8.copy(); sw[0::2] = u8[1::2]; sw[1::2] = u8[0::2]
    muts["I and Q swapped"] = model(u8=sw)
    Rc = R.astype(np.complex128)
    muts["conjugated d"] = Rc[(k >> 10) << 10] * np.conj(d) ** (k & 1023)
    muts["conjugated d"] = model(R=muts["conjugated d"])
    for name, y in muts.items():
        g = dr.gate_ratio(y, y64, bnd)
        print("MUTATION D=%d L=%d %s: %.3g x the gate" % (D, L, name, g))
        assert g > 1.0, name


def test_schedules_and_dispatch_model():
    """The call schedules have the properties the GPU tests are built on, and the dispatch model names, over the shapes, every k_ddc_mfma<13,NT,false,PS>
    instance in both call classes and k_ddc_direct alone (the fused instances: test_ddc_shapes_gpu.py's chain tests)."""
    seen = set()
    for D, L, _, _ in dr.SHAPES:
        sizes, n = dr.schedule(D, L)
        assert n <= 1024 * 96 and len(sizes) >= 3 and all(s % 1024 == 0 for s in sizes) and 1024 in sizes and (n - sum(sizes)) % 1024
        assert ((sizes[0] - L) // D) // 8 + 1 >= 33                 # tiles of the first call
        partial_first = partial_last = False
        pos = 0
        for T in sizes:
            k_first = (pos - L) // D + 1 if pos >= L else 0
            k_hi = (pos + T - L) // D
            if dr.ddc_instance(D, L, False, False, T, B=pos).endswith("whole"):
                partial_first |= k_first % 8 != 0
                partial_last |= (k_hi + 1) % 8 != 0
            pos += T
        # (2, 1025): calls are multiples of 1024 = 64 tiles, and the first output of a call, B / 2 - 512, is a tile's first: every whole call is whole tiles
        assert (partial_first and partial_last) or (D, L) == (2, 1025), (D, L)
        nt = 2 if D <= 80 else 1
        got = dr.ddc_instances(D, L, False, False, sizes, n)
        assert got == {"k_ddc_mfma<13,%d,false,false> whole" % nt, "k_ddc_direct", "k_ddc_mfma<13,%d,false,false> tiles + k_ddc_direct" % nt}, (D, got)
        assert dr.ddc_instances(D, L, False, False, sizes, n, teams=1) == {g.replace("<13,2,", "<13,1,") for g in got}
        seen |= got
    for D, L, _ in dr.RATE_SHAPES:
        sizes, n = dr.schedule(D, L)
        seen |= dr.ddc_instances(D, L, True, False, sizes, n, retunes={2: [(1, 0.3)]} if D == 100 else None)
    for nt in (1, 2):
        assert "k_ddc_mfma<13,%d,false,false> whole" % nt in seen and "k_ddc_mfma<13,%d,false,false> tiles + k_ddc_direct" % nt in seen
        assert "k_ddc_mfma<13,%d,false,true> whole" % nt in seen
    assert "k_ddc_direct" in seen and "k_ddc_mfma<13,1,false,true> whole + k_ddc_direct" in seen
    # shapes outside the matrix-core kernel, unaligned rows, calls without an output
    assert dr.ddc_instance(25, 401, False, False, 1024 * 24) == "k_ddc_direct" and dr.ddc_instance(50, 801, False, False, 1024 * 24, aligned=False) == "k_ddc_direct"
    assert dr.ddc_instance(50, 1025, False, False, 1024) == "" and dr.ddc_instance(164, 6, False, False, 1024 * 64) == "k_ddc_direct"
    assert dr.ddc_instance(50, 801, False, True, 1024 * 64, B=1024 * 8) == "k_ddc_mfma<13,2,true,false> whole"
    assert dr.ddc_instance(100, 451, True, True, 1024 * 64, teams=2) == "k_ddc_mfma<13,1,true,true> whole"
    assert dr.ddc_instance(164, 4, True, False, 1024 * 64, drifting=True) == "k_ddc_direct" == dr.ddc_instance(150, 99, True, False, 1024 * 64, drifting=True)
    assert dr.ddc_instance(164, 4, True, False, 1024 * 64) == "k_ddc_mfma<13,1,false,true> whole" == dr.ddc_instance(150, 100, True, False, 1024 * 64, drifting=True)
