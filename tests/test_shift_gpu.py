"""The shared-rate shifters on the GPU (csdr_amd/csrc/shift.hip) against tests/shift_model.py by words: the rotator table of every variant as
csdr_amd_rotator_generate leaves it on the device, the phase it hands back, and the mixed output of every instance of the mixing kernels, the scan that
runs ahead of MATH / TABLE, the decimating shifter and ADDFAST's tails.

The gate is derived, not measured: host and device run the same float32 operations in the same order with contraction off, so every word is equal except
where the device's and the host's double sin / cos round to different floats, which can only happen where the exact value lies next to a float rounding
tie.  shift_model.exempt marks those samples (within 1024 double ulps of a midpoint); there a rotator component may be one float away, everywhere else the
words are equal.  tests/test_shift_cpu.py holds the inputs used here to at most n / 10^4 exempt samples (none in the chunked cases) and the model to the
C oracle by bits.  Every case prints how many samples were exempt and how many of those differed."""
import ctypes as C
import numpy as np
import pytest
import shift_model as S

pytestmark = pytest.mark.gpu
c64, f32 = np.complex64, np.float32


@pytest.fixture(scope="module")
def gpu():
    import torch  # noqa: F401  (loads the HIP runtime torch bundles first, as bench.py does)
    import csdr_amd
    ctx = csdr_amd.Context(0)
    assert ctx.arch().startswith("gfx950")
    yield ctx
    ctx.close()


def bits(a): return np.ascontiguousarray(a).view(np.uint32)
def word(v): return np.array([v], f32).view(np.uint32)[0]


def crand(seed, *shape):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)).astype(c64)


X = crand(51, 65, 4100)
X.setflags(write=False)


def rot_equals_model(got, got_phase, case, what=""):
    """the device's rotator table against the model: words outside the exempt set, one float at the most inside it; the phase by its word"""
    want, want_phase = S.rot(*case)
    e = S.exempt(*case)
    differs = (bits(got).reshape(-1, 2) != bits(want).reshape(-1, 2)).any(1)
    print("%s%s: %d samples, %d exempt, %d of those differ" % (what, S.case_id(case), got.size, int(e.sum()), int((differs & e).sum())))
    assert not (differs & ~e).any(), np.flatnonzero(differs & ~e)[:8]
    if e.any():
        assert S.ulps_apart(got.real[e], want.real[e]).max() <= 1 and S.ulps_apart(got.imag[e], want.imag[e]).max() <= 1
    assert word(got_phase) == word(want_phase)
    return want, e


# ---------------------------------------------------------------------------------------------------------------- a. rotator tables
@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_rotator_table(gpu, case):
    variant, rate, phase, n, chunk, aux = case
    got, p = gpu.rotator(variant, rate, float(phase), n, chunk, aux)
    rot_equals_model(got, p, case)


def test_unroll_refuses_a_table_smaller_than_the_chunk(gpu):
    import csdr_amd
    with pytest.raises(csdr_amd.CsdrAmdError, match=r"\(-3\).*table size 100 smaller than chunk 128"):
        gpu.rotator("unroll", 0.1, 0.0, 300, 128, 100)


# ---------------------------------------------------------------------------------------------------------------- b. k_mix_cc
def mixed_equals_model(gpu, x, in_pitch=None, out_pitch=None, in_offset=0, out_offset=0, in_place=False):
    """one call of the shifter over x [streams, n] with the mixing cases' rotator: every row equals the model by words, the phase too, and every element
    of the output buffer outside the rows is as it was"""
    variant, rate, phase, chunk, aux = S.MIX_ROT
    s, n = x.shape
    r, want_phase = S.mix_rot(n)
    flat, p = gpu.shift_cc(x, rate, variant, phase=float(phase), chunk=chunk, aux=aux, in_pitch=in_pitch, out_pitch=out_pitch, in_offset=in_offset,
                           out_offset=out_offset, in_place=in_place, full=True)
    op, oo = ((in_pitch or n), in_offset) if in_place else ((out_pitch or n), out_offset)
    rows = flat[oo:oo + s * op].reshape(s, op)
    assert np.array_equal(bits(rows[:, :n]), bits(S.mix_cc(x, r)))
    pad = c64(gpu.PAD)
    assert np.all(rows[:, n:] == pad) and np.all(flat[:oo] == pad) and np.all(flat[oo + s * op:] == pad)
    assert word(p) == word(want_phase)


# (id: the kernel instance and what selects it, streams, n, in_pitch, out_pitch, in_offset, out_offset, in_place)
MIX_CC = [("vec-even-n", 3, 4100, None, None, 0, 0, False),
          ("vec-odd-n-even-pitches-scalar-tail", 3, 4099, 4100, 4102, 0, 0, False),
          ("vec-padded-pitches", 3, 4100, 4106, 4110, 0, 0, False),
          ("vec-in-place", 3, 4100, 4102, None, 0, 0, True),
          ("vec-in-place-odd-n-scalar-tail", 3, 4099, 4100, None, 0, 0, True),
          ("vec-both-pointers-off-16-bytes", 3, 4100, 4100, 4100, 2, 2, False),
          ("scalar-by-odd-in-pitch-3-streams", 3, 4099, 4099, 4100, 0, 0, False),
          ("scalar-by-odd-out-pitch-3-streams", 3, 4099, 4100, 4101, 0, 0, False),
          ("scalar-by-odd-pitches-65-streams", 65, 4099, 4099, 4101, 0, 0, False),
          ("scalar-by-in-pointer-off-8-bytes", 3, 4100, 4100, 4100, 1, 0, False),
          ("scalar-by-out-pointer-off-8-bytes", 3, 4100, 4100, 4100, 0, 1, False),
          ("scalar-in-place-odd-pitch", 3, 4100, 4101, None, 0, 0, True),
          ("scalar-in-place-pointer-off-8-bytes", 3, 4100, 4100, None, 1, 1, True),
          ("vec-one-sample-scalar-tail-only", 3, 1, 2, 2, 0, 0, False),
          ("scalar-one-sample", 3, 1, 1, 1, 0, 0, False)]


@pytest.mark.parametrize("name,streams,n,in_pitch,out_pitch,in_offset,out_offset,in_place", MIX_CC, ids=[m[0] for m in MIX_CC])
def test_mix_cc_instance(gpu, name, streams, n, in_pitch, out_pitch, in_offset, out_offset, in_place):
    """which instance runs follows csdr_amd_mix_cc's rule: k_mix_cc<true> if both pointers (and the rotator's) are multiples of 16 bytes and both pitches
    are even, k_mix_cc<false> otherwise"""
    ip, op = in_pitch or n, (in_pitch or n) if in_place else (out_pitch or n)
    vec = not (ip & 1 or op & 1 or in_offset & 1 or (in_offset if in_place else out_offset) & 1)
    assert vec == name.startswith("vec")
    mixed_equals_model(gpu, X[:streams, :n], in_pitch, out_pitch, in_offset, out_offset, in_place)


@pytest.mark.parametrize("name,n,pitch", [("vec-2051-pairs-on-2048-lanes", 4102, None), ("vec-odd-n-pitch-4104-2051-pairs-and-tail", 4103, 4104),
                                          ("scalar-odd-pitch-4103-samples-on-2048-lanes", 4103, 4103)])
def test_mix_cc_grid_stride(gpu, name, n, pitch):
    """4096 streams cap the grid at 8 blocks of 256 lanes a stream: the lanes that take a second trip through the stride loop, every stream"""
    x = np.random.default_rng(52).random((4096, n, 2), dtype=f32).view(c64)[:, :, 0]
    mixed_equals_model(gpu, x, pitch, pitch)


# ---------------------------------------------------------------------------------------------------------------- c. k_mix_fc
@pytest.mark.parametrize("name,streams,n,in_pitch,out_pitch", [("3-streams-padded-pitches", 3, 4099, 4101, 4103), ("one-sample", 3, 1, None, None),
                                                               ("second-trip-of-the-stride-loop", 1, 512 * 256 + 257, None, None)])
def test_mix_fc(gpu, name, streams, n, in_pitch, out_pitch):
    x = np.random.default_rng(53).uniform(-1, 1, (streams, n)).astype(f32)
    r, _ = S.mix_rot(n)
    flat = gpu.mix_fc(x, r, in_pitch, out_pitch, full=True)
    op = out_pitch or n
    rows = flat[:streams * op].reshape(streams, op)
    assert np.array_equal(bits(rows[:, :n]), bits(S.mix_fc(x, r)))
    assert np.all(rows[:, n:] == c64(gpu.PAD)) and np.all(flat[streams * op:] == c64(gpu.PAD))
    assert np.array_equal(bits(gpu.mix_fc(x[0], r)), bits(S.mix_fc(x[0], r)))       # the one-stream form


def test_shift_addition_fc_is_the_model(gpu):
    variant, rate, phase, chunk, aux = S.MIX_ROT
    x = np.random.default_rng(54).uniform(-1, 1, 4099).astype(f32)
    r, want_phase = S.mix_rot(x.size)
    y, p = gpu.shift_addition_fc(x, rate, phase=float(phase), chunk=chunk)
    assert np.array_equal(bits(y), bits(S.mix_fc(x, r))) and word(p) == word(want_phase)


# ---------------------------------------------------------------------------------------------------------------- d. ShiftAhead
@pytest.mark.parametrize("first,other", [("math", "table"), ("table", "math")])
def test_scan_ahead(first, other):
    """csdr_amd_rotator_generate's rule: a MATH / TABLE call finds its scan done if the call before it on the context had the same rate and the same
    length and handed back the phase this call comes with, whichever of the two variants either call was.  Of the eight calls (shift_model.ahead_calls)
    the 2nd, 3rd, 5th and 8th do: the counter reads 0 1 2 2 3 3 3 4.  Hit or miss, every output and every phase is the model's continuation."""
    import torch  # noqa: F401
    import csdr_amd
    ctx = csdr_amd.Context(0)                            # its own context: the counter starts at 0
    try:
        assert ctx.shift_scans_ahead() == 0
        calls, cases = S.ahead_calls(first, other), S.ahead_cases(first, other)
        assert [c[4] for c in calls] == [False, True, True, False, True, False, False, True]
        p, hits = None, 0
        for k, (variant, rate, n, phase, hit) in enumerate(calls):
            p = p if phase is None else phase
            x = X[k, :n]
            y, got_phase = ctx.shift_cc(x, rate, variant, phase=float(p))
            hits += hit
            assert ctx.shift_scans_ahead() == hits, (k, variant, rate, n)
            case = cases[k]
            assert case[:2] == (variant, rate) and word(case[2]) == word(p)
            want, want_phase = S.rot(*case)
            e = S.exempt(*case)
            differs = (bits(y).reshape(-1, 2) != bits(S.mix_cc(x, want)).reshape(-1, 2)).any(1)
            print("call %d %s: %d exempt, %d of those differ" % (k, S.case_id(case), int(e.sum()), int((differs & e).sum())))
            assert not (differs & ~e).any(), (k, np.flatnonzero(differs & ~e)[:8])
            assert word(got_phase) == word(want_phase), k
            p = f32(got_phase)
        assert hits == 4
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- e. k_dsa
@pytest.mark.parametrize("streams,decimation,n,calls", S.DSA, ids=["%d-streams-decimation-%d-input-%d-calls-%d" % d for d in S.DSA])
def test_decimating_shifter(gpu, streams, decimation, n, calls):
    """a rate, a start phase and a row of dsa data per stream, padded pitches, the status carried over the calls: outputs and status by words"""
    rates = [S.dsa_rate(s) for s in range(streams)]
    st_m = [(0, S.dsa_phase(s), 0) for s in range(streams)]
    st_g = [(0, float(S.dsa_phase(s)), 0) for s in range(streams)]
    op = n // decimation + 5
    silent = 0
    for call in range(calls):
        x = crand(55 + call, streams, n)
        want, st_m = S.dsa(x, rates, decimation, st_m)
        ys, st_g, flat = gpu.decimating_shift_addition_cc(x, rates, decimation, st_g, in_pitch=n + 3, out_pitch=op, full=True)
        rows = flat[:streams * op].reshape(streams, op)
        for s in range(streams):
            assert (st_g[s][0], word(st_g[s][1]), st_g[s][2]) == (st_m[s][0], word(st_m[s][1]), st_m[s][2]), (call, s)
            assert np.array_equal(bits(ys[s]), bits(want[s])), (call, s)
            assert np.all(rows[s, st_g[s][2]:] == c64(gpu.PAD)), (call, s)
        assert np.all(flat[streams * op:] == c64(gpu.PAD))
        silent += st_g[0][2] == 0
    if decimation > n:
        assert 2 <= silent < calls                       # calls without an output, `remain` carried across them
    if streams == 1:                                     # the one-stream form of the wrapper, as its callers use it
        x = crand(60, n)
        y, st = gpu.decimating_shift_addition_cc(x, float(rates[0]), decimation, (1, float(S.dsa_phase(0)), 0))
        want, st_w = S.dsa(x, rates[0], decimation, (1, S.dsa_phase(0), 0))
        assert np.array_equal(bits(y), bits(want)) and (st[0], word(st[1]), st[2]) == (st_w[0], word(st_w[1]), st_w[2])


# ---------------------------------------------------------------------------------------------------------------- f. refusal
def test_more_streams_than_grid_rows_are_refused(gpu):
    """grid.y carries the stream: 65535 streams run, 65536 are refused with -3 and a message in front of any launch -- the output stays as it was, the
    phase too, and no scan is started.  (Pitch 0: every stream reads and writes the one row, so the calls need no more memory than that.)"""
    L = gpu.L
    variant, rate, phase, chunk, aux = S.MIX_ROT
    n = 4
    r, end = S.mix_rot(n)
    x = X[0, :n]
    di, dr, dx = gpu.upload(x), gpu.upload(r), gpu.upload(x.real.copy())
    pad = np.full(n + 4, gpu.PAD, c64)
    hits = gpu.shift_scans_ahead()
    for streams, refused in ((65535, False), (65536, True), (1 << 20, True)):
        for name in ("mix_cc", "mix_fc", "shift_cc"):
            do = gpu.upload(pad)
            ph = C.c_float(float(phase))
            if name == "mix_cc": rc = L.csdr_amd_mix_cc(gpu.h, di.ptr, do.ptr, dr.ptr, streams, n, 0, 0)
            elif name == "mix_fc": rc = L.csdr_amd_mix_fc(gpu.h, dx.ptr, do.ptr, dr.ptr, streams, n, 0, 0)
            else: rc = L.csdr_amd_shift_cc(gpu.h, 1, rate, C.byref(ph), di.ptr, do.ptr, streams, n, 0, 0, chunk, aux)     # MATH: a launch would start a scan
            got = gpu.download(do, c64, n + 4)
            if refused:
                assert rc == -3 and ("%s: n_streams %d exceeds 65535" % (name, streams)) in gpu.err(), (name, streams, rc, gpu.err())
                assert np.array_equal(bits(got), bits(pad)) and ph.value == float(phase), (name, streams)
            else:
                assert rc == 0, (name, gpu.err())
                assert np.all(got[n:] == c64(gpu.PAD))
                if name == "mix_cc": assert np.array_equal(bits(got[:n]), bits(S.mix_cc(x, r)))
                if name == "mix_fc": assert np.array_equal(bits(got[:n]), bits(S.mix_fc(x.real, r)))
    assert gpu.shift_scans_ahead() == hits


# ---------------------------------------------------------------------------------------------------------------- g. ADDFAST's tails
@pytest.mark.parametrize("case", S.TAIL_CASES, ids=S.case_id)
def test_addfast_tails(gpu, case):
    """the samples the reference writes equal the model; each chunk's len % 4 tail, which the reference leaves unwritten, is the input (rot = 1 + 0j)"""
    variant, rate, phase, n, chunk, aux = case
    x = X[7, :n]
    y, p = gpu.shift_cc(x, rate, variant, phase=float(phase), chunk=chunk)
    r, want_phase = S.rot(*case)
    w = S.addfast_written(n, chunk)
    assert (~w).sum() == (n // chunk) * (chunk % 4) + (n % chunk) % 4 and (~w).any()
    assert np.array_equal(bits(y[w]), bits(S.mix_cc(x, r)[w]))
    assert np.array_equal(bits(y[~w]), bits(x[~w]))
    assert word(p) == word(want_phase)
