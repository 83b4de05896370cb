"""GPU checks of carrier recovery (carrier.hip): both kernels against the CPU run of their step functions and the float32 model within the gate G (zero
differing words expected), equal bits between the kernels, every channels-per-wave choice, every cut into calls, every batch position, pitches and
output subsets, channel reset / set, the drop-in against the reference library, the CLI commands and the `csdr chain` stage, argument errors and lifecycle."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

import carrier_model as cm
from test_carrier_cpu import G, REF_LIB

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSDR = os.path.join(ROOT, "csdr_amd", "csdr")
ALL = ("out", "error", "dphase", "nco")
PLL_OUT = ("dphase", "nco")
TILE = 64                                   # k_carrier_tiled's samples per tile


@pytest.fixture(scope="module")
def ctx():
    import csdr_amd
    c = csdr_amd.Context(0)
    yield c
    c.close()


def _params(mode, alpha, beta, dphase_max):
    import csdr_amd
    return csdr_amd.CarrierParams(mode, alpha, beta, dphase_max, 0)


def _outputs(P):
    return ALL if P.mode <= cm.COSTAS_DD else PLL_OUT


def _family(P):
    return "costas" if P.mode <= cm.COSTAS_DD else "pll"


def _gpu(ctx, P, X, outputs=None, generic=False, lanes=0, calls=None, **kw):
    o = ctx.carrier(P, X.shape[0])
    o.force_generic(generic); o.set_lanes(lanes)
    r = o.process(X, outputs or _outputs(P), calls, **kw)
    assert o.kernel_name() == ("k_carrier" if generic else "k_carrier_tiled") or X.shape[1] == 0
    o.close()
    return r


def _walk(P, X, outputs=None):
    import csdr_amd
    rows = [csdr_amd.carrier_debug_walk(P, x, outputs or _outputs(P)) for x in X]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


def _same_bits(a, b, what):
    for k in b:
        d = cm.words_differing(a[k], b[k])
        assert d == 0, "%s: %s differs in %d words, largest deviation %.3g" % (what, k, d, cm.maxdev(a[k], b[k]))


def _within_gate(got, want, family, what):
    """maximum deviation <= G on every output; the number of differing words (zero expected: only a last-bit difference between the device's and the C
    library's double cos / sin / atan2 can make one) goes into the message"""
    for k in want:
        dev, words = cm.maxdev(got[k], want[k]), cm.words_differing(got[k], want[k])
        print("%s %s: largest deviation %.3g, %d differing words" % (what, k, dev, words))
        assert dev <= G[family, k], "%s: %s deviates by %.3g > G = %.3g (%d differing words)" % (what, k, dev, G[family, k], words)


def _batch(kind, case, n_ch, n):
    f = cm.costas_input if kind == "costas" else cm.pll_input
    return np.stack([f(case, n, channel=c) for c in range(n_ch)])


# one parameter set per mode for the equal-bits tests: (kind, case index)
MODES = [("costas", 0), ("costas", 2), ("pll", 2), ("pll", 6)]


def _mode_params(kind, case):
    return _params(*(cm.costas_mode_coefficients(case) if kind == "costas" else cm.pll_mode_coefficients(case)))


# ------------------------------------------------------------------ the kernels against the CPU walk and the model
@pytest.mark.parametrize("case", range(len(cm.COSTAS_CASES)))
def test_costas_vs_walk_and_model(ctx, case):
    P = _params(*cm.costas_mode_coefficients(case))
    X = _batch("costas", case, 5, cm.N)                              # channel 0 is the committed input of the model
    walk = _walk(P, X)
    model, mst = cm.model_costas(case)
    for generic in (False, True):
        got = _gpu(ctx, P, X, generic=generic)
        _within_gate(got, walk, "costas", "case %d generic %d against the CPU walk" % (case, generic))
        _within_gate({k: v[0] for k, v in got.items()}, model, "costas", "case %d generic %d against the model" % (case, generic))


@pytest.mark.parametrize("case", range(len(cm.PLL_CASES)))
def test_pll_vs_walk_and_model(ctx, case):
    P = _params(*cm.pll_mode_coefficients(case))
    X = _batch("pll", case, 5, cm.N)
    walk = _walk(P, X)
    model, mst = cm.model_pll(case)
    for generic in (False, True):
        got = _gpu(ctx, P, X, generic=generic)
        _within_gate(got, walk, "pll", "case %d generic %d against the CPU walk" % (case, generic))
        _within_gate({k: v[0] for k, v in got.items()}, model, "pll", "case %d generic %d against the model" % (case, generic))


# ------------------------------------------------------------------ equal bits by construction
@pytest.mark.parametrize("kind,case", MODES)
def test_tiled_equals_generic_every_lanes(ctx, kind, case):
    P = _mode_params(kind, case)
    X = _batch(kind, case, 130, 4097)
    want = _gpu(ctx, P, X, generic=True)
    for lanes in (1, 2, 3, 4, 7, 8, 15, 16, 33, 64):
        _same_bits(_gpu(ctx, P, X, lanes=lanes), want, "tiled, %d channels per wave" % lanes)
    for lanes in (1, 5, 64):
        _same_bits(_gpu(ctx, P, X, generic=True, lanes=lanes), want, "generic, %d channels per wave" % lanes)
    o = ctx.carrier(P, 130)
    assert 1 <= o.lanes() <= 64
    o.set_lanes(40); assert o.lanes() == 40
    o.force_generic(True); assert o.lanes() == 40
    o.close()


@pytest.mark.parametrize("kind,case", MODES)
def test_cut_invariance(ctx, kind, case):
    P = _mode_params(kind, case)
    sizes = [0, 1, 63, 64, 65, 4097]
    n = sum(sizes)
    X = _batch(kind, case, 5, n)
    for generic in (False, True):
        want = _gpu(ctx, P, X, generic=generic)
        for calls in (sizes, sizes[::-1], [TILE - 1, n - TILE + 1], [TILE, n - TILE], [TILE + 1, n - TILE - 1], [1] * 70 + [0, n - 70],
                      [2 * TILE - 1, 1, 1, n - 2 * TILE - 1]):
            assert sum(calls) == n
            _same_bits(_gpu(ctx, P, X, generic=generic, calls=calls), want, "generic %d calls %r" % (generic, calls[:6]))
    for m in sizes:                                                  # each sample count as a whole stream of its own
        Xm = X[:, :m]
        got = _gpu(ctx, P, Xm)
        _same_bits(got, _gpu(ctx, P, Xm, generic=True), "n = %d" % m)
        assert all(v.shape == (5, m) for v in got.values())


@pytest.mark.parametrize("kind,case", MODES[1:3])
def test_batch_position_invariance(ctx, kind, case):
    """a channel alone against the same channel at positions 0, C - 1, C and last of batches of 1, C, C + 1 and 130 channels"""
    P = _mode_params(kind, case)
    n, Cw = 1000, 4
    others = _batch(kind, case, 130, n)
    x0 = others[77].copy()
    alone = _gpu(ctx, P, x0[None], lanes=Cw)
    _same_bits(_gpu(ctx, P, x0[None], generic=True), alone, "alone, generic")
    for nb in (1, Cw, Cw + 1, 130):
        for pos in sorted({0, Cw - 1, Cw, nb - 1}):
            if pos >= nb:
                continue
            X = others[:nb].copy(); X[pos] = x0
            for generic in (False, True):
                got = _gpu(ctx, P, X, generic=generic, lanes=Cw)
                _same_bits({k: v[pos:pos + 1] for k, v in got.items()}, alone, "batch of %d, position %d, generic %d" % (nb, pos, generic))


@pytest.mark.parametrize("kind,case", MODES[1:3])
def test_pitch_and_output_subsets(ctx, kind, case):
    """pitches above n; each subset of the output pointers gives what all of them give; nothing is written beyond n in a row"""
    import itertools
    P = _mode_params(kind, case)
    names = _outputs(P)
    n, s = 333, 7
    X = _batch(kind, case, s, n)
    want = _gpu(ctx, P, X)
    for generic in (False, True):
        _same_bits(_gpu(ctx, P, X, generic=generic, in_pitch=n + 13, out_pitch=n + 7), want, "pitches, generic %d" % generic)
        for k in range(1, len(names) + 1):
            for sub in itertools.combinations(names, k):
                got = _gpu(ctx, P, X, outputs=sub, generic=generic)
                assert tuple(got) == sub
                _same_bits(got, {m: want[m] for m in sub}, "subset %r, generic %d" % (sub, generic))
    # the columns between n and the pitch keep what they held
    op = n + 7
    for generic in (False, True):
        o = ctx.carrier(P, s); o.force_generic(generic)
        di = ctx.upload(X)
        bufs = {m: ctx.upload(np.full((s, op), -7.5, np.complex64 if m in ("out", "nco") else np.float32)) for m in names}
        o.process_dev(di.ptr, n, n, *[bufs[m].ptr if m in bufs else None for m in ALL], op)
        for m in names:
            dt = np.complex64 if m in ("out", "nco") else np.float32
            y = ctx.download(bufs[m], dt, s * op).reshape(s, op)
            assert np.all(y[:, n:] == -7.5), m
            assert cm.words_differing(y[:, :n], want[m]) == 0, m
        o.close()


def test_unaligned_rows_take_the_generic_kernel(ctx):
    """an input 4 bytes off an 8-byte boundary is served by k_carrier: the same bits"""
    P = _mode_params("costas", 2)
    n, s = 200, 3
    X = _batch("costas", 2, s, n)
    want = _gpu(ctx, P, X)
    o = ctx.carrier(P, s)
    flat = np.zeros(2 * s * n + 1, np.float32); flat[1:] = X.view(np.float32).reshape(-1)
    di = ctx.upload(flat); do = ctx.alloc(8 * s * n + 64)
    o.process_dev(di.at(4), n, n, do.ptr, None, None, None, n)
    assert o.kernel_name() == "k_carrier"
    y = ctx.download(do, np.complex64, s * n).reshape(s, n)
    assert cm.words_differing(y, want["out"]) == 0
    o.close()


@pytest.mark.parametrize("kind,case", MODES[1:3])
def test_reset_and_set_channel(ctx, kind, case):
    import csdr_amd
    P = _mode_params(kind, case)
    names = _outputs(P)
    n, h, s = 2000, 777, 6
    X = _batch(kind, case, s, n)
    for generic in (False, True):
        whole = _gpu(ctx, P, X, generic=generic)
        o = ctx.carrier(P, s); o.force_generic(generic)
        first = o.process(X[:, :h], names)
        g = o.get_channel(1)                                         # the state read back starts another object where this one stands
        o2 = ctx.carrier(P, 1); o2.force_generic(generic); o2.set_channel(0, g)
        _same_bits(o2.process(X[1:2, h:], names), {k: whole[k][1:2, h:] for k in names}, "get_channel / set_channel")
        o2.close()
        o.reset_channel(2)
        o.set_channel(4, csdr_amd.CarrierChan(0.75, -0.02, 0.01))
        second = o.process(X[:, h:], names)
        o.close()
        for c in (0, 1, 3, 5):                                       # the neighbours carry on
            _same_bits({k: np.concatenate([first[k][c], second[k][c]]) for k in names}, {k: whole[k][c] for k in names}, "neighbour %d" % c)
        fresh = _gpu(ctx, P, X[2:3, h:], generic=generic)
        _same_bits({k: second[k][2:3] for k in names}, fresh, "reset channel")
        o1 = ctx.carrier(P, 1); o1.force_generic(generic); o1.set_channel(0, csdr_amd.CarrierChan(0.75, -0.02, 0.01))
        _same_bits({k: second[k][4:5] for k in names}, o1.process(X[4:5, h:], names), "set channel")
        o1.close()
        o = ctx.carrier(P, s); o.force_generic(generic)
        o.process(X[:, :h], names); o.reset()
        _same_bits(o.process(X[:, :h], names), first, "reset")
        o.close()


# ------------------------------------------------------------------ the drop-in
def _ours():
    import csdr_amd
    return cm.bind(C.CDLL(csdr_amd.lib()._name))


@pytest.mark.parametrize("case", [0, 1, 3, 5])
def test_dropin_costas(ctx, case):
    """bpsk_costas_loop_cc of libcsdr_amd.so and of the reference through one ctypes routine, in blocks of 1024, the state through the caller's struct"""
    A = _ours()
    bw, damping, dd, _, _ = cm.COSTAS_CASES[case]
    x = cm.costas_input(case)
    got, st = cm.drive_costas(A, x, bw, damping, dd, block=1024)
    model, mst = cm.model_costas(case)
    _within_gate(got, model, "costas", "drop-in case %d against the model" % case)
    if os.path.exists(REF_LIB):
        want, rst = cm.drive_costas(cm.bind(C.CDLL(REF_LIB)), x, bw, damping, dd, block=1024)
        _within_gate(got, want, "costas", "drop-in case %d against the reference" % case)
        assert (st.alpha, st.beta, st.dphase_max, st.dphase_max_reset_to_zero) == (rst.alpha, rst.beta, rst.dphase_max, rst.dphase_max_reset_to_zero)


@pytest.mark.parametrize("case", [1, 2, 5, 6])
def test_dropin_pll(ctx, case):
    A = _ours()
    kind, coef, _, _ = cm.PLL_CASES[case]
    x = cm.pll_input(case)
    got, st = cm.drive_pll(A, x, kind, coef, block=1024)
    model, mst = cm.model_pll(case)
    _within_gate(got, model, "pll", "drop-in case %d against the model" % case)
    if os.path.exists(REF_LIB):
        want, rst = cm.drive_pll(cm.bind(C.CDLL(REF_LIB)), x, kind, coef, block=1024)
        _within_gate(got, want, "pll", "drop-in case %d against the reference" % case)
        assert (st.alpha, st.pll_type) == (rst.alpha, rst.pll_type)


def test_dropin_keeps_the_reference_quirks(ctx):
    A = _ours()
    st = cm.CostasState(); st.decision_directed = 77
    A.init_bpsk_costas_loop_cc(C.byref(st), 0, 0.707, 0.05)
    assert st.decision_directed == 77
    assert (st.alpha, st.beta, st.dphase_max) == cm.costas_coefficients(0.05, 0.707)
    p = cm.PllState(); p.pll_type = 9; p.iir_temp = 3.5
    A.pll_cc_init_p_controller(C.byref(p), 0.25)
    assert (p.pll_type, p.iir_temp, p.alpha) == (9, 3.5, 0.25)
    p.dphase = 0.5
    x = np.ones(4, np.complex64); nco = np.full(4, 9 + 9j, np.complex64); dph = np.full(4, 9, np.float32)
    A.pll_cc(C.byref(p), cm._p(x), cm._p(dph), cm._p(nco), 4)
    assert p.output_phase == 0.5 and np.all(nco[1:] == 9 + 9j) and np.all(dph == 9)
    assert abs(nco[0] - (np.sin(0.5) + 1j * np.cos(0.5))) < 1e-6
    # NULL outputs: pll_cc without output_dphase, the Costas loop with `output` alone
    kind, coef, _, _ = cm.PLL_CASES[5]
    x = cm.pll_input(5)[:1500]
    model, _ = cm.pll(x, True, *cm.pll_pi_coefficients(coef))
    q = cm.pll_init(A, kind, coef); nco = np.zeros(x.size, np.complex64)
    A.pll_cc(C.byref(q), cm._p(x), None, cm._p(nco), x.size)
    _within_gate(dict(nco=nco), dict(nco=model["nco"]), "pll", "pll_cc with nco alone")


# ------------------------------------------------------------------ the CLI
def _run(cmd, data, timeout=120):
    r = subprocess.run(cmd, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout, r.stderr.decode()


def test_cli_costas(ctx, tmp_path):
    for case, dd_flag in ((0, []), (1, ["--dd"]), (5, ["--decision_directed"])):
        bw, damping, dd, _, _ = cm.COSTAS_CASES[case]
        x = cm.costas_input(case)[:5000]                              # not a multiple of the 1024-sample buffer: the tail is processed too
        model = {k: v[:5000] for k, v in cm.model_costas(case)[0].items()}
        base = [CSDR, "bpsk_costas_loop_cc", repr(bw), repr(damping)] + dd_flag
        out, err = _run(base, x.tobytes())
        _within_gate(dict(out=np.frombuffer(out, np.complex64)), dict(out=model["out"]), "costas", "cli case %d" % case)
        assert "alpha = " in err and ("decision directed mode" in err) == bool(dd)
        for flag, name, dt in (("--output_error", "error", np.float32), ("--output_dphase", "dphase", np.float32), ("--output_nco", "nco", np.complex64)):
            out, _ = _run(base + [flag], x.tobytes())
            _within_gate({name: np.frombuffer(out, dt)}, {name: model[name]}, "costas", "cli case %d %s" % (case, flag))
        files = [str(tmp_path / ("%s_%d.bin" % (k, case))) for k in ("error", "dphase", "nco")]
        out, _ = _run(base + ["--output_combined"] + files, x.tobytes())
        got = dict(out=np.frombuffer(out, np.complex64), error=np.fromfile(files[0], np.float32), dphase=np.fromfile(files[1], np.float32),
                   nco=np.fromfile(files[2], np.complex64))
        _within_gate(got, model, "costas", "cli case %d --output_combined" % case)


def test_cli_pll_and_chain(ctx):
    for case, args in ((0, ["1"]), (2, ["1", "0.1"]), (4, ["2"]), (6, ["2", "0.05", "0.707", "10", "0.1"])):
        x = cm.pll_input(case)[:5000]
        out, err = _run([CSDR, "pll_cc"] + args, x.tobytes())
        _within_gate(dict(nco=np.frombuffer(out, np.complex64)), dict(nco=cm.model_pll(case)[0]["nco"][:5000]), "pll", "cli pll_cc %s" % " ".join(args))
        assert ("alpha=" in err) == (args[0] == "2")
    # resident `csdr chain` stages
    x = cm.pll_input(6)
    out, _ = _run([CSDR, "chain", "pll_cc 2 0.05 | realpart_cf"], x.tobytes())
    _within_gate(dict(nco=np.frombuffer(out, np.float32)), dict(nco=np.ascontiguousarray(cm.model_pll(6)[0]["nco"].real)), "pll", "chain pll_cc | realpart_cf")
    x = cm.costas_input(1)
    out, _ = _run([CSDR, "chain", "gain_ff 1 | bpsk_costas_loop_cc 0.05 0.707 --dd | realpart_cf"], x.tobytes())
    _within_gate(dict(out=np.frombuffer(out, np.float32)), dict(out=np.ascontiguousarray(cm.model_costas(1)[0]["out"].real)), "costas", "chain costas | realpart_cf")


def test_cli_bad_argv(ctx):
    def fails(args, message):
        r = subprocess.run([CSDR] + args, input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr)
    fails(["bpsk_costas_loop_cc"], b"need required parameter (loop_bandwidth)")
    fails(["bpsk_costas_loop_cc", "0.05"], b"need required parameter (damping_factor)")
    fails(["bpsk_costas_loop_cc", "0.05", "0.707", "--output_combined", "a", "b"], b"need required parameters after --output_combined: <error_file> <dphase_file> <nco_file>")
    fails(["bpsk_costas_loop_cc", "0.05", "0.707", "--dd", "--output_combined"], b"need required parameters after --output_combined")
    fails(["pll_cc"], b"need required parameter (pll_type)")
    fails(["pll_cc", "3"], b"invalid pll_type. Valid values are:\n\t1: PLL_P_CONTROLLER\n\t2: PLL_PI_CONTROLLER")


# ------------------------------------------------------------------ argument errors and lifecycle
def test_argument_errors(ctx):
    import csdr_amd
    L = ctx.L
    good = csdr_amd.costas_params(0.05)
    for bad, n_ch in ((_params(4, 0.1, 0.1, 0.1), 1), (_params(-1, 0.1, 0.1, 0.1), 1), (good, 0), (good, -3), (_params(0, 0.1, 0.1, float("nan")), 1)):
        assert not L.csdr_amd_carrier_create(ctx.h, C.byref(bad), n_ch)
        assert b"carrier" in L.csdr_amd_last_error()
    x = ctx.upload(np.zeros((2, 64), np.complex64)); y = ctx.alloc(2 * 64 * 8 + 64)
    o = ctx.carrier(good, 2)
    assert L.csdr_amd_carrier_process(o.h, x.ptr, 64, 64, None, None, None, None, 64) == -3
    assert b"at least one of" in L.csdr_amd_last_error()
    assert L.csdr_amd_carrier_process(o.h, x.ptr, 64, 63, y.ptr, None, None, None, 64) == -3
    assert L.csdr_amd_carrier_process(o.h, x.ptr, 64, 64, y.ptr, None, None, None, 63) == -3
    assert L.csdr_amd_carrier_process(o.h, x.ptr, -1, 64, y.ptr, None, None, None, 64) == -3
    assert L.csdr_amd_carrier_process(o.h, x.ptr, 0, 0, y.ptr, None, None, None, 0) == 0            # a 0-sample call is a no-op
    with pytest.raises(csdr_amd.CsdrAmdError):
        o.reset_channel(2)
    with pytest.raises(csdr_amd.CsdrAmdError):
        o.set_channel(0, csdr_amd.CarrierChan(float("nan"), 0, 0))
    with pytest.raises(csdr_amd.CsdrAmdError):
        o.set_lanes(65)
    o.close()
    o = ctx.carrier(csdr_amd.pll_params(2), 2)
    assert L.csdr_amd_carrier_process(o.h, x.ptr, 64, 64, None, y.ptr, None, None, 64) == -3       # `error` in a PLL mode
    assert b"PLL modes" in L.csdr_amd_last_error()
    assert L.csdr_amd_carrier_process(o.h, x.ptr, 64, 64, y.ptr, None, None, y.ptr, 64) == -3       # `out` in a PLL mode
    assert L.csdr_amd_carrier_process(o.h, x.ptr, 64, 64, None, None, y.ptr, None, 64) == 0
    ctx.sync()
    o.close()


def test_lifecycle_no_growth(ctx):
    import csdr_amd
    import torch
    x = np.zeros((64, 1024), np.complex64)

    def cycle():
        o = ctx.carrier(csdr_amd.costas_params(0.05, 0.707, True), 64)
        o.process(x, ALL)
        o.close()
    cycle()
    ctx.sync()
    f0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        cycle()
    f1 = torch.cuda.mem_get_info(0)[0]
    assert f1 >= f0 - (4 << 20)
