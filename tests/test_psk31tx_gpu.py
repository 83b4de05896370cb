"""GPU checks of the BPSK31 transmit chain (psk31tx.hip) through the C ABI against the float32 model (psk31tx_model.py), bit for bit: every stage range,
the fused kernels against the generic one, cut and batch invariance, bounds, other n_psk, the round trip into the receive object, the flat operators,
the CLI commands and `csdr chain` fusion, the drop-in functions, argument errors and lifecycle."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

import psk31_model as pm
import psk31tx_model as tm
import test_psk31tx_cpu as tc
from test_psk31tx_cpu import bits_eq

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libcsdr_ref.so")
CSDR = os.path.join(ROOT, "csdr_amd", "csdr")
FUSED, GENERIC = "k_psk31tx_plan+k_psk31tx_shape", "k_psk31tx_generic"
# every byte 0..255 and some plain text; _text(k, n) takes n bytes from offset 37 k of the wrapped sequence
ALL_BYTES = np.concatenate([np.arange(256, dtype=np.uint8), np.frombuffer(b"The quick brown fox, 0123456789 de MI355X k", np.uint8)])


@pytest.fixture(scope="module")
def ctx():
    import csdr_amd
    c = csdr_amd.Context(0)
    yield c
    c.close()


def _text(k, n):
    return np.resize(np.roll(ALL_BYTES, -37 * k), n).copy()


def _name(first, last, I=16, forced=False):
    return FUSED if (first, last) == (0, 3) and not forced else GENERIC


def _stage_input(first, text, n_psk, I):
    """the items a channel that starts at stage `first` is fed for `text`: the model's output of the stage in front"""
    if first == 0:
        return text
    return tm.run(text.tobytes(), "varicode", tm.STAGES[first - 1], n_psk, I)[0]


def test_every_stage_range_vs_model(ctx):
    n_in, I = 200, 16
    in_counts = [0, 1, 70, 200, 200]
    texts = [np.resize(np.roll(ALL_BYTES, -off), n_in) for off in (0, 37, 74, 0, 100)]
    assert set(np.concatenate([t[:k] for t, k in zip(texts, in_counts)]).tolist()) == set(range(256))      # bytes without a varicode included
    for f in range(4):
        # every channel's items at stage f, cut to exactly n_in of them so that the rows have one length
        rows = []
        for t in texts:
            full = _stage_input(f, np.resize(t, 4 * n_in) if f else t, 2, I)
            assert full.size >= n_in
            rows.append(full[:n_in])
        X = np.stack(rows)
        for l in range(f, 4):
            o = ctx.psk31_tx(5, 2, I, f, l)
            got = o.process(X, in_counts=in_counts)
            assert o.kernel_name() == _name(f, l)
            for c in range(5):
                want, _ = tm.run(X[c, :in_counts[c]].tobytes() if f < 3 else X[c, :in_counts[c]], tm.STAGES[f], tm.STAGES[l], 2, I)
                assert bits_eq(got[c], want), (f, l, c)
            o.close()


@pytest.mark.parametrize("I", [256, 16, 5, 1])
def test_fused_vs_model_and_generic(ctx, I):
    X = np.stack([_text(k, 70) for k in range(3)])
    o = ctx.psk31_tx(3, 2, I)
    got = o.process(X)
    assert o.kernel_name() == FUSED
    g = ctx.psk31_tx(3, 2, I); g.force_generic()
    gen = g.process(X)
    assert g.kernel_name() == GENERIC
    for c in range(3):
        want = tm.chain(X[c].tobytes(), 2, I)["shape"]
        assert bits_eq(got[c], want), c
        assert bits_eq(gen[c], got[c]), c
        sf, sg = o.get_channel(c), g.get_channel(c)
        assert (sf.diff_state, sf.last_i, sf.last_q) == (sg.diff_state, sg.last_i, sg.last_q)
    o.close(); g.close()


@pytest.mark.parametrize("forced", [False, True])
def test_cut_invariance_and_channel_state(ctx, forced):
    import csdr_amd
    I = 16
    text = _text(1, 200)
    cuts = [0, 1, 3, 64]
    cuts.append(text.size - sum(cuts))
    X = np.stack([text, text, text])
    one = ctx.psk31_tx(3, 2, I); one.force_generic(forced)
    whole = one.process(X)
    assert one.kernel_name() == _name(0, 3, forced=forced)
    o = ctx.psk31_tx(3, 2, I); o.force_generic(forced)
    parts, at, state = [], 0, (0, 0j)
    for k in cuts:
        parts.append(o.process(X[:, at:at + k])[1])
        _, state = tm.run(text[at:at + k].tobytes(), "varicode", "shape", 2, I, state)
        st = o.get_channel(1)
        assert st.diff_state == state[0] and bits_eq(np.array([complex(st.last_i, st.last_q)], np.complex64), np.array([state[1]], np.complex64)), k
        at += k
    assert bits_eq(np.concatenate(parts), whole[1])
    assert bits_eq(whole[1], tm.chain(text.tobytes(), 2, I)["shape"])
    # set_channel and reset_channel on channel 1 leave channels 0 and 2 as they are
    before = [o.get_channel(c) for c in (0, 2)]
    o.set_channel(1, csdr_amd.Psk31TxChan(1, 0.5, -0.25))
    st = o.get_channel(1)
    assert (st.diff_state, st.last_i, st.last_q) == (1, 0.5, -0.25)
    nxt = o.process(np.stack([text[:9]] * 3))
    assert bits_eq(nxt[1], tm.run(text[:9].tobytes(), "varicode", "shape", 2, I, (1, complex(0.5, -0.25)))[0])
    assert bits_eq(nxt[0], tm.run(text[:9].tobytes(), "varicode", "shape", 2, I, (before[0].diff_state, complex(before[0].last_i, before[0].last_q)))[0])
    assert bits_eq(nxt[2], nxt[0])
    o.reset_channel(1)
    st = o.get_channel(1)
    assert (st.diff_state, st.last_i, st.last_q) == (0, 0.0, 0.0)
    again = o.process(np.stack([text[:9]] * 3))
    assert bits_eq(again[1], tm.chain(text[:9].tobytes(), 2, I)["shape"]) and not bits_eq(again[0], again[1])
    one.close(); o.close()


@pytest.mark.parametrize("forced", [False, True])
def test_batch_invariance(ctx, forced):
    I, n = 5, 40
    same = (0, 31, 63, 64, 66)
    X = np.stack([_text(3 if k in same else k, n) for k in range(67)])
    o = ctx.psk31_tx(67, 2, I); o.force_generic(forced)
    got = o.process(X)
    assert o.kernel_name() == _name(0, 3, forced=forced)
    want = tm.chain(X[0].tobytes(), 2, I)["shape"]
    for k in same:
        assert bits_eq(got[k], want), k
    assert bits_eq(got[65], tm.chain(X[65].tobytes(), 2, I)["shape"])
    o.close()


@pytest.mark.parametrize("I", [16, 5, 1])
@pytest.mark.parametrize("forced", [False, True])
def test_nothing_written_beyond_counts(ctx, forced, I):
    n_in = 70
    in_counts = np.array([0, 1, 70, 33], np.int32)
    X = np.stack([_text(k, n_in) for k in range(4)])
    o = ctx.psk31_tx(4, 2, I); o.force_generic(forced)
    pitch = o.max_out(n_in) + 3
    canary = np.full(4 * pitch, np.float32(-123.25)).astype(np.float32)
    can = np.empty(4 * pitch, np.complex64); can.real = canary; can.imag = canary
    di, dn, do, dc = ctx.upload(X), ctx.upload(in_counts), ctx.upload(can), ctx.alloc(64)
    o.process_dev(di.ptr, n_in, dn.ptr, n_in, do.ptr, pitch, dc.ptr)
    assert o.kernel_name() == _name(0, 3, forced=forced)
    cnt = ctx.download(dc, np.int32, 4)
    y = ctx.download(do, np.complex64, 4 * pitch).reshape(4, pitch)
    for c in range(4):
        want = tm.chain(X[c, :in_counts[c]].tobytes(), 2, I)["shape"]
        assert cnt[c] == want.size and bits_eq(y[c, :cnt[c]], want), c
        assert bits_eq(y[c, cnt[c]:], can[:pitch - cnt[c]]), c
    o.close()


def test_argument_errors(ctx):
    import csdr_amd
    for bad in [dict(n_psk=0), dict(n_psk=257), dict(interpolation=0), dict(first="shape", last="mod"), dict(n_channels=0)]:
        with pytest.raises(csdr_amd.CsdrAmdError):
            ctx.psk31_tx(**bad)
    o = ctx.psk31_tx(2, 2, 16)
    X = np.stack([_text(0, 10)] * 2)
    di, do, dc = ctx.upload(X), ctx.alloc(8 * 2 * o.max_out(10)), ctx.alloc(64)
    with pytest.raises(csdr_amd.CsdrAmdError):
        o.process_dev(di.ptr, 10, None, 10, do.ptr, o.max_out(10) - 1, dc.ptr)       # out_pitch below max_out
    with pytest.raises(csdr_amd.CsdrAmdError):
        o.process_dev(di.ptr, 10, None, 9, do.ptr, o.max_out(10), dc.ptr)            # in_pitch below n_in
    with pytest.raises(csdr_amd.CsdrAmdError):
        o.process(X, in_counts=[10, 11])                                             # a count above n_in, checked on the host
    with pytest.raises(csdr_amd.CsdrAmdError):
        o.process(X, in_counts=[-1, 3])
    assert o.kernel_name() == ""                                                     # nothing was launched
    with pytest.raises(csdr_amd.CsdrAmdError):
        o.reset_channel(2)
    with pytest.raises(csdr_amd.CsdrAmdError):
        o.set_channel(0, csdr_amd.Psk31TxChan(2, 0.0, 0.0))
    assert o.max_out(10) == 10 * 12 * 16 and ctx.psk31_tx(1, 2, 16, "diff", "mod").max_out(10) == 10
    o.close()


@pytest.mark.parametrize("n_psk", [4, 8])
def test_other_n_psk(ctx, n_psk):
    I = 16
    rng = np.random.default_rng(n_psk)
    idx = rng.integers(0, 256, (2, 150)).astype(np.uint8)
    idx[0, :n_psk] = np.arange(n_psk)
    o = ctx.psk31_tx(2, n_psk, I, "mod", "shape")
    got = o.process(idx)
    assert o.kernel_name() == GENERIC
    for c in range(2):
        assert bits_eq(got[c], tm.run(idx[c], "mod", "shape", n_psk, I)[0]), c
    o.close()


def test_round_trip_on_the_device(ctx):
    import csdr_amd
    import torch
    I, n_ch = 256, 8
    base = np.arange(1, 128, dtype=np.uint8)
    texts = [np.concatenate([np.roll(base, -c), np.frombuffer(b"Hello", np.uint8)]) for c in range(n_ch)]
    X = np.stack(texts)
    n_in = X.shape[1]
    tx = ctx.psk31_tx(n_ch, 2, I)
    pitch = tx.max_out(n_in)
    d_out = torch.zeros((n_ch, pitch, 2), dtype=torch.float32, device="cuda")
    d_cnt = torch.zeros(n_ch, dtype=torch.int32, device="cuda")
    di = ctx.upload(X)
    torch.cuda.synchronize()
    tx.process_dev(di.ptr, n_in, None, n_in, d_out.data_ptr(), pitch, d_cnt.data_ptr())
    assert tx.kernel_name() == FUSED
    ctx.sync()
    cnt = d_cnt.cpu().numpy()
    # (the texts are rotations of one another, so every channel has the same number of bits)
    n_bits = tm.varicode_encode(texts[0].tobytes()).size
    assert np.array_equal(cnt, np.full(n_ch, n_bits * I))
    sym = d_out[:, I - 1::I, :].contiguous()                       # every I-th sample from offset I - 1: the symbols themselves
    n_sym = sym.shape[1]
    assert n_sym >= n_bits
    rx = ctx.psk31(csdr_amd.psk31_params(), n_ch, "dbpsk", "varicode")
    d_txt = torch.zeros((n_ch, n_sym + 16), dtype=torch.uint8, device="cuda")
    d_rc = torch.zeros(n_ch, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rx.process_dev(sym.data_ptr(), n_bits, n_sym, d_txt.data_ptr(), n_sym + 16, d_rc.data_ptr())
    assert rx.kernel_name() == "k_psk31"
    ctx.sync()
    rc = d_rc.cpu().numpy(); txt = d_txt.cpu().numpy()
    for c in range(n_ch):
        assert txt[c, :rc[c]].tobytes() == texts[c].tobytes(), c
    tx.close(); rx.close()


def test_full_receive_chain_on_transmit_output(ctx):
    """the whole receive object (AGC .. VARICODE, D = I = 16) on the transmit object's output gives what the receive model gives on the model's signal
    (the reference's loop does not return the sent text from a noiseless shaped signal; that is its behaviour, and is not asserted)"""
    import csdr_amd
    I = 16
    text = b"Hello, World! 0123 ~{}" * 3
    tx = ctx.psk31_tx(1, 2, I)
    sig = tx.process(text)
    assert tx.kernel_name() == FUSED
    model_sig = tm.chain(text, 2, I)["shape"]
    assert bits_eq(sig, model_sig)
    P = csdr_amd.psk31_params(decimation=I)
    want = pm.chain(model_sig, decimation=I)
    bits = ctx.psk31(P, 1, "agc", "dbpsk").process(sig)
    got = ctx.psk31(P, 1, "agc", "varicode").process(sig)
    assert np.array_equal(bits, want["bits"]) and got.tobytes() == want["text"]
    tx.close()


def test_flat_operators(ctx):
    rng = np.random.default_rng(9)
    x = rng.integers(0, 3, (3, 100)).astype(np.uint8)
    a, st = ctx.differential_decoder_u8_u8(x[:, :37], state=[0, 1, 2])
    b, st2 = ctx.differential_decoder_u8_u8(x[:, 37:], state=st)
    for c, s0 in enumerate([0, 1, 2]):
        want, ws = tm.differential_decode(x[c], s0)
        assert np.array_equal(np.concatenate([a[c], b[c]]), want) and st2[c] == ws and st[c] == x[c, 36]
    y = rng.integers(0, 256, (2, 120)).astype(np.uint8)
    for ss in (1, 3, 8):
        for nt in (1, 5):
            got = ctx.duplicate_samples_ntimes_u8_u8(y, ss, nt)
            for c in range(2):
                assert np.array_equal(got[c], tm.duplicate_samples(y[c], ss, nt)), (ss, nt, c)
    z = ctx.duplicate_samples_ntimes_u8_u8(y[0, :10], 4, 2)          # a partial last sample is left out
    assert np.array_equal(z, tm.duplicate_samples(y[0, :10], 4, 2)) and z.size == 16


def _run(cmd, data, shell=False, timeout=120):
    r = subprocess.run(cmd, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, shell=shell)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout, r.stderr.decode()


def test_cli_commands_and_chain(ctx):
    text = np.resize(_text(2, 256), 300).tobytes()
    m = tm.chain(text, 2, 256)
    want = m["shape"].tobytes()
    pipe = "%s psk31_varicode_encoder_u8_u8 | %s differential_encoder_u8_u8 | %s psk_modulator_u8_c 2 | %s psk31_interpolate_sine_cc 256" % ((CSDR,) * 4)
    out, _ = _run(pipe, text, shell=True)
    assert out == want
    out, err = _run([CSDR, "chain", "psk31_varicode_encoder_u8_u8 | differential_encoder_u8_u8 | psk_modulator_u8_c 2 | psk31_interpolate_sine_cc 256"], text)
    assert out == want
    assert "fused BPSK31 transmit object" in err
    out, _ = _run([CSDR, "differential_decoder_u8_u8"], m["diff"].tobytes())
    assert out == tm.differential_decode(m["diff"])[0].tobytes()
    out, _ = _run([CSDR, "duplicate_samples_ntimes_u8_u8", "3", "5"], text)
    assert out == tm.duplicate_samples(np.frombuffer(text, np.uint8), 3, 5).tobytes()


@pytest.mark.parametrize("args,message", [
    (["psk_modulator_u8_c"], b"need required parameter (n_psk)"),
    (["psk_modulator_u8_c", "0"], b"n_psk should be between 1 and 256"),
    (["psk_modulator_u8_c", "257"], b"n_psk should be between 1 and 256"),
    (["psk31_interpolate_sine_cc"], b"need required parameter (interpolation)"),
    (["psk31_interpolate_sine_cc", "0"], b"interpolation should be >0"),
    (["duplicate_samples_ntimes_u8_u8"], b"need required parameter (sample_size_bytes)"),
    (["duplicate_samples_ntimes_u8_u8", "0"], b"sample_size_bytes should be >0"),
    (["duplicate_samples_ntimes_u8_u8", "2"], b"need required parameter (ntimes)"),
    (["duplicate_samples_ntimes_u8_u8", "2", "0"], b"ntimes should be >0"),
    (["chain", "psk31_varicode_encoder_u8_u8 | differential_encoder_u8_u8 | psk_modulator_u8_c 300"], b"n_psk should be between 1 and 256"),
])
def test_cli_bad_syntax(ctx, args, message):
    # (psk31_varicode_encoder_u8_u8, differential_encoder_u8_u8 and differential_decoder_u8_u8 take no arguments: nothing to get wrong)
    r = subprocess.run([CSDR] + args, input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode != 0 and message in r.stderr and r.stdout == b""


def test_dropin_functions(ctx):
    import csdr_amd
    A = tc.bind_tx(C.CDLL(csdr_amd.lib()._name))
    text = _text(4, 120).tobytes()
    m = tm.chain(text, 2, 16)
    bits, done = tc.ref_varicode(A, text)
    assert done == len(text) and bits_eq(bits, m["varicode"])
    # room for 2.5 characters: "ab" is 6 + 9 bits, "c" needs 8 more
    got, done = tc.ref_varicode(A, b"abc", room=6 + 9 + 4)
    assert done == 2 and bits_eq(got, tm.varicode_encode(b"ab"))
    got, done = tc.ref_varicode(A, b"\x80\xffa", room=5)          # bytes without a code are consumed, "a" (6 bits) does not fit
    assert done == 2 and got.size == 0
    h = bits.size // 2
    a, st = tc.ref_codec(A, bits[:h], 1, 0)
    b, st2 = tc.ref_codec(A, bits[h:], 1, st)
    assert bits_eq(np.concatenate([a, b]), m["diff"]) and st2 == m["diff"][-1]
    a, st = tc.ref_codec(A, np.array([1, 1, 0, 1], np.uint8), 1, 7)      # a state above 1 stays until the first toggle
    assert a.tolist() == [7, 7, 0, 0] and st == 0
    d, st = tc.ref_codec(A, m["diff"], 0, 0)
    assert bits_eq(d, tm.differential_decode(m["diff"])[0]) and st == m["diff"][-1]
    assert bits_eq(tc.ref_modulate(A, m["diff"], 2), m["mod"])
    assert bits_eq(tc.ref_modulate(A, np.arange(256), 8), tm.symbol_table(8))
    y = np.frombuffer(text, np.uint8)
    assert np.array_equal(tc.ref_duplicate(A, y[:119], 7, 3), tm.duplicate_samples(y[:119], 7, 3))
    k = m["mod"].size // 3
    s1, last = tc.ref_shape(A, m["mod"][:k], 16)
    assert bits_eq(np.array([last]), m["mod"][k - 1:k])              # the returned last_input
    s2, last = tc.ref_shape(A, m["mod"][k:], 16, last)
    assert bits_eq(np.concatenate([s1, s2]), m["shape"]) and bits_eq(np.array([last]), m["mod"][-1:])


def test_lifecycle_no_growth(ctx):
    import torch
    X = np.stack([_text(k, 64) for k in range(64)])
    def cycle():
        o = ctx.psk31_tx(64, 2, 16)
        o.process(X)
        o.close()
    cycle()
    ctx.sync()
    f0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(50):
        cycle()
    f1 = torch.cuda.mem_get_info(0)[0]
    assert f1 >= f0 - (4 << 20)


def test_fused_vs_reference(ctx):
    if not os.path.exists(REF_LIB):
        pytest.skip("reference library not built")
    L = tc.bind_tx(C.CDLL(REF_LIB))
    X = np.stack([_text(k, 70) for k in range(3)])
    o = ctx.psk31_tx(3, 2, 256)
    got = o.process(X)
    assert o.kernel_name() == FUSED
    for c in range(3):
        bits, _ = tc.ref_varicode(L, X[c].tobytes())
        st, _ = tc.ref_codec(L, bits, 1)
        want, _ = tc.ref_shape(L, tc.ref_modulate(L, st, 2), 256)
        assert bits_eq(got[c], want), c
    o.close()
