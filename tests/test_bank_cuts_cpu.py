"""CPU check of the one loop that cuts a debug walk's stream into calls (csrc/bank.hpp: for_each_call), through each of the six csdr_amd_debug_*_walk
functions that use it: the same short input in one call and cut as [0, -5, 3, 10**9, 2] gives the same output bits and the same final state.  A negative
cut counts as 0, a cut beyond the end takes what is left, and the cuts behind it (and the rest) are calls of no items.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import csdr_amd

CUTS = [0, -5, 3, 10**9, 2]
N_SYMBOLS = 37                   # the walks that take symbols or characters
N_SAMPLES = 3 * 64 + 5           # the sample-rate walks: with whole calls of 64 a cut would fall on a tile's edge, the cut at 3 falls inside the first tile


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def _state(st):
    return None if st is None else bytes(st)


def _noise(seed, n):
    r = np.random.default_rng(seed)
    return (0.5 * (r.standard_normal(n) + 1j * r.standard_normal(n))).astype(np.complex64)


def _psk31(first, last):
    P = csdr_amd.psk31_params(rate=0.01, decimation=8)
    x = np.random.default_rng(31).integers(0, 2, N_SAMPLES).astype(np.uint8) if first == "varicode" else _noise(31, N_SAMPLES)

    def run(cuts):
        st = csdr_amd.Psk31Chan(gain=1.0)
        out = csdr_amd.psk31_debug_walk(P, first, last, x, cuts, st, with_extras=last == "timing")
        return out if isinstance(out, tuple) else (out,), st
    return run


def _psk31tx(first, last):
    x = _noise(32, N_SYMBOLS) if first == "shape" else np.random.default_rng(32).integers(0, 2 if first != "varicode" else 128, N_SYMBOLS).astype(np.uint8)

    def run(cuts):
        st = csdr_amd.Psk31TxChan()
        return (csdr_amd.psk31tx_debug_walk(x, 2, 5, first, last, cuts, st),), st
    return run


def _pulsetx(first, last):
    taps = csdr_amd.firdes_rrc_f(13, 3, 0.35)
    x = _noise(33, N_SYMBOLS) if first == "shape" else np.random.default_rng(33).integers(0, 4, N_SYMBOLS).astype(np.uint8)
    return lambda cuts: ((csdr_amd.pulsetx_debug_walk(x, taps, 4, 3, first, last, cuts),), None)


def _rtty(first, last):
    P = csdr_amd.rtty_params(spacing=0.1, filter_length=9, samples_per_bits=4.0, cli_bufsize=64)
    x = _noise(34, N_SAMPLES)
    if first == "serial":
        x = x.real.astype(np.float32)
    return lambda cuts: ((csdr_amd.rtty_debug_walk(P, first, last, x, cuts),), None)


def _carrier(mode):
    P = csdr_amd.costas_params(0.02) if mode == "costas" else csdr_amd.pll_params("PI")
    outputs = csdr_amd.CARRIER_OUTPUTS if mode == "costas" else ("dphase", "nco")
    x = _noise(35, N_SAMPLES)

    def run(cuts):
        st = csdr_amd.CarrierChan(0.25, 0.01, 0.0)
        res = csdr_amd.carrier_debug_walk(P, x, outputs, cuts, st)
        return tuple(res[k] for k in outputs), st
    return run


def _fmmod():
    x = np.random.default_rng(36).uniform(-1, 1, N_SAMPLES).astype(np.float32)

    def run(cuts):
        ph, last, out = csdr_amd.fmmod_debug_walk(x, cuts, 0.125, want_out=True)
        return (ph, out), C.c_float(last)
    return run


WALKS = {
    "psk31 agc..varicode": lambda: _psk31("agc", "varicode"),
    "psk31 agc..timing": lambda: _psk31("agc", "timing"),
    "psk31 varicode": lambda: _psk31("varicode", "varicode"),
    "psk31tx varicode..shape": lambda: _psk31tx("varicode", "shape"),
    "psk31tx shape": lambda: _psk31tx("shape", "shape"),
    "pulsetx mod..shape": lambda: _pulsetx("mod", "shape"),
    "pulsetx shape": lambda: _pulsetx("shape", "shape"),
    "rtty bfsk": lambda: _rtty("bfsk", "bfsk"),
    "rtty bfsk..serial": lambda: _rtty("bfsk", "serial"),
    "rtty serial..baudot": lambda: _rtty("serial", "baudot"),
    "carrier costas": lambda: _carrier("costas"),
    "carrier pll": lambda: _carrier("pll"),
    "fmmod": _fmmod,
}


@pytest.mark.parametrize("name", sorted(WALKS))
def test_cut_into_calls_gives_the_bits_of_one_call(name):
    run = WALKS[name]()
    one, st_one = run(())
    cut, st_cut = run(CUTS)
    assert sum(o.size for o in one) > 0, "the input should produce output"
    assert len(one) == len(cut)
    for a, b in zip(one, cut):
        assert a.dtype == b.dtype and a.shape == b.shape and _bits(a) == _bits(b)
    assert _state(st_one) == _state(st_cut)


def test_the_walks_change_their_state():
    """(so that equal final states above say something)"""
    for name in ("psk31 agc..varicode", "psk31tx varicode..shape", "carrier costas", "fmmod"):
        _, st = WALKS[name]()(())
        fresh = {"psk31": csdr_amd.Psk31Chan(gain=1.0), "psk31tx": csdr_amd.Psk31TxChan(), "carrier": csdr_amd.CarrierChan(0.25, 0.01, 0.0),
                 "fmmod": C.c_float(0.125)}[name.split()[0]]
        assert _state(st) != bytes(fresh), name
