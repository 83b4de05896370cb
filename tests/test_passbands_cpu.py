"""CPU checks of the passband per stream / per SSB channel: every new entry point is declared, exported and bound, and the Python wrapper refuses wrong shapes
before it touches a device."""
import os
import subprocess
import numpy as np
import pytest

from test_abi_cpu import declared_symbols

NEW = ["csdr_amd_fftfilt_create_per_stream", "csdr_amd_fftfilt_set_stream_taps", "csdr_amd_fftfilt_per_stream",
       "csdr_amd_amssb_set_passband", "csdr_amd_amssb_set_channel_taps", "csdr_amd_amssb_get_passband"]
c64 = np.complex64


@pytest.fixture(scope="module")
def libpath():
    import csdr_amd
    if not os.path.exists(csdr_amd.LIB_PATH):
        csdr_amd.build()
    return csdr_amd.LIB_PATH


def test_new_symbols_declared_exported_and_bound(libpath):
    import csdr_amd
    declared = declared_symbols("csdr_amd.h")
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    L = csdr_amd.lib()
    for name in NEW:
        assert name in declared, name + " is not declared in csdr_amd.h"
        assert name in exported, name + " is not exported"
        assert getattr(L, name).argtypes, name + " is not bound"
    assert L.csdr_amd_fftfilt_set_taps.argtypes
    for name in ("set_passband", "get_passband", "set_channel_taps"):
        assert callable(getattr(csdr_amd.AmSsb, name))
    for name in ("set_taps", "set_stream_taps", "per_stream", "process"):
        assert callable(getattr(csdr_amd.FftFilt, name))


@pytest.fixture()
def no_device():
    """a Context that was never opened: any call into the library through it fails with AttributeError"""
    import csdr_amd
    c = object.__new__(csdr_amd.Context)
    c.h = None
    assert not hasattr(c, "L")
    return c


def test_taps_shapes_are_refused_before_the_device(no_device):
    import csdr_amd
    x = np.zeros((5, 4096), c64)
    for taps in (np.ones((4, 63), c64), np.ones((6, 63), c64), np.ones((5, 3, 63), c64), np.ones((5, 0), c64)):
        with pytest.raises(ValueError):
            no_device.bandpass_fir_fft_cc(x, taps, 256)
        with pytest.raises(ValueError):
            csdr_amd.FftFilt(no_device, 256, taps, 5, 1)
    with pytest.raises(AttributeError):                                 # the right shapes go on to the device
        no_device.bandpass_fir_fft_cc(x, np.ones((5, 63), c64), 256)
    with pytest.raises(AttributeError):
        no_device.bandpass_fir_fft_cc(x, np.ones(63, c64), 256)


def test_passband_lists_are_refused_before_the_device(no_device):
    import csdr_amd
    taps = np.ones(79, c64)
    P = csdr_amd.AmSsbParams()
    for bands in ([(0.0, 0.1)] * 3, [(0.0, 0.1)] * 5, [(0.0, 0.1, 0.2)] * 4, [0.0, 0.1, 0.0, 0.1], []):
        with pytest.raises(ValueError):
            csdr_amd.AmSsb(no_device, P, 4, taps=taps, fft_size=512, passbands=bands)
    with pytest.raises(ValueError):
        csdr_amd.AmSsb(no_device, P, 4, passbands=[(0.0, 0.1)] * 3)
    with pytest.raises(AttributeError):                                 # the right length goes on to the device
        csdr_amd.AmSsb(no_device, P, 4, taps=taps, fft_size=512, passbands=[(0.0, 0.1)] * 4)
