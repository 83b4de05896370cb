"""GPU checks of what the per-channel bank objects take from one place in C (csrc/bank.hpp): the channel range check and the d_st + ch arithmetic of
reset_channel / get_channel / set_channel, and the range of set_lanes.  Three channels: the middle one has a neighbour on each side, so a record written
one place too low or too high shows in a neighbour.  65 samples per channel: one whole 64-sample tile and one more."""
import numpy as np
import pytest

import csdr_amd

pytestmark = pytest.mark.gpu

N_CH, N = 3, 65
c64 = np.complex64


@pytest.fixture(scope="module")
def ctx():
    c = csdr_amd.Context(0)
    yield c
    c.close()


def _noise(seed, n=N):
    r = np.random.default_rng(seed)
    return (0.5 * (r.standard_normal((N_CH, n)) + 1j * r.standard_normal((N_CH, n)))).astype(c64)


# class -> (constructor from a context, one process call that moves every channel's state, a valid state that differs from a fresh channel's)
STATEFUL = {
    "Psk31": (lambda c: csdr_amd.Psk31(c, csdr_amd.psk31_params(rate=0.01, decimation=8), N_CH),
              lambda o: o.process(_noise(1)),
              lambda: csdr_amd.Psk31Chan(0.5, 2, 1, 7, 0.1, 0.2, 5)),
    # items are characters; one is the smallest call that moves the state (the last symbol becomes +-1)
    "Psk31Tx": (lambda c: csdr_amd.Psk31Tx(c, N_CH, 2, 4),
                lambda o: o.process(np.array([[ord("e")], [ord("t")], [ord("a")]], np.uint8)),
                lambda: csdr_amd.Psk31TxChan(1, 0.5, -0.5)),
    "Carrier": (lambda c: csdr_amd.Carrier(c, csdr_amd.costas_params(0.02), N_CH),
                lambda o: o.process(_noise(2)),
                lambda: csdr_amd.CarrierChan(0.1, 0.2, 0.3)),
    "AmSsb": (lambda c: csdr_amd.AmSsb(c, csdr_amd.amssb_params("am", block=64), N_CH, max_samples_per_call=1024),
              lambda o: o.process(_noise(3)),
              lambda: csdr_amd.AmSsbChan(0.25, 2.0)),
}
LANES = ("Psk31", "Carrier", "AmSsb")
RTTY = dict(spacing=0.1, filter_length=9, samples_per_bits=4.0, cli_bufsize=64)
# the classes with reset_channel and no state calls: what a channel's state is shows in what the next call writes
RESET_ONLY = {
    "Rtty": (lambda c: csdr_amd.Rtty(c, csdr_amd.rtty_params(**RTTY), N_CH, "bfsk", "bfsk"), lambda o, x: o.process(x)),
    "Squelch": (lambda c: csdr_amd.Squelch(c, N_CH, 16, 1, [0.01] * N_CH, 1024), lambda o, x: o.process(x)[0]),
}


@pytest.mark.parametrize("name", sorted(STATEFUL))
def test_get_channel_returns_what_set_channel_wrote(ctx, name):
    make, _, state = STATEFUL[name]
    with make(ctx) as o:
        fresh = [bytes(o.get_channel(k)) for k in range(N_CH)]
        o.set_channel(1, state())
        assert bytes(o.get_channel(1)) == bytes(state()) != fresh[1]
        assert bytes(o.get_channel(0)) == fresh[0] and bytes(o.get_channel(2)) == fresh[2]


@pytest.mark.parametrize("name", sorted(STATEFUL))
def test_reset_channel_leaves_the_neighbours(ctx, name):
    make, run, _ = STATEFUL[name]
    with make(ctx) as o, make(ctx) as untouched:
        fresh = bytes(untouched.get_channel(1))
        run(o)
        before = [bytes(o.get_channel(k)) for k in range(N_CH)]
        assert all(b != fresh for b in before), "the call should move every channel's state"
        o.reset_channel(1)
        after = [bytes(o.get_channel(k)) for k in range(N_CH)]
        assert after[0] == before[0] and after[2] == before[2]
        assert after[1] == fresh


@pytest.mark.parametrize("name", sorted(RESET_ONLY))
def test_reset_channel_without_state_calls(ctx, name):
    """after reset_channel(1) the next call writes, for channel 1, what a fresh object writes; for channels 0 and 2, what an object that went on writes"""
    make, run = RESET_ONLY[name]
    x = _noise(4, 2 * N)
    with make(ctx) as o, make(ctx) as went_on, make(ctx) as fresh:
        run(o, x[:, :N]); run(went_on, x[:, :N])
        o.reset_channel(1)
        got, on, new = run(o, x[:, N:]), run(went_on, x[:, N:]), run(fresh, x[:, N:])
        for k in (0, 2):
            assert got[k].size and got[k].tobytes() == on[k].tobytes()
        assert got[1].size and got[1].tobytes() == new[1].tobytes()
        assert got[1].tobytes() != on[1].tobytes(), "the channel's state should show in the call"


@pytest.mark.parametrize("name", sorted(STATEFUL) + sorted(RESET_ONLY))
def test_channel_index_out_of_range(ctx, name):
    make = (STATEFUL.get(name) or RESET_ONLY[name])[0]
    with make(ctx) as o:
        for ch in (-1, N_CH):
            with pytest.raises(csdr_amd.CsdrAmdError):
                o.reset_channel(ch)
            if name in STATEFUL:
                with pytest.raises(csdr_amd.CsdrAmdError):
                    o.get_channel(ch)
                with pytest.raises(csdr_amd.CsdrAmdError):
                    o.set_channel(ch, STATEFUL[name][2]())
        o.reset_channel(0); o.reset_channel(N_CH - 1)


@pytest.mark.parametrize("name", LANES)
def test_set_lanes_range(ctx, name):
    with STATEFUL[name][0](ctx) as o:
        for lanes in (64, 5):
            o.set_lanes(lanes)
            assert o.lanes() == lanes
        o.set_lanes(0)
        assert 1 <= o.lanes() <= 64          # automatic: the object's own choice
        o.set_lanes(5)
        for lanes in (-1, 65):
            with pytest.raises(csdr_amd.CsdrAmdError):
                o.set_lanes(lanes)
            assert o.lanes() == 5
