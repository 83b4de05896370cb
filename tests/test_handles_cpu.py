"""CPU checks of the wrapper's handle base (no library, no GPU): csdr_amd._Handle and the members the eight stateful classes inherit from it, driven
against a fake context whose `L` records every C call by name.  The composed C names are compared with the literal names the classes spelled out before
they shared a base; close() follows one contract in all of them: destroy once while the context is open, no C call once it is closed."""
import numpy as np
import pytest

import csdr_amd

H = 0x5EED


class FakeLib:
    """every attribute is a C entry point that records (name, args) and returns what `returns` holds for it (default 0)"""

    def __init__(self):
        self.calls, self.returns = [], {}

    def __getattr__(self, name):
        if not name.startswith("csdr_amd_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return self.returns.get(name, b"k_fake" if name.endswith("_kernel_name") else 0)
        return fn

    def names(self):
        return [n for n, _ in self.calls]


class FakeCtx:
    """what the classes use of a Context: L, h (None once closed), err() and check()"""

    def __init__(self):
        self.L, self.h = FakeLib(), 0xC0DE
        self.L.csdr_amd_last_error = lambda: b"fake error"
        self.checked = []

    def err(self):
        return "fake error"

    def check(self, rc, what=""):
        self.checked.append(what)
        if rc < 0:
            raise csdr_amd.CsdrAmdError("%s failed (%d)" % (what, rc))
        return rc


def _ctx(pre, h=H):
    c = FakeCtx()
    c.L.returns["csdr_amd_%s_create" % pre] = h
    return c


TAPS = np.ones(8, np.float32)
# class name -> (C prefix, constructor from a context, the inherited members the class has besides reset, force_generic and kernel_name)
CHAN, LANES = ("reset_channel", "get_channel", "set_channel"), ("set_lanes", "lanes")
CLASSES = {
    "Waterfall": ("waterfall", lambda c: csdr_amd.Waterfall(c, 1024, 512, 2, 0.0, "HAMMING", "u8", "db", 2, 4096), ()),
    "Resampler": ("resampler", lambda c: csdr_amd.Resampler(c, 3, 2, TAPS, 2), ("max_out",)),
    "Interpolator": ("interp", lambda c: csdr_amd.Interpolator(c, 4, TAPS, 2), ("max_out",)),
    "Psk31": ("psk31", lambda c: csdr_amd.Psk31(c, None, 2), ("max_out",) + CHAN + LANES),
    "Psk31Tx": ("psk31tx", lambda c: csdr_amd.Psk31Tx(c, 2), ("max_out",) + CHAN),
    "Rtty": ("rtty", lambda c: csdr_amd.Rtty(c, None, 2), ("max_out", "reset_channel")),
    "Squelch": ("squelch", lambda c: csdr_amd.Squelch(c, 2), ("reset_channel",)),
    "Carrier": ("carrier", lambda c: csdr_amd.Carrier(c, csdr_amd.CarrierParams(), 2), CHAN + LANES),
    "TxBank": ("txbank", lambda c: csdr_amd.TxBank(c, 2, "fm", 4, TAPS, [0.1, 0.2]), ("max_out",)),
}
COMMON = ("reset", "force_generic", "kernel_name")
OPTIONAL = ("max_out",) + CHAN + LANES
UNCHECKED = ("kernel_name", "max_out", "lanes")          # these return a value, not a status
STATE = {"psk31": csdr_amd.Psk31Chan, "psk31tx": csdr_amd.Psk31TxChan, "carrier": csdr_amd.CarrierChan}


def _make(name):
    pre, make, extra = CLASSES[name]
    c = _ctx(pre)
    obj = make(c)
    assert c.L.names() == ["csdr_amd_%s_create" % pre] and obj.h == H
    c.L.calls.clear()
    return pre, c, obj, extra


def _invoke(obj, pre, member):
    if member == "get_channel":
        return obj.get_channel(1)
    if member == "set_channel":
        return obj.set_channel(1, STATE[pre]())
    args = {"force_generic": (True,), "max_out": (100,), "reset_channel": (1,), "set_lanes": (4,)}.get(member, ())
    return getattr(obj, member)(*args)


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_inherited_members_compose_the_parents_c_names(name):
    pre, c, obj, extra = _make(name)
    for member in COMMON + extra:
        c.L.calls.clear(); del c.checked[:]
        r = _invoke(obj, pre, member)
        (cname, args), = c.L.calls
        assert cname == "csdr_amd_%s_%s" % (pre, member)          # e.g. csdr_amd_psk31_reset_channel: the literal the class called before
        assert args[0] == H
        assert c.checked == ([] if member in UNCHECKED else ["%s_%s" % (pre, member)])
        if member == "kernel_name":
            assert r == "k_fake"
        if member == "get_channel":
            assert isinstance(r, STATE[pre]) and args[1] == 1
        if member == "force_generic":
            assert args[1:] == (1,)
    obj.close()


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_a_class_exposes_only_the_members_it_had(name):
    _, _, obj, extra = _make(name)
    for member in OPTIONAL:
        assert hasattr(obj, member) == (member in extra), member
    obj.close()


def test_who_has_channel_state_and_lanes():
    for name in ("Rtty", "Squelch", "Waterfall", "Resampler", "Interpolator", "TxBank"):
        cls = getattr(csdr_amd, name)
        assert not hasattr(cls, "get_channel") and not hasattr(cls, "set_channel"), name
    assert sorted(n for n in CLASSES if hasattr(getattr(csdr_amd, n), "set_lanes")) == ["Carrier", "Psk31"]
    assert sorted(n for n in CLASSES if hasattr(getattr(csdr_amd, n), "get_channel")) == ["Carrier", "Psk31", "Psk31Tx"]


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_close_destroys_once(name):
    pre, c, obj, _ = _make(name)
    obj.close()
    assert c.L.calls == [("csdr_amd_%s_destroy" % pre, (H,))] and obj.h is None
    obj.close(); obj.__del__()
    assert len(c.L.calls) == 1


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_close_after_the_context_makes_no_c_call(name):
    """Every *_destroy reads the object's context: after Context.close the handle is dropped without a call (Waterfall and the resamplers called destroy)."""
    pre, c, obj, _ = _make(name)
    c.h = None
    obj.close()
    assert c.L.calls == [] and obj.h is None
    obj.__del__()
    assert c.L.calls == []


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_with_closes_when_the_body_raises(name):
    pre, c, obj, _ = _make(name)
    destroyed_at_raise = []
    try:
        with obj as o:
            assert o is obj
            raise KeyError("body")
    except KeyError:
        destroyed_at_raise = list(c.L.names())
    assert destroyed_at_raise == ["csdr_amd_%s_destroy" % pre] and obj.h is None


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_null_create_raises_and_leaves_nothing_to_close(name, monkeypatch):
    pre, make, _ = CLASSES[name]
    c = _ctx(pre, None)
    made = []
    orig = csdr_amd._Handle.__init__

    def spy(self, *a):
        made.append(self)
        orig(self, *a)
    monkeypatch.setattr(csdr_amd._Handle, "__init__", spy)
    with pytest.raises(csdr_amd.CsdrAmdError, match="fake error"):
        make(c)
    assert c.L.names() == ["csdr_amd_%s_create" % pre]
    (obj,) = made
    assert obj.h is None
    obj.__del__()
    assert c.L.names() == ["csdr_amd_%s_create" % pre]


def test_handle_base():
    c = FakeCtx()
    h = csdr_amd._Handle(c, "wfm", H)
    assert h._call("set_rate", 3, 0.5) == 0
    assert c.L.calls == [("csdr_amd_wfm_set_rate", (H, 3, 0.5))] and c.checked == ["wfm_set_rate"]
    c.L.returns["csdr_amd_wfm_set_rate"] = -3
    with pytest.raises(csdr_amd.CsdrAmdError, match="wfm_set_rate"):
        with h:
            h._call("set_rate", 99, 0.1)
    assert c.L.names()[-1] == "csdr_amd_wfm_destroy" and h.h is None
    with pytest.raises(csdr_amd.CsdrAmdError):
        csdr_amd._Handle(c, "wfm", None)
    assert csdr_amd._Handle.h is None          # (set before any constructor can raise)


def test_an_object_without_a_context_is_always_destroyed(monkeypatch):
    """csdr_amd_fracdec_create takes no context, so there is none whose closing could make its destroy unsafe"""
    L = FakeLib()
    monkeypatch.setattr(csdr_amd, "lib", lambda: L)
    with csdr_amd._Handle(None, "fracdec", H) as d:
        d._fn("set_cli_bufsize")(d.h, 1024)
    assert L.calls == [("csdr_amd_fracdec_set_cli_bufsize", (H, 1024)), ("csdr_amd_fracdec_destroy", (H,))]
    d.close()
    assert len(L.calls) == 2
    L.csdr_amd_last_error = lambda: b"no object"
    with pytest.raises(csdr_amd.CsdrAmdError, match="no object"):
        csdr_amd._Handle(None, "loopback", None)
