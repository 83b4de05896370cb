"""CPU checks of the AM / SSB receive chain's tail: the library's host run of the kernels' functions (csdr_amd_debug_amssb_walk) against the oracle and the
compiled reference, never across agc_ff on unequal inputs; the hook's invariance to how a stream is cut; the parameter struct."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

import amssb_model as mm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
f32 = np.float32

SHAPES = [(256, 9), (1001, 5), (64, 7)]                                     # (block, blocks)


def _params(mode, block, agc):
    import csdr_amd
    return csdr_amd.amssb_params(mode, block, agc)


def _check_pre_agc(lib, mode, x, block, pre, what):
    """pre_agc of the hook against lib's stages: SSB to the bit; AM within GATE_AM of the envelope's RMS (the DC block subtracts a level, the absolute error
    stays), float64 arbitrating.  Returns the three figures (hook against lib, hook against float64, lib against float64) for AM."""
    want = mm.oracle_pre_agc(lib, mode, x, block)
    if mode == "ssb":
        mm.assert_bits(pre, want, what)
        return None
    nf = mm.finite_blocks(x, block) * block
    assert np.array_equal(np.isfinite(pre), np.isfinite(want)), what + ": Inf / NaN in other places than the oracle"
    assert not np.isfinite(pre[nf:]).any() or nf == pre.size
    if nf == 0:
        return None
    y64, env = mm.f64_pre_agc_am(x[:nf], block)
    e = (mm.relrms_to(pre[:nf], want[:nf], env), mm.relrms_to(pre[:nf], y64, env), mm.relrms_to(want[:nf], y64, env))
    print("%s: hook against oracle %.3g, hook against float64 %.3g, oracle against float64 %.3g (of the envelope's RMS)" % ((what,) + e))
    assert e[0] <= mm.GATE_AM and e[1] <= mm.GATE_AM, "%s: %r" % (what, e)
    return e


@pytest.mark.parametrize("mode", ["am", "ssb"])
@pytest.mark.parametrize("agc", sorted(mm.AGC_SETS))
@pytest.mark.parametrize("kind", mm.INPUT_KINDS)
def test_hook_vs_oracle(port, mode, agc, kind):
    import csdr_amd
    for si, (block, nb) in enumerate(SHAPES):
        what = "%s %s %s block %d" % (mode, agc, kind, block)
        x = mm.complex_input(mode, kind, nb * block, block, 100 * si + mm.INPUT_KINDS.index(kind))
        P = _params(mode, block, mm.AGC_SETS[agc])
        st = csdr_amd.AmSsbChan(0.0, 1.0)
        s16, pre = csdr_amd.amssb_debug_walk(P, x, st)
        _check_pre_agc(port, mode, x, block, pre, what)
        # from agc_ff on: the oracle on the hook's own pre_agc, the same input on both sides
        want, g = mm.oracle_tail(port, pre, block, mm.AGC_SETS[agc])
        mm.assert_bits(s16, want, what + ": s16")
        assert mm.bits(f32(st.last_gain)) == mm.bits(f32(g)), what + ": last_gain"


@pytest.mark.parametrize("mode", ["am", "ssb"])
def test_hook_vs_reference(ref, mode):
    """pre_agc against the compiled reference on the finite inputs.  (Its agc_ff is a -ffast-math build whose products round otherwise in places; the stages
    from agc_ff on are held to the oracle's bits in test_hook_vs_oracle, as tests/test_audio_blocks_gpu.py holds agc_ff.)"""
    import csdr_amd
    block, nb = 1024, 6
    for kind in mm.INPUT_KINDS[:-1]:
        for agc in sorted(mm.AGC_SETS):
            what = "reference %s %s %s" % (mode, agc, kind)
            x = mm.complex_input(mode, kind, nb * block, block, 7 + mm.INPUT_KINDS.index(kind))
            s16, pre = csdr_amd.amssb_debug_walk(_params(mode, block, mm.AGC_SETS[agc]), x)
            _check_pre_agc(ref, mode, x, block, pre, what)


def test_agc_branches_are_taken(port):
    """the inputs do reach attack, attack wait, hang, decay, the max_gain clamp and the v == 0 branch (a float32 restatement of agc_ff that counts them)"""
    import csdr_amd
    block, nb = 256, 9
    seen = set()
    for kind in mm.INPUT_KINDS[:-1]:
        for agc in mm.AGC_SETS.values():
            x = mm.complex_input("ssb", kind, nb * block, block, mm.INPUT_KINDS.index(kind))
            _, pre = csdr_amd.amssb_debug_walk(_params("ssb", block, agc), x)
            hang_time, ref_, att, dec, mx, wait, alpha = agc[0], f32(agc[1]), f32(agc[2]), f32(agc[3]), f32(agc[4]), agc[5], f32(agc[6])
            last_gain = f32(1)
            for b in range(nb):
                v = pre[b * block:(b + 1) * block]
                hang = aw = 0; gain = last_gain; last_peak = ref_ / last_gain
                for k in range(1, block):
                    av = abs(v[k])
                    with np.errstate(divide="ignore"):
                        error = ref_ / av - gain
                    if v[k] != 0:
                        if error < 0:
                            if last_peak < av:
                                aw = wait; last_peak = av
                            if aw > 0:
                                aw -= 1; dg = f32(0); seen.add("attack_wait")
                            else:
                                dg = error * att; hang = hang_time; seen.add("attack")
                        else:
                            if hang > 0:
                                hang -= 1; dg = f32(0); seen.add("hang")
                            else:
                                dg = error * dec; seen.add("decay")
                        gain = gain + dg
                    else:
                        seen.add("zero")
                    if gain > mx:
                        gain = mx; seen.add("max_gain")
                    if gain < 0:
                        gain = f32(0)
                    gain = gain + last_gain - alpha * last_gain
                    last_gain = gain
    assert seen >= {"attack", "attack_wait", "hang", "decay", "max_gain", "zero"}, seen


@pytest.mark.parametrize("mode", ["am", "ssb"])
def test_hook_cut_invariance(mode):
    """one call of 7 blocks equals calls of 3, 1 and 3 blocks with the state carried"""
    import csdr_amd
    for block in (64, 1001):
        x = mm.complex_input(mode, "steps_zero_runs", 7 * block, block, 5)
        P = _params(mode, block, mm.AGC_ALT)
        st = csdr_amd.AmSsbChan(0.25, 3.0)
        s16, pre = csdr_amd.amssb_debug_walk(P, x, st)
        st2 = csdr_amd.AmSsbChan(0.25, 3.0)
        parts = [csdr_amd.amssb_debug_walk(P, x[a * block:b * block], st2) for a, b in ((0, 3), (3, 4), (4, 7))]
        mm.assert_bits(np.concatenate([p[0] for p in parts]), s16, "s16 in cuts")
        mm.assert_bits(np.concatenate([p[1] for p in parts]), pre, "pre_agc in cuts")
        assert mm.bits(f32(st.last_dc)) == mm.bits(f32(st2.last_dc)) and mm.bits(f32(st.last_gain)) == mm.bits(f32(st2.last_gain))
        if mode == "am":
            assert st.last_dc != 0.25
        # a fresh channel starts as the CLI does (csdr.c:957, 1365)
        mm.assert_bits(csdr_amd.amssb_debug_walk(P, x)[0], csdr_amd.amssb_debug_walk(P, x, csdr_amd.AmSsbChan(0.0, 1.0))[0], "fresh state")


def test_params_abi(tmp_path):
    """csdr_amd_amssb_params: layout against the header, params_default against csdr.c:1342-1361"""
    import csdr_amd
    src = tmp_path / "t.c"
    names = [n for n, _ in csdr_amd.AmSsbParams._fields_]
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"csdr_amd.h\"\nint main(void){printf(\"%zu %zu\", sizeof(csdr_amd_amssb_params), "
                   "sizeof(csdr_amd_amssb_chan));\n" + "".join("printf(\" %%zu\", offsetof(csdr_amd_amssb_params, %s));\n" % n for n in names) + "return 0;}\n")
    exe = str(tmp_path / "t")
    subprocess.run(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(csdr_amd.AmSsbParams), C.sizeof(csdr_amd.AmSsbChan)] + [getattr(csdr_amd.AmSsbParams, n).offset for n in names]
    assert out[:2] == [36, 8]
    for mode, code in (("am", 0), ("ssb", 1)):
        p = csdr_amd.amssb_params(mode)
        assert (p.mode, p.block, p.hang_time, p.attack_wait_time) == (code, 1024, 200, 0)
        assert (p.reference, p.attack_rate, p.decay_rate, p.max_gain, p.gain_filter_alpha, p.limit_max) == \
               (f32(0.2), f32(0.01), f32(0.0001), 65536.0, f32(0.999), 1.0)
    L = csdr_amd.lib()
    bad = csdr_amd.AmSsbParams()
    assert L.csdr_amd_amssb_params_default(C.byref(bad), 2) < 0
    for field, v in (("block", 1), ("block", 16385), ("mode", 7)):
        p = csdr_amd.amssb_params("am"); setattr(p, field, v)
        assert L.csdr_amd_debug_amssb_walk(C.byref(p), None, 0, None, None, None) < 0
