"""What the tests of the squelched WFM receive bank share (csdr_amd_wfmrx_create_squelched, csdr_amd/csrc/wfmrx.hip): the stream model, the two plan functions
restated, the inputs and their levels.

Stream model, per channel:  squelch_and_smeter_cc | fmdemod_quadri_cf | fractional_decimator_ff | deemphasis_wfm_ff | convert_f_s16.  The squelch cuts the
input into blocks of B samples counted from the reset; whole blocks go on (squelch_model.stream: the library's power order, the gate, the level in force when
the block started), a closed one as zeros, and the chain behind is wfmrx_model.expected on that gated stream: the demodulator's previous sample is the last
gated one, a zero sample demodulates to 0, the de-emphasis decays through closed stretches.

Inputs: wfmrx_model.make_input rows (one kind per channel) with the stretches QUIET scaled to 0.05 of their amplitude, so that at the kind's level some
blocks close and some stay open, with B = 1024 as with B = 300 and 301.  The level is LEVEL for the kinds of amplitude 0.7 and the same rule scaled,
WEAK_LEVEL, for `weak` (amplitude 1e-3); `allzero` never opens at LEVEL.  From 5 channels on channel 4 (an fm channel) is at ALL_CLOSED, from 6 on channel 5
(a zeros channel) at 0: always open, its `den == 0` runs inside open blocks."""
import numpy as np

import squelch_model as sm
import wfmrx_model as wm

c64 = np.complex64
f32 = np.float32

QUIET = ((700, 2300), (4000, 5200), (6100, 6500))
QUIET_SCALE = 0.05
LEVEL = 0.05
WEAK_LEVEL = 1e-7
ALL_CLOSED = 10.0
N = 7 * 1024 + 37                     # B = 1024: 7 squelch blocks go on, 37 samples wait; B = 300: 24 blocks, 5 wait; B = 301: 23 blocks, 282 wait
SHAPES = [(n_ch, B, d) for n_ch in (1, 5, 17) for B in (1024, 300) for d in (1, 3)]     # (channels, squelch block, use_every_nth)
RAGGED = [341, 0, 1, 2053]            # then the rest


def squelch_plan(held, n_in, B):
    """csdr_amd_wfmrx_squelch_plan restated: (gated samples handed to the demodulator, samples held afterwards)"""
    m = (held + n_in) // B * B
    return m, held + n_in - m


def plan(rate, P, taps_length, window, where, held, sq_held, n_in, B):
    """the two plans composed: one call of n_in samples -> (audio samples written, where afterwards, floats held, squelch samples held, squelch blocks
    completed)"""
    m, new_sq = squelch_plan(sq_held, n_in, B)
    n_out, where, held = wm.plan(rate, P, taps_length, window, where, held, m)
    return n_out, where, held, new_sq, m // B


def make_input(n_channels, n=N, seed=0):
    """[n_channels, n] complex64: wfmrx_model.make_input with the QUIET stretches scaled down"""
    x = wm.make_input(n_channels, n, seed).copy()
    for a, b in QUIET:
        x[:, a:min(b, n)] *= f32(QUIET_SCALE)
    return x


def levels(n_channels):
    lv = np.array([WEAK_LEVEL if wm.KINDS[k % len(wm.KINDS)] == "weak" else LEVEL for k in range(n_channels)], f32)
    if n_channels > 4:
        lv[4] = ALL_CLOSED
    if n_channels > 5:
        lv[5] = 0.0
    return lv


def gated(x, B, d, level, changes=None):
    """one channel through the squelch -> (gated stream of the whole blocks, powers, flags); changes: squelch_model.stream's"""
    return sm.stream(x, B, d, level, changes)


def expected(port, x, B, d, level, rate=5, P=12, taps=None, changes=None):
    """the oracle's chain on the model's gated stream of one channel -> (s16, float audio, powers, flags)"""
    g, pw, fl = gated(x, B, d, level, changes)
    s16, af = wm.expected(port, g, rate, P, taps)
    return s16, af, pw, fl


def undecidable_blocks(x, B, d, level):
    """the blocks of one channel whose float64 power is within the float32 gate's reach of the level (none at level 0: always open)"""
    if level == 0:
        return []
    nb = x.size // B
    return [k for k in range(nb) if sm.undecidable(B, d, sm.power64(x[k * B:(k + 1) * B], d), float(level))]


def bank_input(n, seed=77):
    """one FM signal at -0.1 of the wide rate for channels tuned at and beside it (tests/test_wfmrx_gpu.py's): every channel sees a constant envelope"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return (wm.fm_baseband(rng, n, dev=0.02) * np.exp(-2j * np.pi * 0.1 * t)).astype(c64)


def bank_composition(ctx, x, tbw, decimation, rates, per, frac_rate, B, d, levels_between=None):
    """ctx.fastddc_bank -> a squelched WfmRx (every level 0 at the start) with `per` channelizer blocks per call; levels_between {call: [(channel, level), ...]}
    is applied in front of that call -> (the s16 audio of every call [n_channels, count], the powers of every call [n_channels, blocks], the flags likewise,
    the bank's rows, the channelizer's per-call counts)"""
    import csdr_amd
    y = ctx.fastddc_bank(x, tbw, decimation, rates, blocks_per_call=per)
    assert all(np.all(c == c[0]) for c in ctx.ddc_call_counts)
    counts = [int(c[0]) for c in ctx.ddc_call_counts]
    audio, powers, flags, at = [], [], [], 0
    with csdr_amd.WfmRx(ctx, len(rates), rate=frac_rate, max_samples_per_call=max(counts), squelch_block=B, use_every_nth=d) as o:
        for call, k in enumerate(counts):
            for ch, level in (levels_between or {}).get(call, []):
                o.set_squelch_level(ch, level)
            s16, _, pw, fl = o.process_squelched(np.stack([row[at:at + k] for row in y]))
            audio.append(s16); powers.append(pw); flags.append(fl)
            at += k
    return audio, powers, flags, y, counts


def smeter_lines(powers, report_every_nth):
    """what `csdr fastddc_wfm_bank_s16 --squelch` writes to its S-meter output for powers [n_channels, blocks]: one line per channel for every block due"""
    return "".join("%d %g\n" % (ch, powers[ch, k]) for k in sm.report_replay(report_every_nth, powers.shape[1]) for ch in range(powers.shape[0]))


if __name__ == "__main__":
    # python wfmrx_squelch_model.py <in.npz> <out.npz>: bank_composition in a process of its own, without torch, as wfmrx_model.py's __main__ (and for its reason)
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import csdr_amd
    a = np.load(sys.argv[1])
    c = csdr_amd.Context(0)
    args = (c, a["x"], float(a["tbw"]), int(a["decimation"]), [float(r) for r in a["rates"]], int(a["per"]), float(a["frac_rate"]), int(a["B"]), int(a["d"]))
    audio, powers, flags, _, _ = bank_composition(*args, levels_between={1: [(int(a["level_channel"]), float(a["level"]))]})
    plain, _, _, _, _ = bank_composition(*args)
    np.savez(sys.argv[2], first=audio[0], second=audio[1], powers=np.concatenate(powers, axis=1), flags=np.concatenate(flags, axis=1),
             plain=np.concatenate(plain, axis=1), torch_loaded="torch" in sys.modules)
    c.close()
