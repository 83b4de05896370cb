"""What the tests of the gated AM / SSB receive bank share (csdr_amd_amssb_enable_squelch, csdr_amd/csrc/amssb.hip): the stream model, the three ways a block
can take through the tail, agc_ff's zero-sample map in numpy float32, the inputs and their levels.

Stream model, per channel:  squelch_and_smeter_cc | amdemod_cf | fastdcblock_ff | agc_ff | limit_ff | convert_f_s16  (realpart_cf in SSB).  The squelch block is
the tail's block B, counted from the reset: squelch_model.stream with the library's power order (power32), the gate and the level in force when the block
started; a closed block goes on as zeros and the tail behind is csdr_amd_debug_amssb_walk on that gated stream.

The three ways of a block: "open" (the tail as without a squelch), "ramp" (AM only: closed while fastdcblock_ff's last_dc is not +-0, the pre-AGC samples are
the ramp from -last_dc to 0 and agc_ff walks them) and "zero" (closed with last_dc +-0, in SSB every closed block: pre-AGC +0, s16 0, and agc_ff moves its gain
by z B - 1 times).

Inputs: a carrier with a tone (AM) or a tone beside an unrelated imaginary part (SSB), whole blocks scaled by QUIET_SCALE after PATTERN, which is shifted from
channel to channel: runs of open, closed, closed, open blocks, so that in AM every closing happens with last_dc != 0 and is followed by zero blocks."""
import numpy as np

import squelch_model as sm

f32, c64 = np.float32, np.complex64

LEVEL = 0.01                          # between the loud blocks' power (about 0.3 in AM, 0.2 in SSB) and the quiet ones' (times QUIET_SCALE^2)
ALL_CLOSED = 10.0
QUIET_SCALE = 0.02
PATTERN = (1, 0, 0, 1, 1, 0, 0, 0, 1, 0, 1, 1)          # 1: loud


def z(alpha, max_gain, g):
    """agc_ff's step on a zero sample as a map of the gain (amssb_agc_zero_step), every operation rounded to float32"""
    with np.errstate(all="ignore"):
        g, alpha, max_gain = f32(g), f32(alpha), f32(max_gain)
        g2 = max_gain if g > max_gain else g
        g2 = f32(0) if g2 < 0 else g2
        return f32(f32(g2 + g) - f32(alpha * g))


def iterate(alpha, max_gain, g, n):
    """z applied n times, one by one"""
    g = f32(g)
    for _ in range(n):
        g = z(alpha, max_gain, g)
    return g


def loud_pattern(ch, nb):
    return np.array([PATTERN[(k + 5 * ch) % len(PATTERN)] for k in range(nb)], bool)


def make_input(mode, n_ch, nb, B, seed=0, extra=0, quiet=True):
    """[n_ch, nb B + extra] complex64; quiet=False: every block loud"""
    n = nb * B + extra
    t = np.arange(n)
    x = np.empty((n_ch, n), c64)
    for ch in range(n_ch):
        rng = np.random.default_rng(1000 * seed + ch)
        if mode == "am":
            v = (0.5 + 0.3 * np.sin(2 * np.pi * t / (37.0 + ch))) * np.exp(2j * np.pi * (0.013 * t + rng.uniform()))
            v = v + 0.01 * (rng.normal(size=n) + 1j * rng.normal(size=n))
        else:
            v = 0.5 * np.sin(2 * np.pi * t / (29.0 + ch) + rng.uniform()) + 0.2 + 1j * rng.uniform(-0.5, 0.5, n)
        scale = np.where(loud_pattern(ch, nb + (1 if extra else 0)) | (not quiet), 1.0, QUIET_SCALE)
        x[ch] = (v * np.repeat(scale, B)[:n]).astype(c64)
    return x


def levels(n_ch):
    """LEVEL; channel 1 always open, channel 2 always closed"""
    lv = np.full(n_ch, LEVEL, f32)
    if n_ch > 1:
        lv[1] = 0.0
    if n_ch > 2:
        lv[2] = ALL_CLOSED
    return lv


def gated(x, B, d, level, changes=None):
    """one channel through the squelch -> (gated stream of the whole blocks, powers, flags)"""
    return sm.stream(x, B, d, level, changes, power=sm.power32)


def flags64(x, B, d, level):
    """the open flags from the float64 power"""
    nb = x.size // B
    return np.array([sm.gate_open(sm.power64(x[k * B:(k + 1) * B], d), level) if level != 0 else True for k in range(nb)], np.uint8)


def undecidable_blocks(x, B, d, level):
    if level == 0:
        return []
    return [k for k in range(x.size // B) if sm.undecidable(B, d, sm.power64(x[k * B:(k + 1) * B], d), float(level))]


def classify(mode, flags, block_means=None, last_dc=0.0):
    """the way of every block: block_means[k] is fastdcblock_ff's mean of an open block k (AM)"""
    ways = []
    for k, fl in enumerate(flags):
        if fl:
            ways.append("open")
            if mode == "am":
                last_dc = float(block_means[k])
        else:
            ways.append("zero" if mode == "ssb" or last_dc == 0 else "ramp")
            last_dc = 0.0
    return ways


def expected(csdr_amd, P, x, d, level, changes=None, state=None):
    """csdr_amd_debug_amssb_walk on the model's gated stream of one channel -> (s16, pre_agc, powers, flags, the state behind)"""
    g, pw, fl = gated(x, P.block, d, level, changes)
    st = csdr_amd.AmSsbChan(0.0, 1.0) if state is None else csdr_amd.AmSsbChan(*state)
    s16, pre = csdr_amd.amssb_debug_walk(P, g, st)
    return s16, pre, pw, fl, (st.last_dc, st.last_gain)


# the shapes the GPU tests run: (channels, block, use_every_nth), NB blocks per channel, both modes
NB = 16
GPU_SHAPES = [(n_ch, B, d) for n_ch in (1, 5, 17) for B in (64, 128, 100, 2) for d in (1, 3)]
GPU_LEVELS = (LEVEL, ALL_CLOSED, 0.0)
