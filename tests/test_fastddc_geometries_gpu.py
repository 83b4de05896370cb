"""The fastddc inverse (fold -> inverse transforms -> scrap -> decimating_shift_addition_cc; fastddc.c:106-166, csdr.c:2302-2378) at EVERY geometry class
that selects other kernels, not only BASELINE config 4's (transition_bw 0.001, decimation 256: fft 65536 / pre_decimation 128 / post_decimation 2).

Which kernels serve a call follows from fastddc_init's geometry, the channel count and the blocks per call (fastddc_mfma.hip: ddc_mfma_create / _submit /
_collect; fftpath.hip: csdr_amd_fastddc_inv_process).  Every case below first asserts that geometry and the kernel instances of every call
(csdr_amd_fastddc_inv_kernels), then compares with the oracle (verify_configs.fastddc_oracle_channels, itself pinned to the compiled reference at the same
geometries by test_oracle_vs_ref.py::test_fastddc_stream):

  case  tbw, D                            fft / pre / post               what only this case runs
  a     0.01, 16                          4096 / 8 / 2                   k_ddc_gemm<.,true> and its K-loop tail (2 k-groups); 260 channels = a second 256-channel group
  b     0.01, 24 and 40                   4096 / 8 / 3, 5                k_ddc_ifft512_post<8> (post_decimation != 2) behind the four-product fold
  c     0.005, 32; 0.0025, 64; 0.002, 128 8192 / 16 .. 32768 / 64; 2     k_ddc_gemm<.,true> at 4, 8, 16 k-groups
  d     0.005, 48                         8192 / 16 / 3                  four equal calls of 7 blocks through the full-size inverse
  e     0.0005, 512 and 768               131072 / 256 / 2, 3            k_ddc_gemm<.,false> (non-persistent: 129 KiB of LDS for two tiles)
  f     0.001, 384                        65536 / 128 / 3                fused forward transform + k_ddc_gemm3 / k_ddc_gemm3n in front of k_ddc_ifft512_post<8>
  g     0.001, 640                        65536 / 128 / 5                k_ddc_xt + k_ddc_gemm3 + k_ddc_ifft512_post<8>
  h     0.00025, 1024                     262144 / 512 / 2               one 32-block tile per workgroup even above 32 blocks (two do not fit the LDS)
  i     0.000125, 2048                    524288 / 1024 / 2              the matrix-core path declines (one tile does not fit): general path
  j     0.05, 5 and 2                     1024 / 1 / 5, 2                k_ddc_fold<16> / <4> (pre_decimation 1)
  k     0.05, 50                          1024 / 2 / 25                  k_ddc_fold_ct<4,4> / <8,4> with post_decimation 25 (2.4 MS/s -> 48 kS/s)

Shapes: 40 blocks = two 32-block accumulator tiles, the second ragged; 33 = one block into the second tile; 37 channels = two channel waves, the second ragged;
260 channels = a second 256-channel group with one active wave.  The `spectra` entry (csdr_amd_fastddc_inv_*) and the `bank` entry (csdr_amd_fastddc_bank_*)
differ in k_ddc_xt against the forward path and in who carries the overlap tail.

Gates: equal sample counts per (channel, call); relative RMS per channel <= 1e-5 (BASELINE's float gate); the same ratio per (channel, call) -- a whole-stream
ratio over 40 blocks hides one wrong block of a ragged tile.  The per-call gate is 1e-5 too, except where the oracle's own worst per-block distance from the
compiled reference (test_oracle_vs_ref.py::test_fastddc_stream prints it; ORACLE_VS_REF below) is already above 1e-6: there ten times that figure."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import verify_configs as vc  # noqa: E402

pytestmark = pytest.mark.gpu
c64 = np.complex64
f32 = np.float32
TOL = 1e-5                  # per channel, whole stream
CROSS = 2e-6                # matrix-core path against the general kernels (the figure of the existing cross-path tests)

# oracle against oracle/_ref, worst relative RMS of ONE block (one shift rate per geometry, 3 .. 12 blocks; measured on the CPU by
# test_oracle_vs_ref.py::test_fastddc_stream) -> the per-call gate of the GPU: 1e-5, or ten times the figure where it exceeds 1e-6
ORACLE_VS_REF = {(0.01, 16): 1.25e-7, (0.01, 24): 1.39e-7, (0.01, 40): 1.57e-7, (0.005, 32): 3.63e-7, (0.0025, 64): 4.35e-7, (0.002, 128): 6.90e-7,
                 (0.005, 48): 7.50e-7, (0.0005, 512): 6.02e-8, (0.0005, 768): 1.70e-6, (0.001, 384): 1.27e-6, (0.001, 640): 1.43e-6,
                 (0.00025, 1024): 7.29e-7, (0.000125, 2048): 3.43e-6, (0.05, 5): 1.61e-7, (0.05, 2): 1.08e-7, (0.05, 50): 5.36e-7}
#   per-call gates that follow: (0.0005, 768) 1.70e-5, (0.001, 384) 1.27e-5, (0.001, 640) 1.43e-5, (0.000125, 2048) 3.43e-5, every other geometry 1e-5


def call_gate(tbw, D):
    fig = ORACLE_VS_REF[(tbw, D)]
    return 10 * fig if fig > 1e-6 else 1e-5


@pytest.fixture(scope="module")
def gpu():
    import torch  # noqa: F401
    import csdr_amd
    ctx = csdr_amd.Context(0)
    assert ctx.arch().startswith("gfx950")
    yield ctx
    ctx.close()


SPECIAL = [-0.4999, 0.4999, 0.0, 0.1234, -0.3711]      # both band edges, no shift, two rates off the 1 / fft grid of either sign


def rates_for(nch, pair=0):
    """Both band edges, 0.0, a positive and a negative rate off the 1 / fft grid at channels 0, last, middle, 1, last - 1; the rest spread like vc.c4_rates.
    Three channels: the edges and 0.  Two channels (cases h, i) cannot hold them all: the case runs twice, pair 0 and 1."""
    if nch == 2:
        return np.array([[-0.4999, 0.0], [0.4999, -0.3711]][pair], f32)
    if nch == 3:
        return np.array([-0.4999, 0.0, 0.4999], f32)
    r = vc.c4_rates(nch).copy()
    for k, v in zip([0, nch - 1, nch // 2, 1, nch - 2], SPECIAL):
        r[k] = v
    return r


def assert_rate_coverage(gpu, tbw, D, rates, fft):
    rates = [float(r) for r in rates]
    assert f32(-0.4999) in rates and f32(0.4999) in rates and 0.0 in rates
    off = [gpu.fastddc_init(tbw, D, r)[0].offsetbin for r in rates]
    assert max(off) > 0 and min(off) < 0, off
    assert any(abs(r * fft - round(r * fft)) > 1e-3 for r in rates)


def make_input(port, seed, n, fmt):
    """uniform complex noise: (what the bank is handed, the same stream as complexf)"""
    rng = np.random.default_rng(seed)
    if fmt == "u8":
        raw = rng.integers(0, 256, 2 * n, dtype=np.uint8)
        return raw, port.convert_u8_f(raw).view(c64)
    x = (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(c64)
    return x, x


_ORACLE = {}      # (tbw, D, nch, pair, schedule, fmt, retune) -> (input, spectra, {channel: [samples per call]}): computed once, shared by the entries and never changed
_RUNS = {}        # the same key + entry -> (streams, counts per call, kernels per call) of the default path, shared with the cross-path test


def oracle_calls(port, tbw, D, rate, spec, calls):
    pd, _ = port.fastddc_init(tbw, D, float(rate))
    blocks = port.fastddc_inv_cc(spec, pd, port.fastddc_taps_fft(pd, float(rate), D), per_block=True)
    ends = np.cumsum(calls)
    return [np.concatenate(blocks[e - n:e]) for n, e in zip(calls, ends)]


def oracle_for(port, key, check):
    tbw, D, nch, pair, schedule, fmt, retune = key
    if key not in _ORACLE:
        pd, _ = port.fastddc_init(tbw, D, 0.0)
        seed = 1000 + D + 7 * nch + pair + len(schedule)
        raw, xf = make_input(port, seed, pd.input_size * sum(schedule), fmt)
        rates = rates_for(nch, pair)
        calls = list(schedule)
        plain = [c for c in check if not retune or c != retune[1]]
        spec, want = vc.fastddc_oracle_channels(xf, tbw, D, rates, plain, calls=calls)
        if retune:      # csdr.c:2329-2376: geometry, taps and shift status of the channel restart with the new rate
            call, ch, rate = retune
            nb0 = sum(calls[:call])
            want[ch] = oracle_calls(port, tbw, D, rates[ch], spec[:nb0], calls[:call]) + oracle_calls(port, tbw, D, rate, spec[nb0:], calls[call:])
        _ORACLE[key] = (raw, spec, want)
    return _ORACLE[key]


def run_gpu(gpu, entry, key, raw, spec):
    tbw, D, nch, pair, schedule, fmt, retune = key
    rates = rates_for(nch, pair)
    if entry == "spectra":
        assert retune is None and all(n <= schedule[0] for n in schedule)
        outs = gpu.fastddc_inv_cc(spec, tbw, D, rates, blocks_per_call=schedule[0])
    else:
        outs = gpu.fastddc_bank(raw, tbw, D, rates, schedule=list(schedule), retune=retune)
    counts = [np.asarray(c) for c in gpu.ddc_call_counts]
    assert [int(c.size) for c in counts] == [nch] * len(schedule)
    return outs, counts, list(gpu.ddc_call_kernels)


def compare(label, outs, counts, want, check, gate_call, min_per_block, schedule):
    """every figure first (printed), then the asserts: counts per (channel, call), ratio per (channel, call), ratio per channel"""
    bad = []; worst_ch = worst_call = 0.0; where = None
    for c in check:
        pos = 0
        for k, w in enumerate(want[c]):
            n = int(counts[k][c])
            if n != w.size or n < schedule[k] * min_per_block - 1:
                bad.append("channel %d call %d: %d samples, oracle %d" % (c, k, n, w.size))
            else:
                r = vc.relrms(outs[c][pos:pos + n], w)
                if r > worst_call:
                    worst_call, where = r, (c, k)
                if not r <= gate_call:
                    bad.append("channel %d call %d: %.3g > %.3g" % (c, k, r, gate_call))
            pos += n
        whole = np.concatenate(want[c])
        if pos != outs[c].size or whole.size != outs[c].size:
            bad.append("channel %d: %d samples, oracle %d" % (c, outs[c].size, whole.size))
        else:
            r = vc.relrms(outs[c], whole)
            worst_ch = max(worst_ch, r)
            if not r <= TOL:
                bad.append("channel %d: %.3g > %.3g" % (c, r, TOL))
    print("\n[fastddc geometry] %s: %d channels compared, worst per channel %.3g (gate %.3g), worst per (channel, call) %.3g at %s (gate %.3g)"
          % (label, len(check), worst_ch, TOL, worst_call, where, gate_call))
    assert not bad, "%s: %s" % (label, "; ".join(bad[:8]))


XT = "k_ddc_xt+"
P256, P512 = "+k_ddc_ifft256d_post<8>", "+k_ddc_ifft512_post<8>"
GENERAL = "+hipfft+k_ddc_post"
EDGES_130 = [0, 1, 31, 32, 63, 64, 65, 95, 96, 127, 128, 129]      # case f / g: the tile edges of the fold (32-channel waves), both ends, the specials of rates_for


def geom(fft, pre, post, inv=512, scrap=64, post_in=448):
    return (fft, inv, pre, post, scrap, post_in)


def case(cid, tbw, D, g, entry, nch, schedule, kernels, fmt="cf32", retune=None, check=None, pairs=(0,)):
    return pytest.param(tbw, D, g, entry, nch, tuple(schedule), kernels, fmt, retune, check, pairs,
                        id="%s-D%d-%s-%dch-%s%s" % (cid, D, entry, nch, "+".join(map(str, schedule)), "" if fmt == "cf32" else "-" + fmt))


def gemm(a, b, post):
    return [XT + "k_ddc_gemm<%s>" % a + post, XT + "k_ddc_gemm<%s>" % b + post]


CASES = (
    # a: spectra and bank, 5 / 37 / 260 channels, 40 blocks then 3
    [case("a", 0.01, 16, geom(4096, 8, 2), e, n, [40, 3], gemm("2,true", "1,true", P256)) for e in ("spectra", "bank") for n in (5, 37, 260)]
    # b: the full-size inverse behind the same folds
    + [case("b", 0.01, D, geom(4096, 8, p), "spectra", 37, [40, 3], gemm("2,true", "1,true", P512)) for D, p in ((24, 3), (40, 5))]
    # c: 4, 8 and 16 k-groups, 33 blocks then 2
    + [case("c", t, D, geom(f, p, 2), "bank", 37, [33, 2], gemm("2,true", "1,true", P256)) for t, D, f, p in ((0.005, 32, 8192, 16), (0.0025, 64, 16384, 32), (0.002, 128, 32768, 64))]
    # d: four calls of 7 blocks
    + [case("d", 0.005, 48, geom(8192, 16, 3), "bank", 9, [7, 7, 7, 7], [XT + "k_ddc_gemm<1,true>" + P512] * 4)]
    # e: non-persistent folds
    + [case("e", 0.0005, D, geom(131072, 256, p), "spectra", 3, [33, 2], gemm("2,false", "1,false", post)) for D, p, post in ((512, 2, P256), (768, 3, P512))]
    # f: the bank's fused forward transform (pass 2 a kernel of its own in front of the narrow fold, inside the eight-wave fold), channel 3 / 96 retuned before call 1
    + [case("f", 0.001, 384, geom(65536, 128, 3), "bank", 5, [3, 2], ["k_ddc_fwd512<16,%d>+k_ddc_fwd128+k_ddc_gemm3n<1>" % q + P512] * 2, fmt=fmt, retune=(1, 3, 0.0517))
       for fmt, q in (("cf32", 0), ("u8", 2))]
    + [case("f", 0.001, 384, geom(65536, 128, 3), "bank", 130, [3, 2], ["k_ddc_fwd512<16,%d>+k_ddc_gemm3<1,true>" % q + P512] * 2, fmt=fmt, retune=(1, 96, 0.0517), check=EDGES_130)
       for fmt, q in (("cf32", 0), ("u8", 2))]
    # g: natural-order spectra into the three-product fold and the full-size inverse
    + [case("g", 0.001, 640, geom(65536, 128, 5), "spectra", 130, [5], [XT + "k_ddc_gemm3<1,false>" + P512], check=EDGES_130)]
    # h: pre_decimation 512 -- two 32-block tiles of spectra (257 KiB) do not fit a workgroup's 160 KiB: one tile per 32 blocks, also for the call of 34
    + [case("h", 0.00025, 1024, geom(262144, 512, 2), "bank", 2, s, [XT + "k_ddc_gemm<1,false>" + P256], pairs=(k,)) for k, s in enumerate(([3], [34]))]
    # i: pre_decimation 1024 -- one tile (256.5 KiB) does not fit either: the matrix-core path declines, the general kernels serve the geometry
    + [case("i", 0.000125, 2048, geom(524288, 1024, 2), "bank", 2, [2], ["k_ddc_fold<4>" + GENERAL], pairs=(0, 1))]
    # j: pre_decimation 1 (odd D, D = 2): the per-channel fold
    + [case("j", 0.05, D, geom(1024, 1, p, inv=1024, scrap=128, post_in=896), e, n, [20, 3], ["k_ddc_fold<16>" + GENERAL, "k_ddc_fold<4>" + GENERAL])
       for D, p in ((5, 5), (2, 2)) for e in ("spectra", "bank") for n in (3, 9)]
    # k: post_decimation 25
    + [case("k", 0.05, 50, geom(1024, 2, 25), "bank", n, [7], ["k_ddc_fold_ct<%d,4>" % ct + GENERAL]) for n, ct in ((6, 4), (9, 8))]
)


@pytest.mark.parametrize("tbw,D,g,entry,nch,schedule,kernels,fmt,retune,check,pairs", CASES)
def test_geometry_class(gpu, port, tbw, D, g, entry, nch, schedule, kernels, fmt, retune, check, pairs):
    """One geometry class: geometry, then the kernel instances of every call, then counts and ratios per (channel, call) and per channel against the oracle.
    pairs: which of the two-channel rate pairs the case runs with, one after the other (rates_for; more channels: one run)."""
    ddc, err = gpu.fastddc_init(tbw, D, 0.0)
    assert err == 0
    assert (ddc.fft_size, ddc.fft_inv_size, ddc.pre_decimation, ddc.post_decimation, ddc.scrap, ddc.post_input_size) == g
    check = list(range(nch)) if check is None else check
    seen = []
    for pair in pairs:
        key = (tbw, D, nch, pair, schedule, fmt, retune)
        raw, spec, want = oracle_for(port, key, check)
        outs, counts, ran = run_gpu(gpu, entry, key, raw, spec)
        _RUNS[key + (entry,)] = (outs, counts, ran)
        assert ran == kernels, ran
        assert gpu.last_ddc_kernels == kernels[-1] and set(kernels) <= gpu.ddc_kernels_seen
        assert len(outs) == nch
        compare("tbw %g D %d %s %d channels%s calls %s %s" % (tbw, D, entry, nch, " (%s)" % fmt if fmt != "cf32" else "", list(schedule), " then ".join(ran[k] for k in range(len(ran)) if k == 0 or ran[k] != ran[k - 1])),
                outs, counts, want, check, call_gate(tbw, D), ddc.post_input_size // ddc.post_decimation, schedule)
        seen += [float(r) for c, r in enumerate(rates_for(nch, pair)) if c in check]
    if nch > 2:
        assert_rate_coverage(gpu, tbw, D, seen, ddc.fft_size)


def test_two_channel_cases_cover_the_rates(gpu):
    """cases h and i have two channels: the rate set every case must hold (edges, 0, either offsetbin sign, off-grid) is spread over their two pairs"""
    for tbw, D, fft in ((0.00025, 1024, 262144), (0.000125, 2048, 524288)):
        assert_rate_coverage(gpu, tbw, D, list(rates_for(2, 0)) + list(rates_for(2, 1)), fft)


CROSS_CASES = [c for c in CASES if (c.id[0] in "ab" and ("37ch" in c.id or "260ch" in c.id)) or (c.id[0] == "f" and "u8" not in c.id)]


@pytest.mark.parametrize("tbw,D,g,entry,nch,schedule,kernels,fmt,retune,check,pairs", CROSS_CASES)
def test_matrix_core_path_against_general_kernels(gpu, port, monkeypatch, tbw, D, g, entry, nch, schedule, kernels, fmt, retune, check, pairs):
    """Cases a, b and f: the same call sequence with CSDR_AMD_DDC_MFMA_OFF set before the object is created runs the general kernels (asserted by name) and gives
    equal counts per call and the matrix-core path's streams to 2e-6 -- EVERY channel (where the oracle compares a subset, this pins the rest)."""
    key = (tbw, D, nch, 0, schedule, fmt, retune)
    raw, spec, _ = oracle_for(port, key, list(range(nch)) if check is None else check)
    if key + (entry,) not in _RUNS:
        _RUNS[key + (entry,)] = run_gpu(gpu, entry, key, raw, spec)
    outs, counts, ran = _RUNS[key + (entry,)]
    assert ran == kernels
    monkeypatch.setenv("CSDR_AMD_DDC_MFMA_OFF", "1")
    gen, gcounts, gran = run_gpu(gpu, entry, key, raw, spec)
    assert gran == ["k_ddc_fold_ct<%d,4>" % (8 if nch >= 8 else 4) + GENERAL] * len(schedule), gran
    for k in range(len(schedule)):
        assert np.array_equal(counts[k], gcounts[k]), "call %d" % k
    ratios = [vc.relrms(gen[c], outs[c]) if gen[c].size == outs[c].size else np.inf for c in range(nch)]
    worst = max(ratios)
    print("\n[fastddc geometry] tbw %g D %d %s %d channels: matrix-core path against the general kernels, worst channel %.3g (gate %.3g)" % (tbw, D, entry, nch, worst, CROSS))
    assert worst <= CROSS, [c for c in range(nch) if not ratios[c] <= CROSS][:8]
