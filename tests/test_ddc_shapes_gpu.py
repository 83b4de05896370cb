"""The fused u8 front end (csdr_amd_ddc_*: k_ddc_mfma / k_ddc_direct, csdr_amd/csrc/ddc_mfma.hip) at every decimation class and kernel instance, against
the float64 reference and the per-sample gate of ddc_reference.py, on byte-domain inputs: uniform random bytes, the rails 0 (int8 -128 on the matrix cores)
and 255, I = 0 / Q = 255, and an FM signal clipped to the rails.

Every case asserts the set of dispatch reports (csdr_amd_ddc_last_instance) against ddc_reference's transcription of the host dispatch; between them the
cases name all eight k_ddc_mfma<13,NT,FUSE,PS> instances (the two-team fused ones: test_ddc_gpu.py, test_rates_gpu.py), both call classes (whole, tiles)
and k_ddc_direct alone.  Calls: ddc_reference.schedule -- a first call of at least 33 tiles with partial first / last tiles, a call of exactly 1024 samples
(k_ddc_direct takes it whole), a further whole call, a ragged last call.  RATIO lines: the worst error as a fraction of the gate."""
import os
import subprocess
import sys
import numpy as np
import pytest

import ddc_reference as dr
import fir_reference as fr
import verify_configs as vc
from tests_helpers import nfm_signal_u8

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
c64, f32 = np.complex64, np.float32
GATED_ROWS = (0, 1, 2, 3, 4, 5, 6, 16, 18)      # every kind of row in the full group, two rows of the ragged one
TEAM_SHAPES = [(50, 801, 0.11), (16, 255, -0.4321)]
TEAM_RATE_SHAPES = [s for s in dr.RATE_SHAPES if (s[0], s[1]) in ((50, 801), (16, 255))]
_default_runs = {}                              # (kind, D, L) -> output of the default (two-team) run, for the comparison with CSDR_AMD_DDC_TEAMS=1


@pytest.fixture(scope="module")
def gpu():
    import torch  # noqa: F401
    import csdr_amd
    ctx = csdr_amd.Context(0)
    yield ctx
    ctx.close()


def _taps(port, D, L, kind):
    return fr.random_taps(L, D + L) if kind == "random" else port.firdes_lowpass_f(L, 0.5 / D)


def _gate_rows(port, y, u8, rows, plans, D, taps):
    """worst gate ratio over `rows`; plans[s] = [(first sample, rate), ...] of row s"""
    n = u8.shape[1] // 2
    L = taps.size
    assert y.shape[1] == (n - L) // D + 1
    phasors, worst = {}, 0.0
    for s in rows:
        plan = tuple(plans[s])
        if plan not in phasors:
            R = dr.phasor_sequence(port, n, plan)
            phasors[plan] = (R, dr.plan_rho(R, plan), max(dr.weight_step(D, L, taps, r) for _, r in plan))
        R, rho, q = phasors[plan]
        y64, c, s1, s2 = dr.reference(port, u8[s], R, D, taps)
        g = dr.gate_ratio(y[s], y64, dr.bound(c, s1, s2, L, q, rho))
        assert g <= 1.0, "row %d: error %.3g x the gate" % (s, g)
        worst = max(worst, g)
    return worst


def _run_shared(gpu, port, D, L, rate, kind, sched_L, teams=2):
    taps = _taps(port, D, L, kind)
    sizes, n = dr.schedule(D, sched_L)
    u8 = dr.byte_rows(n, rate, 100 * D + sched_L)
    y = gpu.ddc_u8(u8, rate, D, taps, block=sizes)
    print("INSTANCES D=%d L=%d %s:" % (D, L, kind), sorted(gpu.ddc_instances))
    assert gpu.ddc_instances == dr.ddc_instances(D, L, False, False, sizes, n, teams)
    worst = _gate_rows(port, y, u8, GATED_ROWS, {s: [(0, rate)] for s in range(19)}, D, taps)
    assert np.array_equal(y[15:19].view(np.uint32), y[0:4].view(np.uint32))          # the copies in the ragged group of 16: bit identical
    print("RATIO ddc teams=%d D=%d L=%d %s rate=%g %.4f" % (teams, D, L, kind, rate, worst))
    return y


def _run_rates(gpu, port, D, L, rates, teams=2):
    """3 streams (random bytes, random bytes, a clipped FM signal at its rate), a rate each; (100, 451): stream 1 is retuned in front of the third call"""
    taps = _taps(port, D, L, "random")
    sizes, n = dr.schedule(D, L)
    rows = dr.byte_rows(n, 0.0, 300 * D + L)
    u8 = np.stack([rows[0], rows[1], dr.fm_clipped_u8(7 * D + L, n, -rates[2])])
    retunes = {2: [(1, 0.3)]} if D == 100 else None
    plans = {s: [(0, float(rates[s]))] for s in range(3)}
    if retunes:
        plans[1].append((sizes[0] + sizes[1], 0.3))
    y = gpu.ddc_u8(u8, np.array(rates, f32), D, taps, block=sizes, retunes=retunes)
    print("INSTANCES rates D=%d L=%d:" % (D, L), sorted(gpu.ddc_instances))
    drifting = any(r in dr.RATES_DRIFT for r in rates)
    assert gpu.ddc_instances == dr.ddc_instances(D, L, True, False, sizes, n, teams, retunes, drifting)
    worst = _gate_rows(port, y, u8, (0, 1, 2), plans, D, taps)
    print("RATIO ddc rates teams=%d D=%d L=%d rates=%s %.4f" % (teams, D, L, rates, worst))
    return y


@pytest.mark.parametrize("D,L,Lo,rate", dr.SHAPES)
def test_ddc_shapes_shared_rate(gpu, port, D, L, Lo, rate):
    """19 streams (one full group of 16, one ragged) through the shared-rate object: random asymmetric taps on every shape, designed lowpass taps on three"""
    _default_runs[("shared", D, L)] = _run_shared(gpu, port, D, L, rate, "random", L)
    if Lo:
        _run_shared(gpu, port, D, Lo, rate, "lowpass", L)


@pytest.mark.parametrize("D,L,rates", dr.RATE_SHAPES)
def test_ddc_shapes_rate_per_stream(gpu, port, D, L, rates):
    """csdr_amd_ddc_create_rates: columns in periods of lcm(8 D, 1024) samples -- 8 tiles at D = 16, 64 at 50, 2 at 64, 16 at 100, 1 at 128"""
    _default_runs[("rates", D, L)] = _run_rates(gpu, port, D, L, rates)


@pytest.mark.parametrize("rates", [(0.2, -0.4321, 0.05), (0.11, -0.4321, 0.3)])
def test_ddc_few_taps_rate_per_stream(gpu, port, rates):
    """(164, 4) with a rate per stream.  The per-stream kernel samples a drifting stream's correction once per 288-sample K-range part: with 4 taps an output's taps
    can all sit 142 samples from there, and the kernel missed the gate by 1.3 (rate 1e-4) to 1.85 (0.05).  Objects with fewer than 100 taps and a drifting stream
    run on k_ddc_direct; without a drifting stream they stay on the matrix cores."""
    _run_rates(gpu, port, 164, 4, rates)
    drifting = any(r in dr.RATES_DRIFT for r in rates)
    assert gpu.ddc_instances == ({"k_ddc_direct"} if drifting else {"k_ddc_direct", "k_ddc_mfma<13,1,false,true> whole"})


def _teams_child(out_path):
    """run with CSDR_AMD_DDC_TEAMS=1 in the environment: the one-team instances at shapes that run on two teams by default"""
    import csdr_amd
    import oracle
    ctx = csdr_amd.Context(0)
    port = oracle.port()
    out = {}
    for D, L, rate in TEAM_SHAPES:
        out["shared_%d_%d" % (D, L)] = _run_shared(ctx, port, D, L, rate, "random", L, teams=1)
    for D, L, rates in TEAM_RATE_SHAPES:
        out["rates_%d_%d" % (D, L)] = _run_rates(ctx, port, D, L, rates, teams=1)
    ctx.close()
    np.savez(out_path, **out)


def test_ddc_one_team_equals_two_teams(gpu, port, tmp_path):
    """CSDR_AMD_DDC_TEAMS=1 (read once per process: a child) at (50, 801) and (16, 255): the same gate, the instances k_ddc_mfma<13,1,...>, and the same bits as
    the default run -- a tile's arithmetic (its K-ranges' integer sums, post factors, the order of the reduction) does not depend on how many tiles a
    workgroup computes side by side."""
    path = str(tmp_path / "one_team.npz")
    env = dict(os.environ, CSDR_AMD_DDC_TEAMS="1")
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(1, %r); import test_ddc_shapes_gpu as t; t._teams_child(%r)" % (HERE, os.path.dirname(HERE), path)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("RATIO") == len(TEAM_SHAPES) + len(TEAM_RATE_SHAPES) and "<13,1,false,false> whole" in r.stdout and "<13,1,false,true> whole" in r.stdout
    one = np.load(path)
    for D, L, rate in TEAM_SHAPES:
        two = _default_runs.get(("shared", D, L))
        if two is None:
            two = _run_shared(gpu, port, D, L, rate, "random", L)
        assert np.array_equal(one["shared_%d_%d" % (D, L)].view(np.uint32), two.view(np.uint32)), (D, L)
    for D, L, rates in TEAM_RATE_SHAPES:
        two = _default_runs.get(("rates", D, L))
        if two is None:
            two = _run_rates(gpu, port, D, L, rates)
        assert np.array_equal(one["rates_%d_%d" % (D, L)].view(np.uint32), two.view(np.uint32)), (D, L)


@pytest.mark.parametrize("per_stream", [False, True])
def test_nfm_chain_one_team_epilogue(gpu, port, per_stream):
    """The fused demodulating epilogue on one team (D = 100: no other team to re-reduce y[k - 1] from, two fetching waves): the NFM chain's s16 audio +-1 LSB against
    the oracle's eight stages per channel, and several calls bit identical to one call."""
    D, S, tbw = 100, 3, 0.01
    sizes = [1024 * 160, 1024 * 90]
    n = 1024 * 300
    L = gpu.firdes_filter_len(tbw)
    assert L % 2 == 1 and L <= 451 and dr.ddc_supported(D, L)
    rates = [-0.085, 0.25, 0.11]
    run_rates = np.array(rates, f32) if per_stream else rates[1]
    u8 = np.stack([nfm_signal_u8(1400 + s, n, offset=-float(rates[s] if per_stream else rates[1])) for s in range(S)])
    nfm_taps = gpu.nfm_taps(48000)
    inst = "k_ddc_mfma<13,1,true,%s> whole" % ("true" if per_stream else "false")
    pcm, _ = gpu.nfm_chain(u8, run_rates, decimation=D, tbw=tbw)
    print("INSTANCES nfm D=%d L=%d:" % (D, L), sorted(gpu.ddc_instances))
    assert gpu.ddc_instances == {inst} == dr.ddc_instances(D, L, per_stream, True, [n], n)
    for s in range(S):
        ps, _ = port.nfm_chain(u8[s], float(rates[s] if per_stream else rates[1]), nfm_taps, D, tbw, 1024)
        assert pcm.shape[1] == ps.size and vc.s16_diff(pcm[s], ps).max() <= 1, "channel %d" % s
    pcm2, _ = gpu.nfm_chain(u8, run_rates, decimation=D, tbw=tbw, block=sizes)
    print("INSTANCES nfm D=%d L=%d in calls:" % (D, L), sorted(gpu.ddc_instances))
    assert gpu.ddc_instances == {inst} == dr.ddc_instances(D, L, per_stream, True, sizes, n)
    m = min(pcm.shape[1], pcm2.shape[1])
    assert m >= pcm.shape[1] - 2048 and np.array_equal(pcm[:, :m], pcm2[:, :m])
