"""The per-stream chunk-seed tables (csdr_amd/csrc/seeds.hip) past their first table: a prepared table taking over, a prepared table that does not fit the call,
retunes around a takeover, drift-correction rows running out in mid-stream, a reset after a takeover, the host phase chain of one or two streams -- and the
shared-rate objects' host-built table rebuilt 16 calls ahead (ddc_mfma.hip, wfm.hip).

A table holds cap = 8 * (max_block_samples / 1024 + 8) chunks; a call of nch chunks asks for nch + 3 entries from chunk B / 1024 - 1 on.  Every case streams
short calls (2 to 4 chunks) through an object whose max_block_samples is 4 chunks (cap = 96) and is compared in two ways:
  * against the oracle's full-stream model (test_rates_gpu.py's stages and gates: relative RMS <= 1e-5 on complex samples, +-1 LSB on s16);
  * bit for bit against a TWIN: the same calls through an object whose max_block_samples is the whole stream, so that its first table covers everything.
    max_block_samples sizes the tables (seeds_create, ctab_cap) and buffers (the NFM back end's pitches, the WFM VALU path's scratch); no grid size and no
    kernel choice reads it (ddc_process_fused, wfm_mfma_launch: they take T), so both objects launch the same kernels on the same tiles and may differ only in
    where the seeds come from.  The phase chain is deterministic float arithmetic: the outputs must be EQUAL.  Every case asserts that the dispatch reports agree.
Each case asserts on csdr_amd_ddc_seed_stats / csdr_amd_wfm_seed_stats / *_tables_built that the path it names ran; SeedModel below mirrors seeds_acquire's
bookkeeping (covers(), the `f` loop) and says where."""
import numpy as np
import pytest
from oracle import relrms
from tests_helpers import nfm_signal_u8, wfm_signal_u8
from test_rates_gpu import oracle_front, RATES, WRATES, TOL
import verify_configs as vc

pytestmark = pytest.mark.gpu
c64, f32 = np.complex64, np.float32
D, L = 50, 801
CH = 1024
MAXB = 4 * CH                              # the small-table objects' max_block_samples
CAP = 8 * (MAXB // CH + 8)                 # seeds_create: k = 8 calls ahead (the 96-MB bound is far away), per_call = max_block_samples / 1024 + 8
SPARE_ROWS = 8                             # seeds_set_drift: alloc_corr(t, rows + 8)
# rates whose float recurrence drifts (ddc_rotator_model_rms > 2e-6: 6e-6 .. 1.7e-5; every rate of NOT_DRIFTING is below 1.2e-6)
DRIFTING = [0.05, 0.25, -0.05, 0.125, -0.25, 0.1, -0.1, 0.2, -0.2, -0.125]
NOT_DRIFTING = [0.11, -0.4321, 0.3, -0.2718, 0.0123, 0.499, -0.3333, 0.085, -0.1234, 0.4, -0.45]


class SeedModel:
    """seeds_acquire's table bookkeeping on the host: which table a call reads and which branch got it there."""

    def __init__(self, cap):
        self.cap = cap; self.first = [0, 0]; self.valid = [False, False]; self.cur = 0; self.fresh = True; self.dirty = False
        self.stats = dict(generated=0, takeovers=0, refits=0, dirty=0, takeover_calls=[], refit_calls=[])

    def _generate(self, dst, first):
        self.first[dst] = first; self.valid[dst] = True; self.stats["generated"] += 1

    def acquire(self, call, first, n, hint):
        cap = self.cap
        assert n + 2 <= cap
        covers = lambda b: self.valid[b] and first >= self.first[b] and first + n <= self.first[b] + cap
        if self.fresh:
            self.valid = [False, False]; self.cur = 0
            self._generate(0, first); self.fresh = False; self.dirty = False
        elif self.dirty or not covers(self.cur):
            o = self.cur ^ 1
            if not self.dirty and covers(o):
                self.cur = o; self.stats["takeovers"] += 1; self.stats["takeover_calls"].append(call)
            else:
                src = [b for b in (self.cur, o) if self.valid[b] and first >= self.first[b] and first + 1 < self.first[b] + cap][0]
                if self.dirty: self.stats["dirty"] += 1
                else: self.stats["refits"] += 1; self.stats["refit_calls"].append(call)
                self.valid[src ^ 1] = False; self._generate(src ^ 1, first); self.cur = src ^ 1
            self.dirty = False
        c, o = self.cur, self.cur ^ 1
        if not (self.valid[o] and self.first[o] > self.first[c]) and hint > 0:
            f = first
            while f + n <= self.first[c] + cap: f += hint
            if 0 <= f - self.first[c] and f - self.first[c] + 1 < cap: self.valid[o] = False; self._generate(o, f)
        return c

    @classmethod
    def run(cls, sizes, cap=CAP, retune_calls=(), reset_at=None):
        """sizes: samples per call (multiples of 1024); retune_calls: calls with a set_rate in front of them"""
        m = cls(cap); B = 0; m.tables = []
        for call, T in enumerate(sizes):
            if call == reset_at: m.fresh = True; m.dirty = False; m.valid = [False, False]; m.cur = 0; B = 0
            if call in retune_calls: m.dirty = True
            nch = T // CH
            m.tables.append(m.acquire(call, B // CH - 1, nch + 3, nch)); B += T
        return m


def check_stats(got, model, **more):
    want = dict(model.stats, **more)
    print("SEED STATS", {k: got[k] for k in sorted(got)})
    for k, v in want.items():
        assert got[k] == v, "seed stats %s: %r, the host model of seeds_acquire says %r (%r)" % (k, got[k], v, got)


@pytest.fixture(scope="module")
def gpu():
    import torch  # noqa: F401
    import csdr_amd
    ctx = csdr_amd.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def taps(port):
    return port.firdes_lowpass_f(L, 0.5 / D)


def moving_signal(seed, plan, n, gen=nfm_signal_u8):
    """a signal that follows the stream's tuning: at -rate in every stretch of plan = [(first sample, rate), ...]"""
    return np.concatenate([gen(seed + i, (plan[i + 1][0] if i + 1 < len(plan) else n) - a, offset=-r) for i, (a, r) in enumerate(plan)])


def err_per_sample(y, want):
    return np.abs(y - want) / np.sqrt(np.mean(np.abs(want) ** 2))


def check_ddc_vs_oracle(port, y, u8, plans, taps, label, windows=()):
    """test_rates_gpu.py's gates on every stream: relative RMS <= 1e-5, and (test_ddc_retune_between_calls' form) no sample off by 1e-4 of the RMS level --
    on the whole stream, and reported for the output ranges `windows` (the calls behind a takeover / retune: a one-chunk phase slip is gross there)."""
    worst = wmax = wwin = 0.0
    for s in range(len(plans)):
        want = oracle_front(port, u8[s], plans[s], D, taps)
        assert y.shape[1] == want.size
        e = err_per_sample(y[s], want); r = relrms(y[s], want); worst = max(worst, r); wmax = max(wmax, e.max())
        for a, b in windows:
            wwin = max(wwin, e[a:b].max())
            assert e[a:b].max() < 1e-4, "%s stream %d: max %g in outputs [%d, %d)" % (label, s, e[a:b].max(), a, b)
        assert r <= TOL and e.max() < 1e-4, "%s stream %d: rms %g max %g at %d" % (label, s, r, e.max(), int(e.argmax()))
    print("ORACLE %s: worst relative RMS %.3g, worst sample %.3g, worst sample behind a switch %.3g" % (label, worst, wmax, wwin))


def call_windows(gpu, calls, n_out):
    """output ranges of the given calls and the call behind each"""
    first = list(gpu.ddc_call_out) + [n_out]
    return [(first[c], first[min(c + 2, len(first) - 1)]) for c in calls]


def run_pair(gpu, u8, rates, taps, sizes, retunes=None):
    """the small-table object and its twin: (y, stats, y_twin, stats_twin, output windows of the small-table object's switches); the dispatch reports agree"""
    n = u8.shape[1] // 2
    assert sum(sizes) == n
    y = gpu.ddc_u8(u8, rates, D, taps, block=sizes, retunes=retunes, max_block=MAXB)
    st, inst = gpu.ddc_seed_stats, set(gpu.ddc_instances)
    assert gpu.ddc_kernels == {"k_ddc_mfma"}, gpu.ddc_kernels           # every call on the matrix-core kernel (whole calls: T % 512 == 0, T >= 2048, >= 4 tiles)
    win = call_windows(gpu, st["takeover_calls"] + st["refit_calls"] + sorted(retunes or {}), y.shape[1])
    yt = gpu.ddc_u8(u8, rates, D, taps, block=sizes, retunes=retunes, max_block=n)
    stt = gpu.ddc_seed_stats
    assert gpu.ddc_kernels == {"k_ddc_mfma"} and set(gpu.ddc_instances) == inst, (inst, gpu.ddc_instances)
    assert stt["takeovers"] == 0 and stt["refits"] == 0, stt              # the twin never leaves its first table (a retune regenerates it in place)
    return y, st, yt, stt, win


def test_takeover(gpu, port, taps):
    """60 equal calls of 4 chunks, 11 streams (three of them on drifting rates: correction rows travel with the tables): the prepared table takes over in front
    of calls 23 and 46, never refitted."""
    S, sizes = 11, [4 * CH] * 60
    n = sum(sizes)
    rates = np.array(RATES[:S], f32)
    u8 = np.stack([nfm_signal_u8(3000 + s, n, offset=-float(rates[s])) for s in range(S)])
    y, st, yt, stt, win = run_pair(gpu, u8, rates, taps, sizes)
    m = SeedModel.run(sizes)
    assert m.stats["takeover_calls"] == [23, 46]
    check_stats(st, m, regrowths=0)
    assert st["takeovers"] >= 2 and st["refits"] == 0 and stt["takeovers"] == 0
    assert np.array_equal(y.view(np.uint32), yt.view(np.uint32)), "small tables and the twin differ first at output %d" % int(np.argmax((y != yt).any(axis=0)))
    check_ddc_vs_oracle(port, y, u8, [[(0, float(r))] for r in rates], taps, "takeover", win)


@pytest.mark.parametrize("sizes,refits,takeovers", [
    ([4 * CH] + [3 * CH] * 65, [30], [61]),                  # the prepared table starts at chunk 91, call 30 starts at 90: one chunk before it -> refit; its successor then fits
    ([4 * CH, 3 * CH] + [2 * CH] * 45 + [3 * CH] * 33, [76], [45]),      # call 45 starts at 92, one chunk behind that start: a takeover at entry 1; the 3-chunk calls then miss
                                                                         # the next prepared table (the regeneration reads table 1)
])
def test_prepared_table_does_not_fit(gpu, port, taps, sizes, refits, takeovers):
    """The first call's size fixes where the prepared table starts; calls of another size reach its neighbourhood one chunk early (seeds_acquire regenerates from
    entries idx, idx + 1 of the current table with idx > 0, not dirty) or one chunk late (a takeover that starts inside the prepared table)."""
    S = 5
    n = sum(sizes)
    rates = np.array(RATES[2:2 + S], f32)                    # 0.05, 0.25, -0.05 drift
    m = SeedModel.run(sizes)
    assert m.stats["refit_calls"] == refits and m.stats["takeover_calls"] == takeovers, m.stats
    u8 = np.stack([nfm_signal_u8(3100 + s, n, offset=-float(rates[s])) for s in range(S)])
    y, st, yt, stt, win = run_pair(gpu, u8, rates, taps, sizes)
    check_stats(st, m, regrowths=0)
    assert st["refits"] >= 1
    assert np.array_equal(y.view(np.uint32), yt.view(np.uint32)), "small tables and the twin differ first at output %d" % int(np.argmax((y != yt).any(axis=0)))
    check_ddc_vs_oracle(port, y, u8, [[(0, float(r))] for r in rates], taps, "refit", win)


RT_SIZES = [4 * CH] * 60
RT_RATES0 = [0.11, 0.25, 0.3]


@pytest.fixture(scope="module")
def untouched(gpu, taps):
    """stream 2 of the retune cases, and what the small-table object gives for it when nothing is retuned"""
    n = sum(RT_SIZES)
    u2 = nfm_signal_u8(3202, n, offset=-RT_RATES0[2])
    u8 = np.stack([nfm_signal_u8(3200, n, offset=-RT_RATES0[0]), nfm_signal_u8(3201, n, offset=-RT_RATES0[1]), u2])
    y = gpu.ddc_u8(u8, np.array(RT_RATES0, f32), D, taps, block=RT_SIZES, max_block=MAXB)
    return u2, y[2].copy()


@pytest.mark.parametrize("call,takeovers", [(22, [45]), (23, [46]), (24, [23, 47])])
def test_retune_around_a_takeover(gpu, port, taps, untouched, call, takeovers):
    """A retune one call before the first takeover (call 23), at it (the prepared table is dropped and rebuilt from the last entries of table 0) and behind it (the
    source of the regeneration is table 1).  Stream 0 goes to a drifting rate, stream 1 leaves one, stream 2 stays and is bit-identical to the run without retunes."""
    sizes = RT_SIZES
    n = sum(sizes); pos = call * 4 * CH
    plans = [[(0, RT_RATES0[0]), (pos, 0.05)], [(0, RT_RATES0[1]), (pos, -0.31)], [(0, RT_RATES0[2])]]
    u2, y2 = untouched
    u8 = np.stack([moving_signal(3210 + 10 * call, plans[0], n), moving_signal(3215 + 10 * call, plans[1], n), u2])
    retunes = {call: [(0, 0.05), (1, -0.31)]}
    m = SeedModel.run(sizes, retune_calls=[call])
    assert m.stats["takeover_calls"] == takeovers and m.stats["dirty"] == 1, m.stats
    assert m.tables[call - 1] == (1 if call == 24 else 0)                 # the table the regeneration reads
    y, st, yt, stt, win = run_pair(gpu, u8, np.array(RT_RATES0, f32), taps, sizes, retunes)
    check_stats(st, m, regrowths=0)
    assert st["dirty"] == 1 and stt["dirty"] == 1 and st["takeovers"] >= 1
    assert np.array_equal(y.view(np.uint32), yt.view(np.uint32)), "small tables and the twin differ first at output %d" % int(np.argmax((y != yt).any(axis=0)))
    assert np.array_equal(y[2].view(np.uint32), y2.view(np.uint32)), "the untouched stream moved"
    check_ddc_vs_oracle(port, y, u8, plans, taps, "retune at call %d" % call, win)


def test_correction_rows_run_out(gpu, port, taps):
    """Created without a drifting stream (no correction rows at all); behind the first takeover ten streams go to drifting rates, one per call from call 24 on.
    seeds_set_rate grows the rows by `rows + 8` whenever none is free: at the first of them (0 -> 9 rows) and at the tenth (9 -> 18); the current table's phases
    survive, the corrections are regenerated, the streams retuned earlier keep theirs: stream 0, drifting since call 24, moves on to another drifting rate in
    front of the same call as the tenth retune, BEHIND it -- the old rate's corrections of the chunk in front of the block (seeds_corr_entry) must have survived
    the regrowth.  Second object: the same schedule on streams that are drifting from the start (18 rows from create: never regrown) and move between drifting
    rates -- seeds_corr_entry hands those corrections out of table 1."""
    S, sizes, first_call, n_ret = 11, [4 * CH] * 60, 24, SPARE_ROWS + 2
    n = sum(sizes)
    retunes = {first_call + j: [(j, DRIFTING[j])] for j in range(n_ret)}
    last = first_call + n_ret - 1
    retunes[last].append((0, 0.2))
    m = SeedModel.run(sizes, retune_calls=sorted(retunes))
    assert m.stats["takeover_calls"][0] == 23 and m.stats["dirty"] == n_ret
    for label, rates0 in (("rows run out", NOT_DRIFTING[:S]), ("drifting from the start", [DRIFTING[(j + 3) % n_ret] for j in range(n_ret)] + NOT_DRIFTING[n_ret:S])):
        plans = [[(0, rates0[s])] + ([(int((first_call + s) * 4 * CH), DRIFTING[s])] if s < n_ret else []) for s in range(S)]
        plans[0].append((last * 4 * CH, 0.2))
        u8 = np.stack([moving_signal(3300 + 10 * s, plans[s], n) for s in range(S)])
        y, st, yt, stt, win = run_pair(gpu, u8, np.array(rates0, f32), taps, sizes, retunes)
        grown = 2 if label == "rows run out" else 0
        check_stats(st, m, regrowths=grown)
        assert stt["regrowths"] == grown and stt["dirty"] == n_ret
        assert np.array_equal(y.view(np.uint32), yt.view(np.uint32)), "%s: small tables and the twin differ first at output %d" % (label, int(np.argmax((y != yt).any(axis=0))))
        check_ddc_vs_oracle(port, y, u8, plans, taps, label, win)


def test_reset_after_a_takeover(gpu, port, taps):
    """csdr_amd_ddc_reset in front of call 30 (the object reads table 1 by then): what follows is the stream a fresh object gives, bit for bit, takeovers included."""
    S, sizes, at = 5, [4 * CH] * 60, 30
    n = sum(sizes); pos = at * 4 * CH
    rates = np.array(RATES[:S], f32)
    u8 = np.stack([nfm_signal_u8(3400 + s, n, offset=-float(rates[s])) for s in range(S)])
    y = gpu.ddc_u8(u8, rates, D, taps, block=sizes, max_block=MAXB, reset_at=at)
    st, cut = gpu.ddc_seed_stats, gpu.ddc_reset_out
    m = SeedModel.run(sizes, reset_at=at)
    assert m.stats["takeover_calls"] == [23, at + 23]
    check_stats(st, m, regrowths=0)
    tail = np.ascontiguousarray(u8[:, 2 * pos:])
    fresh = gpu.ddc_u8(tail, rates, D, taps, block=sizes[at:], max_block=MAXB)
    assert gpu.ddc_seed_stats["takeover_calls"] == [23]
    assert y.shape[1] - cut == fresh.shape[1] and np.array_equal(y[:, cut:].view(np.uint32), fresh.view(np.uint32))
    check_ddc_vs_oracle(port, fresh, tail, [[(0, float(r))] for r in rates], taps, "fresh object")
    check_ddc_vs_oracle(port, y[:, :cut], u8[:, :2 * pos], [[(0, float(r))] for r in rates], taps, "in front of the reset")


@pytest.mark.parametrize("S", [1, 2])
def test_host_phase_chain(gpu, port, taps, monkeypatch, S):
    """One or two streams (the command-line tool's configuration): the phase chain runs on the host into pinned shadows of the two tables (CSDR_AMD_SEED_HOST,
    read at create; default 2 streams) and continues from a shadow at every takeover and retune.  Against the device chain (CSDR_AMD_SEED_HOST=0): bit-identical."""
    sizes, call = [4 * CH] * 60, 30
    n = sum(sizes); pos = call * 4 * CH
    rates0 = [0.25, 0.11][:S]
    plans = [[(0, 0.25), (pos, -0.4321)], [(0, 0.11)]][:S]
    retunes = {call: [(0, -0.4321)]}
    u8 = np.stack([moving_signal(3500 + 10 * s, plans[s], n) for s in range(S)])
    m = SeedModel.run(sizes, retune_calls=[call])
    monkeypatch.delenv("CSDR_AMD_SEED_HOST", raising=False)
    y, st, yt, stt, win = run_pair(gpu, u8, np.array(rates0, f32), taps, sizes, retunes)
    check_stats(st, m, regrowths=0)
    assert st["takeovers"] >= 2 and st["dirty"] == 1
    monkeypatch.setenv("CSDR_AMD_SEED_HOST", "0")
    yd = gpu.ddc_u8(u8, np.array(rates0, f32), D, taps, block=sizes, retunes=retunes, max_block=MAXB)
    check_stats(gpu.ddc_seed_stats, m, regrowths=0)
    assert np.array_equal(y.view(np.uint32), yt.view(np.uint32)), "host chain: small tables and the twin differ first at output %d" % int(np.argmax((y != yt).any(axis=0)))
    assert np.array_equal(y.view(np.uint32), yd.view(np.uint32)), "host and device chain differ first at output %d" % int(np.argmax((y != yd).any(axis=0)))
    check_ddc_vs_oracle(port, y, u8, plans, taps, "host chain S=%d" % S, win)


def test_nfm_chain_with_rates(gpu, port):
    """The NFM chain object with a rate per channel through 60 calls of 4 chunks: s16 +-1 LSB against the oracle's eight stages, bit for bit against the twin."""
    S, sizes = 3, [4 * CH] * 60
    n = sum(sizes)
    rates = np.array([-0.05, 0.11, 0.25], f32)
    u8 = np.stack([nfm_signal_u8(3600 + s, n, offset=-float(rates[s])) for s in range(S)])
    nfm_taps = gpu.nfm_taps(48000)
    pcm, af = gpu.nfm_chain(u8, rates, block=sizes, max_block=MAXB)
    st, inst = gpu.ddc_seed_stats, set(gpu.ddc_instances)
    assert inst == {"k_ddc_mfma<13,2,true,true> whole"}, inst
    pcmt, aft = gpu.nfm_chain(u8, rates, block=sizes, max_block=n)
    assert set(gpu.ddc_instances) == inst and gpu.ddc_seed_stats["takeovers"] == 0
    check_stats(st, SeedModel.run(sizes), regrowths=0)
    assert st["takeovers"] >= 1
    assert np.array_equal(pcm, pcmt) and np.array_equal(af.view(np.uint32), aft.view(np.uint32))
    worst = 0
    for s in range(S):
        ps, _ = port.nfm_chain(u8[s], float(rates[s]), nfm_taps, D, 0.005, 1024)
        k = min(ps.size, pcm.shape[1])
        assert k >= ps.size - 2048 and k >= 3 * 1024                 # (fastagc's two-block latency: whole AGC blocks only)
        worst = max(worst, int(vc.s16_diff(pcm[s, :k], ps[:k]).max()))
        assert vc.s16_diff(pcm[s, :k], ps[:k]).max() <= 1, "channel %d" % s
    print("ORACLE nfm chain: worst s16 difference %d" % worst)


def test_wfm_chain_with_rates(gpu, port):
    """The WFM chain object with a rate per stream through 60 calls of 4 chunks.  k_wfm_mfma_seq takes every call that yields audio (wfm_mfma_launch has no
    smaller-block fallback: 4096 samples are 20 tiles in one column); takeovers in front of calls 23 and 46, stream 1 retuned in front of call 30.  Equal call
    sizes in both runs mean equal columns: the twin is held to 0 LSB."""
    S, sizes, call = 3, [4 * CH] * 60, 30
    n = sum(sizes); pos = call * 4 * CH
    wt = port.firdes_lowpass_f(79, 0.05)
    rates = np.array(WRATES[:S], f32)
    plans = [[(0, float(rates[0]))], [(0, float(rates[1])), (pos, -0.3)], [(0, float(rates[2]))]]
    u8 = np.stack([moving_signal(3700 + 10 * s, plans[s], n, wfm_signal_u8) for s in range(S)])
    retunes = {call: [(1, -0.3)]}
    a, af = gpu.wfm_chain(u8, rates, 10, wt, block=sizes, retunes=retunes, max_block=MAXB)
    st = gpu.wfm_seed_stats
    assert gpu.last_wfm_kernel == "k_wfm_mfma_seq"
    b, bf = gpu.wfm_chain(u8, rates, 10, wt, block=sizes, retunes=retunes, max_block=n)
    assert gpu.last_wfm_kernel == "k_wfm_mfma_seq" and gpu.wfm_seed_stats["takeovers"] == 0
    m = SeedModel.run(sizes, retune_calls=[call])
    check_stats(st, m, regrowths=0)
    assert st["takeovers"] >= 1 and st["dirty"] == 1 and m.stats["takeover_calls"][0] < call
    assert a.shape == b.shape and vc.s16_diff(a, b).max() == 0 and np.array_equal(af.view(np.uint32), bf.view(np.uint32))
    worst = 0
    for s in range(S):
        if len(plans[s]) == 1:
            want, _ = port.wfm_chain(u8[s], float(rates[s]), 10, wt)
        else:
            xf = port.convert_u8_f(u8[s]).view(c64)
            s1, ph = port.shift_addition_cc(xf[:pos], float(rates[s]))
            s2, _ = port.shift_addition_cc(xf[pos:], -0.3, phase=ph)
            dem, _ = port.fmdemod_quadri_cf(port.fir_decimate_cc(np.concatenate([s1, s2]), 10, wt))
            want = port.convert_f_s16(port.deemphasis_wfm_ff(dem[10::5], 50e-6, 48000)[0])      # fractional_decimator_ff 5 == x[5 k + 10] (exact at an integer rate)
        k = min(want.size, a.shape[1])
        assert k >= want.size - 4 and a.shape[1] - k <= 2
        worst = max(worst, int(vc.s16_diff(a[s, :k], want[:k]).max()))
        assert vc.s16_diff(a[s, :k], want[:k]).max() <= 1, "stream %d: %d" % (s, vc.s16_diff(a[s, :k], want[:k]).max())
    print("ORACLE wfm chain: worst s16 difference %d" % worst)


def test_shared_rate_ddc_table_rebuilt(gpu, port, taps):
    """One rate for all streams: the host builds a table of 16 * (max_block_samples / 1024 + 8) = 192 seeds (and, at this drifting rate, their corrections) and
    rebuilds it from c_prev and phase when a call leaves it: in front of call 47 of 60."""
    S, sizes, rate = 3, [4 * CH] * 60, 0.05
    n = sum(sizes)
    u8 = np.stack([nfm_signal_u8(3800 + s, n, offset=-rate) for s in range(S)])
    y = gpu.ddc_u8(u8, rate, D, taps, block=sizes, max_block=MAXB)
    built, inst = gpu.ddc_seed_stats["tables_built"], set(gpu.ddc_instances)
    assert gpu.ddc_kernels == {"k_ddc_mfma"}
    yt = gpu.ddc_u8(u8, rate, D, taps, block=sizes, max_block=n)
    print("TABLES BUILT ddc shared rate:", built, "twin:", gpu.ddc_seed_stats["tables_built"])
    assert built >= 2 and gpu.ddc_seed_stats["tables_built"] == 1 and set(gpu.ddc_instances) == inst
    assert np.array_equal(y.view(np.uint32), yt.view(np.uint32)), "small table and the twin differ first at output %d" % int(np.argmax((y != yt).any(axis=0)))
    first = list(gpu.ddc_call_out) + [y.shape[1]]
    check_ddc_vs_oracle(port, y, u8, [[(0, rate)]] * S, taps, "shared rate", [(first[47], first[49])])


def test_shared_rate_wfm_table_rebuilt(gpu, port):
    """The same for the WFM chain object with one rate: its table is rebuilt in front of call 47."""
    S, sizes, rate = 3, [4 * CH] * 60, -0.085
    n = sum(sizes)
    wt = port.firdes_lowpass_f(79, 0.05)
    u8 = np.stack([wfm_signal_u8(3900 + s, n, offset=-rate) for s in range(S)])
    a, af = gpu.wfm_chain(u8, rate, 10, wt, block=sizes, max_block=MAXB)
    built = gpu.wfm_seed_stats["tables_built"]
    assert gpu.last_wfm_kernel == "k_wfm_mfma_seq"
    b, bf = gpu.wfm_chain(u8, rate, 10, wt, block=sizes, max_block=n)
    print("TABLES BUILT wfm shared rate:", built, "twin:", gpu.wfm_seed_stats["tables_built"])
    assert built >= 2 and gpu.wfm_seed_stats["tables_built"] == 1 and gpu.last_wfm_kernel == "k_wfm_mfma_seq"
    assert a.shape == b.shape and vc.s16_diff(a, b).max() == 0 and np.array_equal(af.view(np.uint32), bf.view(np.uint32))
    worst = 0
    for s in range(S):
        want, wf = port.wfm_chain(u8[s], rate, 10, wt)
        k = min(want.size, a.shape[1])
        assert k >= want.size - 4 and a.shape[1] - k <= 2
        worst = max(worst, int(vc.s16_diff(a[s, :k], want[:k]).max()))
        assert vc.s16_diff(a[s, :k], want[:k]).max() <= 1 and relrms(af[s, :k], wf[:k]) <= TOL, "stream %d" % s
    print("ORACLE wfm shared rate: worst s16 difference %d" % worst)


def test_shared_rate_objects_have_no_seed_stats(gpu, taps):
    """csdr_amd_ddc_seed_stats / csdr_amd_wfm_seed_stats on an object that shares one rate: a clean error, no counters"""
    import ctypes as C
    Lb = gpu.L
    out = (C.c_long * 5)(*([-7] * 5))
    t = np.ascontiguousarray(taps, f32)
    d = Lb.csdr_amd_ddc_create(gpu.h, 1, 0.11, D, t.ctypes.data_as(C.c_void_p), t.size, MAXB)
    assert d
    try:
        assert Lb.csdr_amd_ddc_seed_stats(d, out) < 0 and b"shares one rate" in Lb.csdr_amd_last_error() and list(out) == [-7] * 5
        assert Lb.csdr_amd_ddc_tables_built(d) == 0
    finally:
        Lb.csdr_amd_ddc_destroy(d)
    wt = np.ascontiguousarray(t[:79])
    w = Lb.csdr_amd_wfm_create(gpu.h, 1, 0.11, 10, wt.ctypes.data_as(C.c_void_p), wt.size, 5, 50e-6, 48000, MAXB)
    assert w
    try:
        assert Lb.csdr_amd_wfm_seed_stats(w, out) < 0 and b"shares one rate" in Lb.csdr_amd_last_error() and list(out) == [-7] * 5
        assert Lb.csdr_amd_wfm_tables_built(w) == 0
    finally:
        Lb.csdr_amd_wfm_destroy(w)
