#!/usr/bin/env python3
"""bench_wfmrx.py -- the WFM receive bank on baseband: fmdemod_quadri_cf | fractional_decimator_ff <rate> | deemphasis_wfm_ff | convert_f_s16 for N channels
through one csdr_amd_wfmrx object (wfmrx.hip).

One step = one process call over all channels (`--block` complex samples each, resident in HBM, every channel's state carried from step to step; s16 out only).
Shapes: 4096 and 512 channels x 49152 samples of FM baseband (64 distinct rows, repeated), rates 5 and 5.2083335.  Reported: the time per step of the one-kernel
path (k_wfmrx_front, k_wfmrx_tail) and of the generic path (the stand-alone entry points composed, the yardstick: the kernels this object was built from), measured
alternately in the same process over `--repeats` runs of `--steps` steps each (median, min, max), the bytes each path moves per input sample counted from the
code, and the fraction of the HBM bound for 8 bytes in + 2 / rate bytes out per input sample at 8 TB/s.  --verify compares sampled channels of the two paths bit
for bit (s16 and the float tap) over two steps, and with the oracle's four stages under the test suite's gates.

--squelch measures the bank with squelch_and_smeter_cc in front of every channel (csdr_amd_wfmrx_create_squelched: block 1024, use_every_nth 1) instead: the fused
path (k_fmrx_power, then k_wfmrx_front_sq, which gates the samples as it loads them and does not fetch closed blocks) against the composed path (csdr_amd.Squelch
into a second row buffer, then csdr_amd.WfmRx on its one-kernel path), same input, same process, alternating runs.  --pattern block: every block of a row has its
own amplitude and the row's level lies between two of its block powers so that --closed-fraction of its blocks close; --pattern channel: that share of the
channels is closed throughout and the others are open.  --verify compares sampled channels of the two bit for bit over two steps (s16, float tap), their open
flags with the float64 block powers, and the fused path with the oracle's four stages on the gated rows under the test suite's gates.

One JSON line:
    python bench_wfmrx.py [--gpus 1] [--steps K] [--warmup W] [--repeats R] [--channels 4096] [--block 49152] [--rate 5] [--verify] [--json-out FILE]
                          [--squelch [--closed-fraction 0.5] [--pattern channel|block]]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import bench_common as bc  # noqa: E402

DISTINCT = 64
SAMPLED = 4


def bytes_per_input_sample(rate):
    """from the kernels' loads and stores (rows that hit in L2 not counted twice)
    generic  k_fmdemod 8 in + 4 out; k_fracdec 4 in + 4 / rate out; k_deemph_wfm (4 + 4) / rate; k_from_float (4 + 2) / rate; the copy to the caller's rows (2 + 2) / rate
    fused    k_wfmrx_front 8 in + 4 / rate out; k_wfmrx_tail (4 + 2) / rate"""
    return {"generic": 16 + 18 / rate, "fused": 8 + 10 / rate}


def make_rows(S, N):
    import numpy as np
    rows = []
    for r in range(min(DISTINCT, S)):
        rng = np.random.default_rng(100 + r)
        t = np.arange(N)
        msg = 0.6 * np.sin(2 * np.pi * (0.004 + 0.0003 * r) * t) + 0.4 * np.sin(2 * np.pi * 0.0171 * t + 1.0)
        ph = 2 * np.pi * np.cumsum(0.08 * msg)
        rows.append((0.7 * np.exp(1j * ph) + 0.002 * (rng.normal(size=N) + 1j * rng.normal(size=N))).astype(np.complex64))
    rows = np.stack(rows)
    return np.tile(rows, ((S + rows.shape[0] - 1) // rows.shape[0], 1))[:S]


def oracle_gates(x_row, rate, s16, af):
    """sampled channel against oracle.port()'s four stages: (relrms of the float audio, largest s16 difference, fraction of s16 samples that differ)"""
    import numpy as np
    import oracle
    port = oracle.port()
    dem, _ = port.fmdemod_quadri_cf(x_row)
    a = port.fractional_decimator_ff(dem, rate, 12, None, bufsize=1024)
    e, _ = port.deemphasis_wfm_ff(a, 50e-6, 48000)
    want = port.convert_f_s16(e)
    if e.shape != af.shape:
        return float("inf"), 1 << 16, 1.0
    d = np.abs(s16.astype(np.int32) - want.astype(np.int32))
    return oracle.relrms(af, e), int(d.max()), float((d > 0).mean())


SQ_BLOCK = 1024


def squelch_bytes_per_sample(rate, closed):
    """bytes per input sample, from the kernels' loads and stores:
      composed  k_squelch_wave 8 in + 8 out; then the fused WFM path on the second buffer, 8 + 10 / rate
      fused     k_fmrx_power 8 in; k_wfmrx_front_sq 8 in for the samples of open blocks only + 4 / rate out; k_wfmrx_tail (4 + 2) / rate"""
    return {"composed": 24 + 10 / rate, "fused": 8 + 8 * (1.0 - closed) + 10 / rate}


def make_squelch_rows(S, N, closed, pattern):
    """make_rows and a level per row.  block: every block of SQ_BLOCK samples at an amplitude of its own, the level under which `closed` of the row's blocks
    close (0: all open).  channel: the rows as they are; the first round(closed * S) channels, spread evenly, at a level above every block power, the others 0"""
    import numpy as np
    x = make_rows(S, N)
    nb = N // SQ_BLOCK
    if pattern == "channel":
        c = int(round(closed * S))
        levels = np.zeros(S, np.float32)
        if c:
            levels[np.unique(np.linspace(0, S - 1, c).astype(int))] = 10.0
        return x, levels
    distinct = min(DISTINCT, S)
    levels = np.zeros(distinct, np.float32)
    for r in range(distinct):
        rng = np.random.default_rng(900 + r)
        scale = (0.2 + 0.8 * rng.permutation(nb) / max(nb - 1, 1)).astype(np.float32)     # nb distinct amplitudes: no two block powers close to one another
        x[r::distinct, :nb * SQ_BLOCK] *= np.repeat(scale, SQ_BLOCK)[None, :]
        blocks = x[r, :nb * SQ_BLOCK].reshape(nb, SQ_BLOCK).astype(np.complex128)
        P = np.sort((np.abs(blocks) ** 2).mean(axis=1))
        c = int(round(closed * nb))
        levels[r] = 0.0 if c == 0 else 2 * P[-1] if c >= nb else 0.5 * (P[c - 1] + P[c])
    return x, np.tile(levels, (S + distinct - 1) // distinct)[:S]


def run_squelch(ctx, x_host, levels, args):
    import numpy as np
    import torch
    import csdr_amd
    S, N = x_host.shape
    x = torch.view_as_real(torch.from_numpy(x_host)).cuda()
    gated = torch.empty((S, N, 2), dtype=torch.float32, device="cuda")                      # the composed path's second row buffer
    rows = sorted(set(int(v) for v in np.linspace(0, S - 1, SAMPLED)))
    fused = csdr_amd.WfmRx(ctx, S, rate=args.rate, max_samples_per_call=N, squelch_block=SQ_BLOCK, use_every_nth=1, levels=levels)
    sq = csdr_amd.Squelch(ctx, S, SQ_BLOCK, 1, levels, max_samples_per_call=N)
    rx = csdr_amd.WfmRx(ctx, S, rate=args.rate, max_samples_per_call=N)
    op = fused.max_output(N)
    y = torch.empty((S, op), dtype=torch.int16, device="cuda")
    nb = N // SQ_BLOCK + 1
    flags = torch.empty((S, nb), dtype=torch.uint8, device="cuda")

    def step_fused(f=None, fl=None):
        return fused.process_squelched_dev(x.data_ptr(), N, N, y.data_ptr(), f, op, None, nb, fl)[0]

    def step_composed(f=None):
        k = sq.process_dev(x.data_ptr(), N, N, gated.data_ptr(), N)
        return rx.process_dev(gated.data_ptr(), N, k * SQ_BLOCK, y.data_ptr(), f, op) if k else 0

    res = {"closed_fraction_asked": args.closed_fraction, "pattern": args.pattern}
    torch.cuda.synchronize()
    if args.verify:
        if N % SQ_BLOCK:
            raise SystemExit("--squelch --verify needs --block to be a multiple of %d" % SQ_BLOCK)
        f = torch.empty((S, op), dtype=torch.float32, device="cuda")
        kept = {"fused": [], "composed": []}
        for name, step in (("fused", lambda: step_fused(f.data_ptr(), flags.data_ptr())), ("composed", lambda: step_composed(f.data_ptr()))):
            for _ in range(2):
                got = step()
                ctx.sync()
                kept[name].append((got, y[rows, :got].cpu().numpy(), f[rows, :got].cpu().numpy()))
        same = all(a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)) for a, b in zip(kept["fused"], kept["composed"]))
        fl = flags[:, :N // SQ_BLOCK].cpu().numpy()
        res["closed_fraction"] = round(1.0 - float(fl.mean()), 4)
        figures, flags_ok = [], True
        for i, r in enumerate(rows):                                     # the oracle on the rows gated by the float64 block powers (no block is near its level)
            blocks = x_host[r].reshape(-1, SQ_BLOCK)
            P = (np.abs(blocks.astype(np.complex128)) ** 2).mean(axis=1)
            want_open = (P >= float(levels[r])) | (levels[r] == 0)
            flags_ok = flags_ok and np.array_equal(fl[r].astype(bool), want_open)
            g = (blocks * want_open[:, None]).reshape(-1).astype(np.complex64)
            s16 = np.concatenate([kept["fused"][0][1][i], kept["fused"][1][1][i]])
            af = np.concatenate([kept["fused"][0][2][i], kept["fused"][1][2][i]])
            if want_open.any():
                figures.append(oracle_gates(np.concatenate([g, g]), args.rate, s16, af))
            else:
                figures.append((0.0, 0, 0.0) if not s16.any() and not af.any() else (float("inf"), 1 << 16, 1.0))
        gates = all(rr <= 1e-5 and dmax <= 1 and frac < 0.01 for rr, dmax, frac in figures)
        res["verify"] = {"rows": rows, "steps": 2, "paths_same_bits": bool(same), "flags_ok": bool(flags_ok), "oracle_relrms_max": max(v[0] for v in figures),
                         "oracle_s16_max_diff": max(v[1] for v in figures), "oracle_s16_differing_max": max(v[2] for v in figures),
                         "ok": bool(same and flags_ok and gates and kept["fused"][0][0] > 0)}
        del f
        fused.reset(); sq.reset(); rx.reset()
    steps = {"fused": step_fused, "composed": step_composed}
    ms = {"fused": [], "composed": []}
    out = {}
    for name, step in steps.items():
        for _ in range(1 + args.warmup):
            out[name] = step()
    ctx.sync()
    for _ in range(args.repeats):                                        # the two paths alternate run by run
        for name, step in steps.items():
            ctx.timer_start()
            for _ in range(args.steps):
                step()
            ms[name].append(ctx.timer_stop_ms() / args.steps)
    bps = squelch_bytes_per_sample(args.rate, res.get("closed_fraction", args.closed_fraction))
    for name in steps:
        v = sorted(ms[name])
        res[name] = {"kernel": (fused if name == "fused" else rx).kernel_name(), "samples_out_per_step": out[name], "event_ms_per_step": round(v[len(v) // 2], 4),
                     "event_ms_min": round(v[0], 4), "event_ms_max": round(v[-1], 4), "steps": args.steps, "repeats": args.repeats,
                     "bytes_per_input_sample": round(bps[name], 2), "GBs_moved": round(bps[name] * S * N / (v[len(v) // 2] * 1e-3) / 1e9, 1)}
    res["composed"]["squelch_kernel"] = sq.kernel_name()
    res["fused_over_composed"] = round(res["fused"]["event_ms_per_step"] / res["composed"]["event_ms_per_step"], 4)
    res["fused_faster_beyond_spread"] = bool(res["fused"]["event_ms_max"] < res["composed"]["event_ms_min"])
    res["fused_slower_beyond_spread"] = bool(res["fused"]["event_ms_min"] > res["composed"]["event_ms_max"])
    for o in (fused, sq, rx):
        o.close()
    return res


def main_squelch(ctx, args):
    S, N = args.channels, args.block
    x, levels = make_squelch_rows(S, N, args.closed_fraction, args.pattern)
    r = run_squelch(ctx, x, levels, args)
    t = r["fused"]
    res = {"metric": "MS/s in, squelched WFM receive bank on baseband (squelch_and_smeter_cc .. convert_f_s16) x N channels",
           "value": round(S * N / (t["event_ms_per_step"] * 1e-3) / 1e6, 1), "unit": "complex MS/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": t["event_ms_per_step"], "event_ms_per_step": t["event_ms_per_step"], "higher_is_better": True, "scaling": "weak",
           "vs_baseline": round(1.0 / r["fused_over_composed"], 3), "dtype": "complexf -> s16", "data": "generated",
           "config": {"workload": "squelched WFM receive bank on baseband, batched", "channels": S, "block_samples_per_channel": N, "rate": args.rate, "num_poly_points": 12,
                      "window": 1024, "audio_rate": 48000, "tau": 50e-6, "squelch_block": SQ_BLOCK, "use_every_nth": 1, "closed_fraction": args.closed_fraction,
                      "pattern": args.pattern,
                      "baseline": "csdr_amd.Squelch into a second row buffer, then csdr_amd.WfmRx (its one-kernel path), same input, same process, alternating runs",
                      "hbm_peak_GBs": bc.HBM_PEAK_GBS},
           "roofline": {"bound": "hbm", "kernel": t["kernel"], "kernel_avg_ms": t["event_ms_per_step"],
                        "timer": "HIP events on the context's stream around the objects' calls",
                        "frac": round(t["bytes_per_input_sample"] * S * N / bc.HBM_PEAK_GBS / 1e9 / (t["event_ms_per_step"] * 1e-3), 4)},
           "result": r}
    if args.verify:
        res["verify"] = {"ok": r["verify"]["ok"]}
    return res


def run(ctx, x_host, args):
    import numpy as np
    import torch
    import csdr_amd
    S, N = x_host.shape
    x = torch.view_as_real(torch.from_numpy(x_host)).cuda()
    rows = sorted(set(int(v) for v in np.linspace(0, S - 1, SAMPLED)))
    names = (("fused", False), ("generic", True))
    objs, res, kept = {}, {}, {}
    for name, forced in names:
        objs[name] = csdr_amd.WfmRx(ctx, S, rate=args.rate, max_samples_per_call=N)
        objs[name].force_generic(forced)
    op = objs["fused"].max_output(N)
    y = torch.empty((S, op), dtype=torch.int16, device="cuda")
    if args.verify:                                                      # two steps with the float tap, sampled rows kept for the comparison below
        f = torch.empty((S, op), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()                                         # (torch's stream is not the context's: nothing of torch's may still be in flight)
        for name, _ in names:
            kept[name] = []
            for _ in range(2):
                got = objs[name].process_dev(x.data_ptr(), N, N, y.data_ptr(), f.data_ptr(), op)
                ctx.sync()
                kept[name].append((got, y[rows, :got].cpu().numpy(), f[rows, :got].cpu().numpy()))
            objs[name].reset()
        del f
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in names}
    for name, _ in names:
        o, k = objs[name], {}
        first = o.process_dev(x.data_ptr(), N, N, y.data_ptr(), None, op)
        out = first
        for _ in range(args.warmup):
            out = o.process_dev(x.data_ptr(), N, N, y.data_ptr(), None, op)
        ctx.sync()
        k["kernel"] = o.kernel_name()
        k["samples_out_first_step"], k["samples_out_per_step"] = first, out
        res[name] = k
    for _ in range(args.repeats):                                        # the two paths alternately
        for name, _ in names:
            o = objs[name]
            ctx.timer_start()
            for _ in range(args.steps):
                o.process_dev(x.data_ptr(), N, N, y.data_ptr(), None, op)
            ms[name].append(ctx.timer_stop_ms() / args.steps)
    per = bytes_per_input_sample(args.rate)
    for name, _ in names:
        k, t = res[name], sorted(ms[name])
        k["event_ms_per_step"] = round(t[len(t) // 2], 4)
        k["event_ms_min"], k["event_ms_max"] = round(t[0], 4), round(t[-1], 4)
        k["steps"], k["repeats"] = args.steps, args.repeats
        k["bytes_per_input_sample"] = round(per[name], 3)
        k["GBs_moved"] = round(per[name] * S * N / (k["event_ms_per_step"] * 1e-3) / 1e9, 1)
        k["frac_of_hbm_bound"] = round((8 + 2 / args.rate) * S * N / bc.HBM_PEAK_GBS / 1e9 / (k["event_ms_per_step"] * 1e-3), 4)
        objs[name].close()
    res["fused_over_generic"] = round(res["fused"]["event_ms_per_step"] / res["generic"]["event_ms_per_step"], 4)
    # the one-kernel path counts as faster only beyond the spread the same runs show
    res["fused_faster_beyond_spread"] = bool(res["fused"]["event_ms_max"] < res["generic"]["event_ms_min"])
    if args.verify:
        same = all(a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
                   for a, b in zip(kept["fused"], kept["generic"]))
        figures = []
        for i, r in enumerate(rows):
            s16 = np.concatenate([kept["fused"][0][1][i], kept["fused"][1][1][i]])
            af = np.concatenate([kept["fused"][0][2][i], kept["fused"][1][2][i]])
            figures.append(oracle_gates(np.concatenate([x_host[r], x_host[r]]), args.rate, s16, af))
        gates = all(rr <= 1e-5 and dmax <= 1 and frac < 0.01 for rr, dmax, frac in figures)
        res["verify"] = {"rows": rows, "steps": 2, "paths_same_bits": bool(same), "oracle_relrms_max": max(f[0] for f in figures), "oracle_s16_max_diff": max(f[1] for f in figures),
                         "oracle_s16_differing_max": max(f[2] for f in figures), "ok": bool(same and gates and kept["fused"][0][0] > 0)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5, help="timed runs of --steps steps each per path, alternating: the median is reported, min and max are the spread")
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--block", type=int, default=49152, help="complex samples per channel and step")
    ap.add_argument("--rate", type=float, default=5.0, help="fractional_decimator_ff's rate")
    ap.add_argument("--verify", action="store_true")
    ap.add_argument("--json-out", default=None, help="also append the result line to this file")
    ap.add_argument("--squelch", action="store_true", help="measure the squelched bank: the fused path against csdr_amd.Squelch -> csdr_amd.WfmRx")
    ap.add_argument("--closed-fraction", type=float, default=0.5, help="--squelch: the share of the squelch blocks that close")
    ap.add_argument("--pattern", choices=("channel", "block"), default="block", help="--squelch: closed blocks within every row, or whole channels closed")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_wfmrx.py measures one GPU (--gpus 1)")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_wfmrx.py needs an MI355X; there is no CPU fallback")
    import csdr_amd
    ctx = csdr_amd.Context(0)
    S, N = args.channels, args.block
    if args.squelch:
        res = main_squelch(ctx, args)
        line = json.dumps(res)
        print(line, flush=True)
        if args.json_out:
            with open(args.json_out, "a") as f:
                f.write(line + "\n")
        ctx.close()
        if args.verify and not res["verify"]["ok"]:
            raise SystemExit(1)
        return
    r = run(ctx, make_rows(S, N), args)
    t = r["fused"]
    res = {"metric": "MS/s in, WFM receive bank on baseband (fmdemod_quadri_cf .. convert_f_s16) x N channels", "value": round(S * N / (t["event_ms_per_step"] * 1e-3) / 1e6, 1),
           "unit": "complex MS/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": t["event_ms_per_step"], "event_ms_per_step": t["event_ms_per_step"],
           "higher_is_better": True, "scaling": "weak", "vs_baseline": round(1.0 / r["fused_over_generic"], 3), "dtype": "complexf -> s16", "data": "generated",
           "config": {"workload": "WFM receive bank on baseband, batched", "channels": S, "block_samples_per_channel": N, "rate": args.rate, "num_poly_points": 12, "window": 1024,
                      "audio_rate": 48000, "tau": 50e-6,
                      "baseline": "the generic path of the same object (the stand-alone entry points composed), same input, same process, runs alternating", "hbm_peak_GBs": bc.HBM_PEAK_GBS},
           "roofline": {"bound": "hbm", "kernel": t["kernel"], "kernel_avg_ms": t["event_ms_per_step"],
                        "timer": "HIP events on the context's stream around the object's calls", "frac": t["frac_of_hbm_bound"]},
           "result": r}
    if args.verify:
        res["verify"] = {"ok": r["verify"]["ok"]}
    line = json.dumps(res)
    print(line, flush=True)
    if args.json_out:
        with open(args.json_out, "a") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
