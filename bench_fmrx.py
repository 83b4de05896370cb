#!/usr/bin/env python3
"""bench_fmrx.py -- the NFM receive bank on baseband: fmdemod_quadri_cf | limit_ff | deemphasis_nfm_ff | fastagc_ff | convert_f_s16 for N channels through one
csdr_amd_fmrx object (fmrx.hip).

One step = one process call over all channels (`--block` complex samples each, resident in HBM, every channel's state carried from step to step; s16 out only).
Shape: 4096 channels x 49152 samples (1.024 s at 48 kS/s) of FM baseband (64 distinct rows, repeated).  Reported: the time per step of the one-kernel path
(k_fmrx_front) and of the generic path (csdr_amd_nfm's separate launches, the yardstick: the kernels this object was built from) over `--repeats` runs of
`--steps` steps each (median, min, max), the bytes each path moves per audio sample counted from the code, and the fraction of the HBM bound for 8 bytes in +
2 bytes out per sample at 8 TB/s.  --verify compares sampled channels of the two paths bit for bit (s16 and the float tap) and with one another's next step.

--squelch measures the bank with squelch_and_smeter_cc in front of every channel (csdr_amd_fmrx_create_squelched: block 1024, use_every_nth 1) instead: the fused
path (k_fmrx_power, then k_fmrx_front_sq, which gates the samples as it loads them and skips closed blocks) against the composed path (csdr_amd.Squelch into a
second row buffer, then csdr_amd.FmRx over it: the kernels this path replaces) in the same process on the same input, the two alternating run by run.  Every
block of a row has its own amplitude and the row's level lies between two of its block powers so that --closed-fraction of its blocks close.  Reported: median,
min and max per path, the bytes per input sample counted from the code, and with --verify the sampled channels of the two bit for bit.

One JSON line:
    python bench_fmrx.py [--gpus 1] [--steps K] [--warmup W] [--repeats R] [--channels 4096] [--block 49152] [--verify] [--json-out FILE]
                         [--squelch [--closed-fraction 0.5]]
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
# bytes per audio sample, from the kernels' loads and stores (rows that hit in L2 not counted twice):
#   generic  k_nfm_demod_limit 8 in + 3 digit bytes out; k_nfm_deemph_mfma 3 in + 4 out; k_agc_peaks 4 in; k_agc_apply 4 in + 2 out
#   fused    k_fmrx_front 8 in + 4 out (the peaks ride along); k_agc_apply 4 in + 2 out
BYTES_PER_SAMPLE = {"generic": 8 + 3 + 3 + 4 + 4 + 4 + 2, "fused": 8 + 4 + 4 + 2}


def make_rows(S, N):
    import numpy as np
    rows = []
    for r in range(min(DISTINCT, S)):
        rng = np.random.default_rng(100 + r)
        t = np.arange(N)
        msg = np.sin(2 * np.pi * (300 + 40 * r) / 48e3 * t) + 0.3 * rng.uniform(-1, 1, N)
        ph = 2 * np.pi * np.cumsum(5e3 / 48e3 * msg)
        rows.append((0.7 * np.exp(1j * ph) + 0.01 * (rng.normal(size=N) + 1j * rng.normal(size=N))).astype(np.complex64))
    rows = np.stack(rows)
    return np.tile(rows, ((S + rows.shape[0] - 1) // rows.shape[0], 1))[:S]


def run(ctx, x_host, args):
    import numpy as np
    import torch
    import csdr_amd
    S, N = x_host.shape
    x = torch.view_as_real(torch.from_numpy(x_host)).cuda()
    res = {}
    rows = sorted(set(int(v) for v in np.linspace(0, S - 1, SAMPLED)))
    kept = {}
    for name, forced in (("fused", False), ("generic", True)):
        o = csdr_amd.FmRx(ctx, S, max_samples_per_call=N)
        o.force_generic(forced)
        op = o.max_output(N)
        y = torch.empty((S, op), dtype=torch.int16, device="cuda")
        k = {}
        if args.verify:                                                  # two steps with the float tap, sampled rows kept for the comparison below
            f = torch.empty((S, op), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()                                     # (torch's stream is not the context's: nothing of torch's may still be in flight)
            kept[name] = []
            for _ in range(2):
                got = o.process_dev(x.data_ptr(), N, N, y.data_ptr(), f.data_ptr(), op)
                ctx.sync()
                kept[name].append((got, y[rows, :got].cpu().numpy(), f[rows, :got].cpu().numpy().view(np.uint32)))
            del f
            o.reset()

        def step():
            return o.process_dev(x.data_ptr(), N, N, y.data_ptr(), None, op)

        torch.cuda.synchronize()
        first = step()
        for _ in range(args.warmup):
            out = step()
        ctx.sync()
        k["kernel"] = o.kernel_name()
        k["samples_out_first_step"], k["samples_out_per_step"] = first, out if args.warmup else first
        ms = []
        for _ in range(args.repeats):
            ctx.timer_start()
            for _ in range(args.steps):
                step()
            ms.append(ctx.timer_stop_ms() / args.steps)
        ms.sort()
        k["event_ms_per_step"] = round(ms[len(ms) // 2], 4)
        k["event_ms_min"], k["event_ms_max"] = round(ms[0], 4), round(ms[-1], 4)
        k["steps"], k["repeats"] = args.steps, args.repeats
        n_out = k["samples_out_per_step"]
        k["bytes_per_audio_sample"] = BYTES_PER_SAMPLE[name]
        k["GBs_moved"] = round(BYTES_PER_SAMPLE[name] * S * n_out / (k["event_ms_per_step"] * 1e-3) / 1e9, 1)
        k["frac_of_hbm_bound"] = round((8 * S * N + 2 * S * n_out) / bc.HBM_PEAK_GBS / 1e9 / (k["event_ms_per_step"] * 1e-3), 4)
        res[name] = k
        o.close()
        del y
        torch.cuda.empty_cache()
    res["fused_over_generic"] = round(res["fused"]["event_ms_per_step"] / res["generic"]["event_ms_per_step"], 4)
    # the one-kernel path counts as faster only beyond the spread the same runs show
    res["fused_faster_beyond_spread"] = bool(res["fused"]["event_ms_max"] < res["generic"]["event_ms_min"])
    if args.verify:
        ok = all(a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(kept["fused"], kept["generic"]))
        res["verify"] = {"rows": rows, "steps": 2, "ok": bool(ok and kept["fused"][0][0] > 0)}
    return res


SQ_BLOCK = 1024


def squelch_bytes_per_sample(closed):
    """bytes per input sample, from the kernels' loads and stores:
      composed  k_squelch_wave 8 in + 8 out; then the fused FM path, 18: k_fmrx_front 8 in + 4 out, k_agc_apply 4 in + 2 out
      fused     k_fmrx_power 8 in; k_fmrx_front_sq 8 in for the samples of open blocks only + 4 out; k_agc_apply 4 in + 2 out"""
    return {"composed": 16 + 18, "fused": 8 + 8 * (1.0 - closed) + 4 + 4 + 2}


def make_squelch_rows(S, N, closed):
    """make_rows with every block of SQ_BLOCK samples at an amplitude of its own, and per row the level under which `closed` of its blocks close (0: all open)"""
    import numpy as np
    x = make_rows(S, N)
    nb = N // SQ_BLOCK
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
    fused = csdr_amd.FmRx(ctx, S, max_samples_per_call=N, squelch_block=SQ_BLOCK, use_every_nth=1, levels=levels)
    sq = csdr_amd.Squelch(ctx, S, SQ_BLOCK, 1, levels, max_samples_per_call=N)
    rx = csdr_amd.FmRx(ctx, S, max_samples_per_call=N)
    op = fused.max_output(N)
    y = torch.empty((S, op), dtype=torch.int16, device="cuda")
    nb = N // SQ_BLOCK + 1
    flags = torch.empty((S, nb), dtype=torch.uint8, device="cuda")

    def step_fused(f=None, fl=None):
        return fused.process_squelched_dev(x.data_ptr(), N, N, y.data_ptr(), f, op, None, nb, fl)[0]

    def step_composed(f=None):
        k = sq.process_dev(x.data_ptr(), N, N, gated.data_ptr(), N)
        return rx.process_dev(gated.data_ptr(), N, k * SQ_BLOCK, y.data_ptr(), f, op)

    res = {"closed_fraction_asked": args.closed_fraction}
    torch.cuda.synchronize()
    if args.verify:
        f = torch.empty((S, op), dtype=torch.float32, device="cuda")
        kept = {"fused": [], "composed": []}
        for name, step in (("fused", lambda: step_fused(f.data_ptr(), flags.data_ptr())), ("composed", lambda: step_composed(f.data_ptr()))):
            for _ in range(2):
                got = step()
                ctx.sync()
                kept[name].append((got, y[rows, :got].cpu().numpy(), f[rows, :got].cpu().numpy().view(np.uint32)))
        ok = all(a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(kept["fused"], kept["composed"]))
        res["closed_fraction"] = round(1.0 - float(flags[:, :N // SQ_BLOCK].float().mean().item()), 4)
        res["verify"] = {"rows": rows, "steps": 2, "ok": bool(ok and kept["fused"][0][0] > 0 and kept["fused"][1][1].any())}
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
    bps = squelch_bytes_per_sample(res.get("closed_fraction", args.closed_fraction))
    for name in steps:
        v = sorted(ms[name])
        res[name] = {"kernel": (fused if name == "fused" else rx).kernel_name(), "samples_out_per_step": out[name], "event_ms_per_step": round(v[len(v) // 2], 4),
                     "event_ms_min": round(v[0], 4), "event_ms_max": round(v[-1], 4), "steps": args.steps, "repeats": args.repeats,
                     "bytes_per_input_sample": round(bps[name], 2), "GBs_moved": round(bps[name] * S * N / (v[len(v) // 2] * 1e-3) / 1e9, 1)}
    res["composed"]["squelch_kernel"] = sq.kernel_name()
    res["fused_over_composed"] = round(res["fused"]["event_ms_per_step"] / res["composed"]["event_ms_per_step"], 4)
    res["fused_faster_beyond_spread"] = bool(res["fused"]["event_ms_max"] < res["composed"]["event_ms_min"])
    for o in (fused, sq, rx):
        o.close()
    return res


def main_squelch(ctx, args):
    S, N = args.channels, args.block
    x, levels = make_squelch_rows(S, N, args.closed_fraction)
    r = run_squelch(ctx, x, levels, args)
    t = r["fused"]
    res = {"metric": "MS/s in, squelched NFM receive bank on baseband (squelch_and_smeter_cc .. convert_f_s16) x N channels",
           "value": round(S * N / (t["event_ms_per_step"] * 1e-3) / 1e6, 1), "unit": "complex MS/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": t["event_ms_per_step"], "event_ms_per_step": t["event_ms_per_step"], "higher_is_better": True, "scaling": "weak",
           "vs_baseline": round(1.0 / r["fused_over_composed"], 3), "dtype": "complexf -> s16", "data": "generated",
           "config": {"workload": "squelched NFM receive bank on baseband, batched", "channels": S, "block_samples_per_channel": N, "audio_rate": 48000, "agc_block": 1024,
                      "squelch_block": SQ_BLOCK, "use_every_nth": 1, "closed_fraction": args.closed_fraction,
                      "baseline": "csdr_amd.Squelch into a second row buffer, then csdr_amd.FmRx (its one-kernel path), same input, same process, alternating runs",
                      "hbm_peak_GBs": bc.HBM_PEAK_GBS},
           "roofline": {"bound": "hbm", "kernel": t["kernel"], "kernel_avg_ms": t["event_ms_per_step"],
                        "timer": "HIP events on the context's stream around the objects' calls",
                        "frac": round(t["bytes_per_input_sample"] * S * N / bc.HBM_PEAK_GBS / 1e9 / (t["event_ms_per_step"] * 1e-3), 4)},
           "result": r}
    if args.verify:
        res["verify"] = {"ok": r["verify"]["ok"]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5, help="timed runs of --steps steps each: the median is reported, min and max are the spread")
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--block", type=int, default=49152, help="complex samples per channel and step")
    ap.add_argument("--verify", action="store_true")
    ap.add_argument("--json-out", default=None, help="also append the result line to this file")
    ap.add_argument("--squelch", action="store_true", help="measure the squelched bank: the fused path against csdr_amd.Squelch -> csdr_amd.FmRx")
    ap.add_argument("--closed-fraction", type=float, default=0.5, help="--squelch: the share of every row's squelch blocks that close")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_fmrx.py measures one GPU (--gpus 1)")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_fmrx.py needs an MI355X; there is no CPU fallback")
    import csdr_amd
    ctx = csdr_amd.Context(0)
    S, N = args.channels, args.block
    if args.squelch:
        line = json.dumps(main_squelch(ctx, args))
        print(line, flush=True)
        if args.json_out:
            with open(args.json_out, "a") as f:
                f.write(line + "\n")
        ctx.close()
        return
    r = run(ctx, make_rows(S, N), args)
    t = r["fused"]
    res = {"metric": "MS/s in, NFM receive bank on baseband (fmdemod_quadri_cf .. convert_f_s16) x N channels", "value": round(S * N / (t["event_ms_per_step"] * 1e-3) / 1e6, 1),
           "unit": "complex MS/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": t["event_ms_per_step"], "event_ms_per_step": t["event_ms_per_step"],
           "higher_is_better": True, "scaling": "weak", "vs_baseline": round(1.0 / r["fused_over_generic"], 3), "dtype": "complexf -> s16", "data": "generated",
           "config": {"workload": "NFM receive bank on baseband, batched", "channels": S, "block_samples_per_channel": N, "audio_rate": 48000, "agc_block": 1024,
                      "baseline": "the generic path of the same object (csdr_amd_nfm's kernels, separate launches), same buffers, same process", "hbm_peak_GBs": bc.HBM_PEAK_GBS},
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
