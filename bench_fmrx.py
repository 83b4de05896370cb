#!/usr/bin/env python3
"""bench_fmrx.py -- the NFM receive bank on baseband: fmdemod_quadri_cf | limit_ff | deemphasis_nfm_ff | fastagc_ff | convert_f_s16 for N channels through one
csdr_amd_fmrx object (fmrx.hip).

One step = one process call over all channels (`--block` complex samples each, resident in HBM, every channel's state carried from step to step; s16 out only).
Shape: 4096 channels x 49152 samples (1.024 s at 48 kS/s) of FM baseband (64 distinct rows, repeated).  Reported: the time per step of the one-kernel path
(k_fmrx_front) and of the generic path (csdr_amd_nfm's separate launches, the yardstick: the kernels this object was built from) over `--repeats` runs of
`--steps` steps each (median, min, max), the bytes each path moves per audio sample counted from the code, and the fraction of the HBM bound for 8 bytes in +
2 bytes out per sample at 8 TB/s.  --verify compares sampled channels of the two paths bit for bit (s16 and the float tap) and with one another's next step.

One JSON line:
    python bench_fmrx.py [--gpus 1] [--steps K] [--warmup W] [--repeats R] [--channels 4096] [--block 49152] [--verify] [--json-out FILE]
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
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_fmrx.py measures one GPU (--gpus 1)")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_fmrx.py needs an MI355X; there is no CPU fallback")
    import csdr_amd
    ctx = csdr_amd.Context(0)
    S, N = args.channels, args.block
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
