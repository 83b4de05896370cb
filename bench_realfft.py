#!/usr/bin/env python3
"""bench_realfft.py -- the audio spectrum of N demodulated channels, batched: `[convert_s16_f |] fft_fc M E | logaveragepower_cf A M AVG | compress_fft_adpcm_f_u8 M`
(csdr.c:3414-3498, 1663-1695, 1745-1768) for `--streams` 48 kS/s real streams per call through one csdr_amd_waterfall object with a real in_format
(waterfall.hip, k_wf_onepass_real).

Default shape: 1024 streams, M = 1024 output bins (frames of 2048 samples), a frame every 1600 samples (30 per second), 3 frames per row, one second of
audio (48000 samples) per stream and step, ADPCM rows; f32 and s16 input are both measured.  One step = one csdr_amd_waterfall_process call over all
streams (inputs resident in HBM; overlap, skip and partial row carry over from step to step).

Yardstick: what the library offered for the same rows before the real formats existed -- the complex waterfall at fft_size 2M on the zero-imaginary
widening of the same samples (cf32 input; half of every row is then thrown away).  The widening itself is not charged to it.  The two objects run in
the same process, alternating `--repeats` times; the JSON holds both medians, their ratio, the spread (min .. max over the repeats) and the shape, for
every size of `--sizes` (the first size is the headline; each later size runs at streams / (M / first M) so that a step holds the same bytes).
Roofline, as bench_waterfall.py counts it: algorithmic bytes (input read once + rows written) / 8 TB/s against the event-timed step.

    python bench_realfft.py [--gpus 1] [--steps K] [--warmup W] [--streams 1024] [--seconds 1.0] [--sizes 1024,8192] [--every-per-m 1.5625] [--avg 3]
                            [--out adpcm|db] [--repeats 5] [--generic] [--verify]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import bench_common as bc  # noqa: E402

RATE = 48000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=1.0, help="audio per stream and step at the first size")
    ap.add_argument("--sizes", default="1024,8192", help="output bins M, comma separated; the first is the headline shape")
    ap.add_argument("--every-per-m", type=float, default=1.5625, help="every_n / M (1.5625: 1600 samples at M = 1024)")
    ap.add_argument("--avg", type=int, default=3)
    ap.add_argument("--out", choices=["adpcm", "db"], default="adpcm")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--generic", action="store_true", help="force the framing + hipFFT + post-kernel composition on the real objects (A/B)")
    ap.add_argument("--verify", action="store_true")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_realfft.py measures one GPU (--gpus 1)")
    sizes = [int(v) for v in args.sizes.split(",")]

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_realfft.py needs an MI355X; there is no CPU fallback")
    import csdr_amd
    ctx = csdr_amd.Context(0)
    g = torch.Generator(device="cuda"); g.manual_seed(4321)
    per_size, verify = [], {"ok": True, "cases": []}
    for M in sizes:
        scale = M / sizes[0]
        S = max(1, int(round(args.streams / scale)))
        T = int(round(args.seconds * RATE * scale))
        every = int(round(args.every_per_m * M))
        xf = (torch.rand((S, T), device="cuda", generator=g) * 2 - 1).contiguous()
        xs = torch.round(xf * 32767).to(torch.int16).contiguous()
        xc = torch.stack([xf, torch.zeros_like(xf)], dim=2).contiguous()                  # the zero-imaginary widening, [S, T, 2] floats
        objs = {"f32": (ctx.waterfall(M, every, args.avg, -70.0, "HAMMING", "f32", args.out, S, T), xf, 4),
                "s16": (ctx.waterfall(M, every, args.avg, -70.0, "HAMMING", "s16", args.out, S, T), xs, 2),
                "complex_2m": (ctx.waterfall(2 * M, every, args.avg, -70.0, "HAMMING", "cf32", args.out, S, T), xc, 8)}
        if args.generic:
            objs["f32"][0].force_generic(); objs["s16"][0].force_generic()
        opitch = max((w.max_rows(T) * w.row_bytes + 255) // 256 * 256 for w, _, _ in objs.values())
        y = torch.empty((S, opitch), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        first = {}
        for name, (w, x, _) in objs.items():
            w.reset()
            rows = w.process_dev(x.data_ptr(), T, T, y.data_ptr(), opitch)               # from the reset state: the rows --verify checks
            ctx.sync()
            first[name] = (rows, y[:, :rows * w.row_bytes].clone() if args.verify and name != "complex_2m" else None)
            for _ in range(args.warmup):
                w.process_dev(x.data_ptr(), T, T, y.data_ptr(), opitch)
        ctx.sync(); torch.cuda.synchronize()
        ms = {name: [] for name in objs}
        rows_step = {}
        for _ in range(args.repeats):
            for name, (w, x, _) in objs.items():                                         # alternating: a drift of the machine hits every object alike
                ctx.timer_start()
                rows_total = 0
                for _ in range(args.steps):
                    rows_total += w.process_dev(x.data_ptr(), T, T, y.data_ptr(), opitch)
                ms[name].append(ctx.timer_stop_ms() / args.steps)
                rows_step[name] = rows_total / args.steps
        entry = {"fft_out_size": M, "streams": S, "block_samples_per_stream": T, "every_n": every, "avgnumber": args.avg, "out": args.out,
                 "path": "generic" if args.generic else "default"}
        for name, (w, x, eb) in objs.items():
            med = statistics.median(ms[name])
            algo = S * T * eb + S * rows_step[name] * w.row_bytes
            entry[name] = {"kernel": w.kernel_name(), "ms_per_step": round(med, 4), "spread_ms": [round(min(ms[name]), 4), round(max(ms[name]), 4)],
                           "rows_per_step_per_stream": rows_step[name], "algorithmic_bytes_per_step": algo,
                           "hbm_frac": round(algo / bc.HBM_PEAK_GBS / 1e9 / (med * 1e-3), 4)}
        for name in ("f32", "s16"):
            entry[name]["speedup_vs_complex_2m"] = round(entry["complex_2m"]["ms_per_step"] / entry[name]["ms_per_step"], 3)
            # ahead beyond the spread: the slowest repeat of the real form against the fastest of the yardstick
            entry[name]["ahead_beyond_spread"] = bool(entry[name]["spread_ms"][1] < entry["complex_2m"]["spread_ms"][0])
        per_size.append(entry)
        if args.verify:
            import oracle
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import verify_configs as vc
            import realfft_model as rm
            port = oracle.port()
            win = port.precalculate_window(2 * M, "HAMMING")
            for name in ("f32", "s16"):
                rows, got_all = first[name]
                ok, worst, worst_db, worst_codes = rows > 0, 0.0, 0.0, 0.0
                picked = vc.pick_rows(S, want=3)
                for s in picked:
                    want_p, want_db = rm.rows(objs[name][1][s].cpu().numpy(), name, M, every, win, args.avg, -70.0)
                    ok = ok and want_p.shape[0] == rows
                    got = got_all[s].cpu().numpy()
                    if args.out == "db":
                        db = got.view(np.float32).reshape(rows, M)
                        p = 10.0 ** ((db.astype(np.float64) - float(rm.add_db_eff(-70.0, args.avg))) / 10)
                        worst = max(worst, max(rm.relrms(p[r], want_p[r]) for r in range(rows)))
                        worst_db = max(worst_db, rm.db_gate(db, want_db))
                    else:
                        want = np.frombuffer(port.compress_fft_adpcm_f_u8(want_db.astype(np.float32).ravel(), M), np.uint8)
                        a = got[:want.size]
                        worst_codes = max(worst_codes, float(np.mean(np.stack([a & 15, a >> 4]) != np.stack([want & 15, want >> 4]))))
                if args.out == "db":
                    ok = ok and worst <= 1e-5 and worst_db <= 0.01
                    case = {"fft_out_size": M, "in": name, "streams": picked, "rows": rows, "max_rel_rms_power": worst, "max_db_err_60dB": worst_db, "tolerance": [1e-5, 0.01]}
                else:
                    ok = ok and worst_codes < 0.02
                    case = {"fft_out_size": M, "in": name, "streams": picked, "rows": rows, "adpcm_code_mismatch": worst_codes, "tolerance": 0.02}
                case["ok"] = bool(ok)
                verify["cases"].append(case); verify["ok"] = bool(verify["ok"] and ok)
        for w, _, _ in objs.values():
            w.close()
        del xf, xs, xc, y
    head = per_size[0]
    res = {"metric": "real MS/s in, spectrum rows fft_out %d every %d avg %d (f32 in, %s out) @48 kS/s x N streams" % (head["fft_out_size"], head["every_n"], args.avg, args.out),
           "value": round(head["streams"] * head["block_samples_per_stream"] / (head["f32"]["ms_per_step"] * 1e-3) / 1e6, 1), "unit": "real MS/s", "n_gpus": 1,
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "ms_per_step": head["f32"]["ms_per_step"], "higher_is_better": True, "scaling": "weak",
           "vs_baseline": head["f32"]["speedup_vs_complex_2m"], "dtype": "f32", "data": "synthetic",
           "config": {"workload": "[convert_s16_f |] fft_fc | logaveragepower_cf [| compress_fft_adpcm_f_u8], batched; yardstick: the complex waterfall at 2M on the "
                                  "zero-imaginary widening (cf32), same process, alternating", "stream_rate_sps": RATE},
           "roofline": {"bound": "hbm", "kernel": head["f32"]["kernel"], "kernel_avg_ms": head["f32"]["ms_per_step"], "hbm_peak_GBs": bc.HBM_PEAK_GBS,
                        "algorithmic_bytes_per_step": head["f32"]["algorithmic_bytes_per_step"], "frac": head["f32"]["hbm_frac"]},
           "sizes": per_size}
    if args.verify:
        res["verify"] = verify
    print(json.dumps(res), flush=True)
    ctx.close()
    if args.verify and not verify["ok"]:
        raise SystemExit("bench_realfft.py --verify failed")


if __name__ == "__main__":
    main()
