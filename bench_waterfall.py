#!/usr/bin/env python3
"""bench_waterfall.py -- the waterfall of a web receiver, batched: `convert_u8_f | fft_cc 4096 2867 | logaveragepower_cf A 4096 93 | fft_exchange_sides_ff 4096 |
compress_fft_adpcm_f_u8 4096` (csdr.c:1569-1768) for `--streams` 2.4 MS/s streams per call through one csdr_amd_waterfall object (waterfall.hip).

One step = one csdr_amd_waterfall_process call over all streams (`--block` samples each, inputs resident in HBM; the object's overlap, skip and partial
row carry over from step to step).  Roofline: the larger of two bounds, algorithmic bytes (input + rows) / 8 TB/s and 5 N log2 N flops per frame / 157.3 TF.

    python bench_waterfall.py [--gpus 1] [--steps K] [--warmup W] [--streams 1024] [--block 2400256] [--fft 4096] [--every 2867] [--avg 93]
                              [--in u8|cf32] [--out adpcm|db] [--generic] [--verify] [--no-cpu-baseline]
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import bench_common as bc  # noqa: E402

FLOPS_PEAK = 157.3e12                     # fp32 vector peak of the guide's spec numbers (flop/s)
REF_CSDR = os.path.join(ROOT, "oracle", "_ref", "csdr")


def cpu_reference(args, seconds_of_input=1.0):
    """the reference pipeline from oracle/_ref/csdr on one stream: complex samples per second of wall time"""
    if not os.path.exists(REF_CSDR):
        return None
    import numpy as np
    n = int(2.4e6 * seconds_of_input)
    rng = np.random.default_rng(7)
    if args.in_format == "u8":
        data = rng.integers(0, 256, 2 * n, dtype=np.uint8).tobytes(); head = "%s convert_u8_f | " % REF_CSDR
    else:
        data = (rng.standard_normal(2 * n) * 0.3).astype(np.float32).tobytes(); head = ""
    tail = " | %s compress_fft_adpcm_f_u8 %d" % (REF_CSDR, args.fft) if args.out == "adpcm" else ""
    cmd = head + "%s fft_cc %d %d HAMMING | %s logaveragepower_cf -70 %d %d | %s fft_exchange_sides_ff %d%s" % (
        REF_CSDR, args.fft, args.every, REF_CSDR, args.fft, args.avg, REF_CSDR, args.fft, tail)
    t0 = time.perf_counter()
    r = subprocess.run(["bash", "-c", cmd], input=data, capture_output=True, timeout=600)
    wall = time.perf_counter() - t0
    ldd = subprocess.run(["ldd", REF_CSDR], capture_output=True, text=True).stdout
    fft_lib = "fftw3" if "fftw3" in ldd else ("the FFTW-API shim of oracle/ (a plain radix-2 FFT)" if r.returncode == 0 else "unknown")
    return {"value": round(n / wall / 1e6, 2), "unit": "complex MS/s", "streams": 1, "fft_provider": fft_lib, "pipeline": cmd.replace(REF_CSDR, "csdr"),
            "note": "one stream through the reference's process-per-stage pipeline; a stated baseline, not a credit"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--block", type=int, default=2400256)
    ap.add_argument("--fft", type=int, default=4096)
    ap.add_argument("--every", type=int, default=2867)
    ap.add_argument("--avg", type=int, default=93)
    ap.add_argument("--in", dest="in_format", choices=["u8", "cf32"], default="u8")
    ap.add_argument("--out", choices=["adpcm", "db"], default="adpcm")
    ap.add_argument("--generic", action="store_true", help="force the framing + hipFFT + post-kernel composition (A/B)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--verify", action="store_true")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_waterfall.py measures one GPU (--gpus 1)")

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_waterfall.py needs an MI355X; there is no CPU fallback")
    import csdr_amd
    ctx = csdr_amd.Context(0)
    S, T, N = args.streams, args.block, args.fft
    g = torch.Generator(device="cuda"); g.manual_seed(4321)
    if args.in_format == "u8":
        x = torch.randint(0, 256, (S, 2 * T), dtype=torch.uint8, device="cuda", generator=g)
        in_bytes = 2
    else:
        x = (torch.rand((S, 2 * T), device="cuda", generator=g) * 2 - 1).contiguous()
        in_bytes = 8
    w = ctx.waterfall(N, args.every, args.avg, -70.0, "HAMMING", args.in_format, args.out, S, T)
    if args.generic:
        w.force_generic()
    max_rows = w.max_rows(T)
    opitch = (max_rows * w.row_bytes + 255) // 256 * 256
    y = torch.empty((S, opitch), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def step():
        return w.process_dev(x.data_ptr(), T, T, y.data_ptr(), opitch)

    w.reset()
    first_rows = step()                                               # from the reset state: the rows --verify checks
    ctx.sync()
    first = y[:, :first_rows * w.row_bytes].clone() if args.verify else None
    for _ in range(args.warmup):
        step()
    ctx.sync(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.timer_start()
    rows_total = 0
    for _ in range(args.steps):
        rows_total += step()
    ev_ms = ctx.timer_stop_ms()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    frames = S * (T / args.every)                                     # per step (sustained)
    flops = 5.0 * N * math.log2(N) * frames
    rows_step = rows_total / args.steps
    algo = S * T * in_bytes + S * rows_step * w.row_bytes
    k_ms = ev_ms / args.steps
    t_bytes, t_flops = algo / bc.HBM_PEAK_GBS / 1e9, flops / FLOPS_PEAK
    bind = "flops" if t_flops >= t_bytes else "hbm"
    roof_s = max(t_bytes, t_flops)
    res = {"metric": "complex MS/s in, waterfall fft %d every %d avg %d (%s in, %s out) @2.4 MS/s x N streams" % (N, args.every, args.avg, args.in_format, args.out),
           "value": round(S * T * args.steps / wall / 1e6, 1), "unit": "complex MS/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(wall / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": "convert_u8_f | fft_cc | logaveragepower_cf | fft_exchange_sides_ff | compress_fft_adpcm_f_u8, batched" if args.in_format == "u8"
                      else "fft_cc | logaveragepower_cf | fft_exchange_sides_ff, batched", "streams_per_gpu": S, "block_samples_per_stream": T, "fft_size": N,
                      "every_n": args.every, "avgnumber": args.avg, "in": args.in_format, "out": args.out, "path": "generic" if args.generic else "default",
                      "stream_rate_sps": 2400000},
           "roofline": {"bound": bind, "kernel": w.kernel_name(), "kernel_avg_ms": round(k_ms, 4),
                        "bound_hbm_ms": round(t_bytes * 1e3, 4), "bound_flops_ms": round(t_flops * 1e3, 4),
                        "algorithmic_bytes_per_step": algo, "flops_per_step": flops, "hbm_peak_GBs": bc.HBM_PEAK_GBS, "flops_peak": FLOPS_PEAK,
                        "frac": round(roof_s / (k_ms * 1e-3), 4)},
           "rows_per_step_per_stream": rows_step}
    if args.verify:
        import oracle
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import verify_configs as vc
        import waterfall_model as wm
        port = oracle.port()
        win = port.precalculate_window(N, "HAMMING")
        picked = vc.pick_rows(S, want=3)
        ok, worst, worst_db, worst_codes = first_rows > 0, 0.0, 0.0, 0.0
        for s in picked:
            xs = x[s].cpu().numpy()
            xs = xs if args.in_format == "u8" else xs.view(np.float32).view(np.complex64)
            want_p, want_db = wm.rows(xs, args.in_format, N, args.every, win, args.avg, -70.0)
            want_p, want_db = want_p[:first_rows], want_db[:first_rows]
            got = first[s].cpu().numpy()
            if args.out == "db":
                db = got.view(np.float32).reshape(first_rows, N)
                p = 10.0 ** ((db.astype(np.float64) - float(wm.add_db_eff(-70.0, args.avg))) / 10)
                worst = max(worst, max(wm.relrms(p[r], want_p[r]) for r in range(first_rows)))
                worst_db = max(worst_db, wm.db_gate(db, want_db))
            else:
                want = np.frombuffer(port.compress_fft_adpcm_f_u8(want_db.astype(np.float32).ravel(), N), np.uint8)
                a = got[:want.size]
                worst_codes = max(worst_codes, float(np.mean(np.stack([a & 15, a >> 4]) != np.stack([want & 15, want >> 4]))))
        if args.out == "db":
            ok = ok and worst <= 1e-5 and worst_db <= 0.01
            res["verify"] = {"streams": picked, "rows": first_rows, "max_rel_rms_power": worst, "max_db_err_60dB": worst_db, "tolerance": [1e-5, 0.01], "ok": bool(ok)}
        else:
            ok = ok and worst_codes < 0.02
            res["verify"] = {"streams": picked, "rows": first_rows, "adpcm_code_mismatch": worst_codes, "tolerance": 0.02, "ok": bool(ok)}
    if not args.no_cpu_baseline:
        res["cpu_baseline"] = cpu_reference(args)
    print(json.dumps(res), flush=True)
    w.close()
    ctx.close()
    if args.verify and not res["verify"]["ok"]:
        raise SystemExit("bench_waterfall.py --verify failed")


if __name__ == "__main__":
    main()
