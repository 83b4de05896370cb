#!/usr/bin/env python3
"""bench_resampler.py -- the FIR resamplers, batched: rational_resampler_ff I D (libcsdr.c:607-640) or, with --complex, fir_interpolate_cc I (libcsdr.c:579-605)
for `--streams` streams per call through one csdr_amd_resampler / csdr_amd_interp object (resampler.hip).

One step = one process call over all streams (`--block` samples each, inputs resident in HBM; each stream's history carries over from step to step).
Roofline: the larger of two bounds, algorithmic bytes (input + output) / 8 TB/s and 2 flops per multiply-add / 157.3 TF.

    python bench_resampler.py [--gpus 1] [--steps K] [--warmup W] [--streams 1024] [--block N] [--interp 147] [--decim 160] [--tbw T] [--complex]
                              [--generic] [--verify] [--no-cpu-baseline]
defaults: 147/160 (48 kHz -> 44.1 kHz), tbw 0.001 (3999 taps), 1 048 576 floats per stream; --complex: 262 144 complex samples per stream, tbw 0.05.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import bench_common as bc  # noqa: E402

FLOPS_PEAK = 157.3e12                     # fp32 vector peak (flop/s)
REF_CSDR = os.path.join(ROOT, "oracle", "_ref", "csdr")


def cpu_reference(args, n=1 << 21):
    """the reference command from oracle/_ref/csdr on one stream: input samples per second of wall time"""
    if not os.path.exists(REF_CSDR):
        return None
    import numpy as np
    rng = np.random.default_rng(7)
    if args.complex:
        data = rng.uniform(-1, 1, 2 * n).astype(np.float32).tobytes(); cmd = [REF_CSDR, "fir_interpolate_cc", str(args.interp), str(args.tbw)]
    else:
        data = rng.uniform(-1, 1, n).astype(np.float32).tobytes(); cmd = [REF_CSDR, "rational_resampler_ff", str(args.interp), str(args.decim), str(args.tbw)]
    t0 = time.perf_counter()
    subprocess.run(cmd, input=data, capture_output=True, timeout=600)
    wall = time.perf_counter() - t0
    return {"value": round(n / wall / 1e6, 2), "unit": "MS/s in", "streams": 1, "command": " ".join(["csdr"] + cmd[1:]),
            "note": "one stream through the reference CLI; a stated baseline, not a credit"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--block", type=int, default=None)
    ap.add_argument("--interp", type=int, default=None)
    ap.add_argument("--decim", type=int, default=None)
    ap.add_argument("--tbw", type=float, default=None)
    ap.add_argument("--complex", action="store_true", help="fir_interpolate_cc instead of rational_resampler_ff")
    ap.add_argument("--generic", action="store_true", help="force the generic kernel (A/B)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--verify", action="store_true")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_resampler.py measures one GPU (--gpus 1)")
    if args.complex:
        args.interp = args.interp or 4; args.decim = 1; args.tbw = args.tbw or 0.05; args.block = args.block or 262144
    else:
        args.interp = args.interp or 147; args.decim = args.decim or 160; args.block = args.block or 1 << 20
        args.tbw = args.tbw or (0.001 if (args.interp, args.decim) == (147, 160) else 0.05)

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_resampler.py needs an MI355X; there is no CPU fallback")
    import csdr_amd
    ctx = csdr_amd.Context(0)
    S, N, I, D = args.streams, args.block, args.interp, args.decim
    T = ctx.firdes_filter_len(args.tbw)
    g = torch.Generator(device="cuda"); g.manual_seed(4321)
    eb = 8 if args.complex else 4
    x = (torch.rand((S, N * eb // 4), device="cuda", generator=g) * 2 - 1).contiguous()
    if args.complex:
        obj = ctx.interpolator(I, None, S, args.tbw)
        taps_per_out = sum(max(0, -(-(T - (I - ip)) // I)) for ip in range(I)) / I
    else:
        obj = ctx.resampler(I, D, None, S, args.tbw)
        taps_per_out = float(np.mean([max(0, T - d) // I for d in range(I)]))
    if args.generic:
        obj.force_generic()
    opitch = (obj.max_out(N) + 63) // 64 * 64
    y = torch.empty((S, opitch * eb // 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def step():
        return obj.process_dev(x.data_ptr(), N, N, y.data_ptr(), opitch)

    obj.reset()
    first_n = step()                                                  # from the reset state: the outputs --verify checks
    ctx.sync()
    first = y.clone() if args.verify else None
    for _ in range(args.warmup):
        step()
    ctx.sync(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.timer_start()
    out_total = 0
    for _ in range(args.steps):
        out_total += step()
    ev_ms = ctx.timer_stop_ms()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    out_step = out_total / args.steps
    comps = 2 if args.complex else 1
    flops = 2.0 * S * out_step * taps_per_out * comps
    algo = S * N * eb + S * out_step * eb
    k_ms = ev_ms / args.steps
    t_bytes, t_flops = algo / bc.HBM_PEAK_GBS / 1e9, flops / FLOPS_PEAK
    bind = "flops" if t_flops >= t_bytes else "hbm"
    roof_s = max(t_bytes, t_flops)
    name = "fir_interpolate_cc %d" % I if args.complex else "rational_resampler_ff %d %d" % (I, D)
    res = {"metric": "MS/s in, %s (T %d) x N streams" % (name, T),
           "value": round(S * N * args.steps / wall / 1e6, 1), "unit": "MS/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(wall / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": name + ", batched", "streams_per_gpu": S, "block_samples_per_stream": N, "interpolation": I, "decimation": D,
                      "transition_bw": args.tbw, "taps": T, "taps_per_output": round(taps_per_out, 3), "path": "generic" if args.generic else "default"},
           "roofline": {"bound": bind, "kernel": obj.kernel_name(), "kernel_avg_ms": round(k_ms, 4),
                        "bound_hbm_ms": round(t_bytes * 1e3, 4), "bound_flops_ms": round(t_flops * 1e3, 4),
                        "algorithmic_bytes_per_step": algo, "flops_per_step": flops, "hbm_peak_GBs": bc.HBM_PEAK_GBS, "flops_peak": FLOPS_PEAK,
                        "frac": round(roof_s / (k_ms * 1e-3), 4)},
           "outputs_per_step_per_stream": out_step}
    if args.verify:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import resampler_model as rm
        import verify_configs as vc
        picked = vc.pick_rows(S, want=3)
        taps = obj.taps
        worst, ok = 0.0, first_n > 0
        for s in picked:
            xs = x[s].cpu().numpy()
            if args.complex:
                want = rm.fir_interpolate_cc(xs.view(np.complex64), I, taps)
                got = first[s].cpu().numpy().view(np.complex64)[:first_n]
            else:
                want, _ = rm.rational_resampler_ff(xs, I, D, taps)
                got = first[s].cpu().numpy()[:first_n]
            ok = ok and want.size == first_n
            worst = max(worst, rm.relrms(got, want[:first_n]))
        ok = ok and worst <= 1e-5
        res["verify"] = {"streams": picked, "outputs": first_n, "max_rel_rms": worst, "tolerance": 1e-5, "ok": bool(ok)}
    if not args.no_cpu_baseline:
        res["cpu_baseline"] = cpu_reference(args)
    print(json.dumps(res), flush=True)
    obj.close()
    ctx.close()
    if args.verify and not res["verify"]["ok"]:
        raise SystemExit("bench_resampler.py --verify failed")


if __name__ == "__main__":
    main()
