#!/usr/bin/env python3
"""bench_cfir.py -- the complex-tap FIR, batched: apply_fir_cc with each channel's own peak filter (peaks_fir_cc's taps, one peak rate per channel) for
`--channels` channels per call through one csdr_amd_cfir object (cfir.hip).

One step = one process call over all channels (`--block` complex samples each, resident in HBM; every channel's history carries over from step to
step).  The timed shapes are taps_length 101 (the headline), 31 and 255 (`--taps` picks others).
Roofline: 8 T FP32 flops against 16 bytes (8 in, 8 out) per output; the FP32 bound (157.3 TF, the f32 MFMA and VALU peak) binds over the HBM bound
(8 TB/s) whenever 8 T / 157.3e12 > 16 / 8e12, i.e. T > 39.  frac = the larger bound's time over the measured step.
Beside every shape the same run times the stateless csdr_amd_apply_fir_cc (k_cfir_mfma without the history kernel) and csdr_amd_bfsk_demod_cf at the
same shape, alternating: the discriminator does twice the products and stores half the bytes.

    python bench_cfir.py [--gpus 1] [--steps K] [--warmup W] [--channels 4096] [--block 131072] [--taps 101,31,255] [--generic] [--verify]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench_common as bc  # noqa: E402

FP32_PEAK_TFS = 157.3
SAMPLED = 4                      # rows --verify compares
SPAN = 6000                      # outputs at each end of a sampled row


def channel_rates(S):
    """a peak rate per channel, spread over (-0.45, 0.45)"""
    import numpy as np
    return (-0.45 + 0.9 * (np.arange(S) + 0.5) / S).astype(np.float32)


def shape(ctx, x, S, N, T, args):
    import numpy as np
    import torch
    import csdr_amd
    L = ctx.L
    rates = channel_rates(S)
    taps = np.stack([csdr_amd.firdes_peaks_c(T, [r]) for r in rates])
    d_taps = torch.from_numpy(taps.view(np.float32)).cuda()
    obj = ctx.cfir(S, T)
    obj.set_taps(taps)
    if args.generic:
        obj.force_generic()
    y = torch.empty((S, N, 2), dtype=torch.float32, device="cuda")
    yb = torch.empty((S, N), dtype=torch.float32, device="cuda")
    cnt = torch.empty(S, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def step():
        obj.process_dev(x.data_ptr(), N, N, y.data_ptr(), N, cnt.data_ptr())

    def step_stateless():
        ctx.check(L.csdr_amd_apply_fir_cc(ctx.h, x.data_ptr(), y.data_ptr(), S, N, N, N, d_taps.data_ptr(), T, T, int(args.generic)), "apply_fir_cc")

    def step_bfsk():     # one mark / space pair for every stream (the call takes one): channel 0's taps and channel S - 1's
        ctx.check(L.csdr_amd_bfsk_demod_cf(ctx.h, x.data_ptr(), yb.data_ptr(), S, N, N, N, d_taps.data_ptr(), d_taps.data_ptr() + 8 * T * (S - 1), T, int(args.generic)),
                  "bfsk_demod_cf")

    def timed(fn, steps):
        ctx.timer_start()
        for _ in range(steps):
            fn()
        return ctx.timer_stop_ms() / steps

    obj.reset()
    step()                                                                      # from the reset state: the outputs --verify checks
    ctx.sync()
    ver = None
    if args.verify:
        import cfir_model as cm
        c = cnt.cpu().numpy()
        n_out = N - T + 1
        rows = sorted(set(int(v) for v in np.linspace(0, S - 1, SAMPLED)))
        ok = bool(np.all(c == n_out))
        for k in rows:
            xr = x[k].cpu().numpy().view(np.complex64).ravel()
            yr = y[k].cpu().numpy().view(np.complex64).ravel()[:n_out]
            for lo, hi in ((0, min(SPAN, n_out)), (max(0, n_out - SPAN), n_out)):
                seg = xr[lo:hi + T - 1]
                want = cm.cfir32(seg, taps[k])
                ok = ok and bool(np.array_equal(yr[lo:hi].view(np.uint32), want.view(np.uint32)))
                ok = ok and cm.within(yr[lo:hi], cm.cfir64(seg, taps[k]), cm.cfir_gate(seg, taps[k]))
        ver = {"rows": rows, "outputs_per_row_end": SPAN, "counts_ok": bool(np.all(c == n_out)), "bits_equal_model_and_in_gate": ok, "ok": ok}
    for fn in (step, step_stateless, step_bfsk):
        for _ in range(args.warmup):
            fn()
    ctx.sync(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev_ms = timed(step, args.steps)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / args.steps
    rounds = 3                                                                  # the comparison, alternating, in the same run
    per = max(1, args.steps // rounds)
    ms_s, ms_b, ms_o = [], [], []
    for _ in range(rounds):
        ms_s.append(timed(step_stateless, per)); ms_b.append(timed(step_bfsk, per)); ms_o.append(timed(step, per))
    outs = S * N                                                                 # (steady state: every channel has its T - 1 history)
    flops = 8 * T * outs
    t_fp32 = flops / (FP32_PEAK_TFS * 1e12)
    algo = 16 * outs
    t_hbm = algo / bc.HBM_PEAK_GBS / 1e9
    t_bound = max(t_fp32, t_hbm)
    res = {"taps_length": T, "kernel": obj.kernel_name(), "ms_per_step": round(wall * 1e3, 4), "event_ms_per_step": round(ev_ms, 4),
           "MS_per_s": round(outs / wall / 1e6, 1), "bound": "fp32" if t_fp32 >= t_hbm else "hbm", "bound_fp32_ms": round(t_fp32 * 1e3, 4),
           "bound_hbm_ms": round(t_hbm * 1e3, 4), "flops_per_step": flops, "algorithmic_bytes_per_step": algo, "frac": round(t_bound / (ev_ms * 1e-3), 4),
           "frac_of_fp32_bound": round(t_fp32 / (ev_ms * 1e-3), 4),
           "alternating": {"rounds": rounds, "steps_per_round": per, "cfir_object_ms": [round(v, 4) for v in ms_o], "apply_fir_cc_ms": [round(v, 4) for v in ms_s],
                           "bfsk_demod_cf_ms": [round(v, 4) for v in ms_b], "bfsk_kernel": L.csdr_amd_bfsk_last_kernel().decode(),
                           "cfir_over_bfsk": round(min(ms_s) / min(ms_b), 4)}}
    if ver is not None:
        res["verify"] = ver
    obj.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--block", type=int, default=131072)
    ap.add_argument("--taps", default="101,31,255", help="taps_length of every timed shape; the first is the headline")
    ap.add_argument("--generic", action="store_true", help="force k_cfir_generic (one thread per output)")
    ap.add_argument("--verify", action="store_true")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_cfir.py measures one GPU (--gpus 1)")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_cfir.py needs an MI355X; there is no CPU fallback")
    import csdr_amd
    ctx = csdr_amd.Context(0)
    S, N = args.channels, args.block
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    x = torch.randn((S, N, 2), dtype=torch.float32, device="cuda", generator=g)
    shapes = [shape(ctx, x, S, N, int(t), args) for t in args.taps.split(",")]
    head = shapes[0]
    res = {"metric": "MS/s, complex-tap FIR (apply_fir_cc, T %d, taps per channel) x N channels" % head["taps_length"], "value": head["MS_per_s"], "unit": "MS/s",
           "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": head["ms_per_step"], "event_ms_per_step": head["event_ms_per_step"],
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "generated",
           "config": {"workload": "complex-tap FIR bank, batched", "channels": S, "block_samples_per_channel": N, "fp32_peak_TFs": FP32_PEAK_TFS,
                      "hbm_peak_GBs": bc.HBM_PEAK_GBS},
           "roofline": {"bound": head["bound"], "kernel": head["kernel"], "kernel_avg_ms": head["event_ms_per_step"],
                        "timer": "HIP events around the object's calls (filter and history kernels)", "frac": head["frac"]},
           "shapes": shapes}
    if args.verify:
        res["verify"] = {"ok": all(s["verify"]["ok"] for s in shapes)}
    print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
