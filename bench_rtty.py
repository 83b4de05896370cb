#!/usr/bin/env python3
"""bench_rtty.py -- the RTTY receive chain, batched: bfsk_demod_cf 0.02125 101 | serial_line_decoder_f_u8 176.0176 5 1.5 | rtty_baudot2ascii_u8_u8
(45.45 Bd at 170 Hz shift, 8 kS/s per channel) for `--channels` channels per call through one fused csdr_amd_rtty object (rtty.hip).

One step = one process call over all channels (`--block` complex samples each, resident in HBM; every channel's state carries over from step to step).
The input is 64 distinct generated RTTY signals (texts, carrier offsets, SNRs, bit phases) tiled over the channels.
Roofline: the discriminator dominates.  Its algorithmic cost is 16 L FP32 flops and 8 bytes per input sample; the FP32 bound (157.3 TF, the f32 MFMA
and VALU peak) binds over the HBM bound (8 TB/s) whenever 16 L / 157.3e12 > 8 / 8e12, i.e. L > 10.  `kernel_avg_ms` is the discriminator alone
(a BFSK-only object on the same input, HIP events around its calls); frac = the bound's time over it.

    python bench_rtty.py [--gpus 1] [--steps K] [--warmup W] [--channels 4096] [--block 131072] [--generic] [--verify] [--no-cpu-baseline]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench_common as bc  # noqa: E402

REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libcsdr_ref.so")
TEXTS = ["CQ CQ DE K%dXYZ K" % k for k in range(32)] + ["RYRY TEST %d OK" % (k * 7) for k in range(32)]
FP32_PEAK_TFS = 157.3
SPACING, L_TAPS, SPB, DATABITS, STOPBITS, B = 0.02125, 101, 176.0176, 5, 1.5, 16384


def signals(n_sig, n):
    import numpy as np
    import rtty_model as rm
    xs, sent = [], []
    for k in range(n_sig):
        t = TEXTS[k % len(TEXTS)]
        kw = dict(carrier=0.0003 * ((k % 9) - 4) / 4 + 0.0001, bit_phase=(0.37 * k) % 1, snr_db=[30, 20, 15, 12][k % 4], lead=1500 + 97 * k, seed=k)
        x = rm.rtty_signal(t, **kw)                                             # (at the default block the text ends > 2 B before the block does)
        x = rm.rtty_signal(t, tail=max(0, n - len(x)), **kw)
        xs.append(x[:n]); sent.append(t)
    return np.stack(xs), sent


def cpu_baseline(X, threads=16):
    """bfsk_demod_cf and serial_line_decoder_f_u8 (the CLI's windows) of libcsdr_ref.so, one channel per task on `threads` threads (ctypes releases the
    GIL); the Baudot lookup per character is left out of the timing.  MS/s of input."""
    if not os.path.exists(REF_LIB):
        return None
    import numpy as np
    import rtty_model as rm
    L = rm.ref_lib()
    m, s = rm.ref_peak(L, L_TAPS, np.float32(SPACING) / 2), rm.ref_peak(L, L_TAPS, -np.float32(SPACING) / 2)

    def one(x):
        y = rm.ref_bfsk(L, x, m, s)
        return len(rm.ref_serial_stream(L, y, SPB, DATABITS, STOPBITS, B))
    rows = [np.ascontiguousarray(X[k]) for k in range(min(X.shape[0], 4 * threads))]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, rows))
    wall = time.perf_counter() - t0
    return {"value": round(len(rows) * X.shape[1] / wall / 1e6, 2), "unit": "MS/s in", "threads": threads, "channels": len(rows),
            "what": "bfsk_demod_cf + serial_line_decoder_f_u8 of libcsdr_ref.so (-O3 -ffast-math)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--block", type=int, default=131072)
    ap.add_argument("--generic", action="store_true", help="force k_bfsk_generic (one thread per output)")
    ap.add_argument("--verify", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_rtty.py measures one GPU (--gpus 1)")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rtty.py needs an MI355X; there is no CPU fallback")
    import csdr_amd
    ctx = csdr_amd.Context(0)
    S, N = args.channels, args.block
    X, sent = signals(64, N)
    xs = torch.from_numpy(X.view(np.float32)).cuda()
    x = xs.repeat((S + 63) // 64, 1)[:S].contiguous()                         # channel k carries signal k % 64
    P = csdr_amd.rtty_params(SPACING, L_TAPS, 1024, SPB, DATABITS, STOPBITS, 0.4, B)
    obj = ctx.rtty(P, S, "bfsk", "baudot")
    disc = ctx.rtty(P, S, "bfsk", "bfsk")                                       # the discriminator alone, for its kernel time
    if args.generic:
        obj.force_generic(); disc.force_generic()
    opitch = (obj.max_out(N) + 63) // 64 * 64
    y = torch.empty((S, opitch), dtype=torch.uint8, device="cuda")
    yd = torch.empty((S, N), dtype=torch.float32, device="cuda")
    cnt = torch.empty(S, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def step():
        obj.process_dev(x.data_ptr(), N, N, y.data_ptr(), opitch, cnt.data_ptr())

    def step_disc():
        disc.process_dev(x.data_ptr(), N, N, yd.data_ptr(), N, cnt.data_ptr())

    obj.reset()
    step()                                                                      # from the reset state: the outputs --verify checks
    ctx.sync()
    first, first_cnt = (y.cpu().numpy(), cnt.cpu().numpy()) if args.verify else (None, None)
    for _ in range(args.warmup):
        step()
    ctx.sync(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.timer_start()
    for _ in range(args.steps):
        step()
    ev_ms = ctx.timer_stop_ms()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    for _ in range(args.warmup):
        step_disc()
    ctx.sync()
    ctx.timer_start()
    for _ in range(args.steps):
        step_disc()
    d_ms = ctx.timer_stop_ms() / args.steps
    torch.cuda.synchronize()
    outs = S * N                                                                 # (steady state: every channel has its L - 1 history)
    flops = 16 * L_TAPS * outs
    t_fp32 = flops / (FP32_PEAK_TFS * 1e12)
    algo = S * N * 8
    t_hbm = algo / bc.HBM_PEAK_GBS / 1e9
    bind = "fp32" if t_fp32 >= t_hbm else "hbm"
    t_bound = max(t_fp32, t_hbm)
    res = {"metric": "MS/s in, RTTY receive chain (bfsk_demod_cf L 101 | serial 45.45 Bd 5N1.5 | Baudot) x N channels",
           "value": round(S * N * args.steps / wall / 1e6, 1), "unit": "MS/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(wall / args.steps * 1e3, 4), "event_ms_per_step": round(ev_ms / args.steps, 4), "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": "f32", "data": "generated",
           "config": {"workload": "rtty receive, fused, batched", "channels": S, "block_samples_per_channel": N, "distinct_signals": 64, "B": B,
                      "filter_length": L_TAPS},
           "roofline": {"bound": bind, "kernel": disc.kernel_name(), "kernel_avg_ms": round(d_ms, 4), "timer": "HIP events around the BFSK-only object's calls",
                        "reason": "16 L = %d FP32 flops per 8 input bytes: %.0f flop/B against a ridge of %.1f" % (16 * L_TAPS, 2 * L_TAPS, FP32_PEAK_TFS * 1e3 / bc.HBM_PEAK_GBS),
                        "bound_fp32_ms": round(t_fp32 * 1e3, 4), "bound_hbm_ms": round(t_hbm * 1e3, 4), "flops_per_step": flops, "fp32_peak_TFs": FP32_PEAK_TFS,
                        "algorithmic_bytes_per_step": algo, "hbm_peak_GBs": bc.HBM_PEAK_GBS, "frac": round(t_bound / (d_ms * 1e-3), 4),
                        "rest_of_chain_ms": round(ev_ms / args.steps - d_ms, 4)}}
    if args.verify:
        import rtty_model as rm
        bad = [k for k in range(S) if first[k, :first_cnt[k]].tobytes() != sent[k % 64].upper().encode()]
        sampled = [0, 1, 2, 3, 37, 63]
        m, s = csdr_amd.firdes_peak_c(L_TAPS, np.float32(SPACING) / 2), csdr_amd.firdes_peak_c(L_TAPS, -np.float32(SPACING) / 2)
        gate_ok = True
        one = ctx.rtty(P, 1, "bfsk", "bfsk")
        for k in sampled:
            one.reset()
            g = one.process(X[k])
            gate_ok = gate_ok and g.size == N - L_TAPS + 1 and bool(np.all(np.abs(g - rm.bfsk64(X[k], m, s)) <= rm.bfsk_gate(X[k], m, s)))
        one.close()
        res["verify"] = {"channels_text_ok": S - len(bad), "channels": S, "first_bad": bad[:8], "sampled_rows_in_gate": sampled, "gate_ok": bool(gate_ok),
                         "ok": bool(not bad and gate_ok)}
    if not args.no_cpu_baseline:
        cb = cpu_baseline(X)
        if cb:
            cb["speedup"] = round(res["value"] / cb["value"], 2)
        res["cpu_baseline"] = cb
    print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
