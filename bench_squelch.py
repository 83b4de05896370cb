#!/usr/bin/env python3
"""bench_squelch.py -- squelch_and_smeter_cc, batched: `--channels` channels x `--block` complex samples per step through one csdr_amd_squelch object
(squelch.hip), at the block sizes B = 16384 (one workgroup per block) and B = 1024 (one wave per block), use_every_nth = 1, half of the channels open.

The operator is memory traffic: 8 bytes in and 8 bytes out per complex sample.  Roofline: the HBM bound at those 16 bytes per sample.  Yardstick: the
library's plain streaming kernel csdr_amd_gain_ff over 2 n floats moves exactly the same bytes; it is timed in the same run on the same buffers,
interleaved with the squelch calls, medians of HIP-event times.  A two-pass squelch moves 24 bytes per sample (1.5 x), so the one-pass kernels have earned
their on-chip hold where squelch / gain_ff < 1.5.  The generic (two-pass) kernel is timed beside them.

    python bench_squelch.py [--gpus 1] [--steps K] [--warmup W] [--channels 4096] [--block 131072] [--verify] [--no-cpu-baseline]
"""
import argparse
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
LEVEL = 1e-3
BLOCKS = (16384, 1024)
THRESHOLD = 1.5


def signals(n_sig, n):
    """n_sig distinct rows of complex noise at power 1 (channel k carries row k % n_sig, scaled: even channels 4 x LEVEL = open, odd LEVEL / 4 = closed)"""
    import numpy as np
    rng = np.random.default_rng(2026)
    x = rng.standard_normal((n_sig, n, 2)).astype(np.float32) * np.float32(np.sqrt(0.5))
    return x.view(np.complex64).reshape(n_sig, n)


def channel_scale(k):
    import numpy as np
    return np.float32(np.sqrt(LEVEL * 4)) if k % 2 == 0 else np.float32(np.sqrt(LEVEL / 4))


def scaled_row(X, k):
    """channel k as the GPU buffer holds it: the float32 products of row k % 64"""
    import numpy as np
    return (X[k % X.shape[0]].view(np.float32) * channel_scale(k)).view(np.complex64)


def cpu_baseline(X, B, threads=16):
    """get_power_c of libcsdr_ref.so per block plus the copy (or the zeros) of the reference's loop, one row per task on `threads` threads.  MS/s."""
    if not os.path.exists(REF_LIB):
        return None
    import numpy as np
    import squelch_model as sm
    L = sm.ref_lib()
    rows = [scaled_row(X, k) for k in range(4 * threads)]

    def one(x):
        out = np.empty_like(x)
        for k in range(x.size // B):
            blk = x[k * B:(k + 1) * B]
            out[k * B:(k + 1) * B] = blk if L.get_power_c(sm._p(blk), B, 1) >= LEVEL else 0
        return out[0]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, rows))
    wall = time.perf_counter() - t0
    return {"value": round(len(rows) * X.shape[1] / wall / 1e6, 2), "unit": "MS/s", "threads": threads, "channels": len(rows), "B": B,
            "what": "get_power_c of libcsdr_ref.so (-O3 -ffast-math) and the block copy, per block"}


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--block", type=int, default=131072)
    ap.add_argument("--verify", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_squelch.py measures one GPU (--gpus 1)")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_squelch.py needs an MI355X; there is no CPU fallback")
    import csdr_amd
    ctx = csdr_amd.Context(0)
    S, N = args.channels, args.block
    if N % BLOCKS[0]:
        raise SystemExit("--block should be a multiple of %d" % BLOCKS[0])
    X = signals(64, N)
    xs = torch.from_numpy(X.view(np.float32)).cuda()
    x = xs.repeat((S + 63) // 64, 1)[:S].contiguous()                         # [S, 2 N] floats
    x *= torch.tensor([float(channel_scale(k)) for k in range(S)], device="cuda")[:, None]
    y = torch.empty_like(x)
    levels = np.full(S, LEVEL, np.float32)
    objs, gens, pw, fl = {}, {}, {}, {}
    for B in BLOCKS:
        objs[B] = ctx.squelch(S, B, 1, levels, N)
        gens[B] = ctx.squelch(S, B, 1, levels, N); gens[B].force_generic()
        pw[B] = torch.empty((S, N // B), dtype=torch.float32, device="cuda")
        fl[B] = torch.empty((S, N // B), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def sq(o, B):
        o.process_dev(x.data_ptr(), N, N, y.data_ptr(), N, pw[B].data_ptr(), N // B, fl[B].data_ptr())

    def gain():
        ctx.check(ctx.L.csdr_amd_gain_ff(ctx.h, x.data_ptr(), y.data_ptr(), 2 * S * N, 1.0), "gain_ff")

    calls = [("gain_ff", gain)] + [("one_pass_%d" % B, (lambda B=B: sq(objs[B], B))) for B in BLOCKS] + [("generic_%d" % B, (lambda B=B: sq(gens[B], B))) for B in BLOCKS]
    first = {}
    sampled = [k for k in (0, 1, 2, 3, 37, S - 1) if k < S]
    if args.verify:
        for B in BLOCKS:
            sq(objs[B], B); ctx.sync(); torch.cuda.synchronize()
            first[B] = ({k: y[k].cpu().numpy().view(np.complex64) for k in sampled}, pw[B].cpu().numpy(), fl[B].cpu().numpy())
    for _ in range(args.warmup):
        for _, f in calls:
            f()
    ctx.sync(); torch.cuda.synchronize()
    times = {name: [] for name, _ in calls}
    for _ in range(args.steps):                                                   # interleaved repeats, one HIP-event pair around every call
        for name, f in calls:
            ctx.timer_start(); f(); times[name].append(ctx.timer_stop_ms())
    # the headline: wall time of back-to-back steps of the default configuration
    B0 = BLOCKS[0]
    ctx.sync(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        sq(objs[B0], B0)
    ctx.sync(); torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    med = {k: median(v) for k, v in times.items()}
    algo = 16 * S * N
    t_hbm_ms = algo / bc.HBM_PEAK_GBS / 1e9 * 1e3
    shapes = {}
    for B in BLOCKS:
        t = med["one_pass_%d" % B]
        shapes[str(B)] = {"kernel": objs[B].kernel_name(), "ms": round(t, 4), "gain_ff_ms": round(med["gain_ff"], 4), "ratio_to_gain_ff": round(t / med["gain_ff"], 4),
                          "ratio_met": bool(t / med["gain_ff"] < THRESHOLD), "frac_of_hbm_bound": round(t_hbm_ms / t, 4), "GBs": round(algo / t / 1e6, 1),
                          "generic_ms": round(med["generic_%d" % B], 4), "generic_ratio_to_gain_ff": round(med["generic_%d" % B] / med["gain_ff"], 4),
                          "min_ms": round(min(times["one_pass_%d" % B]), 4), "max_ms": round(max(times["one_pass_%d" % B]), 4)}
    res = {"metric": "MS/s, squelch_and_smeter_cc x N channels (B 16384, use_every_nth 1, half of the channels open)",
           "value": round(S * N * args.steps / wall / 1e6, 1), "unit": "MS/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(wall / args.steps * 1e3, 4), "event_ms_per_step": shapes[str(B0)]["ms"], "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": "f32", "data": "generated",
           "config": {"workload": "squelch and S-meter, batched", "channels": S, "block_samples_per_channel": N, "distinct_signals": 64, "B": list(BLOCKS),
                      "use_every_nth": 1, "open_channels": (S + 1) // 2},
           "roofline": {"bound": "hbm", "kernel": objs[B0].kernel_name(), "kernel_avg_ms": shapes[str(B0)]["ms"],
                        "timer": "HIP events around every call, medians over interleaved repeats (gain_ff, one-pass and generic at both B)",
                        "reason": "no arithmetic to speak of: 8 bytes read and 8 bytes written per complex sample", "algorithmic_bytes_per_step": algo,
                        "hbm_peak_GBs": bc.HBM_PEAK_GBS, "bound_hbm_ms": round(t_hbm_ms, 4), "frac": shapes[str(B0)]["frac_of_hbm_bound"]},
           "yardstick": {"what": "csdr_amd_gain_ff over 2 n floats on the same buffers (the same 16 bytes per sample)", "ms": round(med["gain_ff"], 4),
                         "threshold": THRESHOLD, "why": "a two-pass squelch moves 24 bytes per sample, 1.5 x the bytes of gain_ff"},
           "shapes": shapes}
    if args.verify:
        import squelch_model as sm
        ok, bits, in_gate = True, True, True
        for B in BLOCKS:
            yy, pp, ff = first[B]
            for k in sampled:
                row = scaled_row(X, k)
                got = yy[k]
                wo, wp, wf = sm.stream(row, B, 1, LEVEL)
                bits = bits and got.tobytes() == wo.tobytes() and pp[k].tobytes() == wp.tobytes() and bool(np.array_equal(ff[k], wf))
                P = np.array([sm.power64(row[j * B:(j + 1) * B]) for j in range(N // B)])
                in_gate = in_gate and bool(np.all(np.abs(pp[k].astype(np.float64) - P) <= (B + 8) * sm.U * P))
                ok = ok and bool(wf.all() == (k % 2 == 0)) and bool(wf.any() == (k % 2 == 0))
        res["verify"] = {"sampled_channels": sampled, "bit_identical_to_model": bool(bits), "powers_in_gate": bool(in_gate), "open_closed_as_generated": bool(ok),
                         "ok": bool(bits and in_gate and ok)}
    if not args.no_cpu_baseline:
        cb = cpu_baseline(X, B0)
        if cb:
            cb["speedup"] = round(res["value"] / cb["value"], 2)
        res["cpu_baseline"] = cb
    print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
