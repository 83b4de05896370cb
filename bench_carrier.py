#!/usr/bin/env python3
"""bench_carrier.py -- carrier recovery, batched: `--channels` channels x `--block` complex samples per step through one csdr_amd_carrier object
(carrier.hip): bpsk_costas_loop_cc 0.05 0.707 plain and decision-directed on BPSK at 32 samples per symbol, and pll_cc 2 0.01 on a tone.

Each loop reads 8 bytes and writes 8 bytes per sample (`out` for the Costas loops, the NCO for the PLL, as the commands do), so the roofline named in the
line is the HBM bound at 16 bytes per sample; what binds is the sample-serial chain (a double cos, sin and, decision-directed or PLL, atan2 per sample), and
the line says how far from the HBM bound that leaves each loop.  Both kernels are timed on the same buffers, interleaved, medians of HIP-event times;
`lanes_sweep_ms` times the channels-per-wave choices of both kernels on every loop.

    python bench_carrier.py [--gpus 1] [--steps K] [--warmup W] [--channels 4096] [--block 131072] [--verify] [--no-cpu-baseline] [--no-sweep]
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
# name -> (kind, bandwidth, damping, decision_directed, the output the command writes)
CONFIGS = {"costas": ("costas", 0.05, 0.707, 0, "out"), "costas_dd": ("costas", 0.05, 0.707, 1, "out"), "pll_pi": ("pll", 0.01, 0.707, 0, "nco")}
OUTPUTS = ("out", "error", "dphase", "nco")


def signals(kind, n_sig, n):
    """n_sig distinct rows: BPSK (32 samples per symbol, 20 dB, offsets around 0.001) or tones (around 0.005, 20 dB), each with its own seed and phase"""
    import numpy as np
    import carrier_model as cm
    if kind == "costas":
        return np.stack([cm.bpsk_signal(n, 32, 0.001 * (1 + 0.01 * k), 20, 500 + k) for k in range(n_sig)])
    return np.stack([cm.tone_signal(n, 0.005 * (1 + 0.01 * k), 20, 700 + k) for k in range(n_sig)])


def params_of(name):
    import csdr_amd
    kind, bw, damping, dd, _ = CONFIGS[name]
    return csdr_amd.costas_params(bw, damping, dd) if kind == "costas" else csdr_amd.pll_params(2, bandwidth=bw, damping=damping)


def cpu_baseline(name, X, threads=16):
    """the reference function of libcsdr_ref.so over whole rows, one row per task on `threads` threads.  MS/s."""
    if not os.path.exists(REF_LIB):
        return None
    import carrier_model as cm
    L = cm.bind(C.CDLL(REF_LIB))
    kind, bw, damping, dd, _ = CONFIGS[name]
    rows = [X[k % X.shape[0]] for k in range(4 * threads)]

    states = [cm.costas_init(L, bw, damping, dd) if kind == "costas" else cm.pll_init(L, "PI", bw) for _ in rows]      # (the init prints: not from the pool)

    def one(k):
        if kind == "costas":
            return cm.drive_costas(L, rows[k], bw, damping, dd, st=states[k])[0]["out"][0]
        return cm.drive_pll(L, rows[k], "PI", bw, st=states[k])[0]["nco"][0]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, range(len(rows))))
    wall = time.perf_counter() - t0
    return {"value": round(len(rows) * X.shape[1] / wall / 1e6, 2), "unit": "MS/s", "threads": threads, "channels": len(rows),
            "what": "%s of libcsdr_ref.so (-O3 -ffast-math), every output pointer given" % ("bpsk_costas_loop_cc" if kind == "costas" else "pll_cc")}


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--block", type=int, default=131072)
    ap.add_argument("--verify", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_carrier.py measures one GPU (--gpus 1)")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_carrier.py needs an MI355X; there is no CPU fallback")
    import csdr_amd
    ctx = csdr_amd.Context(0)
    S, N = args.channels, args.block
    n_sig = min(64, S)
    X = {kind: signals(kind, n_sig, N) for kind in ("costas", "pll")}
    x = {kind: torch.from_numpy(X[kind].view(np.float32)).cuda().repeat((S + n_sig - 1) // n_sig, 1)[:S].contiguous() for kind in X}      # [S, 2 N] floats
    y = torch.empty((S, 2 * N), dtype=torch.float32, device="cuda")
    objs = {}
    for name in CONFIGS:
        P = params_of(name)
        objs[name, "tiled"] = ctx.carrier(P, S)
        objs[name, "generic"] = ctx.carrier(P, S); objs[name, "generic"].force_generic()
    torch.cuda.synchronize()

    def step(o, name):
        kind, _, _, _, which = CONFIGS[name]
        o.reset()                                                             # every step walks the same stream from a fresh loop
        o.process_dev(x[kind].data_ptr(), N, N, *[y.data_ptr() if k == which else None for k in OUTPUTS], N)

    calls = [("%s/%s" % (name, kern), (lambda name=name, kern=kern: step(objs[name, kern], name))) for name in CONFIGS for kern in ("tiled", "generic")]
    sampled = [k for k in (0, 1, 2, 37, S - 1) if k < S]
    first = {}
    if args.verify:
        for cname, f in calls:
            f(); ctx.sync(); torch.cuda.synchronize()
            first[cname] = {k: y[k].cpu().numpy().copy() for k in sampled}
    for _ in range(args.warmup):
        for _, f in calls:
            f()
    ctx.sync(); torch.cuda.synchronize()
    times = {cname: [] for cname, _ in calls}
    for _ in range(args.steps):                                               # interleaved repeats, one HIP-event pair around every call
        for cname, f in calls:
            ctx.timer_start(); f(); times[cname].append(ctx.timer_stop_ms())
    med = {k: median(v) for k, v in times.items()}
    sweep = None
    if not args.no_sweep:                                                     # the channels-per-wave choices of both kernels on every loop
        sweep = {name: {"tiled": {}, "generic": {}} for name in CONFIGS}
        for name in CONFIGS:
            for kern, choices in (("tiled", (1, 2, 4, 8, 16, 32, 64)), ("generic", (4, 16, 64))):
                o = objs[name, kern]
                for lanes in choices:
                    o.set_lanes(lanes); step(o, name); ctx.sync()
                    t = []
                    for _ in range(3):
                        ctx.timer_start(); step(o, name); t.append(ctx.timer_stop_ms())
                    sweep[name][kern][str(lanes)] = round(median(t), 3)
                o.set_lanes(0)
    # the headline: wall time of back-to-back steps of the default kernel on the plain Costas loop
    default = "tiled"                                                         # (what the library takes on aligned rows)
    ctx.sync(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(objs["costas", default], "costas")
    ctx.sync(); torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    algo = 16 * S * N
    t_hbm_ms = algo / bc.HBM_PEAK_GBS / 1e9 * 1e3
    shapes = {}
    for name in CONFIGS:
        t, g = med[name + "/tiled"], med[name + "/generic"]
        shapes[name] = {"kernel": objs[name, "tiled"].kernel_name(), "channels_per_wave": objs[name, "tiled"].lanes(), "ms": round(t, 3),
                        "MSps": round(S * N / t / 1e3, 1), "frac_of_hbm_bound": round(t_hbm_ms / t, 5), "ns_per_sample_of_a_channel": round(t * 1e6 / N, 2),
                        "generic_kernel": objs[name, "generic"].kernel_name(), "generic_channels_per_wave": objs[name, "generic"].lanes(), "generic_ms": round(g, 3),
                        "min_ms": round(min(times[name + "/tiled"]), 3), "max_ms": round(max(times[name + "/tiled"]), 3)}
    res = {"metric": "MS/s, bpsk_costas_loop_cc 0.05 0.707 x N channels", "value": round(S * N * args.steps / wall / 1e6, 1), "unit": "MS/s", "n_gpus": 1,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(wall / args.steps * 1e3, 3), "event_ms_per_step": shapes["costas"]["ms"],
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "generated",
           "config": {"workload": "carrier recovery, batched", "channels": S, "block_samples_per_channel": N, "distinct_signals": n_sig,
                      "loops": {k: {"bandwidth": v[1], "damping": v[2], "decision_directed": bool(v[3]), "output": v[4]} for k, v in CONFIGS.items()}},
           "roofline": {"bound": "hbm", "kernel": shapes["costas"]["kernel"], "kernel_avg_ms": shapes["costas"]["ms"],
                        "timer": "HIP events around every call (a state reset and one launch), medians over interleaved repeats of both kernels on the three loops",
                        "reason": "8 bytes read and 8 bytes written per complex sample; the sample-serial chain binds, not the traffic: see frac",
                        "algorithmic_bytes_per_step": algo, "hbm_peak_GBs": bc.HBM_PEAK_GBS, "bound_hbm_ms": round(t_hbm_ms, 4), "frac": shapes["costas"]["frac_of_hbm_bound"]},
           "shapes": shapes, "lanes_sweep_ms": sweep}
    if args.verify:
        import carrier_model as cm
        from test_carrier_cpu import G
        ver = {}
        ok = True
        for name in CONFIGS:
            kind, bw, damping, dd, which = CONFIGS[name]
            fam = "costas" if kind == "costas" else "pll"
            P = params_of(name)
            dt = np.complex64
            words = dev = cross = 0
            for k in sampled:
                row = X[kind][k % n_sig]
                want = csdr_amd.carrier_debug_walk(P, row, (which,))[which]
                got = first[name + "/tiled"][k].view(dt)
                words += cm.words_differing(got, want); dev = max(dev, cm.maxdev(got, want))
                cross += cm.words_differing(got, first[name + "/generic"][k].view(dt))
            m = 4096                                                          # the float32 model on the head of channel 0
            row = X[kind][0][:m]
            model = (cm.costas(row, P.alpha, P.beta, P.dphase_max, bool(dd))[0] if kind == "costas" else cm.pll(row, True, P.alpha, P.beta)[0])[which]
            head = first[name + "/tiled"][0].view(dt)[:m]
            mdev = cm.maxdev(head, model)
            good = bool(dev <= G[fam, which] and mdev <= G[fam, which] and cross == 0)
            ver[name] = {"words_differing_from_cpu_walk": int(words), "largest_deviation_from_cpu_walk": dev, "largest_deviation_from_model_head": mdev,
                         "model_head_words_differing": cm.words_differing(head, model), "gate": G[fam, which], "tiled_vs_generic_words_differing": int(cross), "ok": good}
            ok = ok and good
        ver["sampled_channels"] = sampled
        ver["ok"] = bool(ok)
        res["verify"] = ver
    if not args.no_cpu_baseline:
        cbs = {}
        for name in CONFIGS:
            cb = cpu_baseline(name, X[CONFIGS[name][0]])
            if cb:
                cb["speedup"] = round(shapes[name]["MSps"] / cb["value"], 2)
            cbs[name] = cb
        res["cpu_baseline"] = cbs["costas"]
        res["cpu_baselines"] = cbs
    print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
