#!/usr/bin/env python3
"""bench_shiftbank.py -- the shifter bank: shift_addition_cc, shift_math_cc and shift_table_cc for N streams with a rate PER STREAM through one
csdr_amd_shiftbank object (shiftbank.hip).

One step = one process call over all streams (`--block` complex samples each, resident in HBM, every stream's phase state carried from step to step).
Shapes: 64 streams x 2 Mi samples with 64 distinct rates, and 4096 x 131072 (`--shapes`).  Algorithmic bytes: 16 per sample with a row per stream, 8 per
sample with one input row shared by every stream (timed for the first shape).  frac = the time of those bytes at 8 TB/s over the measured step.
The comparison is the same work without the object: one csdr_amd_shift_cc per stream on the same buffers (each stream's phase carried on the host), timed in
the same process.  profiles/r6_ops.jsonl holds 0.563 (addition) and 0.17 (math, table) of HBM for ONE rate shared by 64 streams.
MATH / TABLE also report the scan-ahead: the hit rate of the timed steps, and a step whose scan runs in the call (a set_rate in front of every step).

One JSON line per variant:
    python bench_shiftbank.py [--gpus 1] [--steps K] [--warmup W] [--shapes 64x2097152,4096x131072] [--variants addition,math,table] [--generic] [--verify]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench_common as bc  # noqa: E402

SAMPLED = 4                      # rows --verify compares
HEAD = 6000                      # samples of a sampled row that --verify also walks on the CPU
R6_ONE_RATE = {"addition": 0.563, "math": 0.1685, "table": 0.1704}


def stream_rates(S):
    """a rate per stream, spread over (-0.45, 0.45)"""
    import numpy as np
    return (-0.45 + 0.9 * (np.arange(S) + 0.5) / S).astype(np.float32)


def shape(ctx, variant, S, N, args):
    import numpy as np
    import torch
    import csdr_amd
    from oracle import relrms
    L = ctx.L
    rates = stream_rates(S)
    aux = 65536 if variant == "table" else 0
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    x = torch.randn((S, N, 2), dtype=torch.float32, device="cuda", generator=g)
    y = torch.empty((S, N, 2), dtype=torch.float32, device="cuda")
    bank = csdr_amd.ShiftBank(ctx, variant, rates, aux=aux, max_samples_per_call=N)
    if args.generic:
        bank.force_generic()
    phases = (C.c_float * S)()
    phase_ptr = [C.cast(C.addressof(phases) + 4 * s, C.POINTER(C.c_float)) for s in range(S)]

    def step():
        bank.process_dev(x.data_ptr(), N, y.data_ptr(), N, N)

    def step_shared():
        bank.process_dev(x.data_ptr(), 0, y.data_ptr(), N, N)

    def step_scan_in_call():
        bank.set_rate(0, float(rates[0]))
        step()

    def step_composed():
        for s in range(S):
            ctx.check(L.csdr_amd_shift_cc(ctx.h, csdr_amd.SHIFT[variant], float(rates[s]), phase_ptr[s], x.data_ptr() + 8 * N * s, y.data_ptr() + 8 * N * s,
                                          1, N, N, N, 1024, aux), "shift_cc")

    def timed(fn, steps):
        ctx.timer_start()
        for _ in range(steps):
            fn()
        return ctx.timer_stop_ms() / steps

    ver = None
    if args.verify:                                      # the first step from the stream's start, both ways
        rows = sorted(set(int(v) for v in np.linspace(0, S - 1, SAMPLED)))
        step(); ctx.sync()
        got = {k: y[k].cpu().numpy().view(np.complex64).ravel() for k in rows}
        step_composed(); ctx.sync()
        bits_ok, gate_ok = True, True
        for k in rows:
            ref = y[k].cpu().numpy().view(np.complex64).ravel()
            bits_ok = bits_ok and bool(np.array_equal(got[k].view(np.uint32), ref.view(np.uint32)))
            xr = x[k].cpu().numpy().view(np.complex64).ravel()[:HEAD]
            walk = csdr_amd.shiftbank_debug_walk(variant, float(rates[k]), xr, aux=aux)
            gate_ok = gate_ok and bool(relrms(got[k][:HEAD], walk) < (1e-6 if variant == "addition" else 1e-5))
        ver = {"rows": rows, "bits_equal_one_shift_cc_per_stream": bits_ok, "cpu_walk_head_in_gate": gate_ok, "ok": bits_ok and gate_ok}
        bank.reset()
        for s in range(S):
            phases[s] = 0.0

    for _ in range(args.warmup):
        step()
    ctx.sync(); torch.cuda.synchronize()
    hits0 = bank.scans_ahead()
    t0 = time.perf_counter()
    ev_ms = timed(step, args.steps)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / args.steps
    hits = bank.scans_ahead() - hits0
    rounds = 3                                           # the comparison, alternating, in the same run
    per = max(1, args.steps // rounds)
    per_cmp = max(1, min(per, 4096 // S))                # (S calls per step, a host phase scan in each MATH / TABLE call)
    ms_b, ms_c = [], []
    for _ in range(rounds):
        ms_c.append(timed(step_composed, per_cmp)); step(); ms_b.append(timed(step, per))
    samples = S * N
    t16 = 16 * samples / bc.HBM_PEAK_GBS / 1e9
    res = {"variant": variant, "streams": S, "block_samples_per_stream": N, "kernel": bank.kernel_name(), "ms_per_step": round(wall * 1e3, 4),
           "event_ms_per_step": round(ev_ms, 4), "MS_per_s": round(samples / (ev_ms * 1e-3) / 1e6, 1), "algorithmic_bytes_per_step": 16 * samples,
           "frac": round(t16 / (ev_ms * 1e-3), 4),
           "alternating": {"rounds": rounds, "bank_steps_per_round": per, "composed_steps_per_round": per_cmp, "bank_ms": [round(v, 4) for v in ms_b],
                           "one_shift_cc_per_stream_ms": [round(v, 4) for v in ms_c], "composed_frac": round(t16 / (min(ms_c) * 1e-3), 4),
                           "bank_over_composed": round(min(ms_b) / min(ms_c), 4)}}
    if variant != "addition":
        step()
        ms_in_call = timed(step_scan_in_call, max(2, per))
        step()
        res["scan_ahead"] = {"timed_steps": args.steps, "hits": hits, "hit_rate": round(hits / args.steps, 4), "ms_scan_ready": round(min(ms_b), 4),
                             "ms_scan_in_call": round(ms_in_call, 4)}
    if S * N <= (1 << 27):                               # the shared input row: 8 bytes per sample
        for _ in range(args.warmup):
            step_shared()
        ms_sh = timed(step_shared, args.steps)
        res["shared_row"] = {"event_ms_per_step": round(ms_sh, 4), "algorithmic_bytes_per_step": 8 * samples, "frac": round(t16 / 2 / (ms_sh * 1e-3), 4)}
    if ver is not None:
        res["verify"] = ver
    bank.close()
    del x, y
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="64x2097152,4096x131072", help="streams x samples per stream of every timed shape; the first is the headline")
    ap.add_argument("--variants", default="addition,math,table")
    ap.add_argument("--generic", action="store_true", help="force k_shiftbank_generic")
    ap.add_argument("--verify", action="store_true")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_shiftbank.py measures one GPU (--gpus 1)")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_shiftbank.py needs an MI355X; there is no CPU fallback")
    import csdr_amd
    ctx = csdr_amd.Context(0)
    dims = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    for variant in args.variants.split(","):
        shapes = [shape(ctx, variant, S, N, args) for S, N in dims]
        head = shapes[0]
        res = {"metric": "MS/s, shift_%s_cc x N streams, a rate per stream (shifter bank)" % variant, "value": head["MS_per_s"], "unit": "MS/s", "n_gpus": 1,
               "steps": args.steps, "warmup": args.warmup, "ms_per_step": head["ms_per_step"], "event_ms_per_step": head["event_ms_per_step"],
               "higher_is_better": True, "scaling": "weak", "vs_baseline": round(1.0 / head["alternating"]["bank_over_composed"], 3), "dtype": "f32", "data": "generated",
               "config": {"workload": "shifter bank, batched", "variant": variant, "streams": head["streams"], "block_samples_per_stream": head["block_samples_per_stream"],
                          "baseline": "one csdr_amd_shift_cc per stream on the same buffers, same process", "hbm_peak_GBs": bc.HBM_PEAK_GBS,
                          "one_rate_for_64_streams_frac_r6": R6_ONE_RATE[variant]},
               "roofline": {"bound": "hbm", "kernel": head["kernel"], "kernel_avg_ms": head["event_ms_per_step"],
                            "timer": "HIP events on the context's stream around the object's calls", "frac": head["frac"]},
               "shapes": shapes}
        if args.verify:
            res["verify"] = {"ok": all(s["verify"]["ok"] for s in shapes)}
        print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
