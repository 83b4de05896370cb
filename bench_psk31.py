#!/usr/bin/env python3
"""bench_psk31.py -- the BPSK31 receive chain, batched: simple_agc_cc 0.001 0.5 | timing_recovery_cc GARDNER 256 0.5 2 --add_q | dbpsk_decoder_c_u8 |
psk31_varicode_decoder_u8_u8 for `--channels` channels per call through one fused csdr_amd_psk31 object (psk31.hip, k_psk31).

One step = one process call over all channels (`--block` complex samples each, resident in HBM; every channel's state carries over from step to step).
The input is 64 distinct generated PSK31 signals (texts, carrier offsets, SNRs, timing phases) tiled over the channels.
Roofline: frac is against the HBM bound, input bytes / 8 TB/s.  Beside it, `chain_estimate` gives an UNMEASURED estimate of the dependent-chain bound:
the gain recurrence's three dependent float ops per sample at `--chain-cycles` cycles per sample (default 12: about 4 cycles each, not probed) times
the samples per channel, at --clock-ghz, when every channel has a SIMD lane of its own.

    python bench_psk31.py [--gpus 1] [--steps K] [--warmup W] [--channels 4096] [--block 131072] [--lanes 0] [--generic] [--verify] [--no-cpu-baseline]
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
TEXTS = ["CQ CQ DE K%dXYZ" % k for k in range(32)] + ["test %d ok" % (k * 7) for k in range(32)]


def signals(n_sig, n):
    import numpy as np
    import psk31_model as pm
    xs, sent = [], []
    for k in range(n_sig):
        t = TEXTS[k % len(TEXTS)]
        x = pm.psk31_signal(t, carrier=0.0002 * ((k % 9) - 4) / 4, phase=0.37 * k, timing_offset=(53 * k) % 256,
                            snr_db=[30, 20, 15, 12][k % 4], preamble=24, postamble=n // 256, seed=k)
        xs.append(x[:n]); sent.append(t)
    return np.stack(xs), sent


def ref_lib():
    import test_psk31_cpu as tc
    L = C.CDLL(REF_LIB)
    L.simple_agc_cc.restype = None
    L.simple_agc_cc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p]
    L.timing_recovery_init.restype = tc.TRState
    L.timing_recovery_init.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_char_p]
    L.timing_recovery_cc.restype = None
    L.timing_recovery_cc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(tc.TRState)]
    L.dbpsk_decoder_c_u8.restype = None
    L.dbpsk_decoder_c_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.psk31_varicode_decoder_push.restype = C.c_char
    L.psk31_varicode_decoder_push.argtypes = [C.POINTER(C.c_ulonglong), C.c_ubyte]
    return L


def cpu_baseline(X, threads=16):
    """the reference's four functions through libcsdr_ref.so, one channel per task on `threads` threads (ctypes releases the GIL); varicode per bit
    in Python is left out of the timing (its cost is per bit, 1/256 of the samples).  MS/s of input."""
    if not os.path.exists(REF_LIB):
        return None
    import numpy as np
    import test_psk31_cpu as tc
    L = ref_lib()

    def one(x):
        a, _ = tc.ref_agc(L, x, 0.001, 0.5, 65535.0)
        s, _, _, _ = tc.ref_timing(L, a, 0, 256, 0.5, 2.0, True)
        b = np.zeros(max(s.size, 1), np.uint8)
        L.dbpsk_decoder_c_u8(s.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), s.size)     # (the static last_input is shared: timing only)
        return s.size
    rows = [np.ascontiguousarray(X[k]) for k in range(min(X.shape[0], 4 * threads))]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, rows))
    wall = time.perf_counter() - t0
    return {"value": round(len(rows) * X.shape[1] / wall / 1e6, 2), "unit": "MS/s in", "threads": threads, "channels": len(rows),
            "what": "simple_agc_cc + timing_recovery_cc + dbpsk_decoder_c_u8 of libcsdr_ref.so (-O3 -ffast-math)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--block", type=int, default=131072)
    ap.add_argument("--lanes", type=int, default=0)
    ap.add_argument("--chain-cycles", type=float, default=12.0)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--generic", action="store_true", help="force k_psk31 (one lane per channel, no LDS staging)")
    ap.add_argument("--verify", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_psk31.py measures one GPU (--gpus 1)")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_psk31.py needs an MI355X; there is no CPU fallback")
    import csdr_amd
    ctx = csdr_amd.Context(0)
    S, N = args.channels, args.block
    X, sent = signals(64, N)
    xs = torch.from_numpy(X.view(np.float32)).cuda()
    x = xs.repeat((S + 63) // 64, 1)[:S].contiguous()                         # channel k carries signal k % 64
    obj = ctx.psk31(csdr_amd.psk31_params(), S, "agc", "varicode")
    if args.lanes:
        obj.set_lanes(args.lanes)
    if args.generic:
        obj.force_generic()
    opitch = (obj.max_out(N) + 63) // 64 * 64
    y = torch.empty((S, opitch), dtype=torch.uint8, device="cuda")
    cnt = torch.empty(S, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def step():
        obj.process_dev(x.data_ptr(), N, N, y.data_ptr(), opitch, cnt.data_ptr())

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
    k_ms = ev_ms / args.steps
    algo = S * N * 8
    t_hbm = algo / bc.HBM_PEAK_GBS / 1e9
    t_chain = N * args.chain_cycles / (args.clock_ghz * 1e9)               # an unmeasured estimate (no probe): reported apart from the measured bound
    bind = "hbm"
    res = {"metric": "MS/s in, BPSK31 receive chain (AGC | Gardner D 256 | DBPSK | varicode) x N channels",
           "value": round(S * N * args.steps / wall / 1e6, 1), "unit": "MS/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(wall / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "generated",
           "config": {"workload": "psk31 receive, fused, batched", "channels": S, "block_samples_per_channel": N, "distinct_signals": 64,
                      "lanes_per_wave": obj.lanes()},
           "roofline": {"bound": bind, "kernel": obj.kernel_name(), "kernel_avg_ms": round(k_ms, 4),
                        "bound_hbm_ms": round(t_hbm * 1e3, 4), "algorithmic_bytes_per_step": algo, "hbm_peak_GBs": bc.HBM_PEAK_GBS,
                        "frac": round(t_hbm / (k_ms * 1e-3), 4),
                        "chain_estimate": {"unmeasured": True, "ms": round(t_chain * 1e3, 4), "cycles_per_sample": args.chain_cycles, "clock_ghz": args.clock_ghz,
                                           "basis": "three dependent VALU ops per sample at about 4 cycles each, not probed",
                                           "frac": round(t_chain / (k_ms * 1e-3), 4)}}}
    if args.verify:
        import psk31_model as pm
        ok, bad = True, []
        for k in range(S):
            txt = first[k, :first_cnt[k]].tobytes()
            if sent[k % 64].encode() not in txt:
                ok = False; bad.append(k)
        sampled = [0, 1, 2, 3, 37, 63]
        stage_ok = True
        if os.path.exists(REF_LIB):
            import test_psk31_cpu as tc
            L = ref_lib()
            for k in sampled:
                a, _ = tc.ref_agc(L, X[k], 0.001, 0.5, 65535.0)
                s, _, _, _ = tc.ref_timing(L, a, 0, 256, 0.5, 2.0, True)
                b = tc.ref_dbpsk(L, s)
                t = tc.ref_varicode(L, b)
                stage_ok = stage_ok and t == first[k, :first_cnt[k]].tobytes()
                gs = ctx.psk31(csdr_amd.psk31_params(), 1, "agc", "timing").process(X[k])
                ms, _, _, _, _ = pm.timing(pm.agc(X[k], 0.001, 0.5)[0], 0, 256, 0.5, 2.0, True)
                stage_ok = stage_ok and np.array_equal(gs.view(np.uint32), ms.view(np.uint32)) and np.array_equal(
                    ctx.psk31(csdr_amd.psk31_params(), 1, "agc", "dbpsk").process(X[k]), b)
        res["verify"] = {"channels_text_ok": S - len(bad), "channels": S, "first_bad": bad[:8], "sampled_vs_reference": sampled,
                         "sampled_ok": bool(stage_ok), "ok": bool(ok and stage_ok)}
    if not args.no_cpu_baseline:
        cb = cpu_baseline(X)
        if cb:
            cb["speedup"] = round(res["value"] / cb["value"], 2)
        res["cpu_baseline"] = cb
    print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
