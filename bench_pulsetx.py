#!/usr/bin/env python3
"""bench_pulsetx.py -- the pulse-shaped symbol transmitter, batched: psk_modulator_u8_c 4 | plain_interpolate_cc 8 | pulse_shaping_filter_cc RRC 8 65 0.35
for `--channels` channels per call through one csdr_amd_pulsetx object (modem.hip).

One step = one process call over all channels (`--symbols` symbols each; symbols and output resident in HBM, every channel's history carries over).
Timed in the same run, on the same buffers: the fused kernel (k_pulsetx_poly), the generic kernel (k_pulsetx_generic) and the composed path
(the modulator, csdr_amd_plain_interpolate_cc, csdr_amd_apply_real_fir_cc: three launches, the zero-stuffed stream written to and read from HBM).
Roofline: the fused kernel is store bound; frac is the HBM store bound (output bytes / 8 TB/s) over the measured time per step, the symbols are
1 / (8 I) of the output.  `fused_over_composed_time` is what was measured; by traffic the composed path moves about three times the bytes.  No target is set
and nothing is hidden: the run reports a fused kernel slower than the composed path in `note` and exits zero.

    python bench_pulsetx.py [--gpus 1] [--steps K] [--warmup W] [--channels 4096] [--symbols 16384] [--interpolation 8] [--taps 65] [--beta 0.35]
                            [--n-psk 4] [--verify] [--no-cpu-baseline]
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


def cpu_baseline(X, n_psk, interpolation, taps, threads=16):
    """the reference's three functions through libcsdr_ref.so, one channel per task on `threads` threads (ctypes releases the GIL).  MS/s of output."""
    if not os.path.exists(REF_LIB):
        return None
    import numpy as np
    import test_pulse_cpu as tc
    L = tc.bind_modem(C.CDLL(REF_LIB))

    def one(row):
        return tc.lib_fir(L, tc.lib_interpolate(L, tc.lib_modulate(L, row, n_psk), interpolation), taps).size
    rows = [np.ascontiguousarray(X[k % X.shape[0]]) for k in range(4 * threads)]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        n_out = sum(ex.map(one, rows))
    wall = time.perf_counter() - t0
    return {"value": round(n_out / wall / 1e6, 2), "unit": "MS/s out", "threads": threads, "channels": len(rows),
            "what": "psk_modulator_u8_c + plain_interpolate_cc + apply_real_fir_cc of libcsdr_ref.so (-O3 -ffast-math)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--symbols", type=int, default=16384)
    ap.add_argument("--interpolation", type=int, default=8)
    ap.add_argument("--taps", type=int, default=65)
    ap.add_argument("--beta", type=float, default=0.35)
    ap.add_argument("--n-psk", type=int, default=4)
    ap.add_argument("--verify", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_pulsetx.py measures one GPU (--gpus 1)")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pulsetx.py needs an MI355X; there is no CPU fallback")
    import csdr_amd
    import pulse_model as pm
    ctx = csdr_amd.Context(0)
    S, N, I, T, P = args.channels, args.symbols, args.interpolation, args.taps, args.n_psk
    taps = csdr_amd.firdes_rrc_f(T, I, args.beta)
    X = np.random.default_rng(31).integers(0, P, (64, N)).astype(np.uint8)        # a fixed generator: the same every run
    x = torch.from_numpy(X).cuda().repeat((S + 63) // 64, 1)[:S].contiguous()      # channel k sends row k % 64
    obj = ctx.pulse_tx(S, P, I, taps)
    mod = ctx.pulse_tx(S, P, 1, None, "mod", "mod")
    opitch = obj.max_out(N)
    y = torch.empty((S, opitch, 2), dtype=torch.float32, device="cuda")
    sym = torch.empty((S, N, 2), dtype=torch.float32, device="cuda")              # the composed path's two intermediate streams
    stuffed = torch.empty((S, N * I, 2), dtype=torch.float32, device="cuda")
    d_taps = ctx.upload(taps)
    sampled = sorted({0, 1, 37, 63, S - 1} & set(range(S)))
    torch.cuda.synchronize()
    counts = {}

    def fused_step():
        counts["n"] = obj.process_dev(x.data_ptr(), N, N, y.data_ptr(), opitch)

    def composed_step():
        mod.process_dev(x.data_ptr(), N, N, sym.data_ptr(), N)
        ctx.check(ctx.L.csdr_amd_plain_interpolate_cc(ctx.h, sym.data_ptr(), stuffed.data_ptr(), S, N, N, N * I, I), "plain_interpolate_cc")
        counts["n"] = ctx.check(ctx.L.csdr_amd_apply_real_fir_cc(ctx.h, stuffed.data_ptr(), y.data_ptr(), S, N * I, N * I, opitch, d_taps.ptr, T), "apply_real_fir_cc")

    def timed(step, before=None):
        if before:
            before()
        step()                                                                  # from the reset state: the outputs --verify checks
        ctx.sync()
        n_first = counts["n"]
        first = {k: y[k, :n_first].cpu().numpy().view(np.complex64).reshape(-1) for k in sampled} if args.verify else None
        for _ in range(args.warmup):
            step()
        ctx.sync(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.timer_start()
        for _ in range(args.steps):
            step()
        ev_ms = ctx.timer_stop_ms()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, ev_ms / args.steps, first

    def use(generic):
        obj.force_generic(generic); obj.reset()

    g_wall, g_ms, g_first = timed(fused_step, lambda: use(True))
    g_name = obj.kernel_name()
    c_wall, c_ms, c_first = timed(composed_step)
    c_name = csdr_amd.lib().csdr_amd_fir_last_instance().decode() if hasattr(csdr_amd.lib(), "csdr_amd_fir_last_instance") else "fir"
    wall, k_ms, first = timed(fused_step, lambda: use(False))
    name = obj.kernel_name()
    n_out = S * counts["n"]                                                     # output samples per step (a step behind the first: N I per channel)
    out_bytes = 8 * n_out
    t_hbm = out_bytes / bc.HBM_PEAK_GBS / 1e9
    composed_bytes = S * (N + 8 * N + 2 * 8 * N * I) + out_bytes                # bytes in, symbols out; symbols in, stuffed out; stuffed in, output out
    res = {"metric": "MS/s out, pulse-shaped PSK transmitter (psk_modulator %d | plain_interpolate x %d | RRC %d taps) x N channels" % (P, I, T),
           "value": round(n_out * args.steps / wall / 1e6, 1), "unit": "MS/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(wall / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "generated",
           "config": {"workload": "pulse shaping transmit, fused, batched", "channels": S, "symbols_per_channel": N, "n_psk": P, "interpolation": I, "taps": T,
                      "beta": args.beta, "distinct_rows": 64, "output_samples_per_step": n_out},
           "roofline": {"bound": "hbm store", "kernel": name, "dominant_kernel": "k_pulsetx_poly", "kernel_avg_ms": round(k_ms, 4),
                        "bound_hbm_ms": round(t_hbm * 1e3, 4), "algorithmic_bytes_per_step": out_bytes + S * N, "hbm_peak_GBs": bc.HBM_PEAK_GBS,
                        "frac": round(t_hbm / (k_ms * 1e-3), 4),
                        "yardstick": {"what": "k_psk31tx_shape on the same kind of machine, the same store-bound shape (DESIGN 4n)", "frac": 0.71}},
           "generic": {"kernel": g_name, "kernel_avg_ms": round(g_ms, 4), "ms_per_step": round(g_wall / args.steps * 1e3, 4),
                       "fused_over_generic_time": round(k_ms / g_ms, 4), "frac": round(t_hbm / (g_ms * 1e-3), 4)},
           "composed": {"what": "psk_modulator_u8_c -> plain_interpolate_cc -> apply_real_fir_cc (decimation 1) on the same buffers", "fir_kernel": c_name,
                        "avg_ms": round(c_ms, 4), "ms_per_step": round(c_wall / args.steps * 1e3, 4), "bytes_per_step": composed_bytes,
                        "bytes_over_fused": round(composed_bytes / (out_bytes + S * N), 3), "fused_over_composed_time": round(k_ms / c_ms, 4)}}
    if k_ms > c_ms:
        res["note"] = "the fused kernel (%.4f ms) is SLOWER than the composed path (%.4f ms) in this run" % (k_ms, c_ms)
    if args.verify:
        ok_bits, ok_gate = True, True
        K = (T + I - 1) // I
        for k in sampled:
            c = pm.symbols(P)[X[k % 64]]
            want = pm.shape32(c, I, taps)
            ok_bits = ok_bits and first[k].shape == want.shape and np.array_equal(first[k].view(np.uint32), want.view(np.uint32))
            ok_bits = ok_bits and np.array_equal(g_first[k].view(np.uint32), want.view(np.uint32))
            w64, mr, mi = pm.shape64(c, I, taps)
            ok_gate = ok_gate and pm.within(first[k], w64, pm.dot_gate(K, mr), pm.dot_gate(K, mi)) and pm.within(c_first[k], w64, pm.dot_gate(T, mr), pm.dot_gate(T, mi))
        res["verify"] = {"sampled_channels": sampled, "against": "tests/pulse_model.py: fused and generic bit for bit against the float32 model, fused and composed within "
                                                                   "their dot-product gates against float64", "ok": bool(ok_bits and ok_gate)}
    if not args.no_cpu_baseline:
        cb = cpu_baseline(X, P, I, taps)
        if cb:
            cb["speedup"] = round(res["value"] / cb["value"], 2)
        res["cpu_baseline"] = cb
    print(json.dumps(res), flush=True)
    ctx.close()
    if args.verify and not res["verify"]["ok"]:
        raise SystemExit("verification failed")


if __name__ == "__main__":
    main()
