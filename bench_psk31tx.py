#!/usr/bin/env python3
"""bench_psk31tx.py -- the BPSK31 transmit chain, batched: psk31_varicode_encoder_u8_u8 | differential_encoder_u8_u8 | psk_modulator_u8_c 2 |
psk31_interpolate_sine_cc 256 for `--channels` channels per call through one csdr_amd_psk31tx object (psk31tx.hip).

One step = one process call over all channels (`--chars` characters each; text and output resident in HBM, every channel's state carries over).  The
fused path (k_psk31tx_plan + k_psk31tx_shape) and the generic kernel (k_psk31tx_generic) are both timed; the run exits non-zero when the fused path is
slower than the generic one.  Roofline: the chain is store bound, frac is the HBM store bound (output bytes / 8 TB/s) over the measured time per step;
the text and the packed states are under 1 % of the output.  `yardstick` repeats the README's figure for a read-plus-write stream on the same machine
(gain_ff / k_squelch_*: 0.70 of HBM) to read the fraction against; no target is set.

    python bench_psk31tx.py [--gpus 1] [--steps K] [--warmup W] [--channels 4096] [--chars 64] [--interpolation 256] [--verify] [--no-cpu-baseline]
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


def texts(n_distinct, n_chars):
    """n_distinct texts of n_chars printable characters (a fixed generator: the same every run)"""
    import numpy as np
    rng = np.random.default_rng(31)
    return rng.integers(32, 127, (n_distinct, n_chars)).astype(np.uint8)


def cpu_baseline(T, interpolation, threads=16):
    """the reference's four functions through libcsdr_ref.so, one channel per task on `threads` threads (ctypes releases the GIL).  MS/s of output."""
    if not os.path.exists(REF_LIB):
        return None
    import numpy as np
    import test_psk31tx_cpu as tc
    L = tc.bind_tx(C.CDLL(REF_LIB))

    def one(t):
        bits, _ = tc.ref_varicode(L, t.tobytes())
        st, _ = tc.ref_codec(L, bits, 1)
        out, _ = tc.ref_shape(L, tc.ref_modulate(L, st, 2), interpolation)
        return out.size
    rows = [np.ascontiguousarray(T[k % T.shape[0]]) for k in range(16 * threads)]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        n_out = sum(ex.map(one, rows))
    wall = time.perf_counter() - t0
    return {"value": round(n_out / wall / 1e6, 2), "unit": "MS/s out", "threads": threads, "channels": len(rows),
            "what": "psk31_varicode_encoder_u8_u8 + differential_codec + psk_modulator_u8_c + psk31_interpolate_sine_cc of libcsdr_ref.so (-O3 -ffast-math)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--chars", type=int, default=64)
    ap.add_argument("--interpolation", type=int, default=256)
    ap.add_argument("--verify", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_psk31tx.py measures one GPU (--gpus 1)")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_psk31tx.py needs an MI355X; there is no CPU fallback")
    import csdr_amd
    import psk31tx_model as tm
    ctx = csdr_amd.Context(0)
    S, N, I = args.channels, args.chars, args.interpolation
    T = texts(64, N)
    x = torch.from_numpy(T).cuda().repeat((S + 63) // 64, 1)[:S].contiguous()     # channel k sends text k % 64
    obj = ctx.psk31_tx(S, 2, I)
    opitch = obj.max_out(N)
    y = torch.empty((S, opitch, 2), dtype=torch.float32, device="cuda")
    cnt = torch.empty(S, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def step():
        obj.process_dev(x.data_ptr(), N, None, N, y.data_ptr(), opitch, cnt.data_ptr())

    def timed(generic):
        obj.force_generic(generic)
        obj.reset()
        step()                                                                  # from the reset state: the outputs --verify checks
        ctx.sync()
        first = None
        if args.verify:
            c = cnt.cpu().numpy()
            first = {k: y[k, :c[k]].cpu().numpy().view(np.complex64).reshape(-1) for k in (0, 1, 37, 63, S - 1)}
        for _ in range(args.warmup):
            step()
        ctx.sync(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.timer_start()
        for _ in range(args.steps):
            step()
        ev_ms = ctx.timer_stop_ms()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, ev_ms / args.steps, obj.kernel_name(), first

    g_wall, g_ms, g_name, g_first = timed(True)
    wall, k_ms, name, first = timed(False)
    n_out = int(cnt.sum().item())                                               # output samples per step
    out_bytes = 8 * n_out
    t_hbm = out_bytes / bc.HBM_PEAK_GBS / 1e9
    res = {"metric": "MS/s out, BPSK31 transmit chain (varicode | differential | BPSK | sine shaping x %d) x N channels" % I,
           "value": round(n_out * args.steps / wall / 1e6, 1), "unit": "MS/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(wall / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "generated",
           "config": {"workload": "psk31 transmit, fused, batched", "channels": S, "chars_per_channel": N, "interpolation": I, "distinct_texts": 64,
                      "output_samples_per_step": n_out},
           "roofline": {"bound": "hbm store", "kernel": name, "dominant_kernel": "k_psk31tx_shape", "kernel_avg_ms": round(k_ms, 4),
                        "bound_hbm_ms": round(t_hbm * 1e3, 4), "algorithmic_bytes_per_step": out_bytes, "hbm_peak_GBs": bc.HBM_PEAK_GBS,
                        "frac": round(t_hbm / (k_ms * 1e-3), 4),
                        "yardstick": {"what": "gain_ff / k_squelch_* on the same machine, a read-plus-write stream (README)", "frac": 0.70}},
           "generic": {"kernel": g_name, "kernel_avg_ms": round(g_ms, 4), "ms_per_step": round(g_wall / args.steps * 1e3, 4),
                       "fused_over_generic_time": round(k_ms / g_ms, 4), "frac": round(t_hbm / (g_ms * 1e-3), 4)}}
    if args.verify:
        ok = True
        for k, got in first.items():
            want = tm.chain(T[k % 64].tobytes(), 2, I)["shape"]
            ok = ok and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
            ok = ok and np.array_equal(g_first[k].view(np.uint32), want.view(np.uint32))
        res["verify"] = {"sampled_channels": sorted(first), "against": "tests/psk31tx_model.py, bit for bit, fused and generic", "ok": bool(ok)}
    if not args.no_cpu_baseline:
        cb = cpu_baseline(T, I)
        if cb:
            cb["speedup"] = round(res["value"] / cb["value"], 2)
        res["cpu_baseline"] = cb
    print(json.dumps(res), flush=True)
    ctx.close()
    if k_ms > g_ms:
        raise SystemExit("the fused path (%.4f ms) is slower than the generic kernel (%.4f ms)" % (k_ms, g_ms))
    if args.verify and not res["verify"]["ok"]:
        raise SystemExit("verification failed")


if __name__ == "__main__":
    main()
