#!/usr/bin/env python3
"""bench_pulserx.py -- the pulse-shaped symbol receiver, batched: pulse_shaping_filter_cc (matched filter) | timing_recovery_cc GARDNER --add_q | realpart_cf |
gain_ff | generic_slicer_f_u8 for `--channels` channels per call through one csdr_amd_pulserx object (modem.hip).

One step = one process call over all channels (`--samples` complexf each, resident in HBM; every channel's tail and loop state carry over).  Two shapes:
RRC 65 taps at 8 samples per symbol (the transmit bench's shape) and the COSINE pulse at 256 samples per symbol (BPSK31's shape, 513 taps).  The signal is
QPSK from the transmit object's CPU walk, 64 distinct rows with a timing offset of row % sps samples, amplitudes stepped per row so that the loop corrects,
and noise 20 dB down.  Timed in the same run, on the same buffers: k_pulserx_tiled at every `lanes` choice, k_pulserx_generic, and the composed device path
(csdr_amd_apply_real_fir_cc, then csdr_amd_psk31 TIMING..TIMING, then the flat realpart_cf / gain_ff / generic_slicer_f_u8 calls: the filtered stream and
the symbols written to and read from HBM; the flat calls take no count per channel and run over whole rows of max_out symbols, about twice those produced).  Reported: the HBM bound (input bytes / 8 TB/s), the multiply-adds of both paths, and the measured ratio fused /
composed, which is not fixed in advance: a fused kernel slower than the composed path is said so in `note` and the run still exits zero.

    python bench_pulserx.py [--gpus 1] [--steps K] [--warmup W] [--channels 4096] [--samples 131072] [--shape rrc|cosine|both] [--verify]
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

SHAPES = {"rrc": dict(sps=8, taps=65, beta=0.35, rms=1.4), "cosine": dict(sps=256, taps=513, beta=None, rms=0.18)}
LANES = (1, 2, 4, 8, 16)
GAIN, N_SYMBOLS = 0.7, 4


def make_rows(csdr_amd, np, sps, taps, n, rms, rows=64):
    """[rows, n] complex64: random QPSK through the transmit object's walk, row k delayed by k % sps samples, RMS behind the matched filter
    rms (1 + 0.1 (k % 4)), white noise 20 dB below the signal"""
    rng = np.random.default_rng(41 + sps)
    n_sym = n // sps + (taps.size + sps - 1) // sps + 2
    t64 = taps.astype(np.float64)
    x = np.zeros((rows, n), np.complex64)
    for k in range(rows):
        y = csdr_amd.pulsetx_debug_walk(rng.integers(0, 4, n_sym).astype(np.uint8), taps, 4, sps)
        d = k % sps
        row = np.zeros(n, np.complex128)
        row[d:] = y[:n - d]
        p = np.mean(np.abs(row) ** 2)
        row += np.sqrt(p / 100 / 2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        probe = np.correlate(row[:16384], t64, "valid")
        x[k] = (row * (rms * (1 + 0.1 * (k % 4)) / np.sqrt(np.mean(np.abs(probe) ** 2)))).astype(np.complex64)
    return x


def run_shape(args, ctx, csdr_amd, np, torch, name):
    import pulserx_model as rm
    sh = SHAPES[name]
    S, N, D, T = args.channels, args.samples, sh["sps"], sh["taps"]
    taps = csdr_amd.firdes_cosine_f(D) if sh["beta"] is None else csdr_amd.firdes_rrc_f(T, D, sh["beta"])
    X = make_rows(csdr_amd, np, D, taps, N, sh["rms"])
    x = torch.from_numpy(X.view(np.float32).reshape(64, N, 2)).cuda().repeat((S + 63) // 64, 1, 1)[:S].contiguous()   # channel k receives row k % 64
    par = csdr_amd.pulserx_params(taps, "GARDNER", D, 0.5, 2.0, True, GAIN, N_SYMBOLS, False)
    obj = ctx.pulse_rx(par, S, "filter", "slice")
    opitch = obj.max_out(N)
    out = torch.zeros((S, opitch), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(S, dtype=torch.int32, device="cuda")
    # the composed path's objects and intermediate streams
    timing = ctx.psk31(csdr_amd.psk31_params(algorithm="GARDNER", decimation=D, loop_gain=0.5, max_error=2.0, use_q=True), S, "timing", "timing")
    n_f = N - T + 1
    spitch = timing.max_out(n_f)
    filtered = torch.empty((S, n_f, 2), dtype=torch.float32, device="cuda")
    symbols = torch.zeros((S, spitch, 2), dtype=torch.float32, device="cuda")  # (zeros: the flat calls below also run over the rows' unwritten ends)
    soft = torch.zeros((S, spitch), dtype=torch.float32, device="cuda")
    sliced = torch.zeros((S, spitch), dtype=torch.uint8, device="cuda")
    ccounts = torch.zeros(S, dtype=torch.int32, device="cuda")
    d_taps = ctx.upload(taps)
    sampled = sorted({0, 1, 37, 63, S - 1} & set(range(S)))
    torch.cuda.synchronize()
    L = ctx.L

    def fused_step():
        obj.process_dev(x.data_ptr(), N, N, out.data_ptr(), opitch, counts.data_ptr())

    def composed_step():
        ctx.check(L.csdr_amd_apply_real_fir_cc(ctx.h, x.data_ptr(), filtered.data_ptr(), S, N, N, n_f, d_taps.ptr, T), "apply_real_fir_cc")
        timing.process_dev(filtered.data_ptr(), n_f, n_f, symbols.data_ptr(), spitch, ccounts.data_ptr())
        ctx.check(L.csdr_amd_realpart_cf(ctx.h, symbols.data_ptr(), soft.data_ptr(), S * spitch), "realpart_cf")
        ctx.check(L.csdr_amd_gain_ff(ctx.h, soft.data_ptr(), soft.data_ptr(), S * spitch, GAIN), "gain_ff")
        ctx.check(L.csdr_amd_generic_slicer_f_u8(ctx.h, soft.data_ptr(), sliced.data_ptr(), S, spitch, spitch, spitch, N_SYMBOLS), "generic_slicer_f_u8")

    def timed(step, before, grab):
        before()
        step()                                                                  # from the reset state: the outputs --verify checks
        ctx.sync()
        first = grab()
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

    def grab_fused():
        c = counts.cpu().numpy()
        return {k: out[k, :c[k]].cpu().numpy() for k in sampled}, int(c.astype(np.int64).sum())

    def grab_composed():
        c = ccounts.cpu().numpy()
        return {k: sliced[k, :c[k]].cpu().numpy() for k in sampled}, int(c.astype(np.int64).sum())

    def use(lanes, generic):
        obj.set_lanes(lanes); obj.force_generic(generic); obj.reset()

    runs = {}
    for lanes in LANES:
        wall, ms, first = timed(fused_step, lambda: use(lanes, False), grab_fused)
        runs[lanes] = dict(wall=wall, ms=ms, first=first, kernel=obj.kernel_name(), lanes=obj.lanes())
    g_wall, g_ms, g_first = timed(fused_step, lambda: use(0, True), grab_fused)
    g_name = obj.kernel_name()
    c_wall, c_ms, c_first = timed(composed_step, timing.reset, grab_composed)
    wall, k_ms, first = timed(fused_step, lambda: use(0, False), grab_fused)    # the default choice, last: what `value` reports
    name_k, default_lanes = obj.kernel_name(), obj.lanes()
    n_symbols_step = first[1]
    in_bytes = 8 * S * N
    t_hbm = in_bytes / bc.HBM_PEAK_GBS / 1e9
    composed_bytes = in_bytes + 2 * 8 * S * n_f + 8 * S * spitch + 3 * 4 * S * spitch + S * spitch
    res = {"shape": name, "kernel": name_k, "lanes": default_lanes, "channels": S, "samples_per_channel": N, "samples_per_symbol": D, "taps": T,
           "symbols_first_step": n_symbols_step, "ms_per_step": round(wall / args.steps * 1e3, 4), "kernel_avg_ms": round(k_ms, 4),
           "msamples_per_s": round(S * N * args.steps / wall / 1e6, 1),
           "bound_hbm_ms": round(t_hbm * 1e3, 4), "frac": round(t_hbm / (k_ms * 1e-3), 4), "input_bytes_per_step": in_bytes,
           "multiply_adds": {"fused_at_most": 3 * 2 * T * n_symbols_step, "fused_at_least": 2 * 2 * T * n_symbols_step, "composed": 2 * T * S * n_f},
           "by_lanes": {str(l): {"channels_per_wave": r["lanes"], "kernel": r["kernel"], "kernel_avg_ms": round(r["ms"], 4)} for l, r in runs.items()},
           "generic": {"kernel": g_name, "kernel_avg_ms": round(g_ms, 4), "fused_over_generic_time": round(k_ms / g_ms, 4)},
           "composed": {"what": "apply_real_fir_cc -> psk31 TIMING..TIMING -> realpart_cf -> gain_ff -> generic_slicer_f_u8 on the same buffers",
                        "avg_ms": round(c_ms, 4), "ms_per_step": round(c_wall / args.steps * 1e3, 4), "bytes_per_step": composed_bytes,
                        "flat_elements_per_step": S * spitch, "symbols_first_step": c_first[1],
                        "flat_note": "realpart_cf, gain_ff and the slicer run over whole rows of max_out symbols (the flat calls take no count per channel), "
                                     "%.2f x the symbols produced: the yardstick is that much slower in its last three launches than it need be"
                                     % (S * spitch / max(c_first[1], 1)),
                        "bytes_over_fused": round(composed_bytes / in_bytes, 3), "fused_over_composed_time": round(k_ms / c_ms, 4)}}
    best = min(runs, key=lambda l: runs[l]["ms"])
    res["best_lanes"] = {"asked": best, "kernel_avg_ms": round(runs[best]["ms"], 4)}
    if k_ms > c_ms:
        res["note"] = "the fused kernel (%.4f ms) is SLOWER than the composed path (%.4f ms) in this run" % (k_ms, c_ms)
    if args.verify:
        ok_walk = ok_model = True
        prefix = min(N, T + 3 * D // 2 + 300 * D)
        for k in sampled:
            want = csdr_amd.pulserx_debug_walk(par, "filter", "slice", X[k % 64])
            for f in [first[0], g_first[0]] + [r["first"][0] for r in runs.values()]:
                ok_walk = ok_walk and f[k].size == want.size and np.array_equal(f[k], want)
            m = rm.receive(X[k % 64][None, :prefix], taps, D, rm.GARDNER, True, 0.5, 2.0, rm.FILTER, rm.SLICE, GAIN, N_SYMBOLS, False)[0]
            ok_model = ok_model and m["bytes"].size > 0 and np.array_equal(first[0][k][:m["bytes"].size], m["bytes"])
        agree = float(np.mean([np.mean(c_first[0][k][:min(c_first[0][k].size, first[0][k].size)] == first[0][k][:min(c_first[0][k].size, first[0][k].size)])
                               for k in sampled]))
        res["verify"] = {"sampled_channels": sampled, "against": "both kernels and every lanes choice bit for bit against the CPU walk over the whole first call, and "
                                                                  "against tests/pulserx_model.py over the first 300 symbols", "ok": bool(ok_walk and ok_model),
                         "composed_bytes_equal_share": round(agree, 4)}
    obj.close(); timing.close()
    del x, out, filtered, symbols, soft, sliced
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=131072)
    ap.add_argument("--shape", choices=["rrc", "cosine", "both"], default="both")
    ap.add_argument("--verify", action="store_true")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_pulserx.py measures one GPU (--gpus 1)")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pulserx.py needs an MI355X; there is no CPU fallback")
    import csdr_amd
    ctx = csdr_amd.Context(0)
    shapes = ["rrc", "cosine"] if args.shape == "both" else [args.shape]
    per = [run_shape(args, ctx, csdr_amd, np, torch, s) for s in shapes]
    a = per[0]
    res = {"metric": "MS/s in, pulse-shaped symbol receiver (matched filter %d taps | timing_recovery_cc GARDNER %d --add_q | realpart | gain | slicer) x N channels"
                     % (a["taps"], a["samples_per_symbol"]),
           "value": a["msamples_per_s"], "unit": "MS/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": a["ms_per_step"],
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "generated",
           "config": {"workload": "pulse-shaped receive, fused, batched", "channels": a["channels"], "samples_per_channel": a["samples_per_channel"],
                      "distinct_rows": 64, "gain": GAIN, "n_symbols": N_SYMBOLS},
           "roofline": {"bound": "hbm load", "kernel": a["kernel"], "dominant_kernel": "k_pulserx_tiled", "kernel_avg_ms": a["kernel_avg_ms"],
                        "bound_hbm_ms": a["bound_hbm_ms"], "algorithmic_bytes_per_step": a["input_bytes_per_step"], "hbm_peak_GBs": bc.HBM_PEAK_GBS, "frac": a["frac"]},
           "shapes": per}
    notes = [p["note"] + " (%s)" % p["shape"] for p in per if "note" in p]
    if notes:
        res["note"] = "; ".join(notes)
    print(json.dumps(res), flush=True)
    ctx.close()
    if args.verify and not all(p["verify"]["ok"] for p in per):
        raise SystemExit("verification failed")


if __name__ == "__main__":
    main()
