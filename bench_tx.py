#!/usr/bin/env python3
"""bench_tx.py -- the fused transmit bank (txmod.hip): `--streams` s16 audio streams x `--block` samples per step through one csdr_amd_txbank object,
    convert_s16_f | gain_ff | fmmod_fc | fir_interpolate_cc 50 (firdes_lowpass_f(801, 0.5 / 50)) | shift_addition_cc r_s | convert_f_u8
each stream with its own shift rate: the mirror of the receiver front end's headline shape (2.4 MS/s out of 48 kS/s audio per stream).  Legs: u8 output
(the headline), cf32 output, AM (dsb_fc | add_dcoffset_cc), and the generic kernel.

The comparison leg times the composed path in the same run, on the same modulated baseband with ONE shared shift rate:
csdr_amd_interp_process -> csdr_amd_shift_cc -> csdr_amd_convert_f_u8.  The fused bank writes 2 bytes per output sample where the composed path moves
8 + 16 + 10 = 34, so `fused_below_composed` has to be true; the script exits with status 1 when it is not, or when --verify finds a deviation.

Two bounds are named: HBM (the output bytes plus the audio read, at 8 TB/s) and fp32 (K taps x 2 components x 2 flop per output at the 157.3 TF/s peak).

    python bench_tx.py [--gpus 1] [--steps K] [--warmup W] [--streams 1024] [--block 48000] [--verify] [--no-composed]
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

I, T = 50, 801
GAIN, Q = 0.8, 0.0
LEGS = {"fm_u8": ("fm", "u8", False), "fm_cf32": ("fm", "cf32", False), "am_u8": ("am", "u8", False), "fm_u8_generic": ("fm", "u8", True)}


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--block", type=int, default=48000)
    ap.add_argument("--verify", action="store_true")
    ap.add_argument("--no-composed", action="store_true")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_tx.py measures one GPU (--gpus 1)")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tx.py needs an MI355X; there is no CPU fallback")
    import csdr_amd
    import txmod_model as tm
    ctx = csdr_amd.Context(0)
    S, N = args.streams, args.block
    K = (T - 1 + I - 1) // I
    n_out = (N - K) * I
    pitch = (n_out + 7) & ~7
    n_sig = min(16, S)
    taps = ctx.firdes_lowpass_f(T, 0.5 / I)
    rates = np.linspace(-0.45, 0.45, S).astype(np.float32) if S > 1 else np.array([0.11], np.float32)
    audio = tm.bank_audio(n_sig, N, 900)
    x = torch.from_numpy(audio).cuda().repeat((S + n_sig - 1) // n_sig, 1)[:S].contiguous()                  # [S, N] s16
    big = torch.empty((S, 2 * pitch), dtype=torch.float32, device="cuda")                                    # cf32 rows: the fused cf32 leg, the composed path's interpolator
    out_u8 = torch.empty((S, 2 * pitch), dtype=torch.uint8, device="cuda")
    objs = {}
    for name, (mode, fmt, generic) in LEGS.items():
        objs[name] = ctx.txbank(S, mode, I, taps, rates, gain=GAIN, q_value=Q, out_format=fmt, max_in_samples=N)
        objs[name].force_generic(generic)

    def step(name):
        o = objs[name]
        o.reset()                                                             # every step sends the same stream from a fresh state
        dst = out_u8 if LEGS[name][1] == "u8" else big
        got = o.process_dev(x.data_ptr(), N, N, dst.data_ptr(), pitch)
        assert got == n_out, (got, n_out)

    calls = [(name, (lambda name=name: step(name))) for name in LEGS]

    composed = None
    if not args.no_composed:
        # the same modulated baseband, made once by the library's own operators
        xf = torch.empty((S, N), dtype=torch.float32, device="cuda")
        bb = torch.empty((S, 2 * N), dtype=torch.float32, device="cuda")
        ph = torch.zeros(S, dtype=torch.float32, device="cuda")
        ctx.check(ctx.L.csdr_amd_convert_s16_f(ctx.h, x.data_ptr(), xf.data_ptr(), S * N), "convert_s16_f")
        ctx.check(ctx.L.csdr_amd_gain_ff(ctx.h, xf.data_ptr(), xf.data_ptr(), S * N, GAIN), "gain_ff")
        ctx.check(ctx.L.csdr_amd_fmmod_fc(ctx.h, xf.data_ptr(), bb.data_ptr(), S, N, N, N, ph.data_ptr()), "fmmod_fc")
        ctx.sync()
        interp = csdr_amd.Interpolator(ctx, I, taps, S)
        shifted = torch.empty((S, 2 * pitch), dtype=torch.float32, device="cuda")
        shared_rate = float(rates[S // 3])
        import ctypes as C

        def composed_step():
            interp.reset()
            got = interp.process_dev(bb.data_ptr(), N, N, big.data_ptr(), pitch)
            assert got == n_out, (got, n_out)
            p0 = C.c_float(0.0)
            ctx.check(ctx.L.csdr_amd_shift_cc(ctx.h, csdr_amd.SHIFT["addition"], shared_rate, C.byref(p0), big.data_ptr(), shifted.data_ptr(), S, n_out, pitch, pitch, 1024, 0),
                      "shift_cc")
            ctx.check(ctx.L.csdr_amd_convert_f_u8(ctx.h, shifted.data_ptr(), out_u8.data_ptr(), S * 2 * pitch), "convert_f_u8")
        calls.append(("composed", composed_step))

    sampled = sorted({k for k in (0, 1, S // 2 + 1, S - 1) if k < S})
    first = {}
    if args.verify:
        for name in LEGS:
            step(name); ctx.sync(); torch.cuda.synchronize()
            dst = out_u8 if LEGS[name][1] == "u8" else big
            first[name] = {k: dst[k].cpu().numpy().copy() for k in sampled}
    for _ in range(args.warmup):
        for _, f in calls:
            f()
    ctx.sync(); torch.cuda.synchronize()
    times = {cname: [] for cname, _ in calls}
    for _ in range(args.steps):                                               # interleaved repeats, one HIP-event pair around every step
        for cname, f in calls:
            ctx.timer_start(); f(); times[cname].append(ctx.timer_stop_ms())
    med = {k: median(v) for k, v in times.items()}
    ctx.sync(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step("fm_u8")
    ctx.sync(); torch.cuda.synchronize()
    wall = time.perf_counter() - t0

    flops = 4.0 * K * S * n_out
    t_fp32_ms = flops / (bc.FP32_PEAK_TFLOPS * 1e12) * 1e3
    shapes = {}
    for name, (mode, fmt, generic) in LEGS.items():
        algo = S * n_out * (2 if fmt == "u8" else 8) + 2 * S * N
        t_hbm_ms = algo / bc.HBM_PEAK_GBS / 1e9 * 1e3
        t = med[name]
        shapes[name] = {"mode": mode, "out_format": fmt, "kernel": objs[name].kernel_name(), "ms": round(t, 3), "min_ms": round(min(times[name]), 3),
                        "max_ms": round(max(times[name]), 3), "out_MSps": round(S * n_out / t / 1e3, 1), "algorithmic_bytes_per_step": algo,
                        "bound_hbm_ms": round(t_hbm_ms, 4), "frac_of_hbm_bound": round(t_hbm_ms / t, 4), "bound_fp32_ms": round(t_fp32_ms, 4),
                        "frac_of_fp32_bound": round(t_fp32_ms / t, 4)}
    head = shapes["fm_u8"]
    binding = "fp32" if head["bound_fp32_ms"] >= head["bound_hbm_ms"] else "hbm"
    res = {"metric": "output MS/s, %d FM transmit streams (s16 audio -> fmmod_fc -> x%d interpolation -> per-stream shift -> u8 IQ)" % (S, I),
           "value": round(S * n_out * args.steps / wall / 1e6, 1), "unit": "MS/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(wall / args.steps * 1e3, 3), "event_ms_per_step": head["ms"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "f32", "data": "generated",
           "config": {"workload": "fused transmit bank", "streams": S, "audio_samples_per_stream": N, "interpolation": I, "taps": T, "taps_per_branch": K,
                      "outputs_per_stream": n_out, "gain": GAIN, "distinct_audio_rows": n_sig, "shift_rates": "linspace(-0.45, 0.45, streams)"},
           "roofline": {"bound": binding, "kernel": head["kernel"], "kernel_avg_ms": head["ms"],
                        "timer": "HIP events around every step (a state reset, the audio-rate modulator, the chunk seeds, k_tx_up, the history copy), medians over interleaved repeats of every leg",
                        "reason": "2 bytes written per output sample and %d real-by-complex taps per output: at u8 the fp32 rate binds, at cf32 HBM" % K,
                        "algorithmic_bytes_per_step": head["algorithmic_bytes_per_step"], "hbm_peak_GBs": bc.HBM_PEAK_GBS, "bound_hbm_ms": head["bound_hbm_ms"],
                        "flop_per_step": flops, "fp32_peak_TFLOPS": bc.FP32_PEAK_TFLOPS, "bound_fp32_ms": head["bound_fp32_ms"],
                        "frac": head["frac_of_fp32_bound"] if binding == "fp32" else head["frac_of_hbm_bound"]},
           "shapes": shapes}
    ok = True
    if not args.no_composed:
        t = med["composed"]
        res["composed"] = {"what": "csdr_amd_interp_process -> csdr_amd_shift_cc (one shared rate) -> csdr_amd_convert_f_u8 on the same FM baseband",
                           "ms": round(t, 3), "min_ms": round(min(times["composed"]), 3), "max_ms": round(max(times["composed"]), 3),
                           "interp_kernel": interp.kernel_name(), "bytes_moved_per_output": 34, "fused_over_composed_time": round(head["ms"] / t, 4)}
        res["fused_below_composed"] = bool(head["ms"] < t)
        ok = ok and res["fused_below_composed"]
    if args.verify:
        import oracle
        port = oracle.port()
        ver = {}
        for name, (mode, fmt, generic) in LEGS.items():
            worst_rms = worst_share = 0.0
            worst_byte = 0
            for k in sampled:
                want = tm.bank_expected(port, audio[k % n_sig], mode, GAIN, Q, I, taps, [(None, float(rates[k]))], fmt)
                if fmt == "u8":
                    got = first[name][k][:2 * n_out].reshape(-1, 2)
                    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
                    worst_byte = max(worst_byte, int(d.max())); worst_share = max(worst_share, float(np.mean(d != 0)))
                else:
                    got = first[name][k][:2 * n_out].view(np.complex64)
                    worst_rms = max(worst_rms, tm.rm.relrms(got, want))
            good = bool(worst_byte <= 1 and worst_share <= 1e-3) if fmt == "u8" else bool(worst_rms <= 1e-5)
            ver[name] = ({"largest_byte_difference": worst_byte, "largest_share_of_bytes_differing": worst_share, "gate": "every byte within 1, share <= 1e-3"}
                         if fmt == "u8" else {"largest_relative_rms": worst_rms, "gate": 1e-5})
            ver[name]["ok"] = good
            ok = ok and good
        same = all(np.array_equal(first["fm_u8"][k], first["fm_u8_generic"][k]) for k in sampled)
        ver["fused_equals_generic_bits"] = bool(same)
        ver["sampled_streams"] = sampled
        ver["ok"] = bool(all(v["ok"] for v in ver.values() if isinstance(v, dict)) and same)
        ok = ok and ver["ok"]
        res["verify"] = ver
    print(json.dumps(res), flush=True)
    for o in objs.values():
        o.close()
    ctx.close()
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
