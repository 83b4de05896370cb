#!/usr/bin/env python3
"""bench_passbands.py -- what a passband per channel costs: bandpass_fir_fft_cc for `--channels` streams x `--block` complex samples per step (CF32, resident in
HBM), `--taps` taps, and the SSB bank (filter | realpart_cf | agc_ff | limit_ff | convert_f_s16) on the same buffers, at bench_amssb.py's shape.

Four legs, interleaved, HIP-event times, medians and min .. max over `--steps` repeats:
    filter_shared        csdr_amd_fftfilt, one taps spectrum for all streams
    filter_per_stream    the same object with `--channels` distinct passbands (a table row per stream)
    bank_shared          csdr_amd_amssb in SSB mode, one passband
    bank_per_channel     the same with a passband per channel
With CSDR_AMD_LIB pointing at a build without the per-stream entry points only the shared legs run: the A/B of the shared path against the parent commit.

The prediction for the per-stream filter: consecutive windows of a stream go to consecutive waves of one XCD, so a stream's table row should come from HBM about
once per call: 8 N bytes (N: the window) on top of the 16 bytes per sample, 1.6 % at N = 4096 and 131072 samples.  The line holds the predicted and the
measured ratio.  --verify compares sampled channels of the timed per-stream configuration with shared-taps filters of those channels' taps, word for word, and
writes profiles/passbands_bench.json.

    python bench_passbands.py [--gpus 1] [--steps 7] [--warmup 1] [--channels 4096] [--block 131072] [--taps 79] [--fft 256] [--verify]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import bench_common as bc  # noqa: E402
from bench_amssb import signals, median  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--block", type=int, default=131072)
    ap.add_argument("--taps", type=int, default=79)
    ap.add_argument("--fft", type=int, default=256)
    ap.add_argument("--agc-block", type=int, default=1024)
    ap.add_argument("--verify", action="store_true")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_passbands.py measures one GPU (--gpus 1)")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_passbands.py needs an MI355X; there is no CPU fallback")
    import csdr_amd
    ctx = csdr_amd.Context(0)
    L = ctx.L
    have_rows = hasattr(L, "csdr_amd_fftfilt_create_per_stream")
    S, N, nt, fft, B = args.channels, args.block, args.taps, args.fft, args.agc_block
    inp = fft - nt + 1
    nb = N // inp
    m = nb * inp                                                              # the filter legs' samples per stream and call
    n_sig = min(64, S)
    X = signals(n_sig, N)
    x = torch.from_numpy(X.view(np.float32)).cuda().repeat((S + n_sig - 1) // n_sig, 1)[:S].contiguous()      # [S, 2 N] floats
    y = torch.empty_like(x)
    s16 = torch.empty((S, N), dtype=torch.int16, device="cuda")
    # distinct passbands: channel c's lower edge walks from -0.4 to 0.3, its width from 0.01 to 0.1
    c = np.arange(S)
    lo = -0.4 + 0.7 * c / max(S - 1, 1); hi = lo + 0.01 + 0.09 * ((c * 37) % S) / S
    bands = np.stack([lo, hi], axis=1).astype(np.float32)
    shared = ctx.firdes_bandpass_c(nt, 0.0, 0.1)
    legs = ["filter_shared", "bank_shared"]
    objs = {"filter_shared": csdr_amd._Handle(ctx, "fftfilt", L.csdr_amd_fftfilt_create(ctx.h, fft, shared.ctypes.data, nt, S, nb)),
            "bank_shared": csdr_amd.AmSsb(ctx, csdr_amd.amssb_params("ssb", B), S, taps=shared, fft_size=fft, max_samples_per_call=N)}
    if have_rows:
        rows = np.stack([ctx.firdes_bandpass_c(nt, float(a), float(b)) for a, b in bands])
        objs["filter_per_stream"] = csdr_amd.FftFilt(ctx, fft, rows, S, nb)
        objs["bank_per_channel"] = csdr_amd.AmSsb(ctx, csdr_amd.amssb_params("ssb", B), S, taps=shared, fft_size=fft, max_samples_per_call=N)
        o = objs["bank_per_channel"]
        for k in range(S):                                                    # (the first call gives every channel its table row)
            o._call("set_channel_taps", k, rows[k].ctypes.data, nt)
        legs = ["filter_shared", "filter_per_stream", "bank_shared", "bank_per_channel"]
    ctx.sync(); torch.cuda.synchronize()

    def prepare(leg):                                                         # every step filters the same stream from the zero state; not timed
        objs[leg].reset()

    def step(leg):
        if leg.startswith("filter"):
            o = objs[leg]
            ctx.check(o._fn("process")(o.h, x.data_ptr(), y.data_ptr(), nb, N, N), "fftfilt")
        else:
            objs[leg].process_dev(x.data_ptr(), N, N, s16.data_ptr(), None, N)

    verify = None
    if args.verify and have_rows:
        sampled = [k for k in (0, 1, 37, 63, S - 1) if k < S]
        prepare("filter_per_stream"); step("filter_per_stream"); ctx.sync(); torch.cuda.synchronize()
        got = {k: y[k, :2 * m].cpu().numpy().view(np.uint64).copy() for k in sampled}
        words = 0
        for k in sampled:                                                     # a shared filter with channel k's taps, on the timed configuration's input
            objs["filter_shared"]._fn("set_taps")(objs["filter_shared"].h, rows[k].ctypes.data, nt)
            prepare("filter_shared"); step("filter_shared"); ctx.sync(); torch.cuda.synchronize()
            words += int(np.count_nonzero(y[k, :2 * m].cpu().numpy().view(np.uint64) != got[k]))
        objs["filter_shared"]._fn("set_taps")(objs["filter_shared"].h, shared.ctypes.data, nt)
        verify = {"sampled_channels": sampled, "samples_per_channel": m, "words_differing_from_shared_filters": words, "ok": words == 0}
    for _ in range(args.warmup):
        for leg in legs:
            prepare(leg); step(leg)
    ctx.sync(); torch.cuda.synchronize()
    times = {leg: [] for leg in legs}
    for _ in range(args.steps):                                               # interleaved repeats, one HIP-event pair around every leg's call
        for leg in legs:
            prepare(leg)
            ctx.timer_start(); step(leg); times[leg].append(ctx.timer_stop_ms())
    out = {leg: {"ms": round(median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)} for leg, t in times.items()}
    out["filter_shared"]["kernel"] = objs["filter_shared"].kernel_name()
    win = L.csdr_amd_fftfilt_window(objs["filter_shared"].h)
    t = out["filter_shared"]["ms"]
    algo = 16 * S * m
    res = {"metric": "MS/s, bandpass_fir_fft_cc x N streams, shared taps", "value": round(S * m / t / 1e3, 1), "unit": "MS/s", "n_gpus": 1, "steps": args.steps,
           "warmup": args.warmup, "higher_is_better": True, "dtype": "f32", "data": "generated", "library": os.environ.get("CSDR_AMD_LIB") or "this tree",
           "config": {"channels": S, "block_samples_per_channel": N, "filter_samples_per_channel": m, "taps": nt, "fft_size": fft, "window": win, "agc_block": B,
                      "distinct_signals": n_sig, "distinct_passbands": S if have_rows else 1},
           "roofline": {"bound": "hbm", "algorithmic_bytes_per_step": algo, "hbm_peak_GBs": bc.HBM_PEAK_GBS, "bound_hbm_ms": round(algo / bc.HBM_PEAK_GBS / 1e6, 4),
                        "frac": round(algo / bc.HBM_PEAK_GBS / 1e6 / t, 4),
                        "timer": "HIP events around every leg's call (the reset in front is not timed), medians and min .. max over interleaved repeats"},
           "legs": out}
    if have_rows:
        res["per_stream_over_shared"] = {"predicted": round(1 + 8.0 * win / (16.0 * m), 4),
                                         "filter_measured": round(out["filter_per_stream"]["ms"] / out["filter_shared"]["ms"], 4),
                                         "bank_measured": round(out["bank_per_channel"]["ms"] / out["bank_shared"]["ms"], 4)}
    if verify is not None:
        res["verify"] = verify
    print(json.dumps(res), flush=True)
    if args.verify and have_rows:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "passbands_bench.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
    for o in objs.values():
        o.close()
    ctx.close()


if __name__ == "__main__":
    main()
