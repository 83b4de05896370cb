#!/usr/bin/env python3
"""bench_noise.py -- the batched AWGN channel: awgn_cc for `--channels` channels per call through one csdr_amd_noise object (noise.hip), each channel
with its own Philox stream and its own SNR.

One step = one call over all channels (`--block` complex samples each, resident in HBM; every channel's position carries over from step to step).
Three paths are timed, alternating, in the same run:
  fused     csdr_amd_noise_awgn_cc: the noise is generated, scaled and added in one kernel and never reaches memory (8 B read + 8 B written per sample)
  generate  csdr_amd_noise_generate: gaussian_noise_c alone (8 B written per sample)
  composed  csdr_amd_noise_generate into HBM, then the flat csdr_amd_awgn_cc on those rows (8 written, then 16 read + 8 written: 32 B per sample)
Each against its HBM bound (8 TB/s spec; the measured float4 copy rate of 6.29 TB/s is reported beside it) and against a VALU bound: the VALU instructions
per Philox block (two samples) counted in the gfx950 ISA of this build -- k_noise_gauss<awgn> 261, k_noise_gauss 239, of which 19 v_mad_u64_u32 (taken as
quarter rate: 4 slots), 16 FP64 and 2 transcendental (2 slots each) -- so 336 and 314 issue slots, at 256 CUs x 4 SIMDs x 32 lanes per clock x 2.4 GHz.
The weights of the slow instructions are assumptions, so the VALU bound is a paper figure; the larger bound's time over the measured step is `frac`, and the
measured generate-against-fused ratio says in practice what the reads cost (a kernel bound by HBM alone would lose them in proportion).

    python bench_noise.py [--gpus 1] [--steps K] [--warmup W] [--channels 4096] [--block 131072] [--verify]
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

VALU_SLOTS = {"fused": 336, "generate": 314, "composed": 314}      # issue slots per Philox block (see above)
LANES_PER_S = 256 * 4 * 32 * 2.4e9
HBM_COPY_GBS = 6290.0            # the measured float4 copy rate
SEED = 2024
SAMPLED = 4                      # rows --verify compares
SPAN = 4096                      # samples at each end of a sampled row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--block", type=int, default=131072)
    ap.add_argument("--verify", action="store_true")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_noise.py measures one GPU (--gpus 1)")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_noise.py needs an MI355X; there is no CPU fallback")
    import csdr_amd
    ctx = csdr_amd.Context(0)
    L = ctx.L
    S, N = args.channels, args.block
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    x = torch.randn((S, N, 2), dtype=torch.float32, device="cuda", generator=g)
    y = torch.empty((S, N, 2), dtype=torch.float32, device="cuda")
    nz = torch.empty((S, N, 2), dtype=torch.float32, device="cuda")
    snr = np.linspace(-10.0, 40.0, S).astype(np.float32)
    obj = ctx.noise(S, "gaussian", SEED, snr_db=snr)
    gains = np.array([obj.get_gains(ch) for ch in range(S)], np.float32)
    d_a = torch.from_numpy(np.ascontiguousarray(gains[:, 0])).cuda(); d_g = torch.from_numpy(np.ascontiguousarray(gains[:, 1])).cuda()
    torch.cuda.synchronize()

    def fused():
        obj.awgn_cc_dev(x.data_ptr(), N, N, y.data_ptr(), N)

    def generate():
        obj.generate_dev(nz.data_ptr(), N, N)

    def composed():
        obj.generate_dev(nz.data_ptr(), N, N)
        ctx.check(L.csdr_amd_awgn_cc(ctx.h, x.data_ptr(), nz.data_ptr(), y.data_ptr(), S, N, N, N, N, d_a.data_ptr(), d_g.data_ptr()), "awgn_cc")

    def timed(fn, steps):
        ctx.timer_start()
        for _ in range(steps):
            fn()
        return ctx.timer_stop_ms() / steps

    ver = None
    if args.verify:
        obj.reset()
        fused(); ctx.sync()
        y_fused = y.clone()
        kernel = obj.kernel_name()
        obj.reset()
        composed(); ctx.sync(); torch.cuda.synchronize()
        same = bool(torch.equal(y_fused.view(torch.int32), y.view(torch.int32)))
        rows = sorted(set(int(v) for v in np.linspace(0, S - 1, SAMPLED)))
        ok = same
        for k in rows:
            xr = x[k].cpu().numpy().view(np.complex64).ravel()
            yr = y_fused[k].cpu().numpy().view(np.complex64).ravel()
            nr = nz[k].cpu().numpy().view(np.complex64).ravel()
            for lo in (0, N - min(SPAN, N)):
                m = min(SPAN, N)
                want = csdr_amd.noise_debug_walk("gaussian", SEED, k, lo, x=xr[lo:lo + m], snr_db=float(snr[k]))
                ok = ok and bool(np.array_equal(yr[lo:lo + m].view(np.uint32), want.view(np.uint32)))
                ok = ok and bool(np.array_equal(nr[lo:lo + m].view(np.uint32), csdr_amd.noise_debug_walk("gaussian", SEED, k, lo, m).view(np.uint32)))
        ver = {"rows": rows, "samples_per_row_end": min(SPAN, N), "fused_equals_composed_bits": same, "bits_equal_cpu_walk": ok, "ok": ok, "kernel": kernel}
    for fn in (fused, generate, composed):
        for _ in range(args.warmup):
            fn()
    ctx.sync(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev_ms = timed(fused, args.steps)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / args.steps
    rounds = 3
    per = max(1, args.steps // rounds)
    ms = {"fused": [], "generate": [], "composed": []}
    for _ in range(rounds):
        ms["generate"].append(timed(generate, per)); ms["composed"].append(timed(composed, per)); ms["fused"].append(timed(fused, per))
    samples = S * N
    paths = {}
    for name, bytes_per_sample in (("fused", 16), ("generate", 8), ("composed", 32)):
        t_hbm = bytes_per_sample * samples / bc.HBM_PEAK_GBS / 1e9
        t_valu = samples / 2 * VALU_SLOTS[name] / LANES_PER_S
        best = min(ms[name])
        paths[name] = {"ms": [round(v, 4) for v in ms[name]], "best_ms": round(best, 4), "bytes_per_sample": bytes_per_sample, "bound_hbm_ms": round(t_hbm * 1e3, 4),
                       "bound_valu_ms": round(t_valu * 1e3, 4), "frac_of_hbm_bound": round(t_hbm / (best * 1e-3), 4), "frac_of_valu_bound": round(t_valu / (best * 1e-3), 4),
                       "achieved_GBs": round(bytes_per_sample * samples / (best * 1e-3) / 1e9, 1),
                       "frac_of_measured_copy_rate": round(bytes_per_sample * samples / (best * 1e-3) / 1e9 / HBM_COPY_GBS, 4)}
    t_hbm = 16 * samples / bc.HBM_PEAK_GBS / 1e9
    t_valu = samples / 2 * VALU_SLOTS["fused"] / LANES_PER_S
    t_bound = max(t_hbm, t_valu)
    res = {"metric": "MS/s, fused awgn_cc (Philox4x32-10, noise per channel) x N channels", "value": round(samples / wall / 1e6, 1), "unit": "MS/s",
           "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(wall * 1e3, 4), "event_ms_per_step": round(ev_ms, 4),
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "generated",
           "config": {"workload": "AWGN channel, batched", "channels": S, "block_samples_per_channel": N, "snr_db": [float(snr[0]), float(snr[-1])],
                      "hbm_peak_GBs": bc.HBM_PEAK_GBS, "valu_slots_per_philox_block": VALU_SLOTS, "hbm_measured_copy_GBs": HBM_COPY_GBS, "valu_lanes_per_s": LANES_PER_S},
           "roofline": {"bound": "valu" if t_valu >= t_hbm else "hbm", "kernel": "k_noise_gauss<awgn>", "kernel_avg_ms": round(ev_ms, 4),
                        "timer": "HIP events around the object's calls (the noise kernel and the position update)", "frac": round(t_bound / (ev_ms * 1e-3), 4),
                        "bound_hbm_ms": round(t_hbm * 1e3, 4), "bound_valu_ms": round(t_valu * 1e3, 4), "algorithmic_bytes_per_launch": 16 * samples},
           "alternating": {"rounds": rounds, "steps_per_round": per, "paths": paths,
                           "fused_over_composed": round(min(ms["fused"]) / min(ms["composed"]), 4), "generate_over_fused": round(min(ms["generate"]) / min(ms["fused"]), 4)}}
    if ver is not None:
        res["verify"] = ver
    print(json.dumps(res), flush=True)
    obj.close()
    ctx.close()


if __name__ == "__main__":
    main()
