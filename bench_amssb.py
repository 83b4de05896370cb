#!/usr/bin/env python3
"""bench_amssb.py -- the AM and SSB audio tails, batched: `--channels` channels x `--block` complex samples per step (CF32 input, resident in HBM) through one
csdr_amd_amssb object per mode (amssb.hip), AGC call length `--agc-block`.

Three legs per mode on the same buffers: the object with its tiled kernel (the default), the object with its one-lane-per-channel kernel (force_generic), and
the composed path of the batch calls a caller had before the object existed: csdr_amd_amdemod_cf -> csdr_amd_fastdcblock_ff -> csdr_amd_agc_ff ->
csdr_amd_limit_ff -> csdr_amd_convert_f_s16 (csdr_amd_realpart_cf in front instead of the first two for SSB), float intermediates in HBM.

The tail reads 8 bytes and writes 2 per sample, so the roofline named in the line is the HBM bound at 10 bytes per sample; what binds is agc_ff's
sample-serial chain, and the line says how far from the HBM bound that leaves it.  Interleaved repeats, medians of HIP-event times, the spread beside them;
`lanes_sweep_ms` times the channels-per-wave choices of the tiled kernel.  --verify compares sampled channels with the CPU run of the kernels' functions by bits.

    python bench_amssb.py [--gpus 1] [--steps K] [--warmup W] [--channels 4096] [--block 131072] [--agc-block 1024] [--verify] [--no-sweep]

--squelch measures the squelch inside the object (csdr_amd_amssb_enable_squelch) instead: per closed fraction and pattern one JSON line with three legs per
mode on the same buffers, alternating: the gated object on its tiled kernel, csdr_amd.Squelch into a second buffer followed by the unsquelched object, and the
gated object on its one-lane kernel.  `--pattern channel` closes whole channels drawn at random, `--pattern block` closes (channel, block) pairs drawn at
random; closed blocks are the signal scaled by 1e-4 under one level for all channels.  Without --closed-fraction / --pattern: 0, 0.5, 0.9 and 1 by channel and
0.5 by block.  Every line counts the (workgroup, block) pairs whose channels were all closed, from the flags the object returned; --verify compares the s16 of
sampled channels between the three legs in every bit.

    python bench_amssb.py --squelch [--closed-fraction f] [--pattern channel|block] [--steps 7] [--verify]
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

MODES = ("am", "ssb")
LEGS = ("tiled", "generic", "composed")


def signals(n_sig, n):
    """n_sig distinct rows: a carrier with a tone at 50 % depth whose level steps by 20 dB now and then, in noise; each row its own seed, offset and timing"""
    import numpy as np
    rows = []
    for k in range(n_sig):
        rng = np.random.default_rng(900 + k)
        t = np.arange(n)
        level = np.repeat(10.0 ** (rng.integers(-1, 2, n // 8192 + 1) * 1.0), 8192)[:n] * 0.3
        sig = level * (1 + 0.5 * np.sin(2 * np.pi * t / (61.0 + k))) * np.exp(2j * np.pi * (0.01 + 0.001 * k) * t + 1j * k)
        rows.append((sig + 0.01 * (rng.normal(size=n) + 1j * rng.normal(size=n))).astype(np.complex64))
    return np.stack(rows)


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


QUIET, SQ_LEVEL = 1e-4, 1e-5             # the loud blocks' power is at least about 1e-3, the scaled ones' at most about 1e-7
SQ_LEGS = ("gated_tiled", "squelch_then_object", "gated_generic")


def squelch_bench(args, ctx, x):
    """--squelch: one JSON line per (pattern, closed fraction)"""
    import numpy as np
    import torch
    import csdr_amd
    S, N, B = args.channels, args.block, args.agc_block
    nblk = N // B
    configs = [("channel", f) for f in (0.0, 0.5, 0.9, 1.0)] + [("block", 0.5)]
    if args.closed_fraction is not None or args.pattern is not None:
        configs = [(args.pattern or "channel", 0.5 if args.closed_fraction is None else args.closed_fraction)]
    P = {m: csdr_amd.amssb_params(m, B) for m in MODES}
    lv = np.full(S, SQ_LEVEL, np.float32)
    xq = torch.empty_like(x)                                                # the input of a configuration
    gated = torch.empty_like(x)                                             # the composed path's second buffer
    s16 = {leg: torch.empty((S, N), dtype=torch.int16, device="cuda") for leg in SQ_LEGS}
    pw = torch.empty((S, nblk), dtype=torch.float32, device="cuda"); fl = torch.empty((S, nblk), dtype=torch.uint8, device="cuda")
    objs = {}
    for m in MODES:
        objs[m, "gated_tiled"] = csdr_amd.AmSsb(ctx, P[m], S, max_samples_per_call=N, squelch=True, levels=lv)
        objs[m, "gated_generic"] = csdr_amd.AmSsb(ctx, P[m], S, max_samples_per_call=N, squelch=True, levels=lv); objs[m, "gated_generic"].force_generic()
        objs[m, "squelch_then_object"] = csdr_amd.AmSsb(ctx, P[m], S, max_samples_per_call=N)
    sq = csdr_amd.Squelch(ctx, S, B, 1, lv, max_samples_per_call=N)
    cnt = np.zeros(S, np.int32)

    def prepare(m, leg):
        objs[m, leg].reset()
        if leg == "squelch_then_object":
            sq.reset()

    def step(m, leg):
        if leg == "squelch_then_object":
            sq.process_dev(xq.data_ptr(), N, N, gated.data_ptr(), N, pw.data_ptr(), nblk, fl.data_ptr(), cnt)
            got = objs[m, leg].process_dev(gated.data_ptr(), N, N, s16[leg].data_ptr(), None, N)
        else:
            got, _ = objs[m, leg].process_squelched_dev(xq.data_ptr(), N, N, s16[leg].data_ptr(), None, N, pw.data_ptr(), nblk, fl.data_ptr())
        assert got == N

    calls = [(m, leg) for m in MODES for leg in SQ_LEGS]
    sampled = sorted(set(k for k in (0, 1, 37, 63, S // 2, S - 2, S - 1) if 0 <= k < S))
    for pattern, frac in configs:
        rng = np.random.default_rng(int(1000 * frac) + (7 if pattern == "block" else 0))
        if pattern == "channel":
            closed = np.zeros((S, nblk), bool); closed[rng.permutation(S)[:int(round(frac * S))]] = True
        else:
            closed = rng.random((S, nblk)) < frac
        scale = torch.from_numpy(np.where(closed, QUIET, 1.0).astype(np.float32)).cuda()
        torch.mul(x.view(S, nblk, 2 * B), scale[:, :, None], out=xq.view(S, nblk, 2 * B))
        torch.cuda.synchronize()
        ver, groups = {}, {}
        for m in MODES:
            for leg in SQ_LEGS:
                prepare(m, leg); step(m, leg); ctx.sync(); torch.cuda.synchronize()
                if leg == "gated_tiled":
                    flags = fl.cpu().numpy()
                    assert np.array_equal(flags == 0, closed), "the flags are not the configuration's"
                    C_ = objs[m, leg].lanes()
                    pad = (-S) % C_
                    allc = np.concatenate([flags == 0, np.ones((pad, nblk), bool)]).reshape(-1, C_, nblk).all(axis=1)
                    groups[m] = {"channels_per_workgroup": C_, "workgroup_blocks": int(allc.size), "all_closed": int(allc.sum()),
                                 "all_closed_fraction": round(float(allc.mean()), 4)}
            if args.verify:
                rows = {leg: s16[leg][sampled].cpu().numpy() for leg in SQ_LEGS}
                ver[m] = {"gated_tiled_vs_composed_words_differing": int(np.count_nonzero(rows["gated_tiled"] != rows["squelch_then_object"])),
                          "gated_generic_vs_composed_words_differing": int(np.count_nonzero(rows["gated_generic"] != rows["squelch_then_object"]))}
                ver[m]["ok"] = not any(ver[m].values())
        for _ in range(args.warmup):
            for m, leg in calls:
                prepare(m, leg); step(m, leg)
        ctx.sync(); torch.cuda.synchronize()
        times = {c: [] for c in calls}
        for _ in range(args.steps):
            for m, leg in calls:
                prepare(m, leg)
                ctx.timer_start(); step(m, leg); times[m, leg].append(ctx.timer_stop_ms())
        shapes = {}
        for m in MODES:
            shapes[m] = {"kernel": objs[m, "gated_tiled"].kernel_name(), "generic_kernel": objs[m, "gated_generic"].kernel_name(), "workgroups": groups[m]}
            for leg in SQ_LEGS:
                shapes[m][leg] = {"ms": round(median(times[m, leg]), 3), "min_ms": round(min(times[m, leg]), 3), "max_ms": round(max(times[m, leg]), 3)}
            shapes[m]["composed_over_gated"] = round(shapes[m]["squelch_then_object"]["ms"] / shapes[m]["gated_tiled"]["ms"], 2)
        t = shapes["am"]["gated_tiled"]["ms"]
        res = {"metric": "MS/s, squelch_and_smeter_cc | amdemod_cf | fastdcblock_ff | agc_ff | limit_ff | convert_f_s16 x N channels", "value": round(S * N / t / 1e3, 1),
               "unit": "MS/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "event_ms_per_step": t, "higher_is_better": True, "dtype": "f32",
               "data": "generated", "library": os.environ.get("CSDR_AMD_LIB") or "this tree",
               "config": {"workload": "AM and SSB audio tails behind a squelch, batched, CF32 input", "channels": S, "block_samples_per_channel": N, "agc_block": B,
                          "pattern": pattern, "closed_fraction": frac, "closed_fraction_drawn": round(float(closed.mean()), 4), "use_every_nth": 1},
               "timer": "HIP events around every leg's calls (the reset in front is not timed), medians over interleaved repeats of the three legs in both modes",
               "shapes": shapes}
        if args.verify:
            ver["sampled_channels"] = sampled; ver["samples_per_channel"] = N; ver["ok"] = bool(all(ver[m]["ok"] for m in MODES))
            res["verify"] = ver
        print(json.dumps(res), flush=True)
    for o in list(objs.values()) + [sq]:
        o.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--block", type=int, default=131072)
    ap.add_argument("--agc-block", type=int, default=1024)
    ap.add_argument("--verify", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--squelch", action="store_true")
    ap.add_argument("--closed-fraction", type=float, default=None)
    ap.add_argument("--pattern", choices=("channel", "block"), default=None)
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_amssb.py measures one GPU (--gpus 1)")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_amssb.py needs an MI355X; there is no CPU fallback")
    import csdr_amd
    ctx = csdr_amd.Context(0)
    L = ctx.L
    S, N, B = args.channels, args.block, args.agc_block
    if N % B:
        raise SystemExit("--block should be a multiple of --agc-block")
    n_sig = min(64, S)
    X = signals(n_sig, N)
    x = torch.from_numpy(X.view(np.float32)).cuda().repeat((S + n_sig - 1) // n_sig, 1)[:S].contiguous()      # [S, 2 N] floats
    if args.squelch:
        squelch_bench(args, ctx, x)
        ctx.close()
        return
    s16 = torch.empty((S, N), dtype=torch.int16, device="cuda")
    fa = torch.empty((S, N), dtype=torch.float32, device="cuda")           # the composed path's intermediates
    fb = torch.empty((S, N), dtype=torch.float32, device="cuda")
    st_dc = ctx.alloc(4 * S); st_gain = ctx.alloc(4 * S)
    ones = np.ones(S, np.float32); zeros = np.zeros(S, np.float32)
    P = {m: csdr_amd.amssb_params(m, B) for m in MODES}
    objs = {}
    for m in MODES:
        objs[m, "tiled"] = csdr_amd.AmSsb(ctx, P[m], S, max_samples_per_call=N)
        objs[m, "generic"] = csdr_amd.AmSsb(ctx, P[m], S, max_samples_per_call=N); objs[m, "generic"].force_generic()
    torch.cuda.synchronize()

    def prepare(m, leg):                                                      # every step walks the same stream from a fresh channel state; not timed
        if leg == "composed":
            ctx.check(L.csdr_amd_h2d(ctx.h, st_dc.ptr, zeros.ctypes.data_as(C.c_void_p), 4 * S), "h2d")
            ctx.check(L.csdr_amd_h2d(ctx.h, st_gain.ptr, ones.ctypes.data_as(C.c_void_p), 4 * S), "h2d")
        else:
            objs[m, leg].reset()

    def step(m, leg):
        if leg != "composed":
            got = objs[m, leg].process_dev(x.data_ptr(), N, N, s16.data_ptr(), None, N)
            assert got == N
            return
        p = P[m]
        if m == "am":
            ctx.check(L.csdr_amd_amdemod_cf(ctx.h, x.data_ptr(), fa.data_ptr(), S * N), "amdemod_cf")
            ctx.check(L.csdr_amd_fastdcblock_ff(ctx.h, fa.data_ptr(), fb.data_ptr(), S, N // B, B, N, N, st_dc.ptr), "fastdcblock_ff")
            src, dst = fb, fa
        else:
            ctx.check(L.csdr_amd_realpart_cf(ctx.h, x.data_ptr(), fb.data_ptr(), S * N), "realpart_cf")
            src, dst = fb, fa
        ctx.check(L.csdr_amd_agc_ff(ctx.h, src.data_ptr(), dst.data_ptr(), S, N, B, N, N, p.reference, p.attack_rate, p.decay_rate, p.max_gain, p.hang_time,
                                    p.attack_wait_time, p.gain_filter_alpha, st_gain.ptr), "agc_ff")
        ctx.check(L.csdr_amd_limit_ff(ctx.h, dst.data_ptr(), src.data_ptr(), S * N, p.limit_max), "limit_ff")
        ctx.check(L.csdr_amd_convert_f_s16(ctx.h, src.data_ptr(), s16.data_ptr(), S * N), "convert_f_s16")

    calls = [(m, leg) for m in MODES for leg in LEGS]
    sampled = [k for k in (0, 1, 37, 63, S - 1) if k < S]
    first = {}
    if args.verify:
        for m, leg in calls:
            prepare(m, leg); step(m, leg); ctx.sync(); torch.cuda.synchronize()
            first[m, leg] = {k: s16[k].cpu().numpy().copy() for k in sampled}
    for _ in range(args.warmup):
        for m, leg in calls:
            prepare(m, leg); step(m, leg)
    ctx.sync(); torch.cuda.synchronize()
    times = {c: [] for c in calls}
    for _ in range(args.steps):                                               # interleaved repeats, one HIP-event pair around every leg's calls
        for m, leg in calls:
            prepare(m, leg)
            ctx.timer_start(); step(m, leg); times[m, leg].append(ctx.timer_stop_ms())
    med = {k: median(v) for k, v in times.items()}
    sweep = None
    if not args.no_sweep:
        sweep = {m: {} for m in MODES}
        for m in MODES:
            o = objs[m, "tiled"]
            for lanes in (1, 4, 16, 64):
                o.set_lanes(lanes); prepare(m, "tiled"); step(m, "tiled"); ctx.sync()
                t = []
                for _ in range(3):
                    prepare(m, "tiled")
                    ctx.timer_start(); step(m, "tiled"); t.append(ctx.timer_stop_ms())
                sweep[m][str(lanes)] = round(median(t), 3)
            o.set_lanes(0)
    # the headline: wall time of back-to-back steps of the default kernel in AM mode
    ctx.sync(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        prepare("am", "tiled"); step("am", "tiled")
    ctx.sync(); torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    algo = 10 * S * N
    t_hbm_ms = algo / bc.HBM_PEAK_GBS / 1e9 * 1e3
    shapes = {}
    for m in MODES:
        t, g, c = med[m, "tiled"], med[m, "generic"], med[m, "composed"]
        spread = lambda leg: {"min_ms": round(min(times[m, leg]), 3), "max_ms": round(max(times[m, leg]), 3)}
        shapes[m] = {"kernel": objs[m, "tiled"].kernel_name(), "channels_per_wave": objs[m, "tiled"].lanes(), "ms": round(t, 3), "spread": spread("tiled"),
                     "MSps": round(S * N / t / 1e3, 1), "frac_of_hbm_bound": round(t_hbm_ms / t, 5), "us_per_sample_of_a_channel": round(t * 1e3 / N, 5),
                     "generic_kernel": objs[m, "generic"].kernel_name(), "generic_channels_per_wave": objs[m, "generic"].lanes(), "generic_ms": round(g, 3),
                     "generic_spread": spread("generic"), "composed_ms": round(c, 3), "composed_spread": spread("composed"),
                     "composed_over_object": round(c / t, 2),
                     "object_not_slower_than_composed": bool(t <= c + (max(times[m, "tiled"]) - min(times[m, "tiled"])) + (max(times[m, "composed"]) - min(times[m, "composed"])))}
    res = {"metric": "MS/s, amdemod_cf | fastdcblock_ff | agc_ff | limit_ff | convert_f_s16 x N channels", "value": round(S * N * args.steps / wall / 1e6, 1),
           "unit": "MS/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(wall / args.steps * 1e3, 3),
           "event_ms_per_step": shapes["am"]["ms"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "generated",
           "config": {"workload": "AM and SSB audio tails, batched, CF32 input", "channels": S, "block_samples_per_channel": N, "agc_block": B,
                      "distinct_signals": n_sig, "agc": "csdr.c:1342-1361 defaults", "limit_max": 1.0},
           "roofline": {"bound": "hbm", "kernel": shapes["am"]["kernel"], "kernel_avg_ms": shapes["am"]["ms"],
                        "timer": "HIP events around every leg's calls (the state reset in front is not timed), medians over interleaved repeats of the three legs in both modes",
                        "reason": "8 bytes read and 2 bytes written per complex sample; agc_ff's sample-serial chain binds, not the traffic: see frac",
                        "algorithmic_bytes_per_step": algo, "hbm_peak_GBs": bc.HBM_PEAK_GBS, "bound_hbm_ms": round(t_hbm_ms, 4), "frac": shapes["am"]["frac_of_hbm_bound"]},
           "shapes": shapes, "lanes_sweep_ms": sweep}
    if args.verify:
        ver = {}
        ok = True
        for m in MODES:
            words = cross = composed_diff = 0
            for k in sampled:
                want, _ = csdr_amd.amssb_debug_walk(P[m], X[k % n_sig])
                words += int(np.count_nonzero(first[m, "tiled"][k] != want))
                cross += int(np.count_nonzero(first[m, "tiled"][k] != first[m, "generic"][k]))
                composed_diff += int(np.count_nonzero(first[m, "composed"][k] != want))
            good = words == 0 and cross == 0
            # (the composed path sums fastdcblock_ff's blocks in another order: its AM audio may differ, and agc_ff then amplifies that; SSB's has no sum in it)
            ver[m] = {"words_differing_from_cpu_walk": words, "tiled_vs_generic_words_differing": cross, "composed_words_differing_from_cpu_walk": composed_diff, "ok": good}
            ok = ok and good
        ver["sampled_channels"] = sampled
        ver["samples_per_channel"] = N
        ver["ok"] = bool(ok)
        res["verify"] = ver
    print(json.dumps(res), flush=True)
    for o in objs.values():
        o.close()
    ctx.close()


if __name__ == "__main__":
    main()
