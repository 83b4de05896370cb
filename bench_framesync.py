#!/usr/bin/env python3
"""bench_framesync.py -- the frame synchroniser: pattern_search_u8_u8 for N channels through one csdr_amd_framesync object (framesync.hip).

One step = one process call over all channels (`--block` sliced bits each, resident in HBM, every channel's searcher carried from step to step).
Shape: 4096 channels x 131072 bytes of random bits with frames of a 32-bit sync word and 256 payload bits planted at random gaps (64 distinct rows, repeated);
L = 32, V = 256, max_mismatch 0 and 2.  Reported per max_mismatch: the time of k_framesync_tiled and of k_framesync_generic, the fraction of the HBM bound
for (bytes in + payload bytes out) at 8 TB/s, and the time of csdr_amd_pack_bits_8to1_u8_u8 over the same input as the project's byte-stream yardstick.
--verify compares sampled channels of the first step (payload, positions) with the CPU walk, for both kernels.

One JSON line per max_mismatch:
    python bench_framesync.py [--gpus 1] [--steps K] [--warmup W] [--channels 4096] [--block 131072] [--mismatch 0,2] [--verify] [--json-out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import bench_common as bc  # noqa: E402

L, V = 32, 256
DISTINCT = 64
SAMPLED = 4


def make_rows(S, N):
    import numpy as np
    rng = np.random.default_rng(1)
    word = rng.integers(0, 2, L).astype(np.uint8)
    rows = rng.integers(0, 2, (min(DISTINCT, S), N)).astype(np.uint8)
    for r in rows:
        at = int(rng.integers(0, 600))
        while at + L + V <= N:
            r[at:at + L] = word
            at += L + V + int(rng.integers(0, 600))
    return word, np.tile(rows, ((S + rows.shape[0] - 1) // rows.shape[0], 1))[:S]


def run(ctx, word, x_host, m, args):
    import numpy as np
    import torch
    import csdr_amd
    S, N = x_host.shape
    x = torch.from_numpy(x_host).cuda()
    y = torch.empty((S, N), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(S, dtype=torch.int32, device="cuda")
    fs = csdr_amd.FrameSync(ctx, word, V, S, m)
    fpitch = fs.max_frames(N)
    pos = torch.zeros((S, fpitch), dtype=torch.int64, device="cuda")
    fcnt = torch.zeros(S, dtype=torch.int32, device="cuda")
    packed = torch.empty((S, N // 8), dtype=torch.uint8, device="cuda")

    def step():
        fs.process_dev(x.data_ptr(), N, N, y.data_ptr(), N, cnt.data_ptr(), None, pos.data_ptr(), fpitch, fcnt.data_ptr())

    def step_pack():
        ctx.check(ctx.L.csdr_amd_pack_bits_8to1_u8_u8(ctx.h, x.data_ptr(), packed.data_ptr(), S, N, N, N // 8), "pack_bits_8to1_u8_u8")

    def timed(fn, steps):
        ctx.timer_start()
        for _ in range(steps):
            fn()
        return ctx.timer_stop_ms() / steps

    res = {"max_mismatch": m}
    rows = sorted(set(int(v) for v in np.linspace(0, S - 1, SAMPLED)))
    for name, forced, steps in (("tiled", False, args.steps), ("generic", True, max(1, min(args.steps, 3)))):
        fs.force_generic(forced)
        fs.reset()
        step(); ctx.sync()
        out_bytes = int(cnt.sum().item())
        k = {"kernel": fs.kernel_name(), "payload_bytes_first_step": out_bytes, "frames_first_step": int(fcnt.sum().item())}
        if args.verify:
            ok = True
            for r in rows:
                want, wpos = csdr_amd.framesync_debug_walk(word, V, x_host[r], m)
                c, f = int(cnt[r].item()), int(fcnt[r].item())
                ok = ok and np.array_equal(y[r, :c].cpu().numpy(), want) and np.array_equal(pos[r, :f].cpu().numpy(), wpos)
            k["verify"] = {"rows": rows, "ok": bool(ok)}
        for _ in range(args.warmup if not forced else 0):
            step()
        ctx.sync(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        ms = timed(step, steps)
        torch.cuda.synchronize()
        k["wall_ms_per_step"] = round((time.perf_counter() - t0) / steps * 1e3, 4)
        k["event_ms_per_step"] = round(ms, 4)
        k["steps"] = steps
        k["algorithmic_bytes_per_step"] = S * N + out_bytes
        k["frac"] = round((S * N + out_bytes) / bc.HBM_PEAK_GBS / 1e9 / (ms * 1e-3), 4)
        res[name] = k
    for _ in range(args.warmup):
        step_pack()
    ms_pack = timed(step_pack, args.steps)
    res["pack_bits_8to1"] = {"event_ms_per_step": round(ms_pack, 4), "algorithmic_bytes_per_step": S * N + S * N // 8,
                             "frac": round((S * N + S * N // 8) / bc.HBM_PEAK_GBS / 1e9 / (ms_pack * 1e-3), 4)}
    res["tiled_over_generic"] = round(res["tiled"]["event_ms_per_step"] / res["generic"]["event_ms_per_step"], 4)
    res["tiled_over_pack_bits"] = round(res["tiled"]["event_ms_per_step"] / ms_pack, 4)
    fs.close()
    del x, y, pos, packed
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--block", type=int, default=131072, help="bytes per channel and step (a multiple of 8)")
    ap.add_argument("--mismatch", default="0,2")
    ap.add_argument("--verify", action="store_true")
    ap.add_argument("--json-out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_framesync.py measures one GPU (--gpus 1)")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_framesync.py needs an MI355X; there is no CPU fallback")
    import csdr_amd
    ctx = csdr_amd.Context(0)
    S, N = args.channels, args.block
    word, x_host = make_rows(S, N)
    for m in (int(v) for v in args.mismatch.split(",")):
        r = run(ctx, word, x_host, m, args)
        t = r["tiled"]
        res = {"metric": "MB/s in, pattern_search_u8_u8 x N channels (frame synchroniser), max_mismatch %d" % m,
               "value": round(S * N / (t["event_ms_per_step"] * 1e-3) / 1e6, 1), "unit": "MB/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": t["wall_ms_per_step"], "event_ms_per_step": t["event_ms_per_step"], "higher_is_better": True, "scaling": "weak",
               "vs_baseline": round(1.0 / r["tiled_over_generic"], 3), "dtype": "u8", "data": "generated",
               "config": {"workload": "frame synchroniser, batched", "channels": S, "block_bytes_per_channel": N, "pattern_length": L, "values_after": V,
                          "max_mismatch": m, "baseline": "k_framesync_generic on the same buffers, same process", "hbm_peak_GBs": bc.HBM_PEAK_GBS},
               "roofline": {"bound": "hbm", "kernel": t["kernel"], "kernel_avg_ms": t["event_ms_per_step"],
                            "timer": "HIP events on the context's stream around the object's calls", "frac": t["frac"]},
               "result": r}
        if args.verify:
            res["verify"] = {"ok": bool(r["tiled"]["verify"]["ok"] and r["generic"]["verify"]["ok"])}
        line = json.dumps(res)
        print(line, flush=True)
        if args.json_out:
            with open(args.json_out, "a") as f:
                f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
