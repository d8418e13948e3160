"""The tiled 3-D sliding-window inference (funcs.segment_volume_tiled: tile sweep + hdu_tile_finalize + largest component) of a
224 x 224 x 12 `denseunet_3d` over a 512 x 512 x Z phantom, against the same number of bare forwards of the same model.
Prints one JSON line per (window_batch, mode).

  python tools/bench_tiled_sweep.py [--z 64] [--reps 3] [--dtype bf16] [--batches 1,4] [--size 224] [--cols 12]

per configuration: `sweep_ms` (tiled_sweep_scores alone, best of reps), `segment_ms` (segment_volume_tiled, host volume in, int16
labels out), `forwards_ms` (as many Model.predict_resident calls as the sweep has steps; captured with capture_predict in graph
mode), `stage_volume_ms` (the per-sweep fixed part: the depth-major host copy of the volume, its upload and the score clear),
`per_tile_ms`, `overhead_per_tile_ms` = (sweep - forwards) / tiles, and `outside_forward_share` = overhead / sweep.
In eager mode the library's launch profiler (hdu_profile_*) gives the kernel-time split of one sweep: `tile_kernel_ms` by kernel,
`tile_kernel_share` of all kernel time, and the bandwidth of hdu_tile_finalize (mask only, as segment_volume_tiled runs it, and
with the float32 score volume) against its algorithmic bytes, back to back (`warm`: the score sits in the last-level cache) and
after a 1 GiB fill (`cold`)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TILE_KERNELS = ("tile_gather_batched_kernel", "tile_accumulate_kernel", "sweep_advance_kernel", "tile_finalize_kernel")


def best_ms(fn, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return 1e3 * min(times)


def kernel_split(lib, fn):
    lib.profile_begin(1 << 18)
    fn()
    torch.cuda.synchronize()
    recs, _ = lib.profile_end()
    per, total = {}, 0.0
    for name, ms in recs:
        total += ms
        key = name.split("(")[0].split("<")[0].split()[-1]
        for k in TILE_KERNELS:
            if k in name:
                key = k
        per[key] = per.get(key, 0.0) + ms
    return per, total, len(recs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--z", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--cols", type=int, default=12)
    a = ap.parse_args()
    lib = importlib.import_module("h-denseunet_amd.lib")
    f = importlib.import_module("h-denseunet_amd.funcs")
    ops = importlib.import_module("h-denseunet_amd.ops")
    sweep = importlib.import_module("h-denseunet_amd.sweep")
    d3 = importlib.import_module("h-denseunet_amd.denseunet3d")
    import parity_utils as U
    lib.load()
    torch.cuda.set_device(0)
    shape = (512, 512, a.z)
    vol = np.random.default_rng(1).normal(0.0, 40.0, shape).astype(np.float32)
    ntiles = len(sweep.tile_table(shape, (a.size, a.size, a.cols)))
    nvox = shape[0] * shape[1] * shape[2]
    for W in (int(v) for v in a.batches.split(",")):
        model = d3.denseunet_3d(U.make_args(1, a.size, a.cols), dtype=a.dtype, window_batch=W)
        steps = -(-ntiles // W)
        for mode in ("eager", "graph"):
            if mode == "graph":
                model.capture_predict()

            def forwards():
                for _ in range(steps):
                    model.predict_resident()

            def run_sweep():
                f.tiled_sweep_scores(model, vol, 3, mode=mode)

            def run_segment():
                try:
                    f.segment_volume_tiled(model, vol, mode=mode, thres=thres)
                except ValueError:
                    pass

            run_sweep()                               # warm-up: plan, capture, first launches
            forwards()
            score, (cx, cy, cz) = f.tiled_sweep_scores(model, vol, 3, mode=mode)
            out = torch.empty(nvox, dtype=torch.float32, device=score.device)
            ops.tile_finalize(score, shape, 3, 1, cx, cy, cz, out_score=out)
            thres = float(out.median())               # an untrained net's scores sit on one side of 0.5: cut the volume in two
            res = {"window_batch": W, "mode": mode, "dtype": a.dtype, "shape": list(shape), "tile": [a.size, a.size, a.cols],
                   "tiles": ntiles, "steps": steps}
            res["sweep_ms"] = round(best_ms(run_sweep, a.reps), 3)
            plan = model._tiled_sweep_plan

            def stage():                              # the per-sweep fixed part: depth-major copy on the host, upload, clears
                v = np.ascontiguousarray(np.asarray(vol, np.float32).transpose(2, 0, 1))
                plan.vol.copy_(torch.from_numpy(v).reshape(-1))
                plan.score.zero_()

            res["stage_volume_ms"] = round(best_ms(stage, a.reps), 3)
            res["forwards_ms"] = round(best_ms(forwards, a.reps), 3)
            run_segment()
            res["segment_ms"] = round(best_ms(run_segment, a.reps), 3)
            res["per_tile_ms"] = round(res["sweep_ms"] / ntiles, 4)
            res["overhead_per_tile_ms"] = round((res["sweep_ms"] - res["forwards_ms"]) / ntiles, 4)
            res["outside_forward_share"] = round((res["sweep_ms"] - res["forwards_ms"]) / res["sweep_ms"], 4)
            if mode == "eager":
                per, total, n = kernel_split(lib, run_sweep)
                res["launches"] = n
                res["kernel_ms"] = round(total, 3)
                res["tile_kernel_ms"] = {k: round(per.get(k, 0.0), 4) for k in TILE_KERNELS[:3]}
                res["tile_kernel_share"] = round(sum(per.get(k, 0.0) for k in TILE_KERNELS[:3]) / total, 5)
                mask = torch.empty(nvox, dtype=torch.uint8, device=score.device)
                flush = torch.empty(1 << 30, dtype=torch.uint8, device=score.device)      # 4 x the 256 MiB last-level cache

                def finalize5(cold, kw):
                    for _ in range(5):
                        if cold:
                            flush.zero_()             # (a torch fill: not one of the library's launches, so not in the split)
                        ops.tile_finalize(score, shape, 3, 1, cx, cy, cz, thres=thres, **kw)

                for label, kw, wbytes in (("mask", dict(out_mask=mask), 1), ("score", dict(out_score=out), 4)):
                    for cold in (False, True):
                        finalize5(cold, kw)
                        per, _, _ = kernel_split(lib, lambda: finalize5(cold, kw))
                        ms = per["tile_finalize_kernel"] / 5
                        # the read touches every 64-byte line of the 3-channel score; the write is the output volume.  Launches
                        # that follow each other find the 192 MiB score in the last-level cache; `cold` evicts it first.
                        tag = "finalize_%s_%s" % (label, "cold" if cold else "warm")
                        res[tag + "_us"] = round(1e3 * ms, 2)
                        res[tag + "_gbs"] = round(nvox * (12 + wbytes) / (ms * 1e-3) / 1e9, 1)
            print(json.dumps(res), flush=True)
        del model


if __name__ == "__main__":
    main()
