#!/usr/bin/env python
"""Times the 2-D slice sweep on one MI355X: the full DenseUNet-161 at b = 8, 512 x 512, bfloat16, over a
512 x 512 x 64 synthetic volume.

  host    funcs.slice_labels_host: numpy batches, Model.predict, np.argmax -- the only way before the sweep existed
  eager   funcs.segment_volume_2d(mode="eager"): the resident sweep, every step driven from the host
  graph   funcs.segment_volume_2d(mode="graph"): one captured step replayed ceil(Z / b) times

All three start from the host volume and end with the uint8 label volume on the host.  The three are run in turn, `--rounds`
times after one warm-up round, in one process; median and minimum per variant.  The raster kernel
(hdu_slice_labels_to_raster) is timed with device events over back-to-back launches against its two-pass byte count (one read
plus one write of X*Y*Z bytes).  Usage: tools/bench_slice_sweep.py [--out FILE] [--rounds N] [--size S --depth Z --batch B]"""
import argparse
import glob
import hashlib
import importlib
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def source_digest():
    """bench.py's digest of the kernel sources (csrc + the C-ABI header)"""
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "h-denseunet_amd", "csrc", "*")) + [os.path.join(ROOT, "include", "hdu.h")]):
        if os.path.isfile(f):
            h.update(os.path.basename(f).encode())
            h.update(open(f, "rb").read())
    return h.hexdigest()[:12]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--depth", type=int, default=64)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--dtype", default="bf16")
    a = ap.parse_args()
    pkg = lambda m: importlib.import_module("h-denseunet_amd." + m)
    lib, ops, f = pkg("lib"), pkg("ops"), pkg("funcs")
    lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("bench_slice_sweep needs the GPU: there is nothing to measure without it")
    S, Z, B = a.size, a.depth, a.batch
    model = pkg("denseunet").DenseUNet(reduction=0.5, args=types.SimpleNamespace(b=B, input_size=S), dtype=a.dtype)
    vol = pkg("synth").synthetic_ct((S, S, Z), seed=3)[0]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    variants = {"host": lambda: f.slice_labels_host(model, vol),
                "eager": lambda: f.segment_volume_2d(model, vol, mode="eager"),
                "graph": lambda: f.segment_volume_2d(model, vol, mode="graph")}
    # the same sweeps up to the device-resident labels (no download): what a cascade pays
    resident = {"eager_resident": lambda: f.slice_sweep_labels(model, vol, mode="eager"),
                "graph_resident": lambda: f.slice_sweep_labels(model, vol, mode="graph")}
    times = {k: [] for k in list(variants) + list(resident)}
    outs = {}
    for r in range(a.rounds + 1):
        for name, fn in list(variants.items()) + list(resident.items()):
            ms, out = timed(fn)
            if r:                                   # round 0 warms every variant up (code objects, the capture, the plan)
                times[name].append(ms)
            elif name in variants:
                outs[name] = out
    counts = np.bincount(outs["host"].reshape(-1), minlength=3).tolist()
    agree = {k: float((outs[k] == outs["host"]).mean()) for k in ("eager", "graph")}
    plan = model._slice_sweep_plan
    # where the wall time of a sweep goes: the host's float32 transpose to [Z][X][Y], its upload, the replayed steps alone
    t0 = time.perf_counter()
    zxy = np.ascontiguousarray(np.asarray(vol, np.float32).transpose(2, 0, 1))
    transpose_ms = (time.perf_counter() - t0) * 1e3
    upload_ms, _ = timed(lambda: plan.vol.copy_(torch.from_numpy(zxy).reshape(-1)))
    ctx = model.ctx
    steps_ms = []
    ctx.learning_phase = 0
    try:
        plan.prepare()
        for _ in range(a.rounds):
            plan.cursor.zero_()
            ms, _ = timed(lambda: [plan.graph.replay() for _ in range(plan.steps)])
            steps_ms.append(ms)
    finally:
        ctx.end_prefold()
        ctx.learning_phase = 1
    download_ms, _ = timed(lambda: plan.labels.cpu().numpy())
    # raster kernel alone
    labels = torch.empty_like(plan.labels)
    n_launch = 200
    for _ in range(10):
        ops.slice_labels_to_raster(plan.planes, plan.shape, (plan.H, plan.W), labels)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n_launch):
        ops.slice_labels_to_raster(plan.planes, plan.shape, (plan.H, plan.W), labels)
    e1.record()
    torch.cuda.synchronize()
    raster_us = e0.elapsed_time(e1) * 1e3 / n_launch
    nbytes = 2 * S * S * Z
    res = {"digest": source_digest(), "shape": [S, S, Z], "batch": B, "dtype": a.dtype, "rounds": a.rounds,
           "label_counts_host": counts, "fraction_equal_to_host": agree, "captures": plan.captures, "replays": plan.replays,
           "ms_per_slice": {k: {"median": float(np.median(v)) / Z, "min": float(np.min(v)) / Z} for k, v in times.items()},
           "ms_per_volume": {k: [round(x, 3) for x in v] for k, v in times.items()},
           "split_ms_per_volume": {"host_transpose": transpose_ms, "upload": upload_ms, "download_labels": download_ms,
                                   "graph_steps_only": [round(x, 3) for x in steps_ms]},
           "raster": {"us_per_launch_back_to_back": raster_us, "launches": n_launch, "bytes_two_pass": nbytes,
                      "TB_per_s": nbytes / (raster_us * 1e-6) / 1e12,
                      "note": "the %d MB of the two volumes fit the 256 MiB Infinity Cache: this is not an HBM rate" % (nbytes >> 20)}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
