"""Host (numpy + scipy) versus device (hdu_metric_* kernels) evaluation of a LiTS label volume on a 512 x 512 x Z phantom:
liver and tumour overlap counts, Dice / VOE / RVD and the surface distances, spacing (0.7, 0.7, 2.5) mm.  Prints a short
report and, as its last line, one JSON object.

  python tools/bench_metrics.py [--z 300] [--reps 3] [--no-host]

truth:  the phantom's labels (liver with a cavity, a second blob, tumours in and outside the liver);
pred:   its noisy scores thresholded at 0.5 / 0.9 (speckle included: a hard case for the surface distances);
host:   metrics.evaluate_labels (four scipy distance transforms);
device: metrics.evaluate_labels_device including the upload of both label volumes and the download of the result words;
        `device_kernel_ms` sums the library's own per-dispatch times (hdu_profile_*), split by kernel, and every pass of the
        distance transform is set against the 8 TB/s HBM roof by the bytes it has to move (pass 1 reads the uint8 mask and
        writes float64, passes 2 and 3 read and write float64)."""
import argparse
import importlib
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROOF = 8.0e12
RTOL_DIST, RTOL_MEAN = 1e-14, 1e-9


def agree(got, ref):
    """the tolerances of tests/test_metrics_device.py; returns the largest relative difference seen"""
    worst = 0.0
    for name in ref:
        g, r = got[name], ref[name]
        for k in ("n_result", "n_reference", "n_intersection", "dice", "voe", "rvd", "n_rt", "n_tr"):
            assert g[k] == r[k] or (math.isnan(g[k]) and math.isnan(r[k])), (name, k, g[k], r[k])
        for k, tol in (("msd", RTOL_DIST), ("asd_rt", RTOL_MEAN), ("asd_tr", RTOL_MEAN), ("assd", RTOL_MEAN), ("rmsd", RTOL_MEAN)):
            if math.isnan(r[k]):
                assert math.isnan(g[k]), (name, k)
                continue
            rel = abs(g[k] - r[k]) / abs(r[k]) if r[k] else abs(g[k])
            assert rel <= tol, (name, k, g[k], r[k], rel)
            worst = max(worst, rel)
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--z", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    from bench_postprocess import phantom
    lib = importlib.import_module("h-denseunet_amd.lib")
    m = importlib.import_module("h-denseunet_amd.metrics")
    lib.load()
    torch.cuda.set_device(0)
    shape, spacing = (512, 512, a.z), (0.7, 0.7, 2.5)
    n = shape[0] * shape[1] * shape[2]
    score, count, coarse = phantom(shape, 512, 512)
    truth = coarse.astype(np.uint8)
    s = score / (count.reshape(-1, 1, 1, 1) + np.float32(1e-4))
    s1, s2 = s[..., 1].transpose(1, 2, 0), s[..., 2].transpose(1, 2, 0)
    pred = ((s1 >= 0.5) | (s2 >= 0.9)).astype(np.uint8)
    pred[s2 >= 0.9] = 2
    del score, s, s1, s2
    res = {"shape": list(shape), "spacing": list(spacing),
           "workspace_bytes": m._MetricWorkspace(shape, torch.device("cuda", 0)).nbytes()}

    got = m.evaluate_labels_device(pred, truth, spacing)            # warm-up (allocations, first launches)
    times = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        again = m.evaluate_labels_device(pred, truth, spacing)
        times.append(time.perf_counter() - t0)
        assert repr(again) == repr(got), "device evaluation is not bit-repeatable"
    res["device_ms"] = round(1e3 * min(times), 2)
    res["device_ms_all"] = [round(1e3 * t, 2) for t in times]

    lib.profile_begin()
    m.evaluate_labels_device(pred, truth, spacing)
    recs, calls = lib.profile_end()
    per = {}
    for name, ms in recs:
        key = name.split("(")[0]
        per[key] = per.get(key, 0.0) + ms
    res["device_kernel_ms"] = round(sum(per.values()), 3)
    res["device_kernels"] = {k: round(v, 3) for k, v in sorted(per.items(), key=lambda kv: -kv[1])}
    passes = {"z": [], "y": [], "x": []}
    for name, _, n0, n1 in calls:
        if name == "hdu_metric_edt":
            assert n1 - n0 == 3
            for axis, (_, ms) in zip("zyx", recs[n0:n1]):
                passes[axis].append(ms)
    bytes_per_pass = {"z": 9 * n, "y": 16 * n, "x": 16 * n}
    res["edt_passes"] = {}
    for axis in "zyx":
        ms = sum(passes[axis]) / len(passes[axis])
        bps = bytes_per_pass[axis] / (ms * 1e-3)
        res["edt_passes"][axis] = {"mean_ms": round(ms, 3), "min_ms": round(min(passes[axis]), 3), "max_ms": round(max(passes[axis]), 3),
                                   "TB_per_s": round(bps / 1e12, 3), "of_8TBps_roof": round(bps / ROOF, 3)}
    res["rework_next"] = "pass " + min("zyx", key=lambda ax: res["edt_passes"][ax]["of_8TBps_roof"])
    res["evaluation"] = got

    if not a.no_host:
        t0 = time.perf_counter()
        ref = m.evaluate_labels(pred, truth, spacing)
        res["host_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        res["worst_relative_difference"] = agree(got, ref)
        res["agree_within_tolerances"] = True
        res["speedup_wall"] = round(res["host_ms"] / res["device_ms"], 1)

    print("segmentation metrics, %d x %d x %d, spacing %s mm" % (shape + (spacing,)))
    if "host_ms" in res:
        print("host   evaluate_labels         %10.1f ms" % res["host_ms"])
    print("device evaluate_labels_device  %10.2f ms wall (upload + kernels + result words), %.3f ms in kernels"
          % (res["device_ms"], res["device_kernel_ms"]))
    for k, v in res["device_kernels"].items():
        print("  %-32s %9.3f ms" % (k, v))
    print("distance transform passes (4 transforms per evaluation; mean / min / max ms per pass, bytes moved against 8 TB/s):")
    for axis in "zyx":
        p = res["edt_passes"][axis]
        print("  pass %s  %8.3f / %8.3f / %8.3f ms  %6.3f TB/s = %4.1f %% of the roof"
              % (axis, p["mean_ms"], p["min_ms"], p["max_ms"], p["TB_per_s"], 100 * p["of_8TBps_roof"]))
    print("next to rework: %s (the lowest share of the roof)" % res["rework_next"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
