"""Host (scipy) versus device (hdu_pp_* kernels) post-processing of the LiTS inference on a 512 x 512 x Z phantom, and the
whole segment_volume (sweep + post-processing) on the same volume.  Prints one JSON line.

  python tools/bench_postprocess.py [--z 300] [--reps 3] [--no-host] [--no-volume] [--volume-dtype bf16]

host:   liver_window_from_mask + segment_liver_tumor on the averaged scores (what predict_tumor_inwindow hands back);
device: liver_window_from_mask_device + segment_liver_tumor_device on the sweep's device score, including the coarse mask's
        upload and the label volume's download; `device_kernel_ms` is the sum of the library's own per-dispatch times of the
        post-processing kernels (hdu_profile_*), `device_kernels` the split by kernel."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def phantom(shape, deps, rows, seed=0):
    """sweep-layout scores: an ellipsoidal liver with noise and a cavity, a second blob, tumours in and outside the liver"""
    X, Y, Z = shape
    rng = np.random.default_rng(seed)
    x, y, z = np.ogrid[:deps, :rows, :Z]
    liver = ((x - 250) / 90.0) ** 2 + ((y - 260) / 70.0) ** 2 + ((z - Z / 2) / (Z / 6.0)) ** 2 < 1
    hole = ((x - 250) ** 2 + (y - 260) ** 2 + (z - Z / 2) ** 2) < 36
    blob = ((x - 420) ** 2 + (y - 60) ** 2 + (z - Z / 4) ** 2) < 200
    tum = ((x - 240) ** 2 + (y - 270) ** 2 + (z - Z / 2 - 5) ** 2) < 400
    stray = ((x - 60) ** 2 + (y - 450) ** 2 + (z - Z / 3) ** 2) < 100
    count = np.full(Z, 3, np.float32)
    count[: Z // 10] = 0
    s_l = np.clip(0.9 * ((liver & ~hole) | blob) + rng.normal(0, 0.2, (deps, rows, Z)), 0, 1).astype(np.float32)
    s_t = np.clip(0.95 * (tum | stray) + rng.normal(0, 0.05, (deps, rows, Z)), 0, 1).astype(np.float32)
    score = np.zeros((Z, deps, rows, 3), np.float32)
    score[..., 1] = (s_l * count).transpose(2, 0, 1)
    score[..., 2] = (s_t * count).transpose(2, 0, 1)
    coarse = np.zeros(shape, np.int16)
    coarse[:deps, :rows][np.broadcast_to(liver | blob, (deps, rows, Z))] = 1
    coarse[:deps, :rows][np.broadcast_to(tum, (deps, rows, Z))] = 2
    return score, count, coarse


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--z", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-volume", action="store_true")
    ap.add_argument("--volume-dtype", default="bf16")
    a = ap.parse_args()
    import importlib
    lib = importlib.import_module("h-denseunet_amd.lib")
    f = importlib.import_module("h-denseunet_amd.funcs")
    hybridnet = importlib.import_module("h-denseunet_amd.hybridnet")
    lib.load()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    shape, deps, rows = (512, 512, a.z), 512, 512
    score, count, coarse = phantom(shape, deps, rows)
    res = {"shape": list(shape), "liver_voxels": int((coarse > 0).sum())}
    score_d = torch.from_numpy(score).to(dev)
    count_d = torch.from_numpy(count).to(dev)

    def device_run():
        md, mini, maxi = f.liver_window_from_mask_device(coarse)
        return f.segment_liver_tumor_device(score_d, count_d, shape, md, 0.5, 0.9), mini, maxi

    got, mini, maxi = device_run()            # warm-up (allocations, first launches)
    times = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        device_run()
        times.append(time.perf_counter() - t0)
    res["device_ms"] = round(1e3 * min(times), 2)
    res["device_ms_all"] = [round(1e3 * t, 2) for t in times]
    lib.profile_begin()
    device_run()
    recs, _ = lib.profile_end()
    per = {}
    for name, ms in recs:
        key = name.split("(")[0]
        per[key] = per.get(key, 0.0) + ms
    res["device_kernel_ms"] = round(sum(per.values()), 3)
    res["device_kernels"] = {k: round(v, 3) for k, v in sorted(per.items(), key=lambda kv: -kv[1])}
    if not a.no_host:
        t0 = time.perf_counter()
        m, hmini, hmaxi = f.liver_window_from_mask(coarse)
        t1 = time.perf_counter()
        s = score / (count.reshape(-1, 1, 1, 1) + np.float32(1e-4))
        out = np.zeros(shape + (3,), np.float32)
        out[:deps, :rows] = s.transpose(1, 2, 0, 3)
        t2 = time.perf_counter()
        ref = f.segment_liver_tumor(out[..., 1], out[..., 2], m, 0.5, 0.9)
        t3 = time.perf_counter()
        res["host_window_ms"] = round(1e3 * (t1 - t0), 1)
        res["host_segment_ms"] = round(1e3 * (t3 - t2), 1)
        res["host_ms"] = round(1e3 * (t3 - t2 + t1 - t0), 1)
        res["identical"] = bool(np.array_equal(got, ref) and np.array_equal(mini, hmini) and np.array_equal(maxi, hmaxi))
    if not a.no_volume:
        import parity_utils as U
        args = U.make_args(1, 224, 12)
        model = hybridnet.dense_rnn_net(args, dtype=a.volume_dtype)
        vol = np.random.default_rng(1).normal(0.0, 40.0, shape).astype(np.float32)
        try:                                          # warm-up on a short slab through the liver
            zc = a.z // 2
            f.segment_volume(model, vol[:, :, zc - 12:zc + 12], coarse[:, :, zc - 12:zc + 12], args, 0.3, 0.4)
        except ValueError:
            pass
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            f.segment_volume(model, vol, coarse, args, 0.3, 0.4)
            res["segment_volume_outcome"] = "labels"
        except ValueError:
            res["segment_volume_outcome"] = "ValueError (no component above threshold)"
        res["segment_volume_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        res["segment_volume_dtype"] = a.volume_dtype
        md, mini, maxi = f.liver_window_from_mask_device(coarse)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f.sweep_scores(model, vol, 3, mini, maxi, args)
        torch.cuda.synchronize()
        res["sweep_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
