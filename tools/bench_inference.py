"""Eager versus captured inference, bf16 and f32, on one box: `Model.predict_resident` of the 2D DenseUNet at 8 x 512 x 512
(eager launch list against capture_predict's replayed graph) and the z-sliding-window sweep of dense_rnn_net with
224 x 224 x 12 windows over a synthetic 224 x 224 x D volume (funcs.sweep_scores mode="eager" against mode="graph").

  python tools/bench_inference.py [--z 64] [--reps 3] [--iters 20] [--tag mi355x] [--out FILE] [--phase-timeout 300]
                                  [--window-batch 1,2,4] [--workloads predict2d,sweep]

--window-batch W1,W2,...: the sweep phase is run once per value on a dense_rnn_net(window_batch=W) (W windows per forward),
eager and captured; every record carries ms per window, slices/s and launches per window, so W = 2 and 4 are read against
W = 1 of the same run.

The parent process never touches the GPU: every (workload, dtype) phase is a fresh child under its own `timeout`, and the
first phase that fails ends the run.  Inside a phase eager and captured are timed in the same process, eager first; every
figure is the list of `--reps` repeated timings (their spread is the yardstick for eager-against-captured), each timing
bracketed by a device synchronisation.  Writes profiles/inference_<tag>.json and prints it as one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _timed(fn, sync, reps):
    out = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def _stats(ms_runs, per):
    return {"ms_runs": [round(v / per, 4) for v in ms_runs], "ms_min": round(min(ms_runs) / per, 4),
            "ms_max": round(max(ms_runs) / per, 4)}


def _launches(lib, fn):
    lib.profile_begin()
    fn()
    recs, _ = lib.profile_end()
    return len(recs)


def phase_predict2d(dtype, a):
    import importlib
    import numpy as np
    import torch
    import parity_utils as U
    lib = importlib.import_module("h-denseunet_amd.lib")
    lib.load()
    torch.cuda.set_device(0)
    m = U.pkg("denseunet").DenseUNet(reduction=0.5, args=U.make_args(8, 512), dtype=dtype)
    x = np.random.default_rng(1).normal(0.0, 40.0, m.input_shape).astype(np.float32)
    m._upload_x(x)
    sync = torch.cuda.synchronize

    def many():
        for _ in range(a.iters):
            m.predict_resident()

    many()                                             # warm-up: allocations, lazily built tables
    res = {"workload": "predict2d", "dtype": dtype, "shape": list(m.input_shape), "iters_per_timing": a.iters}
    res["launches_eager"] = _launches(lib, m.predict_resident)
    res["eager"] = _stats(_timed(many, sync, a.reps), a.iters)
    ref = m._download_logits().clone()
    m.capture_predict()
    many()
    res["captured"] = _stats(_timed(many, sync, a.reps), a.iters)
    res["launches_captured_outside_graph"] = _launches(lib, m.predict_resident)
    res["max_abs_diff_captured_vs_eager"] = float((m._download_logits() - ref).abs().max())
    res["images_per_s_eager"] = round(8e3 / res["eager"]["ms_min"], 1)
    res["images_per_s_captured"] = round(8e3 / res["captured"]["ms_min"], 1)
    return res


def phase_sweep(dtype, a, wb=1):
    import importlib
    import numpy as np
    import torch
    import parity_utils as U
    lib = importlib.import_module("h-denseunet_amd.lib")
    lib.load()
    torch.cuda.set_device(0)
    f, sweep = U.pkg("funcs"), U.pkg("sweep")
    args = U.make_args(1, 224, 12)
    m = U.pkg("hybridnet").dense_rnn_net(args, dtype=dtype, window_batch=wb)
    vol = np.random.default_rng(1).normal(0.0, 40.0, (224, 224, a.z)).astype(np.float32)
    mini, maxi = (0, 0, 0), (223, 223, a.z - 1)
    nwin = len(sweep.window_starts(a.z, 12, mini, maxi))
    sync = torch.cuda.synchronize
    res = {"workload": "sweep", "dtype": dtype, "window_batch": wb, "volume": [224, 224, a.z], "window": [224, 224, 12],
           "windows": nwin, "steps": -(-nwin // wb)}

    def eager():
        return f.sweep_scores(m, vol, 3, mini, maxi, args)

    def graph():
        return f.sweep_scores(m, vol, 3, mini, maxi, args, mode="graph")

    e0, _ = eager()                                    # warm-up
    res["launches_per_window_eager"] = round(_launches(lib, eager) / nwin, 1)      # (+ one torch copy per window, not counted)
    te = _timed(eager, sync, a.reps)
    g0, _ = graph()                                    # warm-up: builds the plan, captures the step
    tg = _timed(graph, sync, a.reps)
    plan = m._sweep_plan
    ctx = m.ctx
    ctx.learning_phase = 0
    try:
        plan.prepare()
        # kernel nodes of the replayed graph (one step = window_batch windows), over the windows of the sweep
        res["launches_per_window_graph"] = round(_launches(lib, plan._step) * res["steps"] / nwin, 1)
    finally:
        ctx.end_prefold()
        ctx.learning_phase = 1
    res["captures"] = plan.captures
    for name, t in (("eager", te), ("graph", tg)):
        res[name] = {"sweep_" + k: v for k, v in _stats(t, 1).items()}
        res[name]["ms_per_window_runs"] = [round(v / nwin, 4) for v in t]
        res[name]["ms_per_window"] = round(min(t) / nwin, 4)
        res[name]["slices_per_s"] = round(1e3 * a.z / min(t), 1)
    g1, _ = graph()
    res["max_abs_score_diff_graph_vs_eager"] = float((g1 - e0).abs().max())
    res["bit_equal_graph_vs_eager"] = bool(torch.equal(g1, e0))
    return res


PHASES = {"predict2d": phase_predict2d, "sweep": phase_sweep}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--z", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tag", default="mi355x")
    ap.add_argument("--phase-timeout", type=int, default=300)
    ap.add_argument("--dtypes", default="bf16,f32")
    ap.add_argument("--window-batch", default="1", help="windows per forward of the sweep phase, e.g. 1,2,4")
    ap.add_argument("--workloads", default="predict2d,sweep")
    ap.add_argument("--out", default=None, help="result file (default profiles/inference_<tag>.json)")
    ap.add_argument("--phase", default=None, help="internal: run ONE phase in this process, e.g. sweep:bf16")
    a = ap.parse_args()
    if a.phase is not None:
        name, dtype, wb = (a.phase.split(":") + ["1"])[:3]
        print("PHASE_RESULT " + json.dumps(PHASES[name](dtype, a, int(wb)) if name == "sweep" else PHASES[name](dtype, a)))
        return 0
    out = {"tool": "tools/bench_inference.py", "reps": a.reps, "phases": []}
    for dtype in a.dtypes.split(","):
        for name, wb in [(n, w) for n in a.workloads.split(",") for w in (a.window_batch.split(",") if n == "sweep" else ["1"])]:
            cmd = ["timeout", "-k", "10", str(a.phase_timeout), sys.executable, os.path.abspath(__file__), "--phase",
                   "%s:%s:%s" % (name, dtype, wb), "--z", str(a.z), "--reps", str(a.reps), "--iters", str(a.iters)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("PHASE_RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-4000:])
                sys.stderr.write("\nphase %s:%s:%s ended with status %d: nothing more is started on the GPU\n" % (name, dtype, wb, p.returncode))
                return 1
            out["phases"].append(json.loads(line[-1][len("PHASE_RESULT "):]))
    path = a.out or os.path.join(ROOT, "profiles", "inference_%s.json" % a.tag)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
