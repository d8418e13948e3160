"""The z-sliding-window sweep of funcs.sweep_scores as ONE captured window step, replayed once per window.

The eager sweep (funcs.sweep_scores, mode="eager") drives every window from the host: a torch copy of the window whose start
plane is a host integer, the weight preparation, the BN fold plan and several hundred launches of the phase-0 forward.  Here the
window start comes from device memory (an int32 table of start planes and one cursor word, include/hdu.h: hdu_sweep_*), so the
step

    hdu_sweep_gather -> phase-0 forward launch list -> hdu_sweep_accumulate -> hdu_sweep_advance

is the same launch list for every window and is captured once into a linear hipGraph.  The weights and the moving statistics
cannot change during a sweep: weight preparation and the batched BN fold run once per sweep, outside the graph.  Between two
windows there is no host-to-device traffic and no host synchronisation.  On the emulator build the same four-part step runs
eagerly from the same device tables.

A model built with window_batch = W > 1 runs W windows per forward: the step is

    hdu_sweep_gather_batched -> forward over W windows -> hdu_sweep_accumulate_batched -> hdu_sweep_advance

replayed ceil(windows / W) times.  The table is padded to a multiple of W with the last start, and the window count of the
sweep is one more device word, so that a partly filled last step adds only its valid slots."""
import numpy as np
import torch

from . import lib as _l
from . import ops


def window_starts(z, img_cols, mini, maxi):
    """the window start planes of lib/funcs.py:12-28, the clamped last window included"""
    window_cols = img_cols // 4                       # lib/funcs.py:12 (py2 integer division)
    right_cols = int(min(z, maxi[2] + 10) - img_cols)
    left_cols = max(0, min(mini[2] - 5, right_cols))
    return [z - img_cols if cols > z - img_cols else cols for cols in range(left_cols, right_cols + window_cols, window_cols)]


class SweepPlan:
    """Resident volume, score, count, start table and cursor of the sweeps of `model` over volumes of depth `z`, and the
    captured window step.  A second sweep over another volume of the same depth reuses the graph; the table always has
    `capacity` entries (the most windows any liver window of this depth can need, padded with the last start), so the window
    count of a sweep is not baked into the captured launches."""

    def __init__(self, model, z, num, preprocess=None):
        if model.kind != "hybrid" or model.ctx.shard_world() > 1:
            raise ValueError("the sweep drives the unsharded hybrid nets with b=1 (test.py:27-29)")
        if not 1 <= num <= 3:
            raise ValueError("num: 1..3 of the 3 class scores (test.py passes 3)")
        self.batch, self.deps, self.rows, self.cols, _ = model.input_shape       # batch = the model's window_batch
        if z < self.cols or self.cols < 3:
            raise ValueError("volume smaller than the network window")
        if preprocess is not None:
            preprocess = tuple(float(v) for v in preprocess)
            if len(preprocess) != 3 or not preprocess[0] <= preprocess[1]:
                raise ValueError("preprocess: (lo, hi, mean) with lo <= hi")
        self.model, self.z, self.num, self.preprocess = model, int(z), int(num), preprocess
        self.plane = self.deps * self.rows
        dev = model.ctx.dev
        self.capacity = (self.z - self.cols) // max(1, self.cols // 4) + 2
        self.capacity = -(-self.capacity // self.batch) * self.batch        # whole steps of `batch` windows
        self.vol = torch.zeros(self.z * self.plane, dtype=torch.float32, device=dev)
        self.score = torch.zeros((self.z, self.deps, self.rows, self.num), dtype=torch.float32, device=dev)
        self.count = torch.zeros(self.z, dtype=torch.float32, device=dev)
        self.starts = torch.zeros(self.capacity, dtype=torch.int32, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)         # window index (batch 1) / step index
        self.nwin = torch.zeros(1, dtype=torch.int32, device=dev)           # windows of the current sweep (batch > 1 reads it)
        self.graph = None
        self._graph_key = None
        self.captures = 0        # graph captures so far
        self.replays = 0         # graph replays (eager window steps on the emulator build) of the last sweep

    def key(self):
        return (self.z, self.num, self.preprocess)

    def _step(self):
        m = self.model
        if self.batch > 1:
            ops.sweep_gather_batched(self.vol, self.z, self.plane, self.cols, self.starts, self.nwin, self.cursor, self.batch,
                                     m.vol, self.preprocess)
            m.ctx.run_forward()
            ops.sweep_accumulate_batched(m.logits.act, self.plane, self.cols, self.z, self.num, self.starts, self.nwin,
                                         self.cursor, self.batch, self.score.reshape(-1), self.count)
            ops.sweep_advance(self.cursor, self.capacity // self.batch)
            return
        ops.sweep_gather(self.vol, self.z, self.plane, self.cols, self.starts, self.cursor, m.vol, self.preprocess)
        m.ctx.run_forward()
        ops.sweep_accumulate(m.logits.act, self.plane, self.cols, self.z, self.num, self.starts, self.cursor,
                             self.score.reshape(-1), self.count)
        ops.sweep_advance(self.cursor, self.capacity)

    def _capture(self):
        """one eager warm-up window on a side stream (the lazily built device tables of the forward must exist before the
        capture), then the step into a linear graph.  Needs learning_phase 0 and the prefold of prepare()."""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        from .keras_api import _graph_capture
        with _graph_capture(g):
            self._step()
        self.graph = g
        self._graph_key = self.model._predict_state()
        self.captures += 1

    def prepare(self):
        """weights and inference-mode BN coefficients of this sweep, once, outside the graph (learning_phase must be 0)"""
        ctx = self.model.ctx
        ctx.prep_weights()
        ctx.prefold()

    def sweep(self, imgs_test, mini, maxi):
        """-> (score float32 device tensor [z][deps][rows][num], count float32 device tensor [z]): the plan's own accumulators,
        valid until the next sweep of this plan"""
        x, y, z = imgs_test.shape[:3]
        if z != self.z or x < self.deps or y < self.rows:
            raise ValueError("this plan sweeps volumes of depth %d at least %d x %d wide" % (self.z, self.deps, self.rows))
        starts = window_starts(self.z, self.cols, mini, maxi)
        nwin = len(starts)
        if nwin > self.capacity:
            raise ValueError("liver window yields %d windows, at most %d expected" % (nwin, self.capacity))
        table = np.full(self.capacity, starts[-1] if nwin else 0, np.int32)
        table[:nwin] = starts
        vol = np.ascontiguousarray(np.asarray(imgs_test[:self.deps, :self.rows, :], np.float32).transpose(2, 0, 1))
        self.vol.copy_(torch.from_numpy(vol).reshape(-1))
        self.starts.copy_(torch.from_numpy(table))
        self.nwin.fill_(nwin)
        ctx = self.model.ctx
        use_graph = not _l.is_emulator()
        ctx.learning_phase = 0
        try:
            self.prepare()
            if use_graph and nwin and (self.graph is None or self._graph_key != self.model._predict_state()):
                self._capture()              # (its warm-up window dirties the accumulators: they are reset below)
            self.score.zero_()
            self.count.zero_()
            self.cursor.zero_()
            self.replays = 0
            for _ in range(-(-nwin // self.batch)):
                if use_graph:
                    self.graph.replay()
                else:
                    self._step()
                self.replays += 1
        finally:
            ctx.end_prefold()
            ctx.learning_phase = 1
        return self.score, self.count


def plan_for(model, z, num, preprocess=None):
    """the model's plan for this depth (one plan is kept per model: another depth, `num` or preprocessing builds a new one)"""
    plan = getattr(model, "_sweep_plan", None)
    key = (int(z), int(num), None if preprocess is None else tuple(float(v) for v in preprocess))
    if plan is None or plan.key() != key:
        plan = SweepPlan(model, z, num, preprocess)
        model._sweep_plan = plan
    return plan
