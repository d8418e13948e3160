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


# ------------------------------------------------------------------ tiled 3-D sweep (lib/funcs.py:54-129 predict_window_mulgpu)
# The volume is tiled in all three axes with overlapping tiles and the scores are averaged.  The step
#
#     hdu_tile_gather_batched -> forward over `batch` tiles -> `batch` x hdu_tile_accumulate -> hdu_sweep_advance
#
# reads its tile starts from a device table of (x0, y0, z0) rows, so it is one launch list for every step.
def tile_starts(n, t):
    """the tile starts of one axis of length n with tile t (lib/funcs.py:56-58, :74-96): stride (t // 3) * 2, the starts past
    n - t clamped onto it"""
    n, t = int(n), int(t)
    w = (t // 3) * 2
    if t < 3 or n < t:
        raise ValueError("a tile of at least 3 and a volume of at least one tile per axis are required")
    return [min(s, n - t) for s in range(0, n - t + w, w)]


def tile_table(shape, tile):
    """the (x0, y0, z0) of every tile in the reference's order (x outermost, z innermost), int32 [ntiles][3]"""
    xs, ys, zs = (tile_starts(n, t) for n, t in zip(shape, tile))
    return np.array([(a, b, c) for a in xs for b in ys for c in zs], np.int32).reshape(-1, 3)


def tile_coverage(shape, tile):
    """(cx, cy, cz) float32: how many tile starts of each axis cover a position.  The tiles are a Cartesian product and every
    tile is run, so cx[x] * cy[y] * cz[z] tiles cover voxel (x, y, z)."""
    out = []
    for n, t in zip(shape, tile):
        c = np.zeros(int(n), np.float32)
        for s in tile_starts(n, t):
            c[s:s + int(t)] += 1
        out.append(c)
    return tuple(out)


def _check_tiled_model(model, num):
    if model.kind != "hybrid" or model.ctx.shard_world() > 1:
        raise ValueError("the tiled sweep drives the unsharded hybrid nets")
    if not 1 <= num <= 3:
        raise ValueError("num: 1..3 of the 3 class scores")


def _check_preprocess(preprocess):
    if preprocess is None:
        return None
    preprocess = tuple(float(v) for v in preprocess)
    if len(preprocess) != 3 or not preprocess[0] <= preprocess[1]:
        raise ValueError("preprocess: (lo, hi, mean) with lo <= hi")
    return preprocess


class TiledSweepPlan:
    """Resident volume, score, start table, cursor, tile count and coverage vectors of the tiled sweeps of `model` over
    volumes of `shape`, and the tile step.  graph=True captures the step once and replays it per step (the step runs eagerly
    on the emulator build); graph=False drives every step from the host with the cursor set by the host -- the same launches."""

    def __init__(self, model, shape, num, preprocess=None):
        _check_tiled_model(model, num)
        self.batch, self.deps, self.rows, self.cols, _ = model.input_shape       # batch = the model's window_batch
        self.shape = tuple(int(v) for v in shape)
        self.tile = (self.deps, self.rows, self.cols)
        if len(self.shape) != 3 or any(n < t for n, t in zip(self.shape, self.tile)) or min(self.tile) < 3:
            raise ValueError("volume smaller than the network window")
        if not 1 <= self.batch <= ops.SWEEP_MAX_BATCH:
            raise ValueError("window_batch: 1..%d" % ops.SWEEP_MAX_BATCH)
        self.preprocess = _check_preprocess(preprocess)
        self.model, self.num = model, int(num)
        X, Y, Z = self.shape
        dev = model.ctx.dev
        table = tile_table(self.shape, self.tile)
        self.ntiles = len(table)
        self.steps = -(-self.ntiles // self.batch)
        padded = np.repeat(table[-1:], self.steps * self.batch, axis=0)          # whole steps, padded with the last tile
        padded[:self.ntiles] = table
        self.table = table
        self.vol = torch.zeros(Z * X * Y, dtype=torch.float32, device=dev)
        self.score = torch.zeros((Z, X, Y, self.num), dtype=torch.float32, device=dev)
        self.starts = torch.from_numpy(np.ascontiguousarray(padded).reshape(-1)).to(dev)
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)              # step index
        self.ntiles_dev = torch.full((1,), self.ntiles, dtype=torch.int32, device=dev)
        self.coverage = tuple(torch.from_numpy(c).to(dev) for c in tile_coverage(self.shape, self.tile))
        self.graph = None
        self._graph_key = None
        self.captures = 0        # graph captures so far
        self.replays = 0         # steps (graph replays, or eager steps) of the last sweep

    def key(self):
        return (self.shape, self.num, self.preprocess)

    def _step(self):
        m = self.model
        ops.tile_gather_batched(self.vol, self.shape, self.tile, self.starts, self.ntiles_dev, self.cursor, self.batch, m.vol,
                                self.preprocess)
        m.ctx.run_forward()
        flat = self.score.reshape(-1)
        for slot in range(self.batch):
            ops.tile_accumulate(m.logits.act, self.shape, self.tile, self.num, self.starts, self.ntiles_dev, self.cursor,
                                self.batch, slot, flat)
        ops.sweep_advance(self.cursor, self.steps)

    def _capture(self):
        """one eager warm-up step on a side stream, then the step into a linear graph (as SweepPlan._capture)"""
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
        """weights and inference-mode BN coefficients of this sweep, once (learning_phase must be 0)"""
        ctx = self.model.ctx
        ctx.prep_weights()
        ctx.prefold()

    def sweep(self, imgs_test, graph=True):
        """-> (score float32 device tensor [Z][X][Y][num] of summed softmax scores, (cx, cy, cz) device coverage vectors): the
        plan's own buffers, valid until the next sweep of this plan"""
        if tuple(int(v) for v in np.shape(imgs_test)[:3]) != self.shape:
            raise ValueError("this plan sweeps volumes of shape %s" % (self.shape,))
        vol = np.ascontiguousarray(np.asarray(imgs_test, np.float32).reshape(self.shape).transpose(2, 0, 1))
        self.vol.copy_(torch.from_numpy(vol).reshape(-1))
        ctx = self.model.ctx
        use_graph = graph and not _l.is_emulator()
        ctx.learning_phase = 0
        try:
            self.prepare()
            if use_graph and (self.graph is None or self._graph_key != self.model._predict_state()):
                self._capture()              # (its warm-up step dirties the score and the cursor: they are reset below)
            self.score.zero_()
            self.cursor.zero_()
            self.replays = 0
            for step in range(self.steps):
                if use_graph:
                    self.graph.replay()
                else:
                    if not graph:
                        self.cursor.fill_(step)      # host-driven: the advance launch below computes the same word
                    self._step()
                self.replays += 1
        finally:
            ctx.end_prefold()
            ctx.learning_phase = 1
        return self.score, self.coverage


def tiled_plan_for(model, shape, num, preprocess=None):
    """the model's tiled plan for this volume shape (one plan is kept per model, keyed by shape, `num` and preprocessing)"""
    plan = getattr(model, "_tiled_sweep_plan", None)
    key = (tuple(int(v) for v in shape), int(num), _check_preprocess(preprocess))
    if plan is None or plan.key() != key:
        plan = TiledSweepPlan(model, shape, num, preprocess)
        model._tiled_sweep_plan = plan
    return plan


# ------------------------------------------------------------------ 2-D slice sweep (train_2ddense.py:58-61 over every plane)
# The 2-D DenseUNet sees the planes c-1, c, c+1 of a volume as the three channels of one input.  The step
#
#     hdu_slice_gather_batched -> forward over `batch` centre planes -> hdu_slice_argmax_store -> hdu_sweep_advance
#
# takes its step index from one device word, so it is one launch list for all ceil(Z / batch) steps; the label planes go to
# the raster order of the post-processing once, after the last step (hdu_slice_labels_to_raster).
class SliceSweepPlan:
    """Resident volume, [Z][H][W] label planes, raster-order label volume and cursor of the slice sweeps of the 2-D `model` over
    volumes of `shape`, and the step.  graph=True captures the step once and replays it per step (the step runs eagerly on the
    emulator build); graph=False drives every step from the host with the cursor set by the host -- the same launches."""

    def __init__(self, model, shape, preprocess=None):
        if model.kind != "2d" or model.ctx.shard_world() > 1 or getattr(model, "window_batch", 1) != 1:
            raise ValueError("the slice sweep drives the unsharded 2-D net (no window_batch)")
        self.batch, self.H, self.W, _ = model.input_shape                  # the model window: the top-left H x W
        self.shape = tuple(int(v) for v in shape)
        if len(self.shape) != 3 or self.shape[0] < self.H or self.shape[1] < self.W or self.shape[2] < 1:
            raise ValueError("volume smaller than the network window")
        if not 1 <= self.batch <= ops.SLICE_MAX_BATCH:
            raise ValueError("batch: 1..%d slices per forward" % ops.SLICE_MAX_BATCH)
        self.preprocess = _check_preprocess(preprocess)
        self.model = model
        X, Y, Z = self.shape
        if X * Y * Z >= 0xFFFFFFFF:
            raise ValueError("volumes of 2^32 - 1 voxels or more are not supported")
        dev = model.ctx.dev
        self.plane = self.H * self.W
        self.steps = -(-Z // self.batch)
        self.vol = torch.zeros(Z * X * Y, dtype=torch.float32, device=dev)
        self.planes = torch.zeros(Z * self.plane, dtype=torch.uint8, device=dev)       # argmax labels, [Z][H][W]
        self.labels = torch.zeros(X * Y * Z, dtype=torch.uint8, device=dev)            # the same in raster order [X][Y][Z]
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)                    # step index
        self.graph = None
        self._graph_key = None
        self.captures = 0        # graph captures so far
        self.replays = 0         # steps (graph replays, or eager steps) of the last sweep

    def key(self):
        return (self.shape, self.preprocess)

    def _step(self):
        m = self.model
        ops.slice_gather_batched(self.vol, self.shape, (self.H, self.W), self.cursor, self.batch, m.x_stage, self.preprocess)
        m.ctx.run_forward()
        ops.slice_argmax_store(m.logits.act, self.plane, self.shape[2], self.cursor, self.batch, self.planes)
        ops.sweep_advance(self.cursor, self.steps)

    def _capture(self):
        """one eager warm-up step on a side stream, then the step into a linear graph (as SweepPlan._capture)"""
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
        """weights and inference-mode BN coefficients of this sweep, once (learning_phase must be 0)"""
        ctx = self.model.ctx
        ctx.prep_weights()
        ctx.prefold()

    def sweep(self, imgs_test, graph=True):
        """-> the uint8 label volume {0, 1, 2} as a flat device tensor in raster order [X][Y][Z], zero outside the model window:
        the plan's own buffer, valid until the next sweep of this plan"""
        if tuple(int(v) for v in np.shape(imgs_test)[:3]) != self.shape:
            raise ValueError("this plan sweeps volumes of shape %s" % (self.shape,))
        vol = np.ascontiguousarray(np.asarray(imgs_test, np.float32).reshape(self.shape).transpose(2, 0, 1))
        self.vol.copy_(torch.from_numpy(vol).reshape(-1))
        ctx = self.model.ctx
        use_graph = graph and not _l.is_emulator()
        ctx.learning_phase = 0
        try:
            self.prepare()
            if use_graph and (self.graph is None or self._graph_key != self.model._predict_state()):
                self._capture()              # (its warm-up step dirties the label planes and the cursor: every valid plane is
            self.cursor.zero_()              #  written again below, and the cursor is reset here)
            self.replays = 0
            for step in range(self.steps):
                if use_graph:
                    self.graph.replay()
                else:
                    if not graph:
                        self.cursor.fill_(step)      # host-driven: the advance launch below computes the same word
                    self._step()
                self.replays += 1
        finally:
            ctx.end_prefold()
            ctx.learning_phase = 1
        ops.slice_labels_to_raster(self.planes, self.shape, (self.H, self.W), self.labels)
        return self.labels


def slice_plan_for(model, shape, preprocess=None):
    """the 2-D model's slice plan for this volume shape (one plan is kept per model, keyed by shape and preprocessing)"""
    plan = getattr(model, "_slice_sweep_plan", None)
    key = (tuple(int(v) for v in shape), _check_preprocess(preprocess))
    if plan is None or plan.key() != key:
        plan = SliceSweepPlan(model, shape, preprocess)
        model._slice_sweep_plan = plan
    return plan
