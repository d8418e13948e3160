"""Drop-in for lib/funcs.py:4-51 `predict_tumor_inwindow`: z-sliding-window inference with score averaging
(SURVEY.md section 8f, row N1).  Same arguments and return values; differences in mechanism only:
 * the CT volume, the accumulated `score` and `score_num` stay resident in HBM for the whole sweep (the reference
   round-trips every window through numpy and grows the TF graph with K.softmax/K.eval nodes per iteration,
   lib/funcs.py:31-32);
 * each window is copied device-to-device into the model's input buffer and run with Model.predict's launch list
   (learning_phase 0).
The 3-class softmax and the `score +=` of a window are ONE launch (hdu_softmax_accumulate) straight off the logits; how many
windows cover a slice (`score_num`) is a function of the window starts alone and is counted on the host."""
import numpy as np
import torch

from . import ops
from . import sweep


def predict_tumor_inwindow(model, imgs_test, num, mini, maxi, args, mode="eager"):
    score, score_num = sweep_scores(model, imgs_test, num, mini, maxi, args, mode=mode)
    if torch.is_tensor(score_num):
        score_num = score_num.cpu().numpy()
    x, y, z = imgs_test.shape[:3]
    img_deps, img_rows = args.input_size, args.input_size
    score = score.cpu().numpy() / (score_num.reshape(z, 1, 1, 1) + np.float32(1e-4))        # lib/funcs.py:36
    out = np.zeros((x, y, z, num), np.float32)
    out[:img_deps, :img_rows] = score.transpose(1, 2, 0, 3)
    return out[:, :, :, num - 2], out[:, :, :, num - 1]


def sweep_scores(model, imgs_test, num, mini, maxi, args, mode="eager", preprocess=None):
    """the window sweep of predict_tumor_inwindow, left on the device: (score float32 device tensor [z][deps][rows][num] of
    summed softmax scores, score_num float32 [z] = windows that covered each plane).
    mode="eager" (default): every window driven from the host, score_num counted on the host (numpy).
    mode="graph": one captured window step replayed per window (sweep.SweepPlan); score and score_num (a DEVICE tensor) are the
    plan's own accumulators, valid until the next graph-mode sweep of this model.
    A model built with window_batch = W > 1 runs W windows per forward in either mode (per step, one softmax_accumulate per
    valid window in window order / one batched accumulate): nothing to pass here.
    preprocess=(lo, hi, mean): `imgs_test` is raw; the network sees min(max(v, lo), hi) - mean (preprocessing.py:15-16,
    test.py:55), applied on the host in eager mode and by the window gather in graph mode."""
    if mode not in ("eager", "graph"):
        raise ValueError("mode: 'eager' or 'graph', not %r" % (mode,))
    batch = args.b
    img_deps, img_rows, img_cols = args.input_size, args.input_size, args.input_cols
    if batch != 1 or model.kind != "hybrid":
        raise ValueError("predict_tumor_inwindow drives the hybrid nets with b=1 (test.py:27-29)")
    window_cols = img_cols // 4                       # lib/funcs.py:12 (py2 integer division)
    x, y, z = imgs_test.shape[:3]
    if x < img_deps or y < img_rows or z < img_cols:
        raise ValueError("volume smaller than the network window")
    if mode == "graph":
        return sweep.plan_for(model, z, num, preprocess).sweep(imgs_test, mini, maxi)
    if preprocess is not None:
        lo, hi, mean = (np.float32(v) for v in preprocess)
        imgs_test = np.clip(np.asarray(imgs_test[:img_deps, :img_rows, :], np.float32), lo, hi) - mean
    right_cols = int(min(z, maxi[2] + 10) - img_cols)
    left_cols = max(0, min(mini[2] - 5, right_cols))
    dev = model.ctx.dev
    # depth-major resident copy of the cropped volume: [z][deps][rows]
    vol = torch.as_tensor(np.ascontiguousarray(np.asarray(imgs_test[:img_deps, :img_rows, :], np.float32).transpose(2, 0, 1))).to(dev)
    if not 1 <= num <= 3:
        raise ValueError("num: 1..3 of the 3 class scores (test.py passes 3)")
    score = torch.zeros((z, img_deps, img_rows, num), dtype=torch.float32, device=dev)
    score_num = np.zeros(z, np.float32)
    plane = img_deps * img_rows
    ctx = model.ctx
    a = model.logits.act
    W = getattr(model, "window_batch", 1)
    if W > 1:
        # W windows per forward: padding slots of the last step repeat the last window and add nothing
        starts = sweep.window_starts(z, img_cols, mini, maxi)
        n = img_cols * plane
        for s0 in range(0, len(starts), W):
            step = starts[s0:s0 + W]
            for i in range(W):
                c0 = step[min(i, len(step) - 1)]
                model.vol[i * n:(i + 1) * n].copy_(vol[c0:c0 + img_cols].reshape(-1))
            ctx.learning_phase = 0
            try:
                ctx.prep_weights()
                ctx.run_forward()
            finally:
                ctx.learning_phase = 1
            for i, c0 in enumerate(step):
                ops.softmax_accumulate(a, (i * img_cols + 1) * plane, (img_cols - 2) * plane, num,
                                       score[c0 + 1:c0 + img_cols - 1].reshape(-1))
                score_num[c0 + 1:c0 + img_cols - 1] += 1
        return score, score_num.reshape(z)
    for cols in range(left_cols, right_cols + window_cols, window_cols):
        c0 = z - img_cols if cols > z - img_cols else cols        # lib/funcs.py:26-28: last window is clamped
        model.vol.copy_(vol[c0:c0 + img_cols].reshape(-1))
        ctx.learning_phase = 0
        try:
            ctx.prep_weights()
            ctx.run_forward()
        finally:
            ctx.learning_phase = 1
        # first / last slice of each window dropped (lib/funcs.py:33): planes 1 .. img_cols-2 of the logits onto planes c0+1 ..
        ops.softmax_accumulate(a, plane, (img_cols - 2) * plane, num, score[c0 + 1:c0 + img_cols - 1].reshape(-1))
        score_num[c0 + 1:c0 + img_cols - 1] += 1
    return score, score_num.reshape(z)


def liver_window_from_mask(mask):
    """test.py:57-62: bounding box (mini, maxi) of the dilated liver mask (labels 1 and 2 merged) that
    `predict_tumor_inwindow` sweeps; returns (dilated mask, mini, maxi)."""
    from scipy import ndimage
    m = np.array(mask, copy=True)
    m[m == 2] = 1
    m = ndimage.binary_dilation(m, iterations=1).astype(m.dtype)
    index = np.where(m == 1)
    if index[0].size == 0:
        raise ValueError("empty liver mask")
    return m, np.min(index, axis=-1), np.max(index, axis=-1)


def _largest_component(binary):
    """skimage.measure.label(..., return_num=True) + regionprops areas + `box.index(max(box)) + 1` (test.py:84-92):
    full connectivity (skimage's default for label is connectivity = ndim), first label wins a tie"""
    from scipy import ndimage
    lab, num = ndimage.label(binary, structure=np.ones((3,) * binary.ndim, dtype=bool))
    if num == 0:
        raise ValueError("no foreground component (the reference raises on max([]) here, test.py:90)")
    areas = np.bincount(lab.ravel(), minlength=num + 1)[1:]
    keep = int(np.argmax(areas)) + 1          # argmax returns the FIRST maximum, like list.index(max(...))
    return (lab == keep).astype(lab.dtype)


def segment_liver_tumor(score1, score2, mask, thres_liver=0.5, thres_tumor=0.8):
    """Host-side post-processing of test.py:70-112: threshold the averaged scores,
    keep the largest liver component, restrict tumours to the (dilated, largest, hole-filled) coarse liver mask, fill
    holes, and return the uint8 label volume {0 background, 1 liver, 2 tumour} that the reference saves as NIfTI.
    `mask` is the ALREADY dilated coarse liver mask of liver_window_from_mask (test.py dilates it a second time
    before labelling, :95 -- reproduced).  scipy.ndimage replaces skimage.measure (same connectivity and tie rule)."""
    from scipy import ndimage
    result1 = np.array(score1, dtype=np.float64, copy=True)
    result2 = np.array(score2, dtype=np.float64, copy=True)
    result1 = (result1 >= thres_liver).astype(np.float64)
    result2 = (result2 >= thres_tumor).astype(np.float64)
    result1[result2 == 1] = 1
    segmask = result2
    liver_res = _largest_component(result1)
    m = ndimage.binary_dilation(mask, iterations=1).astype(np.asarray(mask).dtype)
    liver_labels = _largest_component(m)
    liver_labels = ndimage.binary_fill_holes(liver_labels).astype(int)
    segmask = segmask * liver_labels
    segmask = ndimage.binary_fill_holes(segmask).astype(int).astype(np.uint8)
    liver_res = ndimage.binary_fill_holes(liver_res.astype(np.uint8)).astype(int)
    liver_res[segmask == 1] = 2
    return liver_res.astype(np.uint8)


# ------------------------------------------------------------------ device-resident post-processing (include/hdu.h: hdu_pp_*)
# Bit-identical to liver_window_from_mask / segment_liver_tumor above (same uint8 volumes, same exceptions): thresholds,
# largest 26-connected component, dilation and hole filling run as HIP kernels on masks kept in HBM in the host's raster
# order (x, y, z); only the bounding box, the component counts and the final uint8 label volume come back.
_NO_COMPONENT = "no foreground component (the reference raises on max([]) here, test.py:90)"


def _check_volume(shape):
    if len(shape) != 3 or min(shape) <= 0:
        raise ValueError("a 3-D volume is required")
    n = int(shape[0]) * int(shape[1]) * int(shape[2])
    if n >= 0xFFFFFFFF:
        raise ValueError("volumes of 2^32 - 1 voxels or more are not supported")
    return n


def liver_window_from_mask_device(mask):
    """liver_window_from_mask on the device: `mask` is a host array of any numeric dtype (2 merged into 1, nonzero is the
    liver); returns (dilated mask as a flat uint8 device tensor in raster order, mini, maxi)"""
    m = np.asarray(mask)
    shape = tuple(int(v) for v in m.shape)
    n = _check_volume(shape)
    dev = ops.device()
    src = torch.from_numpy(np.ascontiguousarray(m != 0).view(np.uint8).reshape(n)).to(dev)
    return liver_window_from_device_mask(src, shape)


def liver_window_from_device_mask(mask_dev, shape):
    """liver_window_from_mask of a mask that is already on the device: `mask_dev` is a flat uint8 device tensor in raster
    order (nonzero is the liver), shape = (x, y, z); returns (dilated mask as a flat uint8 device tensor, mini, maxi)"""
    shape = tuple(int(v) for v in shape)
    n = _check_volume(shape)
    if not torch.is_tensor(mask_dev) or mask_dev.dtype != torch.uint8 or mask_dev.numel() != n:
        raise ValueError("mask_dev: a flat uint8 device mask of this volume")
    dev = mask_dev.device
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    ops.pp_dilate(mask_dev.contiguous().reshape(n), shape, out)
    box = torch.tensor([-1, -1, -1, 0, 0, 0], dtype=torch.int32, device=dev)
    ops.pp_bbox(out, shape, box)
    b = box.cpu().numpy().view(np.uint32).astype(np.int64)
    if b[0] == 0xFFFFFFFF:
        raise ValueError("empty liver mask")
    return out, b[:3], b[3:]


class _PostWorkspace:
    """the uint32 root / area words and the fill flags shared by every pass of one volume"""

    def __init__(self, shape, dev):
        self.shape, self.n, self.dev = shape, _check_volume(shape), dev
        self.root = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.area = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.flag = torch.empty(self.n, dtype=torch.uint8, device=dev)

    def mask(self):
        return torch.empty(self.n, dtype=torch.uint8, device=self.dev)

    def largest26(self, binary, out):
        """out = largest 26-connected component of binary; returns the device word counting the components"""
        ops.pp_label(binary, self.shape, 26, False, self.root)
        self.area.zero_()
        best = torch.zeros(1, dtype=torch.int64, device=self.dev)
        ncomp = torch.zeros(1, dtype=torch.int32, device=self.dev)
        ops.pp_largest(self.root, self.shape, self.area, best, ncomp, out)
        return ncomp

    def fill(self, binary, out):
        self.flag.zero_()
        ops.pp_fill_holes(binary, self.shape, self.root, self.flag, out)


def segment_liver_tumor_device(score, count, shape, mask_dev, thres_liver=0.5, thres_tumor=0.8):
    """segment_liver_tumor on the device, from the sweep's own accumulators (sweep_scores): score float32 device tensor
    [z][deps][rows][num], count the windows per plane ([z], host or device), shape = (x, y, z) of the CT volume, mask_dev
    the dilated coarse liver mask of liver_window_from_mask_device.  Returns the uint8 label volume (x, y, z)."""
    shape = tuple(int(v) for v in shape)
    return _segment_liver_tumor_labels(score, count, shape, mask_dev, thres_liver, thres_tumor).cpu().numpy().reshape(shape)


def _segment_liver_tumor_labels(score, count, shape, mask_dev, thres_liver, thres_tumor):
    """segment_liver_tumor_device up to the download: the flat uint8 label volume, still on the device"""
    ws = _PostWorkspace(shape, score.device)
    if mask_dev.dtype != torch.uint8 or mask_dev.numel() != ws.n or mask_dev.device != score.device:
        raise ValueError("mask_dev: the uint8 device mask of liver_window_from_mask_device for this volume")
    if not torch.is_tensor(count):
        count = torch.from_numpy(np.asarray(count, np.float32).reshape(-1))
    count = count.to(device=score.device, dtype=torch.float32).contiguous()
    liver, tumor = ws.mask(), ws.mask()
    ops.pp_threshold(score.contiguous(), count, shape, thres_liver, thres_tumor, liver, tumor)
    a, b = ws.mask(), ws.mask()
    n_liver = ws.largest26(liver, a)                  # liver_res = largest(result1)
    liver_res = ws.mask()
    ws.fill(a, liver_res)                             # liver_res = fill_holes(liver_res)
    ops.pp_dilate(mask_dev.contiguous(), shape, liver)            # the second dilation of test.py:95
    n_mask = ws.largest26(liver, a)
    ws.fill(a, b)                                     # liver_labels
    ops.pp_merge(ops.PP_AND, tumor, b, a)             # Segmask * liver_labels
    ws.fill(a, b)                                     # Segmask = fill_holes(...)
    ops.pp_merge(ops.PP_LABEL, liver_res, b, a)       # liver_res[Segmask == 1] = 2
    counts = torch.cat([n_liver, n_mask]).cpu().numpy()
    if counts[0] == 0 or counts[1] == 0:
        raise ValueError(_NO_COMPONENT)
    return a


def segment_volume(model, imgs_test, liver_mask, args, thres_liver=0.5, thres_tumor=0.9, mode="eager", preprocess=None):
    """test.py:52-112 in one call: the liver window of the coarse mask, the z-sliding-window sweep of `model` and the
    post-processing, with the scores, masks and labels resident in HBM; returns the uint8 label volume (x, y, z) that
    segment_liver_tumor(*predict_tumor_inwindow(...), liver_window_from_mask(liver_mask)[0], ...) computes.
    `mode` / `preprocess`: see sweep_scores (in graph mode the window counts never leave the device)."""
    shape = tuple(int(v) for v in np.shape(imgs_test)[:3])
    if tuple(np.shape(liver_mask)) != shape:
        raise ValueError("liver_mask must have the shape of the CT volume")
    mask_dev, mini, maxi = liver_window_from_mask_device(liver_mask)
    score, score_num = sweep_scores(model, imgs_test, 3, mini, maxi, args, mode=mode, preprocess=preprocess)
    return segment_liver_tumor_device(score, score_num, shape, mask_dev, thres_liver, thres_tumor)


def evaluate_volume(model, imgs_test, liver_mask, truth, args, spacing=None, thres_liver=0.5, thres_tumor=0.9, mode="eager",
                    preprocess=None):
    """segment_volume followed by metrics.evaluate_labels_device against the label volume `truth`, the predicted labels
    staying in HBM in between: returns (uint8 label volume (x, y, z), {"liver": {...}, "tumor": {...}}) -- what
    metrics.evaluate_labels(segment_volume(...), truth, spacing) computes on the host.
    `spacing`: None or the voxel size in mm along x, y, z; the other arguments are segment_volume's."""
    from . import metrics
    shape = tuple(int(v) for v in np.shape(imgs_test)[:3])
    if tuple(np.shape(liver_mask)) != shape or tuple(np.shape(truth)) != shape:
        raise ValueError("liver_mask and truth must have the shape of the CT volume")
    mask_dev, mini, maxi = liver_window_from_mask_device(liver_mask)
    score, score_num = sweep_scores(model, imgs_test, 3, mini, maxi, args, mode=mode, preprocess=preprocess)
    labels = _segment_liver_tumor_labels(score, score_num, shape, mask_dev, thres_liver, thres_tumor)
    evaluation = metrics.evaluate_labels_device(labels, truth, spacing, shape=shape)
    return labels.cpu().numpy().reshape(shape), evaluation


# ------------------------------------------------------------------ tiled 3-D sliding-window inference (lib/funcs.py:54-153)
# predict_window_mulgpu tiles the volume in ALL three axes with overlapping tiles (stride (t // 3) * 2 per axis, the last start
# clamped) and averages the softmax scores; get_binary_mask / GeneSeglivertumor keep the largest component of the 0.5 mask.
# Here the volume, the summed scores and the masks stay in HBM (sweep.TiledSweepPlan, include/hdu.h: hdu_tile_*).
def tiled_sweep_scores(model, imgs_test, num=3, mode="eager", preprocess=None):
    """the tile sweep of predict_window_mulgpu, left on the device: (score float32 device tensor [Z][X][Y][num] of summed
    softmax scores, (cx, cy, cz) float32 device vectors: cx[x] * cy[y] * cz[z] tiles covered voxel (x, y, z)).  Both are the
    plan's own buffers, valid until the next tiled sweep of this model.
    The tile is the model's input window and `batch` its window_batch; the last, partly filled step runs too and adds only its
    valid slots (the reference never predicts those tiles: see predict_window_mulgpu).
    mode="eager": every step driven from the host, which sets the step cursor.  mode="graph": one captured step replayed
    ceil(tiles / batch) times.  Both run the same launches.
    preprocess=(lo, hi, mean): `imgs_test` is raw; the tile gather writes min(max(v, lo), hi) - mean."""
    if mode not in ("eager", "graph"):
        raise ValueError("mode: 'eager' or 'graph', not %r" % (mode,))
    if model.kind != "hybrid" or model.ctx.shard_world() > 1:
        raise ValueError("the tiled sweep drives the unsharded hybrid nets")
    shape = tuple(int(v) for v in np.shape(imgs_test)[:3])
    _, deps, rows, cols, _ = model.input_shape
    if len(shape) != 3 or shape[0] < deps or shape[1] < rows or shape[2] < cols:
        raise ValueError("volume smaller than the network window")
    return sweep.tiled_plan_for(model, shape, num, preprocess).sweep(imgs_test, graph=(mode == "graph"))


def _check_window_call(model, batch, imgs_test, img_deps, img_rows, img_cols, multiloss):
    if multiloss:
        raise ValueError("multiloss=True selects output [2] of a deep-supervision model; these models have one output")
    if model.kind != "hybrid" or model.ctx.shard_world() > 1:
        raise ValueError("the tiled sweep drives the unsharded hybrid nets")
    W, deps, rows, cols, _ = model.input_shape
    if int(batch) != W:
        raise ValueError("batch=%d: the model was built with window_batch=%d" % (batch, W))
    if (int(img_deps), int(img_rows), int(img_cols)) != (deps, rows, cols):
        raise ValueError("tile %s: the model's window is %s" % ((img_deps, img_rows, img_cols), (deps, rows, cols)))
    shape = tuple(int(v) for v in np.shape(imgs_test)[:3])
    if len(shape) != 3 or shape[0] < deps or shape[1] < rows or shape[2] < cols:
        raise ValueError("volume smaller than the network window (the reference dies on a broadcast error here)")
    return shape


def predict_window_mulgpu(model, batch, imgs_test, img_deps, img_rows, img_cols, multiloss, mode="eager", channel=1,
                          preprocess=None):
    """Drop-in for lib/funcs.py:54-129: the float32 (x, y, z) volume of the averaged class-`channel` softmax scores of the
    overlapping tiles (score / score_num, no epsilon; the reference returns channel 1).
    Deviation: the reference predicts a box only when it is full, so with a tile count that is no multiple of `batch` it never
    runs the leftover tiles and the voxels only they cover come out NaN (0 / 0).  Here the last, partly filled step runs too:
    every voxel is covered, and the result equals the reference's wherever that is defined (batch == 1, or a tile count that
    is a multiple of `batch`).
    `batch` must be the model's window_batch and the tile its input window; multiloss must be False."""
    shape = _check_window_call(model, batch, imgs_test, img_deps, img_rows, img_cols, multiloss)
    if not 0 <= int(channel) < 3:
        raise ValueError("channel: 0..2")
    score, (cx, cy, cz) = tiled_sweep_scores(model, imgs_test, 3, mode=mode, preprocess=preprocess)
    out = torch.empty(shape, dtype=torch.float32, device=score.device)
    ops.tile_finalize(score, shape, 3, int(channel), cx, cy, cz, out_score=out.reshape(-1))
    return out.cpu().numpy()


def GeneSeglivertumor(score):
    """lib/funcs.py:138-153: `score` is thresholded IN PLACE at 0.5 (as the reference does) and the largest 26-connected
    component of the result comes back (first label wins a tie; ValueError on an empty mask, where the reference raises on
    max([]))."""
    score[score >= 0.5] = 1
    score[score < 0.5] = 0
    return _largest_component(score)


def get_binary_mask(score, id=None):
    """lib/funcs.py:131-136: np.int16(GeneSeglivertumor(score)); `id` is unused there too"""
    return np.int16(GeneSeglivertumor(score))


def segment_tiled_scores(score, coverage, shape, thres=0.5, channel=1):
    """get_binary_mask on the device, from the tiled sweep's own accumulators (tiled_sweep_scores): score float32 device
    tensor [Z][X][Y][num], coverage = its (cx, cy, cz), shape = (x, y, z).  hdu_tile_finalize writes the mask only; only the
    int16 label volume and the component count come back."""
    shape = tuple(int(v) for v in shape)
    num = int(score.shape[-1])
    if not 0 <= int(channel) < num:
        raise ValueError("channel: 0..%d" % (num - 1))
    ws = _PostWorkspace(shape, score.device)
    mask, out = ws.mask(), ws.mask()
    ops.tile_finalize(score, shape, num, int(channel), *coverage, thres=thres, out_mask=mask)
    ncomp = ws.largest26(mask, out)
    labels = out.to(torch.int16)
    if int(ncomp.cpu()[0]) == 0:
        raise ValueError(_NO_COMPONENT)
    return labels.cpu().numpy().reshape(shape)


def segment_volume_tiled(model, imgs_test, mode="eager", thres=0.5, channel=1, preprocess=None):
    """get_binary_mask(predict_window_mulgpu(...)) with nothing but the int16 label volume and the component count coming back
    to the host: tiled sweep -> hdu_tile_finalize (mask only) -> largest 26-connected component on the device.  Bit-identical
    to the host form."""
    if model.kind != "hybrid" or model.ctx.shard_world() > 1:
        raise ValueError("the tiled sweep drives the unsharded hybrid nets")
    W, deps, rows, cols, _ = model.input_shape
    shape = _check_window_call(model, W, imgs_test, deps, rows, cols, False)
    if not 0 <= int(channel) < 3:
        raise ValueError("channel: 0..2")
    score, coverage = tiled_sweep_scores(model, imgs_test, 3, mode=mode, preprocess=preprocess)
    return segment_tiled_scores(score, coverage, shape, thres, channel)


# ------------------------------------------------------------------ 2-D slice sweep and the CT cascade (test.py:52-112)
# test.py:58 loads the coarse liver mask `livermask/<id>-ori.nii` from a file; the network that makes it is the 2-D DenseUNet of
# train_2ddense.py, which sees the planes c-1, c, c+1 of the volume as the three channels of one slice (:58-61).  Here that net
# runs over every plane of a volume resident in HBM (sweep.SliceSweepPlan, include/hdu.h: hdu_slice_*) and the argmax labels
# stay there, so the cascade  raw CT -> coarse liver mask -> liver window -> hybrid sweep -> label volume  needs no host mask.
def _check_slice_call(model, imgs_test, mode):
    if mode not in ("eager", "graph"):
        raise ValueError("mode: 'eager' or 'graph', not %r" % (mode,))
    if model.kind != "2d" or model.ctx.shard_world() > 1 or getattr(model, "window_batch", 1) != 1:
        raise ValueError("the slice sweep drives the unsharded 2-D net (no window_batch)")
    shape = tuple(int(v) for v in np.shape(imgs_test)[:3])
    _, H, W, _ = model.input_shape
    if len(shape) != 3 or shape[0] < H or shape[1] < W or shape[2] < 1:
        raise ValueError("volume smaller than the network window")
    return shape


def slice_sweep_labels(model, imgs_test, mode="eager", preprocess=None):
    """the 2-D `model` over every plane of the (x, y, z) volume, left on the device: the uint8 labels {0, 1, 2} (argmax of the
    three logits, first maximum) as a flat device tensor in raster order [x][y][z], zero outside the model's top-left H x W
    window.  It is the plan's own buffer, valid until the next slice sweep of this model.
    Plane c is predicted from the planes c-1, c, c+1; the end planes are replicated (include/hdu.h).  `batch` = the model's b
    planes run per forward; the padding slots of the last step repeat the last plane and store nothing.
    mode="eager": every step driven from the host, which sets the step cursor.  mode="graph": one captured step replayed
    ceil(z / b) times.  Both run the same launches.
    preprocess=(lo, hi, mean): `imgs_test` is raw; the gather writes min(max(v, lo), hi) - mean."""
    shape = _check_slice_call(model, imgs_test, mode)
    return sweep.slice_plan_for(model, shape, preprocess).sweep(imgs_test, graph=(mode == "graph"))


def segment_volume_2d(model, imgs_test, mode="eager", preprocess=None):
    """slice_sweep_labels as a host uint8 array (x, y, z): the 2-D DenseUNet as a whole-volume segmenter"""
    shape = _check_slice_call(model, imgs_test, mode)
    labels = slice_sweep_labels(model, imgs_test, mode=mode, preprocess=preprocess)
    return labels.cpu().numpy().reshape(shape).copy()          # (the plan's buffer is reused: never hand out a view of it)


def slice_labels_host(model, imgs_test, preprocess=None):
    """the host composition segment_volume_2d replaces, and its specification: numpy batches of (c-1, c, c+1) slices with the
    same edge-plane and padding rules, Model.predict, np.argmax; returns the uint8 array (x, y, z)"""
    shape = _check_slice_call(model, imgs_test, "eager")
    X, Y, Z = shape
    N, H, W, _ = model.input_shape
    vol = np.asarray(imgs_test, np.float32).reshape(shape)[:H, :W, :]
    if preprocess is not None:
        lo, hi, mean = (np.float32(v) for v in preprocess)
        vol = np.clip(vol, lo, hi) - mean
    out = np.zeros(shape, np.uint8)
    for s0 in range(0, Z, N):
        centres = [min(s0 + i, Z - 1) for i in range(N)]
        x = np.stack([np.stack([vol[:, :, min(max(c + k - 1, 0), Z - 1)] for k in range(3)], axis=-1) for c in centres])
        lab = np.argmax(model.predict(x), axis=-1).astype(np.uint8)
        for i in range(min(N, Z - s0)):
            out[:H, :W, s0 + i] = lab[i]
    return out


def coarse_liver_mask_device(model, imgs_test, mode="eager", preprocess=None, largest=True):
    """the coarse liver mask test.py:58 reads from `livermask/`, made on the device: labels != 0 of slice_sweep_labels (liver
    and tumour merged, as liver_window_from_mask merges them), as a flat uint8 device tensor in raster order.  largest=True
    keeps its largest 26-connected component (ValueError "no foreground component" when there is none)."""
    shape = _check_slice_call(model, imgs_test, mode)
    labels = slice_sweep_labels(model, imgs_test, mode=mode, preprocess=preprocess)
    ws = _PostWorkspace(shape, labels.device)
    out = ws.mask()
    if not largest:
        ops.pp_merge(ops.PP_AND, labels, labels, out)          # out = labels != 0
        return out
    ncomp = ws.largest26(labels, out)                          # (nonzero = set: the labels serve as the mask)
    if int(ncomp.cpu()[0]) == 0:
        raise ValueError(_NO_COMPONENT)
    return out


def _segment_ct_labels(model2d, model_hybrid, imgs_test, args, thres_liver, thres_tumor, mode, preprocess, largest):
    """segment_ct up to the download: the flat uint8 label volume, still on the device"""
    shape = tuple(int(v) for v in np.shape(imgs_test)[:3])
    coarse = coarse_liver_mask_device(model2d, imgs_test, mode=mode, preprocess=preprocess, largest=largest)
    mask_dev, mini, maxi = liver_window_from_device_mask(coarse, shape)
    score, score_num = sweep_scores(model_hybrid, imgs_test, 3, mini, maxi, args, mode=mode, preprocess=preprocess)
    return _segment_liver_tumor_labels(score, score_num, shape, mask_dev, thres_liver, thres_tumor)


def segment_ct(model2d, model_hybrid, imgs_test, args, thres_liver=0.5, thres_tumor=0.9, mode="eager", preprocess=None,
               largest=True):
    """the whole cascade of test.py without the `livermask/` file: the 2-D net's coarse liver mask (coarse_liver_mask_device),
    its liver window, the z-sliding-window sweep of the hybrid net and the post-processing; returns the uint8 label volume
    (x, y, z) that segment_volume(model_hybrid, imgs_test, <that coarse mask on the host>, args, ...) computes.  The coarse mask
    never leaves the device: the volume goes up (once per stage), the bounding box and the labels come down.
    `args` are the hybrid's (b = 1, input_size, input_cols); `mode` / `preprocess` apply to both stages."""
    shape = tuple(int(v) for v in np.shape(imgs_test)[:3])
    labels = _segment_ct_labels(model2d, model_hybrid, imgs_test, args, thres_liver, thres_tumor, mode, preprocess, largest)
    return labels.cpu().numpy().reshape(shape)


def evaluate_ct(model2d, model_hybrid, imgs_test, truth, args, spacing=None, thres_liver=0.5, thres_tumor=0.9, mode="eager",
                preprocess=None, largest=True):
    """segment_ct followed by metrics.evaluate_labels_device against the label volume `truth`, the predicted labels staying in
    HBM in between: returns (uint8 label volume (x, y, z), {"liver": {...}, "tumor": {...}}), like evaluate_volume"""
    from . import metrics
    shape = tuple(int(v) for v in np.shape(imgs_test)[:3])
    if tuple(np.shape(truth)) != shape:
        raise ValueError("truth must have the shape of the CT volume")
    labels = _segment_ct_labels(model2d, model_hybrid, imgs_test, args, thres_liver, thres_tumor, mode, preprocess, largest)
    evaluation = metrics.evaluate_labels_device(labels, truth, spacing, shape=shape)
    return labels.cpu().numpy().reshape(shape), evaluation
