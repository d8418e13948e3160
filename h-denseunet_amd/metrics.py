"""Segmentation metrics of a LiTS label volume: Dice per case and global, VOE, RVD and the surface distances ASSD, maximum
and RMS, as MedPy 0.3.0's metric.binary computes them (the reference's requirements.txt; its dc, jc, ravd, asd, assd, hd with
connectivity 1).

Two forms.  The host functions (numpy + scipy only) are the specification.  The *_device functions compute the same
dictionaries with the volumes resident in HBM (include/hdu.h: hdu_metric_*): borders, an exact squared Euclidean distance
transform in float64 and bit-repeatable sums; only a handful of scalar words come back, in one copy per evaluation.

`result` / `reference` are 3-D arrays, nonzero = foreground; `spacing` is None (unit voxels) or three positive floats in mm
along x, y, z."""
import numpy as np

SURFACE_FIELDS = ("asd_rt", "asd_tr", "assd", "msd", "rmsd", "n_rt", "n_tr")
COUNT_FIELDS = ("n_result", "n_reference", "n_intersection")
STRUCTURES = (("liver", 0), ("tumor", 1))       # (name, class_mode of hdu_metric_*): label >= 1, label == 2


# ------------------------------------------------------------------ host specification
def overlap_counts(result, reference):
    """(|R|, |T|, |R & T|) as Python ints"""
    r = np.asarray(result) != 0
    t = np.asarray(reference) != 0
    return int(np.count_nonzero(r)), int(np.count_nonzero(t)), int(np.count_nonzero(r & t))


def dice_from_counts(nr, nt, ni):
    return 2.0 * ni / (nr + nt) if nr + nt else 0.0       # MedPy dc: 0.0 when both are empty


def jaccard_from_counts(nr, nt, ni):
    union = nr + nt - ni
    return ni / float(union) if union else 0.0            # MedPy jc


def rvd_from_counts(nr, nt, ni=None):
    return (nr - nt) / float(nt) if nt else float("nan")  # MedPy ravd raises on an empty reference; LiTS has such cases


def dice(result, reference):
    return dice_from_counts(*overlap_counts(result, reference))


def jaccard(result, reference):
    return jaccard_from_counts(*overlap_counts(result, reference))


def voe(result, reference):
    return 1.0 - jaccard(result, reference)


def rvd(result, reference):
    return rvd_from_counts(*overlap_counts(result, reference))


def border(mask):
    """mask ^ binary_erosion(mask, 6-connected cross, border_value 0): an object voxel on a face of the volume is border"""
    from scipy import ndimage
    m = np.asarray(mask) != 0
    return m ^ ndimage.binary_erosion(m, structure=ndimage.generate_binary_structure(m.ndim, 1), iterations=1)


def surface_distances(result, reference, spacing=None):
    """MedPy's __surface_distances with connectivity 1: the distance of every border voxel of `result` to the border of
    `reference`"""
    from scipy import ndimage
    r = np.asarray(result) != 0
    t = np.asarray(reference) != 0
    if not r.any():
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if not t.any():
        raise RuntimeError("The second supplied array does not contain any binary object.")
    dt = ndimage.distance_transform_edt(~border(t), sampling=spacing)
    return dt[border(r)]


def _summarise(n_rt, sum_rt, sumsq_rt, max2_rt, n_tr, sum_tr, sumsq_tr, max2_tr):
    asd_rt, asd_tr = sum_rt / n_rt, sum_tr / n_tr
    return {"asd_rt": float(asd_rt), "asd_tr": float(asd_tr), "assd": float((asd_rt + asd_tr) / 2.0),
            "msd": float(np.sqrt(max(max2_rt, max2_tr))), "rmsd": float(np.sqrt((sumsq_rt + sumsq_tr) / (n_rt + n_tr))),
            "n_rt": int(n_rt), "n_tr": int(n_tr)}


def surface_metrics(result, reference, spacing=None):
    """asd_rt / asd_tr: directed mean surface distances; assd: their mean (MedPy assd); msd: the maximum over both directions
    (MedPy hd); rmsd: root mean square over both sample sets; n_rt / n_tr: border voxels sampled"""
    d_rt = surface_distances(result, reference, spacing)
    d_tr = surface_distances(reference, result, spacing)
    return _summarise(d_rt.size, d_rt.sum(), (d_rt ** 2).sum(), (d_rt ** 2).max(),
                      d_tr.size, d_tr.sum(), (d_tr ** 2).sum(), (d_tr ** 2).max())


def _nan_surface():
    out = {k: float("nan") for k in SURFACE_FIELDS}
    return out


def _overlap_entry(nr, nt, ni):
    return {"n_result": int(nr), "n_reference": int(nt), "n_intersection": int(ni), "dice": dice_from_counts(nr, nt, ni),
            "voe": 1.0 - jaccard_from_counts(nr, nt, ni), "rvd": rvd_from_counts(nr, nt)}


def evaluate_labels(pred, truth, spacing=None):
    """label volumes {0, 1, 2} -> {"liver": {...}, "tumor": {...}}: liver = label >= 1, tumour = label == 2; every entry holds
    the counts, dice, voe, rvd and the surface_metrics fields (nan where the structure is empty on either side)"""
    pred, truth = np.asarray(pred), np.asarray(truth)
    if pred.shape != truth.shape or pred.ndim != 3:
        raise ValueError("pred and truth: 3-D label volumes of one shape")
    out = {}
    for name, mode in STRUCTURES:
        r, t = (pred == 2, truth == 2) if mode else (pred >= 1, truth >= 1)
        nr, nt, ni = overlap_counts(r, t)
        e = _overlap_entry(nr, nt, ni)
        e.update(surface_metrics(r, t, spacing) if nr and nt else _nan_surface())
        out[name] = e
    return out


class ScoreBook:
    """per-case evaluations -> the figures the H-DenseUNet paper reports: Dice per case (mean over cases) and Dice global
    (2 sum I / (sum |R| + sum |T|)) per structure, and the nan-ignoring means of the remaining fields.  Host-only."""

    def __init__(self):
        self.cases = []

    def add(self, case_id, evaluation):
        self.cases.append((case_id, evaluation))

    def summary(self):
        out = {"cases": len(self.cases)}
        for name, _ in STRUCTURES:
            es = [ev[name] for _, ev in self.cases]
            nr, nt, ni = (sum(e[k] for e in es) for k in COUNT_FIELDS)
            s = {"dice_per_case": float(np.mean([e["dice"] for e in es])) if es else float("nan"),
                 "dice_global": dice_from_counts(nr, nt, ni)}
            for k in ("voe", "rvd", "asd_rt", "asd_tr", "assd", "msd", "rmsd"):
                v = np.array([e[k] for e in es], np.float64)
                v = v[~np.isnan(v)]
                s[k] = float(v.mean()) if v.size else float("nan")
            out[name] = s
        return out


# ------------------------------------------------------------------ device form (include/hdu.h: hdu_metric_*)
def _check_spacing(spacing):
    if spacing is None:
        return None
    s = tuple(float(v) for v in spacing)
    if len(s) != 3 or not all(np.isfinite(v) and v > 0 for v in s):
        raise ValueError("spacing: None or three positive floats (x, y, z)")
    return s


class _MetricWorkspace:
    """what one evaluation needs besides its inputs, shared by both directions and both structures: two uint8 border
    volumes, the float64 distance field and its pass buffer, the partial sums and the result words"""
    WORDS = 22          # per structure: 3 counts + 2 directions x (n, sum d, sum d2, max d2)

    def __init__(self, shape, dev):
        import torch
        from . import funcs, ops
        self.shape, self.n, self.dev = tuple(int(v) for v in shape), funcs._check_volume(shape), dev
        self.border_r = torch.empty(self.n, dtype=torch.uint8, device=dev)
        self.border_t = torch.empty(self.n, dtype=torch.uint8, device=dev)
        self.d2 = torch.empty(self.n, dtype=torch.float64, device=dev)
        self.tmp = torch.empty(self.n, dtype=torch.float64, device=dev)
        self.partial = torch.empty(4 * ops.METRIC_PARTIALS, dtype=torch.float64, device=dev)
        self.words = torch.zeros(self.WORDS, dtype=torch.int64, device=dev)

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.border_r, self.border_t, self.d2, self.tmp, self.partial, self.words))

    def surface(self, result, reference, class_mode, spacing, words):
        """words[0:4] <- result's border sampled in the reference border's distance field, words[4:8] <- the reverse"""
        from . import ops
        ops.metric_border(result, self.shape, class_mode, self.border_r)
        ops.metric_border(reference, self.shape, class_mode, self.border_t)
        ops.metric_edt(self.border_t, self.shape, spacing, self.tmp, self.d2)
        ops.metric_sample(self.border_r, self.d2, self.shape, self.partial, words[0:4])
        ops.metric_edt(self.border_r, self.shape, spacing, self.tmp, self.d2)
        ops.metric_sample(self.border_t, self.d2, self.shape, self.partial, words[4:8])


def _to_device_u8(a, shape, labels):
    """host array (uploaded once as uint8) or flat uint8 device tensor + shape -> (flat uint8 tensor, shape)"""
    import torch
    from . import funcs, ops
    if torch.is_tensor(a):
        if shape is None:
            raise ValueError("a device tensor needs `shape`")
        shape = tuple(int(v) for v in shape)
        if a.dtype != torch.uint8 or a.dim() != 1 or a.numel() != funcs._check_volume(shape):
            raise ValueError("device volumes: flat uint8 tensors of x * y * z elements")
        return a.contiguous(), shape
    h = np.asarray(a)
    if h.ndim != 3 or (shape is not None and tuple(shape) != h.shape):
        raise ValueError("a 3-D volume is required")
    n = funcs._check_volume(h.shape)
    u8 = h.astype(np.uint8) if labels else (h != 0).view(np.uint8)
    return torch.from_numpy(np.ascontiguousarray(u8).reshape(n)).to(ops.device()), tuple(int(v) for v in h.shape)


def _surface_from_words(w):
    """8 result words of _MetricWorkspace.surface -> the surface_metrics dict"""
    f = w.view(np.float64)
    return _summarise(int(w[0]), f[1], f[2], f[3], int(w[4]), f[5], f[6], f[7])


def surface_metrics_device(result, reference, spacing=None, shape=None):
    """surface_metrics with the volumes in HBM: host arrays, or flat uint8 device tensors together with `shape`"""
    spacing = _check_spacing(spacing)
    r, shape = _to_device_u8(result, shape, False)
    t, shape_t = _to_device_u8(reference, shape, False)
    if shape_t != shape or r.device != t.device:
        raise ValueError("result and reference: volumes of one shape on one device")
    ws = _MetricWorkspace(shape, r.device)
    ws.surface(r, t, 0, spacing, ws.words)
    w = ws.words[:8].cpu().numpy()
    if w[0] == 0:
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if w[4] == 0:
        raise RuntimeError("The second supplied array does not contain any binary object.")
    return _surface_from_words(w)


def evaluate_labels_device(pred, truth, spacing=None, shape=None):
    """evaluate_labels with the label volumes in HBM: host arrays, or flat uint8 device tensors together with `shape`.
    The liver and tumour masks are never materialised: every kernel reads the labels under a class mode."""
    from . import ops
    spacing = _check_spacing(spacing)
    p, shape = _to_device_u8(pred, shape, True)
    t, shape_t = _to_device_u8(truth, shape, True)
    if shape_t != shape or p.device != t.device:
        raise ValueError("pred and truth: 3-D label volumes of one shape on one device")
    ws = _MetricWorkspace(shape, p.device)
    for i, (_, mode) in enumerate(STRUCTURES):
        w = ws.words[11 * i:11 * i + 11]
        ops.metric_counts(p, t, shape, mode, w[0:3])
        ws.surface(p, t, mode, spacing, w[3:11])
    words = ws.words.cpu().numpy()
    out = {}
    for i, (name, _) in enumerate(STRUCTURES):
        w = words[11 * i:11 * i + 11]
        nr, nt, ni = (int(v) for v in w[:3])
        e = _overlap_entry(nr, nt, ni)
        e.update(_surface_from_words(w[3:]) if nr and nt else _nan_surface())
        out[name] = e
    return out
