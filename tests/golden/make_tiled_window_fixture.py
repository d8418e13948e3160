#!/usr/bin/env python
"""tests/golden/make_tiled_window_fixture.py -- TEST INFRASTRUCTURE: golden vectors of the tiled 3-D sliding-window inference
produced BY THE REFERENCE'S OWN lib/funcs.py:predict_window_mulgpu (imported unmodified through oracle.ref_keras.harness, over
the eager backend).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_tiled_window_fixture.py

The function is Python 2 (`window_deps = (img_deps/3)*2` feeds xrange): the tile sizes are handed over as ints whose `/`
floors like Python 2's; nothing in the reference is edited.  The model is a deterministic two-class stand-in with the one
method the loop calls (`predict(box, verbose)` -> (batch, deps, rows, cols, 2) logits, a fixed function of the CT value and of
the in-tile x, y, z position), so the fixture pins the TILING: the per-axis starts incl. the clamped last one, the tile order,
the boxes of `batch` tiles, the overlap counts, the final division -- and, in the last case, the tiles the reference never
predicts when their number is no multiple of `batch` (NaN = 0 / 0 where only they cover).  tests/test_tiled_window.py holds
its numpy restatement (the thing the product's HBM-resident sweep is tested against) to these arrays.
Writes tests/golden/ref_funcs_tiled_window.npz.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.dont_write_bytecode = True


class Py2Int(int):
    """an int whose true division floors, as `/` did for ints in the Python 2 the reference was written for"""

    def __truediv__(self, other):
        return Py2Int(int(self) // int(other))


class StandInModel2:
    """two-class logits = fixed affine maps of the CT value plus terms in the in-tile x, y, z position (so that a mis-placed
    tile, a wrong tile order inside a box or a wrong overlap count changes the result), float32 like a Keras predict"""

    def predict(self, box, batch_size=None, verbose=0):
        b, d, r, c, _ = box.shape
        x = box[..., 0].astype(np.float64)
        xx = np.arange(d, dtype=np.float64)[None, :, None, None]
        yy = np.arange(r, dtype=np.float64)[None, None, :, None]
        zz = np.arange(c, dtype=np.float64)[None, None, None, :]
        out = np.stack([0.01 * x + 0.05 * zz - 0.02 * xx, -0.02 * x + 0.03 * yy + 0.04 * xx - 0.01 * zz], -1)
        return out.astype(np.float32)


CASES = [   # (volume shape, tile, batch); the last one drops its tail tiles (36 tiles, batch 5)
    ((20, 17, 13), (9, 8, 6), 1),
    ((16, 16, 12), (16, 8, 6), 1),
    ((22, 14, 9), (9, 9, 6), 2),
    ((13, 13, 13), (6, 6, 6), 3),
    ((20, 17, 13), (9, 8, 6), 5),
]
SEED0 = 300


def main():
    sys.path.insert(0, ROOT)
    from oracle.ref_keras import harness as H
    if not H.available():
        sys.exit("the reference tree is not present")
    H.setup("float64")
    import funcs as ref_funcs                        # the reference's lib/funcs.py
    out = {}
    for i, (shape, tile, batch) in enumerate(CASES):
        vol = np.random.default_rng(SEED0 + i).normal(0.0, 40.0, shape).astype(np.float32)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = ref_funcs.predict_window_mulgpu(StandInModel2(), batch, vol, Py2Int(tile[0]), Py2Int(tile[1]), Py2Int(tile[2]),
                                                False)
        out["score%d" % i] = np.asarray(s, np.float32)             # (the volume is re-drawn from its seed by the test)
        out["meta%d" % i] = np.array(list(shape) + list(tile) + [batch, SEED0 + i], dtype=np.int64)
        print("case %d: volume %s tile %s batch %d -> mean %.6f, NaN voxels %d" %
              (i, shape, tile, batch, float(np.nanmean(s)), int(np.isnan(s).sum())))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "ref_funcs_tiled_window.npz"), **out)


if __name__ == "__main__":
    main()
