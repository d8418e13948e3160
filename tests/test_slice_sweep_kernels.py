"""The kernels of the 2-D slice sweep (include/hdu.h: hdu_slice_gather_batched / _argmax_store / _labels_to_raster): the step
index comes from one device word.  Gather against numpy slicing with replicated end planes (bit-exact), argmax against
np.argmax (first maximum, signed zeros tie), raster against the numpy transpose with zero padding, and every bad-argument case
refused with the outputs untouched.  No model is built here."""
import ctypes

import numpy as np
import pytest
import torch

import parity_utils as U


def _dev(hdu):
    return U.pkg("ops").device()


def _i32(vals, dev):
    return torch.tensor(np.asarray(vals, np.int32).reshape(-1), dtype=torch.int32, device=dev)


def _slot_of(vol_zxy, c, H, W):
    """the slot of centre plane c as the model input holds it, [H][W][3]: planes c-1, c, c+1, the end planes replicated"""
    Z = vol_zxy.shape[0]
    return np.stack([vol_zxy[min(max(c + k - 1, 0), Z - 1), :H, :W] for k in range(3)], axis=-1)


# ------------------------------------------------------------------ gather
# (X, Y, Z, H, W, batch): two steps, the last with one valid slot / Z = 1 (all three channels are the one plane) and a cropped
# window / more than one workgroup per slot
GATHER_CASES = [(5, 7, 4, 5, 7, 3), (9, 11, 1, 5, 7, 2), (40, 36, 11, 32, 32, 8)]
GATHER_IDS = ["5x7x4b3", "9x11x1b2", "40x36x11b8"]


@pytest.mark.parametrize("offset", [0, 1, 3], ids=["src16", "src4", "src12"])
@pytest.mark.parametrize("case", GATHER_CASES, ids=GATHER_IDS)
def test_slice_gather_equals_numpy_slicing(hdu, case, offset):
    """`offset` floats in front of the volume and a destination 0 or 1 float into its buffer move both alignments; sentinels on
    both sides of the destination stay; a NaN inside the window moves as bits.  EVERY step is run, and cursor words of 99 and -1
    must come out as the last and the first step.  Padding slots repeat the last plane."""
    ops, dev = U.pkg("ops"), _dev(hdu)
    X, Y, Z, H, W, batch = case
    n = H * W * 3
    rng = np.random.default_rng(X * 100 + offset * 10 + batch)
    host = rng.normal(0.0, 300.0, offset + X * Y * Z).astype(np.float32)
    vol_h = host[offset:].reshape(Z, X, Y)
    vol_h[Z // 2, 1, 1] = np.float32("nan")
    vol = torch.from_numpy(host).to(dev)[offset:]
    nsteps = -(-Z // batch)
    saw_nan, seen = False, set()
    for dst_off in (0, 1):
        for word in list(range(nsteps)) + [99, -1]:
            step = min(max(word, 0), nsteps - 1)
            cursor = _i32([word], dev)
            out = torch.full((dst_off + batch * n + 4,), -7.0, dtype=torch.float32, device=dev)
            ops.slice_gather_batched(vol, (X, Y, Z), (H, W), cursor, batch, out[dst_off:dst_off + batch * n])
            got = out.cpu().numpy()
            for i in range(batch):
                c = min(step * batch + i, Z - 1)
                want = np.ascontiguousarray(_slot_of(vol_h, c, H, W)).reshape(-1)
                saw_nan |= bool(np.isnan(want).any())
                seen.add(c)
                g = got[dst_off + i * n: dst_off + (i + 1) * n]
                assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), (dst_off, word, i)
            assert (got[:dst_off] == -7.0).all() and (got[dst_off + batch * n:] == -7.0).all()
            assert int(cursor.cpu()[0]) == word                   # the gather reads the cursor, it never writes it
    assert saw_nan and seen == set(range(Z))


@pytest.mark.parametrize("case", GATHER_CASES, ids=GATHER_IDS)
def test_slice_gather_preprocess(hdu, case):
    """raw HU values -1000..1000 -> clip to [-200, 250] and subtract the mean 48 (preprocessing.py:15-16, test.py:55), float32;
    the value table of test_tile_gather_preprocess sits in the first row of plane 0, inside every window"""
    ops, dev = U.pkg("ops"), _dev(hdu)
    X, Y, Z, H, W, batch = case
    n = H * W * 3
    rng = np.random.default_rng(X)
    host = rng.uniform(-1000.0, 1000.0, 1 + X * Y * Z).astype(np.float32)
    table = np.array([-1000.0, 1000.0, -200.0, 250.0, -200.5, 250.5, 48.0, 0.0], np.float32)
    vol_h = host[1:].reshape(Z, X, Y)
    vol_h[0, 0, :4] = table[:4]                                  # (two rows of four: inside the window of every case)
    vol_h[0, 1, :4] = table[4:]
    vol = torch.from_numpy(host).to(dev)[1:]
    for step in range(-(-Z // batch)):
        out = torch.zeros(batch * n, dtype=torch.float32, device=dev)
        ops.slice_gather_batched(vol, (X, Y, Z), (H, W), _i32([step], dev), batch, out, preprocess=(-200, 250, 48))
        got = out.cpu().numpy()
        for i in range(batch):
            v = np.ascontiguousarray(_slot_of(vol_h, min(step * batch + i, Z - 1), H, W)).reshape(-1)
            want = np.clip(v, -200, 250).astype(np.float32) - np.float32(48)
            assert np.array_equal(got[i * n:(i + 1) * n].view(np.uint32), want.view(np.uint32))
            if step == 0 and i == 0:
                assert set(want.tolist()) >= {-248.0, 202.0, 0.0, -48.0}


# ------------------------------------------------------------------ argmax
def _logits(dev, dtype, M, ld, seed):
    """logits [M][ld] drawn from {-2, -1, -0.0, 0.0, 1, 2} (exact in bfloat16), ties common; the first rows are seeded: all
    three equal, the first two tied for the maximum, the last two tied, and (-0.0, 0.0, -0.0)"""
    ops, lib = U.pkg("ops"), U.pkg("lib")
    hd = lib.HDU_BF16 if dtype == "bf16" else lib.HDU_F32
    rng = np.random.default_rng(seed)
    vals = np.array([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0], np.float32)
    raw = vals[rng.integers(0, 6, (M, ld))]
    raw[0, :3] = [1.0, 1.0, 1.0]
    raw[1, :3] = [2.0, 2.0, -1.0]
    raw[2, :3] = [-1.0, 1.0, 1.0]
    raw[3, :3] = [-0.0, 0.0, -0.0]
    raw[:, 3:] = 9.0                                             # (the padding channels are larger than any class and never win)
    buf = torch.from_numpy(raw.reshape(-1)).to(torch.bfloat16 if dtype == "bf16" else torch.float32).to(dev)
    return ops.Act(buf, 0, 1, 1, 1, M, 3, ld, hd), raw[:, :3]


@pytest.mark.parametrize("ld", [3, 4, 8])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_slice_argmax_equals_numpy_argmax(hdu, dtype, ld):
    """plane 35, Z 4, batch 3: step 0 stores planes 0..2, step 1 plane 3 only (its slots 1 and 2 are past the volume and write
    nothing); labels prefilled with 7, four bytes past Z * plane included"""
    ops, dev = U.pkg("ops"), _dev(hdu)
    plane, Z, batch = 35, 4, 3
    for step in range(2):
        la, raw = _logits(dev, dtype, batch * plane, ld, seed=10 * ld + step)
        want = np.argmax(raw, axis=-1).astype(np.uint8).reshape(batch, plane)
        assert list(want.reshape(-1)[:4]) == [0, 0, 1, 0] and len(set(want.reshape(-1).tolist())) == 3
        buf = torch.full((Z * plane + 4,), 7, dtype=torch.uint8, device=dev)
        ops.slice_argmax_store(la, plane, Z, _i32([step], dev), batch, buf[:Z * plane])
        got = buf.cpu().numpy()
        assert (got[Z * plane:] == 7).all()
        got = got[:Z * plane].reshape(Z, plane)
        for zz in range(Z):
            i = zz - step * batch
            if 0 <= i < batch:
                assert np.array_equal(got[zz], want[i]), (step, zz)
            else:
                assert (got[zz] == 7).all(), (step, zz)


# ------------------------------------------------------------------ raster
RASTER_CASES = [(5, 7, 4, 5, 7), (9, 11, 3, 5, 7), (40, 36, 11, 32, 32), (3, 3, 130, 3, 3), (70, 67, 65, 64, 64)]


@pytest.mark.parametrize("case", RASTER_CASES, ids=["5x7x4", "9x11x3", "40x36x11", "3x3x130", "70x67x65"])
def test_slice_labels_to_raster_equals_numpy_transpose(hdu, case):
    """Z a multiple of four and not, Z and Y past one 64-tile, windows equal to and smaller than the plane; the output starts 0
    and 1 byte into its buffer (whole-word and byte stores) between sentinels"""
    ops, dev = U.pkg("ops"), _dev(hdu)
    X, Y, Z, H, W = case
    rng = np.random.default_rng(X + Z)
    lab = rng.integers(0, 3, (Z, H, W)).astype(np.uint8)
    want = np.zeros((X, Y, Z), np.uint8)
    want[:H, :W, :] = lab.transpose(1, 2, 0)
    labels = torch.from_numpy(lab.reshape(-1)).to(dev)
    for off in (0, 1):
        buf = torch.full((off + X * Y * Z + 5,), 7, dtype=torch.uint8, device=dev)
        ops.slice_labels_to_raster(labels, (X, Y, Z), (H, W), buf[off:off + X * Y * Z])
        got = buf.cpu().numpy()
        assert (got[:off] == 7).all() and (got[off + X * Y * Z:] == 7).all()
        assert np.array_equal(got[off:off + X * Y * Z].reshape(X, Y, Z), want)
    assert len(np.unique(want)) == 3


# ------------------------------------------------------------------ argument errors
def test_slice_argument_errors_leave_outputs_unchanged(hdu):
    ops, lib, dev = U.pkg("ops"), U.pkg("lib"), _dev(hdu)
    L = lib.get()
    X, Y, Z, H, W, batch = 8, 9, 5, 4, 6, 2
    plane, n = H * W, H * W * 3
    vol = torch.arange(X * Y * Z, dtype=torch.float32, device=dev)
    dst = torch.full((batch * n,), -1.0, dtype=torch.float32, device=dev)
    cursor = _i32([1], dev)
    la, raw = _logits(dev, "f32", batch * plane, 4, seed=5)
    planes = torch.full((Z * plane,), 7, dtype=torch.uint8, device=dev)
    out = torch.full((X * Y * Z,), 9, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ops.stream()

    def gather(vol_p=p(vol), X_=X, Y_=Y, Z_=Z, H_=H, W_=W, cursor_p=p(cursor), batch_=batch, pre=0, lo=0.0, hi=0.0, dst_p=p(dst)):
        return L.hdu_slice_gather_batched(vol_p, X_, Y_, Z_, H_, W_, cursor_p, batch_, pre, lo, hi, 0.0, dst_p, st)

    def argmax(dtype=lib.HDU_F32, lg=la.ptr, ldl=la.ld, plane_=plane, Z_=Z, cursor_p=p(cursor), batch_=batch, lab_p=p(planes)):
        return L.hdu_slice_argmax_store(dtype, lg, ldl, plane_, Z_, cursor_p, batch_, lab_p, st)

    def raster(lab_p=p(planes), X_=X, Y_=Y, Z_=Z, H_=H, W_=W, out_p=p(out)):
        return L.hdu_slice_labels_to_raster(lab_p, X_, Y_, Z_, H_, W_, out_p, st)

    bad = [
        (gather, dict(H_=X + 1)), (gather, dict(W_=Y + 1)), (gather, dict(batch_=0)), (gather, dict(batch_=ops.SLICE_MAX_BATCH + 1)),
        (gather, dict(Z_=0)), (gather, dict(vol_p=None)), (gather, dict(cursor_p=None)), (gather, dict(dst_p=None)),
        (gather, dict(H_=0)), (gather, dict(pre=1, lo=2.0, hi=1.0)), (gather, dict(dst_p=ctypes.c_void_p(dst.data_ptr() + 2))),
        (argmax, dict(ldl=2)), (argmax, dict(dtype=7)), (argmax, dict(lg=None)), (argmax, dict(cursor_p=None)),
        (argmax, dict(lab_p=None)), (argmax, dict(batch_=0)), (argmax, dict(batch_=ops.SLICE_MAX_BATCH + 1)), (argmax, dict(Z_=0)),
        (argmax, dict(plane_=0)),
        (raster, dict(H_=X + 1)), (raster, dict(W_=Y + 1)), (raster, dict(Z_=0)), (raster, dict(lab_p=None)),
        (raster, dict(out_p=None)), (raster, dict(H_=0)),
    ]
    label = {gather: "slice_gather_batched", argmax: "slice_argmax_store", raster: "slice_labels_to_raster"}
    for fn, kw in bad:
        assert fn(**kw) == -1, kw                        # HDU_ERR_ARG
        assert label[fn] in L.hdu_last_error().decode(), kw
    assert ops.SLICE_MAX_BATCH == 64
    with pytest.raises(lib.HduError, match="slice_gather_batched"):
        ops.slice_gather_batched(vol, (X, Y, Z), (H, W), cursor, ops.SLICE_MAX_BATCH + 1, torch.zeros(65 * n, device=dev))
    assert (dst.cpu().numpy() == -1.0).all()
    assert (planes.cpu().numpy() == 7).all()
    assert (out.cpu().numpy() == 9).all()
    assert int(cursor.cpu()[0]) == 1
    # and the good calls still go through: step 1 of 3 holds the centre planes 2 and 3
    assert gather() == 0 and argmax() == 0 and raster() == 0
    v = vol.cpu().numpy().reshape(Z, X, Y)
    assert np.array_equal(dst.cpu().numpy()[n:], np.ascontiguousarray(_slot_of(v, 3, H, W)).reshape(-1))
    got = planes.cpu().numpy().reshape(Z, plane)
    want = np.argmax(raw, axis=-1).reshape(batch, plane)
    assert np.array_equal(got[2:4], want) and (got[:2] == 7).all() and (got[4:] == 7).all()
    o = out.cpu().numpy().reshape(X, Y, Z)
    assert np.array_equal(o[:H, :W, :], got.reshape(Z, H, W).transpose(1, 2, 0)) and (o[H:] == 0).all() and (o[:, W:] == 0).all()
