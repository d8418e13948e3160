"""The kernels of the tiled 3-D sliding-window sweep (include/hdu.h: hdu_tile_gather_batched / _accumulate / _finalize): the
tile start (x0, y0, z0) comes from a device table, a device step cursor and a device tile count.  Gather against numpy slicing
(bit-exact), accumulate against ops.softmax_accumulate plus numpy `+=` in slot order (bit-equal), finalize against the numpy
division and transpose (bit-equal), and every bad-argument case refused with the outputs untouched."""
import ctypes

import numpy as np
import pytest
import torch

import parity_utils as U


def _dev(hdu):
    return U.pkg("ops").device()


def _i32(vals, dev):
    return torch.tensor(np.asarray(vals, np.int32).reshape(-1), dtype=torch.int32, device=dev)


def _clamp(entry, shape, tile):
    return tuple(int(min(max(int(s), 0), n - t)) for s, n, t in zip(entry, shape, tile))


def _tile_of(vol_zxy, start, tile):
    """the tile as the model input holds it, [cols][deps][rows], out of the [Z][X][Y] volume"""
    (x0, y0, z0), (deps, rows, cols) = start, tile
    return vol_zxy[z0:z0 + cols, x0:x0 + deps, y0:y0 + rows]


# ------------------------------------------------------------------ gather
GATHER_CASES = [((11, 13, 9), (5, 7, 4)), ((40, 36, 11), (32, 32, 8))]


def _gather_table(shape, tile):
    """the far corner, a duplicate, two out-of-range entries that must clamp to (X-deps, 0, Z-cols) and (0, Y-rows, 0) -- every
    axis past both of its ends -- and odd starts"""
    far = tuple(n - t for n, t in zip(shape, tile))
    return [(0, 0, 0), (1, 3, 2), far, far, (99, -3, 99), (2, 1, 0), (3, 5, 1), (-4, 99, -2)]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("offset", [0, 1, 3], ids=["src16", "src4", "src12"])
@pytest.mark.parametrize("case", GATHER_CASES, ids=["row7", "row32"])
def test_tile_gather_equals_numpy_slicing(hdu, case, offset, batch):
    """rows of 7 floats in a volume of odd Y: no source row base is 16-byte aligned, every group of four crosses rows somewhere;
    rows of 32 floats take the vector load where the row base happens to be aligned.  `offset` floats in front of the volume
    and a destination one float into its buffer move both alignments.  ntiles = 6 of an 8-entry table: the last two entries are
    never valid, and are gathered all the same.  EVERY step of the table is run, so every entry is gathered at least once: the
    duplicate far corner and the out-of-range entry, which must come out as the tile at its clamped start."""
    ops, dev = U.pkg("ops"), _dev(hdu)
    shape, tile = case
    X, Y, Z = shape
    n = tile[0] * tile[1] * tile[2]
    rng = np.random.default_rng(X * 100 + offset * 10 + batch)
    host = rng.normal(0.0, 300.0, offset + X * Y * Z).astype(np.float32)
    vol_h = host[offset:].reshape(Z, X, Y)
    vol_h[1, 1, 1] = np.float32("nan")                        # (inside the first tile) a plain copy moves bits, whatever they encode
    vol = torch.from_numpy(host).to(dev)[offset:]
    table = _gather_table(shape, tile)
    starts, ntiles = _i32(table, dev), _i32([6], dev)
    assert _clamp((99, -3, 99), shape, tile) == (X - tile[0], 0, Z - tile[2])
    assert _clamp((-4, 99, -2), shape, tile) == (0, Y - tile[1], 0)
    nsteps = -(-len(table) // batch)
    saw_nan = False
    seen = set()
    for dst_off in (0, 1):
        for step in range(nsteps):
            cursor = _i32([step], dev)
            out = torch.full((dst_off + batch * n + 4,), -7.0, dtype=torch.float32, device=dev)
            ops.tile_gather_batched(vol, shape, tile, starts, ntiles, cursor, batch, out[dst_off:dst_off + batch * n])
            got = out.cpu().numpy()
            for i in range(batch):
                entry = min(step * batch + i, len(table) - 1)          # the entry is clamped to the table
                want = np.ascontiguousarray(_tile_of(vol_h, _clamp(table[entry], shape, tile), tile)).reshape(-1)
                saw_nan |= bool(np.isnan(want).any())
                seen.add(entry)
                g = got[dst_off + i * n: dst_off + (i + 1) * n]
                assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), (dst_off, step, i)
            assert (got[:dst_off] == -7.0).all() and (got[dst_off + batch * n:] == -7.0).all()
            assert int(cursor.cpu()[0]) == step
    assert saw_nan and seen == set(range(len(table)))


def test_tile_gather_slots_do_not_touch_their_neighbours(hdu):
    """sentinel floats between the slots: a destination of batch views cannot be given to one launch, so each slot is gathered
    as a batch-1 launch into a buffer with sentinels on both sides, and a batch-3 launch must reproduce the three"""
    ops, dev = U.pkg("ops"), _dev(hdu)
    shape, tile = (11, 13, 9), (5, 7, 4)
    X, Y, Z = shape
    n = tile[0] * tile[1] * tile[2]
    host = np.random.default_rng(5).normal(0.0, 9.0, X * Y * Z).astype(np.float32)
    vol = torch.from_numpy(host).to(dev)
    table = [(1, 2, 3), (6, 6, 5), (0, 4, 1)]
    starts, ntiles, cursor = _i32(table, dev), _i32([3], dev), _i32([0], dev)
    out3 = torch.full((1 + 3 * n + 1,), -7.0, dtype=torch.float32, device=dev)
    ops.tile_gather_batched(vol, shape, tile, starts, ntiles, cursor, 3, out3[1:1 + 3 * n])
    got3 = out3.cpu().numpy()
    assert got3[0] == -7.0 and got3[-1] == -7.0
    for i, st in enumerate(table):
        one = torch.full((2 + n + 2,), -7.0, dtype=torch.float32, device=dev)
        ops.tile_gather_batched(vol, shape, tile, _i32([st], dev), _i32([1], dev), _i32([0], dev), 1, one[2:2 + n])
        g = one.cpu().numpy()
        assert (g[:2] == -7.0).all() and (g[2 + n:] == -7.0).all()
        want = np.ascontiguousarray(_tile_of(host.reshape(Z, X, Y), st, tile)).reshape(-1)
        assert np.array_equal(g[2:2 + n], want)
        assert np.array_equal(got3[1 + i * n: 1 + (i + 1) * n], want)


@pytest.mark.parametrize("case", GATHER_CASES, ids=["row7", "row32"])
def test_tile_gather_preprocess(hdu, case):
    """raw HU values -1000..1000 -> clip to [-200, 250] and subtract the mean 48 (preprocessing.py:15-16, test.py:55), float32"""
    ops, dev = U.pkg("ops"), _dev(hdu)
    shape, tile = case
    X, Y, Z = shape
    n = tile[0] * tile[1] * tile[2]
    rng = np.random.default_rng(X)
    host = rng.uniform(-1000.0, 1000.0, 1 + X * Y * Z).astype(np.float32)
    host[1:9] = [-1000.0, 1000.0, -200.0, 250.0, -200.5, 250.5, 48.0, 0.0]
    vol = torch.from_numpy(host).to(dev)[1:]
    table = [(0, 0, 0), (1, 3, 2), tuple(n_ - t for n_, t in zip(shape, tile))]
    out = torch.zeros(3 * n, dtype=torch.float32, device=dev)
    ops.tile_gather_batched(vol, shape, tile, _i32(table, dev), _i32([3], dev), _i32([0], dev), 3, out, preprocess=(-200, 250, 48))
    got = out.cpu().numpy()
    for i, st in enumerate(table):
        v = np.ascontiguousarray(_tile_of(host[1:].reshape(Z, X, Y), st, tile)).reshape(-1)
        want = np.clip(v, -200, 250).astype(np.float32) - np.float32(48)
        assert np.array_equal(got[i * n:(i + 1) * n].view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------ accumulate
def _logits_act(dev, dtype, M, seed):
    """logits [M][ld] as the network leaves them: 3 classes in a padded row (ld 7 for float32, 8 = one chunk for bfloat16)"""
    ops, lib = U.pkg("ops"), U.pkg("lib")
    hd = lib.HDU_BF16 if dtype == "bf16" else lib.HDU_F32
    ld = 8 if dtype == "bf16" else 7
    rng = np.random.default_rng(seed)
    raw = torch.from_numpy(rng.normal(0.0, 3.0, M * ld).astype(np.float32))
    buf = raw.to(torch.bfloat16 if dtype == "bf16" else torch.float32).to(dev)
    return ops.Act(buf, 0, 1, 1, 1, M, 3, ld, hd)


@pytest.mark.parametrize("num", [1, 2, 3])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_tile_accumulate_equals_softmax_accumulate_in_slot_order(hdu, dtype, num):
    """two steps of 3 slots over one score: the first step's tiles overlap pairwise in all three axes and two of them share a
    start (both are added); the second step holds two out-of-range starts, (-5, 99, -1) and (99, -3, 99), which must land on
    the tiles at their clamped starts (0, Y-rows, 0) and (X-deps, 0, Z-cols) and nowhere else (everything outside the tiles is
    compared too), and ntiles = 5 makes its last slot invalid (it adds nothing).  The per-tile softmax
    is ops.softmax_accumulate onto a zero buffer -- the very expression -- and the reference adds it with numpy float32 `+=`
    in slot order."""
    ops, dev = U.pkg("ops"), _dev(hdu)
    shape, tile, batch = (11, 13, 9), (5, 7, 4), 3
    X, Y, Z = shape
    deps, rows, cols = tile
    n = deps * rows * cols
    table = [(1, 2, 1), (3, 5, 2), (1, 2, 1), (-5, 99, -1), (99, -3, 99), (0, 0, 0)]
    assert [_clamp(e, shape, tile) for e in table[3:5]] == [(0, 6, 0), (6, 0, 5)]
    starts, ntiles, cursor = _i32(table, dev), _i32([5], dev), _i32([0], dev)
    rng = np.random.default_rng(num)
    init = rng.uniform(0.0, 1.0, (Z, X, Y, num)).astype(np.float32)
    score = torch.from_numpy(init.copy()).to(dev)
    ref = init.copy()
    touched = np.zeros((Z, X, Y), bool)
    for step in range(2):
        la = _logits_act(dev, dtype, batch * n, seed=31 * step + num)
        for slot in range(batch):
            ops.tile_accumulate(la, shape, tile, num, starts, ntiles, cursor, batch, slot, score.reshape(-1))
            entry = step * batch + slot
            if entry >= 5:
                continue
            sm = torch.zeros(n * num, dtype=torch.float32, device=dev)
            ops.softmax_accumulate(la, slot * n, n, num, sm)
            x0, y0, z0 = _clamp(table[entry], shape, tile)
            ref[z0:z0 + cols, x0:x0 + deps, y0:y0 + rows] += sm.cpu().numpy().reshape(cols, deps, rows, num)
            touched[z0:z0 + cols, x0:x0 + deps, y0:y0 + rows] = True
        assert int(cursor.cpu()[0]) == step
        ops.sweep_advance(cursor, 2)
    got = score.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert not touched.all() and np.array_equal(got[~touched], init[~touched])
    assert not touched[0:4, 0:5, 0:7].all()                   # the invalid slot's tile (0, 0, 0) stayed as it was
    assert float(np.abs(got - init).max()) > 0


# ------------------------------------------------------------------ finalize
@pytest.mark.parametrize("num", [1, 3])
@pytest.mark.parametrize("shape", [(33, 5, 34), (7, 70, 3), (64, 64, 64)], ids=["33x5x34", "7x70x3", "64x64x64"])
def test_tile_finalize_equals_numpy(hdu, shape, num):
    ops, dev = U.pkg("ops"), _dev(hdu)
    X, Y, Z = shape
    rng = np.random.default_rng(X + num)
    score_h = rng.uniform(0.0, 4.0, (Z, X, Y, num)).astype(np.float32)
    cx, cy, cz = (rng.integers(1, 5, n).astype(np.float32) for n in shape)
    count = (cx[None, :, None] * cy[None, None, :] * cz[:, None, None])           # [Z][X][Y]
    score = torch.from_numpy(score_h).to(dev)
    dcx, dcy, dcz = (torch.from_numpy(c).to(dev) for c in (cx, cy, cz))
    for ch in range(num):
        want = np.ascontiguousarray((score_h[..., ch] / count.astype(np.int16)).transpose(1, 2, 0))
        assert want.dtype == np.float32
        hit = float(want[X // 2, Y // 2, Z // 2])             # a threshold that one voxel meets exactly
        for thres in (0.5, hit):
            want_mask = (want.astype(np.float64) >= thres).astype(np.uint8)
            assert 0 < want_mask.sum() < want_mask.size
            for do_score, do_mask in ((True, False), (False, True), (True, True)):
                o = torch.full((X * Y * Z,), -7.0, dtype=torch.float32, device=dev)
                m = torch.full((X * Y * Z,), 9, dtype=torch.uint8, device=dev)
                ops.tile_finalize(score, shape, num, ch, dcx, dcy, dcz, thres=thres, out_score=o if do_score else None,
                                  out_mask=m if do_mask else None)
                if do_score:
                    assert np.array_equal(o.cpu().numpy().view(np.uint32), want.reshape(-1).view(np.uint32))
                else:
                    assert (o.cpu().numpy() == -7.0).all()
                if do_mask:
                    assert np.array_equal(m.cpu().numpy(), want_mask.reshape(-1))
                else:
                    assert (m.cpu().numpy() == 9).all()


# ------------------------------------------------------------------ argument errors
def test_tile_argument_errors_leave_outputs_unchanged(hdu):
    ops, lib, dev = U.pkg("ops"), U.pkg("lib"), _dev(hdu)
    L = lib.get()
    (X, Y, Z), (deps, rows, cols), num, batch = (8, 9, 6), (4, 5, 3), 3, 2
    n = deps * rows * cols
    vol = torch.arange(X * Y * Z, dtype=torch.float32, device=dev)
    dst = torch.full((batch * n,), -1.0, dtype=torch.float32, device=dev)
    starts, cursor, ntiles = _i32([(0, 0, 0), (2, 3, 1)], dev), _i32([0], dev), _i32([2], dev)
    la = _logits_act(dev, "f32", batch * n, seed=5)
    score = torch.full((X * Y * Z * num,), 0.25, dtype=torch.float32, device=dev)
    cx, cy, cz = (torch.ones(k, dtype=torch.float32, device=dev) for k in (X, Y, Z))
    o = torch.full((X * Y * Z,), -7.0, dtype=torch.float32, device=dev)
    m = torch.full((X * Y * Z,), 9, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ops.stream()

    def gather(vol_p=p(vol), X_=X, Y_=Y, Z_=Z, deps_=deps, rows_=rows, cols_=cols, starts_p=p(starts), ntable=2, nt_p=p(ntiles),
               cursor_p=p(cursor), batch_=batch, pre=0, lo=0.0, hi=0.0, dst_p=p(dst)):
        return L.hdu_tile_gather_batched(vol_p, X_, Y_, Z_, deps_, rows_, cols_, starts_p, ntable, nt_p, cursor_p, batch_, pre, lo,
                                         hi, 0.0, dst_p, st)

    def accumulate(dtype=lib.HDU_F32, lg=la.ptr, ldl=la.ld, X_=X, Y_=Y, Z_=Z, deps_=deps, rows_=rows, cols_=cols, num_=num,
                   starts_p=p(starts), ntable=2, nt_p=p(ntiles), cursor_p=p(cursor), batch_=batch, slot=0, score_p=p(score)):
        return L.hdu_tile_accumulate(dtype, lg, ldl, X_, Y_, Z_, deps_, rows_, cols_, num_, starts_p, ntable, nt_p, cursor_p,
                                     batch_, slot, score_p, st)

    def finalize(score_p=p(score), X_=X, num_=num, ch=1, cx_p=p(cx), cy_p=p(cy), cz_p=p(cz), o_p=p(o), m_p=p(m)):
        return L.hdu_tile_finalize(score_p, X_, Y, Z, num_, ch, cx_p, cy_p, cz_p, 0.5, o_p, m_p, st)

    one_in = ctypes.c_void_p(vol.data_ptr() + 1)               # not 4-byte aligned
    bad = [
        (gather, dict(vol_p=None)), (gather, dict(starts_p=None)), (gather, dict(nt_p=None)), (gather, dict(cursor_p=None)),
        (gather, dict(dst_p=None)), (gather, dict(deps_=2)), (gather, dict(rows_=2)), (gather, dict(cols_=2)),
        (gather, dict(X_=deps - 1)), (gather, dict(Y_=rows - 1)), (gather, dict(Z_=cols - 1)), (gather, dict(ntable=0)),
        (gather, dict(batch_=0)), (gather, dict(batch_=ops.SWEEP_MAX_BATCH + 1)), (gather, dict(pre=1, lo=2.0, hi=1.0)),
        (gather, dict(vol_p=one_in)), (gather, dict(dst_p=ctypes.c_void_p(dst.data_ptr() + 2))),
        (accumulate, dict(lg=None)), (accumulate, dict(starts_p=None)), (accumulate, dict(nt_p=None)),
        (accumulate, dict(cursor_p=None)), (accumulate, dict(score_p=None)), (accumulate, dict(dtype=7)),
        (accumulate, dict(num_=0)), (accumulate, dict(num_=4)), (accumulate, dict(ldl=2)), (accumulate, dict(deps_=2)),
        (accumulate, dict(Z_=cols - 1)), (accumulate, dict(ntable=0)), (accumulate, dict(batch_=0)),
        (accumulate, dict(batch_=ops.SWEEP_MAX_BATCH + 1)), (accumulate, dict(slot=-1)), (accumulate, dict(slot=batch)),
        (accumulate, dict(score_p=ctypes.c_void_p(score.data_ptr() + 2))),
        (finalize, dict(score_p=None)), (finalize, dict(cx_p=None)), (finalize, dict(cy_p=None)), (finalize, dict(cz_p=None)),
        (finalize, dict(o_p=None, m_p=None)), (finalize, dict(X_=0)), (finalize, dict(num_=0)), (finalize, dict(num_=4)),
        (finalize, dict(ch=-1)), (finalize, dict(ch=num)), (finalize, dict(o_p=ctypes.c_void_p(o.data_ptr() + 2))),
    ]
    for fn, kw in bad:
        assert fn(**kw) == -1, kw                        # HDU_ERR_ARG
        label = {gather: "tile_gather_batched", accumulate: "tile_accumulate", finalize: "tile_finalize"}[fn]
        assert label in L.hdu_last_error().decode(), kw
    with pytest.raises(lib.HduError, match="tile_accumulate"):
        ops.tile_accumulate(la, (X, Y, Z), (deps, rows, cols), 0, starts, ntiles, cursor, batch, 0, score[:X * Y * Z])
    assert (dst.cpu().numpy() == -1.0).all()
    assert (score.cpu().numpy() == 0.25).all()
    assert (o.cpu().numpy() == -7.0).all() and (m.cpu().numpy() == 9).all()
    assert int(cursor.cpu()[0]) == 0
    # and the good calls still go through
    assert gather() == 0 and accumulate() == 0 and finalize() == 0
    v = vol.cpu().numpy().reshape(Z, X, Y)
    assert np.array_equal(dst.cpu().numpy()[n:], np.ascontiguousarray(v[1:1 + cols, 2:2 + deps, 3:3 + rows]).reshape(-1))
    assert float((score.cpu().numpy() != 0.25).sum()) == n * num
    assert (m.cpu().numpy() <= 1).all()
