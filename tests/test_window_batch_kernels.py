"""The window-batched kernels (include/hdu.h: hdu_slab25d_batched, hdu_sweep_gather_batched, hdu_sweep_accumulate_batched)
against the single-window entry points they generalise, bit for bit: no tolerance anywhere.  Shapes are ragged on purpose:
plane = 5 x 7 = 35 floats is no multiple of 4, so the base of a window slot is 4-byte aligned only; win_planes = 5, z = 11.
Every test runs on the emulator and, marked gpu, on MI355X."""
import ctypes

import numpy as np
import pytest
import torch

import parity_utils as U

PLANE, WP, Z = 35, 5, 11
GUARD = 64          # guard band, in elements, on both sides of every buffer a kernel writes


def _dev(hdu):
    return U.pkg("ops").device()


def _i32(vals, dev):
    return torch.tensor(list(vals), dtype=torch.int32, device=dev)


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy(), np.float32).view(np.uint32)


def _hd(dtype):
    lib = U.pkg("lib")
    return lib.HDU_BF16 if dtype == "bf16" else lib.HDU_F32


def _logits_act(dev, dtype, M, seed):
    """logits [M][ld] as the network leaves them: 3 classes in a padded row (ld 7 for float32, 8 for bfloat16)"""
    ops = U.pkg("ops")
    ld = 8 if dtype == "bf16" else 7
    raw = torch.from_numpy(np.random.default_rng(seed).normal(0.0, 3.0, M * ld).astype(np.float32))
    buf = raw.to(torch.bfloat16 if dtype == "bf16" else torch.float32).to(dev)
    return ops.Act(buf, 0, 1, 1, 1, M, 3, ld, _hd(dtype))


def _window_act(la, i):
    """the rows of window slot i of a batched logits tensor, as a single-window tensor"""
    ops = U.pkg("ops")
    return ops.Act(la.buf, la.off + i * WP * PLANE * la.ld, 1, 1, 1, WP * PLANE, 3, la.ld, la.dtype)


# ------------------------------------------------------------------ slab layer
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_slab25d_batched_equals_per_volume_slab25d(hdu, dtype):
    """B = 3 volumes of D = 4 planes: three hdu_slab25d calls on the three volumes (so an edge slab replicates the plane of its
    own volume, never the neighbour's); B = 1 is hdu_slab25d itself"""
    ops, dev = U.pkg("ops"), _dev(hdu)
    B, D, H, W, C = 3, 4, 5, 7, 8
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    vol = torch.from_numpy(np.random.default_rng(1).normal(0.0, 100.0, B * D * H * W).astype(np.float32)).to(dev)

    def act(buf, n):
        return ops.Act(buf, 0, n, 1, H, W, C, C, _hd(dtype))

    got = torch.full((B * D * H * W * C,), 9.0, dtype=tdt, device=dev)
    ops.slab25d_batched(vol, B, D, H, W, act(got, B * D))
    want = torch.full((B * D * H * W * C,), 9.0, dtype=tdt, device=dev)
    n = D * H * W
    for b in range(B):
        ops.slab25d(vol[b * n:(b + 1) * n], D, H, W, act(want[b * n * C:(b + 1) * n * C], D))
    assert torch.equal(got.view(torch.int16 if dtype == "bf16" else torch.int32),
                       want.view(torch.int16 if dtype == "bf16" else torch.int32))
    g = got.float().cpu().numpy().reshape(B, D, H * W, C)
    v = vol.to(tdt).float().cpu().numpy().reshape(B, D, H * W)
    assert np.array_equal(g[1, 0, :, 0], v[1, 0]) and np.array_equal(g[1, D - 1, :, 2], v[1, D - 1])   # edges of volume 1
    assert (g[..., 3:] == 0).all()
    one = torch.full((n * C,), 9.0, dtype=tdt, device=dev)
    ops.slab25d_batched(vol[:n], 1, D, H, W, act(one, D))
    assert torch.equal(one.float(), want[:n * C].float())


# ------------------------------------------------------------------ gather
@pytest.mark.parametrize("pre", [None, (-200, 250, 48)], ids=["copy", "preprocess"])
def test_sweep_gather_batched_equals_gather_per_slot(hdu, pre):
    """slot i of step s = hdu_sweep_gather driven through the same table with cursor s * batch + i (the last step's padding
    slots included: they gather the clamped table entry); the volume starts one float into its buffer (4-byte aligned source)"""
    ops, dev = U.pkg("ops"), _dev(hdu)
    batch, n = 3, WP * PLANE
    host = np.random.default_rng(2).uniform(-1000.0, 1000.0, 1 + Z * PLANE).astype(np.float32)
    vol = torch.from_numpy(host).to(dev)[1:]
    table = [2, 4, 6, 6, 0, 1]
    starts, nwin = _i32(table, dev), _i32([4], dev)
    for s in (0, 1):
        out = torch.full((GUARD + batch * n + GUARD,), -7.0, dtype=torch.float32, device=dev)
        ops.sweep_gather_batched(vol, Z, PLANE, WP, starts, nwin, _i32([s], dev), batch, out[GUARD:GUARD + batch * n], pre)
        for i in range(batch):
            want = torch.zeros(n, dtype=torch.float32, device=dev)
            ops.sweep_gather(vol, Z, PLANE, WP, starts, _i32([s * batch + i], dev), want, pre)
            assert np.array_equal(_bits(out[GUARD + i * n:GUARD + (i + 1) * n]), _bits(want)), (s, i)
            c0 = table[s * batch + i]
            ref = host[1 + c0 * PLANE:1 + (c0 + WP) * PLANE]
            if pre is not None:
                ref = np.clip(ref, pre[0], pre[1]).astype(np.float32) - np.float32(pre[2])
            assert np.array_equal(_bits(want), ref.view(np.uint32))
        o = out.cpu().numpy()
        assert (o[:GUARD] == -7.0).all() and (o[GUARD + batch * n:] == -7.0).all()


# ------------------------------------------------------------------ accumulate
def _accumulate_case(hdu, dtype, num, table, nwin_h, steps):
    ops, dev = U.pkg("ops"), _dev(hdu)
    batch = 3
    starts, nwin = _i32(table, dev), _i32([nwin_h], dev)
    sentinel = 0.375
    score = torch.full((Z * PLANE * num,), sentinel, dtype=torch.float32, device=dev)
    count = torch.full((Z,), 2.0, dtype=torch.float32, device=dev)
    ref = score.clone()
    ref_count = count.clone()
    touched = np.zeros(Z, bool)
    cursor = _i32([0], dev)
    for s in range(steps):
        la = _logits_act(dev, dtype, batch * WP * PLANE, seed=31 * s + num)
        ops.sweep_accumulate_batched(la, PLANE, WP, Z, num, starts, nwin, cursor, batch, score, count)
        ops.sweep_advance(cursor, len(table) // batch)
        for i in range(batch):
            w = s * batch + i
            if w < nwin_h:                                  # the valid windows, in order, one hdu_sweep_accumulate each
                ops.sweep_accumulate(_window_act(la, i), PLANE, WP, Z, num, starts, _i32([w], dev), ref, ref_count)
                touched[table[w] + 1:table[w] + WP - 1] = True
    assert np.array_equal(_bits(score), _bits(ref))
    assert np.array_equal(_bits(count), _bits(ref_count))
    sc = score.cpu().numpy().reshape(Z, -1)
    assert (sc[~touched] == np.float32(sentinel)).all() and (count.cpu().numpy()[~touched] == 2.0).all()
    assert (sc[touched] != np.float32(sentinel)).any(axis=1).all()
    return count.cpu().numpy() - 2.0


@pytest.mark.parametrize("num", [1, 3])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_sweep_accumulate_batched_two_steps_with_padding_and_duplicate(hdu, dtype, num):
    """table [2, 4, 6, 6], 4 windows, batch 3: step 1 has one valid slot (the second start 6) and two padded ones that add
    nothing (the table is padded to 6 entries with the last start); the duplicate start 6 is added twice overall"""
    cov = _accumulate_case(hdu, dtype, num, [2, 4, 6, 6, 6, 6], 4, 2)
    want = np.zeros(Z, np.float32)
    for c0 in (2, 4, 6, 6):
        want[c0 + 1:c0 + WP - 1] += 1
    assert np.array_equal(cov, want) and cov[9] == 2 and cov[7] == 3      # plane 9: start 6 alone, twice


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_sweep_accumulate_batched_single_partly_filled_step(hdu, dtype):
    """2 windows with batch 3: one step, its third slot is padding"""
    cov = _accumulate_case(hdu, dtype, 3, [1, 5, 5], 2, 1)
    want = np.zeros(Z, np.float32)
    want[2:5] += 1
    want[6:9] += 1
    assert np.array_equal(cov, want)


# ------------------------------------------------------------------ corrupt tables: clamped addressing
@pytest.mark.parametrize("table,cursor_h,nwin_h", [([-3, 40, 2], 0, 3), ([2, 4, 6], 7, 3), ([2, 4, 6], -2, 3), ([0, 3, 6], 0, 99),
                                                   ([0, 3, 6], 0, -1)],
                         ids=["starts-out-of-range", "cursor-beyond-table", "cursor-negative", "nwin-beyond-table", "nwin-negative"])
def test_corrupt_table_stays_inside_the_buffers(hdu, table, cursor_h, nwin_h):
    """a bounds check on the clamped addressing: whatever the table, the cursor and the window count hold, the kernels read
    inside the volume / the logits and write inside dst / score / count.  Guard bands around the three outputs stay intact
    and a NaN band around the volume never reaches dst."""
    ops, dev = U.pkg("ops"), _dev(hdu)
    batch, num, n = 3, 3, WP * PLANE
    hostv = np.full(GUARD + Z * PLANE + GUARD, np.nan, np.float32)
    hostv[GUARD:GUARD + Z * PLANE] = np.random.default_rng(4).normal(0.0, 1.0, Z * PLANE)
    vol = torch.from_numpy(hostv).to(dev)[GUARD:GUARD + Z * PLANE]
    starts, cursor, nwin = _i32(table, dev), _i32([cursor_h], dev), _i32([nwin_h], dev)
    dst = torch.full((GUARD + batch * n + GUARD,), -7.0, dtype=torch.float32, device=dev)
    ops.sweep_gather_batched(vol, Z, PLANE, WP, starts, nwin, cursor, batch, dst[GUARD:GUARD + batch * n])
    d = dst.cpu().numpy()
    assert (d[:GUARD] == -7.0).all() and (d[-GUARD:] == -7.0).all() and np.isfinite(d).all()
    score = torch.full((GUARD + Z * PLANE * num + GUARD,), 0.5, dtype=torch.float32, device=dev)
    count = torch.full((GUARD + Z + GUARD,), 3.0, dtype=torch.float32, device=dev)
    la = _logits_act(dev, "f32", batch * n, seed=9)
    ops.sweep_accumulate_batched(la, PLANE, WP, Z, num, starts, nwin, cursor, batch, score[GUARD:GUARD + Z * PLANE * num],
                                 count[GUARD:GUARD + Z])
    s, c = score.cpu().numpy(), count.cpu().numpy()
    assert (s[:GUARD] == 0.5).all() and (s[-GUARD:] == 0.5).all() and np.isfinite(s).all()
    assert (c[:GUARD] == 3.0).all() and (c[-GUARD:] == 3.0).all()
    inner = s[GUARD:-GUARD].reshape(Z, -1)
    assert (inner[0] == 0.5).all() and (inner[Z - 1] == 0.5).all()        # no window ever adds its own first / last plane
    if nwin_h < 0:
        assert (inner == 0.5).all() and (c == 3.0).all()
    assert int(cursor.cpu()[0]) == cursor_h


# ------------------------------------------------------------------ argument errors
def test_batched_argument_errors_launch_nothing(hdu):
    ops, lib, dev = U.pkg("ops"), U.pkg("lib"), _dev(hdu)
    L = lib.get()
    batch, num, n = 3, 3, WP * PLANE
    vol = torch.arange(Z * PLANE, dtype=torch.float32, device=dev)
    dst = torch.full((batch * n,), -1.0, dtype=torch.float32, device=dev)
    starts, cursor, nwin = _i32([0, 2, 4], dev), _i32([0], dev), _i32([3], dev)
    la = _logits_act(dev, "f32", batch * n, seed=5)
    score = torch.full((Z * PLANE * num,), 0.25, dtype=torch.float32, device=dev)
    count = torch.full((Z,), 2.0, dtype=torch.float32, device=dev)
    slab = torch.full((4 * PLANE * 8,), 5.0, dtype=torch.float32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ops.stream()

    def gather(vol_p=p(vol), starts_p=p(starts), nwin_p=p(nwin), cursor_p=p(cursor), dst_p=p(dst), batch_=batch, wp_=WP, nt=3):
        return L.hdu_sweep_gather_batched(vol_p, Z, PLANE, wp_, starts_p, nt, nwin_p, cursor_p, batch_, 0, 0.0, 0.0, 0.0, dst_p, st)

    def accumulate(dtype=lib.HDU_F32, lg=la.ptr, starts_p=p(starts), nwin_p=p(nwin), cursor_p=p(cursor), score_p=p(score),
                   count_p=p(count), batch_=batch, num_=num, wp_=WP, nt=3):
        return L.hdu_sweep_accumulate_batched(dtype, lg, la.ld, PLANE, wp_, Z, num_, starts_p, nt, nwin_p, cursor_p, batch_,
                                              score_p, count_p, st)

    def slab25d(vol_p=p(vol), out_p=p(slab), B=1, dtype=lib.HDU_F32):
        return L.hdu_slab25d_batched(dtype, vol_p, B, 4, 5, 7, out_p, 8, st)

    bad = [
        (gather, dict(batch_=0)), (gather, dict(batch_=9)), (gather, dict(vol_p=None)), (gather, dict(starts_p=None)),
        (gather, dict(nwin_p=None)), (gather, dict(cursor_p=None)), (gather, dict(dst_p=None)), (gather, dict(wp_=2)),
        (gather, dict(nt=0)),
        (accumulate, dict(batch_=0)), (accumulate, dict(batch_=9)), (accumulate, dict(lg=None)), (accumulate, dict(starts_p=None)),
        (accumulate, dict(nwin_p=None)), (accumulate, dict(cursor_p=None)), (accumulate, dict(score_p=None)),
        (accumulate, dict(count_p=None)), (accumulate, dict(num_=4)), (accumulate, dict(num_=0)), (accumulate, dict(wp_=2)),
        (accumulate, dict(nt=0)), (accumulate, dict(dtype=7)),
        (slab25d, dict(B=0)), (slab25d, dict(vol_p=None)), (slab25d, dict(out_p=None)), (slab25d, dict(dtype=7)),
    ]
    label = {gather: "sweep_gather_batched", accumulate: "sweep_accumulate_batched", slab25d: "slab25d_batched"}
    for fn, kw in bad:
        assert fn(**kw) == -1, kw                        # HDU_ERR_ARG
        assert label[fn] in L.hdu_last_error().decode(), kw
    assert (dst.cpu().numpy() == -1.0).all() and (slab.cpu().numpy() == 5.0).all()
    assert (score.cpu().numpy() == 0.25).all() and (count.cpu().numpy() == 2.0).all()
    # and the good calls still go through
    assert gather() == 0 and accumulate() == 0 and slab25d() == 0
    assert np.array_equal(dst.cpu().numpy()[n:2 * n], vol.cpu().numpy()[2 * PLANE:(2 + WP) * PLANE])
    assert np.array_equal(count.cpu().numpy(), 2.0 + np.array([0, 1, 1, 2, 1, 2, 1, 1, 0, 0, 0], np.float32))
    assert (slab.cpu().numpy().reshape(-1, 8)[:, 3:] == 0.0).all()
