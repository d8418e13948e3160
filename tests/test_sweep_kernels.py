"""The table-driven window kernels of the captured sliding-window sweep (include/hdu.h: hdu_sweep_gather / _accumulate /
_advance): the window start comes from a device table and a device cursor instead of a host integer.  Gather against numpy
slicing (bit-exact), accumulate against ops.softmax_accumulate called as funcs.sweep_scores calls it (bit-equal), advance
saturating, and every bad-argument case refused with the outputs untouched."""
import ctypes

import numpy as np
import pytest
import torch

import parity_utils as U


def _dev(hdu):
    return U.pkg("ops").device()


def _i32(vals, dev):
    return torch.tensor(list(vals), dtype=torch.int32, device=dev)


# ------------------------------------------------------------------ gather
@pytest.mark.parametrize("offset", [0, 1, 3], ids=["src16", "src4", "src12"])
@pytest.mark.parametrize("win_planes", [3, 8])
@pytest.mark.parametrize("hw", [(5, 7), (8, 8), (32, 32)], ids=["5x7", "8x8", "32x32"])
def test_sweep_gather_equals_numpy_slicing(hdu, hw, win_planes, offset):
    """plane 5 x 7 = 35 floats is no multiple of 4 (scalar head / tail, and windows that start off the 16-byte grid); `offset`
    floats in front of the volume leave the source 4-byte but not 16-byte aligned; a destination view one float into its buffer
    forces a scalar head.  Cursor at the first, a middle and the last table entry."""
    ops, dev = U.pkg("ops"), _dev(hdu)
    plane, z = hw[0] * hw[1], 14
    rng = np.random.default_rng(plane * 100 + win_planes * 10 + offset)
    host = rng.normal(0.0, 300.0, offset + z * plane).astype(np.float32)
    host[offset + 5] = np.float32("nan")               # a plain copy moves bits, whatever they encode
    buf = torch.from_numpy(host).to(dev)
    vol = buf[offset:]
    starts_h = [0, 1, 3, z - win_planes]
    starts = _i32(starts_h, dev)
    for dst_off in (0, 1):
        for w in (0, 2, 3):
            cursor = _i32([w], dev)
            out = torch.full((dst_off + win_planes * plane + 4,), -7.0, dtype=torch.float32, device=dev)
            ops.sweep_gather(vol, z, plane, win_planes, starts, cursor, out[dst_off:dst_off + win_planes * plane])
            got = out.cpu().numpy()
            c0 = starts_h[w]
            want = host[offset + c0 * plane: offset + (c0 + win_planes) * plane]
            assert np.array_equal(got[dst_off:dst_off + win_planes * plane].view(np.uint32), want.view(np.uint32))
            assert (got[:dst_off] == -7.0).all() and (got[dst_off + win_planes * plane:] == -7.0).all()
            assert int(cursor.cpu()[0]) == w


def test_sweep_gather_single_window_table(hdu):
    ops, dev = U.pkg("ops"), _dev(hdu)
    plane, z, wp = 35, 5, 5
    host = np.arange(z * plane, dtype=np.float32)
    out = torch.zeros(wp * plane, dtype=torch.float32, device=dev)
    ops.sweep_gather(torch.from_numpy(host).to(dev), z, plane, wp, _i32([0], dev), _i32([0], dev), out)
    assert np.array_equal(out.cpu().numpy(), host)


@pytest.mark.parametrize("hw", [(5, 7), (32, 32)], ids=["5x7", "32x32"])
def test_sweep_gather_preprocess(hdu, hw):
    """raw HU values -1000..1000 -> clip to [-200, 250] and subtract the mean 48 (preprocessing.py:15-16, test.py:55), float32"""
    ops, dev = U.pkg("ops"), _dev(hdu)
    plane, z, wp = hw[0] * hw[1], 9, 4
    rng = np.random.default_rng(plane)
    host = rng.uniform(-1000.0, 1000.0, 1 + z * plane).astype(np.float32)
    host[1:9] = [-1000.0, 1000.0, -200.0, 250.0, -200.5, 250.5, 48.0, 0.0]
    vol = torch.from_numpy(host).to(dev)[1:]
    starts = _i32([0, 2, 5], dev)
    for w, c0 in enumerate([0, 2, 5]):
        out = torch.zeros(wp * plane, dtype=torch.float32, device=dev)
        ops.sweep_gather(vol, z, plane, wp, starts, _i32([w], dev), out, preprocess=(-200, 250, 48))
        v = host[1 + c0 * plane: 1 + (c0 + wp) * plane]
        want = np.clip(v, -200, 250).astype(np.float32) - np.float32(48)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))


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
@pytest.mark.parametrize("case", [((0, 2, 4), 12), ((0, 2, 3), 11)], ids=["overlap", "clamped"])
def test_sweep_accumulate_equals_softmax_accumulate(hdu, case, dtype, num):
    """the reference is the eager sweep's own launch (funcs.sweep_scores): ops.softmax_accumulate(logits, plane,
    (win_planes - 2) * plane, num, score[c0 + 1 : c0 + win_planes - 1]) and score_num[c0 + 1 : c0 + win_planes - 1] += 1 on the
    host.  Windows overlap (starts 0, 2, 4 over z = 12) and, clamped, overlap twice (0, 2, 3 over z = 11)."""
    ops, dev = U.pkg("ops"), _dev(hdu)
    starts_h, z = case
    wp, plane = 8, 35
    starts = _i32(starts_h, dev)
    cursor = _i32([0], dev)
    score = torch.zeros(z * plane * num, dtype=torch.float32, device=dev)
    count = torch.zeros(z, dtype=torch.float32, device=dev)
    ref = torch.zeros((z, plane, num), dtype=torch.float32, device=dev)
    ref_num = np.zeros(z, np.float32)
    touched = np.zeros(z, bool)
    for w, c0 in enumerate(starts_h):
        la = _logits_act(dev, dtype, wp * plane, seed=17 * w + num)
        before = score.clone()
        ops.sweep_accumulate(la, plane, wp, z, num, starts, cursor, score, count)
        ops.sweep_advance(cursor, len(starts_h))
        ops.softmax_accumulate(la, plane, (wp - 2) * plane, num, ref[c0 + 1:c0 + wp - 1].reshape(-1))
        ref_num[c0 + 1:c0 + wp - 1] += 1
        touched[c0 + 1:c0 + wp - 1] = True
        # planes 0 and win_planes-1 of this window (and everything outside it) are not written
        same = (score == before).reshape(z, -1).all(dim=1).cpu().numpy()
        assert same[:c0 + 1].all() and same[c0 + wp - 1:].all()
    assert np.array_equal(score.cpu().numpy().view(np.uint32), ref.reshape(-1).cpu().numpy().view(np.uint32))
    assert np.array_equal(count.cpu().numpy(), ref_num)
    assert float(score.abs().max()) > 0
    assert (score.reshape(z, -1).cpu().numpy()[~touched] == 0).all()


# ------------------------------------------------------------------ advance
def test_sweep_advance_saturates(hdu):
    ops, dev = U.pkg("ops"), _dev(hdu)
    cursor = _i32([0], dev)
    seen = []
    for _ in range(5):
        ops.sweep_advance(cursor, 3)
        seen.append(int(cursor.cpu()[0]))
    assert seen == [1, 2, 2, 2, 2]
    one = _i32([0], dev)
    ops.sweep_advance(one, 1)
    assert int(one.cpu()[0]) == 0


# ------------------------------------------------------------------ argument errors
def test_sweep_argument_errors_leave_outputs_unchanged(hdu):
    ops, lib, dev = U.pkg("ops"), U.pkg("lib"), _dev(hdu)
    L = lib.get()
    plane, z, wp, num = 16, 6, 4, 3
    vol = torch.arange(z * plane, dtype=torch.float32, device=dev)
    dst = torch.full((wp * plane,), -1.0, dtype=torch.float32, device=dev)
    starts, cursor = _i32([0, 2], dev), _i32([1], dev)
    la = _logits_act(dev, "f32", wp * plane, seed=5)
    score = torch.full((z * plane * num,), 0.25, dtype=torch.float32, device=dev)
    count = torch.full((z,), 2.0, dtype=torch.float32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ops.stream()

    def gather(vol_p=p(vol), wp_=wp, starts_p=p(starts), nwin=2, cursor_p=p(cursor), dst_p=p(dst)):
        return L.hdu_sweep_gather(vol_p, z, plane, wp_, starts_p, nwin, cursor_p, 0, 0.0, 0.0, 0.0, dst_p, st)

    def accumulate(dtype=lib.HDU_F32, lg=la.ptr, wp_=wp, num_=num, starts_p=p(starts), nwin=2, cursor_p=p(cursor),
                   score_p=p(score), count_p=p(count)):
        return L.hdu_sweep_accumulate(dtype, lg, la.ld, plane, wp_, z, num_, starts_p, nwin, cursor_p, score_p, count_p, st)

    bad = [
        (gather, dict(vol_p=None)), (gather, dict(starts_p=None)), (gather, dict(cursor_p=None)), (gather, dict(dst_p=None)),
        (gather, dict(wp_=2)), (gather, dict(nwin=0)),
        (accumulate, dict(lg=None)), (accumulate, dict(starts_p=None)), (accumulate, dict(cursor_p=None)),
        (accumulate, dict(score_p=None)), (accumulate, dict(count_p=None)),
        (accumulate, dict(num_=0)), (accumulate, dict(num_=4)), (accumulate, dict(wp_=2)), (accumulate, dict(nwin=0)),
        (accumulate, dict(dtype=7)),
    ]
    for fn, kw in bad:
        assert fn(**kw) == -1, kw                        # HDU_ERR_ARG
        label = "sweep_gather" if fn is gather else "sweep_accumulate"
        assert label in L.hdu_last_error().decode(), kw
    assert L.hdu_sweep_advance(None, 2, st) == -1 and "sweep_advance" in L.hdu_last_error().decode()
    assert L.hdu_sweep_advance(p(cursor), 0, st) == -1 and "sweep_advance" in L.hdu_last_error().decode()
    with pytest.raises(lib.HduError, match="sweep_accumulate"):
        ops.sweep_accumulate(la, plane, wp, z, 0, starts, cursor, score[:z * plane], count)
    assert (dst.cpu().numpy() == -1.0).all()
    assert (score.cpu().numpy() == 0.25).all() and (count.cpu().numpy() == 2.0).all()
    assert int(cursor.cpu()[0]) == 1
    # and the good calls still go through
    assert gather() == 0 and accumulate() == 0
    assert np.array_equal(dst.cpu().numpy(), vol.cpu().numpy()[2 * plane:(2 + wp) * plane])
    assert np.array_equal(count.cpu().numpy(), np.array([2, 2, 2, 3, 3, 2], np.float32))
