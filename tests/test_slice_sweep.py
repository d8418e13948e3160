"""The device-resident 2-D slice sweep (h-denseunet_amd/sweep.py SliceSweepPlan, funcs.segment_volume_2d) against the host
composition it replaces (funcs.slice_labels_host: numpy batches, Model.predict, np.argmax), the coarse liver mask it yields, and
the CT cascade funcs.segment_ct / evaluate_ct against funcs.segment_volume / evaluate_volume fed with that mask from the host.
Every comparison is of uint8 labels, bit for bit.  The emulator tier runs the steps eagerly from the same device words; the
MI355X tier replays the captured graph."""
import numpy as np
import pytest

import parity_utils as U

_SHARED = {}


def _backend(hdu):
    return U.pkg("lib").backend()


def _model2d(hdu, dtype):
    """DenseUNet(b = 3, 32 x 32), built once per backend and dtype"""
    key = ("2d", _backend(hdu), dtype)
    if key not in _SHARED:
        _SHARED[key] = U.pkg("denseunet").DenseUNet(reduction=0.5, args=U.make_args(3, 32), dtype=dtype, nb_layers=(2, 2, 2, 2),
                                                    seed=1)
    return _SHARED[key]


def _hybrid(hdu):
    """the small hybrid of tests/test_sweep_plan.py (its own seeded initial weights, seed 4321)"""
    key = ("hybrid", _backend(hdu))
    if key not in _SHARED:
        args = U.make_args(1, 32, 8)
        m = U.pkg("hybridnet").dense_rnn_net(args, dtype="f32", nb_layers2d=(2, 2, 2, 2), nb_layers3d=(1, 1, 2, 1))
        _SHARED[key] = (m, args)
    return _SHARED[key]


def _host_labels(hdu, dtype, name, vol):
    """the host oracle of one volume, computed once per backend and shared; asserts that every class is well represented"""
    key = ("host", _backend(hdu), dtype, name)
    if key not in _SHARED:
        _SHARED[key] = U.pkg("funcs").slice_labels_host(_model2d(hdu, dtype), vol)
    want = _SHARED[key]
    counts = np.bincount(want.reshape(-1), minlength=3)
    assert want.dtype == np.uint8 and counts.size == 3 and (counts >= 1000).all(), counts
    return want


def _vol7():
    return U.pkg("synth").synthetic_ct((32, 32, 7), seed=3)[0]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_segment_volume_2d_equals_host_composition(hdu, dtype):
    """32 x 32 x 7 volume, b = 3: three steps, the last with one valid slot.  Host oracle on the emulator: 1798 / 3761 / 1609
    voxels of classes 0 / 1 / 2 in float32, 1802 / 3760 / 1606 in bfloat16.  mode="eager" equals the oracle, mode="graph" equals
    eager with three replays, and a second volume of the same shape goes through the same plan without another capture."""
    f, lib = U.pkg("funcs"), U.pkg("lib")
    m = _model2d(hdu, dtype)
    vol = _vol7()
    want = _host_labels(hdu, dtype, "vol7", vol)
    eager = f.segment_volume_2d(m, vol, mode="eager")
    assert eager.dtype == np.uint8 and eager.shape == (32, 32, 7) and np.array_equal(eager, want)
    plan = m._slice_sweep_plan
    assert plan.replays == 3 and plan.captures == 0
    graph = f.segment_volume_2d(m, vol, mode="graph")
    assert np.array_equal(graph, eager)
    assert m._slice_sweep_plan is plan and plan.replays == 3
    captures = plan.captures
    assert captures == (0 if lib.is_emulator() else 1)            # (no graphs on the emulator: the step ran eagerly)
    vol_b = U.pkg("synth").synthetic_ct((32, 32, 7), seed=11)[0]
    graph_b = f.segment_volume_2d(m, vol_b, mode="graph")
    assert m._slice_sweep_plan is plan and plan.captures == captures and plan.replays == 3
    assert np.array_equal(graph_b, f.segment_volume_2d(m, vol_b, mode="eager")) and not np.array_equal(graph_b, graph)
    assert m.ctx.learning_phase == 1 and m.ctx._prefolded_phase is None
    dev = f.slice_sweep_labels(m, vol, mode="graph")
    assert dev is plan.labels and dev.dtype.is_floating_point is False and dev.numel() == 32 * 32 * 7
    assert np.array_equal(dev.cpu().numpy().reshape(32, 32, 7), want)


def test_slice_sweep_crops_to_the_window_and_preprocesses(hdu):
    """a 36 x 34 x 7 volume on the 32-window model: the labels of the top-left 32 x 32 crop, zeros outside; a raw-HU volume with
    preprocess=(-200, 250, 48) equals the volume preprocessed on the host without it, in both modes"""
    f = U.pkg("funcs")
    m = _model2d(hdu, "f32")
    vol = _vol7()
    want = _host_labels(hdu, "f32", "vol7", vol)
    big = np.random.default_rng(9).normal(0.0, 50.0, (36, 34, 7)).astype(np.float32)
    big[:32, :32, :] = vol
    for mode in ("eager", "graph"):
        got = f.segment_volume_2d(m, big, mode=mode)
        assert got.shape == (36, 34, 7) and np.array_equal(got[:32, :32, :], want)
        assert (got[32:] == 0).all() and (got[:, 32:] == 0).all()
    assert np.array_equal(f.slice_labels_host(m, big), got)
    # raw HU: the synthetic volume (already clipped and centred) with its mean put back and its range doubled, so that the clip
    # at -200 and the clip at 250 both bite
    raw = ((vol + np.float32(48)) * np.float32(2)).astype(np.float32)
    assert (raw < -200).any() and (raw > 250).any()
    pre = (-200, 250, 48)
    host = np.clip(raw, -200, 250).astype(np.float32) - np.float32(48)
    ref = f.segment_volume_2d(m, host, mode="eager")
    assert len(np.unique(ref)) >= 2
    for mode in ("eager", "graph"):
        assert np.array_equal(f.segment_volume_2d(m, raw, mode=mode, preprocess=pre), ref)
    assert m._slice_sweep_plan.preprocess == (-200.0, 250.0, 48.0)
    assert np.array_equal(f.slice_labels_host(m, raw, preprocess=pre), ref)


def test_coarse_liver_mask_and_its_window(hdu):
    """coarse_liver_mask_device(largest=True) = the largest 26-connected component of host labels != 0; without `largest` the
    plain labels != 0; liver_window_from_device_mask on it = liver_window_from_mask on the host mask (mask, mini, maxi)"""
    f = U.pkg("funcs")
    m = _model2d(hdu, "f32")
    vol = _vol7()
    want = _host_labels(hdu, "f32", "vol7", vol)
    host_mask = f._largest_component(want != 0).astype(np.uint8)
    for mode in ("eager", "graph"):
        mask_dev = f.coarse_liver_mask_device(m, vol, mode=mode)
        assert mask_dev is not m._slice_sweep_plan.labels
        assert np.array_equal(mask_dev.cpu().numpy().reshape(32, 32, 7), host_mask)
    plain = f.coarse_liver_mask_device(m, vol, largest=False)
    assert np.array_equal(plain.cpu().numpy().reshape(32, 32, 7), (want != 0).astype(np.uint8))
    dil_dev, mini, maxi = f.liver_window_from_device_mask(mask_dev, (32, 32, 7))
    dil, hmini, hmaxi = f.liver_window_from_mask(host_mask)
    assert np.array_equal(dil_dev.cpu().numpy().reshape(32, 32, 7), dil)
    assert np.array_equal(mini, hmini) and np.array_equal(maxi, hmaxi)
    # liver_window_from_mask_device goes through the same function: results unchanged
    d2, mini2, maxi2 = f.liver_window_from_mask_device(host_mask)
    assert np.array_equal(d2.cpu().numpy(), dil_dev.cpu().numpy()) and np.array_equal(mini2, mini) and np.array_equal(maxi2, maxi)
    with pytest.raises(ValueError, match="empty liver mask"):
        f.liver_window_from_device_mask(mask_dev * 0, (32, 32, 7))


def test_segment_ct_equals_segment_volume_with_the_host_mask(hdu):
    """32 x 32 x 14 volume: the 2-D net (b = 3, five steps) gives 3515 / 7558 / 3263 voxels of classes 0 / 1 / 2 on the
    emulator, its largest component holds 10792 voxels and spans the whole volume, so the hybrid (seed 4321, the model of
    tests/test_sweep_plan.py; no other seed was needed) sweeps the windows 0, 2, 4, 6.  With the thresholds of that file's
    segment_volume test the host composition yields 2911 / 5339 / 6086 voxels of background / liver / tumour.  segment_ct
    equals segment_volume fed with the host's coarse mask byte for byte in both modes, and evaluate_ct returns evaluate_volume's
    dictionary."""
    f = U.pkg("funcs")
    m2 = _model2d(hdu, "f32")
    hy, args = _hybrid(hdu)
    vol, truth = U.pkg("synth").synthetic_ct((32, 32, 14), seed=3)
    host = _host_labels(hdu, "f32", "vol14", vol)
    coarse = f._largest_component(host != 0).astype(np.uint8)
    _, mini, maxi = f.liver_window_from_mask(coarse)
    s1, s2 = f.predict_tumor_inwindow(hy, vol, 3, mini, maxi, args, mode="graph")
    tl, tt = float(np.quantile(s1[s1 > 0], 0.4)), float(np.quantile(s2[s2 > 0], 0.5))
    ref = f.segment_volume(hy, vol, coarse, args, tl, tt)
    assert ref.dtype == np.uint8 and (np.bincount(ref.reshape(-1), minlength=3) >= 1000).all()
    for mode in ("eager", "graph"):
        got = f.segment_ct(m2, hy, vol, args, tl, tt, mode=mode)
        assert got.dtype == np.uint8 and got.shape == (32, 32, 14) and np.array_equal(got, ref), mode
    spacing = (0.8, 0.8, 2.5)
    want_labels, want_eval = f.evaluate_volume(hy, vol, coarse, truth, args, spacing, tl, tt, mode="graph")
    got_labels, got_eval = f.evaluate_ct(m2, hy, vol, truth, args, spacing, tl, tt, mode="graph")
    assert np.array_equal(want_labels, ref) and np.array_equal(got_labels, ref)
    assert got_eval == want_eval and set(got_eval) == {"liver", "tumor"}


def test_slice_sweep_refusals(hdu):
    f, sweep = U.pkg("funcs"), U.pkg("sweep")
    m2 = _model2d(hdu, "f32")
    hy, args = _hybrid(hdu)
    vol = _vol7()
    vol14, truth = U.pkg("synth").synthetic_ct((32, 32, 14), seed=3)
    for call in (lambda: f.segment_volume_2d(hy, vol14), lambda: f.slice_sweep_labels(hy, vol14),
                 lambda: f.coarse_liver_mask_device(hy, vol14), lambda: f.segment_ct(hy, hy, vol14, args),
                 lambda: sweep.SliceSweepPlan(hy, (32, 32, 14)), lambda: f.slice_labels_host(hy, vol14)):
        with pytest.raises(ValueError, match="2-D net"):
            call()                                               # a hybrid passed as the 2-D model
    wb = U.pkg("hybridnet").dense_rnn_net(args, dtype="f32", nb_layers2d=(2, 2, 2, 2), nb_layers3d=(1, 1, 2, 1), window_batch=2)
    with pytest.raises(ValueError, match="2-D net"):
        f.segment_volume_2d(wb, vol14)                           # a window_batch model
    with pytest.raises(ValueError, match="2-D net"):
        sweep.slice_plan_for(wb, (32, 32, 14))
    for shape in ((31, 32, 7), (32, 31, 7)):
        with pytest.raises(ValueError, match="smaller than the network window"):
            f.segment_volume_2d(m2, np.zeros(shape, np.float32))
        with pytest.raises(ValueError, match="smaller than the network window"):
            sweep.SliceSweepPlan(m2, shape)
    with pytest.raises(ValueError, match="mode"):
        f.segment_volume_2d(m2, vol, mode="fast")
    with pytest.raises(ValueError, match="preprocess"):
        f.segment_volume_2d(m2, vol, preprocess=(250, -200, 48))
    with pytest.raises(ValueError, match="truth"):
        f.evaluate_ct(m2, hy, vol14, truth[:, :, :13], args)     # a truth of the wrong shape
