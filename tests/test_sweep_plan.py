"""The captured sliding-window sweep (h-denseunet_amd/sweep.py, funcs.sweep_scores(mode="graph")) and the captured predict
(Model.capture_predict / predict_resident) against the eager paths they leave in place.  The emulator tier runs the same
four-part window step (gather, phase-0 forward, accumulate, advance) eagerly from the same device tables; the MI355X tier
replays the captured graph."""
import numpy as np
import pytest
import torch

import parity_utils as U


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _small_hybrid():
    args = U.make_args(1, 32, 8)
    model = U.pkg("hybridnet").dense_rnn_net(args, dtype="f32", nb_layers2d=(2, 2, 2, 2), nb_layers3d=(1, 1, 2, 1))
    return model, args


# ------------------------------------------------------------------ emulator tier
# A forward of the small hybrid takes seconds on the emulator: the liver windows below are chosen so that a sweep has two or
# three windows (still overlapping, and clamped at the end of the volume in one case), and the model is built once.
_SHARED = {}


def _shared_hybrid():
    if "m" not in _SHARED:
        _SHARED["m"] = _small_hybrid()
    return _SHARED["m"]


LOW = ((0, 0, 0), (31, 31, 0))         # window starts 0, 2 over z = 14
HIGH = ((0, 0, 10), (31, 31, 13))      # window starts 5, 6: the last one clamped to z - 8, both overlap on 5 planes


def test_graph_sweep_equals_eager_and_plan_is_reused(emu_lib):
    """32 x 32 x 14 volume, 8-plane windows: score and count of mode="graph" bit-equal to mode="eager"; a second volume of the
    same depth and another liver window through the SAME plan is bit-equal again, so cursor, score and count are reset per
    sweep; another depth builds a new plan"""
    f, sweep = U.pkg("funcs"), U.pkg("sweep")
    model, args = _shared_hybrid()
    assert sweep.window_starts(14, 8, *HIGH) == [5, 6] and sweep.window_starts(14, 8, *LOW) == [0, 2]
    vol_a, _ = U.pkg("synth").synthetic_ct((32, 32, 14), seed=3)
    vol_b, _ = U.pkg("synth").synthetic_ct((32, 32, 14), seed=11)
    plans = []
    for vol, (mini, maxi) in ((vol_a, HIGH), (vol_b, LOW)):
        es, en = f.sweep_scores(model, vol, 3, mini, maxi, args)
        gs, gn = f.sweep_scores(model, vol, 3, mini, maxi, args, mode="graph")
        assert isinstance(en, np.ndarray) and torch.is_tensor(gn)
        assert np.array_equal(_bits(gs), _bits(es))
        assert np.array_equal(gn.cpu().numpy(), en)
        assert float(es.abs().max()) > 0 and en.max() == (2 if maxi is HIGH[1] else 1) + (maxi is LOW[1])
        plan = model._sweep_plan
        assert plan.replays == 2 and plan.captures == 0           # (no graphs on the emulator: the step ran eagerly)
        assert model.ctx.learning_phase == 1 and model.ctx._prefolded_phase is None
        plans.append(plan)
    assert plans[0] is plans[1]
    # predict_tumor_inwindow(mode="graph"): the averaged scores of the eager accumulators above
    mini, maxi = LOW
    want = es.cpu().numpy() / (en.reshape(14, 1, 1, 1) + np.float32(1e-4))
    g1, g2 = f.predict_tumor_inwindow(model, vol_b, 3, mini, maxi, args, mode="graph")
    assert np.array_equal(_bits(g1), _bits(want[..., 1].transpose(1, 2, 0)))
    assert np.array_equal(_bits(g2), _bits(want[..., 2].transpose(1, 2, 0)))
    other = sweep.plan_for(model, 12, 3)
    assert other is not plans[0] and other.z == 12 and model._sweep_plan is other
    with pytest.raises(ValueError, match="mode"):
        f.sweep_scores(model, vol_b, 3, mini, maxi, args, mode="fast")


def test_graph_sweep_preprocess_equals_eager_on_preprocessed_volume(emu_lib):
    """a raw-HU volume with preprocess=(lo, hi, mean) against the eager sweep of the volume preprocessed on the host
    (preprocessing.py:15-16 clip, test.py:55 mean), in both modes of the keyword"""
    f = U.pkg("funcs")
    model, args = _shared_hybrid()
    rng = np.random.default_rng(5)
    raw = rng.uniform(-1000.0, 1000.0, (32, 32, 14)).astype(np.float32)
    pre = (-200, 250, 48)
    host = np.clip(raw, -200, 250).astype(np.float32) - np.float32(48)
    mini, maxi = HIGH
    es, en = f.sweep_scores(model, host, 3, mini, maxi, args)
    gs, gn = f.sweep_scores(model, raw, 3, mini, maxi, args, mode="graph", preprocess=pre)
    assert model._sweep_plan.preprocess == (-200.0, 250.0, 48.0)
    assert np.array_equal(_bits(gs), _bits(es)) and np.array_equal(gn.cpu().numpy(), en)
    e2, _ = f.sweep_scores(model, raw, 3, mini, maxi, args, preprocess=pre)
    assert np.array_equal(_bits(e2), _bits(es))
    assert float(es.abs().max()) > 0


def test_segment_volume_graph_equals_eager(emu_lib):
    """segment_volume(mode="graph") (device count handed straight to the post-processing) equals segment_volume(), uint8, no
    tolerance; a coarse mask confined to the first planes keeps the sweep at three windows"""
    f = U.pkg("funcs")
    model, args = _shared_hybrid()
    vol, lab = U.pkg("synth").synthetic_ct((32, 32, 14), seed=3)
    mask = np.zeros(lab.shape, np.int16)
    mask[8:24, 8:24, 0] = 1
    _, mini, maxi = f.liver_window_from_mask(mask)
    assert U.pkg("sweep").window_starts(14, 8, mini, maxi) == [0, 2, 4]
    s1, s2 = f.predict_tumor_inwindow(model, vol, 3, mini, maxi, args, mode="graph")
    tl, tt = float(np.quantile(s1[s1 > 0], 0.4)), float(np.quantile(s2[s2 > 0], 0.5))
    ref = f.segment_volume(model, vol, mask, args, tl, tt)
    got = f.segment_volume(model, vol, mask, args, tl, tt, mode="graph")
    assert got.dtype == np.uint8 and got.shape == (32, 32, 14) and np.array_equal(got, ref)
    assert (got == 1).any()


@pytest.mark.parametrize("kind", ["2d", "hybrid", "3d"])
def test_capture_predict_keeps_predict(emu_lib, kind):
    """predict() after capture_predict() equals predict() before it, before and after one training step (the weight
    preparation and the BN fold are redone on every call, so new weights and moving statistics are picked up)"""
    ka = U.pkg("keras_api")
    b, size, cols = (2, 32, None) if kind == "2d" else (1, 32, 8)
    if kind == "2d":
        m = U.pkg("denseunet").DenseUNet(reduction=0.5, args=U.make_args(b, size), dtype="f32", nb_layers=(2, 2, 2, 2))
    elif kind == "3d":
        m = U.pkg("densenet3d_sharded").dense_net3d(U.make_args(b, size, cols), dtype="f32", nb_layers3d=(1, 1, 2, 1))
    else:
        m = _small_hybrid()[0]
    m.ctx.dropout_enabled = False
    loss = U.pkg("loss")
    m.compile(optimizer=ka.SGD(lr=1e-3, momentum=0.9, nesterov=True),
              loss=[loss.weighted_crossentropy_2ddense if kind == "2d" else loss.weighted_crossentropy])
    x, y = U.synthetic_batch(kind, b, size, cols)
    before = m.predict(x).copy()             # (on the emulator the returned array aliases the model's staging buffer)
    m.capture_predict()
    assert m._predict_captured
    assert np.array_equal(_bits(m.predict(x)), _bits(before))
    m.train_on_batch(x, y)
    m.predict_resident()                     # the input of the training step is still resident
    after = m._download_logits().cpu().numpy().copy()
    assert not np.array_equal(_bits(after), _bits(before))
    m._predict_captured = False              # the eager path on the trained weights
    assert np.array_equal(_bits(m.predict(x)), _bits(after))
    assert m.ctx.learning_phase == 1 and m.ctx._prefolded_phase is None


# ------------------------------------------------------------------ MI355X tier
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_captured_sweep_full_size(hip_lib, dtype, capsys):
    """the configuration of test_segment_volume_full_size: dense_rnn_net, 224 x 224 x 12 windows over the 224 x 224 x 40
    phantom, maxi[2] clipped so that at most 6 windows run (the model's own seeded initial weights: product is compared with
    product).  Two eager sweeps, then the captured one.  Eager runs bit-equal -> the captured run must be bit-equal to them
    (same kernels, same order).  Otherwise the bound is 4 x the largest eager-to-eager absolute score difference (a third draw
    from the same rounding noise) and the masks at 0.5 may differ on at most 1e-4 of the voxels (the cap of
    test_sliding_window.py).  Both differences are printed before the assertions (DESIGN.md section 3.11 records them)."""
    f = U.pkg("funcs")
    args = U.make_args(1, 224, 12)
    m = U.pkg("hybridnet").dense_rnn_net(args, dtype=dtype)
    vol, lab = U.pkg("synth").synthetic_ct((224, 224, 40), seed=3)
    _, mini, maxi = f.liver_window_from_mask(lab.astype(np.int16))
    # maxi[2] clipped so that at most 6 windows run: starts left, left + 3, ..., left + 15 = min(z, maxi[2] + 10) - 12
    left = max(0, int(mini[2]) - 5)
    maxi = np.array([maxi[0], maxi[1], min(int(maxi[2]), left + 17)])
    nwin = len(U.pkg("sweep").window_starts(40, 12, mini, maxi))
    assert 2 <= nwin <= 6
    e1, n1 = f.sweep_scores(m, vol, 3, mini, maxi, args)
    e2, n2 = f.sweep_scores(m, vol, 3, mini, maxi, args)
    gs, gn = f.sweep_scores(m, vol, 3, mini, maxi, args, mode="graph")
    plan = m._sweep_plan
    assert plan.captures == 1 and plan.replays == nwin and plan.graph is not None
    assert np.array_equal(gn.cpu().numpy(), n1) and np.array_equal(n1, n2)
    assert bool(torch.isfinite(e1).all()) and float(e1.max()) > 0
    noise = float((e1 - e2).abs().max())
    d1, d2 = float((gs - e1).abs().max()), float((gs - e2).abs().max())
    eager_equal = bool(torch.equal(e1, e2))
    with capsys.disabled():
        print("\ncaptured sweep %s: %d windows, eager-to-eager max |d| %.3e (bit-equal: %s), captured-to-eager %.3e / %.3e"
              % (dtype, nwin, noise, eager_equal, d1, d2))
    if eager_equal:
        assert torch.equal(gs, e1)
    else:
        assert max(d1, d2) <= 4.0 * noise
        den = torch.from_numpy(n1).to(gs.device).reshape(-1, 1, 1, 1) + 1e-4
        for e in (e1, e2):
            assert float((((gs / den) >= 0.5) != ((e / den) >= 0.5)).float().mean()) <= 1e-4
    # a second captured sweep reuses the graph
    g2, _ = f.sweep_scores(m, vol, 3, mini, maxi, args, mode="graph")
    assert m._sweep_plan is plan and plan.captures == 1 and plan.replays == nwin
    if eager_equal:
        assert torch.equal(g2, e1)


@pytest.mark.gpu
def test_capture_predict_2d_on_hardware(hip_lib):
    """capture_predict on the 2D net at 1 x 224 x 224 against the eager predict; predict() replays the graph afterwards"""
    m = U.pkg("denseunet").DenseUNet(reduction=0.5, args=U.make_args(1, 224), dtype="f32")
    x, _ = U.synthetic_batch("2d", 1, 224, None)
    a = m.predict(x)
    b = m.predict(x)
    m.capture_predict()
    assert m._predict_graph is not None
    c = m.predict(x)
    noise = float(np.abs(a - b).max())
    print("capture_predict 2d: eager-to-eager max |d| %.3e, captured-to-eager %.3e" % (noise, float(np.abs(c - a).max())))
    assert np.isfinite(a).all() and float(np.abs(a).max()) > 0
    if np.array_equal(a, b):
        assert np.array_equal(c, a)
    else:
        assert float(np.abs(c - a).max()) <= 4.0 * noise
    x2, _ = U.synthetic_batch("2d", 1, 224, None, seed=99)
    assert not np.array_equal(m.predict(x2), c)
