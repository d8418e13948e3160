"""Window-batched hybrid inference: Model(kind="hybrid", window_batch=W) runs W sliding windows per forward, and the sweeps
(funcs.sweep_scores, sweep.SweepPlan) take W from the model.  Windows are independent (phase 0: every BN on stored statistics),
each is held to the float64 oracle's predict of that window alone, and the captured batched sweep is held to the host-driven
batched one.  The emulator tier runs the small hybrid of test_sweep_plan.py; the MI355X tier adds bf16 and the full size."""
import math

import numpy as np
import pytest
import torch

import parity_utils as U
from test_sliding_window import _OraclePredictor, reference_loop

NB2D, NB3D = (2, 2, 2, 2), (1, 1, 2, 1)


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pair_with_batched(size, cols, dtype, W, nb2d=NB2D, nb3d=NB3D, **kw):
    """(W = 1 product model, W-window product model, oracle ParamStore, oracle forward), all on the same weights"""
    m1, P, fwd = U.build_pair("hybrid", "end2end", 1, size, cols, dtype, nb2d, nb3d, **kw)
    mw = U.pkg("hybridnet").dense_rnn_net(U.make_args(1, size, cols), dtype=dtype, nb_layers2d=nb2d, nb_layers3d=nb3d,
                                          window_batch=W)
    mw.set_weights_dict(m1.get_weights_dict())
    return m1, mw, P, fwd


def _windows(W, size, cols, seed0=100):
    """W different windows (W, size, size, cols, 1)"""
    return np.concatenate([U.synthetic_batch("hybrid", 1, size, cols, seed=seed0 + 7 * i)[0] for i in range(W)], 0)


def _oracle_refs(P, fwd, x):
    """the oracle's predict of every window of x alone"""
    return [U.R.predict(P, fwd, torch.tensor(x[i:i + 1], dtype=P.dtype)).numpy() for i in range(x.shape[0])]


def _oracle_errors(model, refs, x, got=None):
    """per window of x: (max |got - ref|, mean |got - ref|, scale, min dice) against the oracle's predict of that window alone"""
    if got is None and model.window_batch == x.shape[0]:
        got = model.predict(x).copy()
    elif got is None:
        got = np.concatenate([model.predict(x[i:i + 1]).copy() for i in range(x.shape[0])], 0)
    out = []
    for i, ref in enumerate(refs):
        d = np.abs(got[i:i + 1] - ref)
        out.append((float(d.max()), float(d.mean()), max(1.0, float(np.abs(ref).max())), min(U.dice_vs_oracle(got[i:i + 1], ref))))
    return out


# ------------------------------------------------------------------ emulator tier: models built once per module
_SHARED = {}


def _shared():
    if "m" not in _SHARED:
        _SHARED["m"] = _pair_with_batched(32, 8, "f32", 3)
    return _SHARED["m"]


def _shared_predict():
    """(three windows, the W = 3 model's logits for them), computed once"""
    if "p" not in _SHARED:
        x = _windows(3, 32, 8)
        _SHARED["p"] = (x, _shared()[1].predict(x).copy())
    return _SHARED["p"]


LOW = ((0, 0, 0), (31, 31, 0))          # window starts 0, 2 over z = 14: one partly filled step of 3
WIDE = ((0, 0, 6), (31, 31, 13))        # window starts 1, 3, 5, 6 (the last one clamped): two steps, the second holds one window


def test_windows_of_one_forward_are_independent(emu_lib):
    """predict on windows (a, b, c) and on (a, b', c): slots 0 and 2 bit-identical, slot 1 different.  Depth padding of the 3D
    convs / pools or a slab edge leaking into the neighbouring window would change slot 0 or 2."""
    _, m3, _, _ = _shared()
    assert m3.input_shape == (3, 32, 32, 8, 1) and m3.output_shape == (3, 32, 32, 8, 3)
    assert m3.vol.numel() == 3 * 8 * 32 * 32
    x, a = _shared_predict()
    x2 = x.copy()
    x2[1] = _windows(1, 32, 8, seed0=991)[0]
    b = m3.predict(x2).copy()
    assert a.shape == (3, 32, 32, 8, 3) and np.isfinite(a).all()
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[2]), _bits(b[2]))
    assert not np.array_equal(_bits(a[1]), _bits(b[1]))
    assert not np.array_equal(_bits(a[0]), _bits(a[2]))


def test_batched_predict_against_float64_oracle(emu_lib, capsys):
    """three different windows in one forward, each against the float64 oracle's predict of that window: the bounds of
    test_gpu_parity.py::test_full_forward_parity_f32 (1e-4 of the logit scale, Dice >= 1 - 1e-3)"""
    m1, m3, P, fwd = _shared()
    x, got = _shared_predict()
    refs = _oracle_refs(P, fwd, x)
    eb = _oracle_errors(m3, refs, x, got)
    e1 = _oracle_errors(m1, refs, x)
    with capsys.disabled():
        print("\nwindow_batch=3 f32 32x32x8 vs float64 oracle, max |err| per window: batched %s, unbatched %s"
              % (["%.2e" % e[0] for e in eb], ["%.2e" % e[0] for e in e1]))
    for mx, _, scale, dice in eb:
        assert mx <= 1e-4 * scale
        assert dice >= 1 - 1e-3


@pytest.mark.parametrize("win,starts", [(LOW, [0, 2]), (WIDE, [1, 3, 5, 6])], ids=["one-step", "two-steps"])
def test_batched_graph_sweep_equals_batched_eager(emu_lib, win, starts):
    """32 x 32 x 14 volume on the W = 3 model: mode="graph" bit-equal to mode="eager" (score and count), ceil(nwin / 3) steps, and
    the count of the W = 1 model's sweep"""
    f, sweep = U.pkg("funcs"), U.pkg("sweep")
    m1, m3, _, _ = _shared()
    args = U.make_args(1, 32, 8)
    mini, maxi = win
    assert sweep.window_starts(14, 8, mini, maxi) == starts
    vol, _ = U.pkg("synth").synthetic_ct((32, 32, 14), seed=3)
    es, en = f.sweep_scores(m3, vol, 3, mini, maxi, args)
    gs, gn = f.sweep_scores(m3, vol, 3, mini, maxi, args, mode="graph")
    plan = m3._sweep_plan
    assert plan.batch == 3 and plan.capacity % 3 == 0
    assert plan.replays == math.ceil(len(starts) / 3) and plan.captures == 0      # (no graphs on the emulator)
    assert np.array_equal(_bits(gs), _bits(es))
    assert np.array_equal(gn.cpu().numpy(), en)
    assert float(es.abs().max()) > 0
    want = np.zeros(14, np.float32)
    for c0 in starts:
        want[c0 + 1:c0 + 7] += 1
    assert np.array_equal(en, want)
    if len(starts) == 2:                      # (the W = 1 model's own sweep: two more forwards, kept to the short case)
        s1, n1 = f.sweep_scores(m1, vol, 3, mini, maxi, args)
        assert np.array_equal(n1, en) and float(s1.abs().max()) > 0
    assert m3.ctx.learning_phase == 1 and m3.ctx._prefolded_phase is None


def test_batched_segment_volume_graph_equals_eager(emu_lib):
    f = U.pkg("funcs")
    _, m3, _, _ = _shared()
    args = U.make_args(1, 32, 8)
    vol, lab = U.pkg("synth").synthetic_ct((32, 32, 14), seed=3)
    mask = np.zeros(lab.shape, np.int16)
    mask[8:24, 8:24, 0] = 1
    _, mini, maxi = f.liver_window_from_mask(mask)
    assert U.pkg("sweep").window_starts(14, 8, mini, maxi) == [0, 2, 4]
    s1, s2 = f.predict_tumor_inwindow(m3, vol, 3, mini, maxi, args, mode="graph")
    tl, tt = float(np.quantile(s1[s1 > 0], 0.4)), float(np.quantile(s2[s2 > 0], 0.5))
    ref = f.segment_volume(m3, vol, mask, args, tl, tt)
    got = f.segment_volume(m3, vol, mask, args, tl, tt, mode="graph")
    assert got.dtype == np.uint8 and got.shape == (32, 32, 14) and np.array_equal(got, ref)
    assert (got == 1).any()


def test_window_batch_model_surface(emu_lib):
    """a W-model is the W = 1 model with more windows per forward: same layers and weights, inference only"""
    ka, hn = U.pkg("keras_api"), U.pkg("hybridnet")
    m1, m3, _, _ = _shared()
    assert m1.window_batch == 1 and m3.window_batch == 3
    assert m3.layer_names() == m1.layer_names()
    w1, w3 = m1.get_weights_dict(), m3.get_weights_dict()
    assert list(w1.keys()) == list(w3.keys())
    for k in w1:
        assert [np.shape(a) for a in w1[k]] == [np.shape(a) for a in w3[k]], k
        assert all(np.array_equal(a, b) for a, b in zip(w1[k], w3[k])), k
    m1.set_weights_dict(w3)
    m3.set_weights_dict(m1.get_weights_dict())
    assert all(np.array_equal(a, b) for k in w1 for a, b in zip(w1[k], m3.get_weights_dict()[k]))
    x, y = U.synthetic_batch("hybrid", 1, 32, 8)
    x3 = np.concatenate([x, x, x], 0)
    m3.compile(optimizer=ka.SGD(lr=1e-3, momentum=0.9, nesterov=True), loss=[U.pkg("loss").weighted_crossentropy])
    for call in (lambda: m3.train_on_batch(x3, y), m3.train_step_resident, m3.capture_graph, lambda: m3.forward_train_mode(x3),
                 lambda: m3.fit_generator(iter([(x3, y)]), 1)):
        with pytest.raises(ValueError, match="inference-only"):
            call()
    with pytest.raises(ValueError, match="expected input"):
        m3.predict(x)
    args = U.make_args(1, 32, 8)
    for bad in (0, 9):
        with pytest.raises(ValueError, match="window_batch"):
            hn.dense_rnn_net(args, dtype="f32", nb_layers2d=NB2D, nb_layers3d=NB3D, window_batch=bad)
    shard = U.pkg("shard").ShardInfo(0, 1)
    with pytest.raises(ValueError, match="window_batch"):
        hn.dense_rnn_net(args, dtype="f32", nb_layers2d=NB2D, nb_layers3d=NB3D, window_batch=2, shard=shard)
    with pytest.raises(ValueError):
        hn.dense_rnn_net(U.make_args(2, 32, 8), dtype="f32", nb_layers2d=NB2D, nb_layers3d=NB3D, window_batch=2)


def test_denseunet_3d_window_batch_builds_and_predicts(emu_lib):
    m = U.pkg("denseunet3d").denseunet_3d(U.make_args(1, 32, 8), dtype="f32", nb_layers2d=NB2D, nb_layers3d=NB3D, window_batch=2)
    x = _windows(2, 32, 8)
    out = m.predict(x).copy()
    assert out.shape == (2, 32, 32, 8, 3) and np.isfinite(out).all() and float(np.abs(out).max()) > 0
    swapped = m.predict(x[::-1].copy())
    assert np.array_equal(_bits(swapped[0]), _bits(out[1])) and np.array_equal(_bits(swapped[1]), _bits(out[0]))


# ------------------------------------------------------------------ MI355X tier
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_batched_predict_against_oracle_on_hardware(hip_lib, dtype, capsys):
    """small hybrid at 64 x 64 x 8, window_batch = 3, per window against the float64 oracle.  f32: 1e-4 of the logit scale and
    Dice >= 1 - 1e-3, as the unbatched predict is held to.  bf16 has no absolute logit bound (storage noise of 0.06 - 0.5), so the
    batched error is held to the UNBATCHED product's error against the same oracle on the same windows: mean absolute error at
    most 1.25 x, maximum at most 2 x.  Both paths draw from the same bf16 storage noise and differ in the split-K grouping only,
    which moves the mean very little and the maximum by at most one extra draw."""
    m1, m3, P, fwd = _pair_with_batched(64, 8, dtype, 3)
    x = _windows(3, 64, 8)
    refs = _oracle_refs(P, fwd, x)
    eb = _oracle_errors(m3, refs, x)
    e1 = _oracle_errors(m1, refs, x)
    bmax, bmean = max(e[0] for e in eb), float(np.mean([e[1] for e in eb]))
    umax, umean = max(e[0] for e in e1), float(np.mean([e[1] for e in e1]))
    with capsys.disabled():
        print("\nwindow_batch=3 %s 64x64x8 vs float64 oracle: batched max %.3e mean %.3e, unbatched max %.3e mean %.3e, min dice "
              "batched %.5f unbatched %.5f" % (dtype, bmax, bmean, umax, umean, min(e[3] for e in eb), min(e[3] for e in e1)))
    if dtype == "f32":
        for mx, _, scale, dice in eb:
            assert mx <= 1e-4 * scale
            assert dice >= 1 - 1e-3
    else:
        assert bmean <= 1.25 * umean
        assert bmax <= 2.0 * umax


def _full_size_case(clip, nwin):
    """the 224 x 224 x 40 phantom with its liver window clipped to maxi[2] <= clip, which gives `nwin` windows of 12 planes"""
    f = U.pkg("funcs")
    vol, lab = U.pkg("synth").synthetic_ct((224, 224, 40), seed=3)
    _, mini, maxi = f.liver_window_from_mask((lab > 0).astype(np.uint8)[:, :, :])
    maxi = np.array([maxi[0], maxi[1], min(int(maxi[2]), clip)])
    assert U.pkg("sweep").window_starts(40, 12, mini, maxi) == list(range(0, 3 * nwin, 3))
    return vol, mini, maxi


@pytest.mark.gpu
def test_batched_sweep_full_size_vs_torch_oracle(hip_lib, capsys):
    """dense_rnn_net 224 x 224 x 12, window_batch = 4, captured, over the 224 x 224 x 40 phantom of
    test_sliding_window.py::test_sliding_window_full_size_vs_torch_oracle with its clipped liver window (maxi[2] <= 22: window
    starts 0, 3, ..., 21, so 8 windows in two full steps; the half-filled last step at full size is the case of
    test_captured_batched_sweep_full_size), against the literal reference loop driven by the float32 torch oracle, with that
    test's bounds."""
    f = U.pkg("funcs")
    args = U.make_args(1, 224, 12)
    _, m4, P, fwd = _pair_with_batched(224, 12, "f32", 4, nb2d=(6, 12, 36, 24), nb3d=(3, 4, 12, 8), odtype=torch.float32,
                                       perturb=False)
    vol, mini, maxi = _full_size_case(22, 8)
    s1, s2 = f.predict_tumor_inwindow(m4, vol, 3, mini, maxi, args, mode="graph")
    plan = m4._sweep_plan
    assert plan.captures == 1 and plan.replays == 2 and plan.graph is not None
    r1, r2 = reference_loop(_OraclePredictor(P, fwd), vol, 3, mini, maxi, args)
    e1, e2 = float(np.abs(s1 - r1).max()), float(np.abs(s2 - r2).max())
    with capsys.disabled():
        print("\nwindow_batch=4 captured sweep vs oracle: max abs score err %.2e / %.2e" % (e1, e2))
    assert e1 <= 1e-3 and e2 <= 1e-3
    for thr in (0.3, 0.5):
        for a, b in ((s1, r1), (s2, r2)):
            assert float(((a >= thr) != (b >= thr)).mean()) <= 1e-4
    assert float(np.abs(r1).max()) > 0
    t1, t2 = f.predict_tumor_inwindow(m4, vol, 3, mini, maxi, args, mode="graph")      # a second sweep reuses the graph
    assert m4._sweep_plan is plan and plan.captures == 1 and plan.replays == 2
    assert float(np.abs(t1 - r1).max()) <= 1e-3 and float(np.abs(t2 - r2).max()) <= 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_captured_batched_sweep_full_size(hip_lib, dtype, capsys):
    """the pattern of test_sweep_plan.py::test_captured_sweep_full_size on the window_batch = 4 model: two host-driven batched
    sweeps, then the captured one.  Eager runs bit-equal -> the captured run must be bit-equal; otherwise within 4 x the
    eager-to-eager difference with the 1e-4 mask cap.  The difference to the W = 1 model's eager sweep is printed, not asserted
    (another split-K grouping: DESIGN.md section 3.11 records it)."""
    f = U.pkg("funcs")
    args = U.make_args(1, 224, 12)
    m4 = U.pkg("hybridnet").dense_rnn_net(args, dtype=dtype, window_batch=4)
    vol, mini, maxi = _full_size_case(17, 6)        # that test's window: 6 windows, two steps, the second half filled
    e1, n1 = f.sweep_scores(m4, vol, 3, mini, maxi, args)
    e2, n2 = f.sweep_scores(m4, vol, 3, mini, maxi, args)
    gs, gn = f.sweep_scores(m4, vol, 3, mini, maxi, args, mode="graph")
    plan = m4._sweep_plan
    assert plan.captures == 1 and plan.replays == 2 and plan.graph is not None
    assert np.array_equal(gn.cpu().numpy(), n1) and np.array_equal(n1, n2)
    assert bool(torch.isfinite(e1).all()) and float(e1.max()) > 0
    noise = float((e1 - e2).abs().max())
    d1, d2 = float((gs - e1).abs().max()), float((gs - e2).abs().max())
    eager_equal = bool(torch.equal(e1, e2))
    den = torch.from_numpy(n1).to(gs.device).reshape(-1, 1, 1, 1) + 1e-4
    m1 = U.pkg("hybridnet").dense_rnn_net(args, dtype=dtype)
    m1.set_weights_dict(m4.get_weights_dict())
    u, nu = f.sweep_scores(m1, vol, 3, mini, maxi, args)
    with capsys.disabled():
        print("\ncaptured window_batch=4 sweep %s: eager-to-eager max |d| %.3e (bit-equal: %s), captured-to-eager %.3e / %.3e; "
              "to the W=1 eager sweep max |d| %.3e, 0.5-mask differs on %.3e of the voxels"
              % (dtype, noise, eager_equal, d1, d2, float((gs - u).abs().max()),
                 float((((gs / den) >= 0.5) != ((u / den) >= 0.5)).float().mean())))
    assert np.array_equal(nu, n1)
    if eager_equal:
        assert torch.equal(gs, e1)
    else:
        assert max(d1, d2) <= 4.0 * noise
        for e in (e1, e2):
            assert float((((gs / den) >= 0.5) != ((e / den) >= 0.5)).float().mean()) <= 1e-4


@pytest.mark.gpu
def test_capture_predict_window_batch_on_hardware(hip_lib, capsys):
    """capture_predict on the W = 4 model: the replayed predict equals the eager one (bit-equal if two eager runs are, otherwise
    within 4 x their difference)"""
    m4 = U.pkg("hybridnet").dense_rnn_net(U.make_args(1, 224, 12), dtype="f32", window_batch=4)
    x = _windows(4, 224, 12)
    a = m4.predict(x).copy()
    b = m4.predict(x).copy()
    m4.capture_predict()
    assert m4._predict_graph is not None
    c = m4.predict(x).copy()
    noise = float(np.abs(a - b).max())
    with capsys.disabled():
        print("\ncapture_predict window_batch=4: eager-to-eager max |d| %.3e, captured-to-eager %.3e" % (noise, float(np.abs(c - a).max())))
    assert a.shape == (4, 224, 224, 12, 3) and np.isfinite(a).all() and float(np.abs(a).max()) > 0
    if np.array_equal(a, b):
        assert np.array_equal(c, a)
    else:
        assert float(np.abs(c - a).max()) <= 4.0 * noise
