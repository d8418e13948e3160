"""Tiled 3-D sliding-window inference (lib/funcs.py:54-153: predict_window_mulgpu, get_binary_mask, GeneSeglivertumor): a
literal numpy restatement of the reference loop is held to arrays the REFERENCE'S OWN function produced
(tests/golden/make_tiled_window_fixture.py), and the HBM-resident product (funcs.predict_window_mulgpu / tiled_sweep_scores /
segment_volume_tiled, sweep.TiledSweepPlan) is held to the restatement driven through Model.predict."""
import os
import sys

import numpy as np
import pytest
import torch

import parity_utils as U

sys.path.insert(0, os.path.join(U.ROOT, "tests", "golden"))
from make_tiled_window_fixture import StandInModel2      # noqa: E402


def _axis_starts(n, t):
    w = (t // 3) * 2                                      # lib/funcs.py:56-58 (py2 integer division)
    return [min(s, n - t) for s in range(0, n - t + w, w)]        # :74-96: a start past n - t is clamped onto it


def _tiles(shape, tile):
    xs, ys, zs = (_axis_starts(n, t) for n, t in zip(shape, tile))
    return [(a, b, c) for a in xs for b in ys for c in zs]


def reference_tiled_loop(model, batch, vol, deps, rows, cols, flush):
    """lib/funcs.py:54-129 restated with numpy (softmax via numpy instead of K.softmax / K.eval); `model` only needs
    .predict(box, verbose).  flush=False is the reference: a box is predicted only when it is full, the leftover tiles never
    are.  flush=True is the product's contract: the last box is padded with its last tile, predicted, and only its valid tiles
    are added."""
    x, y, z = vol.shape
    tiles = _tiles((x, y, z), (deps, rows, cols))
    score = score_num = None
    for t0 in range(0, len(tiles), batch):
        step = tiles[t0:t0 + batch]
        if len(step) < batch and not flush:
            break
        box = np.zeros((batch, deps, rows, cols, 1), np.float32)
        for i in range(batch):
            a, b, c = step[min(i, len(step) - 1)]
            box[i, :, :, :, 0] = vol[a:a + deps, b:b + rows, c:c + cols]
        m = model.predict(box, verbose=0)
        e = np.exp(m - m.max(-1, keepdims=True))
        m = e / e.sum(-1, keepdims=True)
        if score is None:
            score = np.zeros((x, y, z, m.shape[-1]), np.float32)
            score_num = np.zeros((x, y, z, m.shape[-1]), np.int16)
        for i, (a, b, c) in enumerate(step):
            score[a:a + deps, b:b + rows, c:c + cols, :] += m[i]
            score_num[a:a + deps, b:b + rows, c:c + cols, :] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        score = score / score_num
    return score[:, :, :, 1]


# ------------------------------------------------------------------ the restatement against the reference's own function
def _fixture_cases():
    z = np.load(os.path.join(U.ROOT, "tests", "golden", "ref_funcs_tiled_window.npz"))
    n = len([k for k in z.files if k.startswith("meta")])
    assert n == 5
    for i in range(n):
        meta = [int(v) for v in z["meta%d" % i]]
        shape, tile, batch, seed = tuple(meta[0:3]), tuple(meta[3:6]), meta[6], meta[7]
        vol = np.random.default_rng(seed).normal(0.0, 40.0, shape).astype(np.float32)
        yield shape, tile, batch, vol, z["score%d" % i]


def test_restatement_equals_the_references_own_function():
    seen = []
    for shape, tile, batch, vol, want in _fixture_cases():
        ntiles = len(_tiles(shape, tile))
        got = reference_tiled_loop(StandInModel2(), batch, vol, *tile, flush=False)
        assert got.shape == want.shape == shape and got.dtype == np.float32
        if ntiles % batch == 0:
            assert np.isfinite(want).all()
            np.testing.assert_allclose(got, want, atol=2e-6)
            assert 0.1 < float(want.max()) and float(want.std()) > 0.01
        else:
            assert (shape, tile, batch) == ((20, 17, 13), (9, 8, 6), 5) and ntiles == 36
            assert int(np.isnan(want).sum()) == 15
            assert np.array_equal(np.isnan(got), np.isnan(want))
            np.testing.assert_allclose(got[np.isfinite(want)], want[np.isfinite(want)], atol=2e-6)
            # the product's contract: the tail step runs, no voxel is left uncovered; where the tail tiles do not reach, the
            # reference's result stands
            full = reference_tiled_loop(StandInModel2(), batch, vol, *tile, flush=True)
            assert np.isfinite(full).all()
            reach = np.zeros(shape, bool)
            for a, b, c in _tiles(shape, tile)[ntiles - ntiles % batch:]:
                reach[a:a + tile[0], b:b + tile[1], c:c + tile[2]] = True
            assert not (np.isnan(want) & ~reach).any()
            keep = np.isfinite(want) & ~reach
            assert keep.sum() > 0.5 * keep.size
            np.testing.assert_allclose(full[keep], want[keep], atol=2e-6)
        seen.append((shape, tile, batch))
    assert seen == [((20, 17, 13), (9, 8, 6), 1), ((16, 16, 12), (16, 8, 6), 1), ((22, 14, 9), (9, 9, 6), 2),
                    ((13, 13, 13), (6, 6, 6), 3), ((20, 17, 13), (9, 8, 6), 5)]


def test_tile_starts_table_and_coverage():
    sweep = U.pkg("sweep")
    assert sweep.tile_starts(17, 8) == [0, 4, 8, 9]
    assert sweep.tile_starts(8, 8) == [0] and sweep.tile_starts(9, 8) == [0, 1]
    for n, t in ((20, 9), (13, 6), (512, 224), (64, 12), (40, 32), (36, 32), (12, 8)):
        assert sweep.tile_starts(n, t) == _axis_starts(n, t)
    assert (sweep.tile_starts(40, 32), sweep.tile_starts(36, 32), sweep.tile_starts(12, 8)) == ([0, 8], [0, 4], [0, 4])
    shape, tile = (20, 17, 13), (9, 8, 6)
    table = sweep.tile_table(shape, tile)
    assert table.dtype == np.int32 and table.shape == (36, 3)
    assert [tuple(int(v) for v in r) for r in table] == _tiles(shape, tile)
    count = np.zeros(shape, np.int64)
    for a, b, c in _tiles(shape, tile):
        count[a:a + 9, b:b + 8, c:c + 6] += 1
    cx, cy, cz = sweep.tile_coverage(shape, tile)
    assert cx.dtype == np.float32 and (cx.shape, cy.shape, cz.shape) == ((20,), (17,), (13,))
    assert np.array_equal(cx[:, None, None] * cy[None, :, None] * cz[None, None, :], count)
    with pytest.raises(ValueError):
        sweep.tile_starts(7, 8)


# ------------------------------------------------------------------ the product against the restatement (emulator)
TINY = dict(dtype="f32", nb_layers2d=(2, 2, 2, 2), nb_layers3d=(1, 1, 2, 1))
_cache = {}


def _model(W, dtype="f32"):
    kw = dict(TINY, dtype=dtype)
    if W > 1:
        kw["window_batch"] = W
    return U.pkg("hybridnet").dense_rnn_net(U.make_args(1, 32, 8), **kw)


def _emu_case(W):
    """the tiny model of test_sliding_window.py, a (40, 36, 12) volume (8 tiles that overlap in every axis) and the eager product
    result, computed once per window_batch"""
    if W not in _cache:
        model = _model(W)
        vol, _ = U.pkg("synth").synthetic_ct((40, 36, 12), seed=3)
        assert len(_tiles(vol.shape, (32, 32, 8))) == 8
        got = U.pkg("funcs").predict_window_mulgpu(model, W, vol, 32, 32, 8, False)
        _cache[W] = (model, vol, got)
    return _cache[W]


# One sweep of the tiny model over this volume takes about a minute on the emulator (8 or 9 forwards), hence `slow`; every
# test below runs as few sweeps as its claim needs and shares the eager result of _emu_case.
@pytest.mark.slow
@pytest.mark.parametrize("W", [1, 3])
def test_tiled_window_matches_reference_loop(emu_lib, W):
    """W = 3: 8 tiles -> 3 steps, the last with 2 valid slots"""
    model, vol, got = _emu_case(W)
    want = reference_tiled_loop(model, W, vol, 32, 32, 8, flush=True)
    assert got.shape == (40, 36, 12) and got.dtype == np.float32
    assert np.isfinite(got).all() and float(got.std()) > 0
    print("tiled window W=%d vs restatement: max abs err %.3e" % (W, float(np.abs(got - want).max())))
    np.testing.assert_allclose(got, want, atol=2e-6)


@pytest.mark.slow
@pytest.mark.parametrize("W", [1, 3])
def test_tiled_graph_mode_equals_eager(emu_lib, W):
    model, vol, eager = _emu_case(W)
    g = U.pkg("funcs").predict_window_mulgpu(model, W, vol, 32, 32, 8, False, mode="graph")
    assert np.array_equal(g.view(np.uint32), eager.view(np.uint32))
    plan = model._tiled_sweep_plan
    assert plan.replays == -(-8 // W) and plan.ntiles == 8 and plan.steps == -(-8 // W)


@pytest.mark.slow
def test_tiled_plan_reuse_and_preprocessing_in_the_gather(emu_lib):
    """a second volume of the same shape reuses the model's plan; a preprocessing sweep of the raw volume is bit-equal to the
    eager sweep of the host-preprocessed one.  (Nothing is captured on the emulator build, so `captures` says nothing here:
    that a second volume needs no second capture is asserted on hardware, test_captured_tiled_sweep_on_hardware.)"""
    model, vol, _ = _emu_case(1)
    f = U.pkg("funcs")
    plan = U.pkg("sweep").tiled_plan_for(model, vol.shape, 3)
    captures = plan.captures
    raw = (vol * 3.0 + 100.0).astype(np.float32)
    lo, hi, mean = -60.0, 250.0, 48.0
    pre = np.clip(raw, np.float32(lo), np.float32(hi)).astype(np.float32) - np.float32(mean)
    assert (raw < lo).any() and (raw > hi).any() and not np.array_equal(pre, vol)
    s2 = f.tiled_sweep_scores(model, pre, 3, mode="eager")[0]
    assert model._tiled_sweep_plan is plan and plan.captures == captures and plan.replays == 8
    s2 = s2.clone()
    s1 = f.tiled_sweep_scores(model, raw, 3, mode="graph", preprocess=(lo, hi, mean))[0]
    assert model._tiled_sweep_plan is not plan and model._tiled_sweep_plan.key() == ((40, 36, 12), 3, (lo, hi, mean))
    assert torch.equal(s1, s2) and float(s1.abs().max()) > 0


@pytest.mark.slow
def test_segment_volume_tiled_equals_host_post_processing(emu_lib):
    model, vol, score = _emu_case(1)
    f = U.pkg("funcs")
    # get_binary_mask thresholds at 0.5, and the tiny untrained net's scores may sit on one side of it: the device form takes the
    # threshold, so it is first compared at a cut that splits the volume ...
    thres = float(np.median(score))
    got = f.segment_volume_tiled(model, vol, thres=thres)
    want = f.get_binary_mask((score.astype(np.float64) >= thres).astype(np.float32), 0)
    assert got.dtype == np.int16 and want.dtype == np.int16 and got.shape == (40, 36, 12)
    assert np.array_equal(got, want) and 0 < int(want.sum()) < want.size
    # ... and then at the reference's own 0.5 on the scores that sweep left resident (an all-clear mask raises in both forms)
    plan = model._tiled_sweep_plan
    arg = score.copy()
    if (score >= 0.5).any():
        lab = f.segment_tiled_scores(plan.score, plan.coverage, vol.shape)
        assert lab.dtype == np.int16 and np.array_equal(lab, f.get_binary_mask(arg, 0))
    else:
        with pytest.raises(ValueError, match="no foreground component"):
            f.get_binary_mask(arg, 0)
        with pytest.raises(ValueError, match="no foreground component"):
            f.segment_tiled_scores(plan.score, plan.coverage, vol.shape)
    assert np.array_equal(arg, (score >= 0.5).astype(np.float32))


def test_gene_seg_liver_tumor_on_hand_made_volumes():
    f = U.pkg("funcs")
    s = np.zeros((6, 7, 8), np.float32)
    s[0:2, 0:2, 0:2] = 0.9                       # 8 voxels, first in raster order
    s[4:6, 4:6, 4:6] = 0.5                       # 8 voxels: a tie, and 0.5 itself is set
    s[2, 6, 7] = 0.7                             # a smaller one
    s[3, 0, 0] = 0.49
    arg = s.copy()
    lab = f.GeneSeglivertumor(arg)
    want = np.zeros(s.shape, bool)
    want[0:2, 0:2, 0:2] = True
    assert np.array_equal(lab.astype(bool), want) and set(np.unique(lab)) == {0, 1}
    assert np.array_equal(arg, (s >= 0.5).astype(np.float32))          # thresholded in place, as the reference does
    # 26-connectivity: two voxels that touch at a corner are one component
    c = np.zeros((4, 4, 4), np.float32)
    c[0, 0, 0] = c[1, 1, 1] = 1.0
    c[3, 3, 3] = 1.0
    assert int(f.GeneSeglivertumor(c.copy()).sum()) == 2
    m = f.get_binary_mask(s.copy(), 7)
    assert m.dtype == np.int16 and np.array_equal(m.astype(bool), want)
    with pytest.raises(ValueError, match="no foreground component"):
        f.GeneSeglivertumor(np.full((3, 3, 3), 0.2, np.float32))


def test_tiled_argument_errors(emu_lib):
    """every refusal comes before the first forward"""
    f, sweep = U.pkg("funcs"), U.pkg("sweep")
    model = _cache[1][0] if 1 in _cache else _model(1)
    vol = np.zeros((40, 36, 12), np.float32)
    with pytest.raises(ValueError, match="window_batch"):
        f.predict_window_mulgpu(model, 2, vol, 32, 32, 8, False)
    for tile in ((16, 32, 8), (32, 16, 8), (32, 32, 6)):
        with pytest.raises(ValueError, match="window"):
            f.predict_window_mulgpu(model, 1, vol, *tile, False)
    for shape in ((31, 36, 12), (40, 31, 12), (40, 36, 7)):
        with pytest.raises(ValueError, match="smaller"):
            f.predict_window_mulgpu(model, 1, np.zeros(shape, np.float32), 32, 32, 8, False)
    with pytest.raises(ValueError, match="multiloss"):
        f.predict_window_mulgpu(model, 1, vol, 32, 32, 8, True)
    with pytest.raises(ValueError, match="mode"):
        f.predict_window_mulgpu(model, 1, vol, 32, 32, 8, False, mode="captured")
    with pytest.raises(ValueError, match="channel"):
        f.predict_window_mulgpu(model, 1, vol, 32, 32, 8, False, channel=3)
    with pytest.raises(ValueError, match="num"):
        f.tiled_sweep_scores(model, vol, 4)
    with pytest.raises(ValueError, match="preprocess"):
        f.tiled_sweep_scores(model, vol, 3, preprocess=(2.0, 1.0, 0.0))

    class _Ctx:
        def shard_world(self):
            return 1

    class _Model2D:
        kind, ctx, input_shape = "2d", _Ctx(), (1, 32, 32, 3)

    m2d = _Model2D()
    with pytest.raises(ValueError, match="hybrid"):
        f.tiled_sweep_scores(m2d, vol)
    with pytest.raises(ValueError, match="hybrid"):
        f.predict_window_mulgpu(m2d, 1, vol, 32, 32, 8, False)

    class _Sharded:
        def shard_world(self):
            return 2

    class _ShardedModel:
        kind, ctx, input_shape = "hybrid", _Sharded(), (1, 32, 32, 8, 1)

    with pytest.raises(ValueError, match="unsharded"):
        f.tiled_sweep_scores(_ShardedModel(), vol)
    with pytest.raises(ValueError, match="unsharded"):
        sweep.TiledSweepPlan(_ShardedModel(), vol.shape, 3)


def test_compat_funcs_exposes_the_tiled_names(emu_lib):
    sys.path.insert(0, os.path.join(U.ROOT, "compat"))
    try:
        import importlib
        cf = importlib.import_module("lib.funcs")
        f = U.pkg("funcs")
        assert cf.predict_window_mulgpu is f.predict_window_mulgpu
        assert cf.get_binary_mask is f.get_binary_mask and cf.GeneSeglivertumor is f.GeneSeglivertumor
    finally:
        sys.path.remove(os.path.join(U.ROOT, "compat"))


# ------------------------------------------------------------------ hardware
@pytest.mark.gpu
@pytest.mark.parametrize("W", [1, 4])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_captured_tiled_sweep_on_hardware(hip_lib, dtype, W, capsys):
    """the tiny model over a (72, 40, 21) volume: 3 x 2 x 5 = 30 tiles.  Two eager sweeps, then the captured one.  Eager runs
    bit-equal -> the captured run must be bit-equal to them (same kernels, same order).  Otherwise the bound is 4 x the largest
    eager-to-eager absolute score difference and the masks at 0.5 may differ on at most 1e-4 of the voxels
    (test_captured_sweep_full_size's rule).  f32, W = 1 also against the restatement through Model.predict: atol 2e-6, or
    4 x the eager-to-eager noise of the averaged scores if that is larger."""
    f = U.pkg("funcs")
    model = _model(W, dtype)
    vol, _ = U.pkg("synth").synthetic_ct((72, 40, 21), seed=3)
    ntiles = len(_tiles(vol.shape, (32, 32, 8)))
    assert ntiles == 30
    e1 = f.tiled_sweep_scores(model, vol, 3)[0].clone()
    e2 = f.tiled_sweep_scores(model, vol, 3)[0].clone()
    gs, (cx, cy, cz) = f.tiled_sweep_scores(model, vol, 3, mode="graph")
    gs = gs.clone()
    plan = model._tiled_sweep_plan
    assert plan.captures == 1 and plan.replays == -(-ntiles // W) and plan.graph is not None
    assert bool(torch.isfinite(e1).all()) and float(e1.max()) > 0
    noise = float((e1 - e2).abs().max())
    d1, d2 = float((gs - e1).abs().max()), float((gs - e2).abs().max())
    eager_equal = bool(torch.equal(e1, e2))
    with capsys.disabled():
        print("\ncaptured tiled sweep %s W=%d: %d tiles, eager-to-eager max |d| %.3e (bit-equal: %s), captured-to-eager %.3e / %.3e"
              % (dtype, W, ntiles, noise, eager_equal, d1, d2))
    den = (cz.reshape(-1, 1, 1, 1) * cx.reshape(1, -1, 1, 1) * cy.reshape(1, 1, -1, 1))
    assert float(den.min()) >= 1
    if eager_equal:
        assert torch.equal(gs, e1)
    else:
        assert max(d1, d2) <= 4.0 * noise
        for e in (e1, e2):
            assert float((((gs / den) >= 0.5) != ((e / den) >= 0.5)).float().mean()) <= 1e-4
    # a captured sweep of ANOTHER volume of the same shape reuses the plan and its graph, and is held to the eager sweep of
    # that volume by the same rule
    vol2, _ = U.pkg("synth").synthetic_ct((72, 40, 21), seed=4)
    assert not np.array_equal(vol, vol2)
    g2 = f.tiled_sweep_scores(model, vol2, 3, mode="graph")[0].clone()
    assert model._tiled_sweep_plan is plan and plan.captures == 1 and plan.replays == -(-ntiles // W)
    e3 = f.tiled_sweep_scores(model, vol2, 3)[0].clone()
    assert model._tiled_sweep_plan is plan and plan.captures == 1
    d3 = float((g2 - e3).abs().max())
    with capsys.disabled():
        print("second volume, captured-to-eager %.3e, to the first volume's scores %.3e" % (d3, float((g2 - gs).abs().max())))
    assert not torch.equal(g2, gs)
    if eager_equal:
        assert torch.equal(g2, e3)
    else:
        assert d3 <= 4.0 * noise
    if dtype == "f32" and W == 1:
        got = f.predict_window_mulgpu(model, 1, vol, 32, 32, 8, False, mode="graph")
        want = reference_tiled_loop(model, 1, vol, 32, 32, 8, flush=True)
        avg_noise = float(((e1 - e2).abs() / den).max())
        err = float(np.abs(got - want).max())
        with capsys.disabled():
            print("tiled window f32 vs restatement through Model.predict: max abs err %.3e, eager-to-eager noise of the "
                  "averaged scores %.3e" % (err, avg_noise))
        assert err <= max(2e-6, 4.0 * avg_noise)
        # the device post-processing equals the host form: on the scores that sweep left resident (always), and through
        # segment_volume_tiled's own sweep when sweeps are run-to-run bit-equal
        thres = float(np.median(got))
        host = f.get_binary_mask((got.astype(np.float64) >= thres).astype(np.float32), 0)
        assert host.dtype == np.int16 and 0 < int(host.sum()) < host.size
        lab = f.segment_tiled_scores(plan.score, plan.coverage, vol.shape, thres=thres)
        assert lab.dtype == np.int16 and np.array_equal(lab, host)
        lab = f.segment_volume_tiled(model, vol, mode="graph", thres=thres)
        assert lab.dtype == np.int16 and lab.shape == host.shape and plan.captures == 1
        if eager_equal:
            assert np.array_equal(lab, host)
