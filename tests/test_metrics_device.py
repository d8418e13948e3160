"""Device-resident segmentation metrics (include/hdu.h: hdu_metric_*; metrics.*_device, funcs.evaluate_volume) against their
host specification (metrics.py: numpy + scipy, MedPy's definitions), on the x86 emulator build and on the MI355X.

Tolerances.  Unit spacing: every squared distance is an integer below 2^53 and every operation on it is exact, so d2 is
compared exactly.  With a spacing both sides evaluate sqrt(sum (d_i s_i)^2) in double with at most 3 x 2 multiplications, 2
additions and a square root: each within about 2.5 * 2^-53 of the true value, about 6e-16 apart, and rounding is monotone so a
minimum of rounded values is the rounded minimum: rtol 1e-14 (the maximum distance `msd` too).  Means and rmsd: a sum of N
non-negative doubles in any order is within N * 2^-53 relative, N < 2^23 border voxels: 2^-30 = 9.3e-10, rtol 1e-9."""
import math

import numpy as np
import pytest
import torch
from scipy import ndimage

import parity_utils as U

SHAPES = [(23, 17, 13), (40, 9, 31), (3, 70, 2)]
SPACINGS = [(0.7, 0.7, 2.5), (0.6836, 0.6836, 1.25), (2.5, 1.0, 0.7)]
RTOL_DIST, RTOL_MEAN = 1e-14, 1e-9


def M():
    return U.pkg("metrics")


def O():
    return U.pkg("ops")


def dev_u8(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint8).reshape(-1)).to(O().device())


def dev_counts(pred, truth, mode):
    counts = torch.zeros(3, dtype=torch.int64, device=O().device())
    O().metric_counts(dev_u8(pred), dev_u8(truth), pred.shape, mode, counts)
    return tuple(int(v) for v in counts.cpu())


def dev_border(vol, mode=0):
    out = torch.empty(vol.size, dtype=torch.uint8, device=O().device())
    O().metric_border(dev_u8(vol), vol.shape, mode, out)
    return out.cpu().numpy().reshape(vol.shape)


def dev_edt(feature, spacing=None):
    dev = O().device()
    d2 = torch.empty(feature.size, dtype=torch.float64, device=dev)
    tmp = torch.empty(feature.size, dtype=torch.float64, device=dev)
    O().metric_edt(dev_u8(feature), feature.shape, spacing, tmp, d2)
    return d2.cpu().numpy().reshape(feature.shape)


def check_edt_unit(feature):
    assert feature.any()
    ref = np.rint(ndimage.distance_transform_edt(~feature) ** 2)
    np.testing.assert_array_equal(dev_edt(feature), ref)


def check_edt_spacing(feature, spacing):
    ref = ndimage.distance_transform_edt(~feature, sampling=spacing)
    got = np.sqrt(dev_edt(feature, spacing))
    np.testing.assert_array_equal(got == 0, ref == 0)
    np.testing.assert_allclose(got, ref, rtol=RTOL_DIST, atol=0)


def ellipsoid(shape, centre, semi):
    g = np.indices(shape).astype(np.float64)
    return sum(((g[i] - centre[i]) / semi[i]) ** 2 for i in range(3)) <= 1.0


def ellipsoid_pair():
    shape = (23, 17, 13)
    return ellipsoid(shape, (11, 8, 6), (8, 6, 5)), ellipsoid(shape, (12, 7, 6.5), (7, 6.5, 4))


def shifted(a, shift):
    """a moved by `shift` voxels, zeros coming in"""
    out = np.zeros_like(a)
    src = tuple(slice(max(0, -s), a.shape[i] - max(0, s)) for i, s in enumerate(shift))
    dst = tuple(slice(max(0, s), a.shape[i] - max(0, -s)) for i, s in enumerate(shift))
    out[dst] = a[src]
    return out


def synth_label_pair(shape=(32, 32, 12)):
    """synthetic_ct labels and a prediction: liver and tumour eroded by one voxel, moved by (1, -1, 2)"""
    lab = U.pkg("synth").synthetic_ct(shape, seed=3)[1].astype(np.uint8)
    liver = ndimage.binary_erosion(lab >= 1)
    tumor = ndimage.binary_erosion(lab == 2) & liver
    pred = shifted((liver.astype(np.uint8) + tumor), (1, -1, 2))
    return pred, lab


def assert_surface_close(got, ref):
    for k in ("n_rt", "n_tr"):
        assert got[k] == ref[k], k
    np.testing.assert_allclose(got["msd"], ref["msd"], rtol=RTOL_DIST, atol=0)
    for k in ("asd_rt", "asd_tr", "assd", "rmsd"):
        np.testing.assert_allclose(got[k], ref[k], rtol=RTOL_MEAN, atol=0, err_msg=k)


def assert_evaluation_close(got, ref):
    assert set(got) == set(ref) == {"liver", "tumor"}
    for name in ref:
        g, r = got[name], ref[name]
        assert set(g) == set(r)
        for k in ("n_result", "n_reference", "n_intersection"):
            assert g[k] == r[k], (name, k)
        for k in ("dice", "voe", "rvd"):                 # functions of the counts alone
            assert g[k] == r[k] or (math.isnan(g[k]) and math.isnan(r[k])), (name, k, g[k], r[k])
        if math.isnan(r["assd"]):
            assert all(math.isnan(g[k]) for k in M().SURFACE_FIELDS), name
        else:
            assert_surface_close(g, r)


# ------------------------------------------------------------------ CPU tier (emulator)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("density", [0.05, 0.5, 0.95])
def test_counts_match_host(emu_lib, shape, density):
    rng = np.random.default_rng(int(density * 100) + shape[0])
    pred = (rng.random(shape) < density) * rng.integers(1, 3, shape)
    truth = (rng.random(shape) < density) * rng.integers(1, 3, shape)
    assert dev_counts(pred, truth, 0) == M().overlap_counts(pred >= 1, truth >= 1)
    assert dev_counts(pred, truth, 1) == M().overlap_counts(pred == 2, truth == 2)


def faces_boxes(shape):
    X, Y, Z = shape
    for sl in ((slice(0, 2), slice(1, Y - 1), slice(1, Z - 1)), (slice(X - 2, X), slice(1, Y - 1), slice(1, Z - 1)),
               (slice(1, X - 1), slice(0, 2), slice(1, Z - 1)), (slice(1, X - 1), slice(Y - 2, Y), slice(1, Z - 1)),
               (slice(1, X - 1), slice(1, Y - 1), slice(0, 2)), (slice(1, X - 1), slice(1, Y - 1), slice(Z - 2, Z))):
        m = np.zeros(shape, bool)
        m[sl] = True
        yield m


@pytest.mark.parametrize("shape", SHAPES)
def test_border_matches_host(emu_lib, shape):
    rng = np.random.default_rng(shape[1])
    masks = [rng.random(shape) < d for d in (0.05, 0.5, 0.95)]
    masks.append(np.ones(shape, bool))                    # every face voxel is border
    single = np.zeros(shape, bool)
    single[shape[0] // 2, shape[1] // 2, shape[2] // 2] = True
    masks += [single, np.zeros(shape, bool)]
    if min(shape) >= 4:
        masks += list(faces_boxes(shape))
    for m in masks:
        np.testing.assert_array_equal(dev_border(m), M().border(m).astype(np.uint8))
    full = dev_border(np.ones(shape, bool)).astype(bool)
    inner = np.zeros(shape, bool)
    inner[1:-1, 1:-1, 1:-1] = True
    np.testing.assert_array_equal(full, ~inner)
    # a label volume under both class modes: the liver / tumour masks are never materialised
    lab = (rng.random(shape) < 0.7) * rng.integers(1, 3, shape)
    np.testing.assert_array_equal(dev_border(lab, 0), M().border(lab >= 1).astype(np.uint8))
    np.testing.assert_array_equal(dev_border(lab, 1), M().border(lab == 2).astype(np.uint8))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("density", [0.001, 0.05, 0.5])
def test_edt_unit_random(emu_lib, shape, density):
    rng = np.random.default_rng(int(density * 1000) + shape[2])
    f = rng.random(shape) < density
    f[tuple(rng.integers(0, s) for s in shape)] = True     # never empty
    check_edt_unit(f)


@pytest.mark.parametrize("shape", SHAPES)
def test_edt_unit_corners_planes_lines_voxels(emu_lib, shape):
    for corner in np.ndindex(2, 2, 2):
        f = np.zeros(shape, bool)
        f[tuple(c * (s - 1) for c, s in zip(corner, shape))] = True
        check_edt_unit(f)
    mid = tuple(s // 2 for s in shape)
    for axis in range(3):
        plane = np.zeros(shape, bool)
        plane[tuple(mid[a] if a == axis else slice(None) for a in range(3))] = True
        line = np.zeros(shape, bool)
        line[tuple(slice(None) if a == axis else mid[a] for a in range(3))] = True
        voxel = np.zeros(shape, bool)
        voxel[tuple(shape[a] - 1 if a == axis else mid[a] for a in range(3))] = True
        for f in (plane, line, voxel):
            check_edt_unit(f)


def test_edt_unit_ellipsoid_borders(emu_lib):
    for m in ellipsoid_pair():
        check_edt_unit(M().border(m))


@pytest.mark.parametrize("spacing", SPACINGS)
def test_edt_spacing(emu_lib, spacing):
    for shape in SHAPES:
        rng = np.random.default_rng(shape[0])
        for density in (0.001, 0.05, 0.5):
            f = rng.random(shape) < density
            f[tuple(rng.integers(0, s) for s in shape)] = True
            check_edt_spacing(f, spacing)
    for m in ellipsoid_pair():
        check_edt_spacing(M().border(m), spacing)


def test_edt_column_longer_than_the_lds_form(emu_lib):
    """z columns above 24576 voxels take the one-thread-per-column kernel of pass 1"""
    shape = (2, 3, 24600)
    f = np.random.default_rng(9).random(shape) < 0.0005
    f[1, 2, 0] = True
    check_edt_unit(f)
    check_edt_spacing(f, (0.7, 0.7, 2.5))


def test_edt_line_longer_than_64_segments(emu_lib):
    """x and y lines above 1024 voxels: the segments whose minima steer passes 2 and 3 grow beyond 16 positions"""
    for shape in ((1100, 3, 5), (2, 1037, 3)):
        f = np.random.default_rng(shape[1]).random(shape) < 0.002
        f[0, shape[1] - 1, 2] = True
        check_edt_unit(f)
        check_edt_spacing(f, (2.5, 1.0, 0.7))


def test_edt_empty_feature_is_inf(emu_lib):
    for shape in SHAPES:
        for spacing in (None, (0.7, 0.7, 2.5)):
            d2 = dev_edt(np.zeros(shape, bool), spacing)
            assert np.all(np.isposinf(d2))


def test_surface_metrics_device(emu_lib):
    m = M()
    a, b = ellipsoid_pair()
    pred, lab = synth_label_pair()
    for r, t in ((a, b), (pred >= 1, lab >= 1), (pred == 2, lab == 2)):
        assert r.any() and t.any()
        for spacing in (None, (0.7, 0.7, 2.5)):
            ref = m.surface_metrics(r, t, spacing)
            assert ref["msd"] > 0
            assert_surface_close(m.surface_metrics_device(r, t, spacing), ref)
    same = m.surface_metrics_device(a, a, (0.7, 0.7, 2.5))
    assert same == m.surface_metrics(a, a, (0.7, 0.7, 2.5))
    assert same["assd"] == same["msd"] == same["rmsd"] == 0.0 and same["n_rt"] == same["n_tr"] > 0
    # flat uint8 device tensors with their shape
    got = m.surface_metrics_device(dev_u8(a), dev_u8(b), None, shape=a.shape)
    assert_surface_close(got, m.surface_metrics(a, b))


def test_surface_distances_raise_on_empty_masks(emu_lib):
    m = M()
    a, _ = ellipsoid_pair()
    empty = np.zeros(a.shape, bool)
    for r, t in ((empty, a), (a, empty)):
        with pytest.raises(RuntimeError, match="does not contain any binary object"):
            m.surface_distances(r, t)
        with pytest.raises(RuntimeError, match="does not contain any binary object"):
            m.surface_metrics_device(r, t)


def test_evaluate_labels_device(emu_lib):
    m = M()
    pred, lab = synth_label_pair()
    assert (pred == 2).any() and (lab == 2).any()
    for spacing in (None, (0.7, 0.7, 2.5)):
        ref = m.evaluate_labels(pred, lab, spacing)
        got = m.evaluate_labels_device(pred, lab, spacing)
        assert_evaluation_close(got, ref)
        assert 0 < ref["liver"]["dice"] < 1 and ref["liver"]["rvd"] < 0
    same = m.evaluate_labels_device(lab, lab, (0.7, 0.7, 2.5))
    assert_evaluation_close(same, m.evaluate_labels(lab, lab, (0.7, 0.7, 2.5)))
    for s in same.values():
        assert s["dice"] == 1.0 and s["voe"] == 0.0 and s["rvd"] == 0.0 and s["assd"] == s["msd"] == s["rmsd"] == 0.0
    a, b = ellipsoid_pair()
    assert_evaluation_close(m.evaluate_labels_device(a.astype(np.int16) * 2, b.astype(np.int64) * 2), m.evaluate_labels(a * 2, b * 2))


def test_evaluate_labels_empty_structures(emu_lib):
    m = M()
    pred, lab = synth_label_pair()
    no_tumor = np.minimum(lab, 1)
    # tumour missing from the truth: rvd nan, surface fields nan, nothing raised; from both: dice 0
    for p, t in ((pred, no_tumor), (np.minimum(pred, 1), lab), (np.minimum(pred, 1), no_tumor)):
        ref = m.evaluate_labels(p, t)
        got = m.evaluate_labels_device(p, t)
        assert_evaluation_close(got, ref)
        assert all(math.isnan(got["tumor"][k]) for k in m.SURFACE_FIELDS)
        assert not math.isnan(got["liver"]["assd"])
    assert math.isnan(got["tumor"]["rvd"]) and got["tumor"]["dice"] == 0.0
    assert math.isnan(m.evaluate_labels_device(pred, no_tumor)["tumor"]["rvd"])
    assert m.evaluate_labels_device(np.minimum(pred, 1), lab)["tumor"]["rvd"] == -1.0


def test_device_evaluations_are_bit_repeatable(emu_lib):
    m = M()
    pred, lab = synth_label_pair()
    a = m.evaluate_labels_device(pred, lab, (0.7, 0.7, 2.5))
    b = m.evaluate_labels_device(pred, lab, (0.7, 0.7, 2.5))
    assert repr(a) == repr(b)                              # float repr round-trips: equal text = equal bits


def test_scorebook():
    m = M()
    cases = []
    for i, shift in enumerate(((1, -1, 2), (0, 2, 0), (-1, 0, 1))):
        lab = U.pkg("synth").synthetic_ct((23, 17, 13), seed=3 + i)[1].astype(np.uint8)
        pred = shifted(lab, shift)
        if i == 1:
            lab, pred = np.minimum(lab, 1), np.minimum(pred, 1)     # a case without tumour
        cases.append(m.evaluate_labels(pred, lab, (0.7, 0.7, 2.5)))
    book = m.ScoreBook()
    for i, ev in enumerate(cases):
        book.add("case%d" % i, ev)
    s = book.summary()
    assert s["cases"] == 3
    for name in ("liver", "tumor"):
        es = [ev[name] for ev in cases]
        hand = 2.0 * sum(e["n_intersection"] for e in es) / (sum(e["n_result"] for e in es) + sum(e["n_reference"] for e in es))
        assert s[name]["dice_global"] == pytest.approx(hand, rel=1e-15)
        assert s[name]["dice_per_case"] == pytest.approx(np.mean([e["dice"] for e in es]), rel=1e-15)
    assert math.isnan(cases[1]["tumor"]["assd"]) and math.isnan(cases[1]["tumor"]["rvd"])
    for k in ("assd", "rvd", "msd"):
        vals = [cases[i]["tumor"][k] for i in (0, 2)]
        assert not any(math.isnan(v) for v in vals)
        assert s["tumor"][k] == pytest.approx(np.mean(vals), rel=1e-15)
    assert cases[1]["tumor"]["dice"] == 0.0            # MedPy's rule; the case still counts in the per-case mean


def test_refuses_volumes_of_2_32_voxels(emu_lib):
    lib = U.pkg("lib")
    with pytest.raises(lib.HduError, match="2\\^32"):
        lib.check(lib.get().hdu_metric_edt(None, 65536, 65536, 1, None, None, None, None), "hdu_metric_edt")


def test_evaluate_volume_end_to_end(emu_lib):
    """funcs.evaluate_volume on the small float32 hybrid net: segment_volume's labels, evaluate_labels' dictionary"""
    f, m = U.pkg("funcs"), M()
    args = U.make_args(1, 32, 8)
    model = U.pkg("hybridnet").dense_rnn_net(args, dtype="f32", nb_layers2d=(2, 2, 2, 2), nb_layers3d=(1, 1, 2, 1))
    vol, lab = U.pkg("synth").synthetic_ct((32, 32, 12), seed=3)
    mask = (lab > 0).astype(np.int16)
    mask[lab == 2] = 2
    _, mini, maxi = f.liver_window_from_mask(mask)
    s1, s2 = f.predict_tumor_inwindow(model, vol, 3, mini, maxi, args)
    tl, tt = float(np.quantile(s1[s1 > 0], 0.4)), float(np.quantile(s2[s2 > 0], 0.8))
    spacing = (0.7, 0.7, 2.5)
    ref_labels = f.segment_volume(model, vol, mask, args, tl, tt)
    labels, ev = f.evaluate_volume(model, vol, mask, lab, args, spacing, tl, tt)
    assert labels.dtype == np.uint8
    np.testing.assert_array_equal(labels, ref_labels)
    assert_evaluation_close(ev, m.evaluate_labels(ref_labels, lab, spacing))
    assert ev["liver"]["n_result"] > 0


# ------------------------------------------------------------------ MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(515, 24, 1030), (24, 530, 40), (2, 3, 24600), (1100, 3, 5)])
def test_device_edt_long_lines(hip_lib, shape):
    """lines longer than 512 and 1024 (and than the LDS form of pass 1, and than 64 segments of 16 in pass 3) on each axis
    in turn, no axis a multiple of a tile"""
    f = np.random.default_rng(shape[0]).random(shape) < 0.001
    f[shape[0] - 1, 0, shape[2] - 1] = True
    check_edt_unit(f)
    check_edt_spacing(f, (0.7, 0.7, 2.5))


@pytest.mark.gpu
def test_device_evaluation_half_size_phantom(hip_lib):
    """256 x 256 x 48 phantom (liver with a hole, a second blob, tumours inside and outside) against its thresholded noisy
    scores, spacing (0.7, 0.7, 2.5): device == host within the tolerances, two device runs bit-identical"""
    from test_postprocess_device import host_scores, phantom_scores
    m = M()
    shape = (256, 256, 48)
    score, count, truth = phantom_scores(np.random.default_rng(21), shape, 240, 250)
    s1, s2 = host_scores(score, count, shape)
    pred = ((s1 >= 0.5) | (s2 >= 0.9)).astype(np.uint8)
    pred[s2 >= 0.9] = 2
    spacing = (0.7, 0.7, 2.5)
    got = m.evaluate_labels_device(pred, truth, spacing)
    assert repr(m.evaluate_labels_device(pred, truth, spacing)) == repr(got)
    ref = m.evaluate_labels(pred, truth, spacing)
    assert_evaluation_close(got, ref)
    for name in ("liver", "tumor"):
        assert 0 < got[name]["dice"] < 1 and got[name]["msd"] > got[name]["assd"] > 0
