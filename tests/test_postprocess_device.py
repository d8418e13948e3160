"""Device-resident post-processing of the inference (include/hdu.h: hdu_pp_*; funcs.*_device, funcs.segment_volume): every
device result is np.array_equal to the host functions it replaces (funcs.liver_window_from_mask / segment_liver_tumor,
scipy.ndimage), on volumes whose sizes are multiples of no tile, on the x86 emulator build and on the MI355X."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import parity_utils as U

SHAPES = [(23, 17, 13), (40, 9, 31)]
NONE = 0xFFFFFFFF


def F():
    return U.pkg("funcs")


def O():
    return U.pkg("ops")


def dev_u8(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a) != 0).view(np.uint8).reshape(-1)).to(O().device())


def host_roots(binary, conn, background=False):
    """minimum raster index of every voxel's component (ndimage.label), 0xFFFFFFFF off the labelled set"""
    b = (np.asarray(binary) == 0) if background else (np.asarray(binary) != 0)
    lab, n = ndimage.label(b, structure=ndimage.generate_binary_structure(3, 1 if conn == 6 else 3))
    flat = lab.ravel()
    first = np.full(n + 1, NONE, np.uint64)
    idx = np.arange(flat.size, dtype=np.uint64)
    np.minimum.at(first, flat, idx)
    out = first[flat].astype(np.uint32)
    out[flat == 0] = NONE
    return out.reshape(b.shape)


def dev_roots(binary, conn, background=False):
    shape = np.shape(binary)
    root = torch.empty(int(np.prod(shape)), dtype=torch.int32, device=O().device())
    O().pp_label(dev_u8(binary), shape, conn, background, root)
    return root.cpu().numpy().view(np.uint32).reshape(shape)


def dev_largest(binary):
    shape = np.shape(binary)
    ws = F()._PostWorkspace(shape, O().device())
    out = ws.mask()
    n = ws.largest26(dev_u8(binary), out)
    return out.cpu().numpy().reshape(shape), int(n.cpu()[0])


def dev_fill(binary):
    shape = np.shape(binary)
    ws = F()._PostWorkspace(shape, O().device())
    out = ws.mask()
    ws.fill(dev_u8(binary), out)
    return out.cpu().numpy().reshape(shape)


def dev_dilate(binary):
    shape = np.shape(binary)
    out = torch.empty(int(np.prod(shape)), dtype=torch.uint8, device=O().device())
    O().pp_dilate(dev_u8(binary), shape, out)
    return out.cpu().numpy().reshape(shape)


def host_scores(score, count, shape):
    """score [z][deps][rows][num], count [z] as the sweep leaves them -> (score1, score2) exactly as
    predict_tumor_inwindow returns them"""
    z, deps, rows, num = score.shape
    s = score / (count.reshape(z, 1, 1, 1).astype(np.float32) + np.float32(1e-4))
    out = np.zeros(tuple(shape) + (num,), np.float32)
    out[:deps, :rows] = s.transpose(1, 2, 0, 3)
    return out[:, :, :, num - 2], out[:, :, :, num - 1]


def check_components(binary):
    """labels (6 / 26, set / clear voxels), largest component, hole filling and dilation against the host"""
    binary = np.asarray(binary) != 0
    for conn in (6, 26):
        np.testing.assert_array_equal(dev_roots(binary, conn), host_roots(binary, conn))
    np.testing.assert_array_equal(dev_roots(binary, 6, True), host_roots(binary, 6, True))
    if binary.any():
        got, n = dev_largest(binary)
        assert n == ndimage.label(binary, structure=np.ones((3, 3, 3)))[1]
        np.testing.assert_array_equal(got, F()._largest_component(binary.astype(np.uint8)))
    np.testing.assert_array_equal(dev_fill(binary), ndimage.binary_fill_holes(binary).astype(np.uint8))
    np.testing.assert_array_equal(dev_dilate(binary), ndimage.binary_dilation(binary, iterations=1).astype(np.uint8))


def snake(shape):
    """one-voxel-wide boustrophedon path through every (x, z) row of every other y plane, joined at alternating ends"""
    X, Y, Z = shape
    m = np.zeros(shape, bool)
    for y in range(0, Y, 2):
        for x in range(0, X, 2):
            m[x, y, :] = True
            if x + 1 < X:
                zc = Z - 1 if (x // 2) % 2 == 0 else 0
                m[x + 1, y, zc] = True
        if y + 1 < Y:
            m[X - 1 if (X - 1) % 2 == 0 else X - 2, y + 1, 0 if ((X - 1) // 2) % 2 else Z - 1] = True
    return m


def spiral(shape):
    """a square spiral in every x plane, the planes joined at their outer start: long runs along y and z"""
    X, Y, Z = shape
    m = np.zeros(shape, bool)
    for x in range(X):
        y0, y1, z0, z1 = 0, Y - 1, 0, Z - 1
        while y0 <= y1 and z0 <= z1:
            m[x, y0, z0:z1 + 1] = True
            m[x, y0:y1 + 1, z1] = True
            if y1 - y0 >= 2:
                m[x, y1, z0:z1 + 1] = True
            if z1 - z0 >= 2:
                m[x, y0 + 2:y1 + 1, z0] = True
            y0 += 2; y1 -= 2; z0 += 2; z1 -= 2
            if y0 <= y1 and z0 <= z1:
                m[x, y0 - 1, z0] = False      # keep the turns one voxel apart
    return m


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("density", [0.05, 0.3, 0.6, 0.9])
def test_components_random_masks(emu_lib, shape, density):
    rng = np.random.default_rng(int(density * 100) + shape[0])
    check_components(rng.random(shape) < density)


@pytest.mark.parametrize("shape", SHAPES)
def test_components_snakes_and_spirals(emu_lib, shape):
    s = snake(shape)
    assert ndimage.label(s)[1] == 1                 # one long 6-connected path crossing every tile boundary
    check_components(s)
    check_components(spiral(shape))
    check_components(~spiral(shape))


def test_components_diagonal_contacts(emu_lib):
    shape = (23, 17, 13)
    x, y, z = np.indices(shape)
    diag = (x == y) | (x == y + 1) & (z % 2 == 0)
    diag &= ((x + y + z) % 3 != 0)
    corner = np.zeros(shape, bool)
    corner[::2, ::2, ::2] = True
    corner[1::2, 1::2, 1::2] = True                 # a body-centred lattice: 26-connected only through corners
    edge = ((x + y) % 2 == 0) & (z % 3 == 1)        # checkerboard planes: 26- and 18- but not 6-connected
    for m in (diag, corner, edge):
        assert ndimage.label(m, structure=np.ones((3, 3, 3)))[1] < ndimage.label(m)[1]
        check_components(m)


def tie_volume(shape):
    """two equal-area components: A comes first in raster order (smaller x), B first in the sweep's z-major order"""
    m = np.zeros(shape, bool)
    m[1:4, 2:5, 8:11] = True        # A: x 1..3, z 8..10
    m[8:11, 2:5, 1:4] = True        # B: x 8..10, z 1..3
    m[15, 10, 5] = True             # a smaller third one
    return m


def test_largest_tie_is_raster_order(emu_lib):
    m = tie_volume((23, 17, 13))
    got, n = dev_largest(m)
    assert n == 3
    assert got[2, 3, 9] and not got[9, 3, 2]
    np.testing.assert_array_equal(got, F()._largest_component(m.astype(np.uint8)))


def test_fill_holes_each_face(emu_lib):
    shape = (23, 17, 13)
    box = np.zeros(shape, bool)
    box[2:20, 2:15, 2:11] = True
    box[5:8, 5:8, 5:8] = False                      # an enclosed cavity: filled
    base = box.copy()
    check_components(base)
    # a tunnel from the cavity out through each face in turn: the cavity stays open
    tunnels = [(slice(0, 6), 6, 6), (slice(6, 23), 6, 6), (6, slice(0, 6), 6), (6, slice(6, 17), 6),
               (6, 6, slice(0, 6)), (6, 6, slice(6, 13))]
    for t in tunnels:
        m = base.copy()
        m[t] = False
        assert not dev_fill(m)[6, 6, 6]
        check_components(m)
    # a cavity whose wall is the volume's face itself
    m = np.zeros(shape, bool)
    m[0:5, 0:5, 0:5] = True
    m[0, 1:4, 1:4] = False
    check_components(m)


def random_scores(rng, shape, deps, rows, num=3):
    z = shape[2]
    score = rng.random((z, deps, rows, num)).astype(np.float32) * 3
    count = rng.integers(0, 4, z).astype(np.float32)
    score[count == 0] = 0
    return score, count


def dev_threshold(score, count, shape, tl, tt):
    o = O()
    n = int(np.prod(shape))
    liver = torch.empty(n, dtype=torch.uint8, device=o.device())
    tumor = torch.empty(n, dtype=torch.uint8, device=o.device())
    o.pp_threshold(torch.from_numpy(score).to(o.device()), torch.from_numpy(count).to(o.device()), shape, tl, tt, liver, tumor)
    return liver.cpu().numpy().reshape(shape), tumor.cpu().numpy().reshape(shape)


@pytest.mark.parametrize("num", [1, 2, 3])
def test_threshold_matches_host_division_and_compare(emu_lib, num):
    rng = np.random.default_rng(num)
    for shape, deps, rows in (((23, 17, 13), 20, 11), ((40, 9, 31), 40, 9), ((70, 66, 67), 66, 65)):
        score, count = random_scores(rng, shape, deps, rows, num)
        s1, s2 = host_scores(score, count, shape)
        exact = float(s1[s1 > 0.2].flat[7])             # a threshold equal to a score value (float32 -> float64 exactly)
        for tl, tt in ((0.5, 0.9), (exact, float(s2.max())), (0.0, -0.5), (-1.0, 0.0), (0.9, 1e-30)):
            liver, tumor = dev_threshold(score, count, shape, tl, tt)
            r2 = (s2.astype(np.float64) >= tt)
            r1 = (s1.astype(np.float64) >= tl) | r2
            np.testing.assert_array_equal(tumor, r2.astype(np.uint8))
            np.testing.assert_array_equal(liver, r1.astype(np.uint8))


def test_liver_window_from_mask_device(emu_lib):
    rng = np.random.default_rng(5)
    for shape in SHAPES:
        for dtype in (np.int16, np.uint8, np.float64, np.int64):
            coarse = np.zeros(shape, dtype)
            coarse[3:9, 2:7, 4:10] = 1
            coarse[rng.random(shape) < 0.02] = 2
            coarse[shape[0] - 1, shape[1] - 1, shape[2] - 1] = 3
            m, mini, maxi = F().liver_window_from_mask(coarse)
            md, dmini, dmaxi = F().liver_window_from_mask_device(coarse)
            np.testing.assert_array_equal(md.cpu().numpy().reshape(shape), m.astype(np.uint8))
            np.testing.assert_array_equal(dmini, mini)
            np.testing.assert_array_equal(dmaxi, maxi)
    with pytest.raises(ValueError, match="empty liver mask"):
        F().liver_window_from_mask_device(np.zeros((5, 6, 7), np.int16))


def phantom_scores(rng, shape, deps, rows):
    """sweep-layout scores whose thresholds give a large liver with a hole, a second liver blob, tumours inside and outside"""
    X, Y, Z = shape
    x, y, z = np.indices((deps, rows, Z)).astype(np.float32)
    liver = ((x - deps * 0.45) / (deps * 0.3)) ** 2 + ((y - rows * 0.5) / (rows * 0.35)) ** 2 + ((z - Z * 0.5) / (Z * 0.4)) ** 2 < 1
    hole = ((x - deps * 0.45) ** 2 + (y - rows * 0.5) ** 2 + (z - Z * 0.5) ** 2) < 2.5
    blob = ((x - deps * 0.9) ** 2 + (y - rows * 0.1) ** 2 + (z - Z * 0.2) ** 2) < 4
    tum = ((x - deps * 0.4) ** 2 + (y - rows * 0.55) ** 2 + (z - Z * 0.55) ** 2) < 5
    stray = ((x - deps * 0.1) ** 2 + (y - rows * 0.9) ** 2 + (z - Z * 0.8) ** 2) < 3
    count = rng.integers(1, 4, Z).astype(np.float32)
    count[:2] = 0
    s_l = np.clip(0.9 * ((liver & ~hole) | blob) + rng.normal(0, 0.2, liver.shape), 0, 1)
    s_t = np.clip(0.95 * (tum | stray) + rng.normal(0, 0.05, liver.shape), 0, 1)
    score = np.zeros((Z, deps, rows, 3), np.float32)
    score[..., 1] = (s_l * count).transpose(2, 0, 1)
    score[..., 2] = (s_t * count).transpose(2, 0, 1)
    coarse = np.zeros(shape, np.int16)
    coarse[:deps, :rows][liver | blob] = 1
    coarse[:deps, :rows][tum] = 2
    return score, count, coarse


def compare_segment(score, count, coarse, tl, tt):
    f = F()
    shape = coarse.shape
    s1, s2 = host_scores(score, count, shape)
    try:
        ref = f.segment_liver_tumor(s1, s2, f.liver_window_from_mask(coarse)[0], tl, tt)
    except ValueError as e:
        ref = e
    md = f.liver_window_from_mask_device(coarse)[0]
    sd = torch.from_numpy(score).to(O().device())
    if isinstance(ref, ValueError):
        with pytest.raises(ValueError, match="no foreground component"):
            f.segment_liver_tumor_device(sd, count, shape, md, tl, tt)
        return None
    got = f.segment_liver_tumor_device(sd, count, shape, md, tl, tt)
    assert got.dtype == np.uint8 and got.shape == shape
    np.testing.assert_array_equal(got, ref)
    return got


@pytest.mark.parametrize("shape,deps,rows", [((23, 17, 13), 20, 15), ((40, 9, 31), 40, 9)])
def test_segment_liver_tumor_device(emu_lib, shape, deps, rows):
    rng = np.random.default_rng(shape[0])
    score, count, coarse = phantom_scores(rng, shape, deps, rows)
    got = compare_segment(score, count, coarse, 0.5, 0.8)
    assert (got == 1).any() and (got == 2).any()
    s1, _ = host_scores(score, count, shape)
    compare_segment(score, count, coarse, float(s1[s1 > 0.3].flat[3]), 0.9)     # a threshold equal to a score value
    compare_segment(score, count, coarse, 0.0, 0.0)                                # <= 0: the unswept region is marked
    compare_segment(score, count, coarse, -0.25, 0.7)


def test_segment_liver_tumor_device_tie(emu_lib):
    """the two largest liver components have equal areas; raster order and the score layout's z-major order disagree"""
    shape = (23, 17, 13)
    m = tie_volume(shape)
    count = np.ones(shape[2], np.float32)
    score = np.zeros((shape[2], shape[0], shape[1], 3), np.float32)
    score[..., 1] = m.transpose(2, 0, 1) * 0.8
    coarse = m.astype(np.uint8)
    got = compare_segment(score, count, coarse, 0.5, 0.9)
    assert got[2, 3, 9] == 1 and got[9, 3, 2] == 0


def test_segment_liver_tumor_device_empty_raises(emu_lib):
    f = F()
    shape = (23, 17, 13)
    score = np.zeros((13, 23, 17, 3), np.float32)
    count = np.ones(13, np.float32)
    coarse = np.zeros(shape, np.int16)
    coarse[4:8, 4:8, 4:8] = 1
    md = f.liver_window_from_mask_device(coarse)[0]
    with pytest.raises(ValueError, match="no foreground component"):           # no liver above threshold
        f.segment_liver_tumor_device(torch.from_numpy(score), count, shape, md, 0.5, 0.9)
    score[4:6, 4:6, 4:6, 1] = 0.9
    empty = torch.zeros(int(np.prod(shape)), dtype=torch.uint8, device=O().device())
    with pytest.raises(ValueError, match="no foreground component"):           # an empty coarse mask
        f.segment_liver_tumor_device(torch.from_numpy(score), count, shape, empty, 0.5, 0.9)
    compare_segment(score, count, coarse, 0.5, 0.9)


def test_refuses_volumes_of_2_32_voxels(emu_lib):
    lib = U.pkg("lib")
    with pytest.raises(lib.HduError, match="2\\^32"):
        lib.check(lib.get().hdu_pp_dilate(None, 65536, 65536, 1, None, None), "hdu_pp_dilate")
    with pytest.raises(ValueError):
        F()._check_volume((65536, 65536, 1))


def _host_composition(f, model, vol, mask, args, tl, tt):
    m, mini, maxi = f.liver_window_from_mask(mask)
    try:
        return f.segment_liver_tumor(*f.predict_tumor_inwindow(model, vol, 3, mini, maxi, args), m, tl, tt)
    except ValueError as e:
        return e


def test_segment_volume_end_to_end(emu_lib):
    """segment_volume (sweep + post-processing in HBM) against the host composition of test.py on the small hybrid net"""
    f = F()
    args = U.make_args(1, 32, 8)
    model = U.pkg("hybridnet").dense_rnn_net(args, dtype="f32", nb_layers2d=(2, 2, 2, 2), nb_layers3d=(1, 1, 2, 1))
    vol, lab = U.pkg("synth").synthetic_ct((32, 32, 12), seed=3)
    mask = (lab > 0).astype(np.int16)
    mask[lab == 2] = 2
    m, mini, maxi = f.liver_window_from_mask(mask)
    s1, s2 = f.predict_tumor_inwindow(model, vol, 3, mini, maxi, args)
    swept = s1[s1 > 0]
    tl, tt = float(np.quantile(swept, 0.4)), float(np.quantile(s2[s2 > 0], 0.8))
    for thresholds in ((tl, tt), (0.5, 0.9)):
        ref = _host_composition(f, model, vol, mask, args, *thresholds)
        if isinstance(ref, ValueError):
            with pytest.raises(ValueError):
                f.segment_volume(model, vol, mask, args, *thresholds)
            continue
        got = f.segment_volume(model, vol, mask, args, *thresholds)
        np.testing.assert_array_equal(got, ref)
        if thresholds == (tl, tt):
            assert (got == 1).any() and (got == 2).any()


# ------------------------------------------------------------------ MI355X
@pytest.mark.gpu
def test_device_postprocess_full_size(hip_lib):
    """512 x 512 x 96 phantom with noise, several components, holes and a stray tumour response: device == host"""
    f = F()
    shape = (512, 512, 96)
    rng = np.random.default_rng(11)
    score, count, coarse = phantom_scores(rng, shape, 480, 500)
    m, mini, maxi = f.liver_window_from_mask(coarse)
    md, dmini, dmaxi = f.liver_window_from_mask_device(coarse)
    np.testing.assert_array_equal(md.cpu().numpy().reshape(shape), m.astype(np.uint8))
    np.testing.assert_array_equal(dmini, mini)
    np.testing.assert_array_equal(dmaxi, maxi)
    got = compare_segment(score, count, coarse, 0.5, 0.8)
    assert (got == 1).any() and (got == 2).any()
    compare_segment(score, count, coarse, 0.0, 0.9)


@pytest.mark.gpu
def test_device_components_full_size(hip_lib):
    """labels, largest component (with a size tie between the two largest), hole filling at 512 x 512 x 96"""
    shape = (512, 512, 96)
    rng = np.random.default_rng(12)
    noise = rng.random(shape) < 0.3
    for conn in (6, 26):
        np.testing.assert_array_equal(dev_roots(noise, conn), host_roots(noise, conn))
    m = np.zeros(shape, bool)
    m[10:60, 20:70, 40:80] = True                    # A: first in raster order
    m[300:350, 20:70, 2:42] = True                   # B: same area, first in z-major order
    m[100:110, 400:410, 5:15] = True
    m[30:40, 40:50, 55:65] = False                   # a cavity inside A ...
    m[320:330, 40:50, 17:27] = False                 # ... and one inside B: the areas stay equal
    m[400:] |= rng.random((112,) + shape[1:]) < 0.001   # scattered small components away from both
    lab, _ = ndimage.label(m, structure=np.ones((3, 3, 3)))
    assert (lab == lab[20, 30, 50]).sum() == (lab == lab[310, 30, 10]).sum()
    got, n = dev_largest(m)
    ref = F()._largest_component(m.astype(np.uint8))
    np.testing.assert_array_equal(got, ref)
    assert got[20, 30, 50] == 1 and got[310, 30, 10] == 0
    np.testing.assert_array_equal(dev_fill(m), ndimage.binary_fill_holes(m).astype(np.uint8))


@pytest.mark.gpu
def test_device_labels_repeatable(hip_lib):
    """roots are minimum raster indices, so two runs of the label kernels on one input are identical"""
    shape = (512, 512, 96)
    rng = np.random.default_rng(13)
    m = rng.random(shape) < 0.45
    a = dev_roots(m, 26)
    b = dev_roots(m, 26)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(dev_roots(m, 6, True), dev_roots(m, 6, True))


@pytest.mark.gpu
def test_segment_volume_full_size(hip_lib):
    """segment_volume on the full-size float32 dense_rnn_net (224 x 224 x 12 windows over a 224 x 224 x 40 phantom) against
    the host composition segment_liver_tumor(*predict_tumor_inwindow(...), liver_window_from_mask(mask)[0], ...)"""
    f = F()
    args = U.make_args(1, 224, 12)
    m, _, _ = U.build_pair("hybrid", "end2end", 1, 224, 12, "f32", (6, 12, 36, 24), (3, 4, 12, 8),
                           odtype=torch.float32, perturb=False)
    vol, lab = U.pkg("synth").synthetic_ct((224, 224, 40), seed=3)
    mask = lab.astype(np.int16)
    mw, mini, maxi = f.liver_window_from_mask(mask)
    s1, s2 = f.predict_tumor_inwindow(m, vol, 3, mini, maxi, args)
    tl, tt = float(np.quantile(s1[s1 > 0], 0.5)), float(np.quantile(s2[s2 > 0], 0.9))
    ref = f.segment_liver_tumor(s1, s2, mw, tl, tt)
    got = f.segment_volume(m, vol, mask, args, tl, tt)
    np.testing.assert_array_equal(got, ref)
    assert (got == 1).any() and (got == 2).any()
