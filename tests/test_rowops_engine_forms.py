"""The pool / resample / loss / SGD / plumbing kernels of rowops.hip in the forms the engine launches them in
(engine.py, models.py, shard.py), against float64 torch / numpy restatements (oracle/np64.py):

 1. every activation operand a channel slab of a wider, poisoned buffer with its own pixel stride, overwrite and
    accumulate (read-modify-write into a pre-loaded gradient slab);
 2. geometry edges: odd planes under the 2 x 2 average pool, signed inputs / all-negative windows / D = 2, 3 / several
    volumes under the 3 x 3 (x 3) max pool, the depth-halo mode (pad_d = 0) on slabs;
 3. sizes past the grid cap (8192 / 4096 / 2048 blocks of 256), where the grid-stride loops run a second, partial pass;
 4. the loss as LossLayer calls it (row ranges, += into shared sums, loss-only form, labels above 2, saturation in both
    directions) and Nesterov SGD with a gradient scale, two steps.

Like tests/test_kernels.py every test runs under the x86 emulator build and, marked `gpu`, on the gfx950 library (the
past-the-cap cases take about a second each under the emulator, so none is marked `slow`)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import np64 as N64
from test_kernels import BF16, F32, DT, rnd, q, tol, assert_close, mkact, dev, ops_mod

C24 = 24                       # 3 bf16 chunks / 6 f32 chunks per pixel: q % ncc takes every residue
WEIGHTS = (0.78, 0.65, 8.57)


def assert_poison_intact(a, what):
    """every channel of the wide buffer outside the slab `a` still holds mkact's 7.0, in every row"""
    full = a.buf.float().cpu().reshape(-1, a.ld)
    assert full.shape[0] == a.M and 0 < a.off and a.off + a.C <= a.ld
    outside = torch.cat([full[:, :a.off], full[:, a.off + a.C:]], 1)
    assert outside.numel() > 0 and bool((outside == 7.0).all()), "%s: channels outside the slab were written" % what


def got64(a):
    return a.to_torch().cpu().double()


def check_backward_forms(ops, run, grad, dtype, ld, coff, what, operands=()):
    """run(target, accumulate): overwrite over stale values, then accumulate into a pre-loaded slab; the neighbouring
    channels of the target and of every operand stay poisoned"""
    dims = tuple(grad.shape)
    tgt = mkact(ops, torch.full(dims, 3.0, dtype=torch.float64), dtype, ld, coff)
    run(tgt, False)
    assert_close(got64(tgt), grad, dtype, what=what + " overwrite")
    assert_poison_intact(tgt, what + " overwrite")
    g0 = rnd(dims, 11, float(grad.abs().max()), dtype)     # as large as the gradient: a dropped += is far outside tol(dtype)
    tgt = mkact(ops, g0, dtype, ld, coff)
    run(tgt, True)
    assert_close(got64(tgt), q(g0 + grad, dtype), dtype, what=what + " accumulate")
    assert_poison_intact(tgt, what + " accumulate")
    for o in operands:
        assert_poison_intact(o, what + " operand")
    return g0, tgt


# ---------------------------------------------------------------------------------------------------- max pool inputs
def pool_windows(dims, pad_d):
    """(od, oh, ow, depth slice, row slice, column slice, interior?) of every 3 x 3 (x 3), stride 2 window"""
    _, D, H, W, _ = dims
    Do = 1 if D == 1 else (D + 2 * pad_d - 3) // 2 + 1
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = []
    for od in range(Do):
        d0, d1 = (0, 1) if D == 1 else (2 * od - pad_d, 2 * od - pad_d + 3)
        for oh in range(Ho):
            for ow in range(Wo):
                h0, w0 = 2 * oh - 1, 2 * ow - 1
                interior = d0 >= 0 and d1 <= D and h0 >= 0 and h0 + 3 <= H and w0 >= 0 and w0 + 3 <= W
                out.append((od, oh, ow, slice(max(d0, 0), min(d1, D)), slice(max(h0, 0), min(h0 + 3, H)),
                            slice(max(w0, 0), min(w0 + 3, W)), interior))
    return (Do, Ho, Wo), out


def signed_no_ties(dims, seed, pad_d=1):
    """values in [-1, 1], no zeros, no ties: within one volume and channel the magnitudes are a random permutation of
    k / 256 (k = 1 .. D*H*W <= 255, exact in bf16 and f32; a random dither cannot keep bf16 values apart), so whichever signs
    they carry no two elements of a window are equal.  The first border window and, where the geometry has one, the last
    interior window are then made negative in every channel."""
    N, D, H, W, C = dims
    P = D * H * W
    assert P <= 255
    g = torch.Generator().manual_seed(seed)
    mag = torch.stack([torch.randperm(P, generator=g) for _ in range(N * C)]).double().add(1).div(256)
    mag = mag.reshape(N, C, D, H, W).permute(0, 2, 3, 4, 1)
    sign = (torch.rand(dims, generator=g, dtype=torch.float64) < 0.5).double() * 2 - 1
    x = (mag * sign).contiguous()
    _, wins = pool_windows(dims, pad_d)
    border = [w for w in wins if not w[6]]
    inner = [w for w in wins if w[6]]
    for w in border[:1] + inner[-1:]:
        x[:, w[3], w[4], w[5]] = -x[:, w[3], w[4], w[5]].abs()
    return x


def check_signed_input(x, yr, pad_d):
    """the properties the signed max-pool tests rest on, asserted on the generated input itself"""
    dims = tuple(x.shape)
    _, wins = pool_windows(dims, pad_d)
    assert float(x.abs().min()) > 0 and float(x.abs().max()) <= 1.0
    neg_border = neg_inner = 0
    for od, oh, ow, ds, hs, ws, interior in wins:
        v = x[:, ds, hs, ws].reshape(dims[0], -1, dims[4])
        s = v.sort(1).values
        assert bool((s[:, 1:] > s[:, :-1]).all()), "tie inside a window"
        allneg = bool((v < 0).all())
        if allneg and interior:
            neg_inner += 1
            assert bool((yr[:, od, oh, ow] < 0).all())           # no padding in the window: a negative maximum
        if allneg and not interior:
            neg_border += 1
            assert bool((yr[:, od, oh, ow] == 0).all())          # the zero padding wins
    assert neg_border >= 1, "no all-negative border window"
    if any(w[6] for w in wins):
        assert neg_inner >= 1, "no all-negative interior window"
    return neg_border, neg_inner


def ref_maxpool(x, pad_d=1):
    """float64 F.max_pool on the explicitly zero-padded input; returns (leaf, output) for autograd"""
    xr = x.clone().requires_grad_(True)
    xp = xr.permute(0, 4, 1, 2, 3)
    if x.shape[1] == 1:
        yr = F.max_pool2d(F.pad(xp[:, :, 0], (1, 1, 1, 1)), 3, 2)[:, :, None]
    else:
        yr = F.max_pool3d(F.pad(xp, (1, 1, 1, 1, pad_d, pad_d)), 3, 2)
    return xr, yr.permute(0, 2, 3, 4, 1)


def run_maxpool_case(ops, dims, dtype, pad_d, slabs):
    """forward (exact) + argmax, backward overwrite and accumulate everywhere, on dense operands or on four slabs with
    four different strides"""
    N, D, H, W, C = dims
    x = signed_no_ties(dims, 3, pad_d)
    assert bool((q(x, dtype) == x).all())
    xr, yr = ref_maxpool(x, pad_d)
    (Do, Ho, Wo), _ = pool_windows(dims, pad_d)
    odims = (N, Do, Ho, Wo, C)
    assert tuple(yr.shape) == odims
    check_signed_input(x, yr.detach(), pad_d)
    ld = dict(x=(40, 8), y=(56, 16), dy=(48, 8), dx=(64, 32)) if slabs else dict(x=(None, 0), y=(None, 0), dy=(None, 0), dx=(None, 0))
    xa = mkact(ops, x, dtype, *ld["x"])
    y = mkact(ops, torch.full(odims, 3.0, dtype=torch.float64), dtype, *ld["y"])
    amax = torch.full((N * Do * Ho * Wo * C,), 99, dtype=torch.uint8, device=ops.device())   # dense whatever ld(y) is
    ops.maxpool_fwd(xa, y, amax, pad_d=pad_d)
    assert float((got64(y) - yr.detach()).abs().max()) == 0.0
    am = amax.cpu().reshape(odims)
    assert bool(((am < 27) | (am == 255)).all())
    assert bool(((am == 255) == (yr.detach() == 0)).all())       # 255 = the padding won, nowhere else
    dy = rnd(odims, 5, 1.0, dtype)
    (yr * dy).sum().backward()
    grad = xr.grad
    dya = mkact(ops, dy, dtype, *ld["dy"])
    if slabs:
        for a in (xa, y):
            assert_poison_intact(a, "maxpool fwd")
        check_backward_forms(ops, lambda t, acc: ops.maxpool_bwd(amax, dya, t, acc, pad_d), grad, dtype, *ld["dx"],
                             what="maxpool bwd", operands=(dya,))
    else:
        dx = mkact(ops, torch.full(dims, 3.0, dtype=torch.float64), dtype)
        ops.maxpool_bwd(amax, dya, dx, False, pad_d)
        got = got64(dx)
        assert_close(got, grad, dtype, what="maxpool bwd")
        # exactly no gradient wherever the element is not a window's maximum, the all-negative border windows included
        assert bool((grad == 0).any()) and float(got[grad == 0].abs().max()) == 0.0
    return x, grad


# ==================================================================================== 1. slab and accumulate forms
@pytest.mark.parametrize("dtype", DT)
def test_maxpool_slabs_accumulate(hdu, dtype):
    """x, y, dy and dx are slabs with strides 40 / 56 / 48 / 64; the argmax stays dense (opix * C)"""
    run_maxpool_case(ops_mod(), (2, 5, 5, 6, C24), dtype, 1, slabs=True)


@pytest.mark.parametrize("dtype", DT)
def test_maxpool_depth_halo_slabs(hdu, dtype):
    """pad_d = 0 (the neighbouring depth planes are stored): two volumes, slab operands, against F.max_pool3d padded in H
    and W only"""
    run_maxpool_case(ops_mod(), (2, 6, 5, 6, C24), dtype, 0, slabs=True)


@pytest.mark.parametrize("dtype", DT)
def test_avgpool_slabs_accumulate(hdu, dtype):
    ops = ops_mod()
    N, D, H, W = 2, 2, 6, 4
    x = rnd((N, D, H, W, C24), 3, 1.0, dtype)
    xa = mkact(ops, x, dtype, 40, 8)
    odims = (N, D, H // 2, W // 2, C24)
    y = mkact(ops, torch.full(odims, 3.0, dtype=torch.float64), dtype, 56, 16)
    ops.avgpool_fwd(xa, y)
    assert_close(got64(y), torch.tensor(N64.avg_pool(x.numpy(), (1, 2, 2))), dtype, what="avgpool fwd")
    for a in (xa, y):
        assert_poison_intact(a, "avgpool fwd")
    dy = rnd(odims, 4, 1.0, dtype)
    dya = mkact(ops, dy, dtype, 48, 8)
    grad = dy.repeat_interleave(2, 2).repeat_interleave(2, 3) * 0.25
    check_backward_forms(ops, lambda t, acc: ops.avgpool_bwd(dya, t, acc), grad, dtype, 64, 32, "avgpool bwd", (dya,))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("up", [(0, 0, 0), (0, 1, 1), (1, 1, 1)], ids=["add", "up2d", "up3d"])
def test_upsample_bwd_slabs_accumulate(hdu, dtype, up):
    """up = (0, 0, 0) is the engine's strided "add this gradient into that slab" kernel (ConvLayer.backward,
    shard.halo_reduce)"""
    ops = ops_mod()
    N, D, H, W = 2, 2, 3, 5
    g = rnd((N, D << up[0], H << up[1], W << up[2], C24), 5, 1.0, dtype)
    ga = mkact(ops, g, dtype, 48, 8)
    grad = g.reshape(N, D, 1 << up[0], H, 1 << up[1], W, 1 << up[2], C24).sum((2, 4, 6))
    check_backward_forms(ops, lambda t, acc: ops.upsample_bwd(ga, t, up, acc), grad, dtype, 64, 32, "upsample bwd", (ga,))


@pytest.mark.parametrize("dtype", DT)
def test_make_input3d_bwd_slabs_accumulate(hdu, dtype):
    """d(logits2d)[:, 0:3] (+)= scale * d(input3d)[:, 1:4]; the pad channels 3 .. C-1 are zeroed when overwriting and left
    alone when accumulating"""
    ops = ops_mod()
    D, H, W = 3, 4, 5
    din = rnd((1, D, H, W, C24), 3, 1.0, dtype)
    dina = mkact(ops, din, dtype, 40, 8)
    grad = torch.zeros((1, D, H, W, C24), dtype=torch.float64)
    grad[..., :3] = din[..., 1:4] * 250.0
    g0, tgt = check_backward_forms(ops, lambda t, acc: ops.make_input3d_bwd(dina, 250.0, t, acc), grad, dtype, 56, 16,
                                   "make_input3d bwd", (dina,))
    assert float((got64(tgt)[..., 3:] - g0[..., 3:]).abs().max()) == 0.0


# ============================================================================================== 2. geometry edges
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("hw", [(7, 6), (8, 5), (5, 5)], ids=lambda v: "%dx%d" % v)
def test_avgpool_odd_planes(hdu, dtype, hw):
    """an odd last row / column is dropped forward and gets exactly no gradient backward"""
    ops = ops_mod()
    N, D, (H, W), C = 2, 2, hw, 8
    Ho, Wo = H // 2, W // 2
    x = rnd((N, D, H, W, C), 3, 1.0, dtype)
    y = mkact(ops, torch.full((N, D, Ho, Wo, C), 3.0, dtype=torch.float64), dtype)
    ops.avgpool_fwd(mkact(ops, x, dtype), y)
    assert_close(got64(y), torch.tensor(N64.avg_pool(x.numpy(), (1, 2, 2))), dtype, what="avgpool fwd")
    dy = rnd((N, D, Ho, Wo, C), 4, 1.0, dtype)
    dya = mkact(ops, dy, dtype)
    grad = torch.zeros((N, D, H, W, C), dtype=torch.float64)
    grad[:, :, :2 * Ho, :2 * Wo] = dy.repeat_interleave(2, 2).repeat_interleave(2, 3) * 0.25
    dx = mkact(ops, torch.full((N, D, H, W, C), 3.0, dtype=torch.float64), dtype)
    ops.avgpool_bwd(dya, dx)
    got = got64(dx)
    assert float(got[:, :, 2 * Ho:].abs().max() if H % 2 else 0.0) == 0.0
    assert float(got[:, :, :, 2 * Wo:].abs().max() if W % 2 else 0.0) == 0.0
    assert_close(got, grad, dtype, what="avgpool bwd")
    g0 = rnd((N, D, H, W, C), 11, 1.0, dtype)
    dx = mkact(ops, g0, dtype)
    ops.avgpool_bwd(dya, dx, accumulate=True)
    got = got64(dx)
    assert float((got - g0)[:, :, 2 * Ho:].abs().max() if H % 2 else 0.0) == 0.0      # the dropped row keeps its gradient
    assert float((got - g0)[:, :, :, 2 * Wo:].abs().max() if W % 2 else 0.0) == 0.0
    assert_close(got, q(g0 + grad, dtype), dtype, what="avgpool bwd accumulate")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("dims", [(2, 2, 6, 7, 8), (1, 3, 5, 5, 8), (2, 1, 4, 9, 16)], ids=lambda d: "x".join(map(str, d)))
def test_maxpool_signed_input(hdu, dtype, dims):
    """signed input without ties: all-negative windows in the interior (a negative maximum) and at the border (the zero
    padding wins: output 0, no gradient), D = 2 / 3 and two volumes; the gradient is compared everywhere"""
    ops = ops_mod()
    x, grad = run_maxpool_case(ops, dims, dtype, 1, slabs=False)
    _, wins = pool_windows(dims, 1)
    # the corner element belongs to the first (all-negative, padded) window alone: the padding took its gradient
    od, oh, ow, ds, hs, ws, _ = [w for w in wins if not w[6]][0]
    assert (od, oh, ow) == (0, 0, 0) and bool((x[:, ds, hs, ws] < 0).all()) and float(grad[:, 0, 0, 0].abs().max()) == 0.0


# ===================================================================== 3. second pass of the grid-stride loops
POOL_CAP, ROW_CAP, LOSS_CAP = 8192 * 256, 4096 * 256, 2048 * 256
BIG_PLANE = 1449                    # 1449^2 = 2,099,601 pixels = POOL_CAP + 2449: one chunk per pixel, a partial second pass


def dense_act(ops, dims, dtype, values):
    """dense activation filled through its flat buffer (Act.from_torch builds an index per element)"""
    a = ops.Act.alloc(*dims, dtype)
    a.buf.copy_(values.reshape(-1).to(a.buf.dtype))
    return a


def dense64(a):
    return a.buf.float().cpu().reshape(a.N, a.D, a.H, a.W, a.C).double()


def rand_storage(shape, seed, dtype):
    """uniform [-1, 1) values exact in the storage dtype, as float64"""
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1
    return (t.to(torch.bfloat16) if dtype == BF16 else t).double()


def assert_whole(got, ref, dtype, cap_rows, what):
    """the whole tensor; the rows around the end of the first grid pass are named separately for the failure message"""
    g2, r2 = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    s = float(ref.abs().max())
    assert_close(g2[:1000], r2[:1000], dtype, scale=s, what=what + " (first rows)")
    assert_close(g2[cap_rows - 8:cap_rows + 8], r2[cap_rows - 8:cap_rows + 8], dtype, scale=s, what=what + " (rows around the end of the first pass)")
    assert_close(g2[-1000:], r2[-1000:], dtype, scale=s, what=what + " (last rows)")
    assert_close(g2, r2, dtype, scale=s, what=what)


def test_second_pass_avgpool_bwd(hdu):
    ops = ops_mod()
    dtype, C, H = BF16, 8, BIG_PLANE
    assert H * H * (C // 8) > POOL_CAP and (H * H) % 256
    dy = rand_storage((1, 1, H // 2, H // 2, C), 4, dtype)
    dx = dense_act(ops, (1, 1, H, H, C), dtype, torch.full((H * H * C,), 3.0))
    ops.avgpool_bwd(dense_act(ops, tuple(dy.shape), dtype, dy), dx)
    grad = torch.zeros((1, 1, H, H, C), dtype=torch.float64)
    grad[:, :, :H - 1, :H - 1] = dy.repeat_interleave(2, 2).repeat_interleave(2, 3) * 0.25
    assert_whole(dense64(dx), grad, dtype, POOL_CAP, "avgpool bwd past the grid cap")


def test_second_pass_avgpool_fwd(hdu):
    ops = ops_mod()
    dtype, C, H = F32, 4, 2 * BIG_PLANE + 1
    x = rand_storage((1, 1, H, H, C), 3, dtype)
    y = dense_act(ops, (1, 1, BIG_PLANE, BIG_PLANE, C), dtype, torch.full((BIG_PLANE * BIG_PLANE * C,), 3.0))
    ops.avgpool_fwd(dense_act(ops, tuple(x.shape), dtype, x), y)
    ref = x[:, :, :H - 1, :H - 1].reshape(1, 1, BIG_PLANE, 2, BIG_PLANE, 2, C).mean((3, 5))
    assert_whole(dense64(y), ref, dtype, POOL_CAP, "avgpool fwd past the grid cap")


def test_second_pass_upsample_bwd_accumulate(hdu):
    ops = ops_mod()
    dtype, C, H = BF16, 8, BIG_PLANE
    g = rand_storage((1, 1, H, H, C), 5, dtype)
    g0 = rand_storage((1, 1, H, H, C), 11, dtype)
    dz = dense_act(ops, tuple(g0.shape), dtype, g0)
    ops.upsample_bwd(dense_act(ops, tuple(g.shape), dtype, g), dz, (0, 0, 0), accumulate=True)
    assert_whole(dense64(dz), q(g0 + g, dtype), dtype, POOL_CAP, "upsample bwd (add) past the grid cap")


def hashed_signed_plane(H, C, bits, seed):
    """[1, 1, H, H, C] signed f32-exact values whose magnitudes (hash(pixel) + 1) / 2^bits, an odd multiplier mod 2^bits >
    H * H, are pairwise distinct within a channel: no ties and no zeros"""
    P = H * H
    assert P < (1 << bits) and bits <= 24
    pix = torch.arange(P, dtype=torch.int64)[:, None]
    mag = ((pix * 2654435761 + torch.arange(C, dtype=torch.int64)[None, :] * 977) % (1 << bits) + 1).double() / (1 << bits)
    g = torch.Generator().manual_seed(seed)
    x = (mag * ((torch.rand((P, C), generator=g) < 0.5).double() * 2 - 1)).reshape(1, 1, H, H, C)
    assert bool((x.float().double() == x).all())
    return x


def test_second_pass_maxpool_fwd(hdu):
    """f32, C = 4: 1449^2 output pixels (a 2897^2 plane in)"""
    ops = ops_mod()
    dtype, C, Ho = F32, 4, BIG_PLANE
    H = 2 * Ho - 1
    x = hashed_signed_plane(H, C, 24, 3)
    with torch.no_grad():
        yr = ref_maxpool(x)[1]
    y = dense_act(ops, (1, 1, Ho, Ho, C), dtype, torch.full((Ho * Ho * C,), 3.0))
    amax = torch.full((Ho * Ho * C,), 99, dtype=torch.uint8, device=ops.device())
    ops.maxpool_fwd(dense_act(ops, tuple(x.shape), dtype, x), y, amax)
    got = dense64(y)
    assert float((got - yr).abs().max()) == 0.0, "first bad output pixel %d" % int((got != yr).reshape(-1, C).any(1).int().argmax())
    am = amax.cpu().reshape(1, 1, Ho, Ho, C)
    assert bool(((am == 255) == (yr == 0)).all()) and bool(((am < 9) | (am == 255)).all())


def test_second_pass_maxpool_bwd(hdu):
    """f32, C = 4: the backward kernel walks 1449^2 input pixels"""
    ops = ops_mod()
    dtype, C, H = F32, 4, BIG_PLANE
    P = H * H
    x = hashed_signed_plane(H, C, 22, 3)
    Ho = (H - 1) // 2 + 1
    xr, yr = ref_maxpool(x)
    y = dense_act(ops, (1, 1, Ho, Ho, C), dtype, torch.full((Ho * Ho * C,), 3.0))
    amax = torch.full((Ho * Ho * C,), 99, dtype=torch.uint8, device=ops.device())
    ops.maxpool_fwd(dense_act(ops, tuple(x.shape), dtype, x), y, amax)
    assert float((dense64(y) - yr.detach()).abs().max()) == 0.0
    dy = rand_storage((1, 1, Ho, Ho, C), 5, dtype)
    (yr * dy).sum().backward()
    dx = dense_act(ops, tuple(x.shape), dtype, torch.full((P * C,), 3.0))
    ops.maxpool_bwd(amax, dense_act(ops, tuple(dy.shape), dtype, dy), dx)
    assert_whole(dense64(dx), xr.grad, dtype, POOL_CAP, "maxpool bwd past the grid cap")


PLUMB_D, PLUMB_H, PLUMB_W = 3, 600, 583     # 1,049,400 voxels = ROW_CAP + 824


@pytest.mark.parametrize("dtype", DT)
def test_second_pass_plumbing(hdu, dtype):
    """slab25d, make_input3d and make_input3d_bwd over more voxels than 4096 blocks of 256 cover"""
    ops = ops_mod()
    D, H, W = PLUMB_D, PLUMB_H, PLUMB_W
    M = D * H * W
    assert M > ROW_CAP and M % 256
    Cp = 8 if dtype == BF16 else 4
    g = torch.Generator().manual_seed(1)
    vol = (torch.rand((D, H, W), generator=g) * 200 - 100).float()
    out = dense_act(ops, (D, 1, H, W, Cp), dtype, torch.full((M * Cp,), 3.0))
    ops.slab25d(vol.to(ops.device()), D, H, W, out)
    ref = torch.zeros((D, 1, H, W, Cp), dtype=torch.float64)
    for k in range(D):
        for j, kk in enumerate((max(k - 1, 0), k, min(k + 1, D - 1))):
            ref[k, 0, :, :, j] = vol[kk].double()
    assert_whole(dense64(out), q(ref, dtype), dtype, ROW_CAP, "slab25d past the grid cap")
    lg = rand_storage((1, D, H, W, Cp), 2, dtype) * 3
    lg[..., 3:] = 0
    lg = q(lg, dtype)
    i3 = dense_act(ops, (1, D, H, W, Cp), dtype, torch.full((M * Cp,), 3.0))
    ops.make_input3d(vol.to(ops.device()), dense_act(ops, tuple(lg.shape), dtype, lg), 250.0, i3)
    ref = torch.zeros((1, D, H, W, Cp), dtype=torch.float64)
    ref[0, ..., 0] = vol.double()
    ref[0, ..., 1:4] = lg[0, ..., :3] * 250
    assert_whole(dense64(i3), q(ref, dtype), dtype, ROW_CAP, "make_input3d past the grid cap")
    din = rand_storage((1, D, H, W, Cp), 3, dtype)
    dl = dense_act(ops, (1, D, H, W, Cp), dtype, torch.full((M * Cp,), 3.0))
    ops.make_input3d_bwd(dense_act(ops, tuple(din.shape), dtype, din), 250.0, dl)
    ref = torch.zeros((1, D, H, W, Cp), dtype=torch.float64)
    ref[..., :3] = din[..., 1:4] * 250
    assert_whole(dense64(dl), ref, dtype, ROW_CAP, "make_input3d bwd past the grid cap")


@pytest.mark.parametrize("dtype", DT)
def test_second_pass_casts_softmax(hdu, dtype):
    """cast_pad / cast_out over M * C elements and softmax_accumulate over M rows past 4096 blocks of 256"""
    ops = ops_mod()
    Cp = 8 if dtype == BF16 else 4
    M = 350003
    assert M * 3 > ROW_CAP and (M * 3) % 256 and (M * Cp) % 256
    g = torch.Generator().manual_seed(4)
    src = (torch.rand((M, 3), generator=g) * 10 - 5).float()
    a = dense_act(ops, (1, 1, 1, M, Cp), dtype, torch.full((M * Cp,), 3.0))
    ops.cast_pad(src.to(ops.device()), M, 3, a)
    ref = torch.zeros((M, Cp), dtype=torch.float64)
    ref[:, :3] = q(src.double(), dtype)
    assert_whole(dense64(a).reshape(M, Cp), ref, dtype, ROW_CAP // Cp, "cast_pad past the grid cap")
    back = torch.full((M, 3), 3.0, device=ops.device())
    ops.cast_out(a, 3, back)
    assert float((back.cpu().double() - ref[:, :3]).abs().max()) == 0.0          # widening the stored value is exact
    M2 = ROW_CAP + 77
    lg = q(rand_storage((1, 1, 1, M2, Cp), 5, dtype) * 3, dtype)
    score0 = rand_storage((M2, 3), 6, F32).float()
    score = score0.clone().to(ops.device()).reshape(-1)
    ops.softmax_accumulate(dense_act(ops, tuple(lg.shape), dtype, lg), 0, M2, 3, score)
    ref = score0.double() + torch.tensor(N64.softmax(lg.reshape(M2, Cp)[:, :3].numpy()))
    err = (score.cpu().double().reshape(M2, 3) - ref).abs()
    assert float(err.max()) < 2e-6, "softmax_accumulate past the grid cap: first bad row %d" % int(err.max(1).values.argmax())


def test_second_pass_sgd(hdu):
    ops = ops_mod()
    n = ROW_CAP + 77
    p0, v0, g = (rand_storage((n,), s, F32).numpy() for s in (1, 2, 3))
    p, v, gr = (torch.tensor(a, dtype=torch.float32, device=ops.device()) for a in (p0, v0, g))
    ops.sgd_nesterov(p, v, gr, 1e-3, 0.9, 1.0 / 7)
    pn, vn = N64.sgd_nesterov(p0, v0, g * (1.0 / 7), 1e-3, 0.9)
    np.testing.assert_allclose(p.cpu().numpy(), pn, rtol=2e-6, atol=2e-7)
    np.testing.assert_allclose(v.cpu().numpy(), vn, rtol=2e-6, atol=2e-7)
    assert float((gr.cpu().double() - torch.tensor(g)).abs().max()) == 0.0


def wce_reference(z, lab, gs):
    """np64.weighted_crossentropy over the rows labelled 0..2, rescaled from its 1/rows to (loss sum, gs * gradient);
    rows labelled above 2 (the one-hot of depth 3 is all zero there): no loss, no gradient, no count"""
    z, lab = np.asarray(z, dtype=np.float64), np.asarray(lab)
    ok = lab <= 2
    loss, grad_ok = N64.weighted_crossentropy(z[ok], lab[ok], WEIGHTS)
    n = int(ok.sum())
    grad = np.zeros_like(z)
    grad[ok] = grad_ok * n * gs
    return loss * n, grad, [float((lab == i).sum()) for i in range(3)]


@pytest.mark.parametrize("dtype", DT)
def test_second_pass_wce_loss(hdu, dtype):
    """more rows than 2048 blocks of 256: the loss kernel's loop runs twice and the finalize walks all 2048 partials"""
    ops = ops_mod()
    M = LOSS_CAP + 301
    Cp = 8 if dtype == BF16 else 4
    z = rand_storage((M, 3), 3, dtype) * 6
    z = q(z, dtype)
    g = torch.Generator().manual_seed(5)
    lab = torch.randint(0, 3, (M,), generator=g)
    zz = torch.zeros((1, 1, 1, M, Cp), dtype=torch.float64)
    zz[0, 0, 0, :, :3] = z
    dl = dense_act(ops, (1, 1, 1, M, Cp), dtype, torch.full((M * Cp,), 5.0))
    loss = torch.zeros(1, device=ops.device())
    cnt = torch.zeros(3, device=ops.device())
    ops.wce_loss(dense_act(ops, tuple(zz.shape), dtype, zz), lab.to(torch.uint8).to(ops.device()), 0, M, WEIGHTS, 1.0 / M, dl,
                 loss, cnt, ops.Workspace(1 << 16))
    lsum, grad, counts = wce_reference(z.numpy(), lab.numpy(), 1.0 / M)
    L = lsum / M
    assert abs(float(loss.cpu()) / M - L) < 2e-5 * abs(L) + 1e-6
    assert cnt.cpu().tolist() == counts
    got = dense64(dl).reshape(M, Cp)
    assert float(got[:, 3:].abs().max()) == 0.0
    err = (got[:, :3] - torch.tensor(grad)).abs()
    assert float(err.max()) < tol(dtype)[1] * float(np.abs(grad).max()) + 1e-9, "first bad row %d" % int(err.max(1).values.argmax())


# ============================================================================================ 4. loss and SGD forms
def wce_engine_case(ops, dtype):
    """LossLayer's form: one logits activation (a slab, ld 16), the gradient a slab with another stride, two row ranges
    that += into the same sums.  Planted rows: class 0 saturated at +60 under labels 1 / 2 (clipped: no gradient), the labelled
    class saturated (p = 1 exactly: no loss), labels 3 and 255 (outside the one-hot)."""
    M = 40000
    Cp = 8 if dtype == BF16 else 4
    z = rnd((M, 3), 3, 6.0, dtype)
    g = torch.Generator().manual_seed(5)
    lab = torch.randint(0, 3, (M,), generator=g)
    sat0 = [0, 1, 2, 3, 16998, 16999, 17000, 17001, 39998, 39999]
    z[sat0, 0] = 60.0
    lab[sat0] = torch.tensor([1, 2] * 5)
    satl = [10, 11, 12, 17010, 17011, 17012]
    lab[satl] = torch.tensor([0, 1, 2] * 2)
    z[satl, lab[satl]] = 60.0
    odd = {20: 3, 21: 255, 300: 3, 16990: 255, 17020: 3, 17021: 255, 25000: 3, 39990: 255}
    for r, v in odd.items():
        lab[r] = v
    z = q(z, dtype)
    zz = torch.zeros((1, 1, 1, M, Cp), dtype=torch.float64)
    zz[0, 0, 0, :, :3] = z
    la = mkact(ops, zz, dtype, 16, 8)
    labels = lab.to(torch.uint8).to(ops.device())
    return dict(M=M, Cp=Cp, z=z, lab=lab, la=la, labels=labels, sat0=sat0, satl=satl, odd=sorted(odd),
                ranges=((0, 17000), (17000, 23000)), gs=3.0 / M)


def run_wce_ranges(ops, cs, dl):
    loss = torch.full((1,), 1.5, device=ops.device())
    cnt = torch.tensor([10.0, 20.0, 30.0], device=ops.device())
    ws = ops.Workspace(1 << 16)
    for row0, m in cs["ranges"]:
        assert m > 64 * 256              # more than 64 partials: every lane of the finalize kernel loops
        ops.wce_loss(cs["la"], cs["labels"], row0, m, WEIGHTS, cs["gs"], dl, loss, cnt, ws)
    return float(loss.cpu()), cnt.cpu().tolist()


@pytest.mark.parametrize("dtype", DT)
def test_wce_loss_engine_form(hdu, dtype):
    ops = ops_mod()
    cs = wce_engine_case(ops, dtype)
    M, Cp, z, lab = cs["M"], cs["Cp"], cs["z"], cs["lab"]
    dl = mkact(ops, torch.full((1, 1, 1, M, Cp), 5.0, dtype=torch.float64), dtype, 24, 8)
    loss, cnt = run_wce_ranges(ops, cs, dl)
    lsum, grad = 0.0, np.zeros((M, 3))
    counts = [10.0, 20.0, 30.0]
    for row0, m in cs["ranges"]:
        l, gr, c = wce_reference(z[row0:row0 + m].numpy(), lab[row0:row0 + m].numpy(), cs["gs"])
        lsum += l
        grad[row0:row0 + m] = gr
        counts = [a + b for a, b in zip(counts, c)]
    L = lsum / M
    assert abs((loss - 1.5) / M - L) < 2e-5 * abs(L) + 1e-6
    assert cnt == counts
    assert sum(counts) == 60 + M - len(cs["odd"])
    got = got64(dl).reshape(M, Cp)
    assert float(got[:, 3:].abs().max()) == 0.0
    gmax = float(np.abs(grad).max())
    assert float((got[:, :3] - torch.tensor(grad)).abs().max()) < tol(dtype)[1] * gmax + 1e-9
    assert_poison_intact(dl, "wce dlogits")
    assert_poison_intact(cs["la"], "wce logits")
    # labels above 2: exactly nothing, and the rows next to them carry their own gradient
    for r in cs["odd"]:
        assert float(got[r].abs().max()) == 0.0
        for nb in (r - 1, r + 1):
            if nb not in cs["odd"]:
                assert float(got[nb, :3].abs().max()) > 0.0
    # class 0 saturated under another label: p(label) < 1e-10 is clipped, the gradient does not pass
    assert float(got[cs["sat0"]].abs().max()) == 0.0
    # the labelled class saturated: p = 1, no loss; gs * w * (p - onehot) is 0 up to the other classes' e^-60
    assert float(got[cs["satl"]].abs().max()) <= 1e-20
    zs, ls = z[cs["satl"]].numpy(), lab[cs["satl"]].numpy()
    assert wce_reference(zs, ls, cs["gs"])[0] == 0.0
    loss3 = torch.full((1,), 1.5, device=ops.device())
    cnt3 = torch.zeros(3, device=ops.device())
    ops.wce_loss(cs["la"], cs["labels"], cs["satl"][0], 3, WEIGHTS, cs["gs"], None, loss3, cnt3, ops.Workspace(1 << 16))
    assert float(loss3.cpu()) == 1.5 and cnt3.cpu().tolist() == [1.0, 1.0, 1.0]


@pytest.mark.parametrize("dtype", DT)
def test_wce_loss_only_form(hdu, dtype):
    """dlogits = None (evaluation): the same loss and counts as the gradient call, bit for bit, and no buffer written"""
    ops = ops_mod()
    cs = wce_engine_case(ops, dtype)
    dl = mkact(ops, torch.full((1, 1, 1, cs["M"], cs["Cp"]), 5.0, dtype=torch.float64), dtype, 24, 8)
    with_grad = run_wce_ranges(ops, cs, dl)
    logits_before, dl_before = cs["la"].buf.clone(), dl.buf.clone()
    assert run_wce_ranges(ops, cs, None) == with_grad
    assert torch.equal(cs["la"].buf, logits_before) and torch.equal(dl.buf, dl_before)
    assert bool((cs["labels"].cpu() == cs["lab"].to(torch.uint8)).all())


@pytest.mark.parametrize("momentum", [0.9, 0.0])
def test_sgd_nesterov_scaled_two_steps(hdu, momentum):
    ops = ops_mod()
    n, lr, gs = 1003, 1e-3, 1.0 / 7
    p0, v0, g1, g2 = (rnd((n,), s, 1.0).numpy() for s in (1, 2, 3, 4))
    T = lambda a: torch.tensor(a, dtype=torch.float32, device=ops.device())
    p, v = T(p0), T(v0)
    pr, vr = p0, v0
    for g in (g1, g2):
        gd = T(g)
        ops.sgd_nesterov(p, v, gd, lr, momentum, gs)
        pr, vr = N64.sgd_nesterov(pr, vr, g * gs, lr, momentum)
        np.testing.assert_allclose(p.cpu().numpy(), pr, rtol=2e-6, atol=2e-7)
        np.testing.assert_allclose(v.cpu().numpy(), vr, rtol=2e-6, atol=2e-7)
        assert float((gd.cpu().double() - torch.tensor(g)).abs().max()) == 0.0
    assert float(np.abs(pr - p0).max()) > 1e-5           # the steps moved the parameters by more than the tolerance


def test_sgd_nesterov_empty(hdu):
    """n = 0 is a successful no-op"""
    ops = ops_mod()
    p, v, g = (dev(ops, rnd((16,), s, 1.0)) for s in (1, 2, 3))
    before = [t.clone() for t in (p, v, g)]
    rc = hdu.lib.get().hdu_sgd_nesterov(ops.fptr(p), ops.fptr(v), ops.fptr(g), 0, 1e-3, 0.9, 1.0, ops.stream())
    assert rc == 0
    assert all(torch.equal(a, b) for a, b in zip((p, v, g), before))
