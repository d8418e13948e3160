"""Kernel-level checks of the two BN-backward forms that remove full-resolution passes from the decoder's backward:

* hdu_bn_bwd_fused_pw -- the BN backward whose dz is dy . W of a narrow pointwise consumer (a 3-class head stored as one 16-byte
  chunk per pixel), formed in registers by both launches -- against the three launches it replaces (data gradient through
  hdu_conv_fprop into a dz buffer, then hdu_bn_bwd_fused) of the same library, and against float64 autograd;
* the column sums of the stored gradient inside the BN-backward apply launch (the bias gradient of the conv that produced the BN
  input) -- against hdu_colsum over the tensor the same launch stored.

Each case runs on the x86 emulator build and, marked `gpu`, on the gfx950 library."""
import ctypes

import pytest
import torch

from test_kernels import BF16, DT, F32, assert_close, dev, mkact, ops_mod, q, rnd

N, D, H, W = 1, 1, 40, 26          # M = 1040 rows: several row blocks, not a multiple of ROW_UNROLL * ROWS (the tail loops run)
M = N * D * H * W
KCLS = 3
EPS = 1.1e-5
SEED = 1234


def ulp_bf16(t):
    """spacing of bfloat16 (8 significand bits) at |t|"""
    a = t.abs().double().clamp_min(2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 7)


def _bn(ops, x, C, dtype, seed):
    """BN(+Scale) parameters and this batch's fold of x: everything hdu_bn_bwd_fused takes"""
    xa = mkact(ops, x, dtype)
    dv = lambda t: dev(ops, t)
    E = lambda: torch.empty(C, device=ops.device())
    g = dv((rnd((C,), seed + 1, 0.5) + 1.0)); be = dv(rnd((C,), seed + 2, 0.2))
    sg = dv((rnd((C,), seed + 3, 0.5) + 1.0)); sb = dv(rnd((C,), seed + 4, 0.2))
    mean, var, a, b, r = [E() for _ in range(5)]
    ops.bn_stats(xa, mean, var, ops.Workspace(ops.reduce_ws_bytes(M, C)))
    ops.bn_fold(C, mean, var, g, be, EPS, sg, sb, a, b, r)
    return dict(xa=xa, g=g, be=be, sg=sg, sb=sb, mean=mean, a=a, b=b, r=r)


def _head(ops, C, dtype, seed):
    """a K-class pointwise head over C channels: float32 master [CH][C] (rows >= K zero, as the engine pads them), its
    data-gradient copy [C][CH] in the storage dtype (hdu_weight_prep) and an output gradient whose padding lanes carry values"""
    CH = ops.CHUNK[dtype]
    wm = torch.zeros(CH, C, dtype=torch.float64)
    wm[:KCLS] = rnd((KCLS, C), seed, 0.3)
    tdt = torch.bfloat16 if dtype == BF16 else torch.float32
    wd = torch.zeros(C * CH, dtype=tdt, device=ops.device())
    ops.weight_prep(dtype, dev(ops, wm.reshape(-1)), CH, 1, C, None, wd)
    dy = rnd((N, D, H, W, CH), seed + 1, 1.0, dtype)
    return dict(wq=q(wm[:KCLS], dtype), wd=wd, wd_ptr=ctypes.c_void_p(wd.data_ptr()), dy=dy, dya=mkact(ops, dy, dtype))


def _fused(ops, bn, dz, C, dx, acc, keep, slots=16, **kw):
    """one hdu_bn_bwd_fused (or, with pw=, hdu_bn_bwd_fused_pw) call; returns the parameter gradients"""
    sums = torch.zeros(slots * 2 * C, device=ops.device())
    grads = [torch.empty(C, device=ops.device()) for _ in range(4)]
    ops.bn_bwd_fused(dz, bn["xa"], bn["a"], bn["b"], True, bn["mean"], bn["r"], True, bn["g"], bn["be"], bn["sg"], sums, slots,
                     *grads, dx, acc, keep, SEED if keep < 1.0 else 0, None, **kw)
    return grads


_HEAD_CACHE = {}


def _head_case(hdu, ops, dtype, C, keep, acc):
    """reference (three launches) and new path (two launches) of one case, computed once per backend"""
    key = (hdu.lib.backend(), dtype, C, keep, acc)
    if key not in _HEAD_CACHE:
        x = q(rnd((N, D, H, W, C), 21, 2.0, dtype) + 0.25, dtype)
        old = rnd((N, D, H, W, C), 23, 1.0, dtype)
        bn, hd = _bn(ops, x, C, dtype, 30), _head(ops, C, dtype, 40)
        dza = ops.Act.alloc(N, D, H, W, C, dtype)
        ops.conv_fprop(ops.conv_desc(hd["dya"], hd["wd_ptr"], dza, (1, 1, 1)))
        dx_ref, dx_new = mkact(ops, old, dtype), mkact(ops, old, dtype)
        g_ref = _fused(ops, bn, dza, C, dx_ref, acc, keep)
        g_new = _fused(ops, bn, hd["dya"], C, dx_new, acc, keep, pw=(hd["wd_ptr"], KCLS))
        mask = None
        if keep < 1.0:          # the kernel's dropout mask (a hash of the element index), read off a launch that overwrites
            dx_m = ops.Act.alloc(N, D, H, W, C, dtype)
            _fused(ops, bn, dza, C, dx_m, False, keep)
            mask = (dx_m.to_torch().cpu().double() != 0)
        cpu = lambda ts: [t.cpu().double() for t in ts]
        _HEAD_CACHE[key] = dict(x=x, old=old, dy=hd["dy"], wq=hd["wq"], dz=dza.to_torch().cpu().double(), mask=mask,
                                k1=(bn["sg"] * bn["g"] * bn["r"]).cpu().double(),
                                par={k: bn[k].cpu().double() for k in ("g", "be", "sg", "sb")},
                                dx_ref=dx_ref.to_torch().cpu().double(), dx_new=dx_new.to_torch().cpu().double(),
                                g_ref=cpu(g_ref), g_new=cpu(g_new))
    return _HEAD_CACHE[key]


HEAD_CASES = [pytest.param(C, keep, acc, id="C%d-%s-%s" % (C, "drop" if keep < 1 else "nodrop", "acc" if acc else "store"))
              for C in (64, 24) for keep in (0.7, 1.0) for acc in (False, True)]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("C,keep,acc", HEAD_CASES)
def test_head_dz_in_registers_equals_the_three_launches(hdu, dtype, C, keep, acc):
    """hdu_bn_bwd_fused_pw == hdu_conv_fprop (data gradient) + hdu_bn_bwd_fused.  bf16: the in-register sum and the MFMA sum are
    both float32 roundings of the same three exact products, so the bf16 value of g differs by at most one ulp and every du by at
    most |k1| ulp_bf16(g) + ulp_bf16(du); float32 du and the parameter gradients at test_bn_backward_fused_wide's settings."""
    ops = ops_mod()
    cs = _head_case(hdu, ops, dtype, C, keep, acc)
    ref, got = cs["dx_ref"], cs["dx_new"]
    diff = (got - ref).abs()
    print("head dz in registers (%s, C=%d, keep=%.1f, acc=%d): %.4f %% of %d du elements differ, max |diff| %.3e"
          % ("bf16" if dtype == BF16 else "f32", C, keep, acc, 100.0 * float((diff > 0).double().mean()), diff.numel(), float(diff.max())))
    if dtype == BF16:
        lim = cs["k1"].abs() * ulp_bf16(cs["dz"]) + ulp_bf16(ref)
        bad = diff > lim
        assert not bad.any(), "%d/%d du elements beyond |k1| ulp(g) + ulp(du), worst excess %.3e" % (
            int(bad.sum()), bad.numel(), float((diff - lim).max()))
    else:
        assert_close(got, ref, F32, what="head du")
    for a, b, nm in zip(cs["g_new"], cs["g_ref"], ("dgamma", "dbeta", "dsgamma", "dsbeta")):
        assert_close(a, b, F32, scale=float(b.abs().max()), what="head " + nm)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("C,keep,acc", HEAD_CASES)
def test_head_dz_in_registers_vs_float64_autograd(hdu, dtype, C, keep, acc):
    """the same launches against float64 autograd of BN(+Scale) -> ReLU -> 1x1 conv (batch statistics), with the kernel's own
    dropout mask, at assert_close's tolerance of the storage dtype"""
    ops = ops_mod()
    cs = _head_case(hdu, ops, dtype, C, keep, acc)
    xr = cs["x"].clone().requires_grad_(True)
    g, be, sg, sb = [cs["par"][k].clone().requires_grad_(True) for k in ("g", "be", "sg", "sb")]
    xf = xr.reshape(-1, C)
    mu = xf.mean(0); v = ((xf - mu) ** 2).mean(0)
    z = (sg * ((xf - mu) / torch.sqrt(v + EPS) * g + be) + sb).clamp_min(0)
    ((z @ cs["wq"].t()) * cs["dy"].reshape(-1, cs["dy"].shape[-1])[:, :KCLS]).sum().backward()
    want = xr.grad
    if cs["mask"] is not None:
        want = want * cs["mask"] / keep
    if acc:
        want = want + cs["old"]
    assert_close(cs["dx_new"], want, dtype, what="head du vs autograd")
    for got, ref, nm in zip(cs["g_new"], (g.grad, be.grad, sg.grad, sb.grad), ("dgamma", "dbeta", "dsgamma", "dsbeta")):
        assert_close(got, ref, dtype, what="head %s vs autograd" % nm)


SUM_CASES = [pytest.param(C, slots, acc, keep, pw, id="C%d-slots%d-%s-%s%s" % (C, slots, "acc" if acc else "store",
                                                                                  "drop" if keep < 1 else "nodrop", "-pw" if pw else ""))
             for C, pw in ((328, False), (64, False), (64, True)) for slots in (16, 3) for acc in (False, True) for keep in (0.7, 1.0)]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("C,slots,acc,keep,pw", SUM_CASES)
def test_apply_column_sums_equal_colsum_of_what_it_stored(hdu, dtype, C, slots, acc, keep, pw):
    """the [slots][C] table an apply launch fills, folded by hdu_colsum_fold_batched, == hdu_colsum over the dx the same launch
    wrote (two column groups with a partial last one at C = 328; `pw`: the in-register-dz form of the same launch).  A reordered
    float32 sum is bounded relative to the sum of magnitudes -- the sum itself is near zero for a batch-statistics BN without
    dropout -- so the tolerance is assert_close's float32 setting scaled by the largest per-channel sum of |dx|."""
    ops = ops_mod()
    x = q(rnd((N, D, H, W, C), 51, 2.0, dtype) + 0.25, dtype)
    bn = _bn(ops, x, C, dtype, 60)
    dx = mkact(ops, rnd((N, D, H, W, C), 52, 1.0, dtype), dtype)
    tbl = torch.zeros(slots * C, device=ops.device())
    kw = dict(colsum=tbl, colsum_slots=slots)
    if pw:
        hd = _head(ops, C, dtype, 70)
        dz, kw["pw"] = hd["dya"], (hd["wd_ptr"], KCLS)
    else:
        dz = mkact(ops, rnd((N, D, H, W, C), 53, 1.0, dtype), dtype)
    _fused(ops, bn, dz, C, dx, acc, keep, **kw)
    out, ref = torch.full((C,), 7.0, device=ops.device()), torch.empty(C, device=ops.device())
    ops.ColsumPlan([(tbl, slots, C, out)]).run()
    ops.colsum(dx, ref, ops.Workspace(ops.reduce_ws_bytes(M, C)))
    stored = dx.to_torch().cpu().double().reshape(M, C)
    scale = float(stored.abs().sum(0).max())
    assert scale > 0 and float(stored.sum(0).abs().max()) > 0
    assert_close(out.cpu(), ref.cpu().double(), F32, scale=scale, what="column sums in the apply launch")
