"""The second, 2 x 2 down-sampled output of the halo-wide data-gradient launch (hdu_conv_desc.y_ds / ds_only / ds_accumulate): the
gradient of an UpSampling (0, 1, 1) summed from the staged output tile in the epilogue.  Reference, from the same library and the
same forced configuration: the plain launch into a full-resolution buffer, then hdu_upsample_bwd -- every output bit-equal.  Runs on
the emulator build and, marked `gpu`, on the gfx950 library."""
import ctypes
import importlib

import pytest
import torch

BF16, F32 = 0, 1
N, H, W, CIN = 2, 24, 48, 64          # 24 x 48: the last tile is ragged in both directions for TH = 8 (24 = 3 x 8, 48 = 32 + 16) and TH = 16
CONFIGS = ["8x128", "16x64", "16x96", "8x64", "8x96", "16x128", "16x64p"]          # HDU_TUNE_HALO_WIDE = 2 + index
SHAPES = [pytest.param((1, (1, 3, 3), 96), id="2d_cout96"), pytest.param((1, (1, 3, 3), 160), id="2d_cout160_ragged_group"),
          pytest.param((4, (3, 3, 3), 96), id="3x3x3_depth4")]
HDU_TUNE_HALO_WIDE = 29


def _ops():
    return importlib.import_module("h-denseunet_amd.ops")


def _rand(shape, seed, scale, dev):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g) * 2 - 1) * scale).to(torch.bfloat16).to(dev)


def _problem(ops, D, K, cout, h=H, w=W, cin=CIN):
    dev = ops.device()
    x = _rand((N, D, h, w, cin), 21, 1.0, dev)
    wt = _rand((cout,) + K + (cin,), 22, 1.0 / (K[0] * K[1] * K[2] * cin) ** 0.5, dev)
    xa = ops.Act(x.reshape(-1), 0, N, D, h, w, cin, cin, BF16)
    pad = (K[0] // 2, 1, 1)

    def desc(ya):
        return ops.conv_desc(xa, ctypes.c_void_p(wt.data_ptr()), ya, K, (1, 1, 1), pad)
    return desc, (x, wt)


def _full(ops, D, cout, h=H, w=W, fill=None):
    a = ops.Act.alloc(N, D, h, w, cout, BF16)
    if fill is not None:
        a.buf.fill_(fill)
    return a


def _ds_slab(ops, D, cout, old=None):
    """the down-sampled output as a slab of a wider, poisoned buffer (pixel stride cout + 16, first channel 8)"""
    big = ops.Act.alloc(N, D, H // 2, W // 2, cout + 16, BF16)
    big.buf.fill_(7.0)
    a = big.slab(8, cout)
    if old is not None:
        a.from_torch(old)
    return big, a


def _sync(ops):
    if ops.device().type == "cuda":
        torch.cuda.synchronize()


def _outside_untouched(big, cout):
    v = big.buf.reshape(-1, cout + 16)
    return bool((v[:, :8] == 7.0).all()) and bool((v[:, 8 + cout:] == 7.0).all())


@pytest.mark.parametrize("cfg", range(len(CONFIGS)), ids=CONFIGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_downsampled_output_equals_plain_launch_then_upsample_bwd(hdu, shape, cfg):
    D, K, cout = shape
    ops = _ops()
    lib = hdu.lib.get()
    lib.hdu_set_tuning(HDU_TUNE_HALO_WIDE, 2 + cfg)
    try:
        desc, keep = _problem(ops, D, K, cout)
        # ---- reference: plain launch, then hdu_upsample_bwd (store and accumulate form)
        full = _full(ops, D, cout)
        d = desc(full)
        assert ops.conv_kernel_name(d, 0) == "conv_halo_wide_kernel<%s>" % CONFIGS[cfg]
        ops.conv_fprop(d)
        old = _rand((N, D, H // 2, W // 2, cout), 23, 2.0, ops.device())
        ref_big, ref = _ds_slab(ops, D, cout)
        ops.upsample_bwd(full, ref, (0, 1, 1))
        refa_big, refa = _ds_slab(ops, D, cout, old)
        ops.upsample_bwd(full, refa, (0, 1, 1), accumulate=True)
        _sync(ops)
        assert float(full.buf.float().abs().max()) > 0.1 and _outside_untouched(ref_big, cout)
        # ---- ds_only: the full-resolution buffer stays as it was
        poison = _full(ops, D, cout, fill=-3.0)
        big, ds = _ds_slab(ops, D, cout)
        d = desc(poison)
        d.y_ds, d.ldy_ds, d.ds_only = ds.ptr, ds.ld, 1
        ops.conv_fprop(d)
        _sync(ops)
        assert bool((poison.buf == -3.0).all()), "ds_only wrote the full-resolution buffer"
        assert torch.equal(big.buf, ref_big.buf), "ds_only"
        # ---- both outputs
        full2 = _full(ops, D, cout, fill=-3.0)
        big, ds = _ds_slab(ops, D, cout)
        d = desc(full2)
        d.y_ds, d.ldy_ds = ds.ptr, ds.ld
        ops.conv_fprop(d)
        _sync(ops)
        assert torch.equal(full2.buf, full.buf), "two outputs: full resolution"
        assert torch.equal(big.buf, ref_big.buf), "two outputs: down-sampled"
        # ---- ds_accumulate (with and without the full-resolution store)
        for only in (1, 0):
            tgt = _full(ops, D, cout, fill=-3.0)
            big, ds = _ds_slab(ops, D, cout, old)
            d = desc(tgt)
            d.y_ds, d.ldy_ds, d.ds_accumulate, d.ds_only = ds.ptr, ds.ld, 1, only
            ops.conv_fprop(d)
            _sync(ops)
            assert torch.equal(big.buf, refa_big.buf), "ds_accumulate, ds_only = %d" % only
            assert torch.equal(tgt.buf, full.buf) if not only else bool((tgt.buf == -3.0).all())
    finally:
        lib.hdu_set_tuning(HDU_TUNE_HALO_WIDE, 0)


def test_downsampled_output_error_returns(hdu):
    ops = _ops()
    lib = hdu.lib.get()
    HduError = hdu.lib.HduError
    lib.hdu_set_tuning(HDU_TUNE_HALO_WIDE, 2)
    try:
        # odd Ho
        desc, keep = _problem(ops, 1, (1, 3, 3), 96, h=23)
        big, ds = _ds_slab(ops, 1, 96)
        d = desc(_full(ops, 1, 96, h=23))
        d.y_ds, d.ldy_ds, d.ds_only = ds.ptr, ds.ld, 1
        with pytest.raises(HduError, match="even Ho and Wo"):
            ops.conv_fprop(d)
        # misaligned y_ds
        desc, keep2 = _problem(ops, 1, (1, 3, 3), 96)
        d = desc(_full(ops, 1, 96))
        d.y_ds, d.ldy_ds, d.ds_only = ctypes.c_void_p(ds.ptr.value + 8), ds.ld, 1
        with pytest.raises(HduError, match="16-byte aligned"):
            ops.conv_fprop(d)
        # the flags without the pointer, and together with the accumulating full-resolution store
        d = desc(_full(ops, 1, 96))
        d.ds_only = 1
        with pytest.raises(HduError, match="without y_ds"):
            ops.conv_fprop(d)
        d = desc(_full(ops, 1, 96))
        d.y_ds, d.ldy_ds, d.accumulate = ds.ptr, ds.ld, 1
        with pytest.raises(HduError, match="excludes accumulate"):
            ops.conv_fprop(d)
        # shapes that no halo-wide configuration takes: a pointwise conv (forced configuration), a 16-channel contraction under the
        # library's own choice, and the halo-wide kernels switched off
        x1 = _rand((N, 1, H, W, CIN), 31, 1.0, ops.device())
        w1 = _rand((96, CIN), 32, 0.1, ops.device())
        d = ops.conv_desc(ops.Act(x1.reshape(-1), 0, N, 1, H, W, CIN, CIN, BF16), ctypes.c_void_p(w1.data_ptr()), _full(ops, 1, 96),
                          (1, 1, 1))
        d.y_ds, d.ldy_ds = ds.ptr, ds.ld
        with pytest.raises(HduError, match="halo-wide"):
            ops.conv_fprop(d)
        lib.hdu_set_tuning(HDU_TUNE_HALO_WIDE, 0)
        desc16, keep3 = _problem(ops, 1, (1, 3, 3), 96, cin=16)
        d = desc16(_full(ops, 1, 96))
        assert not ops.conv_kernel_name(d, 0).startswith("conv_halo_wide_kernel")
        d.y_ds, d.ldy_ds = ds.ptr, ds.ld
        with pytest.raises(HduError, match="halo-wide"):
            ops.conv_fprop(d)
        lib.hdu_set_tuning(HDU_TUNE_HALO_WIDE, 1)
        d = desc(_full(ops, 1, 96))
        d.y_ds, d.ldy_ds = ds.ptr, ds.ld
        with pytest.raises(HduError, match="halo-wide"):
            ops.conv_fprop(d)
        _sync(ops)
        assert bool((big.buf == 7.0).all()), "a refused launch wrote the down-sampled output"
    finally:
        lib.hdu_set_tuning(HDU_TUNE_HALO_WIDE, 0)
