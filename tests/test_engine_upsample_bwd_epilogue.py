"""Engine-level check of HDU_UPS_BWD_EPILOGUE (ConvLayer._ups_epilogue: the up-sampling gradient of conv_up0..4 summed in the epilogue
of their halo-wide data-gradient launches, hdu_conv_desc.y_ds): one bf16 training step of the reduced-depth 2D DenseUNet (2 x 64 x 64,
dropout on) with the switch on against the same step with it off, from the same seeded state, under the atomics-free reductions of
parity_utils.ordered_reductions -- loss and every parameter bit-equal, and the C-ABI call log of both steps.  The layers of this small
net are below the halo-wide kernels' size thresholds, so a configuration is forced through the HDU_TUNE_HALO_WIDE tuning key."""
import collections

import torch

import parity_utils as U

NB = (2, 2, 2, 2)
B, SIZE = 2, 64
HDU_TUNE_HALO_WIDE = 29
HDU_TUNE_HALO_TARGET_WGS = 7
UPS = ("conv_up0", "conv_up1", "conv_up2", "conv_up3", "conv_up4")


def _one_step(on, monkeypatch):
    monkeypatch.setenv("HDU_UPS_BWD_EPILOGUE", on)
    m = U.pkg("denseunet").DenseUNet(reduction=0.5, args=U.make_args(B, SIZE), dtype="bf16", nb_layers=NB)
    m.compile(optimizer=U.pkg("keras_api").SGD(lr=1e-3, momentum=0.9, nesterov=True), loss=[U.pkg("loss").weighted_crossentropy_2ddense])
    assert m.ctx.dropout_enabled and m.ctx.ups_bwd_epilogue == (on == "1")
    x, y = U.synthetic_batch("2d", B, SIZE, None)
    lib = U.pkg("lib")
    lib.profile_begin()
    loss = m.train_on_batch(x, y)
    recs, calls = lib.profile_end()
    ups = [c for c in m.ctx.convs if c.name in UPS]
    assert len(ups) == 5 and all(c.up == (0, 1, 1) for c in ups)
    # the data-gradient launches of conv_up0..4 (by their flipped filter) and what they were asked for
    dgrad = {}
    for name, args, _, _ in calls:
        if name == "hdu_conv_fprop":
            d = args[0]._obj
            for c in ups:
                if c.wd_ptr is not None and d.w == c.wd_ptr.value:
                    dgrad[c.name] = (bool(d.y_ds), int(d.ds_only), int(d.ds_accumulate))
    return dict(loss=loss, P=m.ctx.P.clone(), names=collections.Counter(c[0] for c in calls), launches=len(recs), dgrad=dgrad,
                kernels=collections.Counter(r[0].split("<")[0] for r in recs),
                skips={c.name: c.skip is not None for c in ups})


def test_step_with_upsample_gradient_in_epilogue_is_bit_equal(hdu, monkeypatch):
    if hdu.lib.backend() == "emu-x86":
        monkeypatch.setenv("HIPEMU_THREADS", "1")
    lib = hdu.lib.get()
    with U.ordered_reductions():
        lib.hdu_set_tuning(HDU_TUNE_HALO_WIDE, 2)
        # ordered_reductions gives every filter-gradient element ONE writer through HDU_TUNE_WGRAD_TARGET_WGS, which the halo-tile
        # filter-gradient kernels of the bf16 step do not read: they size their pixel splits by this key (measured on MI355X without
        # it: two runs of the SAME switch setting differ in 20-30 elements of the conv_up3 / conv_up4 filter gradients)
        lib.hdu_set_tuning(HDU_TUNE_HALO_TARGET_WGS, 1)
        try:
            on, off = (_one_step(s, monkeypatch) for s in ("1", "0"))
        finally:
            lib.hdu_set_tuning(HDU_TUNE_HALO_WIDE, 0)
            lib.hdu_set_tuning(HDU_TUNE_HALO_TARGET_WGS, 0)
    # ---- call log: the five hdu_upsample_bwd calls of conv_up0..4 are gone and nothing came in their place
    assert off["names"]["hdu_upsample_bwd"] == 5 and on["names"]["hdu_upsample_bwd"] == 0, (off["names"], on["names"])
    delta = collections.Counter(on["names"])
    delta.subtract(off["names"])
    assert {k: v for k, v in delta.items() if v} == {"hdu_upsample_bwd": -5}, delta
    assert on["launches"] == off["launches"] - 5, (on["launches"], off["launches"])
    assert off["kernels"]["upsample_bwd_kernel"] == 5 and on["kernels"]["upsample_bwd_kernel"] == 0
    assert on["kernels"]["conv_halo_wide_kernel"] == off["kernels"]["conv_halo_wide_kernel"] >= 5
    # a layer with a skip writes both outputs (d(x_eff) is the skip's gradient), conv_up4 only the sums
    assert set(on["dgrad"]) == set(UPS)
    for n, (has_ds, only, acc) in on["dgrad"].items():
        assert has_ds and not acc and only == (0 if on["skips"][n] else 1), (n, has_ds, only, acc)
    assert not on["skips"]["conv_up4"] and all(v == (False, 0, 0) for v in off["dgrad"].values())
    # ---- bit-equal step
    assert on["loss"] == off["loss"], (on["loss"], off["loss"])
    diff = int((on["P"] != off["P"]).sum())
    print("switch on vs off: loss %.9g / %.9g, %d of %d parameters differ" % (on["loss"], off["loss"], diff, on["P"].numel()))
    assert torch.equal(on["P"], off["P"]), "%d of %d parameters differ after the step" % (diff, on["P"].numel())

