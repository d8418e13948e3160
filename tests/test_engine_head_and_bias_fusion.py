"""Engine-level checks of HDU_HEAD_DZ_FUSED (the classifier's data gradient formed inside its input BN's backward launches,
hdu_bn_bwd_fused_pw) and HDU_BIAS_SUMS_IN_APPLY (the conv_up* bias gradients summed by the BN-backward apply launch that writes
their output gradient, folded by one hdu_colsum_fold_batched launch): one training step of the reduced-depth 2D DenseUNet
(2 x 64 x 64, dropout on) with both paths on against the same step with both off, from the same seeded state -- gradients, and the
C-ABI call log of both steps.  On the card also a captured step replayed twice."""
import collections

import numpy as np
import pytest
import torch

import parity_utils as U

NB = (2, 2, 2, 2)
B, SIZE = 2, 64
# C-ABI calls of ONE first training step of this net as the commit before the two paths existed logs them (entry point -> calls):
# what HDU_HEAD_DZ_FUSED=0 HDU_BIAS_SUMS_IN_APPLY=0 must still log.  The two storage types differ in the filter gradients only
# (bf16: seven batched launches + the stem's own; float32 parity mode: one launch per layer).
_COMMON = {"hdu_affine_act": 1, "hdu_avgpool2_bwd": 3, "hdu_avgpool2_fwd": 3, "hdu_bn_bwd_apply_sums": 19, "hdu_bn_bwd_fused": 7,
           "hdu_bn_fold": 12, "hdu_bn_stats": 12, "hdu_bn_stats_fold": 14, "hdu_cast_pad": 1, "hdu_colsum": 7, "hdu_conv_fprop": 53,
           "hdu_materialize": 13, "hdu_maxpool3s2_bwd": 1, "hdu_maxpool3s2_fwd": 1, "hdu_sgd_nesterov": 1, "hdu_upsample_bwd": 5,
           "hdu_wce_loss": 1, "hdu_weight_prep_batched": 1, "hdu_zero_regions": 1}
PARENT_CALLS = {"f32": dict(_COMMON, hdu_conv_wgrad=27), "bf16": dict(_COMMON, hdu_conv_wgrad=1, hdu_wgrad_plan_run=7)}
NAMED = ("conv_up0", "conv_up1", "conv_up2", "conv_up3", "conv_up4", "bn_up4", "dense167classifer")


def _build(dtype, on, monkeypatch):
    monkeypatch.setenv("HDU_HEAD_DZ_FUSED", on)
    monkeypatch.setenv("HDU_BIAS_SUMS_IN_APPLY", on)
    m = U.pkg("denseunet").DenseUNet(reduction=0.5, args=U.make_args(B, SIZE), dtype=dtype, nb_layers=NB)
    m.compile(optimizer=U.pkg("keras_api").SGD(lr=1e-3, momentum=0.9, nesterov=True), loss=[U.pkg("loss").weighted_crossentropy_2ddense])
    assert m.ctx.dropout_enabled and m.ctx.head_dz_fused == (on == "1") and m.ctx.bias_sums_in_apply == (on == "1")
    return m


def _one_step(dtype, on, monkeypatch):
    m = _build(dtype, on, monkeypatch)
    x, y = U.synthetic_batch("2d", B, SIZE, None)
    lib = U.pkg("lib")
    lib.profile_begin()
    loss = m.train_on_batch(x, y)
    _, calls = lib.profile_end()
    cls = next(c for c in m.ctx.convs if c.name == "dense167classifer")
    head_dgrad = sum(1 for name, args, _, _ in calls if name == "hdu_conv_fprop" and args[0]._obj.w == cls.wd_ptr.value)
    return dict(loss=loss, grads=m.get_grads_dict(), names=collections.Counter(c[0] for c in calls), head_dgrad=head_dgrad)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_step_with_both_paths_equals_step_without(hdu, monkeypatch, dtype):
    if hdu.lib.backend() == "emu-x86":
        # one emulator thread: workgroups run in launch order, so the float atomics of every run add in the same order
        monkeypatch.setenv("HIPEMU_THREADS", "1")
        on, off = (_one_step(dtype, s, monkeypatch) for s in ("1", "0"))
        off2 = off                      # (a second OFF step would be bit-equal here)
    else:
        on, off, off2 = (_one_step(dtype, s, monkeypatch) for s in ("1", "0", "0"))
    # ---- call log
    assert on["head_dgrad"] == 0, "the classifier's data gradient is still launched"
    assert off["head_dgrad"] == 1
    assert dict(off["names"]) == PARENT_CALLS[dtype], sorted((collections.Counter(PARENT_CALLS[dtype]) - off["names"]).items()) + \
        sorted((off["names"] - collections.Counter(PARENT_CALLS[dtype])).items())
    assert on["names"]["hdu_colsum"] == off["names"]["hdu_colsum"] - 5
    delta = collections.Counter(on["names"])
    delta.subtract(off["names"])
    assert {k: v for k, v in delta.items() if v} == {"hdu_colsum": -5, "hdu_conv_fprop": -1, "hdu_bn_bwd_fused": -1,
                                                     "hdu_bn_bwd_fused_pw": 1, "hdu_colsum_fold_batched": 1}, delta
    assert off["names"] == off2["names"]
    # ---- loss and gradients: the tolerance of the model-parity tests for two runs of one mode (per gradient, 5e-4 of its scale
    # in float32; the storage precision in bf16) on top of the distance two runs of the OFF step have from each other
    assert abs(on["loss"] - off["loss"]) <= 1e-5 * abs(off["loss"])
    rel = 5e-4 if dtype == "f32" else 2e-2
    gmax = max(float(np.abs(a).max()) for gs in off["grads"].values() for a in gs)
    worst = {}
    for n, gs in off["grads"].items():
        for i, a in enumerate(gs):
            sc = max(float(np.abs(a).max()), 1e-3 * gmax)
            err = float(np.abs(on["grads"][n][i] - a).max())
            noise = float(np.abs(off2["grads"][n][i] - a).max())
            worst[(n, i)] = (err / sc, noise / sc)
            what = ("%s gradient %d (%s)" % (n, i, "kernel" if i == 0 and a.ndim > 1 else "bias / gamma / beta")
                    if n.startswith(NAMED) else "gradient %d of %s" % (i, n))
            assert err <= 4.0 * noise + rel * sc, "%s: |on - off| = %.3e of its scale, |off' - off| = %.3e" % (what, err / sc, noise / sc)
    named = {k: v for k, v in worst.items() if k[0].startswith(NAMED)}
    assert len(named) >= 5 * 2 + 2 + 2
    print("on vs off (%s): largest |on - off| / scale over the decoder tail's gradients %.3e (off vs off: %.3e), over all %.3e"
          % (dtype, max(v[0] for v in named.values()), max(v[1] for v in named.values()), max(v[0] for v in worst.values())))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_captured_step_clears_the_column_sum_tables(hip_lib, monkeypatch, dtype):
    """a captured step with both paths on, replayed twice from the same state: the conv_up* bias gradients of the second replay
    are the first replay's, not twice them -- the column-sum tables are cleared by the step's own zero launch, inside the graph"""
    m = _build(dtype, "1", monkeypatch)
    x, y = U.synthetic_batch("2d", B, SIZE, None)
    m.train_on_batch(x, y)
    m.train_step_resident()
    torch.cuda.synchronize()
    ctx = m.ctx
    assert ctx._csum_plan is not None and len(ctx._csum_plan[0]) == 5
    state = (ctx.P.clone(), ctx.V.clone(), ctx.seed_dev.clone(), m.optimizer.iterations, [(r.mean.clone(), r.var.clone()) for r in ctx.stat_roots])

    def restore():
        ctx.P.copy_(state[0]); ctx.V.copy_(state[1]); ctx.seed_dev.copy_(state[2])
        m.optimizer.iterations = state[3]
        for r, (mu, va) in zip(ctx.stat_roots, state[4]):
            r.mean.copy_(mu); r.var.copy_(va)

    def bias_grads():
        m.train_step_resident()
        torch.cuda.synchronize()
        return {c.name: c.bias.grad.clone() for c in ctx.convs if c.name.startswith("conv_up")}

    eager = bias_grads()
    # A conv in front of a batch-statistics BN has a bias gradient of exactly zero (conv_up0 .. 3: what is computed is the sum of
    # the roundings of dy); conv_up4 sits in front of dropout and has a real one (a fifth of the sum of |dy|).  So the yardstick
    # of every comparison is the largest per-channel sum of |dy|, as for the kernel test of the column sums.  float32: a reordered
    # sum stays below 1e-4 of it.  bf16: the float atomics upstream move a stored dy to a neighbouring bf16 value from run to run,
    # one ulp <= 2^-7 |dy| each, and conv_up0 has only 32 rows to average that over: 2^-7 of the sum of |dy| bounds it.  A table
    # that is not cleared adds the previous replay's sums on top: 0.2 of the yardstick in conv_up4.
    mag = {c.name: float(c.out.grad.to_torch().abs().sum(dim=(0, 1, 2, 3)).max()) for c in ctx.convs if c.name.startswith("conv_up")}
    restore()
    m.capture_graph(warmup=0)
    assert m._graph is not None
    restore()
    first = bias_grads()
    restore()
    second = bias_grads()
    assert len(first) == 5
    rel = 1e-4 if dtype == "f32" else 2.0 ** -7
    assert float(eager["conv_up4"].abs().max()) >= 10 * rel * mag["conv_up4"]        # (a doubled gradient would be seen)
    for n in first:
        assert mag[n] > 0
        for tag, g in (("first", first[n]), ("second", second[n])):
            err = float((g - eager[n]).abs().max())
            assert err <= rel * mag[n], "%s bias gradient of the %s replay vs the eager step: %.3e of sum |dy|" % (n, tag, err / mag[n])
