"""CPU checks of the oracle's 16-bit storage rounding (pacing_oracle.StorageRounding), which tests/test_gpu_h16_oracle.py
compares the device with: how it rounds, the loss scale, the order of rounded gradient sums, and that a missing site raises."""
import pytest
import torch

from oracle import pacing_oracle as O
from tests import _golden as G


def test_values_round_from_fp32_not_from_fp64():
    """1 + 2^-11 + 2^-40: fp64 -> fp16 rounds up (numpy converts directly), fp64 -> fp32 -> fp16 is a tie and rounds to even
    (1.0), as the device does from its fp32 value."""
    import numpy as np
    x = torch.tensor([1 + 2.0 ** -11 + 2.0 ** -40], dtype=torch.float64)
    assert float(np.float16(x.numpy()[0])) == 1 + 2.0 ** -10
    st = O.StorageRounding(torch.float16, 1.0, {})
    assert float(st.value(x)) == 1.0
    assert st.value(x).dtype == torch.float64


def test_gradients_are_rounded_with_the_loss_scale():
    """2^-30 underflows fp16 (smallest subnormal 2^-24) unless it is scaled by 2^10 first; the scale is removed exactly."""
    for scale, want in ((1.0, 0.0), (1024.0, 2.0 ** -30)):
        st = O.StorageRounding(torch.float16, scale, {'t': 'B'})
        x = torch.ones(1, dtype=torch.float64, requires_grad=True)
        (st.act(x, 't') * 2.0 ** -30).sum().backward()
        assert float(x.grad) == want
    st = O.StorageRounding(torch.bfloat16, 1024.0, {'t': 'FB'})
    x = torch.tensor([1 + 2.0 ** -9], dtype=torch.float64, requires_grad=True)
    y = st.act(x, 't')
    assert float(y.detach()) == 1.0                         # bf16: 8 significand bits, tie to even
    (y * (1 + 2.0 ** -8 + 2.0 ** -10)).sum().backward()
    assert float(x.grad) == 1 + 2.0 ** -7                   # the gradient rounded as well (above the midpoint)


def test_uses_add_in_engine_order_with_a_rounding_after_each_add():
    """uses ['dec', 'aux', 'next']: round(round(round(g_dec) + g_aux) + g_next)."""
    st = O.StorageRounding(torch.bfloat16, 1.0, {'s': ['dec', 'aux', 'next']})
    x = torch.ones(1, dtype=torch.float64, requires_grad=True)
    g = {'dec': 1 + 2.0 ** -9, 'aux': 2.0 ** -9, 'next': 2.0 ** -10}
    sum(st.use(x, 's', u) * v for u, v in g.items()).sum().backward()
    r = lambda v: float(torch.tensor([v], dtype=torch.float64).float().to(torch.bfloat16).double())   # noqa: E731
    assert float(x.grad) == r(r(r(g['dec']) + g['aux']) + g['next'])
    assert float(x.grad) != r(g['dec'] + g['aux'] + g['next'])
    st2 = O.StorageRounding(torch.bfloat16, 1.0, {'s': 'fused'})
    y = torch.ones(1, dtype=torch.float64)
    assert st2.use(y, 's', 'anything') is y


def _tiny():
    from tests import _golden as G
    args = O.default_args(**G.TINY, **G.FULL)
    return args, O.init_state(args, seed=3), O.synthetic_batch(2, 32, 32, seed=1, keep=0.1)


def _all_sites(args, flags='FB'):
    sites = {'input': 'F', 'aux_path.layer_bottleneck:z': flags, 'aux_path.layer_bottleneck:y': flags}
    for p in O.conv_layer_prefixes(args):
        sites.update({p + ':z': flags, p + ':y': flags, p + ':split': 0})
    enc = O.stage_plan(args)['enc']
    for k in range(1, 7):
        if enc[k - 1]['pool']:
            sites[f'backbone.enc_block{k}.pooling'] = 'B'
        sites[f'backbone.enc_block{k}'] = 'fused' if k < 6 and enc[k]['pool'] else ['dec', 'aux', 'next']
    for k in range(1, 6):
        sites[f'backbone.dec_block{k}.up'] = flags
        sites[f'backbone.dec_block{k}.cat'] = 'B'
    return sites


def test_oracle_step_with_storage_rounding():
    """Sites switched on but rounding to fp32 (a no-op): the step equals the plain oracle's to fp32 rounding (the split BatchNorm
    is written out instead of F.batch_norm) and every site is reached.  Rounding to fp16: every stored y is an fp16 number, the
    step moves by the size of fp16 rounding, and a site missing from the map raises."""
    args, sd, batch = _tiny()
    ref_out, ref_grads, _ = O.train_step({k: v.clone() for k, v in sd.items()}, batch, 0, args, training=True)
    st = O.StorageRounding(torch.float32, 1024.0, _all_sites(args))
    O.STORAGE = st
    try:
        out, grads, _ = O.train_step({k: v.clone() for k, v in sd.items()}, batch, 0, args, training=True)
    finally:
        O.STORAGE = None
    assert set(st.sites) == st.seen
    for k in ('segmentation/logits', 'loss_pce', 'loss_cr', 'loss_aux_cls'):
        assert float((out[k] - ref_out[k]).abs().max()) <= 1e-5 * float(ref_out[k].abs().max()), k
    for k, g in ref_grads.items():
        if g is not None and float(g.norm()) > 0 and not G.is_bias_before_bn(k):
            assert float((grads[k] - g).norm() / g.norm()) < 1e-4, k
    O.STORAGE, O.TAP = O.StorageRounding(torch.float16, 1024.0, _all_sites(args)), {}
    try:
        out16, grads16, _ = O.train_step({k: v.clone() for k, v in sd.items()}, batch, 0, args, training=True)
        taps = O.TAP
    finally:
        O.STORAGE, O.TAP = None, None
    for prefix, calls in taps.items():
        for _, y in calls:
            assert torch.equal(y.detach(), y.detach().half().float()), prefix
    e = float((out16['segmentation/logits'] - ref_out['segmentation/logits']).abs().max() / ref_out['segmentation/logits'].abs().max())
    assert 1e-5 < e < 3e-2, e
    sites = _all_sites(args)
    del sites['backbone.dec_block3.cat']
    O.STORAGE = O.StorageRounding(torch.float16, 1024.0, sites)
    try:
        with pytest.raises(KeyError, match='dec_block3.cat'):
            O.train_step({k: v.clone() for k, v in sd.items()}, batch, 0, args, training=True)
    finally:
        O.STORAGE = None
