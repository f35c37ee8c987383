"""The two split-fp16 operand formats, emulated in numpy: where the bounds of tests/test_gpu_operand_range.py and the figures of
docs/operand_range.md come from.

  scaled     v ~ hi + lo / 2048,  hi = fp16(v), lo = fp16((v - hi) * 2048): forward activations (operand scale 1), weights, the
             gradients of the forward / data-gradient kernels and every Winograd transform-domain operand;
  unscaled   v ~ hi + lo,         hi = fp16(v), lo = fp16(v - hi): the dz operand of the direct weight-gradient kernels
             (WgradH16Args, pp_conv.hip), after dz was brought into [2^9, 2^10) by the power of two of f16_scales.
The errors are max norms relative to the largest value of the operand (a forward tensor) or of the output channel (dz).
"""
import numpy as np
import pytest


def split_scaled(v):
    v = v.astype(np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        hi = v.astype(np.float16)
        lo = ((v - hi.astype(np.float32)) * np.float32(2048)).astype(np.float16)
        return hi.astype(np.float64) + lo.astype(np.float64) / 2048


def split_unscaled(v):
    v = v.astype(np.float32)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64) + lo.astype(np.float64)


def f16_scale(amax, clamp=True):
    """s_in of f16_scales (pp_common.h): the power of two that brings amax into [2^9, 2^10), in fp32 arithmetic"""
    _, e = np.frexp(np.float32(amax))
    e = int(e)
    if clamp:
        e = min(max(e, -100), 100)
    with np.errstate(over='ignore'):
        return np.ldexp(np.float32(1), 10 - e)


def _rel(rep, v):
    return float(np.max(np.abs(rep - v.astype(np.float64))) / np.max(np.abs(v)))


@pytest.fixture(scope='module')
def x():
    return np.random.default_rng(0).standard_normal(1 << 16)


def test_scaled_split_is_flat_from_2_m14_to_2_13(x):
    """randn * 2^k (largest value 4.4 * 2^k): 1.0e-7 of the maximum for every k from -14 to +12, i.e. values up to 2^14.1 --
    22 significant bits wherever hi and the residual are normal fp16 numbers.  Below, the residual times 2048 sinks into the
    fp16 subnormals and the error doubles per step of k; above 65504 hi is inf."""
    flat = [_rel(split_scaled(x * 2.0 ** k), (x * 2.0 ** k).astype(np.float32)) for k in range(-14, 13)]
    assert max(flat) <= 2.0 ** -23 and min(flat) >= 2.0 ** -24, flat
    below = {k: _rel(split_scaled(x * 2.0 ** k), (x * 2.0 ** k).astype(np.float32)) for k in (-16, -20, -26)}
    assert 1.5e-7 < below[-16] < 2.5e-7 and 2.5e-6 < below[-20] < 4e-6 and 1.5e-4 < below[-26] < 2.5e-4, below
    # the declared envelope of the forward (2^-10 ... 2^10) lies inside the flat part with 2^4 / 2^2 to spare, and even 2^-26 is
    # no worse than 2.1e-4 of the operand's maximum
    assert not np.isfinite(split_scaled(np.float32([70000.0]))).all()         # hi = inf, lo = -inf: NaN, no saturation


def test_unscaled_low_part_loses_bits_in_small_channels(x):
    """An output channel of dz that lies 2^j below the tensor's maximum: 6e-8 of the channel's own maximum up to j = 8 (the
    low part is a normal fp16 number), then the low part is a multiple of 2^-24 and the error 2^(j - 35): 1.2e-7 at j = 12,
    2e-6 at j = 16, 3e-5 at j = 20.  22 bits at j = 12 is what the per-channel bound TOL = 1e-4 of the GPU test rests on; the
    accumulated gradient of a channel is a sum over pixels of such values, so its relative error is no larger."""
    top = (x * 1e-7).astype(np.float32)
    s = float(f16_scale(np.max(np.abs(top))))
    assert 2.0 ** 9 <= float(np.max(np.abs(top))) * s < 2.0 ** 10
    err = {}
    for j in (0, 4, 8, 12, 16, 20):
        ch = (top * np.float32(2.0 ** -j)).astype(np.float64) * s
        err[j] = float(np.max(np.abs(split_unscaled(ch) - ch)) / np.max(np.abs(ch)))
    assert all(5.5e-8 < err[j] < 6.5e-8 for j in (0, 4, 8)), err
    assert 1.1e-7 < err[12] < 1.3e-7 and 1.8e-6 < err[16] < 2.1e-6 and 2.9e-5 < err[20] < 3.2e-5, err
    assert err[12] <= 2.0 ** -22                    # "at least 22 significant bits down to 2^-12"


def test_operand_scale_of_a_vanishing_gradient():
    """2^(10 - e) is no fp32 number for a maximum below 2^-117: without the clamp the scale is inf (every staged value inf or
    0 * inf, the low part inf - inf); with it the scale stays finite for every positive fp32 maximum, subnormals included, and is
    unchanged wherever it was finite before and the maximum lies inside [2^-100, 2^100]."""
    for e in (-120, -130, -145):
        assert np.isinf(f16_scale(2.0 ** e, clamp=False)) and np.isfinite(f16_scale(2.0 ** e))
        assert float(f16_scale(2.0 ** e)) == 2.0 ** 110
    for m in (1e-30, 1e-7, 1.0, 3.0e4, 1e30):
        assert f16_scale(m) == f16_scale(m, clamp=False) and 2.0 ** 9 <= m * float(f16_scale(m)) < 2.0 ** 10
