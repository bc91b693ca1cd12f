"""Pins tests/act_hard_inputs.py on the CPU: over the whole sweep, a float32 numpy restatement of every csrc/act.hpp formula and
torch's own eager float32 evaluation both stay inside the per-element bars -- so the bars are reachable by a float32 evaluation,
and the ELU form chosen does not cancel (the cancelling form exp(x) - 1, as a negative control, misses them)."""
import numpy as np
import pytest
import torch

import act_hard_inputs as ah

SWEEPS = [torch.bfloat16, torch.float16, torch.float32]


def _sweep(dtype):
    x = ah.activation_sweep(dtype)
    return x, ah.cycle(x.shape, dtype=dtype), ah.sweep_valid(x)


@pytest.fixture(scope='module', params=SWEEPS, ids=['bf16', 'f16', 'f32'])
def sweep(request):
    x, dy, valid = _sweep(request.param)
    return request.param, x, dy, valid, {kind: ah.act_case(x, dy, kind) for kind in ah.KINDS}


def test_sweep_holds_every_finite_pattern_and_the_cycle():
    for dtype in (torch.bfloat16, torch.float16):
        x, dy, valid = _sweep(dtype)
        assert x.shape == (256, 256) and x.dtype == dtype
        bits = x.view(torch.int16).reshape(-1).numpy().view(np.uint16)
        finite = torch.isfinite(torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16)).view(dtype))
        assert set(bits.tolist()) == set(np.arange(65536)[finite.numpy()].tolist())
        assert sorted(set(dy.float().reshape(-1).tolist())) == sorted(ah.CYCLE)
        assert torch.equal(dy.reshape(-1)[:3].double(), torch.tensor(ah.CYCLE, dtype=torch.float64))


@pytest.mark.parametrize('kind', ah.KINDS)
def test_restatement_and_eager_float32_stay_inside_the_bars(sweep, kind):
    """the values are held to the bars of FLOAT32 storage (the tightest: h = 2^-24 |ref|), whatever type the sweep's inputs have"""
    dtype, x, dy, valid, cases = sweep
    xs = x.float().numpy()
    new = {'y': ah.act_fwd32(xs, kind), 'dx': dy.float().numpy() * ah.act_grad32(xs, kind)}
    for name, (eager, ref, s) in cases[kind].items():
        floor = ah.FLOOR[(kind, name)]
        tag = f'{kind} {name} ({dtype})'
        assert ah.act_ratio(tag + ' restatement', torch.from_numpy(new[name]), ref, s, torch.float32, floor, valid) <= 1.0
        assert ah.act_ratio(tag + ' eager', eager, ref, s, torch.float32, floor, valid) <= 1.0


def test_relu_restatement_is_exact_and_keeps_nan():
    x = ah.activation_sweep(torch.float32).numpy()
    assert np.array_equal(ah.act_fwd32(x, 'relu'), torch.relu(torch.from_numpy(x)).numpy())
    assert np.isnan(ah.act_fwd32(np.array([np.nan, 1.0], dtype=np.float32), 'relu')[0])
    assert ah.act_grad32(np.zeros(1, dtype=np.float32), 'relu')[0] == 0            # the derivative at 0 is 0


def test_cancelling_elu_form_misses_the_float16_storage_bar():
    """exp(x) - 1 evaluated in float32 everywhere is outside the bar of the fp16 sweep (its error near x = -2^-14 is 2^-24, where an
    fp16 result is held to 2^-25 plus the floor), and far outside once the same values are held to float32 storage: the sweep tells
    the two forms apart"""
    x, dy, valid = _sweep(torch.float16)
    _, ref, s = ah.act_case(x, dy, 'elu')['y']
    bad = torch.from_numpy(ah.act_fwd32(x.float().numpy(), 'elu', series_below=0.0))
    good = torch.from_numpy(ah.act_fwd32(x.float().numpy(), 'elu'))
    assert ah.act_ratio('elu y, exp(x) - 1', bad, ref, s, torch.float16, ah.FLOOR[('elu', 'y')], valid) > 1.5
    assert ah.act_ratio('elu y, exp(x) - 1, float32 storage', bad, ref, s, torch.float32, ah.FLOOR[('elu', 'y')], valid) > 100.0
    assert ah.act_ratio('elu y, act.hpp form', good, ref, s, torch.float16, ah.FLOOR[('elu', 'y')], valid) <= 1.0


def test_keep_pattern_restatement_is_a_fair_generator():
    keep = ah.keep_pattern_np(1 << 18, 2, 0.25, 0xabcdef)
    assert abs(keep.mean() - 0.75) <= 0.0043                      # 5 binomial standard deviations of 262144 draws
    assert not np.array_equal(keep, ah.keep_pattern_np(1 << 18, 2, 0.25, 0xabcdef, counter=1))
    assert np.array_equal(ah.keep_pattern_np(64, 4, 0.0, 1), np.ones(64, dtype=bool))
