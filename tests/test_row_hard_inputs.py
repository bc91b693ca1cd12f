"""tests/row_hard_inputs.py on the CPU: the inputs have the properties their docstrings claim, torch's own float32 composition
(rounded to the storage type) stays inside every bar against float64 -- so the bars can be met by the reference alone -- and the
two mutants of profiles/row_hard_inputs_mutant_check.txt, restated in torch, do NOT."""

import numpy as np
import pytest
import torch

import row_hard_inputs as rh

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ['f32', 'bf16', 'f16']


# ---------------------------------------------------------------------------------------------------------------
# A
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,finite', [(torch.bfloat16, 65280), (torch.float16, 63488)], ids=['bf16', 'f16'])
def test_every_finite_pattern_exactly_once(dtype, finite):
    x = rh.finite_patterns(dtype)
    assert x.shape == (65536,) and torch.isfinite(x).all()
    bits = x.view(torch.int16).numpy().view(np.uint16)
    every = torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16)).view(dtype)
    want = np.arange(65536, dtype=np.uint16)[torch.isfinite(every).numpy()]
    assert len(want) == finite
    assert np.array_equal(np.unique(bits), want)                       # every finite pattern ...
    counts = np.bincount(bits, minlength=65536)
    assert counts[0] == 1 + 65536 - finite and np.all(counts[want[1:]] == 1)        # ... once; +0 also stands in for the rest
    valid = rh.sweep_valid(x)
    assert int((~valid).sum()) == (254 if dtype == torch.bfloat16 else 0)           # fp16 subnormals are normal float32 numbers
    assert float(x.float().abs().max()) == float(torch.finfo(dtype).max)
    assert bool(torch.signbit(x[x == 0]).any())                         # -0 is in


def test_float32_sweep():
    x = rh.activation_sweep(torch.float32)
    assert x.shape == (833, 256) and x.dtype == torch.float32
    flat = x.reshape(-1)
    n = 65536 + 16385 + 2 * 65536
    assert torch.all(flat[n:] == 0) and flat.numel() - n < 256
    grid = flat[65536:65536 + 16385]
    assert float(grid[0]) == -8 and float(grid[-1]) == 8 and torch.all(grid[1:] - grid[:-1] == 2.0 ** -10)
    mag = flat[65536 + 16385:65536 + 16385 + 65536]
    assert 2.0 ** -20 < float(mag.min()) < 2.0 ** -19.99 and 2.0 ** 3.99 < float(mag.max()) < 2.0 ** 4
    assert torch.equal(flat[n - 65536:n], -mag)
    rh.sweep_valid(x)


def test_cycle_and_storage_rounding():
    c = rh.cycle((2, 6))
    assert c.reshape(-1).tolist() == [1.0, -0.75, 3.0] * 4
    assert rh.cycle((2, 4), by_column=True)[1].tolist() == [1.0, -0.75, 3.0, 1.0]
    assert rh.cycle((3,), shift=1).tolist() == [-0.75, 3.0, 1.0]
    # h bounds the rounding of any float64 into the type (half an ulp is 2^-9 / 2^-12 / 2^-25 relative)
    g = torch.Generator().manual_seed(0)
    v = torch.randn(4096, generator=g, dtype=torch.float64) * torch.exp2(torch.randint(-20, 15, (4096,), generator=g).double())
    for dtype in DTYPES:
        assert torch.all((v.to(dtype).double() - v).abs() <= rh.storage_h(v, dtype))


def _rounded(t, dtype, ref=None):
    """torch's float32 result as stored (where float32 itself overflowed -- elementwise_ratio counts those --, the reference)"""
    if ref is not None:
        t = torch.where(torch.isfinite(t), t, ref.float())
    return t.to(dtype)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_eager_float32_gelu_is_inside_the_bars_and_the_mutant_is_not(dtype):
    x = rh.activation_sweep(dtype)
    valid = rh.sweep_valid(x)
    dy = rh.cycle(x.shape).to(dtype)
    case = rh.gelu_case(x, dy)
    for name in ('y', 'dx'):
        eager, ref, s = case[name]
        ratio, E = rh.elementwise_ratio(f'gelu {name}', _rounded(eager, dtype, ref), eager, ref, s, dtype, rh.FLOOR['gelu', name], valid,
                                        signed_zero=name == 'y')
        assert ratio < 1, (name, ratio)
    # mutant 1: Phi(v) = 0 for v < -4.5
    eager, ref, s = case['y']
    mutant = torch.where(x.float() < -4.5, x.float() * 0.0, eager)
    ratio, _ = rh.elementwise_ratio('gelu y, mutant', _rounded(mutant, dtype, ref), eager, ref, s, dtype, rh.FLOOR['gelu', 'y'], valid)
    assert ratio > 1, ratio


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('kind', rh.KINDS)
def test_eager_float32_glu_is_inside_the_bars(kind, dtype):
    g = rh.activation_sweep(dtype)
    valid = rh.sweep_valid(g)
    e, dy = rh.cycle(g.shape).to(dtype), rh.cycle(g.shape, shift=1).to(dtype)
    case = rh.glu_case(g, e, dy, kind)
    for name in ('y', 'd_g', 'd_e'):
        eager, ref, s = case[name]
        ratio, E = rh.elementwise_ratio(f'{kind} {name}', _rounded(eager, dtype, ref), eager, ref, s, dtype, rh.FLOOR[kind, name], valid,
                                        signed_zero=name == 'y')
        assert ratio < 1, (name, ratio)
    if kind == 'geglu':
        eager, ref, s = case['y']
        mutant = torch.where(g.float() < -4.5, eager * 0.0, eager)
        ratio, _ = rh.elementwise_ratio('geglu y, mutant', _rounded(mutant, dtype, ref), eager, ref, s, dtype, rh.FLOOR[kind, 'y'], valid)
        assert ratio > 1, ratio


def test_saturated_references_are_told_apart():
    """3 * gelu(3.4e38) has no finite bf16 rounding: the infinity of the right sign passes, a finite value or the wrong sign does not"""
    x = rh.activation_sweep(torch.bfloat16)
    valid = rh.sweep_valid(x)
    case = rh.glu_case(x, rh.cycle(x.shape).to(torch.bfloat16), rh.cycle(x.shape, shift=1).to(torch.bfloat16), 'geglu')
    eager, ref, s = case['y']
    sat = ref.abs() > float(torch.finfo(torch.bfloat16).max)
    assert 0 < int(sat.sum()) < 400
    good = _rounded(eager, torch.bfloat16, ref)
    assert torch.isinf(good[sat]).all()
    rh.elementwise_ratio('sat', good, eager, ref, s, torch.bfloat16, rh.FLOOR['geglu', 'y'], valid)
    for bad in (torch.where(sat, torch.ones_like(good), good), torch.where(sat, -good, good)):
        with pytest.raises(AssertionError, match='saturated'):
            rh.elementwise_ratio('sat', bad, eager, ref, s, torch.bfloat16, rh.FLOOR['geglu', 'y'], valid)


# ---------------------------------------------------------------------------------------------------------------
# B
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_structured_rows_properties(dtype):
    M, C = 77, 64
    x = rh.structured_rows(M, C, dtype)
    kinds = rh.row_kinds(dtype)
    assert x.shape == (M, C) and x.dtype == dtype and torch.isfinite(x).all()
    assert M % 32 and 1003 % 32 and len(kinds) < 32                    # every kind inside the first tile; a tail tile
    ref = rh.ln_reference(x, *rh.ln_params(C), 1e-5)
    tile = ref['rstd'][:32]
    assert float(tile.max() / tile.min()) > 1e4                        # neighbours in one tile: orders of magnitude apart
    for r, kind in enumerate(kinds):
        if kind[0] in ('const', 'zero'):
            assert float(x[r].double().var(unbiased=False)) == 0 and abs(float(ref['rstd'][r]) - 1e-5 ** -0.5) < 1e-9
        if kind[0] == 'zero':
            assert torch.all(x[r] == 0)
        if kind[0] == 'outlier':
            assert int((x[r].double().abs() > 5e3).sum()) == 1
        if kind[0] == 'alternating':
            assert float(x[r].double().sum()) == 0 and float(x[r].double().abs().min()) >= 3e4
        if kind[0] == 'edge':
            assert float(x[r].double().abs().min()) > 5.9e4
    means = ref['mean'][:len(kinds)]
    assert float(means.max()) >= 999 and float(means.min()) <= -999


def _tile_rstd_mutant(x, gamma, beta, eps):
    """mutant 2 in torch: a row takes the rstd of the first row of its 32-row tile"""
    r = rh.ln_reference(x, gamma, beta, eps, dt=torch.float32)
    first = (torch.arange(x.shape[0]) // 32) * 32
    rstd = r['rstd'][first]
    return dict(y=(x.float() - r['mean'][:, None]) * rstd[:, None] * gamma + beta, mean=r['mean'], rstd=rstd)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('M,C', [(77, 64), (77, 768), (1003, 256)])
def test_eager_float32_layer_norm_is_inside_the_bars_and_the_mutant_is_not(M, C, dtype):
    x = rh.structured_rows(M, C, dtype)
    gamma, beta = rh.ln_params(C)
    dy = torch.randn(M, C, generator=torch.Generator().manual_seed(M + C)).to(dtype)
    ref = rh.ln_reference(x, gamma, beta, 1e-5, dy)
    eager = rh.ln_eager32(x, gamma, beta, 1e-5, dy)
    new = dict(y=eager['y'].to(dtype), mean=eager['mean'], rstd=eager['rstd'])
    ratios = rh.ln_forward_ratios('ln', x, gamma, new, ref, eager, dtype)
    assert max(ratios.values()) < 1, ratios
    bar = rh.ln_backward_row_bar(x, ref, eager['dx'], dtype)
    assert rh._worst('ln dx', (eager['dx'].to(dtype).double() - ref['dx']).norm(dim=-1), bar) < 1
    terms = dy.double() * ref['xhat']
    assert rh._worst('ln dgamma', (eager['dgamma'].double() - ref['dgamma']).abs(),
                     rh.column_sum_bar(terms, extra=rh.ln_dgamma_extra(x, dy, ref))) < 1
    assert rh._worst('ln dbeta', (eager['dbeta'].double() - ref['dbeta']).abs(), rh.column_sum_bar(dy)) < 1
    # the conditioning term is a statement about the input, not a blank cheque: on the plain rows (m = 0, s = 1) it is small
    plain = [r for r in range(M) if rh.row_kinds(dtype)[r % len(rh.row_kinds(dtype))] == ('offset', 0.0, 1.0)]
    cond = rh.ln_delta(x) * ref['rstd'] * float(gamma.double().norm())
    assert float((cond / ref['y'].norm(dim=-1))[plain].max()) < 1e-5
    mut = _tile_rstd_mutant(x, gamma, beta, 1e-5)
    mut['y'] = mut['y'].to(dtype)
    ratios = rh.ln_forward_ratios('ln mutant', x, gamma, mut, ref, eager, dtype)
    assert ratios['y'] > 1 and ratios['rstd'] > 1 and ratios['mean'] < 1, ratios


# ---------------------------------------------------------------------------------------------------------------
# C
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('rows,C', rh.XENT_SHAPES)
def test_cross_entropy_rows_inputs_and_eager(rows, C, dtype):
    x, target, w = rh.xent_rows(rows, C, dtype)
    assert x.shape == (rows, C) and torch.isfinite(x).all() and int(target[0]) == 0 and int(target[-1]) == C - 1
    assert 0 <= int(target.min()) and int(target.max()) < C and 0 < int((w == 0).sum()) < rows
    xd = x.double()
    top2 = xd.topk(2, -1).values
    r = torch.arange(rows)
    assert torch.all((top2[:, 0] - top2[:, 1])[(r % 7 == 1) | (r % 7 == 2)] >= 50)
    inner = (r > 0) & (r < rows - 1)
    on, off_ = inner & (r % 7 == 1), inner & (r % 7 == 2)
    assert torch.all(xd.argmax(-1)[on] == target[on]) and torch.all(xd.argmax(-1)[off_] != target[off_])
    assert torch.all(xd[r % 7 == 3] == 0.5)
    off = rh.XENT_OFFSET[dtype]
    assert torch.all(xd[r % 7 == 4] > off - 100) and torch.all(xd[r % 7 == 5] < -off + 100)
    lo = float(torch.finfo(dtype).min)
    assert torch.all((xd[r % 7 == 6] == lo).sum(-1) >= 1)
    assert float(rh.xent_magnitude(x)[r % 7 == 6].max()) < 10            # the floor of those rows is not set by finfo.min
    case = rh.xent_case(x, target, w)
    e = case['eager']
    new = dict(xent=e['xent'], lse=e['lse'], grad=e['grad'].to(dtype))
    ratios = rh.xent_ratios('xent', x, w, new, case, dtype)
    assert max(ratios.values()) < 1, ratios


def test_a_rounded_log_sum_exp_misses_the_gradient_bar():
    """Why the backward kernel must not rebuild the softmax from a saved float32 log-sum-exp: at a common offset of 1e4 that number
    is rounded to 2^-10, and exp(x - lse) carries the whole rounding."""
    rows, C = 513, 40
    x, target, w = rh.xent_rows(rows, C, torch.float32)
    case = rh.xent_case(x, target, w)
    e = case['eager']
    grad = w[:, None] * (torch.exp(x - e['lse'][:, None]) - torch.nn.functional.one_hot(target, C))
    ratios = rh.xent_ratios('xent from lse', x, w, dict(xent=e['xent'], lse=e['lse'], grad=grad), case, torch.float32)
    assert ratios['grad'] > 1 and ratios['lse'] < 1, ratios
    # ... and what tgt_cross_entropy_bwd does instead: lse as the offset only, the row normalised by its own sum
    e_ = torch.exp(x - e['lse'][:, None])
    grad = w[:, None] * (e_ / e_.sum(-1, keepdim=True) - torch.nn.functional.one_hot(target, C))
    ratios = rh.xent_ratios('xent renormalised', x, w, dict(xent=e['xent'], lse=e['lse'], grad=grad), case, torch.float32)
    assert ratios['grad'] < 1, ratios


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('K', rh.GAUSS_KS)
def test_gaussian_basis_inputs_and_eager(K, dtype):
    x, mul, bias, means, stds = rh.gaussian_inputs(K)
    assert x.numel() == 4608 and int((stds == 0).sum()) >= 1 and float(stds.min()) < 0 and float(stds.abs()[stds != 0].min()) < 2e-3
    gy = torch.randn(*x.shape, K, generator=torch.Generator().manual_seed(K)).to(dtype)
    ref = rh.gaussian_case(x, mul, bias, means, stds, gy, torch.float64)
    eager = rh.gaussian_case(x, mul, bias, means, stds, gy, torch.float32)
    assert float((ref['y'] == 0).double().mean()) > 0.01                # exp underflows somewhere
    new = dict(eager, y=eager['y'].to(dtype))
    ratios = rh.gaussian_ratios('gauss', new, ref, eager, dtype, x)
    assert max(ratios.values()) < 1, ratios
    assert torch.all(ref['dstds'][stds == 0] == 0)
    assert all(torch.isfinite(v).all() for v in eager.values())
