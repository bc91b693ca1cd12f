"""The gated output stage of TriangularUpdate (tgt_edge_gated_out_fwd / _bwd, ops.gated_linear_residual_layer_norm) against
float64 on the values as the kernel sees them, on the GPU.

  z = a w^T + bias = [z_g | z_l];  t = sigmoid(z_g) * z_l;  s = res + row_scale[row / rows_per_sample] * t;  y = LayerNorm(s)
  backward, dt given: dz = [dt z_l sigma (1 - sigma) | dt sigma];  d_a = dz w;  dw = dz^T a;  db = column sums of dz

Shapes: M = 25 (one partial 32-row tile, no row_scale); M = 147 = 3 graphs of 49 rows with DropPath factors [1/0.9, 0, 1/0.9]
(five tiles, two of which straddle two graphs); the same with the grid capped at 2 workgroups (each walks several tiles and
carries its weight-gradient accumulators across them).  K in {16, 32, 64}: every instantiation.  Weight gains 1 and 6 (saturated
gates).  The rows of `res` differ in mean and spread inside every tile: means -5 / 0 / 5 and spreads 0.1 .. 10 for the kernel
test, where y / mean / rstd are held to the float64 LayerNorm of the row AS STORED (the definition of y above and the practice
of tests/test_hip_edge_gemm.py: a 16-bit s at 5 +- 0.1 carries a rounding step of a third of its spread, which no LayerNorm of
the stored row can undo); means -1.5 / 0 / 1.5 and spreads 1 .. 10 for the autograd test, whose reference is float64 end to end
-- there the LayerNorm amplifies the storage rounding of s by rms(s) / std(s) <= 2, which the bars leave room for.

Bars: the project's own 16-bit bars (tests/test_hip_triplet_hard_inputs.py): rel-L2 bf16 8e-3 / fp16 1e-3 for forward
quantities, twice that for gradients.  A CPU simulation of the single rounding of dz gave bf16 1.5-3.0e-3, fp16 2.0-3.6e-4.
profiles/parity_errors_triupd.json records the measured errors (TGT_PARITY_LOG)."""
import ctypes as C

import numpy as np
import pytest
import torch

import parity_log

pytestmark = pytest.mark.gpu

TOL = parity_log.Tol({torch.bfloat16: 8e-3, torch.float16: 1e-3})
BF16, F16 = torch.bfloat16, torch.float16
CH = 256
SCALES = [1 / 0.9, 0.0, 1 / 0.9]
CONFIGS = {'M25': (25, None, 0), 'M147': (147, 49, 0), 'M147cap2': (147, 49, 2)}        # M, rows_per_sample, grid cap
PARAMS = [(c, K, gain, dt) for c in CONFIGS for K in (16, 32, 64) for gain in (1, 6) for dt in (BF16, F16)]


def case_id(v):
    return str(v).replace('torch.', '')


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return parity_log.record(float((a - b).norm() / (b.norm() + 1e-30)))


def check(got, ref, tol, grads, what):
    errs = {k: rel(got[k], ref[k]) for k in ref}
    limit = {k: tol * (2 if k in grads else 1) for k in ref}
    print(what, 'rel-L2', {k: f'{v:.3e}' for k, v in errs.items()}, 'bars', limit)
    for k, t in got.items():
        assert torch.isfinite(t).all(), (what, k, 'not finite')
    bad = {k: (errs[k], limit[k]) for k in ref if not errs[k] < limit[k]}
    assert not bad, (what, bad)


_cache = {}


def make_inputs(M, K, gain, dtype, rps, harsh=True):
    """operands in `dtype` (gamma / beta float32) on the CPU and the float64 results on them; shared, never written to"""
    key = (M, K, gain, dtype, rps, harsh)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(1000 * M + 10 * K + gain)
    rnd = lambda *s: torch.from_numpy(rng.standard_normal(s))
    a = rnd(M, K).to(dtype)
    w = (rnd(2 * CH, K) * (gain / K ** 0.5)).to(dtype)
    bias = (rnd(2 * CH) * 0.5).to(dtype)
    row_mean = torch.from_numpy(rng.choice([-5.0, 0.0, 5.0] if harsh else [-1.5, 0.0, 1.5], M))[:, None]
    row_std = torch.from_numpy(10.0 ** rng.uniform(-1 if harsh else 0, 1, M))[:, None]
    res = (rnd(M, CH) * row_std + row_mean).to(dtype)
    gamma, beta = (1 + 0.3 * rnd(CH)).float(), (0.3 * rnd(CH)).float()
    scale = None if rps is None else torch.tensor(SCALES, dtype=torch.float32)
    row_scale = torch.ones(M, 1, dtype=torch.float64) if rps is None else scale.double()[torch.arange(M) // rps][:, None]
    dt = (rnd(M, CH) * row_scale).to(dtype)              # the gradient at t arrives times row_scale
    eps = 1e-5
    a64, w64, b64, r64, dt64 = a.double(), w.double(), bias.double(), res.double(), dt.double()
    z = a64 @ w64.t() + b64
    zg, zl = z[:, :CH], z[:, CH:]
    sg = torch.sigmoid(zg)
    s = r64 + row_scale * (sg * zl)
    dz = torch.cat((dt64 * zl * sg * (1 - sg), dt64 * sg), dim=1)
    ref_f = dict(s=s)
    ref_b = dict(d_a=dz @ w64, dw=dz.t() @ a64, db=dz.sum(0))
    _cache[key] = (a, w, bias, res, gamma, beta, scale, dt, eps, ref_f, ref_b)
    return _cache[key]


def layer_norm64(s, gamma, beta, eps):
    """float64 (y, mean, rstd) of the LayerNorm of s"""
    s = s.detach().double().cpu()
    mean, var = s.mean(1), s.var(1, unbiased=False)
    rstd = (var + eps).rsqrt()
    return dict(y=(s - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double(), mean=mean, rstd=rstd)


def run_raw(a, w, bias, res, gamma, beta, scale, dt, eps, rps, cap):
    """the two C entries; outputs pre-filled with NaN: every element must be written"""
    from tgt_amd import _lib, ops
    L = _lib.lib()
    M, K = a.shape
    dev = lambda t: None if t is None else t.cuda()
    a, w, bias, res, gamma, beta, scale, dt = map(dev, (a, w, bias, res, gamma, beta, scale, dt))
    nan = lambda *s, dtype=a.dtype: torch.full(s, float('nan'), dtype=dtype, device='cuda')
    s, y, mean, rstd = nan(M, CH), nan(M, CH), nan(M, dtype=torch.float32), nan(M, dtype=torch.float32)
    L.tgt_edge_linear_set_grid_cap(cap)
    try:
        parts = L.tgt_edge_gated_out_parts(M)
        assert parts == (min(cap, (M + 31) // 32) if cap else min((M + 31) // 32, parts))
        g = ops._gated_args(a, w, bias, CH)
        g.res, g.s, g.y, g.gamma, g.beta, g.eps = res.data_ptr(), s.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps
        g.mean, g.rstd = mean.data_ptr(), rstd.data_ptr()
        g.row_scale, g.rows_per_sample = (None if scale is None else scale.data_ptr()), (rps or 0)
        ops._launch('tgt_edge_gated_out_fwd', C.byref(g))
        d_a = nan(M, K)
        dw_part, db_part = nan(parts, 2 * CH, K, dtype=torch.float32), nan(parts, 2 * CH, dtype=torch.float32)
        g.parts, g.dt, g.d_a, g.ld_da, g.dw_partial, g.db_partial = parts, dt.data_ptr(), d_a.data_ptr(), K, dw_part.data_ptr(), db_part.data_ptr()
        ops._launch('tgt_edge_gated_out_bwd', C.byref(g))
        dw = ops.sum_planes(dw_part, torch.empty(2 * CH, K, dtype=torch.float32, device='cuda'), defer=False)
        db = ops.sum_rows(db_part, defer=False)
        torch.cuda.synchronize()
    finally:
        L.tgt_edge_linear_set_grid_cap(0)
    assert torch.isfinite(dw_part).all() and torch.isfinite(db_part).all()          # every plane / row written
    return dict(s=s, y=y, mean=mean, rstd=rstd), dict(d_a=d_a, dw=dw, db=db), parts


@pytest.mark.parametrize('config,K,gain,dtype', PARAMS, ids=case_id)
def test_gated_stage_kernels(config, K, gain, dtype):
    M, rps, cap = CONFIGS[config]
    a, w, bias, res, gamma, beta, scale, dt, eps, ref_f, ref_b = make_inputs(M, K, gain, dtype, rps)
    tol = TOL[dtype]
    fwd, bwd, parts = run_raw(a, w, bias, res, gamma, beta, scale, dt, eps, rps, cap)
    if cap:
        assert parts == cap < (M + 31) // 32              # a workgroup walks several tiles
    what = f'gated stage {config} K={K} gain={gain} {dtype}'
    check(dict(s=fwd['s']), ref_f, tol, (), what + ' fwd')
    check({k: fwd[k] for k in ('y', 'mean', 'rstd')}, layer_norm64(fwd['s'], gamma, beta, eps), tol, (), what + ' LayerNorm of s as stored')
    check(bwd, ref_b, tol, ('d_a', 'dw', 'db'), what + ' bwd')
    if rps is not None:
        dropped = slice(rps, 2 * rps)                     # the graph whose DropPath factor is 0
        assert torch.equal(fwd['s'][dropped].cpu(), res[dropped]), 's != res where the factor is 0'
        assert (bwd['d_a'][dropped] == 0).all()
    fwd2, bwd2, _ = run_raw(a, w, bias, res, gamma, beta, scale, dt, eps, rps, cap)
    for got, again in ((fwd, fwd2), (bwd, bwd2)):
        for k in got:
            assert torch.equal(got[k], again[k]), (k, 'two runs differ')


def test_the_grid_cap_changes_no_forward_bit():
    """the persistent walk (2 workgroups over 5 tiles) gives the rows the bits of one workgroup per tile"""
    M, rps, _ = CONFIGS['M147']
    args = make_inputs(M, 32, 1, BF16, rps)[:9]
    f0, b0, _ = run_raw(*args, rps, 0)
    f2, b2, _ = run_raw(*args, rps, 2)
    for k in f0:
        assert torch.equal(f0[k], f2[k]), k
    assert torch.equal(b0['d_a'], b2['d_a'])


@pytest.mark.parametrize('K,gain,dtype,fused', [(K, gain, dt, f) for K in (16, 32, 64) for gain in (1, 6) for dt in (BF16, F16)
                                                for f in (True, False)], ids=case_id)
def test_gated_linear_residual_layer_norm_through_autograd(K, gain, dtype, fused, monkeypatch):
    """ops.gated_linear_residual_layer_norm under autocast with float32 parameters, fused launch and composition, against float64
    autograd of the formula on the operands as the kernels see them (parameters rounded to the compute dtype)"""
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_TRIUPD_GATED', fused)
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)
    B, N = 3, 7
    M = B * N * N
    a, w, bias, res, gamma, beta, scale, _, eps, _, _ = make_inputs(M, K, gain, dtype, N * N, harsh=False)
    rng = np.random.default_rng(7 + K + gain)
    gs, gy = (torch.from_numpy(rng.standard_normal((B, N, N, CH))).to(dtype) for _ in range(2))
    leaf = lambda t: t.cuda().requires_grad_(True)
    va, res_d = leaf(a.view(B, N, N, K)), leaf(res.view(B, N, N, CH))
    w_p, b_p, g_p, be_p = leaf(w.float()), leaf(bias.float()), leaf(gamma), leaf(beta)
    prof = ops.profile_kernels(True)
    try:
        with torch.autocast('cuda', dtype=dtype):
            s, y = ops.gated_linear_residual_layer_norm(va, w_p, b_p, res_d, scale.cuda(), g_p, be_p, eps)
        assert s.dtype == dtype and y.dtype == dtype
        ((s.float() * gs.cuda().float()).sum() + (y.float() * gy.cuda().float()).sum()).backward()
        torch.cuda.synchronize()
    finally:
        ops.profile_kernels(False)
    assert ({'tgt_edge_gated_out_fwd', 'tgt_edge_gated_out_bwd'} <= set(prof)) == fused
    got = dict(s=s.detach(), y=y.detach(), d_va=va.grad, d_res=res_d.grad, dw=w_p.grad, db=b_p.grad, dgamma=g_p.grad, dbeta=be_p.grad)
    # float64 autograd
    leaf64 = lambda t: t.double().requires_grad_(True)
    va64, res64, w64, b64, g64, be64 = map(leaf64, (a.view(B, N, N, K), res.view(B, N, N, CH), w, bias, gamma, beta))
    z = va64 @ w64.t() + b64
    t = torch.sigmoid(z[..., :CH]) * z[..., CH:]
    s64 = res64 + scale.double().view(B, 1, 1, 1) * t
    y64 = torch.nn.functional.layer_norm(s64, (CH,), g64, be64, eps)
    ((s64 * gs.double()).sum() + (y64 * gy.double()).sum()).backward()
    ref = dict(s=s64.detach(), y=y64.detach(), d_va=va64.grad, d_res=res64.grad, dw=w64.grad, db=b64.grad, dgamma=g64.grad, dbeta=be64.grad)
    check(got, ref, TOL[dtype], ('d_va', 'd_res', 'dw', 'db', 'dgamma', 'dbeta'),
          f'gated_linear_residual_layer_norm K={K} gain={gain} {dtype} {"fused" if fused else "composed"}')
    assert torch.equal(s.detach()[1].cpu(), res.view(B, N, N, CH)[1]) and (va.grad[1] == 0).all()      # the dropped graph
