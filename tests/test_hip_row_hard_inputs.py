"""The activation, normalisation and loss row kernels -- the streaming kernels and the fused epilogues of the edge-row GEMMs -- held
to float64 per element / per row on the inputs of tests/row_hard_inputs.py (the bars and their derivations are there; the same
helper is pinned on the CPU by tests/test_row_hard_inputs.py):

  A  every finite 16-bit input of GELU / geglu / glu / swiglu, forward and backward, through tgt_gelu_dropout_*, tgt_glu_dropout_* and
     (bit for bit the same pre-activations, through an identity weight) TGT_EPI_GELU, TGT_EPI_GELU_BWD, TGT_EPI_GLU
  B  LayerNorm rows whose neighbours inside one 32-row tile differ by orders of magnitude: ops.layer_norm, ops.add_layer_norm,
     TGT_EPI_RESID + LayerNorm, TGT_EPI_LN_BWD, and their column sums
  C  ops.cross_entropy_rows on peaked / flat / offset rows, ops.gaussian_basis with sigma down to 0.01 and a second grid trip

Every ratio err / bar is filed in the parity log (TGT_PARITY_LOG, group `rows`; profiles/parity_errors_row_hard_inputs.json);
profiles/row_hard_inputs_mutant_check.txt records which mutants this file sees and the older files do not."""
import functools

import pytest
import torch

import parity_log
import row_hard_inputs as rh

from tgt_amd import _lib, ops

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ['f32', 'bf16', 'f16']
DT16 = [torch.bfloat16, torch.float16]
IDS16 = ['bf16', 'f16']


def file_ratio(name, ratio):
    parity_log.Tol.last = 'rows'
    parity_log.record(ratio)
    assert ratio <= 1, (name, ratio)


def check_elementwise(tag, case, names, new, dtype, valid, kind):
    for name in names:
        eager, ref, s = case[name]
        ratio, e_new = rh.elementwise_ratio(f'{tag} {name}', new[name], eager, ref, s, dtype, rh.FLOOR[kind, name], valid,
                                            signed_zero=name == 'y')
        file_ratio(f'{tag} {name}', ratio)
        if dtype == torch.float32:          # the float32 evaluation itself, free of storage rounding: the largest err / s
            parity_log.Tol.last = f'err_over_s {tag} {name}'
            parity_log.record(e_new)


@functools.lru_cache(maxsize=None)
def sweep(dtype):
    x = rh.activation_sweep(dtype).cuda()
    return x, rh.sweep_valid(x)


def bit_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------
# A. activations
# ---------------------------------------------------------------------------------------------------------------
def gelu_fwd(x):
    y = torch.empty_like(x)
    _lib.check(_lib.lib().tgt_gelu_dropout_fwd(x.data_ptr(), y.data_ptr(), x.numel(), ops._DT[x.dtype], 0.0, 0, None), 'tgt_gelu_dropout_fwd')
    return y


def gelu_bwd(x, dy):
    dx = torch.empty_like(x)
    _lib.check(_lib.lib().tgt_gelu_dropout_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), ops._DT[x.dtype], 0.0, 0, None),
               'tgt_gelu_dropout_bwd')
    return dx


def glu_fwd(x, kind):
    rows, cols = x.shape[0], x.shape[1] // 2
    y = torch.empty(rows, cols, dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().tgt_glu_dropout_fwd(x.data_ptr(), y.data_ptr(), rows, cols, _lib.GLU_KINDS[kind], ops._DT[x.dtype], 0.0, 0,
                                              None, 0, None), 'tgt_glu_dropout_fwd')
    return y


def glu_bwd(x, dy, kind):
    rows, cols = x.shape[0], x.shape[1] // 2
    dx = torch.empty_like(x)
    _lib.check(_lib.lib().tgt_glu_dropout_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), rows, cols, _lib.GLU_KINDS[kind],
                                              ops._DT[x.dtype], 0.0, 0, None, 0, None), 'tgt_glu_dropout_bwd')
    return dx


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_gelu_streaming_kernels_over_the_whole_domain(dtype):
    x, valid = sweep(dtype)
    dy = rh.cycle(x.shape).to(dtype).cuda()
    new = dict(y=gelu_fwd(x), dx=gelu_bwd(x, dy))
    torch.cuda.synchronize()
    check_elementwise('gelu', rh.gelu_case(x, dy), ('y', 'dx'), new, dtype, valid, 'gelu')


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('kind', rh.KINDS)
def test_glu_streaming_kernels_over_the_whole_domain(kind, dtype):
    g, valid = sweep(dtype)
    e, dy = rh.cycle(g.shape).to(dtype).cuda(), rh.cycle(g.shape, shift=1).to(dtype).cuda()
    x = torch.cat([g, e], dim=-1).contiguous()
    y, dx = glu_fwd(x, kind), glu_bwd(x, dy, kind)
    torch.cuda.synchronize()
    cols = g.shape[1]
    new = dict(y=y, d_g=dx[:, :cols], d_e=dx[:, cols:])
    check_elementwise(kind, rh.glu_case(g, e, dy, kind), ('y', 'd_g', 'd_e'), new, dtype, valid, kind)


def through_identity(x, valid, got):
    """the pre-activation an identity weight hands the epilogue: the sweep bit for bit -- except that the GEMM's sum starts from +0,
    so the one -0 comes out as +0 (x + 0 in IEEE arithmetic).  Inputs below the smallest normal float32 are not asserted."""
    want = torch.where(x == 0, torch.zeros_like(x), x)
    assert bit_equal(torch.where(valid, got, want), want)


@pytest.mark.parametrize('dtype', DT16, ids=IDS16)
def test_gelu_epilogue_over_the_whole_domain(dtype):
    """TGT_EPI_GELU on W = I (K = N = 256), no bias: out2 is the sweep, out its GELU"""
    x, valid = sweep(dtype)
    w = torch.eye(256, dtype=dtype, device='cuda')
    pre = torch.empty_like(x)
    out = ops.edge_linear_raw(x, w, None, _lib.EPI_GELU, out2=pre)
    torch.cuda.synchronize()
    through_identity(x, valid, pre)
    dy = rh.cycle(x.shape).to(dtype).cuda()
    check_elementwise('EPI_GELU', rh.gelu_case(pre, dy), ('y',), dict(y=out), dtype, valid, 'gelu')


@pytest.mark.parametrize('dtype', DT16, ids=IDS16)
def test_gelu_backward_epilogue_over_the_whole_domain(dtype):
    """TGT_EPI_GELU_BWD: a = the dy cycle through W = I (exact: every value of the cycle is a 16-bit number), res = the sweep"""
    x, valid = sweep(dtype)
    w = torch.eye(256, dtype=dtype, device='cuda')
    dy = rh.cycle(x.shape).to(dtype).cuda()
    out = ops.edge_linear_raw(dy, w, None, _lib.EPI_GELU_BWD, res=x)
    torch.cuda.synchronize()
    check_elementwise('EPI_GELU_BWD', rh.gelu_case(x, dy), ('dx',), dict(dx=out), dtype, valid, 'gelu')


@pytest.mark.parametrize('dtype', DT16, ids=IDS16)
@pytest.mark.parametrize('kind', rh.KINDS)
def test_glu_epilogue_over_the_whole_domain(kind, dtype):
    """TGT_EPI_GLU on the 256 -> 512 Linear with weight [I; 0] and bias [0; e0]: g = the sweep, e = e0 (the cycle, by column)"""
    g, valid = sweep(dtype)
    w = torch.cat([torch.eye(256), torch.zeros(256, 256)]).to(dtype).cuda()
    e0 = rh.cycle((256,)).to(dtype).cuda()
    bias = torch.cat([torch.zeros(256, dtype=dtype, device='cuda'), e0])
    out2 = torch.empty(g.shape[0], 512, dtype=dtype, device='cuda')
    out = torch.empty(g.shape[0], 256, dtype=dtype, device='cuda')
    ops.edge_linear_raw(g, w, bias, _lib.EPI_GLU, out=out, out2=out2, flags=_lib.GLU_KINDS[kind] << _lib.EDGE_GLU_KIND_SHIFT)
    torch.cuda.synchronize()
    through_identity(g, valid, out2[:, :256])
    e = e0.expand(g.shape[0], 256).contiguous()
    assert torch.equal(out2[:, 256:], e)
    dy = rh.cycle(g.shape, shift=1).to(dtype).cuda()
    check_elementwise(f'EPI_GLU {kind}', rh.glu_case(out2[:, :256], e, dy, kind), ('y',), dict(y=out), dtype, valid, kind)


# ---------------------------------------------------------------------------------------------------------------
# B. LayerNorm rows with structure
# ---------------------------------------------------------------------------------------------------------------
LN_SHAPES = [(77, 64), (77, 256), (77, 768), (1003, 64), (1003, 256), (1003, 768)]
EPI_SHAPES = [(77, 64), (77, 256), (1003, 64), (1003, 256)]
SAMPLES = {77: 7, 1003: 17}              # whole samples of 11 / 59 rows


def _dy(M, C, dtype, seed):
    return torch.randn(M, C, generator=torch.Generator().manual_seed(M * C + seed)).to(dtype).cuda()


def check_columns(tag, x, dy, ref, eager, dgamma, dbeta, given_stats=False):
    terms = dy.double() * ref['xhat']
    e_g = None if eager is None else eager['dgamma'].double() - ref['dgamma']
    e_b = None if eager is None else eager['dbeta'].double() - ref['dbeta']
    file_ratio(f'{tag} dgamma', rh._worst(f'{tag} dgamma', (dgamma.double() - ref['dgamma']).abs(),
                                          rh.column_sum_bar(terms, e_g, rh.ln_dgamma_extra(x, dy, ref, given_stats))))
    file_ratio(f'{tag} dbeta', rh._worst(f'{tag} dbeta', (dbeta.double() - ref['dbeta']).abs(), rh.column_sum_bar(dy, e_b)))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('M,C', LN_SHAPES)
def test_layer_norm_structured_rows(M, C, dtype):
    x = rh.structured_rows(M, C, dtype).cuda()
    gamma, beta = rh.ln_params(C, 'cuda')
    dy = _dy(M, C, dtype, 1)
    ref = rh.ln_reference(x, gamma, beta, 1e-5, dy)
    eager = rh.ln_eager32(x, gamma, beta, 1e-5, dy)
    xg, wg, bg = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = ops.layer_norm(xg, wg, bg, 1e-5, out_dtype=dtype)
    mean, rstd = y.grad_fn.saved_tensors[2:4]
    y.backward(dy)
    torch.cuda.synchronize()
    for k, r in rh.ln_forward_ratios('layer_norm', x, gamma, dict(y=y, mean=mean, rstd=rstd), ref, eager, dtype).items():
        file_ratio(f'layer_norm {k}', r)
    bar = rh.ln_backward_row_bar(x, ref, eager['dx'], dtype)
    file_ratio('layer_norm dx', rh._worst('layer_norm dx', (xg.grad.double() - ref['dx']).norm(dim=-1), bar))
    check_columns('layer_norm', x, dy, ref, eager, wg.grad, bg.grad)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('M,C', LN_SHAPES)
def test_add_layer_norm_structured_rows(M, C, dtype):
    """s = res + scale_b x with a per-sample scale that is 0 for one sample, y = LayerNorm(s as stored); backward with a stream
    gradient ds: d_res = ds + LN_bwd(dy), d_x = scale_b d_res (the stored d_res times the factor, stored: two roundings).  The
    factors stay at or below 1: the fp16 rows next to 65504 have no room for more."""
    B = SAMPLES[M]
    rows = rh.structured_rows(M, C, dtype).cuda()
    half = (rows.double() / 2).to(dtype)
    x, res = half.view(B, M // B, C), (rows.double() - half.double()).to(dtype).view(B, M // B, C)
    scale = torch.tensor([1.0, 0.0, 0.75, 0.5], device='cuda').repeat(5)[:B].contiguous()
    gamma, beta = rh.ln_params(C, 'cuda')
    dy, ds = _dy(M, C, dtype, 2), _dy(M, C, dtype, 3)
    xg, rg = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
    wg, bg = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    s, y = ops.add_layer_norm(xg, rg, scale, wg, bg, 1e-5, out_dtype=dtype)
    mean, rstd = s.grad_fn.saved_tensors[2:4]
    torch.autograd.backward([s, y], [ds.view_as(s), dy.view_as(y)])
    torch.cuda.synchronize()
    sc = scale.double().repeat_interleave(M // B)[:, None]
    # the stream: two float32 roundings (the product, the sum) and the storage rounding
    s64 = res.double().view(M, C) + x.double().view(M, C) * sc
    s_bar = rh.storage_h(s64, dtype) + 2 * rh.U32 * (res.double().view(M, C).abs() + (x.double().view(M, C) * sc).abs())
    file_ratio('add_layer_norm s', rh._worst('add_layer_norm s', (s.double().view(M, C) - s64).abs().reshape(-1), s_bar.reshape(-1)))
    # LayerNorm of the stream AS STORED
    st = s.detach().view(M, C)
    ref = rh.ln_reference(st, gamma, beta, 1e-5, dy)
    eager = rh.ln_eager32(st, gamma, beta, 1e-5, dy)
    new = dict(y=y.detach().view(M, C), mean=mean, rstd=rstd)
    for k, r in rh.ln_forward_ratios('add_layer_norm', st, gamma, new, ref, eager, dtype).items():
        file_ratio(f'add_layer_norm {k}', r)
    d_res64 = ref['dx'] + ds.double()
    ref_r = dict(ref, dx=d_res64)
    eager_r = eager['dx'].double() + ds.double()
    bar = rh.ln_backward_row_bar(st, ref_r, eager_r, dtype)
    file_ratio('add_layer_norm d_res', rh._worst('add_layer_norm d_res', (rg.grad.double().view(M, C) - d_res64).norm(dim=-1), bar))
    ref_x = dict(ref, dx=d_res64 * sc)
    bar = rh.ln_backward_row_bar(st, ref_x, eager_r * sc, dtype, roundings=2, factor=sc.view(-1))
    file_ratio('add_layer_norm d_x', rh._worst('add_layer_norm d_x', (xg.grad.double().view(M, C) - d_res64 * sc).norm(dim=-1), bar))
    assert torch.all(xg.grad.view(M, C)[sc.view(-1) == 0] == 0) and torch.all(y.detach().view(B, -1)[0].isfinite())
    check_columns('add_layer_norm', st, dy, ref, eager, wg.grad, bg.grad)


@pytest.mark.parametrize('dtype', DT16, ids=IDS16)
@pytest.mark.parametrize('M,C', EPI_SHAPES)
def test_residual_layer_norm_epilogue_structured_rows(M, C, dtype):
    """TGT_EPI_RESID with ln=: half of every row arrives through an identity weight, the other half as the residual (C = 64: the
    K = 256 kernel, the rows padded with zero columns)"""
    rows = rh.structured_rows(M, C, dtype).cuda()
    half = (rows.double() / 2).to(dtype)
    res = (rows.double() - half.double()).to(dtype)
    K = 256
    a = torch.zeros(M, K, dtype=dtype, device='cuda')
    a[:, :C] = half
    w = torch.eye(C, K, dtype=dtype, device='cuda')
    gamma, beta = rh.ln_params(C, 'cuda')
    mean, rstd = torch.empty(M, device='cuda'), torch.empty(M, device='cuda')
    y = torch.empty(M, C, dtype=dtype, device='cuda')
    out = ops.edge_linear_raw(a, w, None, _lib.EPI_RESID, res=res, ln=(gamma, beta, 1e-5), stats=(mean, rstd), y=y)
    torch.cuda.synchronize()
    s64 = half.double() + res.double()
    file_ratio('EPI_RESID out', rh._worst('EPI_RESID out', (out.double() - s64).abs().reshape(-1),
                                          (rh.storage_h(s64, dtype) + rh.U32 * (half.double().abs() + res.double().abs())).reshape(-1)))
    ref = rh.ln_reference(out, gamma, beta, 1e-5)
    eager = rh.ln_eager32(out, gamma, beta, 1e-5)
    for k, r in rh.ln_forward_ratios('EPI_RESID', out, gamma, dict(y=y, mean=mean, rstd=rstd), ref, eager, dtype).items():
        file_ratio(f'EPI_RESID {k}', r)


@pytest.mark.parametrize('dtype', DT16, ids=IDS16)
@pytest.mark.parametrize('M,C', EPI_SHAPES)
def test_layer_norm_backward_epilogue_structured_rows(M, C, dtype):
    """TGT_EPI_LN_BWD: dy through an identity weight (exact), res = the structured rows, their statistics handed in as the float32
    roundings of the exact ones, a stream gradient ds_in and a per-graph scale with a zero"""
    s = rh.structured_rows(M, C, dtype).cuda()
    gamma, _ = rh.ln_params(C, 'cuda')
    dy, ds = _dy(M, C, dtype, 4), _dy(M, C, dtype, 5)
    ref = rh.ln_reference(s, gamma, torch.zeros_like(gamma), 1e-5, dy)
    eager = rh.ln_eager32(s, gamma, torch.zeros_like(gamma), 1e-5, dy)
    mean, rstd = ref['mean'].float().contiguous(), ref['rstd'].float().contiguous()
    B = SAMPLES[M]
    rps = M // B
    scale = torch.tensor([1.0, 0.0, 0.75, 0.5], device='cuda').repeat(5)[:B].contiguous()
    w = torch.eye(C, dtype=dtype, device='cuda')
    partial = torch.zeros(_lib.lib().tgt_edge_linear_parts(M, C), 3 * C, device='cuda')
    dres = torch.empty(M, C, dtype=dtype, device='cuda')
    dx = torch.empty(M, C, dtype=dtype, device='cuda')
    ops.edge_linear_raw(dy, w, None, _lib.EPI_LN_BWD, ln=(gamma, None, 1e-5), stats=(mean, rstd), res=s, ds_in=ds, out=dres, out2=dx,
                        row_scale=scale, rows_per_sample=rps, colsum_partial=partial)
    torch.cuda.synchronize()
    sc = scale.double().repeat_interleave(rps)[:, None]
    d_res64 = ref['dx'] + ds.double()
    eager_r = eager['dx'].double() + ds.double()
    bar = rh.ln_backward_row_bar(s, dict(ref, dx=d_res64), eager_r, dtype, given_stats=True)
    file_ratio('EPI_LN_BWD d_res', rh._worst('EPI_LN_BWD d_res', (dres.double() - d_res64).norm(dim=-1), bar))
    bar = rh.ln_backward_row_bar(s, dict(ref, dx=d_res64 * sc), eager_r * sc, dtype, given_stats=True, roundings=2, factor=sc.view(-1))
    file_ratio('EPI_LN_BWD d_x', rh._worst('EPI_LN_BWD d_x', (dx.double() - d_res64 * sc).norm(dim=-1), bar))
    assert torch.all(dx[sc.view(-1) == 0] == 0)
    tot = partial.double().sum(0)
    check_columns('EPI_LN_BWD', s, dy, ref, eager, tot[:C], tot[C:2 * C], given_stats=True)
    # the third plane: the column sums of the x-branch gradient AS STORED
    file_ratio('EPI_LN_BWD colsum d_x', rh._worst('EPI_LN_BWD colsum d_x', (tot[2 * C:] - dx.double().sum(0)).abs(), rh.column_sum_bar(dx)))


# ---------------------------------------------------------------------------------------------------------------
# C. cross entropy rows, Gaussian basis
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('rows,C', rh.XENT_SHAPES)
def test_cross_entropy_rows_hard_rows(rows, C, dtype):
    logits, target, w = (t.cuda() for t in rh.xent_rows(rows, C, dtype))
    case = rh.xent_case(logits, target, w)
    x = logits.clone().requires_grad_(True)
    xent = ops.cross_entropy_rows(x, target)
    lse = xent.grad_fn.saved_tensors[2]
    (xent * w).sum().backward()
    torch.cuda.synchronize()
    assert xent.dtype == torch.float32 and x.grad.dtype == dtype
    for k, r in rh.xent_ratios('xent', logits, w, dict(xent=xent.detach(), lse=lse, grad=x.grad), case, dtype).items():
        file_ratio(f'xent {k}', r)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('K', rh.GAUSS_KS)
def test_gaussian_basis_hard_inputs(K, dtype):
    x, mul, bias, means, stds = (t.cuda() for t in rh.gaussian_inputs(K))
    assert _lib.lib().tgt_gaussian_basis_parts(x.numel()) < x.numel()            # the capped grid: some wave takes a second pair
    gy = torch.randn(*x.shape, K, generator=torch.Generator().manual_seed(K)).to(dtype).cuda()
    ref = rh.gaussian_case(x, mul, bias, means, stds, gy, torch.float64)
    eager = rh.gaussian_case(x, mul, bias, means, stds, gy, torch.float32)
    dev = [t.clone().requires_grad_(True) for t in (mul, bias, means, stds)]
    with torch.autocast('cuda', dtype=dtype, enabled=dtype != torch.float32):
        y = ops.gaussian_basis(x, *dev)
    assert y.dtype == dtype
    y.backward(gy)
    torch.cuda.synchronize()
    new = dict(y=y.detach(), dmul=dev[0].grad, dbias=dev[1].grad, dmeans=dev[2].grad, dstds=dev[3].grad)
    assert all(torch.isfinite(v).all() for v in new.values())
    assert torch.all(new['dstds'][stds == 0] == 0)
    for k, r in rh.gaussian_ratios('gaussian', new, ref, eager, dtype, x).items():
        file_ratio(f'gaussian {k}', r)
