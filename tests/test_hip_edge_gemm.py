"""tgt_edge_linear (csrc/edge_gemm.hip) through the C ABI against float64 restatements of the chains it replaces:
nn.LayerNorm -> nn.Linear -> GELU/Dropout -> nn.Linear -> residual add_ on the edge rows
(reference lib/tgt/layers/layers.py:37-38,:62-80,:155-160,:270-290; triplet.py:207-211,:248-249) and their
autograd backward.  Tolerances: the kernel rounds its result once to the 16-bit storage type, so against a float64
evaluation of the same rounded operands the error is one rounding of the output (bf16: 2^-8 relative per element;
rel-L2 <= 4e-3; fp16 <= 5e-4), plus fp32 accumulation noise."""
import math

import pytest
import torch

import parity_log

from tgt_amd import _lib, ops

pytestmark = pytest.mark.gpu

TOL = parity_log.Tol({torch.bfloat16: 4e-3, torch.float16: 5e-4})


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return parity_log.record(float((a - b).norm() / (b.norm() + 1e-30)))


def _mk(M, K, N, dtype, seed, bias=True):
    g = torch.Generator(device='cuda').manual_seed(seed)
    a = torch.randn(M, K, device='cuda', generator=g).to(dtype)
    w = (torch.randn(N, K, device='cuda', generator=g) / math.sqrt(K)).to(dtype)
    b = (torch.randn(N, device='cuda', generator=g) * 0.5).to(dtype) if bias else None
    return a, w, b, g


def _ln64(x, gamma, beta, eps):
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(var + eps)
    return (x - mu) * rstd * gamma.double() + beta.double(), mu.squeeze(-1), rstd.squeeze(-1)


SHAPES = [(300, 64, 8), (300, 64, 24), (257, 64, 256), (1000, 128, 128), (1024, 256, 128), (513, 256, 256),
          (640, 256, 1600), (384, 128, 256), (130, 256, 32), (128, 256, 64), (777, 256, 512), (64, 256, 512)]


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('M,K,N', SHAPES)
def test_plain_linear_matches_float64(M, K, N, dtype):
    a, w, b, g = _mk(M, K, N, dtype, 1)
    out = ops.edge_linear_raw(a, w, b)
    ref = a.double() @ w.double().t() + b.double()
    assert rel(out, ref) < TOL[dtype]
    # no bias, per-graph output scale, strided operand views
    big = torch.randn(M, K + 8, device='cuda', generator=g).to(dtype)
    av = big[:, 8:]
    sc = torch.rand(math.ceil(M / 100), device='cuda', generator=g) + 0.5
    dst = torch.full((M, N + 8), 7.0, dtype=dtype, device='cuda')
    ops.edge_linear_raw(av, w, None, out=dst[:, :N], out_scale=sc, rows_per_sample=100)
    ref = (av.double() @ w.double().t()) * sc.double().repeat_interleave(100)[:M, None]
    assert rel(dst[:, :N], ref) < TOL[dtype]
    assert torch.all(dst[:, N:] == 7.0)                 # nothing written past the N columns


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('M,K,N', [(300, 64, 64), (513, 256, 256), (1024, 256, 512), (260, 128, 128)])
def test_gelu_dropout_epilogue_equals_standalone_kernel(M, K, N, dtype, p):
    a, w, b, g = _mk(M, K, N, dtype, 3)
    seed = 0x1234567 if p else 0
    pre = torch.empty(M, N, dtype=dtype, device='cuda')
    out = ops.edge_linear_raw(a, w, b, _lib.EPI_GELU, out2=pre, dropout=(p, seed))
    ref = a.double() @ w.double().t() + b.double()
    assert rel(pre, ref) < TOL[dtype]
    # the activation is the standalone kernel's function of the STORED pre-activation, same keep pattern
    y = torch.empty_like(pre)
    _lib.check(_lib.lib().tgt_gelu_dropout_fwd(pre.data_ptr(), y.data_ptr(), pre.numel(), ops._DT[dtype], p, seed, None), 'gd')
    torch.cuda.synchronize()
    # same arithmetic in two kernels (scalar there, packed pairs here): the keep pattern is identical, a value may differ by one
    # unit in the last place of the 16-bit result where hipcc contracted the erf polynomial differently
    assert torch.equal(out == 0, y == 0)
    diff = (out.float() - y.float()).abs()
    assert float((diff > 0).float().mean()) < 2e-3
    assert float((diff / y.float().abs().clamp_min(1e-3)).max()) < (2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -9)
    if p:
        kept = float((out != 0).float().mean())
        assert abs(kept - (1 - p)) < 0.02


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('M,K,N', [(300, 64, 64), (700, 64, 256), (513, 256, 256), (384, 128, 256), (391, 512, 256)])
def test_residual_epilogue(M, K, N, dtype):
    a, w, b, g = _mk(M, K, N, dtype, 4)
    res = torch.randn(M, N, device='cuda', generator=g).to(dtype)
    sc = (torch.rand(math.ceil(M / 64), device='cuda', generator=g) > 0.3).float() / 0.7       # DropPath factors
    out = ops.edge_linear_raw(a, w, b, _lib.EPI_RESID, res=res, row_scale=sc, rows_per_sample=64)
    ref = res.double() + (a.double() @ w.double().t() + b.double()) * sc.double().repeat_interleave(64)[:M, None]
    assert rel(out, ref) < TOL[dtype]
    out = ops.edge_linear_raw(a, w, b, _lib.EPI_RESID, res=res)
    assert rel(out, res.double() + a.double() @ w.double().t() + b.double()) < TOL[dtype]


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('M,K,N', [(300, 64, 256), (1000, 256, 256), (257, 128, 128), (640, 256, 64), (129, 64, 200), (1003, 512, 256)])
def test_residual_epilogue_with_layernorm_of_the_new_row(M, K, N, dtype):
    """out = res + scale*(a W^T + b) and y = LayerNorm(out as stored): the fused `residual add + LayerNorm` entry of
    the next sub-block (reference layers.py:270-290 followed by the next block's nn.LayerNorm)"""
    a, w, b, g = _mk(M, K, N, dtype, 8)
    res = (torch.randn(M, N, device='cuda', generator=g) * 1.5).to(dtype)
    sc = (torch.rand(math.ceil(M / 64), device='cuda', generator=g) > 0.3).float() / 0.7
    gamma = torch.rand(N, device='cuda', generator=g) + 0.5
    beta = torch.randn(N, device='cuda', generator=g) * 0.2
    mean, rstd = torch.empty(M, device='cuda'), torch.empty(M, device='cuda')
    y = torch.empty(M, N, dtype=dtype, device='cuda')
    out = ops.edge_linear_raw(a, w, b, _lib.EPI_RESID, res=res, row_scale=sc, rows_per_sample=64, ln=(gamma, beta, 1e-5),
                              stats=(mean, rstd), y=y)
    ref = res.double() + (a.double() @ w.double().t() + b.double()) * sc.double().repeat_interleave(64)[:M, None]
    assert rel(out, ref) < TOL[dtype]
    y64, mu64, rs64 = _ln64(out, gamma, beta, 1e-5)                 # of the row AS STORED
    assert rel(mean, mu64) < 1e-5 and rel(rstd, rs64) < 1e-5
    assert rel(y, y64) < TOL[dtype]
    y2 = ops.layer_norm(out, gamma, beta, 1e-5, out_dtype=dtype)    # the standalone kernel on the same stored row
    assert rel(y, y2) < (2e-3 if dtype == torch.bfloat16 else 3e-4)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('p', [0.0, 0.1])
def test_gelu_backward_epilogue_equals_standalone_kernel(dtype, p):
    M, K, N = 520, 256, 256            # dz (M,K) @ W2 (K_out=256 rows of W2^T) -> d_a, then through the activation
    a, w, _, g = _mk(M, K, N, dtype, 5, bias=False)
    pre = torch.randn(M, N, device='cuda', generator=g).to(dtype)
    sc = torch.rand(math.ceil(M / 40), device='cuda', generator=g) + 0.5
    seed = 0xabcdef if p else 0
    out = ops.edge_linear_raw(a, w, None, _lib.EPI_GELU_BWD, res=pre, out_scale=sc, rows_per_sample=40, dropout=(p, seed))
    dy = ((a.double() @ w.double().t()) * sc.double().repeat_interleave(40)[:M, None]).to(dtype)
    dx = torch.empty_like(pre)
    _lib.check(_lib.lib().tgt_gelu_dropout_bwd(pre.data_ptr(), dy.data_ptr(), dx.data_ptr(), pre.numel(), ops._DT[dtype], p, seed,
                                               None), 'gd')
    torch.cuda.synchronize()
    # dy is rounded once in both paths, but from fp32 (kernel) vs float64 (here): allow the last-bit flips that causes
    assert rel(out, dx) < TOL[dtype]
    assert float(((out == 0) != (dx == 0)).float().mean()) < 1e-3


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('M,K,N,with_ds,with_scale', [(300, 128, 256, True, True), (513, 64, 256, True, False),
                                                      (260, 256, 128, False, True), (200, 64, 64, False, False),
                                                      (1024, 256, 256, True, True)])
def test_layernorm_backward_epilogue(M, K, N, with_ds, with_scale, dtype):
    """dz (M,K) @ Wt (N,K)^T = dy (M,N), LayerNorm backward over N with the stream gradient added"""
    a, w, _, g = _mk(M, K, N, dtype, 6, bias=False)
    s = (torch.randn(M, N, device='cuda', generator=g) * 1.3 + 0.2).to(dtype)
    gamma = torch.rand(N, device='cuda', generator=g) + 0.5
    _, mu, rs = _ln64(s, gamma, torch.zeros_like(gamma), 1e-5)
    mean, rstd = mu.float().contiguous(), rs.float().contiguous()
    ds = torch.randn(M, N, device='cuda', generator=g).to(dtype) if with_ds else None
    rps = 50
    sc = (torch.rand(math.ceil(M / rps), device='cuda', generator=g) + 0.5) if with_scale else None
    parts = _lib.lib().tgt_edge_linear_parts(M, N)
    partial = torch.zeros(parts, 3 * N, device='cuda')
    dres = torch.empty(M, N, dtype=dtype, device='cuda')
    dx = torch.empty(M, N, dtype=dtype, device='cuda') if with_scale else None
    ops.edge_linear_raw(a, w, None, _lib.EPI_LN_BWD, ln=(gamma, None, 1e-5), stats=(mean, rstd), res=s, ds_in=ds, out=dres,
                        out2=dx, row_scale=sc, rows_per_sample=rps if with_scale else 0, colsum_partial=partial)
    dy = (a.double() @ w.double().t()).to(dtype).double()               # the unfused chain stores dy in the 16-bit type
    xh = (s.double() - mu[:, None]) * rs[:, None]
    gg = dy * gamma.double()
    ref = rs[:, None] * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True))
    if with_ds:
        ref = ref + ds.double()
    assert rel(dres, ref) < TOL[dtype]
    tot = partial.double().sum(0)
    assert rel(tot[:N], (dy * xh).sum(0)) < 1e-4
    assert rel(tot[N:2 * N], dy.sum(0)) < 1e-4
    if with_scale:
        refx = dres.double() * sc.double().repeat_interleave(rps)[:M, None]
        assert rel(dx, refx) < TOL[dtype]
        assert rel(tot[2 * N:], dx.double().sum(0)) < 1e-4            # column sums of the gradient AS STORED
    else:
        assert rel(tot[2 * N:], dres.double().sum(0)) < 1e-4


def test_unsupported_shapes_raise_instead_of_falling_back():
    a, w, b, _ = _mk(64, 48, 64, torch.bfloat16, 7)
    with pytest.raises(RuntimeError, match='unsupported'):
        ops.edge_linear_raw(a, w, b)
    for K, N in ((512, 512), (512, 128), (16, 64), (272, 64), (1600, 256)):      # (the general tile kernel of round 2 is gone)
        a, w, b, _ = _mk(64, K, N, torch.bfloat16, 7)
        with pytest.raises(RuntimeError, match='unsupported'):
            ops.edge_linear_raw(a, w, b)
    a, w, b, g = _mk(64, 256, 256, torch.bfloat16, 7)
    with pytest.raises(RuntimeError, match='unsupported'):            # no LayerNorm prologue any more
        ops.edge_linear_raw(a, w, b, ln=(torch.ones(256, device='cuda'), torch.zeros(256, device='cuda'), 1e-5))
    with pytest.raises(RuntimeError):
        ops.edge_linear_raw(a.float(), w.float(), b.float())


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('B,N,K,C,with_scale', [(3, 10, 64, 256, True), (2, 16, 256, 256, False), (4, 9, 128, 64, True)])
def test_linear_residual_layer_norm_op_matches_the_two_launch_composition(B, N, K, C, with_scale, dtype, monkeypatch):
    """autograd op used by TGT_Layer (lin_O_e / lin_W2 + residual + next LayerNorm): fused launch vs
    ops.linear -> ops.add_layer_norm, outputs and every gradient"""
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)
    g = torch.Generator(device='cuda').manual_seed(11)

    def mk(*shape, scale=1.0):
        return (torch.randn(*shape, device='cuda', generator=g) * scale)

    x0, res0 = mk(B, N, N, K).to(dtype), mk(B, N, N, C).to(dtype)
    w0, b0 = mk(C, K, scale=K ** -0.5), mk(C, scale=0.3)
    lw0, lb0 = torch.rand(C, device='cuda', generator=g) + 0.5, mk(C, scale=0.2)
    sc = ((torch.rand(B, device='cuda', generator=g) > 0.3).float() / 0.7) if with_scale else None
    gs, gy = mk(B, N, N, C).to(dtype), mk(B, N, N, C).to(dtype)
    outs = []
    for fused in (True, False):
        monkeypatch.setattr(ops, '_EDGE_GEMM', fused)
        leaves = [t.clone().requires_grad_(True) for t in (x0, res0, w0, b0, lw0, lb0)]
        x, res, w, b, lw, lb = leaves
        with torch.autocast('cuda', dtype=dtype):
            s, y = ops.linear_residual_layer_norm(x, w, b, res, sc, lw, lb, 1e-5)
        assert (type(s.grad_fn).__name__ == '_LinearResidualLNBackward') == fused
        ((s.float() * gs.float()).sum() + (y.float() * gy.float()).sum()).backward()
        outs.append([s, y] + [t.grad for t in leaves])
    names = ['s', 'y', 'dx', 'dres', 'dW', 'db', 'dln_w', 'dln_b']
    for name, a, b_ in zip(names, *outs):
        tol = 3 * TOL[dtype] if name.startswith('d') else TOL[dtype]
        assert rel(a, b_) < tol, (name, rel(a, b_))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('B,N,K', [(3, 10, 64), (4, 12, 256)])
def test_prescaled_residual_matches_the_scaled_composition(B, N, K, dtype, monkeypatch):
    """DropPath folded into the producer (TGT_EDGE_BIAS_SCALED + tgt_add_layer_norm_bwd without d_x): feeding x * scale with
    prescaled=True must give the outputs and EVERY gradient of the plain op on x (the gradient of x through the product rule:
    d x = scale * d x')"""
    C = 256
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)
    g = torch.Generator(device='cuda').manual_seed(23)
    mk = lambda *shape, scale=1.0: torch.randn(*shape, device='cuda', generator=g) * scale
    x0, res0 = mk(B, N, N, K).to(dtype), mk(B, N, N, C).to(dtype)
    w0, b0 = mk(C, K, scale=K ** -0.5), mk(C, scale=0.3)
    lw0, lb0 = torch.rand(C, device='cuda', generator=g) + 0.5, mk(C, scale=0.2)
    sc = (torch.rand(B, device='cuda', generator=g) > 0.3).float() / 0.7
    sc[0] = 0.0                                            # a dropped graph
    gs, gy = mk(B, N, N, C).to(dtype), mk(B, N, N, C).to(dtype)
    outs = []
    for pres in (True, False):
        leaves = [t.clone().requires_grad_(True) for t in (x0, res0, w0, b0, lw0, lb0)]
        x, res, w, b, lw, lb = leaves
        with torch.autocast('cuda', dtype=dtype):
            if pres:
                xs = x * sc.view(-1, 1, 1, 1).to(dtype)    # (exact: the factors are 0 or 1/0.7 rounded once either way)
                s, y = ops.linear_residual_layer_norm(xs, w, b, res, sc, lw, lb, 1e-5, prescaled=True)
                assert type(s.grad_fn).__name__ == '_LinearResidualLNBackward'
            else:
                s, y = ops.linear_residual_layer_norm(x, w, b, res, sc, lw, lb, 1e-5)
        ((s.float() * gs.float()).sum() + (y.float() * gy.float()).sum()).backward()
        outs.append([s, y] + [t.grad for t in leaves])
    names = ['s', 'y', 'dx', 'dres', 'dW', 'db', 'dln_w', 'dln_b']
    for name, a, b_ in zip(names, *outs):
        tol = 3 * TOL[dtype] if name.startswith('d') else TOL[dtype]
        assert rel(a, b_) < tol, (name, rel(a, b_))
    assert float(outs[0][2][0].abs().max()) == 0.0        # the dropped graph's input gets no gradient


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
def test_gelu_dropout_sample_scale(dtype):
    """tgt_gelu_dropout_scaled_*: y = scale[b] * dropout(gelu(x)) and its backward, same drop pattern as the unscaled op"""
    B, R, C = 3, 50, 64
    g = torch.Generator(device='cuda').manual_seed(5)
    x0 = torch.randn(B, R, C, device='cuda', generator=g).to(dtype)
    dy = torch.randn(B, R, C, device='cuda', generator=g).to(dtype)
    sc = torch.tensor([0.0, 1.25, 1.25], device='cuda')
    for p in (0.0, 0.2):
        xa, xb = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
        ya = ops._ActDropout.apply(xa, ops._ACT_FAMILIES['gelu'], None, p, 1234, sc)
        yb = ops._ActDropout.apply(xb, ops._ACT_FAMILIES['gelu'], None, p, 1234, None)
        ya.backward(dy)
        yb.backward(dy)
        ref, gref = yb.float() * sc.view(-1, 1, 1), xb.grad.float() * sc.view(-1, 1, 1)
        tol = {torch.float32: 1e-6, torch.bfloat16: 8e-3, torch.float16: 1e-3}[dtype]
        assert rel(ya, ref) < tol and rel(xa.grad, gref) < tol
        assert float(ya[0].abs().max()) == 0.0 and float(xa.grad[0].abs().max()) == 0.0


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('with_scale', [False, True])
@pytest.mark.parametrize('colsum', [True, False])
def test_linear_gelu_dropout_node_equals_the_unfused_chain(dtype, p, with_scale, colsum, monkeypatch):
    """lin_W1 + GELU + dropout (+ the folded DropPath factor) as one launch and one autograd node (the FFN's hidden
    activation on the edge rows, reference layers.py:155-158) against Linear -> tgt_gelu_dropout: same drop pattern (same
    seed draw), outputs and every gradient within the GEMM's rounding"""
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)
    monkeypatch.setattr(ops, '_GELU_BWD_COLSUM', colsum)        # lin_W1's bias gradient from the activation's backward pass (ABI 24) or a separate pass
    g = torch.Generator(device='cuda').manual_seed(13)
    B, n, K, N = 4, 9, 256, 256
    x = torch.randn(B, n, n, K, device='cuda', generator=g)
    w = torch.randn(N, K, device='cuda', generator=g) * K ** -0.5
    b = torch.randn(N, device='cuda', generator=g) * 0.1
    dy = torch.randn(B, n, n, N, device='cuda', generator=g).to(dtype)
    sc = torch.tensor([1.25, 0.0, 1.25, 1.25], device='cuda') if with_scale else None
    outs = []
    for fused in (True, False):
        ins = [t.clone().requires_grad_(True) for t in (x, w, b)]
        torch.manual_seed(77)                      # both draw ONE seed from the CPU generator
        with torch.autocast('cuda', dtype=dtype):
            if fused:
                assert ops.linear_gelu_dropout_ok(ins[0], ins[1], sc)
                y = ops.linear_gelu_dropout(ins[0], ins[1], ins[2], p, True, sc)
            else:
                y = ops.gelu_dropout(ops.linear(ins[0], ins[1], ins[2]), p, True, sc)
        y.backward(dy)
        outs.append((y, [t.grad for t in ins]))
    torch.cuda.synchronize()
    (y1, g1), (y0, g0) = outs
    assert y1.dtype == dtype and torch.isfinite(y1).all()
    assert rel(y1, y0) < TOL[dtype]
    # the same elements are dropped (up to pre-activations that round across zero ... none at these sizes: compare the patterns)
    assert float(((y1 == 0) != (y0 == 0)).float().mean()) < 2e-3
    if with_scale:
        assert float(y1[1].abs().max()) == 0
    for a_, b_, name in zip(g1, g0, ('dx', 'dw', 'db')):
        assert rel(a_, b_) < 2 * TOL[dtype], (name, rel(a_, b_))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('prescaled', [False, True])
def test_ffn_block_with_fused_activation_both_ways(dtype, p, prescaled, monkeypatch):
    """the edge FFN as the layer runs it (reference layers.py:155-160, 284-290): lin_W1 + GELU + dropout as one launch, and in
    the backward the activation's derivative as the epilogue of lin_W2's data-gradient GEMM (the closing node receives the
    activation detached and returns the gradient of the PRE-activation) -- against the unfused chain with the same seed draw:
    stream, normalised rows and every gradient within the GEMMs' rounding"""
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)
    g = torch.Generator(device='cuda').manual_seed(21)
    B, n, C = 4, 9, 256
    x = torch.randn(B, n, n, C, device='cuda', generator=g)
    res = torch.randn(B, n, n, C, device='cuda', generator=g).to(dtype)
    w1 = torch.randn(C, C, device='cuda', generator=g) * C ** -0.5
    b1 = torch.randn(C, device='cuda', generator=g) * 0.1
    w2 = torch.randn(C, C, device='cuda', generator=g) * C ** -0.5
    b2 = torch.randn(C, device='cuda', generator=g) * 0.1
    lw = torch.rand(C, device='cuda', generator=g) + 0.5
    lb = torch.randn(C, device='cuda', generator=g) * 0.2
    d_s = torch.randn(B, n, n, C, device='cuda', generator=g).to(dtype)
    d_y = torch.randn(B, n, n, C, device='cuda', generator=g).to(dtype)
    sc = torch.tensor([1.25, 0.0, 1.25, 1.25], device='cuda')
    runs = []
    for fused in (True, False):
        monkeypatch.setattr(ops, '_FFN_GELU_EPI', fused)
        monkeypatch.setattr(ops, '_FFN_GELU_BWD_EPI', fused)
        ins = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2, res, lw, lb)]
        torch.manual_seed(5)
        with torch.autocast('cuda', dtype=dtype):
            fold = sc if prescaled else None
            if fused:
                act = ops.linear_gelu_dropout(ins[0], ins[1], ins[2], p, True, fold)
                assert hasattr(act, '_tgt_gelu')
            else:
                act = ops.gelu_dropout(ops.linear(ins[0], ins[1], ins[2]), p, True, fold)
            s, y = ops.linear_residual_layer_norm(act, ins[3], ins[4], ins[5], sc, ins[6], ins[7], 1e-5, prescaled=prescaled)
        torch.autograd.backward([s, y], [d_s, d_y])
        runs.append((s, y, [t.grad for t in ins]))
    torch.cuda.synchronize()
    (s1, y1, g1), (s0, y0, g0) = runs
    assert rel(s1, s0) < TOL[dtype] and rel(y1, y0) < TOL[dtype]
    for a_, b_, name in zip(g1, g0, ('dx', 'dw1', 'db1', 'dw2', 'db2', 'dres', 'dgamma', 'dbeta')):
        assert a_ is not None and torch.isfinite(a_).all(), name
        assert rel(a_, b_) < 3 * TOL[dtype], (name, rel(a_, b_))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('rows,cols', [(4100, 256), (333, 64), (9000, 512), (77, 128), (262144, 256)])
@pytest.mark.parametrize('p', [0.0, 0.2])
def test_gelu_backward_with_bias_gradient_column_sums(dtype, rows, cols, p):
    """tgt_gelu_dropout_bwd_colsum: dx bit-equal to tgt_gelu_dropout_scaled_bwd, colsum = float64 column sums of the STORED dx"""
    g = torch.Generator(device='cuda').manual_seed(3)
    x = torch.randn(rows, cols, device='cuda', generator=g).to(dtype)
    dy = torch.randn(rows, cols, device='cuda', generator=g).to(dtype)
    L = _lib.lib()
    seed = 0x51ed if p else 0
    dx0, dx1 = torch.empty_like(x), torch.empty_like(x)
    _lib.check(L.tgt_gelu_dropout_scaled_bwd(x.data_ptr(), dy.data_ptr(), dx0.data_ptr(), x.numel(), ops._DT[dtype], p, seed, None, 0, None), 'a')
    cs = torch.empty(cols, device='cuda')
    partial = torch.empty(L.tgt_gelu_colsum_parts() * cols, device='cuda')
    _lib.check(L.tgt_gelu_dropout_bwd_colsum(x.data_ptr(), dy.data_ptr(), dx1.data_ptr(), x.numel(), ops._DT[dtype], p, seed, None, 0,
                                             cols, partial.data_ptr(), cs.data_ptr(), None), 'b')
    torch.cuda.synchronize()
    assert torch.equal(dx0, dx1)
    want = dx0.double().sum(0)
    assert float((cs.double() - want).abs().max()) <= 1e-5 * float(want.abs().max()) + 1e-6


# ---------------------------------------------------------------------------------------------------------------
# BASELINE size: M = B*N*N = 262144 rows -> 8192 row tiles on 256 persistent workgroups = 32 tiles per workgroup.
# Everything above runs <= 1 tile per workgroup (unless capped); these cases walk the double-buffered stage hand-over
# and the cross-tile accumulators of every DEFAULT-ON instantiation the way the benchmark does.
#   (1) sampled row blocks (first / last tiles, a workgroup's 2nd..4th tile, odd tile indices) against float64;
#   (2) slice equality: rows [s:e) of the full launch == a launch on that slice alone, bit for bit (a row's result
#       does not depend on which workgroup / pipeline stage computed it).
# ---------------------------------------------------------------------------------------------------------------
SIZE_M = 262144
SIZE_BLOCKS = [(0, 96), (32 * 255, 32 * 258), (32 * 256 * 3 - 32, 32 * 256 * 3 + 64), (32 * 4001, 32 * 4004),
               (SIZE_M - 128, SIZE_M)]
SIZE_SLICES = [(0, 4096), (1024 * 31, 1024 * 33), (SIZE_M - 1024, SIZE_M)]      # (whole graphs: the per-graph factor is indexed from the slice's first row)
SIZE_CASES = {
    # name: (K, N, epilogue, prescaled bias, LayerNorm of the new row, row_scale)
    'lin_W2+res+LN (K=256)': (256, 256, 'resid', False, True, True),
    'lin_W2+res+LN prescaled (K=256)': (256, 256, 'resid', True, True, True),
    'lin_O_e+res+LN prescaled (K=64)': (64, 256, 'resid', True, True, True),
    'lin_O_e+res+LN (K=64)': (64, 256, 'resid', False, True, False),
    'lin_W1+GELU+dropout (K=256)': (256, 256, 'gelu', False, False, True),
    'lin_O+res+LN (K=512)': (512, 256, 'resid', False, True, True),
    'lin_O+res+LN no DropPath (K=512)': (512, 256, 'resid', False, True, False),
    'lin_EG slice (N=128)': (256, 128, 'bias', False, False, False),
    'third arm slice (N=64)': (256, 64, 'bias', False, False, False),
    'ungated third arm slice (N=32)': (256, 32, 'bias', False, False, False),
    'lin_O data gradient (K=256 -> N=512)': (256, 512, 'bias', False, False, False),
}


def _size_case_run(case, a, w, b, res, sc, gamma, beta, rps, p=0.0, seed=0):
    K, N, epi, pres, ln, with_sc = SIZE_CASES[case]
    M = a.shape[0]
    scale = sc if with_sc else None
    if epi == 'bias':
        return (ops.edge_linear_raw(a, w, b),)
    if epi == 'gelu':
        pre = torch.empty(M, N, dtype=a.dtype, device='cuda')
        act = ops.edge_linear_raw(a, w, b, _lib.EPI_GELU, out2=pre, dropout=(p, seed), row_scale=scale, rows_per_sample=rps)
        return act, pre
    mean, rstd = torch.empty(M, device='cuda'), torch.empty(M, device='cuda')
    y = torch.empty(M, N, dtype=a.dtype, device='cuda')
    out = ops.edge_linear_raw(a, w, b, _lib.EPI_RESID, res=res, row_scale=scale, rows_per_sample=rps, ln=(gamma, beta, 1e-5),
                              stats=(mean, rstd), y=y, flags=_lib.EDGE_BIAS_SCALED if pres else 0)
    return out, y, mean, rstd


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('case', list(SIZE_CASES))
def test_default_on_instantiations_at_baseline_size(case, dtype):
    K, N, epi, pres, ln, with_sc = SIZE_CASES[case]
    M, rps = SIZE_M, 1024
    a, w, b, g = _mk(M, K, N, dtype, 31)
    res = (torch.randn(M, N, device='cuda', generator=g) * 1.5).to(dtype)
    sc = (torch.rand(M // rps, device='cuda', generator=g) > 0.2).float() / 0.8
    gamma = torch.rand(N, device='cuda', generator=g) + 0.5
    beta = torch.randn(N, device='cuda', generator=g) * 0.2
    full = _size_case_run(case, a, w, b, res, sc, gamma, beta, rps)
    torch.cuda.synchronize()
    # (1) float64 on sampled row blocks
    for s, e in SIZE_BLOCKS:
        z = a[s:e].double() @ w.double().t()
        f = sc.double().repeat_interleave(rps)[s:e, None] if with_sc else 1.0
        if epi == 'bias':
            assert rel(full[0][s:e], z + b.double()) < TOL[dtype], (case, s)
        elif epi == 'gelu':
            assert rel(full[1][s:e], z + b.double()) < TOL[dtype], (case, s)
            pre = full[1][s:e].double()                              # the activation is a function of the STORED pre-activation
            act = pre * 0.5 * (1 + torch.erf(pre / math.sqrt(2.0))) * f
            assert rel(full[0][s:e], act) < TOL[dtype], (case, s)
        else:
            ref = res[s:e].double() + ((z + f * b.double()) if pres else (z + b.double()) * f)
            assert rel(full[0][s:e], ref) < TOL[dtype], (case, s)
            y64, mu64, rs64 = _ln64(full[0][s:e], gamma, beta, 1e-5)  # of the row AS STORED
            assert rel(full[2][s:e], mu64) < 1e-5 and rel(full[3][s:e], rs64) < 1e-5, (case, s)
            assert rel(full[1][s:e], y64) < TOL[dtype], (case, s)
    # (2) slice equality, bit for bit (dropout off: its keep pattern is indexed by the absolute row)
    for s, e in SIZE_SLICES:
        part = _size_case_run(case, a[s:e], w, b, res[s:e], sc[s // rps:], gamma, beta, rps)
        for t_full, t_part in zip(full, part):
            assert torch.equal(t_full[s:e], t_part), (case, s)
    # nothing non-finite anywhere, and the ragged end (M not a multiple of the 32-row tile) leaves the tail alone
    for t in full:
        assert bool(torch.isfinite(t.float()).all())
    Mr = M - 17
    sent = [torch.full_like(t, 7.0) for t in full]
    if epi == 'bias':
        ops.edge_linear_raw(a[:Mr], w, b, out=sent[0][:Mr])
        assert torch.equal(sent[0][:Mr], full[0][:Mr]) and bool((sent[0][Mr:] == 7.0).all())


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_gelu_dropout_epilogue_at_baseline_size_equals_standalone_kernel(dtype):
    """lin_W1 + GELU + dropout (p > 0, per-graph DropPath factor) at M = 262144: the stored activation equals the standalone
    activation kernel's function of the stored pre-activation -- same keep pattern, every element."""
    M, K, N, rps, p, seed = SIZE_M, 256, 256, 1024, 0.1, 0x5eed1234
    a, w, b, g = _mk(M, K, N, dtype, 37)
    sc = (torch.rand(M // rps, device='cuda', generator=g) > 0.2).float() / 0.8
    pre = torch.empty(M, N, dtype=dtype, device='cuda')
    act = ops.edge_linear_raw(a, w, b, _lib.EPI_GELU, out2=pre, dropout=(p, seed), row_scale=sc, rows_per_sample=rps)
    y = torch.empty_like(pre)
    _lib.check(_lib.lib().tgt_gelu_dropout_scaled_fwd(pre.data_ptr(), y.data_ptr(), pre.numel(), ops._DT[dtype], p, seed,
                                                      sc.data_ptr(), rps * N, None), 'gd')
    torch.cuda.synchronize()
    # same arithmetic, compiled twice: hipcc contracts the erf polynomial into other fma forms in the two kernels, so one element
    # in ~1e4 (fp16) differs by one unit in the last place of the 16-bit result (the 1024-row test above never meets one).  The KEEP
    # PATTERN must be identical.
    assert torch.equal(act == 0, y == 0)
    diff = (act.float() - y.float()).abs()
    assert float((diff > 0).float().mean()) < 1e-3            # (measured: 0 of 67 M in bf16, 1.4e-4 in fp16)
    assert float((diff / y.float().abs().clamp_min(1e-3)).max()) < (2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -9)
    kept = float((act.view(M // rps, -1)[sc > 0] != 0).float().mean())
    assert abs(kept - (1 - p)) < 5e-3
    for s, e in SIZE_BLOCKS:
        assert rel(pre[s:e], a[s:e].double() @ w.double().t() + b.double()) < TOL[dtype]


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('case', ['lin_W2+res+LN prescaled (K=256)', 'lin_O_e+res+LN prescaled (K=64)', 'lin_W1+GELU+dropout (K=256)',
                                  'lin_EG slice (N=128)', 'lin_O+res+LN (K=512)', 'lin_O data gradient (K=256 -> N=512)'])
@pytest.mark.parametrize('cap', [1, 3])
def test_grid_cap_hook_walks_many_tiles_per_workgroup(case, dtype, cap):
    """tgt_edge_linear_set_grid_cap: with `cap` persistent workgroups a 50-tile problem is 17..50 tiles per workgroup; the result
    must equal the uncapped launch bit for bit (what the small-model tests rely on to exercise the tile walk)."""
    K, N, epi, pres, ln, with_sc = SIZE_CASES[case]
    M, rps = 1600 - 9, 100
    a, w, b, g = _mk(M, K, N, dtype, 41)
    res = torch.randn(M, N, device='cuda', generator=g).to(dtype)
    sc = (torch.rand(-(-M // rps), device='cuda', generator=g) > 0.2).float() / 0.8
    gamma = torch.rand(N, device='cuda', generator=g) + 0.5
    beta = torch.randn(N, device='cuda', generator=g) * 0.2
    ref = _size_case_run(case, a, w, b, res, sc, gamma, beta, rps)
    try:
        _lib.lib().tgt_edge_linear_set_grid_cap(cap)
        got = _size_case_run(case, a, w, b, res, sc, gamma, beta, rps)
        torch.cuda.synchronize()
    finally:
        _lib.lib().tgt_edge_linear_set_grid_cap(0)
    for r_, g_ in zip(ref, got):
        assert torch.equal(r_, g_), case
    z = a.double() @ w.double().t()
    if epi == 'bias':
        assert rel(got[0], z + b.double()) < TOL[dtype]


# ---------------------------------------------------------------------------------------------------------------
# The two BACKWARD epilogues at BASELINE size, against float64: lin_W2's data gradient + GELU / dropout backward + lin_W1's
# bias-gradient column sums (EPI_GELU_BWD), and the consumer's data gradient + LayerNorm backward + stream gradient + row scale
# + three column-sum planes (EPI_LN_BWD).  At 262144 rows each persistent workgroup walks 32 tiles and writes ONE colsum_partial
# row, so the cross-tile accumulators are what the column sums test; under grid caps 1 and 3 a ~1600-row problem is 17..50
# tiles per workgroup.  (Above, these epilogues run one tile per workgroup, and at size they are only held to each other.)
# ---------------------------------------------------------------------------------------------------------------
_CHUNK = 32768          # float64 references over all rows go in chunks of this many rows (one 262144-row piece is 0.5 GB)


def _colsum_close(got, want):
    """the bar of test_gelu_backward_with_bias_gradient_column_sums: max |got - want| <= 1e-5 max |want| + 1e-6 (error on record
    relative to max |want|)"""
    top = float(want.abs().max())
    err = parity_log.record(float((got - want).abs().max()) / (top + 1e-30))
    return err * top <= 1e-5 * top + 1e-6, err


def _gelu_bwd_check(M, rps, dtype, p, with_scale, blocks, slices=()):
    TOL[dtype]                  # (files the comparisons below under this dtype in the parity log)
    K = N = 256
    a, w, _, g = _mk(M, K, N, dtype, 43, bias=False)
    pre = torch.randn(M, N, device='cuda', generator=g).to(dtype)
    sc = (torch.rand(-(-M // rps), device='cuda', generator=g) + 0.5) if with_scale else None
    seed = 0x9e1b5eed if p else 0
    L = _lib.lib()

    def run(s, e):
        cs = torch.empty(L.tgt_edge_linear_parts(e - s, N), N, device='cuda')
        out = ops.edge_linear_raw(a[s:e], w, None, _lib.EPI_GELU_BWD, res=pre[s:e], out_scale=None if sc is None else sc[s // rps:],
                                  rows_per_sample=rps if with_scale else 0, dropout=(p, seed), colsum_partial=cs)
        return out, cs

    out, cs = run(0, M)
    keep = None
    if p:                   # the keep pattern of the standalone kernel (same generator, indexed by the absolute element)
        one, kd = torch.ones_like(pre), torch.empty_like(pre)
        _lib.check(L.tgt_gelu_dropout_bwd(pre.data_ptr(), one.data_ptr(), kd.data_ptr(), pre.numel(), ops._DT[dtype], p, seed, None), 'gd')
        keep = kd != 0
        del one, kd
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(cs).all())
    f = sc.double().repeat_interleave(rps)[:M, None] if with_scale else None
    for s, e in blocks:
        dy = (a[s:e].double() @ w.double().t()).to(dtype).double()          # the GEMM result is rounded to the 16-bit type first,
        if with_scale:
            dy = (dy * f[s:e]).to(dtype).double()                             # and again after the per-graph factor
        x = pre[s:e].double()
        ref = dy * (0.5 * (1 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)) / (1 - p)
        if keep is not None:
            ref = ref * keep[s:e]
        assert rel(out[s:e], ref) < TOL[dtype], (s, rel(out[s:e], ref))
    # the column sums (lin_W1's bias gradient) are those of the d_pre AS STORED
    want = torch.zeros(N, dtype=torch.float64, device='cuda')
    for i in range(0, M, _CHUNK):
        want += out[i:i + _CHUNK].double().sum(0)
    ok, err = _colsum_close(cs.double().sum(0), want)
    assert ok, ('colsum', err)
    for s, e in slices:     # a row's result does not depend on the workgroup / stage that computed it
        assert torch.equal(out[s:e], run(s, e)[0]), s


def _ln_bwd_check(M, K, rps, dtype, blocks, slices=()):
    TOL[dtype]                  # (files the comparisons below under this dtype in the parity log)
    N = 256
    a, w, _, g = _mk(M, K, N, dtype, 47, bias=False)
    s_ = (torch.randn(M, N, device='cuda', generator=g) * 1.3 + 0.2).to(dtype)
    gamma = torch.rand(N, device='cuda', generator=g) + 0.5
    ds = torch.randn(M, N, device='cuda', generator=g).to(dtype)
    sc = (torch.rand(-(-M // rps), device='cuda', generator=g) > 0.2).float() / 0.8          # DropPath factors, zeros included
    zero = torch.zeros_like(gamma)
    mean, rstd = torch.empty(M, device='cuda'), torch.empty(M, device='cuda')
    for i in range(0, M, _CHUNK):
        _, mu, rs = _ln64(s_[i:i + _CHUNK], gamma, zero, 1e-5)
        mean[i:i + _CHUNK], rstd[i:i + _CHUNK] = mu.float(), rs.float()
    L = _lib.lib()

    def run(s, e):
        partial = torch.empty(L.tgt_edge_linear_parts(e - s, N), 3 * N, device='cuda')
        dres = torch.empty(e - s, N, dtype=dtype, device='cuda')
        dx = torch.empty(e - s, N, dtype=dtype, device='cuda')
        ops.edge_linear_raw(a[s:e], w, None, _lib.EPI_LN_BWD, ln=(gamma, None, 1e-5), stats=(mean[s:e], rstd[s:e]), res=s_[s:e],
                            ds_in=ds[s:e], out=dres, out2=dx, row_scale=sc[s // rps:], rows_per_sample=rps, colsum_partial=partial)
        return dres, dx, partial

    dres, dx, partial = run(0, M)
    torch.cuda.synchronize()
    for t in (dres, dx, partial):
        assert bool(torch.isfinite(t).all())
    f = sc.double().repeat_interleave(rps)[:M, None]

    def ref64(s, e):
        dy = (a[s:e].double() @ w.double().t()).to(dtype).double()          # the unfused chain stores dy in the 16-bit type
        _, mu, rs = _ln64(s_[s:e], gamma, zero, 1e-5)
        xh = (s_[s:e].double() - mu[:, None]) * rs[:, None]
        gg = dy * gamma.double()
        d = rs[:, None] * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True)) + ds[s:e].double()
        return dy, xh, d

    for s, e in blocks:
        _, _, d = ref64(s, e)
        assert rel(dres[s:e], d) < TOL[dtype], ('d_res', s)
        assert rel(dx[s:e], dres[s:e].double() * f[s:e]) < TOL[dtype], ('dx', s)        # of the d_res AS STORED
    # the three planes: dgamma = sum dy xhat, dbeta = sum dy, the consumer's bias gradient = sum of dx AS STORED
    want = torch.zeros(3, N, dtype=torch.float64, device='cuda')
    for i in range(0, M, _CHUNK):
        dy, xh, _ = ref64(i, min(M, i + _CHUNK))
        want[0] += (dy * xh).sum(0)
        want[1] += dy.sum(0)
        want[2] += dx[i:i + _CHUNK].double().sum(0)
    tot = partial.double().sum(0).view(3, N)
    for j, name in enumerate(('dgamma', 'dbeta', 'dx colsum')):
        assert rel(tot[j], want[j]) < 1e-4, (name, rel(tot[j], want[j]))
    for s, e in slices:
        part = run(s, e)
        assert torch.equal(dres[s:e], part[0]) and torch.equal(dx[s:e], part[1]), s


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('with_scale', [True, False])
def test_gelu_backward_epilogue_at_baseline_size(dtype, p, with_scale):
    _gelu_bwd_check(SIZE_M, 1024, dtype, p, with_scale, SIZE_BLOCKS, SIZE_SLICES if p == 0 else ())


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('K', [256, 128])        # the consumer: lin_W1 (256 -> 256), lin_EG (256 -> 128)
def test_layernorm_backward_epilogue_at_baseline_size(dtype, K):
    _ln_bwd_check(SIZE_M, K, 1024, dtype, SIZE_BLOCKS, SIZE_SLICES)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('case', ['gelu_bwd', 'gelu_bwd scaled p=0.1', 'ln_bwd K=256', 'ln_bwd K=128'])
@pytest.mark.parametrize('cap', [1, 3])
def test_grid_cap_hook_walks_many_tiles_in_the_backward_epilogues(case, dtype, cap):
    """the backward epilogues with 17..50 tiles per workgroup (1591 rows on `cap` workgroups), every row against float64"""
    M, rps = 1600 - 9, 100
    _lib.lib().tgt_edge_linear_set_grid_cap(cap)
    try:
        if case.startswith('gelu_bwd'):
            _gelu_bwd_check(M, rps, dtype, 0.1 if 'p=0.1' in case else 0.0, 'scaled' in case, [(0, M)])
        else:
            _ln_bwd_check(M, int(case.split('K=')[1]), rps, dtype, [(0, M)])
    finally:
        _lib.lib().tgt_edge_linear_set_grid_cap(0)


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm backward as the epilogue of the consumer's data-gradient GEMM (ops._lazy_dgrad / ops._ln_backward): the Linear
# behind a residual + LayerNorm entry hands (dz, W) to the entry's backward instead of computing dx = dz W; one launch then
# does GEMM + LayerNorm backward + stream-gradient add + dgamma / dbeta / bias-gradient sums (reference autograd of
# layers.py:37-38,:62-63 [mha_ln_e -> lin_EG] and :155-157 [ffn_ln -> lin_W1]).  Against the unfused backward, every gradient.
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('consumer', ['lin_EG', 'lin_W1+GELU', 'lin_W1+GELU+dropout'])
@pytest.mark.parametrize('producer', ['add_ln', 'add_ln_noscale', 'lin_resid_ln', 'lin_resid_ln_prescaled'])
def test_layernorm_backward_fused_into_the_consumer_dgrad(producer, consumer, dtype, monkeypatch):
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)
    B, N, C, K = 5, 9, 256, 64
    g = torch.Generator(device='cuda').manual_seed(77)
    mk = lambda *shape, scale=1.0: torch.randn(*shape, device='cuda', generator=g) * scale
    x0 = mk(B, N, N, K if producer.startswith('lin') else C).to(dtype)
    res0 = mk(B, N, N, C).to(dtype)
    w0, b0 = mk(C, K, scale=K ** -0.5), mk(C, scale=0.3)
    lw0, lb0 = torch.rand(C, device='cuda', generator=g) + 0.5, mk(C, scale=0.2)
    Nc = 128 if consumer == 'lin_EG' else 256
    wc0, bc0 = mk(Nc, C, scale=C ** -0.5), mk(Nc, scale=0.3)
    sc = None if producer == 'add_ln_noscale' else (torch.rand(B, device='cuda', generator=g) > 0.3).float() / 0.7
    if sc is not None:
        sc[1] = 0.0
    gs, gz = mk(B, N, N, C).to(dtype), mk(B, N, N, Nc).to(dtype)
    p = 0.1 if consumer.endswith('dropout') else 0.0
    runs = []
    for fused in (True, False):
        monkeypatch.setattr(ops, '_EPI_LN_BWD', fused)
        before = list(ops._lazy_dgrads)
        leaves = [t.clone().requires_grad_(True) for t in (x0, res0, w0, b0, lw0, lb0, wc0, bc0)]
        x, res, w, b, lw, lb, wc, bc = leaves
        torch.manual_seed(5)                                  # (the dropout seed of linear_gelu_dropout comes from the CPU generator)
        with torch.autocast('cuda', dtype=dtype):
            if producer.startswith('add_ln'):
                s, y = ops.add_layer_norm(x, res, sc, lw, lb, 1e-5)
            elif producer == 'lin_resid_ln':
                s, y = ops.linear_residual_layer_norm(x, w, b, res, sc, lw, lb, 1e-5)
            else:
                xs_ = x * sc.view(-1, 1, 1, 1).to(dtype)
                s, y = ops.linear_residual_layer_norm(xs_, w, b, res, sc, lw, lb, 1e-5, prescaled=True)
            z = ops.linear(y, wc, bc) if consumer == 'lin_EG' else ops.linear_gelu_dropout(y, wc, bc, p, True)
        ((s.float() * gs.float()).sum() + (z.float() * gz.float()).sum()).backward()
        torch.cuda.synchronize()
        after = list(ops._lazy_dgrads)
        assert (after[1] - before[1] == 1) == fused and (after[0] - before[0] == 1) == fused, (before, after)
        runs.append([s, z] + [t.grad for t in leaves])
    names = ['s', 'z', 'dx', 'dres', 'dW', 'db', 'dln_w', 'dln_b', 'dWc', 'dbc']
    for name, a, b_ in zip(names, *runs):
        if a is None or b_ is None:
            assert a is None and b_ is None, name
            continue
        tol = 3 * TOL[dtype] if name.startswith('d') else 1e-6
        assert rel(a, b_) < tol, (name, rel(a, b_))
        assert bool(torch.isfinite(a.float()).all()), name


def test_lazy_dgrad_token_carries_its_product():
    """the token a consumer returns instead of dx is a zero scalar expanded to the gradient's shape (no memory) that carries
    (dz, W); materialising it gives the product; writing into it is refused"""
    dz, w = torch.randn(64, 128, device='cuda', dtype=torch.bfloat16), torch.randn(128, 256, device='cuda', dtype=torch.bfloat16)
    tok = ops._lazy_dgrad(dz, w, (4, 16, 256))
    assert tok.shape == (4, 16, 256) and tok.stride() == (0, 0, 0) and float(tok.float().abs().max()) == 0.0
    got = ops._materialize_dgrad(tok)
    assert rel(got.view(64, 256), dz.double() @ w.double()) < TOL[torch.bfloat16]
    plain = torch.randn(4, 16, 256, device='cuda')
    assert ops._materialize_dgrad(plain) is plain and ops._take_lazy_dgrad(plain) is None


@pytest.mark.parametrize('consumers', ['one', 'two_linears', 'linear_and_other', 'retain_grad'])
def test_lazy_dgrad_handover_is_safe_for_any_use_of_the_layernorm_output(consumers, monkeypatch):
    """the LayerNorm entry offers the lazy data gradient on EVERY output y; a y with two consumers (two
    Linears, a Linear and something else), retain_grad or another hook must still get the complete gradient.  Every variant
    against the same graph with the hand-over switched off (TGT_EPI_LN_BWD=0 path), gradient by gradient."""
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)
    B, N, C = 3, 9, 256
    dt = torch.bfloat16
    g = torch.Generator(device='cuda').manual_seed(23)
    mk = lambda *shape, scale=1.0: torch.randn(*shape, device='cuda', generator=g) * scale
    x0, res0 = mk(B, N, N, C).to(dt), mk(B, N, N, C).to(dt)
    lw0, lb0 = torch.rand(C, device='cuda', generator=g) + 0.5, mk(C, scale=0.2)
    w10, b10, w20, b20 = mk(C, C, scale=C ** -0.5), mk(C, scale=0.1), mk(128, C, scale=C ** -0.5), mk(128, scale=0.1)
    go1, go2, gs = mk(B, N, N, C).to(dt), mk(B, N, N, 128).to(dt), mk(B, N, N, C).to(dt)
    outs = []
    for lazy in (True, False):
        monkeypatch.setattr(ops, '_EPI_LN_BWD', lazy)
        ops._lazy_dgrads[:] = [0, 0, 0]
        leaves = [t.clone().requires_grad_(True) for t in (x0, res0, lw0, lb0, w10, b10, w20, b20)]
        x, res, lw, lb, w1, b1, w2, b2 = leaves
        with torch.autocast('cuda', dtype=dt):
            s, y = ops.add_layer_norm(x, res, None, lw, lb)
            if consumers == 'retain_grad':
                y.retain_grad()
            loss = (ops.linear(y, w1, b1).float() * go1.float()).sum() + (s.float() * gs.float()).sum()
            if consumers == 'two_linears':
                loss = loss + (ops.linear(y, w2, b2).float() * go2.float()).sum()
            elif consumers == 'linear_and_other':
                loss = loss + (y.float() ** 2).sum() * 0.01
        loss.backward()
        if lazy:
            assert ops._lazy_dgrads[0] >= 1                                  # the Linear(s) did hand over
            if consumers == 'one':
                assert ops._lazy_dgrads[1] == 1 and ops._lazy_dgrads[2] == 0       # ... and the entry fused the only token
            if consumers in ('two_linears', 'linear_and_other'):
                assert ops._lazy_dgrads[1] == 0 and ops._lazy_dgrads[2] >= 1       # ... or the hook completed the gradient
        grads = [t.grad for t in leaves if t.grad is not None]
        assert all(bool(torch.isfinite(t.float()).all()) for t in grads)
        outs.append(grads + ([y.grad] if consumers == 'retain_grad' else []))
    assert len(outs[0]) == len(outs[1])
    for a, b_ in zip(*outs):
        assert rel(a, b_) < 2 * TOL[dt], (consumers, rel(a, b_))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('with_scale', [True, False])
def test_lin_O_residual_layer_norm_with_permuted_columns(dtype, with_scale, monkeypatch):
    """ops.linear_residual_layer_norm(col_perm=...): lin_O of the triplet modules (in_features 512, its input columns in the
    kernels' channel order) + DropPath + residual + the edge FFN's LayerNorm as ONE launch (K = 512 row kernel), against the
    composition linear_permuted_cols -> add_layer_norm: outputs and every gradient (reference triplet.py:248-249, layers.py:284-290)"""
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)
    B, N, C = 4, 11, 256
    g = torch.Generator(device='cuda').manual_seed(19)
    mk = lambda *shape, scale=1.0: torch.randn(*shape, device='cuda', generator=g) * scale
    va0, res0 = mk(B, N, N, 2 * C).to(dtype), mk(B, N, N, C).to(dtype)
    w0, b0 = mk(C, 2 * C, scale=(2 * C) ** -0.5), mk(C, scale=0.3)
    lw0, lb0 = torch.rand(C, device='cuda', generator=g) + 0.5, mk(C, scale=0.2)
    perm = torch.randperm(2 * C, device='cuda', generator=g).int()
    inv = torch.empty_like(perm)
    inv[perm.long()] = torch.arange(2 * C, device='cuda', dtype=torch.int32)
    sc = ((torch.rand(B, device='cuda', generator=g) > 0.3).float() / 0.7) if with_scale else None
    gs, gy = mk(B, N, N, C).to(dtype), mk(B, N, N, C).to(dtype)
    outs = []
    for fused in (True, False):
        monkeypatch.setattr(ops, '_EDGE_K512', fused)
        leaves = [t.clone().requires_grad_(True) for t in (va0, res0, w0, b0, lw0, lb0)]
        va, res, w, b, lw, lb = leaves
        with torch.autocast('cuda', dtype=dtype):
            s, y = ops.linear_residual_layer_norm(va, w, b, res, sc, lw, lb, 1e-5, col_perm=(perm, inv))
        assert (type(s.grad_fn).__name__ == '_LinearResidualLNBackward') == fused
        ((s.float() * gs.float()).sum() + (y.float() * gy.float()).sum()).backward()
        outs.append([s, y] + [t.grad for t in leaves])
    # float64 of the forward, independent of both paths
    z = va0.double() @ w0.to(dtype).double()[:, perm.long()].t() + b0.to(dtype).double()
    ref = res0.double() + (z if sc is None else z * sc.double().view(-1, 1, 1, 1))
    assert rel(outs[0][0], ref) < TOL[dtype]
    names = ['s', 'y', 'dva', 'dres', 'dW', 'db', 'dln_w', 'dln_b']
    for name, a, b_ in zip(names, *outs):
        tol = 3 * TOL[dtype] if name.startswith('d') else TOL[dtype]
        assert rel(a, b_) < tol, (name, rel(a, b_))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('rows', [1000, 4096 + 5])
def test_lin_O_data_gradient_on_the_wide_kernel_vs_library_and_float64(rows, dtype, monkeypatch):
    """the data gradient of a 512 -> 256 Linear on the edge rows (lin_O, reference triplet.py:248-249 under autograd) runs on
    edge_wide512_kernel (K = 256 -> N = 512, weights resident): against the library GEMM it replaces and against float64"""
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)
    g = torch.Generator(device='cuda').manual_seed(23)
    x0 = torch.randn(rows, 512, device='cuda', generator=g).to(dtype)
    w0 = torch.randn(256, 512, device='cuda', generator=g) * 512 ** -0.5
    dy = torch.randn(rows, 256, device='cuda', generator=g).to(dtype)
    grads = []
    for own in (True, False):
        monkeypatch.setattr(ops, '_EDGE_N512', own)
        x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
        with torch.autocast('cuda', dtype=dtype):
            y = ops.linear(x, w)
        y.backward(dy)
        grads.append((x.grad, w.grad))
    ref = dy.double() @ w0.to(dtype).double()
    assert rel(grads[0][0], ref) < TOL[dtype] and rel(grads[1][0], ref) < TOL[dtype]
    assert rel(grads[0][0], grads[1][0]) < TOL[dtype]
    assert torch.equal(grads[0][1], grads[1][1])            # (the weight gradient does not depend on the route)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_transpose_many_one_launch(dtype):
    """tgt_transpose_many (ABI 27): W^T of many 16-bit matrices in one launch, ragged shapes included -- what the Trainer refreshes
    after every optimizer step for the data-gradient launches (ops.WeightTransposes)"""
    import ctypes as C
    g = torch.Generator(device='cuda').manual_seed(5)
    shapes = [(256, 256), (128, 256), (256, 64), (256, 512), (33, 70), (1, 17), (100, 1), (64, 64)]
    src = [torch.randn(r, c, device='cuda', generator=g).to(dtype) for r, c in shapes]
    dst = [torch.full((c, r), 7.0, dtype=dtype, device='cuda') for r, c in shapes]
    rows = []
    for s_, d_, (r, c) in zip(src, dst, shapes):
        rows += [s_.data_ptr(), d_.data_ptr(), r | (c << 32)]
    table = torch.tensor(rows, dtype=torch.int64).cuda()
    L = _lib.lib()
    for blocks in (1, 16):
        for d_ in dst:
            d_.fill_(7.0)
        _lib.check(L.tgt_transpose_many(C.c_void_p(table.data_ptr()), len(shapes), blocks,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'tgt_transpose_many')
        torch.cuda.synchronize()
        for s_, d_ in zip(src, dst):
            assert torch.equal(d_, s_.t())
    _lib.check(L.tgt_transpose_many(None, 0, 16, C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'empty')


# ------------------------------------------------------------------------------------------------------------------
# Fused weight gradient (ABI 30, csrc/edge_wgrad.hip): the data-gradient launch of a 256 -> 256 edge Linear also returns dW = a^T X
# with X recomputed in the row phase.  The data gradient / column sums must equal the plain launch BIT FOR BIT (same k order, same
# epilogue arithmetic), dW is held to the float64 product of the stored operands (fp32 accumulation: 1e-5 at 262144 rows).
# ------------------------------------------------------------------------------------------------------------------
def _gelu_act64(pre, p, seed, sc, rps, dtype):
    """the forward's activation on the stored pre-activation: dropout(gelu(pre)) * sample_scale, by the standalone kernel"""
    act = torch.empty_like(pre)
    L = _lib.lib()
    if sc is None:
        _lib.check(L.tgt_gelu_dropout_fwd(pre.data_ptr(), act.data_ptr(), pre.numel(), ops._DT[dtype], p, seed, None), 'g')
    else:
        _lib.check(L.tgt_gelu_dropout_scaled_fwd(pre.data_ptr(), act.data_ptr(), pre.numel(), ops._DT[dtype], p, seed, sc.data_ptr(),
                                                 rps * pre.shape[1], None), 'g')
    return act


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('M,cap,with_scale', [(520, 0, True), (33, 0, False), (4096, 3, True), (1000, 1, False), (262144, 0, True)])
def test_fused_weight_gradient_gelu_backward(M, cap, with_scale, dtype, p):
    N = K = 256
    a, w, _, g = _mk(M, K, N, dtype, 11, bias=False)
    pre = torch.randn(M, N, device='cuda', generator=g).to(dtype)
    rps = 1024 if M == 262144 else 40
    sc = (torch.rand(math.ceil(M / rps), device='cuda', generator=g) + 0.5) if with_scale else None
    seed = 0x5eed if p else 0
    L = _lib.lib()
    L.tgt_edge_linear_set_grid_cap(cap)
    try:
        parts = L.tgt_edge_linear_parts(M, N)
        cs0, cs1 = torch.empty(parts, N, device='cuda'), torch.empty(parts, N, device='cuda')
        dwp = torch.full((parts, N, K), float('nan'), device='cuda')
        kw = dict(res=pre, out_scale=sc, rows_per_sample=rps if with_scale else 0, dropout=(p, seed))
        out0 = ops.edge_linear_raw(a, w, None, _lib.EPI_GELU_BWD, colsum_partial=cs0, **kw)
        out1 = ops.edge_linear_raw(a, w, None, _lib.EPI_GELU_BWD, colsum_partial=cs1, dw_partial=dwp, **kw)
    finally:
        L.tgt_edge_linear_set_grid_cap(0)
    torch.cuda.synchronize()
    assert torch.equal(out0, out1) and torch.equal(cs0.sum(0), cs1.sum(0))
    act = _gelu_act64(pre, p, seed, sc, rps, dtype)
    dw = dwp.sum(0)
    assert torch.isfinite(dw).all()
    # chunked float64 reference (a 262144-row float64 product in one piece would take 1 GB)
    ref = torch.zeros(N, K, dtype=torch.float64, device='cuda')
    for i in range(0, M, 32768):
        ref += a[i:i + 32768].double().t() @ act[i:i + 32768].double()
    assert rel(dw, ref) < 2e-5, rel(dw, ref)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('M,cap,with_ds,with_scale', [(300, 0, True, True), (1024, 2, False, False), (4100, 1, True, False), (262144, 0, True, True)])
def test_fused_weight_gradient_layernorm_backward(M, cap, with_ds, with_scale, dtype):
    N = K = 256
    a, w, _, g = _mk(M, K, N, dtype, 12, bias=False)
    s = (torch.randn(M, N, device='cuda', generator=g) * 1.3 + 0.2).to(dtype)
    gamma = torch.rand(N, device='cuda', generator=g) + 0.5
    beta = torch.randn(N, device='cuda', generator=g) * 0.3
    # the forward's y / mean / rstd, by the LayerNorm kernel on the stored stream rows
    y = torch.empty_like(s)
    mean, rstd = torch.empty(M, device='cuda'), torch.empty(M, device='cuda')
    L = _lib.lib()
    _lib.check(L.tgt_layer_norm_fwd(s.data_ptr(), ops._DT[dtype], gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), ops._DT[dtype],
                                    mean.data_ptr(), rstd.data_ptr(), M, N, 1e-5, None), 'ln')
    ds = torch.randn(M, N, device='cuda', generator=g).to(dtype) if with_ds else None
    rps = 1024 if M == 262144 else 50
    sc = (torch.rand(math.ceil(M / rps), device='cuda', generator=g) + 0.5) if with_scale else None
    L.tgt_edge_linear_set_grid_cap(cap)
    try:
        parts = L.tgt_edge_linear_parts(M, N)
        outs = []
        for fused in (False, True):
            partial = torch.empty(parts, 3 * N, device='cuda')
            dres = torch.empty(M, N, dtype=dtype, device='cuda')
            dx = torch.empty(M, N, dtype=dtype, device='cuda') if with_scale else None
            dwp = torch.full((parts, N, K), float('nan'), device='cuda') if fused else None
            ops.edge_linear_raw(a, w, None, _lib.EPI_LN_BWD, ln=(gamma, beta if fused else None, 1e-5), stats=(mean, rstd), res=s, ds_in=ds,
                                out=dres, out2=dx, row_scale=sc, rows_per_sample=rps if with_scale else 0, colsum_partial=partial,
                                dw_partial=dwp)
            outs.append((dres, dx, partial.sum(0), dwp))
    finally:
        L.tgt_edge_linear_set_grid_cap(0)
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][2], outs[1][2])
    if with_scale:
        assert torch.equal(outs[0][1], outs[1][1])
    dw = outs[1][3].sum(0)
    assert torch.isfinite(dw).all()
    ref = torch.zeros(N, K, dtype=torch.float64, device='cuda')
    for i in range(0, M, 32768):
        ref += a[i:i + 32768].double().t() @ y[i:i + 32768].double()
    # X is recomputed from (s, mean, rstd): a last-bit difference to the stored y on a few elements is possible (fma contraction), hence
    # not the 1e-5 of the GELU form
    assert rel(dw, ref) < 2e-4, rel(dw, ref)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('p', [0.0, 0.1])
def test_ffn_block_backward_with_fused_weight_gradient_equals_the_unfused_step(dtype, p, monkeypatch):
    """the edge FFN through ops.linear_gelu_dropout + ops.linear_residual_layer_norm: TGT_EDGE_WGRAD on / off give the same gradients
    (lin_W2's weight gradient: fp32 sums in another order, everything else bit for bit)"""
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)
    B, Nn, C_ = 3, 12, 256
    g = torch.Generator(device='cuda').manual_seed(77)
    x0 = torch.randn(B, Nn, Nn, C_, device='cuda', generator=g).to(dtype)
    res0 = torch.randn(B, Nn, Nn, C_, device='cuda', generator=g).to(dtype)
    W1 = (torch.randn(C_, C_, device='cuda', generator=g) / 16).requires_grad_()
    b1 = (torch.randn(C_, device='cuda', generator=g) * 0.1).requires_grad_()
    W2 = (torch.randn(C_, C_, device='cuda', generator=g) / 16).requires_grad_()
    b2 = (torch.randn(C_, device='cuda', generator=g) * 0.1).requires_grad_()
    lw = (torch.rand(C_, device='cuda', generator=g) + 0.5).requires_grad_()
    lb = (torch.randn(C_, device='cuda', generator=g) * 0.1).requires_grad_()
    scale = torch.tensor([1.25, 0.0, 1.25], device='cuda')
    gs = torch.randn(B, Nn, Nn, C_, device='cuda', generator=g).to(dtype)
    gy = torch.randn(B, Nn, Nn, C_, device='cuda', generator=g).to(dtype)
    results = []
    for fused in (False, True):
        monkeypatch.setattr(ops, '_EDGE_WGRAD', fused)
        ops.reset_random_pools()
        torch.manual_seed(5)
        x = x0.clone().requires_grad_()
        res = res0.clone().requires_grad_()
        with torch.autocast('cuda', dtype=dtype):
            act = ops.linear_gelu_dropout(x, W1, b1, p, True, sample_scale=scale)
            s, y = ops.linear_residual_layer_norm(act, W2, b2, res, scale, lw, lb, prescaled=True)
        grads = torch.autograd.grad([s, y], [x, res, W1, b1, W2, b2, lw, lb], [gs, gy])
        results.append(grads)
    # float64 weight gradient of lin_W2 from the stored operands (at this row count the unfused path is ONE 16-bit GEMM, i.e. rounded
    # to the storage type; the fused launch keeps fp32)
    for i, (g0, g1) in enumerate(zip(*results)):
        if i == 4:
            assert rel(g1, g0) < TOL[dtype], rel(g1, g0)
        else:
            assert torch.equal(g0, g1), i
