"""The gated activations of the FFN block (geglu / glu / swiglu: reference lib/tgt/layers/activations.py:4-25) on the HIP kernels:
the streaming pair tgt_glu_dropout_fwd / _bwd (csrc/glu.hip), the TGT_EPI_GLU epilogue of the 256 -> 512 edge-row GEMM
(csrc/edge_glu.hip), and FFN / TGT_Layer on top of them.

Error bars.  Every comparison against float64 is RELATIVE TO TORCH'S OWN COMPOSITION in the same dtype on the same stored inputs:
    err_new = max|new - f64|  <=  2 * err_eager + floor,      err_eager = max|eager - f64|,   floor = 1.5e-7 * max|e|
(the factor two covers another summation / rounding order, the floor is the documented bound of the erf approximation in gelu_cdf
times the largest linear-half value).  The ratio err_new / (2 err_eager + floor) of every comparison is filed in the parity log
(TGT_PARITY_LOG, group `glu`)."""
import math

import pytest
import torch
import torch.nn.functional as F

import golden_util as gu
import parity_log
from oracle import modules as om

from tgt_amd import _lib, ops

pytestmark = pytest.mark.gpu

KINDS = ['geglu', 'glu', 'swiglu']
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
GATE = {'geglu': F.gelu, 'glu': torch.sigmoid, 'swiglu': F.silu}


def bar(name, new, eager, ref, e_max):
    """the stated bar (module docstring) for one tensor; files the ratio under `glu`"""
    ref = ref.detach().double()
    err_new = float((new.detach().double() - ref).abs().max())
    err_eager = float((eager.detach().double() - ref).abs().max())
    bound = 2.0 * err_eager + 1.5e-7 * float(e_max)
    parity_log.Tol.last = 'glu'
    parity_log.record(err_new / bound)
    print(f'{name}: err_new {err_new:.3e} err_eager {err_eager:.3e} bound {bound:.3e} ratio {err_new / bound:.3f}')
    assert err_new <= bound, (name, err_new, err_eager, bound)


def compose(x, kind):
    """torch's own composition (the reference's activation) in x's dtype"""
    g, e = x.chunk(2, dim=-1)
    return e * GATE[kind](g)


def glu_fwd(x, kind, p=0.0, seed=0, scale=None, eps_=0):
    rows, cols = x.numel() // x.shape[-1], x.shape[-1] // 2
    y = torch.empty(*x.shape[:-1], cols, dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().tgt_glu_dropout_fwd(x.data_ptr(), y.data_ptr(), rows, cols, _lib.GLU_KINDS[kind], ops._DT[x.dtype], p, seed,
                                              None if scale is None else scale.data_ptr(), eps_, None), 'tgt_glu_dropout_fwd')
    return y


def glu_bwd(x, dy, kind, p=0.0, seed=0, scale=None, eps_=0):
    rows, cols = x.numel() // x.shape[-1], x.shape[-1] // 2
    dx = torch.empty_like(x)
    _lib.check(_lib.lib().tgt_glu_dropout_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), rows, cols, _lib.GLU_KINDS[kind],
                                              ops._DT[x.dtype], p, seed, None if scale is None else scale.data_ptr(), eps_, None),
               'tgt_glu_dropout_bwd')
    return dx


def keep_pattern(rows, cols, dtype, p, seed):
    """the generator's keep mask over (rows, cols): the forward of an input whose activation is nowhere zero"""
    return glu_fwd(torch.ones(rows, 2 * cols, dtype=dtype, device='cuda'), 'glu', p, seed) != 0


def _inputs(rows, cols, dtype, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(rows, 2 * cols, device='cuda', generator=g).to(dtype)
    dy = torch.randn(rows, cols, device='cuda', generator=g).to(dtype)
    return x, dy


# (3, 8): one vector per row in fp16; (67, 256): the edge width, odd rows, more than one block; (5, 768): the node width;
# (1024, 24): rows of three vectors, a divisor that is no power of two
SHAPES = [(3, 8), (67, 256), (5, 768), (1024, 24)]


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('rows,cols', SHAPES)
def test_streaming_pair_matches_float64(rows, cols, kind, dtype):
    x, dy = _inputs(rows, cols, dtype, 11)
    x64 = x.double().requires_grad_(True)
    y64 = compose(x64, kind)
    y64.backward(dy.double())
    xe = x.clone().requires_grad_(True)
    ye = compose(xe, kind)
    ye.backward(dy)
    xn = x.clone().requires_grad_(True)
    yn = ops.glu_dropout(xn, kind, 0.3, False)            # eval mode: p is forced to 0
    assert yn.shape == (rows, cols) and yn.dtype == dtype
    yn.backward(dy)
    e_max = x[:, cols:].abs().max()
    bar('y', yn, ye, y64, e_max)
    bar('d_g', xn.grad[:, :cols], xe.grad[:, :cols], x64.grad[:, :cols], e_max)
    bar('d_e', xn.grad[:, cols:], xe.grad[:, cols:], x64.grad[:, cols:], e_max)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('rows,cols', SHAPES)
def test_streaming_pair_dropout_and_sample_scale(rows, cols, kind, dtype):
    p, seed = 0.25, 0x5eed1234
    x, dy = _inputs(rows, cols, dtype, 12)
    rps = (rows + 2) // 3                                   # three samples (the last one may be short), whole rows each
    scale = torch.tensor([1.25, 0.0, 1.0], device='cuda')[:(rows + rps - 1) // rps].contiguous()
    eps_ = rps * cols
    y0, dx0 = glu_fwd(x, kind), glu_bwd(x, dy, kind)
    y, dx = glu_fwd(x, kind, p, seed, scale, eps_), glu_bwd(x, dy, kind, p, seed, scale, eps_)
    keep = keep_pattern(rows, cols, dtype, p, seed)
    assert 0 < int(keep.sum()) < keep.numel() or keep.numel() < 64
    assert torch.all(y[~keep] == 0)
    assert torch.all(dx[:, :cols][~keep] == 0) and torch.all(dx[:, cols:][~keep] == 0)
    # kept values: the p = 0 values times scale / (1 - p) (the factor as the kernel forms it, in fp32) within one rounding of the
    # dtype: got = round(r k) and want = round(r) k are each half an ulp from r k, i.e. eps (1 + eps / 2) |want| apart at most
    k = (torch.tensor(1.0, device='cuda') / torch.tensor(1.0 - p, device='cuda', dtype=torch.float32)) * scale
    k = k.repeat_interleave(rps)[:rows, None].double()
    fi = torch.finfo(dtype)
    for name, got, base in (('y', y, y0), ('d_g', dx[:, :cols], dx0[:, :cols]), ('d_e', dx[:, cols:], dx0[:, cols:])):
        want = base.double() * k
        err = (got.double() - want).abs()
        assert torch.all(err[keep] <= fi.eps * (1 + fi.eps) * want.abs()[keep] + fi.smallest_normal), (name, float(err[keep].max()))
    # the same seed gives the same result; another seed another pattern
    assert torch.equal(y, glu_fwd(x, kind, p, seed, scale, eps_))
    assert torch.equal(dx, glu_bwd(x, dy, kind, p, seed, scale, eps_))
    if keep.numel() >= 64:
        assert not torch.equal(keep, keep_pattern(rows, cols, dtype, p, seed + 1))


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
def test_streaming_kept_fraction(dtype):
    keep = keep_pattern(1024, 256, dtype, 0.25, 0xabcdef)     # 262144 outputs; 5 binomial standard deviations = 0.0043
    assert abs(float(keep.float().mean()) - 0.75) <= 0.0043


def test_ops_glu_dropout_draws_a_seed_and_saves_only_x():
    x, dy = _inputs(64, 256, torch.bfloat16, 13)
    scale = torch.tensor([2.0, 0.0], device='cuda')
    torch.manual_seed(5)
    xn = x.view(2, 32, 512).clone().requires_grad_(True)
    y = ops.glu_dropout(xn, 'swiglu', 0.25, True, scale)
    assert [t.shape for t in y.grad_fn.saved_tensors if t is not None and t.dim() > 1] == [xn.shape]
    y.backward(dy.view(2, 32, 256))
    assert torch.all(y[1] == 0) and torch.all(xn.grad[1] == 0)
    kept = float((y[0] != 0).float().mean())
    assert abs(kept - 0.75) < 5 * math.sqrt(0.75 * 0.25 / y[0].numel())
    torch.manual_seed(5)
    assert torch.equal(y, ops.glu_dropout(xn.detach(), 'swiglu', 0.25, True, scale))
    assert not torch.equal(y, ops.glu_dropout(xn.detach(), 'swiglu', 0.25, True, scale))      # the next seed
    with pytest.raises(RuntimeError, match='unknown gated activation'):
        ops.glu_dropout(xn, 'reglu', 0.0, False)


# ---------------------------------------------------------------------------------------------------------------
# TGT_EPI_GLU
# ---------------------------------------------------------------------------------------------------------------
GUARD = 3


def _glu_launch(a, w, b, kind, p, seed, scale, rps, wide):
    """(out2 buffer, its view, out buffer, its view): guard rows behind both, out2 optionally with padded rows (ldo2 = 576)"""
    M = a.shape[0]
    buf2 = torch.full((M + GUARD, 576 if wide else 512), 7.0, dtype=a.dtype, device='cuda')
    buf = torch.full((M + GUARD, 256), 7.0, dtype=a.dtype, device='cuda')
    out2, out = buf2[:M, :512], buf[:M]
    ops.edge_linear_raw(a, w, b, _lib.EPI_GLU, out=out, out2=out2, dropout=(p, seed), row_scale=scale, rows_per_sample=rps,
                        flags=_lib.GLU_KINDS[kind] << _lib.EDGE_GLU_KIND_SHIFT)
    return buf2, out2, buf, out


@pytest.fixture
def grid_cap(request):
    _lib.lib().tgt_edge_linear_set_grid_cap(request.param)
    yield request.param
    _lib.lib().tgt_edge_linear_set_grid_cap(0)


@pytest.mark.parametrize('grid_cap', [0, 1, 3], indirect=True)
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('M', [33, 520, 1000])
def test_glu_epilogue(M, dtype, grid_cap):
    """out2 bit-equal to the TGT_EPI_BIAS launch, out bit-equal to tgt_glu_dropout_fwd on it, both against float64, nothing
    written at or past row M; grid caps 1 and 3: one workgroup walks several tiles and a tail tile"""
    g = torch.Generator(device='cuda').manual_seed(M)
    a = torch.randn(M, 256, device='cuda', generator=g).to(dtype)
    w = (torch.randn(512, 256, device='cuda', generator=g) / 16).to(dtype)
    bias = (torch.randn(512, device='cuda', generator=g) * 0.5).to(dtype)
    rps = 8
    sc_all = torch.tensor([0.0, 1.0, 1.25], device='cuda')[torch.randint(0, 3, (M // rps,), device='cuda', generator=g)].contiguous()
    case = 0
    for b in (bias, None):
        plain = ops.edge_linear_raw(a, w, b)                              # TGT_EPI_BIAS on the same operands
        pre64 = a.double() @ w.double().t() + (0 if b is None else b.double())
        pre_e = F.linear(a, w, b)
        e_max = pre64[:, 256:].abs().max()
        for scale in ((sc_all, None) if M % rps == 0 else (None,)):
            for p in (0.0, 0.1):
                kind, case = KINDS[case % 3], case + 1
                seed = 0x77aa55 + case if p else 0
                buf2, out2, buf, out = _glu_launch(a, w, b, kind, p, seed, scale, rps if scale is not None else 0, wide=case % 2 == 0)
                assert torch.equal(out2, plain), (kind, p, case)
                y = glu_fwd(out2.contiguous(), kind, p, seed, scale, rps * 256 if scale is not None else 0)
                assert torch.equal(out, y), (kind, p, case)
                assert torch.all(buf2[M:] == 7.0) and torch.all(buf2[:, 512:] == 7.0) and torch.all(buf[M:] == 7.0)
                # float64: the activation of the float64 pre-activation under the same keep pattern and factors
                k = torch.ones(M, 1, device='cuda') if scale is None else scale.repeat_interleave(rps)[:, None]
                if p:
                    k = k * keep_pattern(M, 256, dtype, p, seed) / torch.tensor(1.0 - p, device='cuda', dtype=torch.float32)
                bar(f'{kind} p={p} out2', out2, pre_e, pre64, e_max)
                # (torch's dropout / scaling of a 16-bit tensor: fp32 arithmetic on the stored activation, one more rounding)
                bar(f'{kind} p={p} out', out, (compose(pre_e, kind).float() * k).to(dtype), compose(pre64, kind) * k.double(), e_max)


def test_glu_epilogue_supported_shapes_and_refusals():
    assert ops.edge_linear_supported(256, 512, torch.bfloat16, _lib.EPI_GLU)
    assert ops.edge_linear_supported(256, 512, torch.float16, _lib.EPI_GLU, row_scale=True)
    assert not ops.edge_linear_supported(128, 512, torch.bfloat16, _lib.EPI_GLU)
    assert not ops.edge_linear_supported(256, 256, torch.bfloat16, _lib.EPI_GLU)
    q = _lib.EdgeLinearArgs()
    q.M, q.K, q.N, q.dtype, q.epilogue = 128, 256, 512, _lib.TGT_F32, _lib.EPI_GLU
    assert _lib.lib().tgt_edge_linear_supported(q) == 0
    q.dtype, q.flags = _lib.TGT_BF16, 3 << _lib.EDGE_GLU_KIND_SHIFT                   # no such kind
    assert _lib.lib().tgt_edge_linear_supported(q) == 0
    for K, N, dtype in ((128, 512, torch.bfloat16), (256, 256, torch.bfloat16), (256, 512, torch.float32)):
        a = torch.zeros(64, K, dtype=dtype, device='cuda')
        w = torch.zeros(N, K, dtype=dtype, device='cuda')
        with pytest.raises(RuntimeError, match=r'code 2\).*unsupported'):
            ops.edge_linear_raw(a, w, None, _lib.EPI_GLU, out=torch.empty(64, N // 2, dtype=dtype, device='cuda'),
                                out2=torch.empty(64, N, dtype=dtype, device='cuda'))
    a = torch.zeros(64, 256, dtype=torch.bfloat16, device='cuda')
    w = torch.zeros(512, 256, dtype=torch.bfloat16, device='cuda')
    with pytest.raises(RuntimeError, match='epilogue operand missing'):
        ops.edge_linear_raw(a, w, None, _lib.EPI_GLU, out=torch.empty(64, 256, dtype=torch.bfloat16, device='cuda'))


# ---------------------------------------------------------------------------------------------------------------
# FFN and TGT_Layer
# ---------------------------------------------------------------------------------------------------------------
def _ffn_run(ffn, x, dy, dtype):
    x = x.clone().requires_grad_(True)
    ctx = torch.autocast('cuda', dtype=dtype) if dtype is not None else torch.autocast('cuda', enabled=False)
    with ctx:
        y = ffn(x)
    y.backward(dy.to(y.dtype))
    return y, x.grad, {k: p.grad for k, p in ffn.named_parameters()}


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('activation', KINDS)
@pytest.mark.parametrize('shape', [(2, 9, 9, 256), (2, 9, 768)], ids=['edge256', 'node768'])
def test_ffn_matches_the_oracle(shape, activation, dtype, monkeypatch):
    """FFN under autocast against oracle.modules.FFN in float64 with the same state_dict; torch's own composition = the oracle module
    in float32 under the same autocast.  Edge rows take the fused launch (256 -> 512), node rows the library GEMM + streaming pair."""
    from tgt_amd.tgt.layers.blocks import FFN
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)
    width = shape[-1]
    g = torch.Generator(device='cuda').manual_seed(21)
    x = torch.randn(*shape, device='cuda', generator=g)
    dy = torch.randn(*shape, device='cuda', generator=g)
    new = gu.fill_params(FFN(width, 1., act_dropout=0., activation=activation), seed=4).cuda().train()
    eager = gu.fill_params(om.FFN(width, 1., 0., activation), seed=4).cuda().train()
    ref = gu.fill_params(om.FFN(width, 1., 0., activation), seed=4).cuda().double().train()
    prof = ops.profile_kernels(True)
    try:
        yn, dxn, gn = _ffn_run(new, x, dy, dtype)
    finally:
        ops.profile_kernels(False)
    if width == 256:
        assert 'tgt_edge_linear' in prof and len(prof['tgt_glu_dropout_bwd']) == 1 and 'tgt_glu_dropout_fwd' not in prof, sorted(prof)
    else:
        assert len(prof['tgt_glu_dropout_fwd']) == 1 and len(prof['tgt_glu_dropout_bwd']) == 1, sorted(prof)
    ye, dxe, ge = _ffn_run(eager, x, dy, dtype)
    y6, dx6, g6 = _ffn_run(ref, x.double(), dy.double(), None)
    with torch.no_grad():
        e_max = ref.lin_W1(ref.ffn_ln(x.double()))[..., width:].abs().max()
    bar('y', yn, ye, y6, e_max)
    bar('dx', dxn, dxe, dx6, e_max)
    assert sorted(gn) == sorted(g6)
    for k in sorted(g6):
        bar(k, gn[k], ge[k], g6[k], e_max)


@pytest.mark.parametrize('shape', [(4, 9, 9, 256), (4, 9, 768)], ids=['edge256', 'node768'])
def test_ffn_hidden_folds_the_drop_path_factor(shape, monkeypatch):
    """hidden(x, sample_scale): a graph whose factor is 0 gets exactly zero activation and sends exactly zero gradient back"""
    from tgt_amd.tgt.layers.blocks import FFN
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)
    ffn = gu.fill_params(FFN(shape[-1], 1., act_dropout=0.1, activation='geglu'), seed=6).cuda().train()
    assert ffn.can_fold_scale()
    x = torch.randn(*shape, device='cuda').requires_grad_(True)
    scale = torch.tensor([2.0, 0.0, 2.0, 2.0], device='cuda')
    with torch.autocast('cuda', dtype=torch.bfloat16):
        hid = ffn.hidden(x, scale)
    assert hid.shape == shape and hid.dtype == torch.bfloat16
    hid.backward(torch.ones_like(hid))
    assert torch.all(hid[1] == 0) and torch.all(x.grad[1] == 0)
    assert float(hid[0].abs().max()) > 0 and float(x.grad[0].abs().max()) > 0
    assert all(torch.isfinite(p.grad).all() for p in (ffn.lin_W1.weight, ffn.lin_W1.bias))


class _FixedScales:
    """stands in for the DropPath factor pool: a fixed cycle of factors (keep probability 0.5), every graph dropped somewhere"""
    cycle = ([2.0, 0.0, 2.0, 2.0], [2.0, 2.0, 0.0, 2.0], [0.0, 2.0, 2.0, 0.0])
    n = 0

    @classmethod
    def take(cls, B, keep, device):
        cls.n += 1
        return torch.tensor(cls.cycle[cls.n % 3], device=device)


def test_two_layer_swiglu_stack_with_drop_path(monkeypatch):
    """Two TGT layers, swiglu, DropPath 0.5 and activation dropout in train mode (B = 4, N = 9) under bf16 autocast: the FFN's
    DropPath factor folded into the activation (FFN.can_fold_scale) against the same model with the factor applied at the residual
    add, on the same factors and seeds -- the bars of test_hip_model.py::test_drop_path_folded_into_producers_matches_the_plain_wiring
    (one more bf16 rounding per branch and layer)."""
    from tgt_amd.tgt import Graph, TGT_Encoder
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)
    monkeypatch.setattr(ops, '_scale_pool', _FixedScales)
    B, N, W, C = 4, 9, 768, 256
    kw = dict(node_width=W, edge_width=C, num_heads=64, activation='swiglu', scale_degree=True, node_update=True, edge_update=True,
              triplet_heads=0, node_ffn_multiplier=1., edge_ffn_multiplier=1., source_dropout=0.,
              drop_path=TGT_Encoder.IndivConfig([0.5, 0.5]), node_act_dropout=0., edge_act_dropout=0.1)
    g = torch.Generator(device='cuda').manual_seed(3)
    h0 = torch.randn(B, N, W, device='cuda', generator=g)
    e0 = torch.randn(B, N, N, C, device='cuda', generator=g)
    mask = gu.additive_mask([9, 5, 9, 7], N, torch.float32).cuda()
    gh, ge = torch.randn(B, N, W, device='cuda', generator=g), torch.randn(B, N, N, C, device='cuda', generator=g)
    runs = []
    for fold in (True, False):
        monkeypatch.setattr(ops, '_PRESCALE', fold)
        model = gu.fill_params(TGT_Encoder(model_height=2, **kw), seed=9).cuda().train()
        seen = []
        for layer in model.TGT_layers:
            def hidden(x, sample_scale=None, orig=layer.edge_ffn.hidden):
                out = orig(x, sample_scale)
                seen.append((sample_scale, out.detach()))
                return out
            layer.edge_ffn.hidden = hidden
        torch.manual_seed(123)
        _FixedScales.n = 0
        h, e = h0.clone().requires_grad_(True), e0.clone().requires_grad_(True)
        prof = ops.profile_kernels(True)
        try:
            with torch.autocast('cuda', dtype=torch.bfloat16):
                out = model(Graph(h=h, e=e, mask=mask))
            ((out.h.float() * gh).sum() + (out.e.float() * ge).sum()).backward()
            torch.cuda.synchronize()
        finally:
            ops.profile_kernels(False)
        # the node FFNs run the streaming pair, the edge FFNs the fused launch and the streaming backward
        assert len(prof['tgt_glu_dropout_fwd']) == 2 and len(prof['tgt_glu_dropout_bwd']) == 4 and 'tgt_edge_linear' in prof, sorted(prof)
        assert len(seen) == 2
        for sample_scale, hid in seen:
            assert (sample_scale is not None) == fold
            if fold:                                        # a dropped graph: exactly zero FFN-branch input of lin_W2
                assert int((sample_scale == 0).sum()) >= 1
                assert torch.all(hid[sample_scale == 0] == 0) and float(hid[sample_scale != 0].abs().max()) > 0
        grads = {k: p.grad for k, p in model.named_parameters()}
        assert all(torch.isfinite(t).all() for t in (out.h, out.e, h.grad, e.grad)) and \
            all(torch.isfinite(t).all() for t in grads.values() if t is not None)
        runs.append((out.h.detach(), out.e.detach(), h.grad, e.grad, grads))
    a, b = runs

    def rel(u, v):
        return float((u.double() - v.double()).norm() / (v.double().norm() + 1e-30))
    for i, name in enumerate(('h', 'e', 'dh', 'de')):
        assert rel(a[i], b[i]) < (2e-2 if i < 2 else 4e-2), (name, rel(a[i], b[i]))
    for k in b[4]:
        assert (a[4][k] is None) == (b[4][k] is None), k
        if b[4][k] is not None and float(b[4][k].abs().max()) > 0:
            assert rel(a[4][k], b[4][k]) < 6e-2, (k, rel(a[4][k], b[4][k]))
