"""The plain activations of the FFN block (relu / silu / elu: reference lib/tgt/layers/activations.py:21-25) on the HIP kernels:
the streaming pair tgt_act_dropout_fwd / _bwd (csrc/act.hip), the TGT_EPI_ACT / TGT_EPI_ACT_BWD epilogues of the edge-row GEMM
(csrc/edge_act.hip), ops.act_dropout / linear_act_dropout, and FFN / TGT_Encoder on top of them.

Error bars.  Kernel level: the per-element bars of tests/act_hard_inputs.py (one rounding into the storage type + a counted float32
floor) against float64 on the values as stored.  Module level: the bar of tests/test_hip_glu.py, relative to torch's own composition
in the same dtype on the same inputs,  err_new <= 2 err_eager + 1.5e-7 max|pre-activation|.  Ratios go to the parity log (`act`)."""
import math

import pytest
import torch

import act_hard_inputs as ah
import golden_util as gu
import parity_log
from oracle import modules as om

from tgt_amd import _lib, ops

pytestmark = pytest.mark.gpu

KINDS = list(ah.KINDS)
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ['f32', 'bf16', 'f16']


def _scale_ptr(scale):
    return None if scale is None else scale.data_ptr()


def act_fwd(x, kind, p=0.0, seed=0, scale=None, eps_=0):
    y = torch.empty_like(x)
    _lib.check(_lib.lib().tgt_act_dropout_fwd(x.data_ptr(), y.data_ptr(), x.numel(), _lib.ACT_KINDS[kind], ops._DT[x.dtype], p, seed,
                                              _scale_ptr(scale), eps_, None), 'tgt_act_dropout_fwd')
    return y


def act_bwd(x, dy, kind, p=0.0, seed=0, scale=None, eps_=0):
    dx = torch.empty_like(x)
    _lib.check(_lib.lib().tgt_act_dropout_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), _lib.ACT_KINDS[kind], ops._DT[x.dtype],
                                              p, seed, _scale_ptr(scale), eps_, None), 'tgt_act_dropout_bwd')
    return dx


def ratio(name, r):
    parity_log.Tol.last = 'act'
    parity_log.record(r)
    assert r <= 1.0, (name, r)


def check_case(tag, x, dy, kind, y, dx, dtype):
    """y, dx of the kernels against the float64 case of the stored x, dy at the bars of act_hard_inputs"""
    case = ah.act_case(x, dy, kind)
    valid = ah.sweep_valid(x)
    for name, new in (('y', y), ('dx', dx)):
        _, ref, s = case[name]
        ratio(f'{tag} {kind} {name}', ah.act_ratio(f'{tag} {kind} {name}', new, ref, s, dtype, ah.FLOOR[(kind, name)], valid))


def _inputs(rows, cols, dtype, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = (torch.randn(rows, cols, device='cuda', generator=g) * 2).to(dtype)
    dy = torch.randn(rows, cols, device='cuda', generator=g).to(dtype)
    return x, dy


# (3, 8): one vector per row in fp16; (67, 256): the edge width, odd rows, more than one block; (5, 768): the node width;
# (1024, 24): rows of three vectors
SHAPES = [(3, 8), (67, 256), (5, 768), (1024, 24)]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('rows,cols', SHAPES)
def test_streaming_pair_matches_float64(rows, cols, kind, dtype):
    x, dy = _inputs(rows, cols, dtype, 11)
    xn = x.clone().requires_grad_(True)
    yn = ops.act_dropout(xn, kind, 0.3, False)            # eval mode: p is forced to 0
    assert yn.shape == (rows, cols) and yn.dtype == dtype
    yn.backward(dy)
    check_case('ops', x, dy, kind, yn.detach(), xn.grad, dtype)
    assert torch.equal(yn.detach(), act_fwd(x, kind)) and torch.equal(xn.grad, act_bwd(x, dy, kind))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('rows,cols', SHAPES)
def test_streaming_pair_dropout_and_sample_scale(rows, cols, kind, dtype):
    p, seed = 0.25, 0x5eed1234
    x, dy = _inputs(rows, cols, dtype, 12)
    x = torch.where(x == 0, torch.ones_like(x), x)          # (no exact zeros: a zero output then means dropped -- relu aside)
    rps = (rows + 2) // 3                                   # three samples (the last one may be short), whole rows each
    scale = torch.tensor([1.25, 0.0, 1.0], device='cuda')[:(rows + rps - 1) // rps].contiguous()
    eps_ = rps * cols
    y0, dx0 = act_fwd(x, kind), act_bwd(x, dy, kind)
    y, dx = act_fwd(x, kind, p, seed, scale, eps_), act_bwd(x, dy, kind, p, seed, scale, eps_)
    # the keep pattern: the numpy restatement of the generator, and what the GELU kernel draws for the same (seed, element)
    keep = torch.from_numpy(ah.keep_pattern_np(rows * cols, x.element_size(), p, seed)).view(rows, cols).cuda()
    ones, kd = torch.ones_like(x), torch.empty_like(x)
    _lib.check(_lib.lib().tgt_gelu_dropout_fwd(ones.data_ptr(), kd.data_ptr(), ones.numel(), ops._DT[dtype], p, seed, None), 'gd')
    assert torch.equal(keep, kd != 0)
    live = scale.repeat_interleave(rps)[:rows, None].expand(rows, cols) != 0
    assert torch.all(y[~keep] == 0) and torch.all(dx[~keep] == 0) and torch.all(y[~live] == 0) and torch.all(dx[~live] == 0)
    if kind != 'relu':
        assert torch.equal(y != 0, keep & live & (y0 != 0))
    # kept values: the p = 0 values times scale / (1 - p) (the factor as the kernel forms it, in fp32) within one rounding of the
    # dtype: got = round(r k) and want = round(r) k are each half an ulp from r k, i.e. eps (1 + eps / 2) |want| apart at most
    k = (torch.tensor(1.0, device='cuda') / torch.tensor(1.0 - p, device='cuda', dtype=torch.float32)) * scale
    k = k.repeat_interleave(rps)[:rows, None].double()
    fi = torch.finfo(dtype)
    for name, got, base in (('y', y, y0), ('dx', dx, dx0)):
        want = base.double() * k
        err = (got.double() - want).abs()
        assert torch.all(err[keep] <= fi.eps * (1 + fi.eps) * want.abs()[keep] + fi.smallest_normal), (name, float(err[keep].max()))
    # the same seed gives the same result; another seed another pattern
    assert torch.equal(y, act_fwd(x, kind, p, seed, scale, eps_)) and torch.equal(dx, act_bwd(x, dy, kind, p, seed, scale, eps_))
    if keep.numel() >= 64:
        assert not torch.equal(y != 0, act_fwd(x, kind, p, seed + 1, scale, eps_) != 0)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_streaming_kept_fraction(dtype):
    keep = act_fwd(torch.ones(1024, 256, dtype=dtype, device='cuda'), 'silu', 0.25, 0xabcdef) != 0
    assert abs(float(keep.float().mean()) - 0.75) <= 0.0043      # 262144 outputs; 5 binomial standard deviations = 0.0043


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_relu_is_exact_and_propagates_nan(dtype):
    x = ah.activation_sweep(dtype).cuda()
    y = act_fwd(x, 'relu')
    want = torch.relu(x)
    assert torch.equal(y, want)                              # (torch.equal: -0 == +0, the signed zero aside)
    assert torch.equal(act_bwd(x, torch.full_like(x, 3.0), 'relu'), torch.where(x > 0, 3.0, 0.0).to(dtype))      # derivative 0 at 0
    bad = torch.tensor([float('nan'), 1.0, -1.0, float('inf'), -float('inf'), 0.0, float('nan'), 2.0], dtype=dtype, device='cuda')
    out = act_fwd(bad, 'relu')
    assert torch.isnan(out[0]) and torch.isnan(out[6]) and torch.equal(out[1:6], torch.relu(bad)[1:6]) and out[3] == float('inf')


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('kind', KINDS)
def test_hard_input_sweep(kind, dtype):
    """every finite 16-bit pattern (fp32: the wider sweep) x CYCLE, forward and backward, per-element bars"""
    x = ah.activation_sweep(dtype)
    dy = ah.cycle(x.shape, dtype=dtype)
    xc, dc = x.cuda(), dy.cuda()
    check_case('sweep', x, dy, kind, act_fwd(xc, kind).cpu(), act_bwd(xc, dc, kind).cpu(), dtype)


# ---------------------------------------------------------------------------------------------------------------
# TGT_EPI_ACT / TGT_EPI_ACT_BWD
# ---------------------------------------------------------------------------------------------------------------
GUARD = 3
TOL = parity_log.Tol({torch.bfloat16: 4e-3, torch.float16: 5e-4})          # the table of tests/test_hip_edge_gemm.py


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return parity_log.record(float((a - b).norm() / (b.norm() + 1e-30)))


@pytest.fixture
def grid_cap(request):
    _lib.lib().tgt_edge_linear_set_grid_cap(request.param)
    yield request.param
    _lib.lib().tgt_edge_linear_set_grid_cap(0)


def _mk(M, K, dtype, seed, bias=True):
    g = torch.Generator(device='cuda').manual_seed(seed)
    a = torch.randn(M, K, device='cuda', generator=g).to(dtype)
    w = (torch.randn(256, K, device='cuda', generator=g) / math.sqrt(K)).to(dtype)
    b = (torch.randn(256, device='cuda', generator=g) * 0.5).to(dtype) if bias else None
    return a, w, b, g


def _flags(kind):
    return _lib.ACT_KINDS[kind] << _lib.EDGE_ACT_KIND_SHIFT


@pytest.mark.parametrize('grid_cap', [0, 1, 3], indirect=True)
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('K', [64, 128, 256])
@pytest.mark.parametrize('M', [33, 520, 1000])
def test_act_epilogue(M, K, dtype, grid_cap):
    """out2 bit-equal to the TGT_EPI_BIAS launch, out bit-equal to tgt_act_dropout_fwd on it, nothing written at or past row M or
    beside the 256 columns; grid caps 1 and 3: one workgroup walks several tiles and a tail tile"""
    a, w, bias, g = _mk(M, K, dtype, M + K)
    rps = 8
    sc_all = torch.tensor([0.0, 1.0, 1.25], device='cuda')[torch.randint(0, 3, (M // rps,), device='cuda', generator=g)].contiguous()
    case = 0
    for b in (bias, None):
        plain = ops.edge_linear_raw(a, w, b)                              # TGT_EPI_BIAS on the same operands
        assert rel(plain, a.double() @ w.double().t() + (0 if b is None else b.double())) < TOL[dtype]
        for scale in ((sc_all, None) if M % rps == 0 else (None,)):
            for p in (0.0, 0.1):
                kind, case = KINDS[case % 3], case + 1
                seed = 0x77aa55 + case if p else 0
                wide = case % 2 == 0                                      # out2 with padded rows (ldo2 = 320)
                buf2 = torch.full((M + GUARD, 320 if wide else 256), 7.0, dtype=dtype, device='cuda')
                buf = torch.full((M + GUARD, 256), 7.0, dtype=dtype, device='cuda')
                out2, out = buf2[:M, :256], buf[:M]
                ops.edge_linear_raw(a, w, b, _lib.EPI_ACT, out=out, out2=out2, dropout=(p, seed), row_scale=scale,
                                    rows_per_sample=rps if scale is not None else 0, flags=_flags(kind))
                assert torch.equal(out2, plain), (kind, p, case)
                y = act_fwd(out2.contiguous(), kind, p, seed, scale, rps * 256 if scale is not None else 0)
                assert torch.equal(out, y), (kind, p, case)
                assert torch.all(buf2[M:] == 7.0) and torch.all(buf2[:, 256:] == 7.0) and torch.all(buf[M:] == 7.0)


def _colsum_close(got, want):
    """the bar of tests/test_hip_edge_gemm.py::_colsum_close: max |got - want| <= 1e-5 max |want| + 1e-6"""
    top = float(want.abs().max())
    err = parity_log.record(float((got - want).abs().max()) / (top + 1e-30))
    return err * top <= 1e-5 * top + 1e-6, err


@pytest.mark.parametrize('grid_cap', [0, 1, 3], indirect=True)
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('K', [64, 128, 256])
@pytest.mark.parametrize('M', [33, 520, 1000])
def test_act_backward_epilogue(M, K, dtype, grid_cap):
    """TGT_EPI_ACT_BWD held as tests/test_hip_edge_gemm.py holds TGT_EPI_GELU_BWD (_gelu_bwd_check): against float64 of the GEMM result
    rounded to the storage type [and again after the per-graph factor] times act'(pre) keep / (1 - p) at TOL; the column sums are
    those of the result as stored; against the streaming backward on the rounded gradient; guard rows intact"""
    L = _lib.lib()
    a, w, _, g = _mk(M, K, dtype, 43 + M + K, bias=False)
    pre = (torch.randn(M, 256, device='cuda', generator=g) * 2).to(dtype)
    rps = 40
    for case, kind in enumerate(KINDS):
        p = (0.0, 0.1, 0.1)[(case + (M % 3)) % 3]
        with_scale = (case + M) % 2 == 0
        sc = (torch.rand(-(-M // rps), device='cuda', generator=g) + 0.5) if with_scale else None
        seed = 0x9e1b5eed + case if p else 0
        buf = torch.full((M + GUARD, 256), 7.0, dtype=dtype, device='cuda')
        out = buf[:M]
        cs = torch.full((L.tgt_edge_linear_parts(M, 256) + 1, 256), 7.0, device='cuda')
        ops.edge_linear_raw(a, w, None, _lib.EPI_ACT_BWD, out=out, res=pre, out_scale=sc, rows_per_sample=rps if with_scale else 0,
                            dropout=(p, seed), colsum_partial=cs[:-1], flags=_flags(kind))
        assert torch.all(buf[M:] == 7.0) and torch.all(cs[-1] == 7.0)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(cs).all())
        keep = torch.from_numpy(ah.keep_pattern_np(M * 256, 2, p, seed)).view(M, 256).cuda() if p else None
        dy = (a.double() @ w.double().t()).to(dtype).double()           # the GEMM result is rounded to the 16-bit type first,
        if with_scale:
            dy = (dy * sc.double().repeat_interleave(rps)[:M, None]).to(dtype).double()      # and again after the per-graph factor
        x = pre.double().requires_grad_(True)
        ah.FN[kind](x).backward(dy)
        ref = x.grad / (1 - p)
        if keep is not None:
            ref = ref * keep
        assert rel(out, ref) < TOL[dtype], (kind, rel(out, ref))
        # the streaming backward on the gradient as rounded here (from float64; the kernel rounds from fp32: last-bit flips)
        dx = act_bwd(pre, dy.to(dtype), kind, p, seed)
        assert rel(out, dx) < TOL[dtype]
        assert float(((out == 0) != (dx == 0)).float().mean()) < 1e-3
        ok, err = _colsum_close(cs[:-1].double().sum(0), out.double().sum(0))
        assert ok, ('colsum', kind, err)
        # without the column sums: the same result
        assert torch.equal(out, ops.edge_linear_raw(a, w, None, _lib.EPI_ACT_BWD, res=pre, out_scale=sc, rows_per_sample=rps if with_scale else 0,
                                                    dropout=(p, seed), flags=_flags(kind)))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('kind', KINDS)
def test_act_epilogues_on_live_tiles(kind, dtype):
    """tgt_edge_linear_live: dead tiles get zeros in every output, live tiles are bit-equal to the plain launch"""
    B, N, K = 5, 12, 128
    counts = torch.tensor([12, 3, 0, 7, 12], dtype=torch.int32, device='cuda')
    M = B * N * N
    live = ops.edge_live_tiles(counts, N)
    tiles = live.tiles.cpu()
    n_live, n_tiles = int(tiles[0]), (M + 31) // 32
    assert 0 < n_live < n_tiles
    alive = torch.zeros(n_tiles * 32, dtype=torch.bool)
    for t in tiles[1:1 + n_live].tolist():
        alive[32 * t:32 * t + 32] = True
    alive = alive[:M].cuda()
    a, w, b, g = _mk(M, K, dtype, 5)
    pre = torch.randn(M, 256, device='cuda', generator=g).to(dtype)
    sc = torch.rand(B, device='cuda', generator=g) + 0.5
    kw = dict(rows_per_sample=N * N, dropout=(0.1, 0x1234), flags=_flags(kind))
    for cap in (0, 2):
        _lib.lib().tgt_edge_linear_set_grid_cap(cap)
        try:
            o2p, o2l = torch.empty(M, 256, dtype=dtype, device='cuda'), torch.full((M, 256), 7.0, dtype=dtype, device='cuda')
            op = ops.edge_linear_raw(a, w, b, _lib.EPI_ACT, out2=o2p, row_scale=sc, **kw)
            ol = ops.edge_linear_raw(a, w, b, _lib.EPI_ACT, out=torch.full((M, 256), 7.0, dtype=dtype, device='cuda'), out2=o2l,
                                     row_scale=sc, live=live, **kw)
            assert torch.equal(ol[alive], op[alive]) and torch.equal(o2l[alive], o2p[alive])
            assert torch.all(ol[~alive] == 0) and torch.all(o2l[~alive] == 0)
            parts = _lib.lib().tgt_edge_linear_parts(M, 256)
            csp, csl = torch.empty(parts, 256, device='cuda'), torch.empty(parts, 256, device='cuda')
            bp = ops.edge_linear_raw(a, w, None, _lib.EPI_ACT_BWD, res=pre, out_scale=sc, colsum_partial=csp, **kw)
            bl = ops.edge_linear_raw(a, w, None, _lib.EPI_ACT_BWD, out=torch.full((M, 256), 7.0, dtype=dtype, device='cuda'), res=pre,
                                     out_scale=sc, colsum_partial=csl, live=live, **kw)
            assert torch.equal(bl[alive], bp[alive]) and torch.all(bl[~alive] == 0)
            ok, err = _colsum_close(csl.double().sum(0), bl.double().sum(0))
            assert ok, ('colsum', err)
        finally:
            _lib.lib().tgt_edge_linear_set_grid_cap(0)


def test_act_epilogue_refusals_on_the_device():
    a = torch.zeros(64, 256, dtype=torch.bfloat16, device='cuda')
    w = torch.zeros(256, 256, dtype=torch.bfloat16, device='cuda')
    with pytest.raises(RuntimeError, match='epilogue operand missing'):
        ops.edge_linear_raw(a, w, None, _lib.EPI_ACT)
    with pytest.raises(RuntimeError, match='epilogue operand missing'):
        ops.edge_linear_raw(a, w, None, _lib.EPI_ACT_BWD)
    with pytest.raises(RuntimeError, match='take no bias'):
        ops.edge_linear_raw(a, w, torch.zeros(256, dtype=torch.bfloat16, device='cuda'), _lib.EPI_ACT_BWD, res=a)
    with pytest.raises(RuntimeError, match=r'code 2\).*unsupported'):
        ops.edge_linear_raw(a, w, None, _lib.EPI_ACT_BWD, res=a, dw_partial=torch.empty(2, 256, 256, device='cuda'))
    with pytest.raises(RuntimeError, match=r'code 2\).*unsupported'):
        ops.edge_linear_raw(a, w, None, _lib.EPI_ACT, out2=torch.empty_like(a), flags=3 << _lib.EDGE_ACT_KIND_SHIFT)


# ---------------------------------------------------------------------------------------------------------------
# ops
# ---------------------------------------------------------------------------------------------------------------
def test_ops_act_dropout_draws_a_seed_and_saves_only_x():
    x, dy = _inputs(64, 256, torch.bfloat16, 13)
    x = torch.where(x == 0, torch.ones_like(x), x)
    scale = torch.tensor([2.0, 0.0], device='cuda')
    torch.manual_seed(5)
    xn = x.view(2, 32, 256).clone().requires_grad_(True)
    y = ops.act_dropout(xn, 'silu', 0.25, True, scale)
    assert [t.shape for t in y.grad_fn.saved_tensors if t is not None and t.dim() > 1] == [xn.shape]
    y.backward(dy.view(2, 32, 256))
    assert torch.all(y[1] == 0) and torch.all(xn.grad[1] == 0)
    kept = float((y[0] != 0).float().mean())
    assert abs(kept - 0.75) < 5 * math.sqrt(0.75 * 0.25 / y[0].numel())
    torch.manual_seed(5)
    assert torch.equal(y, ops.act_dropout(xn.detach(), 'silu', 0.25, True, scale))
    assert not torch.equal(y, ops.act_dropout(xn.detach(), 'silu', 0.25, True, scale))      # the next seed
    with pytest.raises(RuntimeError, match='unknown activation'):
        ops.act_dropout(xn, 'tanh', 0.0, False)
    with pytest.raises(RuntimeError, match='no kernel for dtype'):
        ops.act_dropout(xn.double(), 'relu', 0.0, False)


@pytest.mark.parametrize('fused', [False, True], ids=['streaming', 'epilogue'])
def test_graph_safe_mode_mixes_the_step_counter(fused, monkeypatch):
    """graph-safe mode: the seed of a call is its position in the step, so two steps differ only through the device counter the
    kernels mix in -- bumped in between: another pattern; the same counter value: the same result"""
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)
    g = torch.Generator(device='cuda').manual_seed(2)
    x = torch.randn(96, 256, device='cuda', generator=g).to(torch.bfloat16)
    w = (torch.randn(256, 256, device='cuda', generator=g) / 16).to(torch.bfloat16)
    ctr = torch.zeros(1, dtype=torch.int64, device='cuda')

    def step():
        ops.begin_step()
        if fused:
            assert ops.linear_act_dropout_ok(x, w)
            return ops.linear_act_dropout(x, w, None, 'elu', 0.25, True)
        return ops.act_dropout(x, 'elu', 0.25, True)

    try:
        ops.graph_safe_rng(True)
        ops.set_seed_counter(ctr)
        y0 = step()
        y0b = step()
        ops.bump_seed_counter()
        y1 = step()
        ctr.zero_()
        y0c = step()
    finally:
        ops.set_seed_counter(None)
        ops.graph_safe_rng(False)
    assert torch.equal(y0, y0b) and torch.equal(y0, y0c)
    assert not torch.equal(y0 != 0, y1 != 0)
    # the pattern of counter value 1 is that of the mixed seed
    if not fused:
        ops.graph_safe_rng(True)
        ops.begin_step()
        seed = ops._host_seed()
        ops.graph_safe_rng(False)
        keep = torch.from_numpy(ah.keep_pattern_np(x.numel(), 2, 0.25, seed, counter=1)).view_as(x).cuda()
        assert torch.equal(y1 != 0, keep & (act_fwd(x, 'elu') != 0))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('kind', KINDS)
def test_linear_act_dropout_takes_over_the_backward(kind, dtype, monkeypatch):
    """linear_act_dropout returns the activation with the record linear_residual_layer_norm needs; the closing Linear then runs the
    activation's backward as TGT_EPI_ACT_BWD, and the block equals the unfused chain (knob off) within one storage rounding"""
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)
    B, N = 3, 10
    g = torch.Generator(device='cuda').manual_seed(7)
    x0 = torch.randn(B, N, N, 256, device='cuda', generator=g).to(dtype)
    res0 = torch.randn(B, N, N, 256, device='cuda', generator=g).to(dtype)
    w1, w2 = ((torch.randn(256, 256, device='cuda', generator=g) / 16).requires_grad_(True) for _ in range(2))
    b1, b2 = ((torch.randn(256, device='cuda', generator=g) * 0.1).requires_grad_(True) for _ in range(2))
    lw, lb = torch.ones(256, device='cuda', requires_grad=True), torch.zeros(256, device='cuda', requires_grad=True)
    sc = torch.tensor([2.0, 0.0, 2.0], device='cuda')
    gs, gy = torch.randn(B, N, N, 256, device='cuda', generator=g).to(dtype), torch.randn(B, N, N, 256, device='cuda', generator=g).to(dtype)
    runs = []
    for knob in (True, False):
        monkeypatch.setattr(ops, '_FFN_ACT_EPI', knob)
        for t in (w1, w2, b1, b2, lw, lb):
            t.grad = None
        x, res = x0.clone().requires_grad_(True), res0.clone().requires_grad_(True)
        torch.manual_seed(11)
        prof = ops.profile_kernels(True)
        try:
            with torch.autocast('cuda', dtype=dtype):
                if knob:
                    assert ops.linear_act_dropout_ok(x, w1)
                    act = ops.linear_act_dropout(x, w1, b1, kind, 0.1, True)
                    assert act._tgt_gelu[4] == _lib.ACT_KINDS[kind] and act._tgt_gelu[0].shape == act.shape
                else:
                    assert not ops.linear_act_dropout_ok(x, w1)
                    act = ops.act_dropout(ops.linear(x, w1, b1), kind, 0.1, True)
                s, y = ops.linear_residual_layer_norm(act, w2, b2, res, sc, lw, lb)
            ((s.float() * gs).sum() + (y.float() * gy).sum()).backward()
            torch.cuda.synchronize()
        finally:
            ops.profile_kernels(False)
        if knob:
            assert 'tgt_act_dropout_fwd' not in prof and 'tgt_act_dropout_bwd' not in prof, sorted(prof)
        else:
            assert len(prof['tgt_act_dropout_fwd']) == 1 and len(prof['tgt_act_dropout_bwd']) == 1, sorted(prof)
        runs.append([s.detach(), y.detach(), x.grad, res.grad] + [t.grad for t in (w1, w2, b1, b2, lw, lb)])
    TOL[dtype]
    for i, (u, v) in enumerate(zip(*runs)):
        assert rel(u, v) < 2 * TOL[dtype], (i, rel(u, v))


# ---------------------------------------------------------------------------------------------------------------
# FFN and TGT_Encoder
# ---------------------------------------------------------------------------------------------------------------
def bar(name, new, eager, ref, e_max):
    """tests/test_hip_glu.py::bar: err_new <= 2 err_eager + 1.5e-7 e_max; files the ratio under `act`"""
    ref = ref.detach().double()
    err_new = float((new.detach().double() - ref).abs().max())
    err_eager = float((eager.detach().double() - ref).abs().max())
    bound = 2.0 * err_eager + 1.5e-7 * float(e_max)
    parity_log.Tol.last = 'act'
    parity_log.record(err_new / bound)
    print(f'{name}: err_new {err_new:.3e} err_eager {err_eager:.3e} bound {bound:.3e} ratio {err_new / bound:.3f}')
    assert err_new <= bound, (name, err_new, err_eager, bound)


def _ffn_run(ffn, x, dy, dtype):
    x = x.clone().requires_grad_(True)
    for p in ffn.parameters():
        p.grad = None
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
    in float32 under the same autocast.  Knob on: edge rows take the fused launch, node rows the library GEMM + streaming pair; knob
    off: the streaming pair everywhere; both inside the same bars."""
    from tgt_amd.tgt.layers.blocks import FFN
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)
    width = shape[-1]
    g = torch.Generator(device='cuda').manual_seed(21)
    x = torch.randn(*shape, device='cuda', generator=g)
    dy = torch.randn(*shape, device='cuda', generator=g)
    new = gu.fill_params(FFN(width, 1., act_dropout=0., activation=activation), seed=4).cuda().train()
    eager = gu.fill_params(om.FFN(width, 1., 0., activation), seed=4).cuda().train()
    ref = gu.fill_params(om.FFN(width, 1., 0., activation), seed=4).cuda().double().train()
    ye, dxe, ge = _ffn_run(eager, x, dy, dtype)
    y6, dx6, g6 = _ffn_run(ref, x.double(), dy.double(), None)
    with torch.no_grad():
        e_max = ref.lin_W1(ref.ffn_ln(x.double())).abs().max()
    for knob in (True, False):
        monkeypatch.setattr(ops, '_FFN_ACT_EPI', knob)
        prof = ops.profile_kernels(True)
        try:
            yn, dxn, gn = _ffn_run(new, x, dy, dtype)
        finally:
            ops.profile_kernels(False)
        if width == 256 and knob:
            assert 'tgt_edge_linear' in prof and len(prof['tgt_act_dropout_bwd']) == 1 and 'tgt_act_dropout_fwd' not in prof, sorted(prof)
        else:
            assert len(prof['tgt_act_dropout_fwd']) == 1 and len(prof['tgt_act_dropout_bwd']) == 1, sorted(prof)
        bar(f'knob {knob} y', yn, ye, y6, e_max)
        bar(f'knob {knob} dx', dxn, dxe, dx6, e_max)
        assert sorted(gn) == sorted(g6)
        for k in sorted(g6):
            bar(f'knob {knob} {k}', gn[k], ge[k], g6[k], e_max)


class _FixedScales:
    """stands in for the DropPath factor pool: the same factors for every branch (keep probability 0.5, one graph dropped)"""
    factors = [2.0, 0.0, 2.0, 2.0]

    @classmethod
    def take(cls, B, keep, device):
        assert B == 4 and keep == 0.5
        return torch.tensor(cls.factors, device=device)


def test_two_layer_silu_encoder_trains_one_step_against_the_oracle(monkeypatch):
    """Two TGT layers with activation='silu' and DropPath (0 in the first layer, 0.5 in the second: the encoder's ramp) in train mode
    under bf16 autocast, one forward + backward: outputs, input gradients and every parameter gradient against oracle.modules.
    TGT_Encoder in float64 on the same DropPath factors.  Bar, per tensor: ||new - ref|| <= 2 ||eager - ref|| + 1e-6 ||ref||, eager = the
    oracle in float32 under the same autocast (another rounding order, as in bar())."""
    from tgt_amd.tgt import Graph, TGT_Encoder
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)
    monkeypatch.setattr(ops, '_scale_pool', _FixedScales)

    def oracle_drop_path(self, x):
        if self.drop_path > 0 and self.training:
            assert self.drop_path == 0.5
            return x * torch.tensor(_FixedScales.factors, device=x.device, dtype=x.dtype).view([-1] + [1] * (x.ndim - 1))
        return x
    monkeypatch.setattr(om.DropPath, 'forward', oracle_drop_path)
    B, N, W, C = 4, 9, 768, 256
    kw = dict(node_width=W, edge_width=C, num_heads=64, activation='silu', scale_degree=True, node_update=True, edge_update=True,
              triplet_heads=0, node_ffn_multiplier=1., edge_ffn_multiplier=1., source_dropout=0., drop_path=0.5,
              node_act_dropout=0., edge_act_dropout=0.)
    g = torch.Generator(device='cuda').manual_seed(3)
    h0 = torch.randn(B, N, W, device='cuda', generator=g)
    e0 = torch.randn(B, N, N, C, device='cuda', generator=g)
    mask = gu.additive_mask([9, 5, 9, 7], N, torch.float32).cuda()
    gh, ge = torch.randn(B, N, W, device='cuda', generator=g), torch.randn(B, N, N, C, device='cuda', generator=g)

    def run(model, dt, autocast):
        h, e = h0.to(dt).clone().requires_grad_(True), e0.to(dt).clone().requires_grad_(True)
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
            out = model(Graph(h=h, e=e, mask=mask.to(dt)))
        ((out.h.to(dt) * gh.to(dt)).sum() + (out.e.to(dt) * ge.to(dt)).sum()).backward()
        res = {'h': out.h.detach(), 'e': out.e.detach(), 'dh': h.grad, 'de': e.grad}
        res.update({k: p.grad for k, p in model.named_parameters()})
        return res

    new_model = gu.fill_params(TGT_Encoder(model_height=2, **kw), seed=9).cuda().train()
    assert [layer.drop_path.drop_path for layer in new_model.TGT_layers] == [0.0, 0.5]
    prof = ops.profile_kernels(True)
    try:
        new = run(new_model, torch.float32, True)
        torch.cuda.synchronize()
    finally:
        ops.profile_kernels(False)
    # the node FFNs run the streaming pair; the edge FFNs the fused launch: the first layer's activation backward runs inside lin_W2's
    # data-gradient launch (the next layer's entry owns that Linear), the last layer's closing Linear is a plain one
    assert len(prof['tgt_act_dropout_fwd']) == 2 and len(prof['tgt_act_dropout_bwd']) == 3 and 'tgt_edge_linear' in prof, sorted(prof)
    eager = run(gu.fill_params(om.TGT_Encoder(model_height=2, **kw), seed=9).cuda().train(), torch.float32, True)
    ref = run(gu.fill_params(om.TGT_Encoder(model_height=2, **kw), seed=9).cuda().double().train(), torch.float64, False)
    assert sorted(new) == sorted(ref)
    parity_log.Tol.last = 'act'
    for k in sorted(ref):
        assert (new[k] is None) == (ref[k] is None), k
        if ref[k] is None:
            continue
        r = ref[k].double()
        err_new, err_eager = float((new[k].double() - r).norm()), float((eager[k].double() - r).norm())
        bound = 2 * err_eager + 1e-6 * float(r.norm())
        parity_log.record(err_new / max(bound, 1e-300))
        print(f'{k}: err_new {err_new:.3e} err_eager {err_eager:.3e} |ref| {float(r.norm()):.3e}')
        assert torch.isfinite(new[k]).all() and err_new <= bound, (k, err_new, err_eager)
    # the dropped graph: the second layer adds nothing to it, so its gradient reaches the input through the first layer only
    assert float(new['de'][1].abs().max()) > 0
