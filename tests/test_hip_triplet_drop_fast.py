"""Attention dropout inside the round-4 triplet backward (tri_att_bwd2_kernel's DROP instantiations: 16-bit, D = 16, N <= 32,
H % 8 == 0), which a call with dropout_p > 0 now stays on (tgt_triplet_attention_family; TGT_TRI_DROP_FAST=0: the general
tri_att_bwd_kernel, as before).

Bars: the float64 oracle with the SAME keep pattern (golden_util.triplet_dropout_keep), the forward at TOL[dtype] and the gradients at
2 * TOL[dtype] of tests/test_hip_ops.py -- the bars the general kernels are held to with dropout on; a wrong pattern misses them by
orders of magnitude (half of the weights differ).  Everything else here is bitwise.

The forward of these calls is library GEMM + tri_att_fwd_kernel: the projection-fused forward keeps refusing dropout_p > 0
(profiles/tri_drop_fast_isa.txt), so nothing here is about it.

Shapes: N = 32 (full tile, a ragged graph inside), 20, and 11 (odd, zero-filled slab rows: the LDS-DMA loads write nothing past N);
C = 256 / H = 16 (two head groups per graph and direction) and C = 128 / H = 8 (one)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import golden_util as gu
from oracle import core
from test_hip_ops import TOL
from test_hip_triplet_dropout_counter import _check

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
SHAPES = [(3, 32, (32, 17, 32)), (2, 20, (20, 13)), (2, 11, (11, 7))]
WIDTHS = [(256, 16), (128, 8)]
VARIANTS = ['gated', 'ungated', 'axial']
SEED = 0x1234567890ABCDEF


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _rnd(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape))


def _layout(width, variant):
    from tgt_amd import ops
    return ops.TripletLayout(width[0], width[1], gated=variant == 'gated', biased=variant != 'axial')


@pytest.fixture(autouse=True)
def _every_size_takes_the_big_batch_paths(monkeypatch):
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 0)
    monkeypatch.delenv('TGT_TRI_DROP_FAST', raising=False)


def _keep_dirs(B, N, H, p, seed):
    units = (((np.arange(B)[:, None, None, None] * 2 + np.arange(2)[None, :, None, None]) * H +
              np.arange(H)[None, None, :, None]) * N + np.arange(N)[None, None, None, :]).reshape(-1)
    keep, scale = gu.triplet_dropout_keep(seed, p, units, N)
    keep = torch.from_numpy(keep.reshape(B, 2, H, N, N, N))            # (b, dir, h, j, i, k)
    assert abs(float(keep.float().mean()) - (1 - p)) < 0.02
    return [keep[:, d].permute(0, 3, 2, 4, 1).contiguous() for d in (0, 1)], scale      # (b, i, j, k, h)


def _oracle_va(f64, mask, L, C_, H, p, seed):
    """Va in the kernels' channel order from a float64 fused row (kernel order), with the kernels' keep pattern"""
    from tgt_amd import layout
    B, N = f64.shape[0], f64.shape[1]
    idx, oidx = layout.head_major_index(C_, H), layout.va_cols_head_major(C_, H)

    def to_ref(x_hm):
        out = torch.empty_like(x_hm)
        out[..., idx] = x_hm
        return out
    blk = lambda lo: torch.cat([to_ref(f64[..., lo + q * C_: lo + (q + 1) * C_]) for q in range(3)], -1)
    nb = (2 if L.gated else 1) * H
    eg_in = f64[..., 6 * C_: 6 * C_ + nb] if L.biased else None
    eg_out = f64[..., 6 * C_ + nb: 6 * C_ + 2 * nb] if L.biased else None
    keep, scale = _keep_dirs(B, N, H, p, seed)
    va = core.triplet_attention_core(blk(0), eg_in, blk(3 * C_), eg_out, mask.double(), H, L.gated, L.biased,
                                     dropout=(keep[0], keep[1], scale))
    return va[..., oidx]


@functools.lru_cache(maxsize=None)
def _plain_case(shape, width, variant, dtype, p):
    """inputs of ops.triplet_attention and the oracle's (out, d_fused) for them; computed once, never modified"""
    B, N, nodes = shape
    C_, H = width
    L = _layout(width, variant)
    rng = np.random.default_rng(100 * N + H)
    fused, d_out = _rnd(rng, B, N, N, L.width).to(dtype), _rnd(rng, B, N, N, 2 * C_).to(dtype)
    mask = gu.additive_mask(list(nodes), N, torch.float32)
    f64 = fused.double().requires_grad_(True)
    va = _oracle_va(f64, mask, L, C_, H, p, SEED)
    (va * d_out.double()).sum().backward()
    return fused.cuda(), d_out.cuda(), mask.reshape(B, N, N).cuda(), va.detach(), f64.grad


@functools.lru_cache(maxsize=None)
def _proj_case(shape, variant, dtype, p):
    """inputs of ops.projected_triplet_attention (C = 256, H = 16) and the oracle's (out, dx, dw, db)"""
    B, N, nodes = shape
    C_, H = WIDTHS[0]
    L = _layout(WIDTHS[0], variant)
    assert L.width == L.used
    rng = np.random.default_rng(7 * N + 1)
    x = _rnd(rng, B, N, N, C_).to(dtype)
    w = (_rnd(rng, L.width, C_) * C_ ** -0.5).to(dtype)
    b = (_rnd(rng, L.width) * 0.1).to(dtype)
    d_out = _rnd(rng, B, N, N, 2 * C_).to(dtype)
    mask = gu.additive_mask(list(nodes), N, torch.float32)
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    f64 = torch.nn.functional.linear(x64, w64, b64)        # (lin(x) -> the core, as test_projection_fused_triplet_attention_vs_oracle)
    va = _oracle_va(f64, mask, L, C_, H, p, SEED)
    (va * d_out.double()).sum().backward()
    return x.cuda(), w.cuda(), b.cuda(), d_out.cuda(), mask.reshape(B, N, N).cuda(), va.detach(), x64.grad, w64.grad, b64.grad


def _run_plain(case, L, p, seed=SEED, graph_scale=None, node_counts=None):
    from tgt_amd import ops
    fused, d_out, mask3 = case[:3]
    fx = fused.clone().requires_grad_(True)
    out = ops.triplet_attention(fx, mask3, L, dropout=(p, seed), graph_scale=graph_scale, node_counts=node_counts)
    out.backward(d_out)
    return out.detach(), fx.grad[..., :L.used]


def _run_proj(case, L, p, seed=SEED, node_counts=None):
    from tgt_amd import ops
    x, w, b, d_out, mask3 = case[:5]
    xs, ws, bs = (t.clone().requires_grad_(True) for t in (x, w, b))
    out = ops.projected_triplet_attention(xs, ws, bs, mask3, L, dropout=(p, seed), node_counts=node_counts)
    out.backward(d_out)
    return out.detach(), xs.grad, ws.grad, bs.grad


def _bwd_family(L, shape, dtype, p, colsum):
    """tgt_triplet_attention_family for the backward argument block ops builds for this call"""
    from tgt_amd import ops, _lib
    B, N, _ = shape
    fused = torch.empty(B, N, N, L.width, dtype=dtype, device='cuda')
    out = torch.empty(B, N, N, 2 * L.C, dtype=dtype, device='cuda')
    mask3 = torch.zeros(B, N, N, device='cuda')
    cs = ops._colsum_workspace(B, L.width, L.used, fused.device) if colsum else None
    a = ops._tri_args(fused, mask3, out, L, out, torch.empty_like(fused), cs, dropout=(p, SEED))
    return _lib.lib().tgt_triplet_attention_family(C.byref(a), 1)


# ---- 1. parity with the float64 oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [BF16, F16])
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('width', WIDTHS)
@pytest.mark.parametrize('shape', SHAPES)
def test_backward_without_column_sums_matches_the_oracle(shape, width, variant, dtype):
    L = _layout(width, variant)
    case = _plain_case(shape, width, variant, dtype, 0.3)
    out, dx = _run_plain(case, L, 0.3)
    e_out, e_dx = _rel(out, case[3]), _rel(dx, case[4][..., :L.used])
    print(f'fwd {e_out:.3e} d_fused {e_dx:.3e} (bars {TOL[dtype]:.1e} / {2 * TOL[dtype]:.1e})')
    assert e_out < TOL[dtype], ('fwd', e_out)
    assert e_dx < 2 * TOL[dtype], ('d_fused', e_dx)


@pytest.mark.parametrize('dtype', [BF16, F16])
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('shape,p', [(s, 0.3) for s in SHAPES] + [(SHAPES[1], 0.05)])
def test_backward_with_column_sums_matches_the_oracle(shape, p, variant, dtype):
    L = _layout(WIDTHS[0], variant)
    case = _proj_case(shape, variant, dtype, p)
    got = _run_proj(case, L, p)
    errs = [_rel(g, e) for g, e in zip(got, case[5:])]
    print('fwd %.3e dx %.3e dw %.3e db %.3e' % tuple(errs), f'(bars {TOL[dtype]:.1e} / {2 * TOL[dtype]:.1e})')
    assert errs[0] < TOL[dtype], ('fwd', errs[0])
    for name, e in zip(('dx', 'dw', 'db'), errs[1:]):
        assert e < 2 * TOL[dtype], (name, e)


# ---- 2. the round-4 kernel is what ran -------------------------------------------------------------------------------------
@pytest.mark.parametrize('width', WIDTHS)
@pytest.mark.parametrize('colsum', [False, True])
def test_the_dropout_backward_takes_the_round4_kernel(width, colsum):
    """(fails on the parent commit: no such symbol, and its library routes p > 0 to tri_att_bwd_kernel)"""
    from tgt_amd import _lib
    for shape in SHAPES:
        for variant in VARIANTS:
            L = _layout(width, variant)
            assert _bwd_family(L, shape, BF16, 0.3, colsum) == _lib.TRI_FAMILY_BWD2
            assert _bwd_family(L, shape, F16, 0.0, colsum) == _lib.TRI_FAMILY_BWD2
    assert _bwd_family(_layout((64, 4), 'gated'), SHAPES[1], BF16, 0.3, colsum) == _lib.TRI_FAMILY_GENERAL


def test_the_backward_launch_is_the_library_entry_that_routes():
    from tgt_amd import ops
    L = _layout(WIDTHS[0], 'gated')
    case = _proj_case(SHAPES[1], 'gated', BF16, 0.3)
    prof = ops.profile_kernels(True)
    try:
        _run_proj(case, L, 0.3)
        torch.cuda.synchronize()
    finally:
        ops.profile_kernels(False)
    assert len(prof.get('tgt_triplet_attention_bwd', ())) == 1 and len(prof.get('tgt_triplet_attention_fwd', ())) == 1


# ---- 3. bitwise contracts dropout must not break ------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [BF16, F16])
@pytest.mark.parametrize('variant', VARIANTS)
def test_two_backward_runs_are_bit_identical(variant, dtype):
    L = _layout(WIDTHS[0], variant)
    case = _proj_case(SHAPES[0], variant, dtype, 0.3)
    a, b = _run_proj(case, L, 0.3), _run_proj(case, L, 0.3)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    L8 = _layout(WIDTHS[1], variant)
    case8 = _plain_case(SHAPES[2], WIDTHS[1], variant, dtype, 0.3)
    a, b = _run_plain(case8, L8, 0.3), _run_plain(case8, L8, 0.3)
    assert all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize('width', WIDTHS)
@pytest.mark.parametrize('shape', SHAPES)
def test_node_counts_change_nothing_below_the_count(shape, width):
    """with counts the units j >= n are not computed (zeros out, their d_out not read); everything with j < n -- the dropout units keep
    the tensor's N -- is the call without counts, bit for bit: out, and d_fused where the incoming gradient of the padded columns is
    zero (the counts' contract)"""
    B, N, nodes = shape
    L = _layout(width, 'gated')
    fused, d_out, mask3 = _plain_case(shape, width, 'gated', BF16, 0.3)[:3]
    counts = torch.tensor(nodes, dtype=torch.int32, device='cuda')
    d_out = d_out.clone()
    for b_, n in enumerate(nodes):
        d_out[b_, :, n:] = 0
    case = (fused, d_out, mask3)
    out0, dx0 = _run_plain(case, L, 0.3)
    out1, dx1 = _run_plain(case, L, 0.3, node_counts=counts)
    for b_, n in enumerate(nodes):
        assert torch.equal(out1[b_, :, :n], out0[b_, :, :n])
        assert not out1[b_, :, n:].any()
    # Q rows (i, j) and the third arm are per unit j; the partner rows K / V (j, k) / (k, j) of padded units are zeros with counts
    # and products with a zero d_out without: equal up to the sign of zero, so compare values
    assert torch.equal(dx1.float() + 0.0, dx0.float() + 0.0)


def test_dropped_graphs_are_zeros_and_kept_graphs_unchanged(monkeypatch):
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_TRI_SKIP_BWD', True)
    shape = SHAPES[0]
    L = _layout(WIDTHS[0], 'gated')
    fused, d_out, mask3 = _plain_case(shape, WIDTHS[0], 'gated', BF16, 0.3)[:3]
    gs = torch.tensor([2.0, 0.0, 2.0], device='cuda')
    d_out = d_out.clone()
    d_out[1] = 0                                            # (behind the multiplication by the factor)
    case = (fused, d_out, mask3)
    out0, dx0 = _run_plain(case, L, 0.3)
    out1, dx1 = _run_plain(case, L, 0.3, graph_scale=gs)
    for b_ in (0, 2):
        assert torch.equal(out1[b_], out0[b_]) and torch.equal(dx1[b_], dx0[b_])
    assert not out1[1].any() and not dx1[1].any()


# ---- 4. the step counter ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant,dtype', [('gated', BF16), ('ungated', BF16), ('axial', BF16), ('gated', F16)])
def test_round4_backward_follows_the_step_counter(variant, dtype):
    """the four checks of tests/test_hip_triplet_dropout_counter.py (counter at c == seed + c * golden without one; c = 0 == the plain
    call; successive counters differ; p = 0 never reads it), on calls whose backward is tri_att_bwd2: with and without column sums"""
    L = _layout(WIDTHS[0], variant)
    case = _proj_case(SHAPES[1], variant, dtype, 0.3)
    _check(lambda p, seed: _run_proj(case, L, p, seed))
    L8 = _layout(WIDTHS[1], variant)
    case8 = _plain_case(SHAPES[2], WIDTHS[1], variant, dtype, 0.3)
    _check(lambda p, seed: _run_plain(case8, L8, p, seed))


# ---- 5. against the general backward ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [BF16, F16])
@pytest.mark.parametrize('variant', VARIANTS)
def test_agrees_with_the_general_backward(variant, dtype, monkeypatch):
    from tgt_amd import ops, _lib
    L = _layout(WIDTHS[0], variant)
    case = _proj_case(SHAPES[0], variant, dtype, 0.3)
    fast = _run_proj(case, L, 0.3)
    monkeypatch.setattr(ops, '_TRI_DROP_FAST', False)
    monkeypatch.setenv('TGT_TRI_DROP_FAST', '0')           # the library asks per call
    assert _bwd_family(L, SHAPES[0], dtype, 0.3, True) == _lib.TRI_FAMILY_GENERAL
    slow = _run_proj(case, L, 0.3)
    monkeypatch.setenv('TGT_TRI_DROP_FAST', '1')
    assert torch.equal(fast[0], slow[0])                   # the forward is the same kernel
    errs = [_rel(f, s) for f, s in zip(fast[1:], slow[1:])]
    print('dx %.3e dw %.3e db %.3e' % tuple(errs))
    assert all(e < 2 * TOL[dtype] for e in errs), errs
    assert not all(torch.equal(f, s) for f, s in zip(fast[1:], slow[1:]))      # two kernels: the switch did switch


# ---- 6. module level ----------------------------------------------------------------------------------------------------------
def test_module_trains_with_attention_dropout_on_the_round4_backward():
    from tgt_amd import ops
    from tgt_amd.tgt.layers.triplet import TripletAttention
    B, N = 2, 20
    rng = np.random.default_rng(5)
    e = _rnd(rng, B, N, N, 256).to(BF16).cuda()
    mask = gu.additive_mask([20, 13], N, torch.float32).cuda()
    mod = gu.fill_params(TripletAttention(256, 16, attention_dropout=0.3), seed=3).to(BF16).cuda().train()
    ref = gu.fill_params(TripletAttention(256, 16, attention_dropout=0.0), seed=3).to(BF16).cuda().train()

    def step(m):
        torch.manual_seed(11)
        x = e.clone().requires_grad_(True)
        m.zero_grad(set_to_none=True)
        prof = ops.profile_kernels(True)
        try:
            y = m(x, mask)
            y.float().square().mean().backward()
            torch.cuda.synchronize()
        finally:
            ops.profile_kernels(False)
        return y.detach(), x.grad, prof

    y1, g1, prof = step(mod)
    y2, g2, _ = step(mod)
    assert len(prof['tgt_triplet_attention_bwd']) == 1
    assert torch.equal(y1, y2) and torch.equal(g1, g2)                 # same torch seed: same drawn seed, same pattern
    assert torch.isfinite(y1.float()).all() and torch.isfinite(g1.float()).all()
    assert all(p.grad is not None and torch.isfinite(p.grad.float()).all() for p in mod.parameters())
    y0, g0, _ = step(ref)
    assert not torch.equal(y1, y0)                                      # dropout is on
    # MC-dropout prediction (train mode under no_grad) draws a pattern too; .eval() is the p = 0 module bit for bit
    with torch.no_grad():
        torch.manual_seed(11)
        assert torch.equal(mod(e, mask), y1)
        assert torch.equal(mod.eval()(e, mask), ref.eval()(e, mask))
