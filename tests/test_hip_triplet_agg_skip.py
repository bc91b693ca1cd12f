"""The triplet aggregate kernels skip the graphs DropPath drops (tgt_triplet_aggregate_fwd_skip / _bwd_skip / _proj_fwd_skip;
ops.triplet_aggregate(..., graph_scale=), ops.projected_triplet_aggregate(..., graph_scale=), TripletAggregate.takes_graph_scale),
on the GPU.

The reference is always the same call WITHOUT graph_scale -- the call tests/test_hip_ops.py, test_hip_triplet_agg_kb.py and
test_hip_triplet_agg_proj.py hold to the float64 oracle -- so every comparison is bitwise (torch.equal): a kept graph is computed
exactly as without the pointer, a dropped graph is exact zeros, and there is no tolerance to choose."""
import functools

import numpy as np
import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
# (B, N, num_nodes, C, H): the smallest shapes that reach every instantiation of the kernels (HG x NT of csrc/triplet_aggregate.hip,
# the head groups / tile counts / KT forms of csrc/triplet_aggregate_kb.hip; fp32 takes HG 4 where the 16-bit types take HG 8, and
# KT 2 where they take KT 4)
SHAPES = {
    'hg8': (5, 32, (32, 17, 32, 9, 32), 256, 16),
    'hg4nt1': (5, 20, (20, 13, 20, 1, 7), 64, 4),
    'hg1': (4, 5, (5, 1, 5, 3), 48, 3),
    'nt2': (3, 40, (40, 33, 36), 64, 4),
    'hg1nt2': (2, 40, (40, 33), 48, 3),
    'kb3tiles': (3, 72, (72, 65, 70), 64, 4),
    'kbhg1': (2, 96, (96, 80), 48, 3),
    'kb4tiles': (2, 128, (128, 100), 64, 4),
}
DROPOUT = (0.25, 0x5DEECE66D1234567)


def rnd(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape))


def scale_of(B):
    """the DropPath factors of the tests: odd graphs dropped, the others at 1 / keep"""
    return torch.tensor([0.0 if b % 2 else 1.25 for b in range(B)], dtype=torch.float32, device='cuda')


@functools.lru_cache(maxsize=None)
def case(shape, dtype, gated, dropout):
    """inputs on the device and the run WITHOUT graph_scale (output, input gradient): computed once, never modified"""
    from tgt_amd import ops
    B, N, nn_, C, H = SHAPES[shape]
    L = ops.AggregateLayout(C, H, gated=gated)
    rng = np.random.default_rng(300 + 10 * list(SHAPES).index(shape) + DTYPES.index(dtype))
    sc = scale_of(B)
    live = (sc != 0).view(B, 1, 1, 1)
    fused = rnd(rng, B, N, N, L.width).to(dtype).cuda()
    d_out = rnd(rng, B, N, N, 2 * C).to(dtype).cuda() * live.to(dtype)          # what the dropped graphs receive: zeros
    mask3 = gu.additive_mask(list(nn_), N, torch.float32).reshape(B, N, N).cuda()
    fx = fused.clone().requires_grad_(True)
    va = ops.triplet_aggregate(fx, mask3, L, dropout=dropout)
    va.backward(d_out)
    torch.cuda.synchronize()
    return dict(B=B, N=N, C=C, L=L, sc=sc, fused=fused, d_out=d_out, mask3=mask3, dropout=dropout, va=va.detach(), grad=fx.grad,
                live=[b for b in range(B) if b % 2 == 0], dead=[b for b in range(B) if b % 2])


def run_skip(c, fused=None, d_out=None):
    from tgt_amd import ops
    fx = (c['fused'] if fused is None else fused).clone().requires_grad_(True)
    va = ops.triplet_aggregate(fx, c['mask3'], c['L'], dropout=c['dropout'], graph_scale=c['sc'])
    va.backward(c['d_out'] if d_out is None else d_out)
    torch.cuda.synchronize()
    return va.detach(), fx.grad


def zeros_exactly(t):
    return bool((t == 0).all())


# ------------------------------------------------------------------------------------------------------------------ 1: op level
@pytest.mark.parametrize('dropout', [(0.0, 0), DROPOUT], ids=['nodrop', 'drop'])
@pytest.mark.parametrize('gated', [True, False], ids=['gated', 'ungated'])
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_dropped_graphs_are_zeros_and_kept_graphs_do_not_move(shape, dtype, gated, dropout, monkeypatch):
    """forward: kept graphs bit-equal to the call without the factors (with attention dropout on: the drop pattern of a kept
    graph does not move), dropped graphs exact zeros; the whole input gradient bit-equal and finite, whether the backward is
    given the factors (TGT_TRI_SKIP=2) or computes every graph (the default)"""
    from tgt_amd import ops
    c = case(shape, dtype, gated, dropout)
    live, dead = c['live'], c['dead']
    assert live and dead
    if dropout[0] > 0:
        assert not torch.equal(c['va'], case(shape, dtype, gated, (0.0, 0))['va'])          # (the dropout is on)
    for b in dead:
        assert float(c['va'][b].float().abs().sum()) > 0                                   # (the full run computes them)
    for skip_bwd in (False, True):
        monkeypatch.setattr(ops, '_TRI_SKIP_BWD', skip_bwd)
        va, grad = run_skip(c)
        assert torch.equal(va[live], c['va'][live])
        assert zeros_exactly(va[dead])
        assert torch.isfinite(grad).all() and torch.isfinite(c['grad']).all()
        assert torch.equal(grad, c['grad'])
        assert zeros_exactly(grad[dead])


def test_graph_scale_is_validated():
    from tgt_amd import ops
    c = case('hg1', F32, True, (0.0, 0))
    for bad in (c['sc'].double(), c['sc'][:-1].contiguous(), c['sc'].cpu(), torch.stack([c['sc'], c['sc']], 1)[:, 0]):
        with pytest.raises(RuntimeError, match='graph_scale must be a contiguous float32 device tensor'):
            ops.triplet_aggregate(c['fused'], c['mask3'], c['L'], graph_scale=bad)


# ------------------------------------------------------------------------------------------------------------------ 2: not read
@pytest.mark.parametrize('gated', [True, False], ids=['gated', 'ungated'])
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_dropped_graphs_are_not_read(shape, dtype, gated, monkeypatch):
    """NaN in every `fused` row of the dropped graphs: the forward's output is exact zeros there and finite everywhere, kept
    graphs are still bit-equal.  With the factors handed to the backward, NaN in the dropped graphs' d_out too: their gradient
    rows are exact zeros, the kept graphs' rows bit-equal"""
    from tgt_amd import ops
    c = case(shape, dtype, gated, (0.0, 0))
    live, dead = c['live'], c['dead']
    fused = c['fused'].clone()
    fused[dead] = float('nan')
    monkeypatch.setattr(ops, '_TRI_SKIP_BWD', False)
    with torch.no_grad():
        va = ops.triplet_aggregate(fused, c['mask3'], c['L'], graph_scale=c['sc'])
    torch.cuda.synchronize()
    assert torch.isfinite(va).all() and zeros_exactly(va[dead]) and torch.equal(va[live], c['va'][live])
    monkeypatch.setattr(ops, '_TRI_SKIP_BWD', True)
    d_out = c['d_out'].clone()
    d_out[dead] = float('nan')
    va, grad = run_skip(c, fused, d_out)
    assert torch.isfinite(va).all() and zeros_exactly(va[dead]) and torch.equal(va[live], c['va'][live])
    assert torch.isfinite(grad).all() and zeros_exactly(grad[dead])
    assert torch.equal(grad[live], c['grad'][live])


# ------------------------------------------------------------------------------------- 3: projection-fused inference forward
CW, HP = 256, 16


@pytest.fixture
def small_rows(monkeypatch):
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_AGG_PROJ_INFER', True)
    monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 1)            # (the fused kernel also below 65536 edge rows)


def _attend(m, x, mask, sc=None, profile=False):
    from tgt_amd import ops
    prof = ops.profile_kernels(True) if profile else None
    try:
        va = m.attend(x, mask) if sc is None else m.attend(x, mask, graph_scale=sc)
        torch.cuda.synchronize()
        names = set(ops.kernel_times_ms(prof)) if profile else None
    finally:
        if profile:
            ops.profile_kernels(False)
    return va, names


@pytest.mark.parametrize('gated', [True, False], ids=['gated', 'ungated'])
@pytest.mark.parametrize('dtype', [BF16, F16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('N,nn_', [(20, (20, 13, 20, 1, 7)), (32, (32, 17, 32, 9, 32))], ids=['n20', 'n32'])
def test_projection_fused_forward_skips_dropped_graphs(N, nn_, dtype, gated, small_rows):
    from tgt_amd.tgt.layers import triplet
    B = 5
    cls = triplet.TripletAggregate if gated else triplet.TripletAggregateUngated
    m = gu.fill_params(cls(CW, HP), seed=7).cuda().to(dtype).eval()
    rng = np.random.default_rng(40 + N)
    x = rnd(rng, B, N, N, CW).to(dtype).cuda()
    mask = gu.additive_mask(list(nn_), N, torch.float32).cuda()
    sc = scale_of(B)
    live, dead = [0, 2, 4], [1, 3]
    x_nan = x.clone()
    x_nan[dead] = float('nan')
    with torch.no_grad():
        want, names = _attend(m, x, mask, profile=True)
        assert 'tgt_triplet_aggregate_proj_fwd' in names
        got, names = _attend(m, x, mask, sc, profile=True)
        assert 'tgt_triplet_aggregate_proj_fwd' in names and 'tgt_triplet_aggregate_fwd' not in names
        got_nan, _ = _attend(m, x_nan, mask, sc)
    assert want.shape == (B, N, N, 2 * CW) and torch.isfinite(want).all()
    for b in dead:
        assert float(want[b].float().abs().sum()) > 0
    for va in (got, got_nan):
        assert torch.equal(va[live], want[live])
        assert zeros_exactly(va[dead])                        # all 2C columns, those where E/G were parked included
    assert torch.equal(got, got_nan)
    # grad enabled: fused_linear + tgt_triplet_aggregate_fwd_skip, against its own run without the factors
    want_g, names = _attend(m, x, mask, profile=True)
    assert want_g.requires_grad and 'tgt_triplet_aggregate_fwd' in names and 'tgt_triplet_aggregate_proj_fwd' not in names
    got_g, names = _attend(m, x, mask, sc, profile=True)
    assert got_g.requires_grad and 'tgt_triplet_aggregate_fwd' in names and 'tgt_triplet_aggregate_proj_fwd' not in names
    assert torch.equal(got_g[live], want_g[live]) and zeros_exactly(got_g[dead])
    for b in dead:
        assert float(want_g[b].detach().float().abs().sum()) > 0


# ------------------------------------------------------------------------------------------------------------------- 4: layer
LAYER_SEED = 3


def _layer_run(triplet_type, skip, monkeypatch):
    """one training forward + backward of a TGT_Layer from a fixed seed: (h, e, parameter gradients, the factors the aggregate got)"""
    from tgt_amd import ops
    from tgt_amd.tgt.layers import blocks, TGT_Layer
    from tgt_amd.tgt.stack import Graph
    B, N = 8, 12
    nn_ = [12, 7, 12, 3, 9, 12, 1, 5]
    cfg = dict(gu.TINY_LAYER_CFG, triplet_type=triplet_type, drop_path=0.5)
    layer = gu.fill_params(TGT_Layer(**cfg), seed=21).cuda().train()
    rng = np.random.default_rng(22)
    h = rnd(rng, B, N, cfg['node_width']).float().cuda()
    e = rnd(rng, B, N, N, cfg['edge_width']).float().cuda()
    mask = gu.additive_mask(nn_, N, torch.float32).cuda()
    seen = []
    real = ops.projected_triplet_aggregate

    def spy(*args, **kw):
        seen.append(kw.get('graph_scale'))
        return real(*args, **kw)
    monkeypatch.setattr(ops, 'projected_triplet_aggregate', spy)
    monkeypatch.setattr(blocks, '_TRI_SKIP', skip)
    torch.manual_seed(LAYER_SEED)
    ops.reset_random_pools()
    g = layer(Graph(h=h, e=e, mask=mask))
    gh, ge = rnd(rng, *g.h.shape).float().cuda(), rnd(rng, *g.e.shape).float().cuda()
    ((g.h * gh).sum() + (g.e * ge).sum()).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in layer.named_parameters()}
    assert len(seen) == 1
    return g.h.detach(), g.e.detach(), grads, seen[0]


@pytest.mark.parametrize('triplet_type', ['aggregate', 'aggregate_ungated'])
def test_layer_hands_the_droppath_factor_to_the_aggregate(triplet_type, monkeypatch):
    """TGT_Layer draws the triplet branch's DropPath factor before the branch runs for a module that advertises
    takes_graph_scale; moving the draw changes no drawn value (the factors come from the device generator's pool, nothing else
    draws from it in between), so the layer's outputs and every parameter gradient are bit-equal with and without the skip"""
    from tgt_amd.tgt.layers import triplet
    assert triplet.TripletAggregate.takes_graph_scale is True
    assert triplet.TripletAggregateUngated.takes_graph_scale is True
    h0, e0, g0, sc0 = _layer_run(triplet_type, False, monkeypatch)
    h1, e1, g1, sc1 = _layer_run(triplet_type, True, monkeypatch)
    assert sc0 is None
    assert sc1 is not None and sc1.shape == (8,) and sc1.dtype == torch.float32
    n_zero = int((sc1 == 0).sum())
    assert 0 < n_zero < 8, sc1                                 # (all kept or all dropped: the test would pass vacuously)
    assert torch.isfinite(h1).all() and torch.isfinite(e1).all()
    assert torch.equal(h0, h1) and torch.equal(e0, e1)
    assert sorted(g0) == sorted(g1) and all(v is not None for v in g1.values())
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
