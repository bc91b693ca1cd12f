"""The projection-fused triplet aggregate forward (tgt_triplet_aggregate_proj_fwd, csrc/triplet_aggregate_proj.hip; taken by
ops.projected_triplet_aggregate when no backward can follow and TGT_AGG_PROJ_INFER is on), on the GPU.

The kernel fixes C = 256, H = 16, D = 16, so the shapes are already its smallest: a full tile plus a ragged graph, padded rows in
the tile with a one-node graph among others, and the single-node graph.  Bars: tests/test_hip_ops.py's forward TOL against the
float64 oracle (the projection in float64 too), 2 * TOL between two paths that are each within TOL of that oracle.

Memory: the call measured is the aggregate step itself, `attend` on LayerNorm'd rows (what TGT_Layer calls; the LayerNorm and lin_O
around it are other steps, fused elsewhere).  Its no_grad form allocates the result and the fused weights alone -- the narrow E/G
rows are projected into columns of the result (ops._agg_proj_eg_view) -- so its peak stays below the 576-wide fused row."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_util as gu
import parity_log
from oracle import core

pytestmark = pytest.mark.gpu

TOL = parity_log.Tol({torch.bfloat16: 8e-3, torch.float16: 1e-3})          # tests/test_hip_ops.py: forward
CW, H = 256, 16
SHAPES = [(2, 32, (32, 20)), (3, 17, (17, 1, 9)), (1, 1, (1,))]          # B, N, num_nodes
DTYPES = [torch.bfloat16, torch.float16]
P_DROP, SEED = 0.25, 987654321                              # tests/test_hip_ops.py::test_triplet_aggregate_dropout


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return parity_log.record(float((a - b).norm() / (b.norm() + 1e-30)))


def rnd(rng, *shape, scale=1.0):
    return torch.from_numpy(rng.standard_normal(shape) * scale)


_cases = {}


def _case(shape, dtype, gated):
    """inputs of one case on the device, the float64 oracle's result (kernel channel order) and the first fused run: computed
    once, never modified"""
    key = (shape, dtype, gated)
    if key not in _cases:
        from tgt_amd import ops, layout
        B, N, nn_ = shape
        L = ops.AggregateLayout(CW, H, gated=gated)
        assert L.width == L.used
        rng = np.random.default_rng(1000 + 100 * SHAPES.index(shape) + 10 * DTYPES.index(dtype) + int(gated))
        x = rnd(rng, B, N, N, CW).to(dtype)
        w = (rnd(rng, L.width, CW) * CW ** -0.5).to(dtype)
        b = (rnd(rng, L.width) * 0.1).to(dtype)
        mask = gu.additive_mask(list(nn_), N, torch.float32)
        c = dict(B=B, N=N, L=L, dtype=dtype, gated=gated, x=x.cuda(), w=w.cuda(), b=b.cuda(), mask3=mask.reshape(B, N, N).cuda())
        c['eg'] = torch.addmm(c['b'][2 * CW:], c['x'].view(-1, CW), c['w'][2 * CW:].t()).view(B, N, N, L.used - 2 * CW)
        # float64 oracle on the float64 projection, channels re-ordered as tests/test_hip_ops.py::test_triplet_aggregate does
        f64 = torch.nn.functional.linear(x.double(), w.double(), b.double())
        idx, oidx = layout.head_major_index(CW, H), layout.va_cols_head_major(CW, H)
        v_both = torch.cat([_to_ref(f64[..., p * CW:(p + 1) * CW], idx) for p in range(2)], -1)
        c['oracle_in'] = (v_both, f64[..., 2 * CW:L.used], mask.double(), oidx)
        c['ref'] = core.triplet_aggregate_core(v_both, f64[..., 2 * CW:L.used], mask.double(), H, gated)[..., oidx]
        code, out = _proj_fwd(c)
        assert code == 0
        c['out'] = out
        _cases[key] = c
    return _cases[key]


def _to_ref(x_hm, idx):
    out = torch.empty_like(x_hm)
    out[..., idx] = x_hm
    return out


def _proj_fwd(c, dropout=(0.0, 0), sl=None):
    """one tgt_triplet_aggregate_proj_fwd call with a.v = NULL on a NaN-filled out: (return code, out).  sl: a slice of graphs."""
    from tgt_amd import ops, _lib
    x, eg, mask3 = (c[k] if sl is None else c[k][sl].contiguous() for k in ('x', 'eg', 'mask3'))
    out = torch.full((x.shape[0], c['N'], c['N'], 2 * CW), float('nan'), dtype=c['dtype'], device='cuda')
    a = ops._agg_proj_args(eg, mask3, out, c['L'], dropout)
    assert a.v[0] is None and a.v[1] is None
    code = _lib.lib().tgt_triplet_aggregate_proj_fwd(C.byref(a), ops._ptr(x), CW, ops._ptr(c['w']), ops._ptr(c['b']), ops._stream())
    torch.cuda.synchronize()
    return code, out


@pytest.mark.parametrize('gated', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_against_the_float64_oracle(shape, dtype, gated):
    c = _case(shape, dtype, gated)
    assert not torch.isnan(c['out']).any()                   # every row of the NaN-filled out was written
    tol = TOL[dtype]
    err = rel(c['out'], c['ref'])
    print(f'aggregate proj vs oracle: {shape} {dtype} gated={gated}: rel-L2 {err:.3e} (bar {TOL[dtype]:.0e})')
    assert err < tol, err


@pytest.mark.parametrize('gated', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_against_the_unfused_path(shape, dtype, gated):
    """today's path on the same inputs: library GEMM of the whole fused row + tgt_triplet_aggregate_fwd"""
    from tgt_amd import ops
    c = _case(shape, dtype, gated)
    with torch.no_grad():
        want = ops.triplet_aggregate(ops.linear(c['x'], c['w'], c['b']), c['mask3'], c['L'])
    torch.cuda.synchronize()
    err = rel(c['out'], want)
    print(f'aggregate proj vs unfused: {shape} {dtype} gated={gated}: rel-L2 {err:.3e} (bar {2 * TOL[dtype]:.0e})')
    assert err < 2 * TOL[dtype], err


@pytest.mark.parametrize('gated', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_dropout_drops_what_the_plain_kernel_drops(shape, dtype, gated):
    """p = 0.25: within TOL of the oracle GIVEN the keep pattern of the plain kernel's generator (unit (b*2 + dir)*H + h)"""
    c = _case(shape, dtype, gated)
    B, N = c['B'], c['N']
    units = ((np.arange(B)[:, None, None] * 2 + np.arange(2)[None, :, None]) * H + np.arange(H)[None, None, :]).reshape(-1)
    keep, scale = gu.triplet_dropout_keep(SEED, P_DROP, units, N)
    keep = torch.from_numpy(keep.reshape(B, 2, H, N, N))                # (b, dir, h, i, k)
    keep_in = keep[:, 0].permute(0, 2, 3, 1).contiguous()               # (b, i, k, h)
    keep_out = keep[:, 1].permute(0, 3, 2, 1).contiguous()              # (b, k, i, h)
    v_both, eg64, mask64, oidx = c['oracle_in']
    ref = core.triplet_aggregate_core(v_both, eg64, mask64, H, gated, dropout=(keep_in, keep_out, scale))[..., oidx]
    code, out = _proj_fwd(c, dropout=(P_DROP, SEED))
    assert code == 0 and not torch.isnan(out).any()
    err = rel(out, ref)
    print(f'aggregate proj dropout vs oracle: {shape} {dtype} gated={gated}: rel-L2 {err:.3e} (bar {TOL[dtype]:.0e})')
    assert err < TOL[dtype], err
    if N > 1:                                                # (one node: a single weight, both seeds may keep it)
        _, other = _proj_fwd(c, dropout=(P_DROP, SEED + 1))
        assert not torch.equal(out, other)
        assert not torch.equal(out, c['out'])


@pytest.mark.parametrize('gated', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
def test_bit_equal_runs_and_graph_indexing(dtype, gated):
    for shape in SHAPES:
        c = _case(shape, dtype, gated)
        code, again = _proj_fwd(c)
        assert code == 0 and torch.equal(again.view(torch.int16), c['out'].view(torch.int16))
    c = _case(SHAPES[1], dtype, gated)
    code, alone = _proj_fwd(c, sl=slice(0, 1))               # graph 0 of the B = 3 case, run alone with B = 1
    assert code == 0 and torch.equal(alone[0].view(torch.int16), c['out'][0].view(torch.int16))


# ----------------------------------------------------------------------------------------------------------------- module level
class _Spy:
    """which argument builder every aggregate forward went through: 'proj' (ops._agg_proj_args, the fused entry point) or
    'plain' (ops._agg_args alone: tgt_triplet_aggregate_fwd / _bwd)"""

    def __init__(self, monkeypatch):
        from tgt_amd import ops
        self.calls = []
        real_proj, real_plain = ops._agg_proj_args, ops._agg_args

        def plain(*args, **kw):
            self.calls.append('plain')
            return real_plain(*args, **kw)

        def proj(*args, **kw):
            a = real_proj(*args, **kw)
            assert self.calls.pop() == 'plain'               # (it builds on _agg_args)
            self.calls.append('proj')
            return a
        monkeypatch.setattr(ops, '_agg_args', plain)
        monkeypatch.setattr(ops, '_agg_proj_args', proj)


@pytest.fixture
def small_rows(monkeypatch):
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_AGG_PROJ_INFER', True)
    monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 1)            # (the fused kernel also below 65536 edge rows)


def _module(cls_name, B, N, nn_, dtype=torch.bfloat16, seed=5):
    from tgt_amd.tgt.layers import triplet
    m = gu.fill_params(getattr(triplet, cls_name)(CW, H), seed=seed).cuda().to(dtype).eval()
    rng = np.random.default_rng(seed + 1)
    e = rnd(rng, B, N, N, CW).to(dtype).cuda()
    mask = gu.additive_mask(list(nn_), N, torch.float32).cuda()
    return m, e, mask


def _parent_path(m, e, mask):
    """the module's forward spelled out on the calls it made before ops.projected_triplet_aggregate existed"""
    from tgt_amd import ops
    lin_b = m.lin_EG if m.gated else m.lin_E
    fused = ops.fused_linear(m.tri_ln_e(e), m._table, (m.lin_V.weight, m.lin_V.bias, lin_b.weight, lin_b.bias))
    return m._out_proj(ops.triplet_aggregate(fused, ops.as_mask3(mask, e.shape[0], e.shape[1]), m._layout))


@pytest.mark.parametrize('cls_name', ['TripletAggregate', 'TripletAggregateUngated'])
def test_module_takes_the_fused_kernel_only_without_a_backward(cls_name, small_rows, monkeypatch):
    from tgt_amd import ops
    m, e, mask = _module(cls_name, 2, 32, (32, 20))
    keys = sorted(m.state_dict())
    spy = _Spy(monkeypatch)
    y_grad = m(e, mask)
    assert y_grad.requires_grad and spy.calls == ['plain']
    assert torch.equal(y_grad, _parent_path(m, e, mask))     # grad enabled: the path it always took
    spy.calls.clear()
    with torch.no_grad():
        y_infer = m(e, mask)
    for p in m.parameters():
        p.requires_grad_(False)
    y_frozen = m(e, mask)                                     # grad mode on, nothing requires grad: no backward either
    torch.cuda.synchronize()
    assert spy.calls == ['proj', 'proj']
    assert not y_infer.requires_grad and not y_frozen.requires_grad
    assert torch.equal(y_infer, y_frozen)
    err = rel(y_infer, y_grad)
    print(f'{cls_name}: no_grad (fused) vs grad enabled (unfused): rel-L2 {err:.3e} (bar {2 * TOL[torch.bfloat16]:.1e})')
    assert torch.isfinite(y_infer).all() and err < 2 * TOL[torch.bfloat16], err
    # knob off: the no_grad call is the grad-enabled one, bit for bit
    monkeypatch.setattr(ops, '_AGG_PROJ_INFER', False)
    spy.calls.clear()
    with torch.no_grad():
        y_off = m(e, mask)
    assert spy.calls == ['plain'] and torch.equal(y_off, y_grad.detach())
    assert sorted(m.state_dict()) == keys


def _peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del y
    return rise


def _peaks():
    B, N = 4, 32
    m, e, mask = _module('TripletAggregate', B, N, (32, 20, 32, 9))
    with torch.no_grad():
        x = m.tri_ln_e(e)

    def infer():
        with torch.no_grad():
            return m.attend(x, mask)
    infer()                                                   # warm the allocator (and the mask / index memos)
    m.attend(x, mask)
    rise_infer, rise_grad = _peak_rise(infer), _peak_rise(lambda: m.attend(x, mask))
    print(f'peak rise of attend: no_grad {rise_infer} bytes, grad enabled {rise_grad} bytes, fused 576-wide row tensor {B * N * N * 576 * 2} bytes')
    return B * N * N, rise_infer, rise_grad


def test_no_grad_peak_stays_below_the_fused_row(small_rows):
    """B = 4, N = 32: the no_grad call's peak rise stays below the size of the 576-wide tensor, the grad-enabled call's does not"""
    rows, rise_infer, rise_grad = _peaks()
    fused_bytes = rows * 576 * 2
    assert rise_grad > fused_bytes, (rise_grad, fused_bytes)
    assert rise_infer < fused_bytes, (rise_infer, fused_bytes)


def test_no_grad_forward_does_not_allocate_the_fused_row(small_rows):
    """both calls allocate the fused weights and the result; the grad-enabled one also the 576-wide fused row (the slack of 64
    channels covers allocator rounding)"""
    rows, rise_infer, rise_grad = _peaks()
    assert rise_grad - rise_infer >= rows * 512 * 2, (rise_grad, rise_infer)


@pytest.mark.parametrize('gated', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
def test_eg_inside_the_result_columns(dtype, gated):
    """the E/G rows placed where ops.projected_triplet_aggregate puts them -- inside `out`, each direction's in that direction's own
    columns -- give the result of the call with a separate E/G tensor, bit for bit, and every element of out is overwritten"""
    from tgt_amd import ops, _lib
    for shape in SHAPES:
        c = _case(shape, dtype, gated)
        out = torch.full((c['B'], c['N'], c['N'], 2 * CW), float('nan'), dtype=dtype, device='cuda')
        egv, c0 = ops._agg_proj_eg_view(out, c['L'])
        ne = c['L'].used - 2 * CW
        assert c0 + ne // 2 == CW and c0 >= 0                # half of the E/G columns on either side of the directions' boundary
        egv.copy_(c['eg'].view(-1, ne))
        a = ops._agg_proj_args(out, c['mask3'], out, c['L'])
        code = _lib.lib().tgt_triplet_aggregate_proj_fwd(C.byref(a), ops._ptr(c['x']), CW, ops._ptr(c['w']), ops._ptr(c['b']), ops._stream())
        torch.cuda.synchronize()
        assert code == 0 and torch.equal(out.view(torch.int16), c['out'].view(torch.int16))


def test_graphed_forward_replays_the_fused_kernel(small_rows, monkeypatch):
    """tgt_amd/pcqm/graphed.py on a 2-layer TGT-Agx2 distance predictor at N = 20: capture and replay take the fused kernel and
    the replay equals the eager no_grad forward bit for bit"""
    from tgt_amd.pcqm import TGT_Distance
    from tgt_amd.pcqm.graphed import GraphedForward
    from tgt_amd.training import configs
    cfg = dict(configs.tgt_agx2_12x2(dropouts=False), model_height=2, layer_multiplier=1)
    geom = dict(B=2, N=20, num_nodes=[20, 7])
    model = gu.fill_params(TGT_Distance(**cfg), seed=61).cuda().eval()
    b0 = {k: v.cuda() for k, v in gu.model_batch(geom, seed=62).items()}
    b1 = {k: v.cuda() for k, v in gu.model_batch(geom, seed=63).items()}
    spy = _Spy(monkeypatch)
    gf = GraphedForward(model, b0, autocast_dtype=torch.bfloat16, warmup=1)
    assert len(spy.calls) >= 2 * 2 and set(spy.calls) == {'proj'}      # (warm-up + capture) x 2 layers, all fused
    for b in (b1, b0):
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            want = model(b)
        got = gf(b)
        torch.cuda.synchronize()
        got, want = (t if isinstance(t, (tuple, list)) else (t,) for t in (got, want))
        assert all(torch.equal(g, w_) for g, w_ in zip(got, want))
    assert set(spy.calls) == {'proj'}
