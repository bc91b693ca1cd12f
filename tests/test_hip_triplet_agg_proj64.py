"""The projection-fused triplet aggregate forward for 33..64 nodes (tgt_triplet_aggregate_proj64_fwd,
csrc/triplet_aggregate_proj64.hip; taken by ops.projected_triplet_aggregate when no backward can follow and
TGT_AGG_PROJ64_INFER is on), on the GPU.  Modelled on tests/test_hip_triplet_agg_proj.py.

The kernel fixes C = 256, H = 16, D = 16, so the shapes are already its smallest: one row past a 32-row tile (31 padding keys in
the second key tile, a one-node graph among others), config 4's node count with a ragged second tile, both tiles full with a graph
that ends inside the second tile, and a padded size that exceeds every graph.  Bars: tests/test_hip_ops.py's forward TOL against
the float64 oracle (the projection in float64 too) at every N, 2 * TOL between two HIP paths that are each held to that oracle.

A padding key k >= N has an all-zero X row, so its V is the projection BIAS: the large-bias cases (bias drawn at scale 4.0) fail
by orders of magnitude when such a key has any weight at all."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_util as gu
import parity_log
import triplet_hard_inputs as hi
from oracle import core

pytestmark = pytest.mark.gpu

TOL = parity_log.Tol({torch.bfloat16: 8e-3, torch.float16: 1e-3})          # tests/test_hip_ops.py: forward
CW, H = 256, 16
SHAPES64 = [(3, 33, (33, 1, 17)),   # one row past a 32-tile: 31 padding keys in the second key tile; a one-node graph
            (2, 48, (48, 35)),      # config 4's node count, ragged second tile
            (2, 64, (64, 40)),      # both tiles full; a graph that ends inside the second tile
            (1, 40, (33,))]         # the padded size exceeds every graph
DTYPES = [torch.bfloat16, torch.float16]
BF16 = torch.bfloat16
P_DROP, SEED = 0.25, 987654321                              # tests/test_hip_ops.py::test_triplet_aggregate_dropout
BIAS_SCALE = 4.0                                            # the large-bias cases (0.1 everywhere else)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return parity_log.record(float((a - b).norm() / (b.norm() + 1e-30)))


def rnd(rng, *shape, scale=1.0):
    return torch.from_numpy(rng.standard_normal(shape) * scale)


def _to_ref(x_hm, idx):
    out = torch.empty_like(x_hm)
    out[..., idx] = x_hm
    return out


def _oracle(x, w, b, mask4, L, gated, dropout=None):
    """(float64 oracle on the float64 projection in kernel channel order, its inputs)"""
    from tgt_amd import layout
    f64 = torch.nn.functional.linear(x.double(), w.double(), b.double())
    idx, oidx = layout.head_major_index(CW, H), layout.va_cols_head_major(CW, H)
    v_both = torch.cat([_to_ref(f64[..., p * CW:(p + 1) * CW], idx) for p in range(2)], -1)
    args = (v_both, f64[..., 2 * CW:L.used], mask4.double(), oidx)
    return core.triplet_aggregate_core(args[0], args[1], args[2], H, gated)[..., oidx], args


def _build(B, N, mask4, dtype, gated, seed, bias_scale=0.1):
    """inputs of one case on the device (mask4: (B,N,N,1) additive, CPU) and the float64 oracle's result"""
    from tgt_amd import ops
    L = ops.AggregateLayout(CW, H, gated=gated)
    assert L.width == L.used
    rng = np.random.default_rng(seed)
    x = rnd(rng, B, N, N, CW).to(dtype)
    w = (rnd(rng, L.width, CW) * CW ** -0.5).to(dtype)
    b = rnd(rng, L.width) * 0.1
    b[:2 * CW] *= bias_scale / 0.1                           # (the V bias alone: the E/G logits keep their scale)
    b = b.to(dtype)
    c = dict(B=B, N=N, L=L, dtype=dtype, gated=gated, x=x.cuda(), w=w.cuda(), b=b.cuda(), mask3=mask4.reshape(B, N, N).float().cuda(),
             cpu=(x, w, b, mask4))
    c['eg'] = torch.addmm(c['b'][2 * CW:], c['x'].view(-1, CW), c['w'][2 * CW:].t()).view(B, N, N, L.used - 2 * CW)
    c['ref'], c['oracle_in'] = _oracle(x, w, b, mask4, L, gated)
    return c


_cases = {}


def _case(shape, dtype, gated):
    """one case of SHAPES64 and its first fused run: computed once, never modified"""
    key = (shape, dtype, gated)
    if key not in _cases:
        B, N, nn_ = shape
        c = _build(B, N, gu.additive_mask(list(nn_), N, torch.float32), dtype, gated,
                   6400 + 100 * SHAPES64.index(shape) + 10 * DTYPES.index(dtype) + int(gated))
        code, out = _proj_fwd(c)
        assert code == 0
        c['out'] = out
        _cases[key] = c
    return _cases[key]


def _proj_fwd(c, dropout=(0.0, 0), sl=None, graph_scale=None):
    """one tgt_triplet_aggregate_proj64_fwd(_skip) call with a.v = NULL on a NaN-filled out: (return code, out).  sl: a slice of
    graphs."""
    from tgt_amd import ops, _lib
    x, eg, mask3 = (c[k] if sl is None else c[k][sl].contiguous() for k in ('x', 'eg', 'mask3'))
    out = torch.full((x.shape[0], c['N'], c['N'], 2 * CW), float('nan'), dtype=c['dtype'], device='cuda')
    a = ops._agg_proj_args(eg, mask3, out, c['L'], dropout)
    assert a.v[0] is None and a.v[1] is None
    args = (ops._ptr(x), CW, ops._ptr(c['w']), ops._ptr(c['b']), ops._stream())
    if graph_scale is None:
        code = _lib.lib().tgt_triplet_aggregate_proj64_fwd(C.byref(a), *args)
    else:
        code = _lib.lib().tgt_triplet_aggregate_proj64_fwd_skip(C.byref(a), ops._ptr(graph_scale), *args)
    torch.cuda.synchronize()
    return code, out


# ------------------------------------------------------------------------------------------------------------- 1, 2: parity
@pytest.mark.parametrize('gated', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES64)
def test_against_the_float64_oracle(shape, dtype, gated):
    c = _case(shape, dtype, gated)
    assert not torch.isnan(c['out']).any()                   # every row of the NaN-filled out was written
    err = rel(c['out'], c['ref'])
    print(f'aggregate proj64 vs oracle: {shape} {dtype} gated={gated}: rel-L2 {err:.3e} (bar {TOL[dtype]:.0e})')
    assert err < TOL[dtype], err


@pytest.mark.parametrize('gated', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES64)
def test_against_the_unfused_path(shape, dtype, gated):
    """the path without the kernel on the same inputs: library GEMM of the whole fused row + tgt_triplet_aggregate_fwd"""
    from tgt_amd import ops
    c = _case(shape, dtype, gated)
    with torch.no_grad():
        want = ops.triplet_aggregate(ops.linear(c['x'], c['w'], c['b']), c['mask3'], c['L'])
    torch.cuda.synchronize()
    err = rel(c['out'], want)
    print(f'aggregate proj64 vs unfused: {shape} {dtype} gated={gated}: rel-L2 {err:.3e} (bar {2 * TOL[dtype]:.0e})')
    assert err < 2 * TOL[dtype], err


# ------------------------------------------------------------------------------------------------------------- 3: large bias
@pytest.mark.parametrize('gated', [True, False])
@pytest.mark.parametrize('shape', SHAPES64[:2], ids=['n33', 'n48'])
def test_large_v_bias_padding_keys_have_no_weight(shape, gated):
    """V bias at scale 4.0 (BIAS_SCALE), bf16.  On the CPU first: the oracle with V and the result rounded to bf16 -- what any bf16
    kernel must do at least -- stays within TOL at this scale (measured here, printed; about 2.5e-3), so the bar is reachable and
    the scale did not have to be lowered."""
    B, N, nn_ = shape
    c = _build(B, N, gu.additive_mask(list(nn_), N, torch.float32), BF16, gated, 6900 + N + int(gated), bias_scale=BIAS_SCALE)
    v_both, eg64, mask64, oidx = c['oracle_in']
    assert float(c['b'][:2 * CW].float().abs().mean()) > 2.0
    rounded = core.triplet_aggregate_core(v_both.to(BF16).double(), eg64, mask64, H, gated)[..., oidx].to(BF16)
    floor = rel(rounded, c['ref'])
    print(f'aggregate proj64 large bias: bf16-rounded oracle vs oracle at bias scale {BIAS_SCALE}: rel-L2 {floor:.3e}')
    assert floor < TOL[BF16], (floor, 'lower BIAS_SCALE')
    code, out = _proj_fwd(c)
    assert code == 0 and not torch.isnan(out).any()
    err = rel(out, c['ref'])
    print(f'aggregate proj64 large bias vs oracle: {shape} gated={gated}: rel-L2 {err:.3e} (bar {TOL[BF16]:.0e})')
    assert err < TOL[BF16], err


# ---------------------------------------------------------------------------------------------------------------- 4: dropout
@pytest.mark.parametrize('gated', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES64)
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
    print(f'aggregate proj64 dropout vs oracle: {shape} {dtype} gated={gated}: rel-L2 {err:.3e} (bar {TOL[dtype]:.0e})')
    assert err < TOL[dtype], err
    _, other = _proj_fwd(c, dropout=(P_DROP, SEED + 1))
    assert not torch.equal(out, other)
    assert not torch.equal(out, c['out'])


# ----------------------------------------------------------------------------------------------------------- 5: bit equality
@pytest.mark.parametrize('gated', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
def test_bit_equal_runs_and_graph_indexing(dtype, gated):
    for shape in SHAPES64:
        c = _case(shape, dtype, gated)
        code, again = _proj_fwd(c)
        assert code == 0 and torch.equal(again.view(torch.int16), c['out'].view(torch.int16))
    c = _case(SHAPES64[0], dtype, gated)
    code, alone = _proj_fwd(c, sl=slice(0, 1))               # graph 0 of the B = 3 case, run alone with B = 1
    assert code == 0 and torch.equal(alone[0].view(torch.int16), c['out'][0].view(torch.int16))


@pytest.mark.parametrize('gated', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
def test_eg_inside_the_result_columns(dtype, gated):
    """the E/G rows placed where ops.projected_triplet_aggregate puts them -- inside `out`, each direction's in that direction's own
    columns -- give the result of the call with a separate E/G tensor, bit for bit, and every element of out is overwritten"""
    from tgt_amd import ops, _lib
    for shape in SHAPES64:
        c = _case(shape, dtype, gated)
        out = torch.full((c['B'], c['N'], c['N'], 2 * CW), float('nan'), dtype=dtype, device='cuda')
        egv, c0 = ops._agg_proj_eg_view(out, c['L'])
        ne = c['L'].used - 2 * CW
        egv.copy_(c['eg'].view(-1, ne))
        a = ops._agg_proj_args(out, c['mask3'], out, c['L'])
        code = _lib.lib().tgt_triplet_aggregate_proj64_fwd(C.byref(a), ops._ptr(c['x']), CW, ops._ptr(c['w']), ops._ptr(c['b']), ops._stream())
        torch.cuda.synchronize()
        assert code == 0 and not torch.isnan(out).any()
        assert torch.equal(out.view(torch.int16), c['out'].view(torch.int16))


# ------------------------------------------------------------------------------------------------- 6: nothing outside `out`
@pytest.mark.parametrize('gated', [True, False])
@pytest.mark.parametrize('shape', SHAPES64[:2], ids=['n33', 'n48'])
def test_nothing_outside_out_is_written(shape, gated):
    """`out` is a view inside a larger buffer with 4 KB of pattern on either side: both guards are unchanged after the call"""
    from tgt_amd import ops, _lib
    c = _case(shape, BF16, gated)
    B, N = c['B'], c['N']
    guard, n = 4096 // 2, B * N * N * 2 * CW
    buf = torch.empty(guard + n + guard, dtype=BF16, device='cuda')
    pattern = torch.arange(2 * guard, device='cuda', dtype=torch.int16) * 31 + 7
    buf.view(torch.int16)[:guard] = pattern[:guard]
    buf.view(torch.int16)[guard + n:] = pattern[guard:]
    out = buf[guard:guard + n].view(B, N, N, 2 * CW)
    out.fill_(float('nan'))
    a = ops._agg_proj_args(c['eg'], c['mask3'], out, c['L'])
    code = _lib.lib().tgt_triplet_aggregate_proj64_fwd(C.byref(a), ops._ptr(c['x']), CW, ops._ptr(c['w']), ops._ptr(c['b']), ops._stream())
    torch.cuda.synchronize()
    assert code == 0
    assert torch.equal(buf.view(torch.int16)[:guard], pattern[:guard])
    assert torch.equal(buf.view(torch.int16)[guard + n:], pattern[guard:])
    assert torch.equal(out.view(torch.int16), c['out'].view(torch.int16))


# ------------------------------------------------------------------------------------------------------------ 7: dropped graphs
@pytest.fixture
def small_rows(monkeypatch):
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_AGG_PROJ_INFER', True)
    monkeypatch.setattr(ops, '_AGG_PROJ64_INFER', True)
    monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 1)            # (the fused kernel also below 65536 edge rows)


class _Launches:
    """the names of every aggregate forward entry point ops._launch was asked for"""

    def __init__(self, monkeypatch):
        from tgt_amd import ops
        self.names = []
        real = ops._launch

        def launch(entry, *args, **kw):
            if entry.startswith('tgt_triplet_aggregate'):
                self.names.append(entry)
            return real(entry, *args, **kw)
        monkeypatch.setattr(ops, '_launch', launch)


def _module(cls_name, B, N, nn_, dtype=BF16, seed=5):
    from tgt_amd.tgt.layers import triplet
    m = gu.fill_params(getattr(triplet, cls_name)(CW, H), seed=seed).cuda().to(dtype).eval()
    rng = np.random.default_rng(seed + 1)
    e = rnd(rng, B, N, N, CW).to(dtype).cuda()
    mask = gu.additive_mask(list(nn_), N, torch.float32).cuda()
    return m, e, mask


@pytest.mark.parametrize('gated', [True, False], ids=['gated', 'ungated'])
@pytest.mark.parametrize('N,nn_', [(40, (40, 13, 33, 1, 40)), (64, (64, 40, 64, 9, 33))], ids=['n40', 'n64'])
def test_dropped_graphs_are_zeros_and_unread(N, nn_, gated, small_rows, monkeypatch):
    B = 5
    m, x, mask = _module('TripletAggregate' if gated else 'TripletAggregateUngated', B, N, nn_, seed=7)
    sc = torch.tensor([0.0 if b % 2 else 1.25 for b in range(B)], dtype=torch.float32, device='cuda')
    live, dead = [0, 2, 4], [1, 3]
    x_nan = x.clone()
    x_nan[dead] = float('nan')
    spy = _Launches(monkeypatch)
    with torch.no_grad():
        want = m.attend(x, mask)
        got = m.attend(x, mask, graph_scale=sc)
        got_nan = m.attend(x_nan, mask, graph_scale=sc)
    torch.cuda.synchronize()
    assert spy.names == ['tgt_triplet_aggregate_proj64_fwd'] + 2 * ['tgt_triplet_aggregate_proj64_fwd_skip']
    assert want.shape == (B, N, N, 2 * CW) and torch.isfinite(want).all()
    for b in dead:
        assert float(want[b].float().abs().sum()) > 0
    for va in (got, got_nan):
        assert torch.equal(va[live], want[live])
        assert bool((va[dead] == 0).all())                    # all 2C columns, those where E/G were parked included
    assert torch.equal(got, got_nan)


# ---------------------------------------------------------------------------------------------------------------- 8: pair mask
@pytest.mark.parametrize('gated', [True, False], ids=['gated', 'ungated'])
def test_pair_mask(gated):
    """tests/triplet_hard_inputs.py::pair_mask (not symmetric, leading key blocks closed) at N = 40, bf16"""
    B, N, nn_ = 2, 40, (40, 33)
    mask = hi.pair_mask(nn_, N, np.random.default_rng(6440 + int(gated)))
    c = _build(B, N, mask.unsqueeze(-1), BF16, gated, 6450 + int(gated))
    code, out = _proj_fwd(c)
    assert code == 0 and not torch.isnan(out).any()
    err = rel(out, c['ref'])
    print(f'aggregate proj64 pair mask vs oracle: gated={gated}: rel-L2 {err:.3e} (bar {TOL[BF16]:.0e})')
    assert err < TOL[BF16], err


# --------------------------------------------------------------------------------------------------------------- 9: module level
def _parent_path(m, e, mask):
    """the module's forward spelled out on the calls it made before ops.projected_triplet_aggregate existed"""
    from tgt_amd import ops
    lin_b = m.lin_EG if m.gated else m.lin_E
    fused = ops.fused_linear(m.tri_ln_e(e), m._table, (m.lin_V.weight, m.lin_V.bias, lin_b.weight, lin_b.bias))
    return m._out_proj(ops.triplet_aggregate(fused, ops.as_mask3(mask, e.shape[0], e.shape[1]), m._layout))


@pytest.mark.parametrize('cls_name', ['TripletAggregate', 'TripletAggregateUngated'])
def test_module_takes_the_fused_kernel_only_without_a_backward(cls_name, small_rows, monkeypatch):
    from tgt_amd import ops
    m, e, mask = _module(cls_name, 2, 48, (48, 35))
    keys = sorted(m.state_dict())
    spy = _Launches(monkeypatch)
    y_grad = m(e, mask)
    assert y_grad.requires_grad and spy.names == ['tgt_triplet_aggregate_fwd']
    assert torch.equal(y_grad, _parent_path(m, e, mask))     # grad enabled: the path it always took
    spy.names.clear()
    with torch.no_grad():
        y_infer = m(e, mask)
    for p in m.parameters():
        p.requires_grad_(False)
    y_frozen = m(e, mask)                                     # grad mode on, nothing requires grad: no backward either
    torch.cuda.synchronize()
    assert spy.names == 2 * ['tgt_triplet_aggregate_proj64_fwd']
    assert not y_infer.requires_grad and not y_frozen.requires_grad
    assert torch.equal(y_infer, y_frozen)
    err = rel(y_infer, y_grad)
    print(f'{cls_name}: N = 48 no_grad (fused) vs grad enabled (unfused): rel-L2 {err:.3e} (bar {2 * TOL[BF16]:.1e})')
    assert torch.isfinite(y_infer).all() and err < 2 * TOL[BF16], err
    # knob off: the no_grad call is the grad-enabled one, bit for bit
    monkeypatch.setattr(ops, '_AGG_PROJ64_INFER', False)
    spy.names.clear()
    with torch.no_grad():
        y_off = m(e, mask)
    assert spy.names == ['tgt_triplet_aggregate_fwd'] and torch.equal(y_off, y_grad.detach())
    monkeypatch.setattr(ops, '_AGG_PROJ64_INFER', True)
    # N = 32 still takes the N <= 32 kernel
    m32, e32, mask32 = _module(cls_name, 2, 32, (32, 20))
    spy.names.clear()
    with torch.no_grad():
        m32(e32, mask32)
    assert spy.names == ['tgt_triplet_aggregate_proj_fwd']
    assert sorted(m.state_dict()) == keys


# -------------------------------------------------------------------------------------------------------------------- 10: memory
def _peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del y
    return rise


def test_no_grad_peak_stays_below_the_fused_row(small_rows):
    """B = 4, N = 48: the no_grad call's peak rise stays below the size of the 576-wide tensor, the grad-enabled call's does not"""
    B, N = 4, 48
    m, e, mask = _module('TripletAggregate', B, N, (48, 20, 40, 33))
    with torch.no_grad():
        x = m.tri_ln_e(e)

    def infer():
        with torch.no_grad():
            return m.attend(x, mask)
    infer()                                                   # warm the allocator (and the mask / index memos)
    m.attend(x, mask)
    rise_infer, rise_grad = _peak_rise(infer), _peak_rise(lambda: m.attend(x, mask))
    fused_bytes = B * N * N * 576 * 2
    print(f'peak rise of attend at N = 48: no_grad {rise_infer} bytes, grad enabled {rise_grad} bytes, fused 576-wide row tensor {fused_bytes} bytes')
    assert rise_grad > fused_bytes, (rise_grad, fused_bytes)
    assert rise_infer < fused_bytes, (rise_infer, fused_bytes)


# -------------------------------------------------------------------------------------------------------------- 11: graph replay
def test_graphed_forward_replays_the_fused_kernel(small_rows, monkeypatch):
    """tgt_amd/pcqm/graphed.py on a 2-layer TGT-Agx2 distance predictor at N = 40: capture and replay take the new kernel and
    the replay equals the eager no_grad forward bit for bit"""
    from tgt_amd.pcqm import TGT_Distance
    from tgt_amd.pcqm.graphed import GraphedForward
    from tgt_amd.training import configs
    cfg = dict(configs.tgt_agx2_12x2(dropouts=False), model_height=2, layer_multiplier=1)
    geom = dict(B=2, N=40, num_nodes=[40, 23])
    model = gu.fill_params(TGT_Distance(**cfg), seed=61).cuda().eval()
    b0 = {k: v.cuda() for k, v in gu.model_batch(geom, seed=62).items()}
    b1 = {k: v.cuda() for k, v in gu.model_batch(geom, seed=63).items()}
    spy = _Launches(monkeypatch)
    gf = GraphedForward(model, b0, autocast_dtype=torch.bfloat16, warmup=1)
    assert len(spy.names) >= 2 * 2 and set(spy.names) == {'tgt_triplet_aggregate_proj64_fwd'}     # (warm-up + capture) x 2 layers
    for b in (b1, b0):
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            want = model(b)
        got = gf(b)
        torch.cuda.synchronize()
        got, want = (t if isinstance(t, (tuple, list)) else (t,) for t in (got, want))
        assert all(torch.equal(g, w_) for g, w_ in zip(got, want))
    assert set(spy.names) == {'tgt_triplet_aggregate_proj64_fwd'}
