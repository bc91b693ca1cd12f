"""Attention dropout inside the 16-wide-tile triplet kernels (tri_att16_fwd_kernel / tri_att16_bwd_kernel's DROP instantiations:
16-bit, D = 16, 33..64 nodes), which a call with dropout_p > 0 takes under TGT_TRI_DROP16=1 (tgt_triplet_attention_family; unset / 0:
the general 32-wide kernels, as before).  The library reads the variable per call, so the tests set it with monkeypatch.setenv.

Bars: the float64 oracle with the SAME keep pattern (golden_util.triplet_dropout_keep), the forward at TOL[dtype] and the gradients at
2 * TOL[dtype] of tests/test_hip_ops.py -- the bars the general kernels are held to with dropout on; a wrong pattern misses them by
orders of magnitude (half of the weights differ).  Switch off against on: the sum of the two bars (both sides are within theirs of
one oracle).  Everything else here is bitwise.

Shapes (B, N, node counts): (2, 33, (33, 20)) third block with one real row, odd N; (2, 48, (48, 35)) three full blocks;
(2, 49, (49, 40)) fourth block with one real row -- forward <4,4>, backward <2,4>; (2, 64, (64, 50)) four full blocks.  Widths
(C, H) = (256, 16) (several head groups) and (64, 4) (one).  Every input value is exact in bf16 AND fp16, so one float64 oracle per
(shape, width, variant, p) serves both dtypes; at N = 49 and 64 the variant x dtype product is thinned to four of its six members
(the oracle of one such case takes seconds)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import golden_util as gu
from test_hip_ops import TOL
from test_hip_triplet_drop_fast import _layout, _oracle_va, _rel, _rnd, _run_plain, _run_proj
from test_hip_triplet_dropout_counter import _check

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
SHAPES = [(2, 33, (33, 20)), (2, 48, (48, 35)), (2, 49, (49, 40)), (2, 64, (64, 50))]
WIDTHS = [(256, 16), (64, 4)]
VARIANTS = ['gated', 'ungated', 'axial']
PS = [0.1, 0.5]
SEED = 0x1234567890ABCDEF
FULL = [(v, d) for v in VARIANTS for d in (BF16, F16)]
THIN = [('gated', BF16), ('gated', F16), ('ungated', F16), ('axial', BF16)]
# (shape, variant, dtype) with the two dtypes of one variant next to each other: they share the cached oracle
GRID = [(s, v, d) for s in SHAPES for v, d in (FULL if s[1] <= 48 else THIN)]


@pytest.fixture(autouse=True)
def _switch_on(monkeypatch):
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 0)
    monkeypatch.setenv('TGT_TRI_DROP16', '1')


def _both(rng, *shape, scale=1.0):
    """standard normal values that bf16 and fp16 both hold exactly (bf16's 8 bits, and none below fp16's normal range)"""
    x = (_rnd(rng, *shape) * scale).to(BF16)
    return torch.where(x.to(F16).to(BF16) == x, x, torch.zeros_like(x))


@functools.lru_cache(maxsize=None)
def _plain_inputs(shape, width, variant):
    B, N, nodes = shape
    L = _layout(width, variant)
    rng = np.random.default_rng(100 * N + width[1])
    return _both(rng, B, N, N, L.width), _both(rng, B, N, N, 2 * width[0]), gu.additive_mask(list(nodes), N, torch.float32)


@functools.lru_cache(maxsize=2)
def _plain_oracle(shape, width, variant, p, seed=SEED):
    """(out, d_fused) of the float64 oracle, kept in float32; computed once per case, never modified"""
    fused, d_out, mask = _plain_inputs(shape, width, variant)
    f64 = fused.double().requires_grad_(True)
    va = _oracle_va(f64, mask, _layout(width, variant), width[0], width[1], p, seed)
    (va * d_out.double()).sum().backward()
    return va.detach().float(), f64.grad.float()


def _plain_case(shape, width, variant, dtype):
    fused, d_out, mask = _plain_inputs(shape, width, variant)
    return fused.to(dtype).cuda(), d_out.to(dtype).cuda(), mask.reshape(shape[0], shape[1], shape[1]).cuda()


@functools.lru_cache(maxsize=None)
def _proj_inputs(shape, variant):
    B, N, nodes = shape
    C_, H = WIDTHS[0]
    L = _layout(WIDTHS[0], variant)
    assert L.width == L.used
    rng = np.random.default_rng(7 * N + 1)
    return (_both(rng, B, N, N, C_), _both(rng, L.width, C_, scale=C_ ** -0.5), _both(rng, L.width, scale=0.1),
            _both(rng, B, N, N, 2 * C_), gu.additive_mask(list(nodes), N, torch.float32))


@functools.lru_cache(maxsize=2)
def _proj_oracle(shape, variant, p):
    """(out, dx, dw, db) of lin(x) -> the core in float64"""
    x, w, b, d_out, mask = _proj_inputs(shape, variant)
    C_, H = WIDTHS[0]
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    va = _oracle_va(torch.nn.functional.linear(x64, w64, b64), mask, _layout(WIDTHS[0], variant), C_, H, p, SEED)
    (va * d_out.double()).sum().backward()
    return va.detach().float(), x64.grad.float(), w64.grad.float(), b64.grad.float()


def _proj_case(shape, variant, dtype):
    x, w, b, d_out, mask = _proj_inputs(shape, variant)
    return tuple(t.to(dtype).cuda() for t in (x, w, b, d_out)) + (mask.reshape(shape[0], shape[1], shape[1]).cuda(),)


def _families(L, shape, dtype, p, colsum=False):
    """tgt_triplet_attention_family (forward, backward) for the argument blocks ops builds for this call"""
    from tgt_amd import ops, _lib
    B, N, _ = shape
    fused = torch.empty(B, N, N, L.width, dtype=dtype, device='cuda')
    out = torch.empty(B, N, N, 2 * L.C, dtype=dtype, device='cuda')
    mask3 = torch.zeros(B, N, N, device='cuda')
    cs = ops._colsum_workspace(B, L.width, L.used, fused.device) if colsum else None
    fwd = ops._tri_args(fused, mask3, out, L, dropout=(p, SEED))
    bwd = ops._tri_args(fused, mask3, out, L, out, torch.empty_like(fused), cs, dropout=(p, SEED))
    fam = _lib.lib().tgt_triplet_attention_family
    return fam(C.byref(fwd), 0), fam(C.byref(bwd), 1)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 1. the 16-wide tiles are what runs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('width', WIDTHS)
def test_the_dropout_call_takes_the_16_wide_tiles(width, monkeypatch):
    """(fails on the parent commit: its library ignores the variable)  Asserted so that a silent fallback to the general kernels
    cannot pass the parity checks below"""
    from tgt_amd import _lib
    t16, gen = _lib.TRI_FAMILY_TILES16, _lib.TRI_FAMILY_GENERAL
    for shape in SHAPES:
        for variant in VARIANTS:
            L = _layout(width, variant)
            for colsum in (False, True):
                assert _families(L, shape, BF16, 0.1, colsum) == (t16, t16)
                assert _families(L, shape, F16, 0.5, colsum) == (t16, t16)
    monkeypatch.setenv('TGT_TRI_DROP16', '0')
    L = _layout(width, 'gated')
    assert _families(L, SHAPES[0], BF16, 0.1) == (gen, gen) and _families(L, SHAPES[0], BF16, 0.0) == (t16, t16)


# ---- 2. parity with the float64 oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,variant,dtype', GRID)
@pytest.mark.parametrize('p', PS)
@pytest.mark.parametrize('width', WIDTHS)
def test_core_matches_the_oracle(shape, variant, dtype, p, width):
    L = _layout(width, variant)
    want = _plain_oracle(shape, width, variant, p)
    out, dx = _run_plain(_plain_case(shape, width, variant, dtype), L, p)
    e_out, e_dx = _rel(out, want[0]), _rel(dx, want[1][..., :L.used])
    print(f'fwd {e_out:.3e} d_fused {e_dx:.3e} (bars {TOL[dtype]:.1e} / {2 * TOL[dtype]:.1e})')
    assert e_out < TOL[dtype], ('fwd', e_out)
    assert e_dx < 2 * TOL[dtype], ('d_fused', e_dx)


@pytest.mark.parametrize('shape,variant,dtype', GRID)
@pytest.mark.parametrize('p', PS)
def test_projected_op_matches_the_oracle(shape, variant, dtype, p):
    """ops.projected_triplet_attention at C = 256: the backward with column sums (the projection's bias gradient)"""
    L = _layout(WIDTHS[0], variant)
    want = _proj_oracle(shape, variant, p)
    got = _run_proj(_proj_case(shape, variant, dtype), L, p)
    errs = [_rel(g, e) for g, e in zip(got, want)]
    print('fwd %.3e dx %.3e dw %.3e db %.3e' % tuple(errs), f'(bars {TOL[dtype]:.1e} / {2 * TOL[dtype]:.1e})')
    assert errs[0] < TOL[dtype], ('fwd', errs[0])
    for name, e in zip(('dx', 'dw', 'db'), errs[1:]):
        assert e < 2 * TOL[dtype], (name, e)


def test_the_launches_are_the_library_entries_that_route():
    from tgt_amd import ops
    L = _layout(WIDTHS[0], 'gated')
    case = _proj_case(SHAPES[0], 'gated', BF16)
    prof = ops.profile_kernels(True)
    try:
        _run_proj(case, L, 0.1)
        with torch.no_grad():          # no backward follows: still library GEMM + the attention core (the fused forward needs p = 0)
            ops.projected_triplet_attention(*case[:3], case[4], L, dropout=(0.1, SEED))
        torch.cuda.synchronize()
    finally:
        ops.profile_kernels(False)
    assert len(prof.get('tgt_triplet_attention_bwd', ())) == 1 and len(prof.get('tgt_triplet_attention_fwd', ())) == 2
    assert not prof.get('tgt_triplet_attention_proj64_fwd')


# ---- 3. switch off against on ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('variant,dtype', THIN)
def test_agrees_with_the_general_kernels(shape, variant, dtype, monkeypatch):
    from tgt_amd import _lib
    L = _layout(WIDTHS[0], variant)
    case = _proj_case(shape, variant, dtype)
    on = _run_proj(case, L, 0.1)
    L4 = _layout(WIDTHS[1], variant)
    case4 = _plain_case(shape, WIDTHS[1], variant, dtype)
    on4 = _run_plain(case4, L4, 0.5)
    monkeypatch.setenv('TGT_TRI_DROP16', '0')           # the library asks per call
    assert _families(L, shape, dtype, 0.1, True) == (_lib.TRI_FAMILY_GENERAL,) * 2
    off, off4 = _run_proj(case, L, 0.1), _run_plain(case4, L4, 0.5)
    errs = [_rel(a, b) for a, b in zip(on + on4, off + off4)]
    print('out %.3e dx %.3e dw %.3e db %.3e | out %.3e d_fused %.3e' % tuple(errs))
    assert errs[0] < 2 * TOL[dtype] and errs[4] < 2 * TOL[dtype], errs
    assert all(e < 4 * TOL[dtype] for e in errs[1:4] + errs[5:]), errs
    assert not _same(on, off)                            # two kernel families: the switch did switch


# ---- 4. bitwise contracts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('variant,dtype', THIN)
def test_two_runs_are_bit_identical(shape, variant, dtype):
    L = _layout(WIDTHS[0], variant)
    case = _proj_case(shape, variant, dtype)
    assert _same(_run_proj(case, L, 0.5), _run_proj(case, L, 0.5))
    L4 = _layout(WIDTHS[1], variant)
    case4 = _plain_case(shape, WIDTHS[1], variant, dtype)
    assert _same(_run_plain(case4, L4, 0.1), _run_plain(case4, L4, 0.1))


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('dtype', [BF16, F16])
def test_p0_does_not_see_the_switch(shape, dtype, monkeypatch):
    L = _layout(WIDTHS[0], 'gated')
    case = _proj_case(shape, 'gated', dtype)
    on = _run_proj(case, L, 0.0)
    monkeypatch.setenv('TGT_TRI_DROP16', '0')
    assert _same(on, _run_proj(case, L, 0.0))


@pytest.mark.parametrize('width', WIDTHS)
@pytest.mark.parametrize('shape', SHAPES)
def test_node_counts_change_nothing_below_the_count(shape, width):
    """with counts the units j >= n are not computed (zeros out, their d_out not read); everything with j < n -- the dropout units keep
    the tensor's N -- is the call without counts, bit for bit: out, and d_fused where the incoming gradient of the padded columns is
    zero (the counts' contract)"""
    B, N, nodes = shape
    L = _layout(width, 'gated')
    fused, d_out, mask3 = _plain_case(shape, width, 'gated', BF16)
    counts = torch.tensor(nodes, dtype=torch.int32, device='cuda')
    d_out = d_out.clone()
    for b_, n in enumerate(nodes):
        d_out[b_, :, n:] = 0
    case = (fused, d_out, mask3)
    out0, dx0 = _run_plain(case, L, 0.5)
    out1, dx1 = _run_plain(case, L, 0.5, node_counts=counts)
    for b_, n in enumerate(nodes):
        assert torch.equal(out1[b_, :n, :n], out0[b_, :n, :n])
        assert not out1[b_, :, n:].any()
    # (the partner rows of padded units are zeros with counts and products with a zero d_out without: equal up to the sign of zero)
    assert torch.equal(dx1.float() + 0.0, dx0.float() + 0.0)


def test_node_counts_with_column_sums():
    shape = SHAPES[2]
    L = _layout(WIDTHS[0], 'gated')
    x, w, b, d_out, mask3 = _proj_case(shape, 'gated', F16)
    counts = torch.tensor(shape[2], dtype=torch.int32, device='cuda')
    d_out = d_out.clone()
    for b_, n in enumerate(shape[2]):
        d_out[b_, :, n:] = 0
    case = (x, w, b, d_out, mask3)
    r0, r1 = _run_proj(case, L, 0.1), _run_proj(case, L, 0.1, node_counts=counts)
    for b_, n in enumerate(shape[2]):
        assert torch.equal(r1[0][b_, :n, :n], r0[0][b_, :n, :n]) and not r1[0][b_, :, n:].any()
    for got, want, name in zip(r1[1:], r0[1:], ('dx', 'dw', 'db')):
        assert _rel(got, want) < 2 * TOL[F16], name       # (other summation orders behind the kernel: the GEMMs see other zero rows)


@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[3]])
def test_dropped_graphs_are_zeros_and_kept_graphs_unchanged(shape, monkeypatch):
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_TRI_SKIP_BWD', True)          # (TGT_TRI_SKIP=2: the factors reach the backward kernel too)
    L = _layout(WIDTHS[0], 'gated')
    fused, d_out, mask3 = _plain_case(shape, WIDTHS[0], 'gated', BF16)
    gs = torch.tensor([2.0, 0.0], device='cuda')
    d_out = d_out.clone()
    d_out[1] = 0                                            # (behind the multiplication by the factor)
    case = (fused, d_out, mask3)
    out0, dx0 = _run_plain(case, L, 0.1)
    out1, dx1 = _run_plain(case, L, 0.1, graph_scale=gs)
    assert torch.equal(out1[0], out0[0]) and torch.equal(dx1[0], dx0[0])
    assert not out1[1].any() and not dx1[1].any()


# ---- 5. the step counter -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,variant,dtype', [(SHAPES[0], 'gated', BF16), (SHAPES[1], 'ungated', BF16), (SHAPES[2], 'axial', BF16),
                                                  (SHAPES[3], 'gated', F16)])
def test_the_16_wide_kernels_follow_the_step_counter(shape, variant, dtype):
    """the four checks of tests/test_hip_triplet_dropout_counter.py (counter at c == seed + c * golden without one; c = 0 == the plain
    call; successive counters differ; p = 0 never reads it), with and without column sums"""
    L = _layout(WIDTHS[0], variant)
    case = _proj_case(shape, variant, dtype)
    _check(lambda p, seed: _run_proj(case, L, p, seed))
    L4 = _layout(WIDTHS[1], variant)
    case4 = _plain_case(shape, WIDTHS[1], variant, dtype)
    _check(lambda p, seed: _run_plain(case4, L4, p, seed))


def test_forward_and_backward_of_one_counter_value_agree():
    """counter at 5: output AND gradient match the oracle at that value's effective seed -- both kernels drew the same pattern"""
    from tgt_amd import ops
    shape, width, p = SHAPES[2], WIDTHS[1], 0.5
    L = _layout(width, 'gated')
    want = _plain_oracle(shape, width, 'gated', p, ops.step_seed(SEED, 5))
    ctr = torch.full((1,), 5, dtype=torch.int64, device='cuda')
    ops.set_seed_counter(ctr)
    try:
        out, dx = _run_plain(_plain_case(shape, width, 'gated', BF16), L, p)
        torch.cuda.synchronize()
    finally:
        ops.set_seed_counter(None)
    assert _rel(out, want[0]) < TOL[BF16] and _rel(dx, want[1][..., :L.used]) < 2 * TOL[BF16]
    plain = _plain_oracle(shape, width, 'gated', p)
    assert _rel(out, plain[0]) > 0.3                         # (and not the pattern of the bare seed)


# ---- 6. module level ---------------------------------------------------------------------------------------------------------------
def test_module_output_with_the_switch_on_and_off(monkeypatch):
    from tgt_amd.tgt.layers.triplet import TripletAttention
    B, N = 2, 40
    rng = np.random.default_rng(5)
    e = _rnd(rng, B, N, N, 256).to(BF16).cuda()
    mask = gu.additive_mask([40, 33], N, torch.float32).cuda()
    mod = gu.fill_params(TripletAttention(256, 16, attention_dropout=0.2), seed=3).to(BF16).cuda().train()

    def step():
        torch.manual_seed(11)
        x = e.clone().requires_grad_(True)
        mod.zero_grad(set_to_none=True)
        y = mod(x, mask)
        y.float().square().mean().backward()
        return y.detach(), x.grad

    y1, g1 = step()
    y1b, g1b = step()
    assert torch.equal(y1, y1b) and torch.equal(g1, g1b)              # same torch seed: same drawn seed, same pattern
    monkeypatch.setenv('TGT_TRI_DROP16', '0')
    y0, g0 = step()
    assert torch.isfinite(y1.float()).all() and torch.isfinite(g1.float()).all()
    print('out %.3e dx %.3e' % (_rel(y1, y0), _rel(g1, g0)))
    assert _rel(y1, y0) < 2 * TOL[BF16]
    assert not torch.equal(y1, y0)                                      # two kernel families
    with torch.no_grad():                                               # MC-dropout prediction: a pattern is drawn, and it is this one
        torch.manual_seed(11)
        assert _rel(mod(e, mask), y1) < 2 * TOL[BF16]


def test_graphed_mc_forward_at_40_nodes_replays_the_eager_one():
    """the shallowest model the layer stack builds (two layers: its DropPath ramp divides by height - 1) at the full width (edge
    width 256, 16 triplet heads) and N = 40, every noise source on:
    GraphedForward(stochastic=True) == the eager graph-safe forward bit for bit, and two replays of one batch differ"""
    from tgt_amd import ops, pcqm, _lib
    from tgt_amd.pcqm.graphed import GraphedForward, eager_graph_safe_forward
    assert _families(_layout(WIDTHS[0], 'gated'), (2, 40, None), BF16, 0.1)[0] == _lib.TRI_FAMILY_TILES16
    geom = dict(B=2, N=40, num_nodes=[40, 33])
    kwargs = dict(gu.FULL_AT_CFG, model_height=2, source_dropout=0.3, drop_path=0.1, node_act_dropout=0.1, edge_act_dropout=0.1,
                  triplet_dropout=0.1)
    batch = {k: v.cuda() for k, v in gu.model_batch(geom, seed=41).items()}
    batch['num_nodes'] = torch.tensor(geom['num_nodes']).cuda()
    clone = lambda out: tuple(t.clone() for t in out) if isinstance(out, (tuple, list)) else (out.clone(),)
    runs = []
    try:
        for graphed in (False, True):
            torch.manual_seed(77)
            ops.reset_random_pools()
            m = gu.fill_params(pcqm.TGT_Multi(**kwargs), seed=32).cuda().train()
            if graphed:
                with GraphedForward(m, batch, autocast_dtype=BF16, warmup=1, stochastic=True) as gf:
                    gf.load(batch)
                    runs.append([clone(gf.sample()) for _ in range(2)])
            else:
                counter = torch.zeros(1, dtype=torch.int64, device='cuda')
                ops.graph_safe_rng(True)
                ops.set_seed_counter(counter)
                outs = []
                for it in range(3):
                    with torch.no_grad(), torch.autocast('cuda', dtype=BF16):
                        out = eager_graph_safe_forward(m, counter, batch)
                    if it:
                        outs.append(clone(out))
                runs.append(outs)
                ops.set_seed_counter(None)
                ops.graph_safe_rng(False)
    finally:
        ops.set_seed_counter(None)
        ops.graph_safe_rng(False)
    for want, got in zip(*runs):
        assert _same(want, got)
    assert all(torch.isfinite(t.float()).all() for t in runs[1][0])
    assert not _same(runs[1][0], runs[1][1])
