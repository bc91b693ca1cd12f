"""The projection-fused triplet attention forward for 33..64 nodes (tgt_triplet_attention_proj64_fwd,
csrc/triplet_attention_proj64.hip; taken by ops._ProjectedTripletAttention when no backward can follow and TGT_TRI_PROJ64_INFER is
on), on the GPU.  Modelled on tests/test_hip_triplet_agg_proj64.py.

The kernel fixes C = 256, H = 16, D = 16, so the shapes are already its smallest: one row past a 32-row tile (15 padding keys in the
last 16-key block, a one-node graph among others), config 4's node count (three key blocks: the fourth is skipped), every block full
with a graph that ends inside the second tile, and a padded size that exceeds every graph.  Bars: tests/test_hip_ops.py's forward
TOL against the float64 oracle (oracle.core.triplet_attention_core on the float64 projection) at every N, 2 * TOL between two HIP
paths that are each held to that oracle.

A padding key k >= N has an all-zero X row, so its K and V are the projection BIAS: the large-bias cases (V bias drawn at scale 4.0)
fail by orders of magnitude when such a key has any weight at all."""
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
SHAPES64 = [(3, 33, (33, 1, 17)),   # one row past a 32-tile: 15 padding keys in the last 16-key block; a one-node graph
            (2, 48, (48, 35)),      # config 4's node count
            (2, 64, (64, 40)),      # every tile full; a graph that ends inside the second tile
            (1, 40, (33,))]         # the padded size exceeds every graph
DTYPES = [torch.bfloat16, torch.float16]
VARIANTS = ['gated', 'ungated', 'axial']
BF16 = torch.bfloat16
V_BIAS_SCALE = 4.0                                          # the large-bias cases: V rows of the bias (Q / K: 0.1, as everywhere else)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return parity_log.record(float((a - b).norm() / (b.norm() + 1e-30)))


def rnd(rng, *shape, scale=1.0):
    return torch.from_numpy(rng.standard_normal(shape) * scale)


def _layout(variant):
    from tgt_amd import ops
    L = ops.TripletLayout(CW, H, gated=variant == 'gated', biased=variant != 'axial')
    assert L.D == 16 and L.width == L.used
    return L


def _oracle(f64, eg64, mask4, L, round_to=None):
    """float64 oracle on a float64 projection f64 (B,N,N,>=6C) in kernel channel order and the third-arm columns eg64
    ([E_in | G_in | E_out | G_out] / [E_in | E_out] / None); round_to: Q/K/V rounded to that dtype first"""
    from tgt_amd import layout
    idx, oidx = layout.head_major_index(CW, H), layout.va_cols_head_major(CW, H)

    def to_ref(t):
        o = torch.empty_like(t)
        o[..., idx] = t
        return o

    def blk(lo):
        parts = [to_ref(f64[..., lo + p * CW: lo + (p + 1) * CW]) for p in range(3)]
        if round_to is not None:
            parts = [p.to(round_to).double() for p in parts]
        return torch.cat(parts, -1)
    nb = (2 if L.gated else 1) * H
    eg_in = eg64[..., :nb] if L.biased else None
    eg_out = eg64[..., nb:2 * nb] if L.biased else None
    return core.triplet_attention_core(blk(0), eg_in, blk(3 * CW), eg_out, mask4.double(), H, L.gated, L.biased)[..., oidx]


def _build(B, N, mask4, dtype, variant, seed, v_bias_scale=0.1, hard=False):
    """inputs of one case on the device (mask4: (B,N,N,1) additive, CPU) and the float64 oracle's result.  hard: the third-arm
    columns are triplet_hard_inputs.hard_logits of the float64 projection, cast to dtype -- E/G is an INPUT of the kernel, so the
    oracle gets those columns as the kernel does (rounded); Q/K/V stay the float64 projection"""
    L = _layout(variant)
    rng = np.random.default_rng(seed)
    x = rnd(rng, B, N, N, CW).to(dtype)
    w = (rnd(rng, L.width, CW) * CW ** -0.5).to(dtype)
    b = rnd(rng, L.width) * 0.1
    for p in (2, 5):                                         # the V rows of both directions
        b[p * CW:(p + 1) * CW] *= v_bias_scale / 0.1
    b = b.to(dtype)
    c = dict(B=B, N=N, L=L, dtype=dtype, variant=variant, x=x.cuda(), w=w.cuda(), b=b.cuda(),
             mask3=mask4.reshape(B, N, N).float().cuda(), mask4=mask4)
    f64 = torch.nn.functional.linear(x.double(), w.double(), b.double())
    eg64 = f64[..., 6 * CW:L.used] if L.biased else None
    if not L.biased:
        c['eg'] = None
    elif hard:
        c['eg'] = hi.hard_logits(eg64, H, N, L.gated).to(dtype).cuda()
        eg64 = c['eg'].double().cpu()
    else:
        c['eg'] = torch.addmm(c['b'][6 * CW:], c['x'].view(-1, CW), c['w'][6 * CW:].t()).view(B, N, N, L.used - 6 * CW)
    c['f64'], c['eg64'] = f64, eg64
    c['ref'] = _oracle(f64, eg64, mask4, L)
    return c


_cases = {}


def _case(shape, dtype, variant):
    """one case of SHAPES64 and its first fused run: computed once, never modified"""
    key = (shape, dtype, variant)
    if key not in _cases:
        B, N, nn_ = shape
        c = _build(B, N, gu.additive_mask(list(nn_), N, torch.float32), dtype, variant,
                   7400 + 100 * SHAPES64.index(shape) + 10 * DTYPES.index(dtype) + VARIANTS.index(variant))
        code, out = _proj_fwd(c)
        assert code == 0, _err()
        c['out'] = out
        _cases[key] = c
    return _cases[key]


def _err():
    from tgt_amd import _lib
    return _lib.lib().tgt_last_error()


def _proj_fwd(c, sl=None, graph_scale=None, counts=False, x=None, out=None):
    """one tgt_triplet_attention_proj64_fwd(_counts) call with a.qkv = NULL on a NaN-filled out: (return code, out).  sl: a slice
    of graphs; counts: False = the plain entry point, None = _counts with NULL, a tensor = _counts with it; x: another X"""
    from tgt_amd import ops, _lib
    xs = c['x'] if x is None else x
    xs, eg, mask3 = (t if (sl is None or t is None) else t[sl].contiguous() for t in (xs, c['eg'], c['mask3']))
    if out is None:
        out = torch.full((xs.shape[0], c['N'], c['N'], 2 * CW), float('nan'), dtype=c['dtype'], device='cuda')
    a = ops._tri_args(None, mask3, out, c['L'], eg=eg, graph_scale=graph_scale)
    assert a.qkv[0] is None and a.qkv[1] is None and a.flags & _lib.TRI_NO_QKV_STORE
    args = (ops._ptr(xs), CW, ops._ptr(c['w']), ops._ptr(c['b']), ops._stream())
    if counts is False:
        code = _lib.lib().tgt_triplet_attention_proj64_fwd(C.byref(a), *args)
    else:
        code = _lib.lib().tgt_triplet_attention_proj64_fwd_counts(C.byref(a), ops._ptr(counts), *args)
    torch.cuda.synchronize()
    return code, out


# ------------------------------------------------------------------------------------------------------------- 1, 2: parity
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES64)
def test_against_the_float64_oracle(shape, dtype, variant):
    c = _case(shape, dtype, variant)
    assert not torch.isnan(c['out']).any()                   # every row of the NaN-filled out was written
    err = rel(c['out'], c['ref'])
    print(f'attention proj64 vs oracle: {shape} {dtype} {variant}: rel-L2 {err:.3e} (bar {TOL[dtype]:.0e})')
    assert err < TOL[dtype], err


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES64)
def test_against_the_unfused_path(shape, dtype, variant):
    """the path without the kernel on the same inputs: library GEMM of the whole fused row + tgt_triplet_attention_fwd"""
    from tgt_amd import ops
    c = _case(shape, dtype, variant)
    with torch.no_grad():
        want = ops.triplet_attention(ops.linear(c['x'], c['w'], c['b']), c['mask3'], c['L'])
    torch.cuda.synchronize()
    err = rel(c['out'], want)
    print(f'attention proj64 vs unfused: {shape} {dtype} {variant}: rel-L2 {err:.3e} (bar {2 * TOL[dtype]:.0e})')
    assert err < 2 * TOL[dtype], err


# ------------------------------------------------------------------------------------------------------------- 3: large bias
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('shape', SHAPES64[:2], ids=['n33', 'n48'])
def test_large_v_bias_padding_keys_have_no_weight(shape, variant):
    """V bias at scale 4.0 (V_BIAS_SCALE), Q / K bias at 0.1, bf16.  On the CPU first: the oracle with Q, K, V and the result
    rounded to bf16 -- what any bf16 kernel must do at least -- stays within TOL at this scale (measured here, printed), so the bar
    is reachable and the scale did not have to be lowered."""
    B, N, nn_ = shape
    c = _build(B, N, gu.additive_mask(list(nn_), N, torch.float32), BF16, variant, 7900 + N + VARIANTS.index(variant),
               v_bias_scale=V_BIAS_SCALE)
    assert float(c['b'][2 * CW:3 * CW].float().abs().mean()) > 2.0 and float(c['b'][:2 * CW].float().abs().mean()) < 0.2
    rounded = _oracle(c['f64'], c['eg64'], c['mask4'], c['L'], round_to=BF16).to(BF16)
    floor = rel(rounded, c['ref'])
    print(f'attention proj64 large V bias: bf16-rounded oracle vs oracle at V bias scale {V_BIAS_SCALE}: rel-L2 {floor:.3e}')
    assert floor < TOL[BF16], (floor, 'lower V_BIAS_SCALE')
    code, out = _proj_fwd(c)
    assert code == 0 and not torch.isnan(out).any()
    err = rel(out, c['ref'])
    print(f'attention proj64 large V bias vs oracle: {shape} {variant}: rel-L2 {err:.3e} (bar {TOL[BF16]:.0e})')
    assert err < TOL[BF16], err


# ---------------------------------------------------------------------------------------------------------------- 4: pair mask
@pytest.mark.parametrize('variant', VARIANTS)
def test_pair_mask_and_hard_logits(variant):
    """tests/triplet_hard_inputs.py::pair_mask (not symmetric, leading key blocks closed) with hard_logits at N = 40, bf16"""
    B, N, nn_ = 2, 40, (40, 33)
    mask = hi.pair_mask(nn_, N, np.random.default_rng(7440 + VARIANTS.index(variant)))
    c = _build(B, N, mask.unsqueeze(-1), BF16, variant, 7450 + VARIANTS.index(variant), hard=True)
    code, out = _proj_fwd(c)
    assert code == 0 and not torch.isnan(out).any()
    err = rel(out, c['ref'])
    print(f'attention proj64 pair mask + hard logits vs oracle: {variant}: rel-L2 {err:.3e} (bar {TOL[BF16]:.0e})')
    assert err < TOL[BF16], err


# ----------------------------------------------------------------------------------------------------------- 5: bit equality
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_bit_equal_runs_and_graph_indexing(dtype, variant):
    for shape in SHAPES64:
        c = _case(shape, dtype, variant)
        code, again = _proj_fwd(c)
        assert code == 0 and torch.equal(again.view(torch.int16), c['out'].view(torch.int16))
    c = _case(SHAPES64[0], dtype, variant)
    code, alone = _proj_fwd(c, sl=slice(0, 1))               # graph 0 of the B = 3 case, run alone with B = 1
    assert code == 0 and torch.equal(alone[0].view(torch.int16), c['out'][0].view(torch.int16))


@pytest.mark.parametrize('variant', VARIANTS[:2])
def test_third_arm_rows_at_any_alignment(variant):
    """the E/G columns inside a wider row at an odd element offset (ld_eg = 70, columns shifted by 3: nothing 8-byte aligned, the
    kernel's element-wise staging) give the result of the 8-byte aligned tensor, bit for bit"""
    from tgt_amd import ops, _lib
    for shape in (SHAPES64[0], SHAPES64[3]):
        c = _case(shape, BF16, variant)
        B, N, ne = c['B'], c['N'], c['eg'].shape[-1]
        wide = torch.full((B, N, N, 70), float('nan'), dtype=BF16, device='cuda')
        wide[..., 3:3 + ne] = c['eg']
        out = torch.full((B, N, N, 2 * CW), float('nan'), dtype=BF16, device='cuda')
        a = ops._tri_args(None, c['mask3'], out, c['L'], eg=c['eg'])
        a.eg = (C.c_void_p * 2)(wide.data_ptr(), wide.data_ptr())
        a.ld_eg = (C.c_int64 * 2)(70, 70)
        a.e_off = (C.c_int32 * 2)(a.e_off[0] + 3, a.e_off[1] + 3)
        a.g_off = (C.c_int32 * 2)(a.g_off[0] + 3, a.g_off[1] + 3)
        code = _lib.lib().tgt_triplet_attention_proj64_fwd(C.byref(a), ops._ptr(c['x']), CW, ops._ptr(c['w']), ops._ptr(c['b']), ops._stream())
        torch.cuda.synchronize()
        assert code == 0, _err()
        assert torch.equal(out.view(torch.int16), c['out'].view(torch.int16))


# ------------------------------------------------------------------------------------------------- 6: nothing outside `out`
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('shape', SHAPES64[:2], ids=['n33', 'n48'])
def test_nothing_outside_out_is_written(shape, variant):
    """`out` is a view inside a larger buffer with 4 KB of pattern on either side: both guards are unchanged after the call"""
    c = _case(shape, BF16, variant)
    B, N = c['B'], c['N']
    guard, n = 4096 // 2, B * N * N * 2 * CW
    buf = torch.empty(guard + n + guard, dtype=BF16, device='cuda')
    pattern = torch.arange(2 * guard, device='cuda', dtype=torch.int16) * 31 + 7
    buf.view(torch.int16)[:guard] = pattern[:guard]
    buf.view(torch.int16)[guard + n:] = pattern[guard:]
    out = buf[guard:guard + n].view(B, N, N, 2 * CW)
    out.fill_(float('nan'))
    code, _ = _proj_fwd(c, out=out)
    assert code == 0
    assert torch.equal(buf.view(torch.int16)[:guard], pattern[:guard])
    assert torch.equal(buf.view(torch.int16)[guard + n:], pattern[guard:])
    assert torch.equal(out.view(torch.int16), c['out'].view(torch.int16))


# ------------------------------------------------------------------------------------------------------------ 7: dropped graphs
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_dropped_graphs_are_zeros_and_unread(dtype, variant):
    """graph_scale with zeros: the dropped graphs' rows are all zeros even when their X is NaN, the live graphs are bit-equal to the
    call without factors"""
    for shape, factors in ((SHAPES64[0], (0.0, 1.25, 0.0)), (SHAPES64[1], (1.25, 0.0))):
        c = _case(shape, dtype, variant)
        sc = torch.tensor(factors, dtype=torch.float32, device='cuda')
        dead = [b for b, f in enumerate(factors) if f == 0.0]
        live = [b for b, f in enumerate(factors) if f != 0.0]
        x_nan = c['x'].clone()
        x_nan[dead] = float('nan')
        for xs in (c['x'], x_nan):
            code, out = _proj_fwd(c, graph_scale=sc, x=xs)
            assert code == 0
            assert torch.equal(out[dead].view(torch.int16), torch.zeros_like(out[dead]).view(torch.int16))
            assert torch.equal(out[live].view(torch.int16), c['out'][live].view(torch.int16))
        assert float(c['out'][dead].float().abs().max()) > 0


# --------------------------------------------------------------------------------------------------------------- 8: node counts
COUNTS = [0, 1, 15, 16, 17, 31, 32, 33, 40, 45]             # inside, on and past a 16- and a 32-row edge; 0, 1, N and past N (clamped)


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_node_counts(dtype, variant):
    """N = 40, one graph per count, every graph's mask fully open (keys are not bounded by the count): out[b, :, j >= n, :] is zeros,
    the block j < n is bit-equal to the call without counts, X rows of units j >= n are not read (NaN there), NULL counts equal the
    plain entry point"""
    N, B = 40, len(COUNTS)
    key = ('counts', dtype, variant)
    if key not in _cases:
        c = _build(B, N, gu.additive_mask([N] * B, N, torch.float32), dtype, variant, 7800 + 10 * DTYPES.index(dtype) + VARIANTS.index(variant))
        code, c['out'] = _proj_fwd(c)
        assert code == 0
        _cases[key] = c
    c = _cases[key]
    assert not torch.isnan(c['out']).any()
    counts = torch.tensor(COUNTS, dtype=torch.int32, device='cuda')
    # the X rows of a unit j >= n: edges (i, j) (both directions) and (j, k) (inward) -- NaN there must not matter
    x_nan = c['x'].clone()
    for b, n in enumerate(COUNTS):
        x_nan[b, :, n:] = float('nan')
        x_nan[b, n:, :] = float('nan')
    code, got = _proj_fwd(c, counts=counts)
    code2, got_nan = _proj_fwd(c, counts=counts, x=x_nan)
    assert code == 0 and code2 == 0
    for b, n in enumerate(COUNTS):
        n = min(n, N)
        assert torch.equal(got[b, :, n:].view(torch.int16), torch.zeros_like(got[b, :, n:]).view(torch.int16))
        assert torch.equal(got[b, :, :n].view(torch.int16), c['out'][b, :, :n].view(torch.int16))
        assert torch.equal(got_nan[b, :, n:].view(torch.int16), torch.zeros_like(got[b, :, n:]).view(torch.int16))
        # (keys ARE read up to N: rows (j, k >= n) of a real unit j are NaN in x_nan, so only the zero block is compared with it)
    code, null_counts = _proj_fwd(c, counts=None)
    assert code == 0 and torch.equal(null_counts.view(torch.int16), c['out'].view(torch.int16))


# --------------------------------------------------------------------------------------------------------------- 9: module level
@pytest.fixture
def small_rows(monkeypatch):
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_TRI_PROJ', True)
    monkeypatch.setattr(ops, '_TRI_PROJ_INFER', True)
    monkeypatch.setattr(ops, '_TRI_PROJ64_INFER', True)
    monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 1)            # (the fused kernels also below 65536 edge rows)


class _Launches:
    """the names of every triplet attention entry point ops._launch was asked for"""

    def __init__(self, monkeypatch):
        from tgt_amd import ops
        self.names = []
        real = ops._launch

        def launch(entry, *args, **kw):
            if entry.startswith('tgt_triplet_attention'):
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


@pytest.mark.parametrize('cls_name', ['TripletAttention', 'TripletAttentionUngated', 'AxialAttention'])
def test_module_takes_the_fused_kernel_only_without_a_backward(cls_name, small_rows, monkeypatch):
    from tgt_amd import ops
    m, e, mask = _module(cls_name, 2, 48, (48, 35))
    keys = sorted(m.state_dict())
    spy = _Launches(monkeypatch)
    # grad enabled: the entry points and the bits of the path without the feature (knob off = the parent's code)
    monkeypatch.setattr(ops, '_TRI_PROJ64_INFER', False)
    y_parent = m(e, mask)
    parent_names = list(spy.names)
    spy.names.clear()
    monkeypatch.setattr(ops, '_TRI_PROJ64_INFER', True)
    y_grad = m(e, mask)
    assert y_grad.requires_grad and spy.names == parent_names == ['tgt_triplet_attention_fwd']
    assert torch.equal(y_grad, y_parent)
    spy.names.clear()
    with torch.no_grad():
        y_infer = m(e, mask)
    for p in m.parameters():
        p.requires_grad_(False)
    y_frozen = m(e, mask)                                     # grad mode on, nothing requires grad: no backward either
    torch.cuda.synchronize()
    assert spy.names == 2 * ['tgt_triplet_attention_proj64_fwd']
    assert not y_infer.requires_grad and not y_frozen.requires_grad
    assert torch.equal(y_infer, y_frozen)
    err = rel(y_infer, y_grad)
    print(f'{cls_name}: N = 48 no_grad (fused) vs grad enabled (unfused): rel-L2 {err:.3e} (bar {2 * TOL[BF16]:.1e})')
    assert torch.isfinite(y_infer).all() and err < 2 * TOL[BF16], err
    # knob off: the no_grad call is the grad-enabled one, bit for bit
    monkeypatch.setattr(ops, '_TRI_PROJ64_INFER', False)
    spy.names.clear()
    with torch.no_grad():
        y_off = m(e, mask)
    assert spy.names == ['tgt_triplet_attention_fwd'] and torch.equal(y_off, y_grad.detach())
    monkeypatch.setattr(ops, '_TRI_PROJ64_INFER', True)
    # N = 32 still takes the N <= 32 kernel, N = 72 the key-blocked path
    for N, nn_, want in ((32, (32, 20), ['tgt_triplet_attention_proj_fwd']), (72, (72, 50), ['tgt_triplet_attention_fwd'])):
        m2, e2, mask2 = _module(cls_name, 2, N, nn_)
        spy.names.clear()
        with torch.no_grad():
            m2(e2, mask2)
        assert spy.names == want, (N, spy.names)
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


def test_no_grad_peak_stays_below_the_qkv_tensor(small_rows):
    """B = 4, N = 48: the no_grad call's peak rise stays below the size of the (B,N,N,6C) tensor, the grad-enabled call's does not"""
    B, N = 4, 48
    m, e, mask = _module('TripletAttention', B, N, (48, 20, 40, 33))
    with torch.no_grad():
        x = m.tri_ln_e(e)

    def infer():
        with torch.no_grad():
            return m.attend(x, mask)
    infer()                                                   # warm the allocator (and the mask / index memos)
    m.attend(x, mask)
    rise_infer, rise_grad = _peak_rise(infer), _peak_rise(lambda: m.attend(x, mask))
    qkv_bytes = B * N * N * 6 * CW * 2
    print(f'peak rise of attend at N = 48: no_grad {rise_infer} bytes, grad enabled {rise_grad} bytes, (B,N,N,6C) tensor {qkv_bytes} bytes')
    assert rise_grad > qkv_bytes, (rise_grad, qkv_bytes)
    assert rise_infer < qkv_bytes, (rise_infer, qkv_bytes)


# -------------------------------------------------------------------------------------------------------------- 11: graph replay
def test_graphed_forward_replays_the_fused_kernel(small_rows, monkeypatch):
    """tgt_amd/pcqm/graphed.py on a 2-layer TGT-At at N = 40.  Warm-up and CAPTURE go through ops._launch and take the new entry
    point, which the spy sees.  A replay calls no ops._launch at all (asserted), so what shows that the replayed graph holds the
    new kernel is the second half: the replay equals the eager no_grad forward -- which the spy sees taking the new entry point --
    bit for bit, on two batches."""
    from tgt_amd.pcqm import TGT_Multi
    from tgt_amd.pcqm.graphed import GraphedForward
    from tgt_amd.training import configs
    cfg = dict(configs.tgt_at_24l(dropouts=False), model_height=2)
    geom = dict(B=2, N=40, num_nodes=[40, 23])
    model = gu.fill_params(TGT_Multi(**cfg), seed=61).cuda().eval()
    b0 = {k: v.cuda() for k, v in gu.model_batch(geom, seed=62).items()}
    b1 = {k: v.cuda() for k, v in gu.model_batch(geom, seed=63).items()}
    spy = _Launches(monkeypatch)
    gf = GraphedForward(model, b0, autocast_dtype=torch.bfloat16, warmup=1)
    assert len(spy.names) >= 2 * 2 and set(spy.names) == {'tgt_triplet_attention_proj64_fwd'}     # (warm-up + capture) x 2 layers
    for b in (b1, b0):
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            want = model(b)
        seen = len(spy.names)
        got = gf(b)
        torch.cuda.synchronize()
        assert len(spy.names) == seen                         # (a replay launches nothing from the host side)
        got, want = (t if isinstance(t, (tuple, list)) else (t,) for t in (got, want))
        assert all(torch.equal(g, w_) for g, w_ in zip(got, want))
    assert set(spy.names) == {'tgt_triplet_attention_proj64_fwd'}     # (the eager reference forwards as well)
