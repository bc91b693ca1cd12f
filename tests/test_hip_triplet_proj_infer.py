"""The projection-fused triplet forward without its Q/K/V stores (TGT_TRI_NO_QKV_STORE, csrc/triplet_attention_proj.hip: the
STORE = false instantiation; ops._ProjectedTripletAttention takes it when no backward can follow), on the GPU.

The flagged kernel is the training kernel minus the global stores of the projected rows, so `out` is compared with
torch.equal -- no tolerance -- and the training branch is held to the float64 oracle at the bars of tests/test_hip_ops.py.
Shapes: C = 256 is fixed by the kernel; one head group with a ragged graph at the full tile, two head groups with padded rows
in every tile, and the single-node graph.  The kernel also fixes D = 16, so the one-head-group cases (H = 8) exist at the C
level only: 8 heads of 16 channels inside the 256-wide Q / K / V / O blocks of the H = 16 row layout, the other 128 channels of
each block untouched (`_layout`).  The Python layer derives D = C / H and cannot express them; what goes through ops.py or a
module runs H = 16."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_util as gu
from oracle import core

pytestmark = pytest.mark.gpu

TOL = {torch.bfloat16: 8e-3, torch.float16: 1e-3}          # tests/test_hip_ops.py: forward; gradients twice that
CW = 256
SHAPES = [(2, 32, (32, 20), 8), (2, 20, (20, 7), 16), (1, 1, (1,), 8)]          # B, N, num_nodes, H
DTYPES = [torch.bfloat16, torch.float16]
VARIANTS = ['gated', 'ungated', 'axial']
SENTINEL = 0x5AA5                                           # bit pattern of every 16-bit element of a Q/K/V buffer nobody may write


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rnd(rng, *shape, scale=1.0):
    return torch.from_numpy(rng.standard_normal(shape) * scale)


_cases = {}


def _layout(H, variant):
    """the row layout of C = 256, 16 heads of D = 16, walked by the first H heads only (H = 8: one head group)"""
    from tgt_amd import ops
    L = ops.TripletLayout(CW, 16, gated=variant == 'gated', biased=variant != 'axial')
    assert L.D == 16 and L.width == L.used and H in (8, 16)
    L.H = H
    return L


def _cols(H, blocks):
    """the channels the first H heads own in a row of `blocks` 256-wide blocks"""
    return torch.cat([torch.arange(H * 16) + k * CW for k in range(blocks)]).cuda()


def _case(shape, dtype, variant):
    """inputs of one C-level case on the device + the unflagged run's (out, Q/K/V rows): computed once, never modified"""
    key = (shape, dtype, variant)
    if key not in _cases:
        from tgt_amd import ops
        B, N, nn_, H = shape
        L = _layout(H, variant)
        rng = np.random.default_rng(100 * SHAPES.index(shape) + 10 * DTYPES.index(dtype) + VARIANTS.index(variant))
        x = rnd(rng, B, N, N, CW).to(dtype).cuda()
        w = (rnd(rng, L.width, CW) * CW ** -0.5).to(dtype).cuda()
        b = (rnd(rng, L.width) * 0.1).to(dtype).cuda()
        mask3 = gu.additive_mask(list(nn_), N, torch.float32).reshape(B, N, N).cuda()
        eg = torch.addmm(b[6 * CW:], x.view(-1, CW), w[6 * CW:].t()).view(B, N, N, L.used - 6 * CW) if L.biased else None
        c = dict(B=B, N=N, L=L, x=x, w=w, b=b, mask3=mask3, eg=eg, dtype=dtype, ocols=_cols(H, 2), qcols=_cols(H, 6))
        qkv = torch.zeros(B, N, N, 6 * CW, dtype=dtype, device='cuda')
        code, out = _proj_fwd(c, qkv, flag=False)
        assert code == 0
        c['out'], c['qkv'] = out, qkv
        _cases[key] = c
    return _cases[key]


def _proj_fwd(c, qkv, flag, graph_scale=None):
    """one tgt_triplet_attention_proj_fwd call: (return code, out).  qkv None = null pointers."""
    from tgt_amd import ops, _lib
    out = torch.full((c['B'], c['N'], c['N'], 2 * CW), float('nan'), dtype=c['dtype'], device='cuda')
    a = ops._tri_args(qkv if qkv is not None else torch.empty(c['B'], c['N'], c['N'], 6 * CW, dtype=c['dtype'], device='cuda'),
                      c['mask3'], out, c['L'], eg=c['eg'], graph_scale=graph_scale)
    if qkv is None:
        a.qkv = (C.c_void_p * 2)(None, None)
    if flag:
        a.flags |= _lib.TRI_NO_QKV_STORE
    code = _lib.lib().tgt_triplet_attention_proj_fwd(C.byref(a), ops._ptr(c['x']), CW, ops._ptr(c['w']), ops._ptr(c['b']), ops._stream())
    torch.cuda.synchronize()
    return code, out


def _sentinel(c):
    return torch.full((c['B'], c['N'], c['N'], 6 * CW), SENTINEL, dtype=torch.int16, device='cuda')


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_flag_leaves_qkv_untouched_and_out_bit_equal(shape, dtype, variant):
    from tgt_amd import ops
    c = _case(shape, dtype, variant)
    oc, qc = c['ocols'], c['qcols']
    assert not torch.isnan(c['out'][..., oc]).any()                              # the plain run wrote every O row of its heads ...
    want = ops.triplet_attention(ops.linear(c['x'], c['w'], c['b']), c['mask3'], c['L'])
    assert rel(c['out'][..., oc], want[..., oc]) < TOL[dtype]                    # ... with the attention of the projected rows
    assert rel(c['qkv'][..., qc], ops.linear(c['x'], c['w'][:6 * CW], c['b'][:6 * CW])[..., qc]) < TOL[dtype]      # (and did write Q/K/V)
    buf = _sentinel(c)
    code, out = _proj_fwd(c, buf.view(dtype), flag=True)
    assert code == 0
    assert torch.equal(out.view(torch.int16), c['out'].view(torch.int16))
    assert torch.equal(buf, _sentinel(c))


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_flag_takes_null_qkv_pointers(shape, dtype, variant):
    from tgt_amd import _lib
    c = _case(shape, dtype, variant)
    code, out = _proj_fwd(c, None, flag=True)
    assert code == 0, _lib.lib().tgt_last_error()
    assert torch.equal(out.view(torch.int16), c['out'].view(torch.int16))


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_flag_with_a_dropped_graph(dtype, variant):
    """graph_scale = [1.25, 0]: the dropped graph gets zero O rows (and nothing else happens for it), the other graph is the
    plain run's, bit for bit"""
    for shape in SHAPES[:2]:
        c = _case(shape, dtype, variant)
        sc = torch.tensor([1.25, 0.0], dtype=torch.float32, device='cuda')
        code, out = _proj_fwd(c, None, flag=True, graph_scale=sc)
        assert code == 0
        oc = c['ocols']
        assert torch.equal(out[1][..., oc].view(torch.int16), torch.zeros_like(out[1][..., oc]).view(torch.int16))
        assert torch.equal(out[0].view(torch.int16), c['out'][0].view(torch.int16))
        assert float(c['out'][1][..., oc].float().abs().max()) > 0


# ----------------------------------------------------------------------------------------------------------------- module level
class _Spy:
    """records what every ops._tri_args call was given: (the Q/K/V tensor or None, the flags of the argument block)"""

    def __init__(self, monkeypatch):
        from tgt_amd import ops
        self.calls = []
        real = ops._tri_args

        def spy(fused, *args, **kw):
            a = real(fused, *args, **kw)
            self.calls.append((fused, int(a.flags)))
            return a
        monkeypatch.setattr(ops, '_tri_args', spy)

    def no_store(self):
        from tgt_amd import _lib
        return [bool(f & _lib.TRI_NO_QKV_STORE) for _, f in self.calls]


def _module(B, N, nn_, H=16, dtype=torch.bfloat16, seed=5):
    from tgt_amd.tgt.layers.triplet import TripletAttention
    m = gu.fill_params(TripletAttention(CW, H), seed=seed).cuda().to(dtype).eval()
    rng = np.random.default_rng(seed + 1)
    e = rnd(rng, B, N, N, CW).to(dtype).cuda()
    mask = gu.additive_mask(list(nn_), N, torch.float32).cuda()
    return m, e, mask


@pytest.fixture
def small_rows(monkeypatch):
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_TRI_PROJ', True)
    monkeypatch.setattr(ops, '_TRI_PROJ_INFER', True)
    monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 1)            # (the projection-fused kernel also below 65536 edge rows)


def test_module_no_grad_equals_grad_enabled(small_rows, monkeypatch):
    m, e, mask = _module(2, 32, (32, 20))
    spy = _Spy(monkeypatch)
    y_grad = m(e, mask)
    assert y_grad.requires_grad
    with torch.no_grad():
        y_infer = m(e, mask)
    for p in m.parameters():
        p.requires_grad_(False)
    y_frozen = m(e, mask)                                     # grad mode on, nothing requires grad: no backward either
    torch.cuda.synchronize()
    assert spy.no_store() == [False, True, True]
    assert spy.calls[0][0] is not None and spy.calls[1][0] is None and spy.calls[2][0] is None
    assert not y_infer.requires_grad and not y_frozen.requires_grad
    assert torch.equal(y_infer, y_grad.detach()) and torch.equal(y_frozen, y_grad.detach())


def _peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del y
    return rise


def test_no_grad_forward_does_not_allocate_qkv(small_rows):
    """the Q/K/V tensor (B N^2 6C 2 bytes = 12.6 MB at B = 4, N = 32) is the only thing the inference path removes: the peak of
    the no_grad call stays below its size, the grad-enabled call's does not"""
    B, N = 4, 32
    m, e, mask = _module(B, N, (32, 20, 32, 9))
    qkv_bytes = B * N * N * 6 * CW * 2

    def infer():
        with torch.no_grad():
            return m(e, mask)
    infer()                                                   # warm the allocator (and the mask / index memos)
    m(e, mask)
    rise_infer, rise_grad = _peak_rise(infer), _peak_rise(lambda: m(e, mask))
    print(f'peak rise: no_grad {rise_infer} bytes, grad enabled {rise_grad} bytes, Q/K/V tensor {qkv_bytes} bytes')
    assert rise_infer < qkv_bytes, (rise_infer, qkv_bytes)
    assert rise_grad > qkv_bytes, (rise_grad, qkv_bytes)


@pytest.mark.parametrize('dtype', DTYPES)
def test_knob_off_writes_qkv_as_before(dtype, small_rows, monkeypatch):
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_TRI_PROJ_INFER', False)
    c = _case(SHAPES[1], dtype, 'gated')                      # (H = 16: a layout ops.py can express)
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        out = ops.projected_triplet_attention(c['x'], c['w'], c['b'], c['mask3'], c['L'])
    torch.cuda.synchronize()
    assert spy.no_store() == [False]
    fused = spy.calls[0][0]
    assert fused is not None and fused.shape == (c['B'], c['N'], c['N'], 6 * CW)
    assert torch.equal(fused.view(torch.int16), c['qkv'].view(torch.int16))      # allocated AND filled: the plain run's rows
    assert torch.equal(out.view(torch.int16), c['out'].view(torch.int16))
    B, N = 4, 32
    m, e, mask = _module(B, N, (32, 20, 32, 9))

    def infer():
        with torch.no_grad():
            return m(e, mask)
    infer()
    assert _peak_rise(infer) > B * N * N * 6 * CW * 2


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_training_branch_still_matches_the_oracle(dtype, variant, small_rows, monkeypatch):
    """grad enabled: the path with the Q/K/V rows, forward and backward against the float64 oracle (as
    tests/test_hip_ops.py::test_projection_fused_triplet_attention_vs_oracle, at this file's first geometry -- B = 2, N = 32,
    one ragged graph -- with H = 16: the backward writes every channel of the row only for a layout with D = C / H)"""
    from tgt_amd import ops, layout
    B, N, nn_, H = SHAPES[0][:3] + (16,)
    gated, biased = variant == 'gated', variant != 'axial'
    L = ops.TripletLayout(CW, H, gated=gated, biased=biased)
    assert ops._proj_fused_ok(torch.empty(B, N, N, CW), N, L, dtype), 'shape must be one the projection-fused kernel takes'
    rng = np.random.default_rng(23 + VARIANTS.index(variant))
    x = rnd(rng, B, N, N, CW).to(dtype)
    w = (rnd(rng, L.width, CW) * CW ** -0.5).to(dtype)
    b = (rnd(rng, L.width) * 0.1).to(dtype)
    d_out = rnd(rng, B, N, N, 2 * CW).to(dtype)
    mask = gu.additive_mask(list(nn_), N, torch.float32)

    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    f64 = torch.nn.functional.linear(x64, w64, b64)
    idx, oidx = layout.head_major_index(CW, H), layout.va_cols_head_major(CW, H)

    def to_ref(t):
        o = torch.empty_like(t)
        o[..., idx] = t
        return o

    def blk(lo):
        return torch.cat([to_ref(f64[..., lo + p * CW: lo + (p + 1) * CW]) for p in range(3)], -1)
    nb = (2 if gated else 1) * H
    eg_in = f64[..., 6 * CW: 6 * CW + nb] if biased else None
    eg_out = f64[..., 6 * CW + nb: 6 * CW + 2 * nb] if biased else None
    va_ref = core.triplet_attention_core(blk(0), eg_in, blk(3 * CW), eg_out, mask.double(), H, gated, biased)[..., oidx]
    (va_ref * d_out.double()).sum().backward()

    spy = _Spy(monkeypatch)
    xin, win, bin_ = (t.cuda().requires_grad_(True) for t in (x, w, b))
    va = ops.projected_triplet_attention(xin, win, bin_, mask.reshape(B, N, N).cuda(), L)
    va.backward(d_out.cuda())
    torch.cuda.synchronize()
    assert spy.no_store() == [False, False] and spy.calls[0][0] is not None      # (forward, backward: both on the Q/K/V rows)
    tol = TOL[dtype]
    figures = dict(fwd=rel(va, va_ref), dx=rel(xin.grad, x64.grad), dw=rel(win.grad[:L.used], w64.grad[:L.used]),
                   db=rel(bin_.grad[:L.used], b64.grad[:L.used]))
    print(dtype, variant, figures)
    assert torch.isfinite(va).all()
    assert figures['fwd'] < tol, figures
    assert figures['dx'] < 2 * tol and figures['dw'] < 2 * tol and figures['db'] < 2 * tol, figures


def test_graphed_forward_replays_the_inference_path(small_rows, monkeypatch):
    """tgt_amd/pcqm/graphed.py on a 2-layer TGT-At at N = 20: capture and replay take the kernel without Q/K/V stores and the
    replay equals the eager no_grad forward bit for bit"""
    from tgt_amd.pcqm import TGT_Multi
    from tgt_amd.pcqm.graphed import GraphedForward
    cfg = dict(gu.FULL_AT_CFG, model_height=2)
    geom = dict(B=2, N=20, num_nodes=[20, 7])
    model = gu.fill_params(TGT_Multi(**cfg), seed=61).cuda().eval()
    b0 = {k: v.cuda() for k, v in gu.model_batch(geom, seed=62).items()}
    b1 = {k: v.cuda() for k, v in gu.model_batch(geom, seed=63).items()}
    spy = _Spy(monkeypatch)
    gf = GraphedForward(model, b0, autocast_dtype=torch.bfloat16, warmup=1)
    assert len(spy.no_store()) >= 2 * 2 and all(spy.no_store())      # (warm-up + capture) x 2 layers, all without Q/K/V
    for b in (b1, b0):
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            want = model(b)
        got = gf(b)
        torch.cuda.synchronize()
        assert all(torch.equal(g, w) for g, w in zip(got, want))
    assert all(spy.no_store())
