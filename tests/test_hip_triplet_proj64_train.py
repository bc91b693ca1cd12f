"""The TRAINING form of the projection-fused triplet attention forward for 33..64 nodes (tgt_triplet_attention_proj64_train_fwd,
csrc/triplet_attention_proj64.hip built with -DTGT_TRI_PROJ64_INST=2; taken by ops._ProjectedTripletAttention when a backward can
follow and TGT_TRI_PROJ64_TRAIN=1), on the GPU.  It is the inference kernel of tests/test_hip_triplet_proj64.py plus one store of
every projected Q, K and V value, so the shapes, inputs, oracle and bars are that file's: SHAPES64 (C = 256, H = 16, D = 16 are
fixed by the kernel), the forward TOL of tests/test_hip_ops.py against float64 and 2 * TOL between two HIP paths that are each
held to that oracle.

What is new is the Q/K/V tensor: every row below N written exactly once with the value the kernel itself consumed, nothing else
written, rows of dropped graphs and of padded units left alone, and a backward (tgt_triplet_attention_bwd, untouched) that reads
those rows and arrives at the oracle's gradients."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_util as gu
from test_hip_triplet_proj64 import (BF16, COUNTS, CW, DTYPES, H, SHAPES64, TOL, V_BIAS_SCALE, VARIANTS, _Launches, _build, _case, _cases,
                                     _err, _module, _oracle, _proj_fwd, rel, rnd)

pytestmark = pytest.mark.gpu

BLOCKS = ['Q_in', 'K_in', 'V_in', 'Q_out', 'K_out', 'V_out']             # column blocks of CW of the Q/K/V row (ops.TripletLayout)


def bits(t):
    return t.view(torch.int16)


def _pattern(n, flip=0):
    """n int16 values that are finite, NaN-free numbers in bf16 and in fp16 (sign and top exponent bit clear); flip: another
    pattern that differs from the first in EVERY element"""
    return (((torch.arange(n, device='cuda', dtype=torch.int32) * 31 + 7) & 0x3fff) ^ flip).to(torch.int16)


def _train_fwd(c, sl=None, graph_scale=None, counts=False, x=None, out=None, qkv=None):
    """one tgt_triplet_attention_proj64_train_fwd(_counts) call on NaN-filled out / qkv unless given: (return code, out, qkv).
    Arguments as test_hip_triplet_proj64._proj_fwd"""
    from tgt_amd import ops, _lib
    xs = c['x'] if x is None else x
    xs, eg, mask3 = (t if (sl is None or t is None) else t[sl].contiguous() for t in (xs, c['eg'], c['mask3']))
    B, N = xs.shape[0], c['N']
    if out is None:
        out = torch.full((B, N, N, 2 * CW), float('nan'), dtype=c['dtype'], device='cuda')
    if qkv is None:
        qkv = torch.full((B, N, N, 6 * CW), float('nan'), dtype=c['dtype'], device='cuda')
    a = ops._tri_args(qkv, mask3, out, c['L'], eg=eg, graph_scale=graph_scale)
    assert a.qkv[0] == qkv.data_ptr() and a.ld_qkv[0] == 6 * CW and not a.flags & _lib.TRI_NO_QKV_STORE
    args = (ops._ptr(xs), CW, ops._ptr(c['w']), ops._ptr(c['b']), ops._stream())
    if counts is False:
        code = _lib.lib().tgt_triplet_attention_proj64_train_fwd(C.byref(a), *args)
    else:
        code = _lib.lib().tgt_triplet_attention_proj64_train_fwd_counts(C.byref(a), ops._ptr(counts), *args)
    torch.cuda.synchronize()
    return code, out, qkv


_tcases = {}


def _tcase(shape, dtype, variant):
    """the inference test's case (inputs, oracle, the inference kernel's out) and the first training run on it: computed once,
    never modified"""
    key = (shape, dtype, variant)
    if key not in _tcases:
        c = _case(shape, dtype, variant)
        code, out, qkv = _train_fwd(c)
        assert code == 0, _err()
        _tcases[key] = dict(c, t_out=out, t_qkv=qkv)
    return _tcases[key]


# -------------------------------------------------------------------------------------------------------- 1: out, bit for bit
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES64)
def test_out_is_the_inference_kernels_bit_for_bit(shape, dtype, variant):
    c = _tcase(shape, dtype, variant)
    assert not torch.isnan(c['t_out']).any()
    assert torch.equal(bits(c['t_out']), bits(c['out']))


# --------------------------------------------------------------------------------------------------------- 2: the stored rows
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES64)
def test_stored_qkv_against_the_float64_projection_and_the_gemm(shape, dtype, variant):
    """every one of the six column blocks on its own as well as the whole tensor: a wrong block is a sixth of the norm"""
    c = _tcase(shape, dtype, variant)
    got = c['t_qkv']
    assert not torch.isnan(got).any()                          # every row of the NaN-filled tensor was written
    want = c['f64'][..., :6 * CW]
    gemm = torch.addmm(c['b'][:6 * CW], c['x'].view(-1, CW), c['w'][:6 * CW].t()).view_as(got)
    torch.cuda.synchronize()
    for name, lo in [('whole', None)] + [(n, i * CW) for i, n in enumerate(BLOCKS)]:
        sl = slice(None) if lo is None else slice(lo, lo + CW)
        e64, eg = rel(got[..., sl], want[..., sl]), rel(got[..., sl], gemm[..., sl])
        print(f'proj64 train Q/K/V {name}: {shape} {dtype} {variant}: vs float64 {e64:.3e} (bar {TOL[dtype]:.0e}), vs GEMM {eg:.3e} '
              f'(bar {2 * TOL[dtype]:.0e})')
        assert e64 < TOL[dtype], (name, e64)
        assert eg < 2 * TOL[dtype], (name, eg)


# ---------------------------------------------------------------------------------------- 3: every row written, nothing else
def _guarded(n, flip, dtype):
    """a view of n elements inside a patterned buffer with 4 KB of guard on either side, itself pre-filled with the pattern"""
    guard = 4096 // 2
    buf = _pattern(guard + n + guard, flip)
    return buf, buf[guard:guard + n].view(dtype), guard


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('shape', SHAPES64[:2], ids=['n33', 'n48'])
def test_every_row_is_written_and_nothing_outside(shape, variant):
    """qkv and out are views inside larger patterned buffers.  Two runs on two patterns that differ in every element: an element the
    kernel does not write differs between the runs, so equal results (and equal to the reference run's) mean that every element was
    written; the guards keep their pattern"""
    c = _tcase(shape, BF16, variant)
    B, N = c['B'], c['N']
    results = []
    for flip in (0, 0x1555):
        qbuf, qv, guard = _guarded(B * N * N * 6 * CW, flip, BF16)
        obuf, ov, _ = _guarded(B * N * N * 2 * CW, flip, BF16)
        q_before, o_before = qbuf.clone(), obuf.clone()
        code, out, qkv = _train_fwd(c, out=ov.view(B, N, N, 2 * CW), qkv=qv.view(B, N, N, 6 * CW))
        assert code == 0, _err()
        for buf, before in ((qbuf, q_before), (obuf, o_before)):
            assert torch.equal(buf[:guard], before[:guard]) and torch.equal(buf[-guard:], before[-guard:])
        results.append((out, qkv))
    assert not torch.equal(_pattern(64, 0), _pattern(64, 0x1555)) and bool((_pattern(4096, 0) != _pattern(4096, 0x1555)).all())
    for out, qkv in results:
        assert torch.equal(bits(qkv), bits(c['t_qkv']))
        assert torch.equal(bits(out), bits(c['t_out']))


# ------------------------------------------------------------------------------------------------------------- 4: large V bias
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('shape', SHAPES64[:2], ids=['n33', 'n48'])
def test_large_v_bias(shape, variant):
    """V bias at scale 4.0 as in the inference test (whose CPU leg shows that TOL is reachable there): a padding key with any weight
    fails `out` by orders of magnitude; the stored V rows are finite and still the float64 projection's"""
    B, N, nn_ = shape
    c = _build(B, N, gu.additive_mask(list(nn_), N, torch.float32), BF16, variant, 7900 + N + VARIANTS.index(variant),
               v_bias_scale=V_BIAS_SCALE)
    code, out, qkv = _train_fwd(c)
    assert code == 0 and not torch.isnan(out).any()
    err = rel(out, c['ref'])
    print(f'proj64 train large V bias vs oracle: {shape} {variant}: rel-L2 {err:.3e} (bar {TOL[BF16]:.0e})')
    assert err < TOL[BF16], err
    for lo in (2 * CW, 5 * CW):
        assert torch.isfinite(qkv[..., lo:lo + CW]).all()
        assert rel(qkv[..., lo:lo + CW], c['f64'][..., lo:lo + CW]) < TOL[BF16]
    code, ref_out = _proj_fwd(c)
    assert code == 0 and torch.equal(bits(out), bits(ref_out))


# ------------------------------------------------------------------------------------------------------- 5: autograd end to end
@pytest.fixture
def knob_on(monkeypatch):
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_TRI_PROJ', True)
    monkeypatch.setattr(ops, '_TRI_PROJ64_TRAIN', True)
    monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 1)            # (the fused kernels also below 65536 edge rows)


def _op_run(c, d_out, graph_scale=None, node_counts=None, x=None):
    """ops.projected_triplet_attention forward + backward on the case's (x, w, b): (out, [dx, dw, db])"""
    from tgt_amd import ops
    ins = [t.clone().requires_grad_(True) for t in (c['x'] if x is None else x, c['w'], c['b'])]
    out = ops.projected_triplet_attention(*ins, c['mask3'], c['L'], graph_scale=graph_scale, node_counts=node_counts)
    out.backward(d_out)
    torch.cuda.synchronize()
    return out.detach(), [t.grad for t in ins]


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES64[:2], ids=['n33', 'n48'])
def test_autograd_against_the_float64_oracle(shape, dtype, variant, knob_on, monkeypatch):
    """the scheme of tests/test_hip_ops.py::test_projection_fused_triplet_attention_vs_oracle: forward within TOL, dx / dw / db
    within 2 * TOL of the float64 oracle's; and all four within 2 * TOL of the run with the knob off"""
    from tgt_amd import ops
    c = _tcase(shape, dtype, variant)
    B, N, L = c['B'], c['N'], c['L']
    rng = np.random.default_rng(8100 + N + 10 * DTYPES.index(dtype) + VARIANTS.index(variant))
    d_out = rnd(rng, B, N, N, 2 * CW).to(dtype)
    x64, w64, b64 = (t.double().cpu().requires_grad_(True) for t in (c['x'], c['w'], c['b']))
    f64 = torch.nn.functional.linear(x64, w64, b64)
    ref = _oracle(f64, f64[..., 6 * CW:L.used] if L.biased else None, c['mask4'], L)
    (ref * d_out.double()).sum().backward()

    spy = _Launches(monkeypatch)
    out, grads = _op_run(c, d_out.cuda())
    assert spy.names == ['tgt_triplet_attention_proj64_train_fwd', 'tgt_triplet_attention_bwd'], spy.names
    assert torch.equal(bits(out), bits(c['t_out']))            # (the op's forward is the kernel's)
    monkeypatch.setattr(ops, '_TRI_PROJ64_TRAIN', False)
    spy.names.clear()
    out_off, grads_off = _op_run(c, d_out.cuda())
    assert spy.names == ['tgt_triplet_attention_fwd', 'tgt_triplet_attention_bwd'], spy.names
    tol = TOL[dtype]
    errs = [rel(out, ref.detach())] + [rel(g, r.grad) for g, r in zip(grads, (x64, w64, b64))]
    offs = [rel(out, out_off)] + [rel(g, o) for g, o in zip(grads, grads_off)]
    for i, name in enumerate(('fwd', 'dx', 'dw', 'db')):
        bar = tol if i == 0 else 2 * tol
        print(f'proj64 train autograd {name}: {shape} {dtype} {variant}: vs float64 {errs[i]:.3e} (bar {bar:.0e}), vs knob off '
              f'{offs[i]:.3e} (bar {2 * tol:.0e})')
    for i, name in enumerate(('fwd', 'dx', 'dw', 'db')):
        assert all(torch.isfinite(t).all() for t in [out] + grads)
        assert errs[i] < (tol if i == 0 else 2 * tol), (name, errs[i])
        assert offs[i] < 2 * tol, (name, offs[i])


# -------------------------------------------------------------------------------------------------------------- 6: dropped graphs
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_dropped_graphs_have_no_rows_and_no_gradient(dtype, variant, knob_on):
    for shape, factors in ((SHAPES64[0], (0.0, 1.25, 0.0)), (SHAPES64[1], (1.25, 0.0))):
        c = _tcase(shape, dtype, variant)
        B, N = c['B'], c['N']
        sc = torch.tensor(factors, dtype=torch.float32, device='cuda')
        dead = [b for b, f in enumerate(factors) if f == 0.0]
        live = [b for b, f in enumerate(factors) if f != 0.0]
        x_nan = c['x'].clone()
        x_nan[dead] = float('nan')
        for xs in (c['x'], x_nan):
            qkv = _pattern(B * N * N * 6 * CW).view(c['dtype']).view(B, N, N, 6 * CW)
            before = qkv.clone()
            code, out, qkv = _train_fwd(c, graph_scale=sc, x=xs, qkv=qkv)
            assert code == 0, _err()
            assert torch.equal(bits(out[dead]), bits(torch.zeros_like(out[dead])))
            assert torch.equal(bits(qkv[dead]), bits(before[dead]))           # not one Q/K/V row of a dropped graph
            assert torch.equal(bits(out[live]), bits(c['t_out'][live]))
            assert torch.equal(bits(qkv[live]), bits(c['t_qkv'][live]))
        assert float(c['t_out'][dead].float().abs().max()) > 0
        # through autograd (finite X: a weight gradient is a product with X): the dropped graphs get what arrives behind the
        # residual add's multiplication, zeros; the backward is given the factors and must not read their Q/K/V rows, which the
        # forward left as torch.empty made them
        rng = np.random.default_rng(8200 + N)
        alive = (sc != 0).view(B, 1, 1, 1).to(dtype)
        d_out = rnd(rng, B, N, N, 2 * CW).to(dtype).cuda() * alive
        out_full, grads_full = _op_run(c, d_out)
        out_skip, grads_skip = _op_run(c, d_out, graph_scale=sc)
        assert torch.equal(bits(out_skip[live]), bits(out_full[live])) and float(out_skip[dead].float().abs().max()) == 0
        for g, r in zip(grads_skip, grads_full):
            assert torch.isfinite(g).all()
            assert torch.equal(g, r), float((g.float() - r.float()).abs().max())
        assert float(grads_skip[0][dead].float().abs().max()) == 0 and float(grads_skip[0][live].float().abs().max()) > 0


# ----------------------------------------------------------------------------------------------------------------- 7: node counts
def _counts_case(dtype, variant):
    """N = 40, one graph per count of COUNTS, every mask fully open (the inference test's case) and its training run"""
    N, B = 40, len(COUNTS)
    key = ('counts', dtype, variant)
    if key not in _cases:
        c = _build(B, N, gu.additive_mask([N] * B, N, torch.float32), dtype, variant, 7800 + 10 * DTYPES.index(dtype) + VARIANTS.index(variant))
        code, c['out'] = _proj_fwd(c)
        assert code == 0
        _cases[key] = c
    if key not in _tcases:
        c = _cases[key]
        code, out, qkv = _train_fwd(c)
        assert code == 0, _err()
        _tcases[key] = dict(c, t_out=out, t_qkv=qkv)
    return _tcases[key]


def _written(N):
    """(len(COUNTS), N, N, 6 CW) bool: the Q/K/V elements of the units j < n -- rows [:, j] (Q, and K / V outward) and [j, :]
    (K / V inward)"""
    m = torch.zeros(len(COUNTS), N, N, 6 * CW, dtype=torch.bool, device='cuda')
    for b, n in enumerate(COUNTS):
        n = min(n, N)
        m[b, :, :n, :CW] = True
        m[b, :n, :, CW:3 * CW] = True
        m[b, :, :n, 3 * CW:] = True
    return m


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_node_counts(dtype, variant):
    c = _counts_case(dtype, variant)
    N, B = c['N'], c['B']
    assert torch.equal(bits(c['t_out']), bits(c['out'])) and not torch.isnan(c['t_qkv']).any()
    counts = torch.tensor(COUNTS, dtype=torch.int32, device='cuda')
    written = _written(N)
    x_nan = c['x'].clone()                                      # NaN in the X rows of every unit j >= n, as the inference test
    for b, n in enumerate(COUNTS):
        x_nan[b, :, n:] = float('nan')
        x_nan[b, n:, :] = float('nan')
    for xs in (c['x'], x_nan):
        qkv = _pattern(B * N * N * 6 * CW).view(dtype).view(B, N, N, 6 * CW)
        before = qkv.clone()
        code, out, qkv = _train_fwd(c, counts=counts, x=xs, qkv=qkv)
        assert code == 0, _err()
        # the rows of the units j >= n are untouched, whatever their X rows hold
        assert torch.equal(bits(qkv)[~written], bits(before)[~written])
        for b, n in enumerate(COUNTS):
            n = min(n, N)
            assert torch.equal(bits(out[b, :, n:]), bits(torch.zeros_like(out[b, :, n:])))
        if xs is c['x']:
            # ... and everything with j < n is the call without counts, bit for bit
            assert torch.equal(bits(qkv)[written], bits(c['t_qkv'])[written])
            for b, n in enumerate(COUNTS):
                n = min(n, N)
                assert torch.equal(bits(out[b, :, :n]), bits(c['t_out'][b, :, :n]))
        # (x_nan: keys ARE read up to N, so rows (j, k >= n) of a real unit are NaN there -- only the untouched part is compared)
    code, out, qkv = _train_fwd(c, counts=None)
    assert code == 0 and torch.equal(bits(out), bits(c['t_out'])) and torch.equal(bits(qkv), bits(c['t_qkv']))


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_node_counts_gradients(dtype, variant, knob_on, monkeypatch):
    """through ops with the knob on, masks that close the padded nodes (what the model gives) and a cotangent that is zero at the
    padded columns: out[:, j < n] and every gradient are those of the run without counts, bit for bit -- the backward gets the
    same counts and does not read the rows the forward did not write"""
    N, B = 40, len(COUNTS)
    key = ('counts-grad', dtype, variant)
    if key not in _cases:
        _cases[key] = _build(B, N, gu.additive_mask([min(n, N) for n in COUNTS], N, torch.float32), dtype, variant,
                             8300 + 10 * DTYPES.index(dtype) + VARIANTS.index(variant))
    c = _cases[key]
    counts = torch.tensor(COUNTS, dtype=torch.int32, device='cuda')
    rng = np.random.default_rng(8350)
    cols = (torch.arange(N)[None, :] < torch.tensor(COUNTS)[:, None]).view(B, 1, N, 1).to(dtype).cuda()
    d_out = rnd(rng, B, N, N, 2 * CW).to(dtype).cuda() * cols
    spy = _Launches(monkeypatch)
    out_ref, grads_ref = _op_run(c, d_out)
    out, grads = _op_run(c, d_out, node_counts=counts)
    assert spy.names == ['tgt_triplet_attention_proj64_train_fwd', 'tgt_triplet_attention_bwd',
                         'tgt_triplet_attention_proj64_train_fwd_counts', 'tgt_triplet_attention_bwd_counts'], spy.names
    for b, n in enumerate(COUNTS):
        n = min(n, N)
        assert torch.equal(bits(out[b, :, :n]), bits(out_ref[b, :, :n])) and float(out[b, :, n:].float().abs().sum()) == 0
    for k, (g, r) in enumerate(zip(grads, grads_ref)):
        assert torch.isfinite(g).all(), k
        assert torch.equal(g, r), (k, float((g.float() - r.float()).abs().max()))


# ------------------------------------------------------------------------------------------------------------------- 8: knob off
def _unfused_forward(c):
    """the forward of the commit before this kernel, by hand: the library GEMMs of ops._ProjectedTripletAttention's split branch
    (biased layouts) or its one GEMM (axial), then tgt_triplet_attention_fwd"""
    from tgt_amd import ops, _lib
    B, N, L = c['B'], c['N'], c['L']
    x2 = c['x'].view(-1, CW)
    out = torch.empty(B, N, N, 2 * CW, dtype=c['dtype'], device='cuda')
    if L.biased:
        fused = torch.addmm(c['b'][:6 * CW], x2, c['w'][:6 * CW].t()).view(B, N, N, 6 * CW)
        eg = ops._narrow_linear(x2, c['w'][6 * CW:L.used], c['b'][6 * CW:L.used], c['dtype']).view(B, N, N, L.used - 6 * CW)
        a = ops._tri_args(fused, c['mask3'], out, L, eg=eg)
    else:
        _, _, fused = ops._linear_forward(c['x'], c['w'], c['b'], c['dtype'])
        a = ops._tri_args(fused, c['mask3'], out, L)
    _lib.check(_lib.lib().tgt_triplet_attention_fwd(C.byref(a), ops._stream()), 'tgt_triplet_attention_fwd')
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('variant', VARIANTS)
def test_knob_off_is_the_unfused_path(variant, monkeypatch):
    from tgt_amd import knobs, ops
    assert knobs._SPEC['tri_proj64_train'][1] is False          # ships off
    monkeypatch.setattr(ops, '_TRI_PROJ', True)
    monkeypatch.setattr(ops, '_TRI_PROJ64_INFER', True)
    monkeypatch.setattr(ops, '_TRI_PROJ64_TRAIN', False)
    monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 1)
    c = _tcase(SHAPES64[1], BF16, variant)
    spy = _Launches(monkeypatch)
    ins = [t.clone().requires_grad_(True) for t in (c['x'], c['w'], c['b'])]
    out = ops.projected_triplet_attention(*ins, c['mask3'], c['L'])
    assert out.requires_grad and spy.names == ['tgt_triplet_attention_fwd']
    assert torch.equal(bits(out.detach()), bits(_unfused_forward(c)))


@pytest.mark.parametrize('cls_name', ['TripletAttention', 'TripletAttentionUngated', 'AxialAttention'])
def test_module_paths_with_the_knob_on_and_off(cls_name, knob_on, monkeypatch):
    """the grad-enabled N = 48 module forward: knob off, the launch and the bits it has without the feature; knob on, the new entry
    point, within 2 * TOL of it; a call without a backward keeps the inference kernel; N = 32 and N = 72 keep their paths"""
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_TRI_PROJ_INFER', True)
    monkeypatch.setattr(ops, '_TRI_PROJ64_INFER', True)
    m, e, mask = _module(cls_name, 2, 48, (48, 35))
    spy = _Launches(monkeypatch)
    monkeypatch.setattr(ops, '_TRI_PROJ64_TRAIN', False)
    y_off = m(e, mask)
    assert spy.names == ['tgt_triplet_attention_fwd']
    spy.names.clear()
    y_off2 = m(e, mask)
    assert torch.equal(y_off, y_off2)
    monkeypatch.setattr(ops, '_TRI_PROJ64_TRAIN', True)
    spy.names.clear()
    y_on = m(e, mask)
    assert y_on.requires_grad and spy.names == ['tgt_triplet_attention_proj64_train_fwd']
    y_on.float().square().sum().backward()
    torch.cuda.synchronize()
    assert spy.names == ['tgt_triplet_attention_proj64_train_fwd', 'tgt_triplet_attention_bwd']
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    err = rel(y_on, y_off)
    print(f'{cls_name}: N = 48 grad enabled, knob on vs off: rel-L2 {err:.3e} (bar {2 * TOL[BF16]:.1e})')
    assert torch.isfinite(y_on).all() and err < 2 * TOL[BF16], err
    spy.names.clear()
    with torch.no_grad():
        m(e, mask)
    assert spy.names == ['tgt_triplet_attention_proj64_fwd']     # (no backward: the inference kernel keeps priority)
    monkeypatch.setattr(ops, '_TRI_PROJ64_INFER', False)
    spy.names.clear()
    with torch.no_grad():
        y_plain = m(e, mask)
    assert spy.names == ['tgt_triplet_attention_fwd'] and torch.equal(y_plain, y_off.detach())      # (... and the storing form is for calls a backward can follow only)
    monkeypatch.setattr(ops, '_TRI_PROJ64_INFER', True)
    for N, nn_, want in ((32, (32, 20), ['tgt_triplet_attention_proj_fwd']), (72, (72, 50), ['tgt_triplet_attention_fwd'])):
        m2, e2, mask2 = _module(cls_name, 2, N, nn_)
        spy.names.clear()
        assert m2(e2, mask2).requires_grad
        assert spy.names == want, (N, spy.names)


def test_the_slow_path_notice_does_not_fire(knob_on, recwarn):
    from tgt_amd import ops
    c = _tcase(SHAPES64[1], BF16, 'gated')
    said = set(ops._slow_path_said)
    ops._slow_path_said.discard(('tri_proj', 'N > 32'))
    try:
        ins = [t.clone().requires_grad_(True) for t in (c['x'], c['w'], c['b'])]
        ops.projected_triplet_attention(*ins, c['mask3'], c['L'])
        torch.cuda.synchronize()
        assert ('tri_proj', 'N > 32') not in ops._slow_path_said
        assert not [w for w in recwarn.list if 'projection-fused forward' in str(w.message)]
    finally:
        ops._slow_path_said.clear()
        ops._slow_path_said.update(said)


# ------------------------------------------------------------------------------------------------------------ 9: bit-equal repeats
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_bit_equal_runs_and_graph_indexing(dtype, variant):
    for shape in SHAPES64:
        c = _tcase(shape, dtype, variant)
        code, out, qkv = _train_fwd(c)
        assert code == 0 and torch.equal(bits(out), bits(c['t_out'])) and torch.equal(bits(qkv), bits(c['t_qkv']))
    c = _tcase(SHAPES64[0], dtype, variant)
    code, out, qkv = _train_fwd(c, sl=slice(0, 1))             # graph 0 of the B = 3 case, run alone with B = 1
    assert code == 0 and torch.equal(bits(out[0]), bits(c['t_out'][0])) and torch.equal(bits(qkv[0]), bits(c['t_qkv'][0]))


# ----------------------------------------------------------------------------------------------------------------- 10: model level
def test_model_step_with_the_knob_on_and_off(knob_on, monkeypatch):
    """TGT_Multi, 2 layers, N = 40, bf16 autocast, no dropout of any kind: forward + loss + backward with the knob on and off.  The
    loss within 2e-2 of the knob-off one (tests/test_hip_model.py's bar on the forward outputs of two HIP wirings of the same model,
    test_drop_path_folded_into_producers_matches_the_plain_wiring), every parameter gradient finite"""
    from tgt_amd import ops
    from tgt_amd.pcqm import TGT_Multi
    from tgt_amd.training.step import pretrain_loss, StepConfig
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)
    cfg = dict(gu.MODEL_CASES['multi_at_tiny'][1], model_height=2, node_width=64, edge_width=256, num_heads=4, triplet_heads=16,
               triplet_dropout=0, source_dropout=0., drop_path=0., node_act_dropout=0., edge_act_dropout=0.)
    geom = dict(B=2, N=40, num_nodes=[40, 23])
    batch = {k: v.cuda() for k, v in gu.model_batch(geom, seed=72).items()}
    scfg = StepConfig(num_dist_bins=cfg['num_dist_bins'], mixed_precision=None)
    spy = _Launches(monkeypatch)
    losses = {}
    for on in (False, True):
        monkeypatch.setattr(ops, '_TRI_PROJ64_TRAIN', on)
        model = gu.fill_params(TGT_Multi(**cfg), seed=71).cuda().train()
        torch.manual_seed(5)
        ops.reset_random_pools()
        spy.names.clear()
        with torch.autocast('cuda', dtype=torch.bfloat16):
            loss = pretrain_loss(model(batch), batch, scfg)
        loss.backward()
        torch.cuda.synchronize()
        fwd = 'tgt_triplet_attention_proj64_train_fwd' if on else 'tgt_triplet_attention_fwd'
        assert spy.names == 2 * [fwd] + 2 * ['tgt_triplet_attention_bwd'], spy.names
        assert torch.isfinite(loss)
        for k, p in model.named_parameters():
            assert p.grad is None or torch.isfinite(p.grad).all(), k
        assert sum(p.grad is not None for p in model.parameters()) > 0
        losses[on] = float(loss.detach())
    diff = abs(losses[True] - losses[False]) / abs(losses[False])
    print(f'2-layer TGT_Multi, N = 40, bf16: loss knob off {losses[False]:.6f}, on {losses[True]:.6f}, relative difference {diff:.3e} (bar 2e-2)')
    assert diff < 2e-2, diff
