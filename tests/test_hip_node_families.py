"""Node attention: every kernel family against the float64 oracle, on hard inputs and on plain ones, on the GPU.

Cases, the family each must take and the two kinds of input: tests/node_family_cases.py.  The family is asserted on the real tensors,
forward and backward, before anything is launched.  Oracle: oracle.core.egt_attention_core / edge_update_core in float64 on the values
as stored.  Bars are the stated ones of tests/test_hip_ops.py -- rel-L2 2e-6 (fp32) / 8e-3 (bf16) / 1e-3 (fp16) on outputs, twice
that on gradients; the measured maxima are profiles/parity_errors_node_families.json."""
import functools

import pytest
import torch

import node_family_cases as nfc
import parity_log
from oracle import core

pytestmark = pytest.mark.gpu

TOL = parity_log.Tol({torch.float32: 2e-6, torch.bfloat16: 8e-3, torch.float16: 1e-3})
FLAGS = [(True, True), (False, False)]            # scale_degree, want_edges


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return parity_log.record(float((a - b).norm() / (b.norm() + 1e-30)))


def _params(kind):
    return [pytest.param(c, dt, id='-'.join(map(str, c.shape)) + '-' + str(dt).replace('torch.', ''))
            for c in nfc.CASES if kind in c.kinds for dt in c.dtypes]


@functools.lru_cache(maxsize=None)
def reference(shape, dtype, kind, scale_degree, want_edges):
    """inputs (as the kernel sees them) and the oracle's outputs / gradients; computed once per combination, never modified"""
    B, N, W, H = shape
    qkv, eg, d_v, d_h, mask = nfc.inputs(shape, dtype, kind)
    q64, e64 = qkv.double().requires_grad_(True), eg.double().requires_grad_(True)
    v_ref, h_ref = core.egt_attention_core(q64, e64, mask.double().unsqueeze(-1), H, scale_degree)
    loss = (v_ref * d_v.double()).sum()
    if want_edges:
        loss = loss + (h_ref * d_h.double()).sum()
    loss.backward()
    out = dict(qkv=qkv, eg=eg, d_v=d_v, d_h=d_h, mask=mask, v=v_ref.detach(), h=h_ref.detach(), dq=q64.grad, de=e64.grad)
    assert all(torch.isfinite(out[k]).all() for k in ('v', 'h', 'dq', 'de')), 'the oracle is not finite on these inputs'
    return out


def check(case, dtype, kind, scale_degree, want_edges):
    from tgt_amd import ops
    B, N, W, H = case.shape
    r = reference(case.shape, dtype, kind, scale_degree, want_edges)
    qx, ex = r['qkv'].cuda().requires_grad_(True), r['eg'].cuda().requires_grad_(True)
    m = r['mask'].cuda()
    got = (nfc.family(qx, ex, m, H, 0), nfc.family(qx, ex, m, H, 1))
    assert got == (nfc.family_id(case.fwd), nfc.family_id(case.bwd)), (case, got)           # before anything is launched
    v, hh = ops.node_attention(qx, ex, m, H, scale_degree, want_edges)
    loss = (v.float() * r['d_v'].cuda().float()).sum()
    if want_edges:
        loss = loss + (hh.float() * r['d_h'].cuda().float()).sum()
    loss.backward()
    torch.cuda.synchronize()
    dq, de = qx.grad, ex.grad
    tol = TOL[dtype]
    errs = {'vatt': rel(v, r['v']), 'dqkv': rel(dq, r['dq']), 'deg': rel(de, r['de'])}
    if want_edges:
        errs['hhat'] = rel(hh, r['h'])
    print(case.shape, dtype, kind, scale_degree, want_edges, case.fwd, case.bwd, errs)
    assert torch.isfinite(v).all() and torch.isfinite(dq).all() and torch.isfinite(de).all()
    assert hh is None or torch.isfinite(hh).all()
    assert errs['vatt'] < tol and errs.get('hhat', 0.0) < tol, errs
    assert errs['dqkv'] < 2 * tol and errs['deg'] < 2 * tol, errs
    return r, de


@pytest.mark.parametrize('scale_degree,want_edges', FLAGS)
@pytest.mark.parametrize('case,dtype', _params('hard'))
def test_hard_inputs(case, dtype, scale_degree, want_edges):
    """per-(query, key) -inf masks with whole leading key blocks masked, logits spread over +-20 with the maximum in the later keys"""
    r, de = check(case, dtype, 'hard', scale_degree, want_edges)
    # a masked pair takes no part in the softmax or the gate: its dG is exactly 0 and its dE is the H_hat gradient alone
    H = case.shape[3]
    dead = torch.isinf(r['mask']).cuda()
    assert (de[..., H:][dead] == 0).all()
    assert torch.equal(de[..., :H][dead], r['d_h'].cuda()[dead] if want_edges else torch.zeros_like(de[..., :H][dead]))


@pytest.mark.parametrize('scale_degree,want_edges', FLAGS)
@pytest.mark.parametrize('case,dtype', _params('plain'))
def test_plain_inputs(case, dtype, scale_degree, want_edges):
    """unit-normal inputs and the padding mask of golden_util.additive_mask, ragged where B = 2: the parity check of
    test_hip_ops.py::test_node_attention on the D / heads-per-lane / head-block instantiations its cases do not reach"""
    check(case, dtype, 'plain', scale_degree, want_edges)


@functools.lru_cache(maxsize=None)
def logits_reference(shape, dtype, qk_scale):
    B, N, W, H = shape
    qkv, eg, _, d_h, _ = nfc.inputs(shape, torch.float64, 'plain')
    qk, eb, d_h = (qkv[..., :2 * W] * qk_scale).to(dtype), eg[..., :H].to(dtype).contiguous(), d_h.to(dtype)
    q64, e64 = qk.double().requires_grad_(True), eb.double().requires_grad_(True)
    ref = core.edge_update_core(q64, e64, H)
    (ref * d_h.double()).sum().backward()
    return dict(qk=qk, eb=eb, d_h=d_h, out=ref.detach(), dq=q64.grad, de=e64.grad)


@pytest.mark.parametrize('qk_scale', [1.0, 4.0])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('shape', nfc.LOGITS_CASES, ids=lambda s: '-'.join(map(str, s)))
def test_edge_logits(shape, dtype, qk_scale):
    """ops.edge_logits (logits_only: no mask, no softmax, no V) against oracle.core.edge_update_core, forward and both gradients, at
    unit scale and with Q and K times 4 (only magnitude matters)"""
    from tgt_amd import ops
    H = shape[3]
    r = logits_reference(shape, dtype, qk_scale)
    qx, ex = r['qk'].cuda().requires_grad_(True), r['eb'].cuda().requires_grad_(True)
    lane = nfc.family_id('LANE')
    assert nfc.family(qx, ex, None, H, 0, logits_only=True) == lane and nfc.family(qx, ex, None, H, 1, logits_only=True) == lane
    out = ops.edge_logits(qx, ex, H)
    out.backward(r['d_h'].cuda())
    torch.cuda.synchronize()
    tol = TOL[dtype]
    errs = {'out': rel(out, r['out']), 'dqk': rel(qx.grad, r['dq']), 'de': rel(ex.grad, r['de'])}
    print(shape, dtype, qk_scale, errs)
    assert torch.isfinite(out).all() and torch.isfinite(qx.grad).all() and torch.isfinite(ex.grad).all()
    assert errs['out'] < tol, errs
    assert errs['dqk'] < 2 * tol and errs['de'] < 2 * tol, errs
