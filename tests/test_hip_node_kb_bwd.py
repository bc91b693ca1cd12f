"""Node attention backward for graphs padded to 65..128 nodes (csrc/node_attention_kb_bwd.hip: key-blocked, matrix-core tiles,
softmax statistics read from what the forward saved) against the float64 oracle, on the GPU.

Oracle and bars are those of tests/test_hip_ops.py::test_node_attention: oracle.core.egt_attention_core in float64 on the values as
the kernel sees them; rel-L2 8e-3 (bf16) / 1e-3 (fp16) on outputs, twice that on gradients."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_util as gu
from node_family_cases import family
from oracle import core

pytestmark = pytest.mark.gpu

TOL = {torch.bfloat16: 8e-3, torch.float16: 1e-3}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [  # B, N, num_nodes, W, H
    (1, 65, (65,), 64, 8),            # D = 8; one key past four blocks: a last chunk of one live key, a last query block of one live row
    (2, 80, (80, 71), 96, 8),         # D = 12; ragged batch, padded rows and keys inside a block
    (2, 96, (96, 33), 256, 16),       # D = 16, two head groups; graph 1: whole key chunks masked, whole query blocks padded
    (1, 72, (72,), 768, 64),          # BASELINE width, eight head groups, D = 12; the forward runs on the key-blocked kernel
    (1, 128, (128,), 128, 8),         # D = 16, the upper limit, every block full
]
FP16_CASES = [CASES[0], CASES[1], CASES[4]]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rnd(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape))


@functools.lru_cache(maxsize=None)
def reference(case, dtype, scale_degree, want_edges):
    """inputs (as the kernel sees them) and the oracle's outputs / gradients; computed once per combination, never modified"""
    B, N, nn_, W, H = case
    rng = np.random.default_rng(1000 * N + W + H)
    qkv, eg = rnd(rng, B, N, 3 * W).to(dtype), rnd(rng, B, N, N, 2 * H).to(dtype)
    d_v, d_h = rnd(rng, B, N, W).to(dtype), rnd(rng, B, N, N, H).to(dtype)
    mask = gu.additive_mask(list(nn_), N, torch.float32)
    q64, e64 = qkv.double().requires_grad_(True), eg.double().requires_grad_(True)
    v_ref, h_ref = core.egt_attention_core(q64, e64, mask.double(), H, scale_degree)
    loss = (v_ref * d_v.double()).sum()
    if want_edges:
        loss = loss + (h_ref * d_h.double()).sum()
    loss.backward()
    return dict(qkv=qkv, eg=eg, d_v=d_v, d_h=d_h, mask=mask.reshape(B, N, N), v=v_ref.detach(), h=h_ref.detach(), dq=q64.grad, de=e64.grad)


def run(case, dtype, scale_degree, want_edges, fn=None, expect=None):
    from tgt_amd import ops
    r = reference(case, dtype, scale_degree, want_edges)
    H = case[4]
    qx, ex = r['qkv'].cuda().requires_grad_(True), r['eg'].cuda().requires_grad_(True)
    m = r['mask'].cuda()
    fam = family(qx, ex, m, H)
    assert expect is None or fam == expect, (fam, expect)           # before anything is launched
    v, hh = (fn or ops.node_attention)(qx, ex, m, H, scale_degree, want_edges)
    loss = (v.float() * r['d_v'].cuda().float()).sum()
    if want_edges:
        loss = loss + (hh.float() * r['d_h'].cuda().float()).sum()
    loss.backward()
    torch.cuda.synchronize()
    return r, fam, v, hh, qx.grad, ex.grad


def check(case, dtype, scale_degree, want_edges, fn=None, expect=None):
    r, fam, v, hh, dq, de = run(case, dtype, scale_degree, want_edges, fn, expect)
    errs = {'vatt': rel(v, r['v']), 'dqkv': rel(dq, r['dq']), 'deg': rel(de, r['de'])}
    if want_edges:
        errs['hhat'] = rel(hh, r['h'])
    print(case, dtype, scale_degree, want_edges, 'family', fam, errs)
    assert torch.isfinite(v).all() and torch.isfinite(dq).all() and torch.isfinite(de).all()
    assert hh is None or torch.isfinite(hh).all()
    tol = TOL[dtype]
    assert errs['vatt'] < tol and errs.get('hhat', 0.0) < tol, errs
    assert errs['dqkv'] < 2 * tol and errs['deg'] < 2 * tol, errs
    return fam


@pytest.mark.parametrize('scale_degree,want_edges', [(True, True), (False, False)])
@pytest.mark.parametrize('case,dtype', [(c, torch.bfloat16) for c in CASES] + [(c, torch.float16) for c in FP16_CASES])
def test_parity(case, dtype, scale_degree, want_edges):
    from tgt_amd import _lib
    check(case, dtype, scale_degree, want_edges, expect=_lib.NODE_FAMILY_KB_BWD)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('case', [(2, 80, 256, 32), (1, 128, 128, 8)])
def test_arbitrary_mask_and_large_logits(case, dtype):
    """The construction of test_hip_ops.py::test_node_attention_arbitrary_mask_and_large_logits: scattered masked keys, the first key
    block masked for every third query, the first 64 keys (a whole key chunk) for every fifth, the last key always live, logits
    spread over +-20 with the later keys carrying the maximum"""
    from tgt_amd import _lib, ops
    B, N, W, H = case
    rng = np.random.default_rng(N + H)
    qkv = rnd(rng, B, N, 3 * W).to(dtype)
    eg = rnd(rng, B, N, N, 2 * H)
    eg[..., :H] *= 6.0
    eg[:, :, N // 2:, :H] += 12.0
    eg = eg.to(dtype)
    d_v, d_h = rnd(rng, B, N, W).to(dtype), rnd(rng, B, N, N, H).to(dtype)
    m = torch.zeros(B, N, N)
    m[torch.from_numpy(rng.random((B, N, N)) < 0.2)] = -float('inf')
    m[:, 1::3, :16] = -float('inf')
    m[:, 2::5, :64] = -float('inf')
    m[:, :, N - 1] = 0.0
    q64, e64 = qkv.double().requires_grad_(True), eg.double().requires_grad_(True)
    v_ref, h_ref = core.egt_attention_core(q64, e64, m.double().reshape(gu.additive_mask([N] * B, N, torch.float32).shape), H, True)
    ((v_ref * d_v.double()).sum() + (h_ref * d_h.double()).sum()).backward()
    qx, ex = qkv.cuda().requires_grad_(True), eg.cuda().requires_grad_(True)
    assert family(qx, ex, m.cuda(), H) == _lib.NODE_FAMILY_KB_BWD
    v, hh = ops.node_attention(qx, ex, m.cuda(), H, True, True)
    ((v.float() * d_v.cuda().float()).sum() + (hh.float() * d_h.cuda().float()).sum()).backward()
    errs = {'vatt': rel(v, v_ref), 'hhat': rel(hh, h_ref), 'dqkv': rel(qx.grad, q64.grad), 'deg': rel(ex.grad, e64.grad)}
    print(case, dtype, errs)
    assert torch.isfinite(v).all() and torch.isfinite(qx.grad).all() and torch.isfinite(ex.grad).all()
    tol = TOL[dtype]
    assert errs['vatt'] < tol and errs['hhat'] < tol, errs
    assert errs['dqkv'] < 2 * tol and errs['deg'] < 2 * tol, errs
    # a masked pair takes no part in the softmax or the gate: its dG is exactly 0 and its dE is the H_hat gradient alone
    dead = torch.isinf(m).cuda()
    assert (ex.grad[..., H:][dead] == 0).all()
    assert torch.equal(ex.grad[..., :H][dead], d_h.cuda()[dead])


def test_hhat_scale():
    from tgt_amd import ops
    B, N, nn_, W, H = 3, 80, [80, 66, 70], 128, 16
    dtype = torch.bfloat16
    rng = np.random.default_rng(3)
    qkv, eg = rnd(rng, B, N, 3 * W).to(dtype).cuda(), rnd(rng, B, N, N, 2 * H).to(dtype).cuda()
    gv, gh = rnd(rng, B, N, W).to(dtype).cuda(), rnd(rng, B, N, N, H).to(dtype).cuda()
    mask = gu.additive_mask(nn_, N, torch.float32).reshape(B, N, N).cuda()
    sc = torch.tensor([1.25, 0.0, 1.25], device='cuda')
    sc4 = sc.view(-1, 1, 1, 1)
    qa, ea = qkv.clone().requires_grad_(True), eg.clone().requires_grad_(True)
    va, ha = ops.node_attention(qa, ea, mask, H, True, True, hhat_scale=sc)
    torch.autograd.backward([va, ha], [gv, gh])
    qb, eb = qkv.clone().requires_grad_(True), eg.clone().requires_grad_(True)
    vb, hb = ops.node_attention(qb, eb, mask, H, True, True)
    torch.autograd.backward([vb, hb], [gv, (gh.float() * sc4).to(dtype)])       # (graph 1: a zero d_hhat -- the V_att path alone)
    torch.cuda.synchronize()
    tol = TOL[dtype]
    assert torch.equal(va, vb)
    assert rel(ha, hb.float() * sc4) < tol
    assert rel(qa.grad, qb.grad) < 2 * tol and rel(ea.grad, eb.grad) < 2 * tol
    assert torch.isfinite(ea.grad).all() and torch.isfinite(qa.grad).all()
    assert torch.equal(ea.grad[1, ..., :H], eb.grad[1, ..., :H])


def test_two_runs_are_bit_equal():
    _, _, _, _, dq1, de1 = run(CASES[1], torch.bfloat16, True, True)
    _, _, _, _, dq2, de2 = run(CASES[1], torch.bfloat16, True, True)
    assert torch.equal(dq1, dq2) and torch.equal(de1, de2)


def _switch_child():
    """(child process) the N = 80 case with the switch as the environment has it: family and errors as one JSON line"""
    r, fam, v, hh, dq, de = run(CASES[1], torch.bfloat16, True, True)
    print(json.dumps({'family': fam, 'vatt': rel(v, r['v']), 'hhat': rel(hh, r['h']), 'dqkv': rel(dq, r['dq']), 'deg': rel(de, r['de']),
                      'finite': bool(torch.isfinite(dq).all() and torch.isfinite(de).all())}))


def test_switch_restores_the_lane_per_head_backward():
    from tgt_amd import _lib
    check(CASES[1], torch.bfloat16, True, True, expect=_lib.NODE_FAMILY_KB_BWD)
    env = dict(os.environ, TGT_NODE_KB_BWD='0',
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, 'tests')] + [p for p in [os.environ.get('PYTHONPATH')] if p]))
    out = subprocess.run([sys.executable, '-c', 'import test_hip_node_kb_bwd as t; t._switch_child()'], env=env, cwd=ROOT, timeout=120,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0, out.stderr.decode(errors='replace')[-2000:]
    got = json.loads(out.stdout.decode().strip().splitlines()[-1])
    print(got)
    tol = TOL[torch.bfloat16]
    assert got['family'] == _lib.NODE_FAMILY_LANE and got['finite']
    assert got['vatt'] < tol and got['hhat'] < tol and got['dqkv'] < 2 * tol and got['deg'] < 2 * tol, got


def test_no_slow_path_notice_for_shapes_the_backward_takes(monkeypatch):
    from tgt_amd import ops
    seen = []
    monkeypatch.setattr(ops, '_slow_path_notice', lambda key, msg: seen.append(key))
    B, N, W, H = 4, 128, 256, 32                            # B N N = 65536: the threshold of the notice
    qkv = torch.zeros(B, N, 3 * W, dtype=torch.bfloat16, device='cuda')
    eg = torch.zeros(B, N, N, 2 * H, dtype=torch.bfloat16, device='cuda')
    mask = gu.additive_mask([N] * B, N, torch.float32).reshape(B, N, N).cuda()
    ops.node_attention(qkv, eg, mask, H, True, True)
    torch.cuda.synchronize()
    assert not [k for k in seen if k[0] == 'node_mfma'], seen


def test_dispatcher_layer():
    from tgt_amd import _lib, torch_ops
    torch_ops.build_op_library()
    t = torch_ops.load()
    check((1, 80, (71,), 256, 32), torch.bfloat16, True, True, fn=t.egt_attention, expect=_lib.NODE_FAMILY_KB_BWD)


def test_above_the_limit_is_unchanged():
    from tgt_amd import _lib
    check((1, 129, (129,), 64, 8), torch.bfloat16, True, True, expect=_lib.NODE_FAMILY_LANE)
