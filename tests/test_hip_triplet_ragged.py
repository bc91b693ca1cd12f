"""Per-graph node counts of the triplet ATTENTION kernels (tgt_triplet_attention_fwd_counts / _bwd_counts / _proj_fwd_counts,
tgt_mask_node_counts), on the GPU: the walk over the shared node j ends at the graph's own n, and because every key past n is
closed by the mask (weight exactly 0) and the cotangent of a padded column is zero, the real block of the output and ALL
gradients are compared with torch.equal against the same op called without counts -- no tolerance.

Which kernel a case takes (csrc/triplet_attention.hip: triplet_attention_run and the eligibility predicates next to it):
  gen16 / gen8 / gen32   fp32, N <= 32, H = 4: tri_att_fwd_kernel / tri_att_bwd_kernel, HG = 4, NT = 1, D = 16 / 8 / 32
  bwd2                   16-bit, C = 128, H = 8, N = 20: tri_att_fwd_kernel HG = 8; backward tri_att_bwd2_kernel (LDS-DMA form;
                         the register-prefetch form needs TGT_TRI_BWD2_DMA=0 at library load: the child-process test below)
  proj                   16-bit, C = 256, H = 16, N = 20 through projected_triplet_attention: tri_att_proj_fwd_kernel (STORE = true
                         with autograd, STORE = false under no_grad), backward tri_att_bwd2_kernel with column sums
  t16                    16-bit, N = 40 / 48, H = 4: tri_att16_fwd_kernel / tri_att16_bwd_kernel <HG 4, NQ 3>; N = 52: <4, 4> forward,
                         <2, 4> backward; fp32 at N = 40: the two-tile generic kernels (NT = 2)
  kb                     N = 72: the key-blocked kernels, which accept the counts and ignore them
Counts: one inside, one on and one past a 16- and 32-wide tile edge at N = 40 / 48; a full, a one-node and an empty graph."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_util as gu
from oracle import core

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-6, torch.bfloat16: 8e-3, torch.float16: 1e-3}      # tests/test_hip_ops.py: forward, rel-L2 against float64
COUNTS = {12: [12, 1, 0, 7], 20: [20, 11, 1], 40: [40, 17, 33, 0], 48: [48, 17, 33, 0], 52: [52, 49, 17, 0], 72: [72, 40]}
BIG = 8192.0                                                                 # finite and exact in every dtype; what padded d_out columns are filled with
VARIANTS = ['gated', 'ungated', 'axial']
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16

# name -> (kind, N, C, H, dtypes, variants)
FAMILIES = {
    'gen16': ('plain', 12, 64, 4, [F32], VARIANTS),
    'gen8': ('plain', 12, 32, 4, [F32], ['gated']),
    'gen32': ('plain', 20, 128, 4, [F32], ['gated']),
    'bwd2': ('plain', 20, 128, 8, [BF16, F16], VARIANTS),
    'bwd2_colsum': ('proj', 20, 128, 8, [BF16, F16], VARIANTS),
    'proj': ('proj', 20, 256, 16, [BF16, F16], VARIANTS),
    't16_40': ('plain', 40, 64, 4, [F32, BF16, F16], ['gated']),
    't16_48': ('plain', 48, 64, 4, [BF16, F16], ['gated', 'axial']),
    't16_48_colsum': ('proj', 48, 64, 4, [BF16], ['gated']),
    't16_52': ('plain', 52, 64, 4, [BF16], ['gated']),
}
CASES = [(f, dt, v) for f, (_, _, _, _, dts, vs) in FAMILIES.items() for dt in dts for v in vs]
IDS = [f'{f}-{str(dt)[6:]}-{v}' for f, dt, v in CASES]


def rnd(rng, *shape, scale=1.0):
    return torch.from_numpy(rng.standard_normal(shape) * scale)


def to_ref(x_hm, idx):
    out = torch.empty_like(x_hm)
    out[..., idx] = x_hm
    return out


@pytest.fixture(autouse=True)
def small_rows(monkeypatch):
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_TRI_PROJ', True)
    monkeypatch.setattr(ops, '_TRI_PROJ_INFER', True)
    monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 1)            # (the projection-fused kernel also below 65536 edge rows)


def col_mask(counts, N, dtype):
    """(B,1,N,1): 1 at the real columns j < n of every graph"""
    return (torch.arange(N)[None, :] < torch.tensor(counts)[:, None]).view(len(counts), 1, N, 1).to(dtype).cuda()


def real_mask(counts, N):
    nm = torch.arange(N)[None, :] < torch.tensor(counts)[:, None]
    return (nm[:, :, None] & nm[:, None, :]).unsqueeze(-1).cuda()


def run(c, node_counts, d_out, dropout=(0.0, 0), graph_scale=None, grad=True):
    """one forward (+ backward) of the case's op: (out, [gradients of its inputs])"""
    from tgt_amd import ops
    ins = [t.clone().requires_grad_(grad) for t in c['inputs']]
    if c['kind'] == 'plain':
        out = ops.triplet_attention(ins[0], c['mask3'], c['L'], dropout, graph_scale, node_counts)
    else:
        out = ops.projected_triplet_attention(*ins, c['mask3'], c['L'], dropout=dropout, graph_scale=graph_scale, node_counts=node_counts)
    if grad:
        out.backward(d_out)
    torch.cuda.synchronize()
    return out.detach(), [t.grad for t in ins]


_cases = {}


def make_case(family, dtype, variant, dropout=(0.0, 0)):
    """inputs on the device, the counts, the cotangent (zero at the padded columns) and R = the op WITHOUT counts: computed once,
    never modified"""
    key = (family, dtype, variant, dropout)
    if key in _cases:
        return _cases[key]
    from tgt_amd import ops
    kind, N, C, H = FAMILIES[family][:4]
    counts = COUNTS[N]
    B = len(counts)
    L = ops.TripletLayout(C, H, gated=variant == 'gated', biased=variant != 'axial')
    rng = np.random.default_rng(1000 * list(FAMILIES).index(family) + 10 * VARIANTS.index(variant) + [F32, BF16, F16].index(dtype))
    if kind == 'plain':
        inputs = [rnd(rng, B, N, N, L.width).to(dtype).cuda()]
    else:
        w = (rnd(rng, L.width, C) * C ** -0.5).to(dtype)
        b = (rnd(rng, L.width) * 0.1).to(dtype)
        w[L.used:] = 0
        b[L.used:] = 0
        inputs = [rnd(rng, B, N, N, C).to(dtype).cuda(), w.cuda(), b.cuda()]
    c = dict(kind=kind, N=N, C=C, H=H, B=B, L=L, counts=counts, dtype=dtype, variant=variant, inputs=inputs, dropout=dropout,
             mask3=gu.additive_mask(counts, N, torch.float32).reshape(B, N, N).cuda(),
             nc=torch.tensor(counts, dtype=torch.int32, device='cuda'),
             d_out=rnd(rng, B, N, N, 2 * C).to(dtype).cuda() * col_mask(counts, N, dtype))
    c['R'] = run(c, None, c['d_out'], dropout)
    _cases[key] = c
    return c


def check_against_reference(c, out, grads, what):
    """items 1, 2, 4 of the contract: real block equal, padded columns exactly zero, every gradient equal"""
    R_out, R_grads = c['R']
    for b, n in enumerate(c['counts']):
        assert torch.equal(out[b, :n, :n], R_out[b, :n, :n]), (what, 'real block', b, n)
        assert float(out[b, :, n:].float().abs().sum()) == 0, (what, 'padded columns', b, n)
        assert torch.isfinite(out[b, :, :n]).all(), (what, 'finite', b, n)
    for k, (g, r) in enumerate(zip(grads, R_grads)):
        assert torch.isfinite(g).all(), (what, 'gradient finite', k)
        assert torch.equal(g, r), (what, 'gradient', k, float((g.float() - r.float()).abs().max()))


def oracle_out(c):
    """float64 oracle of the case's forward in the kernels' channel order (tests/test_hip_ops.py::test_triplet_attention /
    ::test_projection_fused_triplet_attention_vs_oracle)"""
    from tgt_amd import layout
    C, H, L = c['C'], c['H'], c['L']
    gated, biased = c['variant'] == 'gated', c['variant'] != 'axial'
    ins = [t.double().cpu() for t in c['inputs']]
    f64 = ins[0] if c['kind'] == 'plain' else torch.nn.functional.linear(*ins)
    idx, oidx = layout.head_major_index(C, H), layout.va_cols_head_major(C, H)

    def blk(lo):
        return torch.cat([to_ref(f64[..., lo + p * C: lo + (p + 1) * C], idx) for p in range(3)], -1)
    nb = (2 if gated else 1) * H
    eg_in = f64[..., 6 * C: 6 * C + nb] if biased else None
    eg_out = f64[..., 6 * C + nb: 6 * C + 2 * nb] if biased else None
    mask = gu.additive_mask(c['counts'], c['N'], torch.float64)
    return core.triplet_attention_core(blk(0), eg_in, blk(3 * C), eg_out, mask, H, gated, biased)[..., oidx]


@pytest.mark.parametrize('family,dtype,variant', CASES, ids=IDS)
def test_counts_skip_padded_nodes_bit_exactly(family, dtype, variant):
    """forward: real block equal to the run without counts, padded columns exactly zero, real block at the float64 oracle;
    backward: whole d_fused (projected: x.grad, weight and bias gradients -- the bias gradient IS the kernel's column sums) equal;
    the padded columns of d_out are not read: filled with a large constant, nothing moves; counts = N is the run without counts"""
    c = make_case(family, dtype, variant)
    out, grads = run(c, c['nc'], c['d_out'])
    check_against_reference(c, out, grads, 'counts')
    # 3. the real block against the oracle
    real = real_mask(c['counts'], c['N'])
    want = oracle_out(c) * real.cpu()
    got = (out * real).double().cpu()
    err = float((got - want).norm() / (want.norm() + 1e-30))
    print(family, dtype, variant, 'real block vs float64 oracle: rel-L2', err)
    assert err < TOL[dtype], err
    # 4. padded d_out columns are not read
    poisoned = torch.where(col_mask(c['counts'], c['N'], dtype).bool().expand_as(c['d_out']), c['d_out'], torch.full_like(c['d_out'], BIG))
    assert float((poisoned - c['d_out']).abs().max()) == BIG
    out_p, grads_p = run(c, c['nc'], poisoned)
    assert torch.equal(out_p, out)
    for k, (g, r) in enumerate(zip(grads_p, grads)):
        assert torch.equal(g, r), ('poisoned d_out moved gradient', k)
    # 7. counts = N: the run without counts, everywhere
    full = torch.full((c['B'],), c['N'], dtype=torch.int32, device='cuda')
    out_f, grads_f = run(c, full, c['d_out'])
    assert torch.equal(out_f, c['R'][0])
    for k, (g, r) in enumerate(zip(grads_f, c['R'][1])):
        assert torch.equal(g, r), ('counts = N', k)


@pytest.mark.parametrize('dtype', [BF16, F16])
@pytest.mark.parametrize('variant', VARIANTS)
def test_projection_fused_inference_with_counts(dtype, variant):
    """under no_grad the projection-fused forward keeps Q/K/V on chip (STORE = false): same contract, and the real block is the
    training forward's bit for bit"""
    c = make_case('proj', dtype, variant)
    with torch.no_grad():
        out, _ = run(c, c['nc'], None, grad=False)
        out_none, _ = run(c, None, None, grad=False)
    assert torch.equal(out_none, c['R'][0])
    for b, n in enumerate(c['counts']):
        assert torch.equal(out[b, :n, :n], c['R'][0][b, :n, :n])
        assert float(out[b, :, n:].float().abs().sum()) == 0
        assert torch.isfinite(out[b, :, :n]).all()


@pytest.mark.parametrize('family,dtype', [('gen16', F32), ('bwd2', BF16), ('proj', BF16), ('t16_40', BF16)])
def test_graph_scale_wins_over_the_count(family, dtype, monkeypatch):
    """graph 1 (0 < n < N) dropped by DropPath: all zeros for it whatever its count, the other graphs as with counts alone"""
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_TRI_SKIP_BWD', True)
    c = make_case(family, dtype, 'gated')
    assert 0 < c['counts'][1] < c['N']
    sc = torch.ones(c['B'], dtype=torch.float32, device='cuda')
    sc[1] = 0
    d_out = c['d_out'].clone()
    d_out[1] = 0                                                # what a dropped graph receives
    out, grads = run(c, c['nc'], d_out, graph_scale=sc)
    want_out, want_grads = run(c, c['nc'], d_out)
    assert float(out[1].float().abs().sum()) == 0
    assert float(want_out[1].float().abs().sum()) > 0
    keep = [b for b in range(c['B']) if b != 1]
    assert torch.equal(out[keep], want_out[keep])
    for g, w in zip(grads, want_grads):
        assert torch.isfinite(g).all() and torch.equal(g, w)
    assert float(grads[0][1].float().abs().sum()) == 0


def test_dropout_pattern_of_computed_units_does_not_move():
    """attention dropout p = 0.25 on the generic kernels: the unit index keeps N, so items 1, 2 and 4 hold unchanged"""
    c = make_case('gen16', F32, 'gated', dropout=(0.25, 0x1234567))
    plain = make_case('gen16', F32, 'gated')
    assert not torch.equal(c['R'][0], plain['R'][0])            # (the dropout is on)
    out, grads = run(c, c['nc'], c['d_out'], dropout=c['dropout'])
    check_against_reference(c, out, grads, 'dropout')


def test_counts_are_ignored_above_64_nodes():
    """N = 72: the key-blocked kernels accept the counts and compute everything"""
    from tgt_amd import ops
    N, C, H = 72, 64, 4
    counts = COUNTS[N]
    B = len(counts)
    L = ops.TripletLayout(C, H, gated=True, biased=True)
    rng = np.random.default_rng(72)
    c = dict(kind='plain', L=L, inputs=[rnd(rng, B, N, N, L.width).to(BF16).cuda()],
             mask3=gu.additive_mask(counts, N, torch.float32).reshape(B, N, N).cuda())
    d_out = rnd(rng, B, N, N, 2 * C).to(BF16).cuda()
    out, grads = run(c, torch.tensor(counts, dtype=torch.int32, device='cuda'), d_out)
    want, want_grads = run(c, None, d_out)
    assert torch.equal(out, want) and torch.equal(grads[0], want_grads[0])
    assert float(out[1, :, counts[1]:].float().abs().max()) > 0     # (computed, not skipped)


def _count_rule(mask):
    """numpy statement of tgt_mask_node_counts"""
    open_ = mask > -np.finfo(np.float32).max / 2
    cols = open_.any(axis=1)                                     # (B, N): column j has an open entry in some row i
    return np.array([0 if not r.any() else 1 + int(np.nonzero(r)[0].max()) for r in cols], dtype=np.int32)


def test_mask_node_counts():
    from tgt_amd import ops
    for N, counts in COUNTS.items():
        m = gu.additive_mask(counts, N, torch.float32).reshape(len(counts), N, N).cuda()
        got = ops.mask_node_counts(m)
        assert got.dtype == torch.int32 and got.is_cuda
        assert got.tolist() == counts, (N, got.tolist())
    N, lo = 33, torch.finfo(torch.float32).min                  # crosses a wave
    m = torch.full((4, N, N), lo)
    m[0, 3, N - 1] = 0                                          # a single open entry in the last column
    m[2, 20, 5] = 0                                             # an open entry only below the diagonal (graph 1: all closed)
    m[3] = gu.additive_mask([17], N, torch.float32).reshape(N, N)
    m[3, 2, 30] = -1.0e38                                       # open by the rule (> finfo.min / 2), not zero
    got = ops.mask_node_counts(m.cuda())
    assert got.tolist() == _count_rule(m.numpy()).tolist() == [N, 0, 6, 31]


def test_node_counts_argument_is_checked():
    from tgt_amd import ops
    c = make_case('gen16', F32, 'gated')
    bad = [c['nc'].long(), c['nc'][:2], c['nc'].cpu(), torch.zeros(2 * c['B'], dtype=torch.int32, device='cuda')[::2]]
    for nc in bad:
        with pytest.raises(RuntimeError, match='node_counts'):
            ops.triplet_attention(c['inputs'][0], c['mask3'], c['L'], node_counts=nc)
    w = torch.zeros(c['L'].width, c['C'], device='cuda')
    with pytest.raises(RuntimeError, match='node_counts'):
        ops.projected_triplet_attention(torch.zeros(c['B'], c['N'], c['N'], c['C'], device='cuda'), w, w[:, 0].contiguous(), c['mask3'], c['L'],
                                        node_counts=bad[0])
    big = torch.tensor([1000, -5, 3, 7], dtype=torch.int32, device='cuda')      # the kernels clamp: 12, 0, 3, 7
    out = ops.triplet_attention(c['inputs'][0], c['mask3'], c['L'], node_counts=big)
    torch.cuda.synchronize()
    assert torch.equal(out[0], c['R'][0][0]) and float(out[1].abs().sum()) == 0 and float(out[2, :, 3:].abs().sum()) == 0


_CHILD = r'''
import sys, torch
sys.path.insert(0, sys.argv[1])
import test_hip_triplet_ragged as t
from tgt_amd import ops
ops._SPLIT_MIN_ROWS = 1
for fam in ('bwd2', 'bwd2_colsum'):
    c = t.make_case(fam, torch.bfloat16, 'gated')
    out, grads = t.run(c, c['nc'], c['d_out'])
    t.check_against_reference(c, out, grads, fam)
print('child OK')
'''


def test_register_prefetch_form_of_bwd2():
    """the library reads TGT_TRI_BWD2_DMA once, at its first launch: the register-prefetch instantiation of tri_att_bwd2_kernel
    needs a process of its own (with and without column sums; same checks as above)"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, TGT_TRI_BWD2_DMA='0')
    r = subprocess.run([sys.executable, '-c', _CHILD, here], env=env, cwd=os.path.dirname(here), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b'child OK' in r.stdout, r.stdout.decode(errors='replace')[-3000:]
