"""TGT_TRI_COUNTS_KB on the GPU (csrc/triplet_attention_kb.hip; TGT_TRI_RAGGED_KB=1 / ops._TRI_RAGGED_KB): the key-blocked triplet
attention kernels for 65..128 nodes use the per-graph node counts -- the walk over the shared node ends at n, and 32-row query
tiles, 32-key blocks and owned tiles at or past n32 (n rounded up to 32) are skipped.  Because the mask closes every key past n
(weight exactly 0) and the cotangent of every padded row and column is zero, the real block of the output and the WHOLE gradient
are compared with torch.equal against the same op called without counts; the float64 oracle is held to the bars of
tests/test_hip_triplet_kb.py (2e-6 / 8e-3 / 1e-3, rel-L2 of the real block).

Shapes: N = 72 with C = 64, H = 4 (head group 4: query tiles of 32 / 32 / 8 rows) and counts on, one past and one below every
tile edge plus a one-node and an empty graph; N = 72, H = 2 (head group 1); N = 100 (a last tile of 4 rows); N = 128.  fp32 is
the form without register prefetch."""
import numpy as np
import pytest
import torch

import golden_util as gu
import triplet_kb_util as ku
from oracle import core

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-6, torch.bfloat16: 8e-3, torch.float16: 1e-3}      # tests/test_hip_triplet_kb.py
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
BIG = 8192.0                                                                 # finite and exact in every dtype
VARIANTS = ['gated', 'ungated', 'axial']
# name -> (N, C, H, counts)
SHAPES = {
    'n72h4': (72, 64, 4, [72, 65, 64, 33, 32, 1, 0]),
    'n72h2': (72, 32, 2, [72, 40, 0]),
    'n100': (100, 32, 2, [100, 97, 50]),
    'n128': (128, 32, 2, [128, 96, 31]),
}
CASES = ([('n72h4', BF16, v) for v in VARIANTS] + [('n72h4', F16, 'gated'), ('n72h4', F32, 'gated')] +
         [(s, BF16, 'gated') for s in ('n72h2', 'n100', 'n128')])
IDS = [f'{s}-{str(dt)[6:]}-{v}' for s, dt, v in CASES]


@pytest.fixture(autouse=True)
def switch_on(monkeypatch):
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_TRI_RAGGED_KB', True)


def rnd(rng, *shape, scale=1.0):
    return torch.from_numpy(rng.standard_normal(shape) * scale)


def n32(n):
    return (n + 31) // 32 * 32


def real_mask(counts, N):
    nm = torch.arange(N)[None, :] < torch.tensor(counts)[:, None]
    return (nm[:, :, None] & nm[:, None, :]).unsqueeze(-1).cuda()


def col_mask(counts, N):
    return (torch.arange(N)[None, :] < torch.tensor(counts)[:, None]).view(len(counts), 1, N, 1).cuda()


def run(c, node_counts, d_out, dropout=None, graph_scale=None):
    """one forward + backward: (out, d_fused)"""
    from tgt_amd import ops
    x = c['fused'].clone().requires_grad_(True)
    out = ops.triplet_attention(x, c['mask3'], c['L'], c['dropout'] if dropout is None else dropout, graph_scale, node_counts)
    out.backward(d_out)
    torch.cuda.synchronize()
    return out.detach(), x.grad


_cases = {}


def make_case(shape, dtype, variant, dropout=(0.0, 0)):
    """inputs on the device, the counts, the cotangent (zero at every padded row and column) and R = the op WITHOUT counts:
    computed once, never modified"""
    key = (shape, dtype, variant, dropout)
    if key in _cases:
        return _cases[key]
    from tgt_amd import ops
    N, C, H, counts = SHAPES[shape]
    B = len(counts)
    L = ops.TripletLayout(C, H, gated=variant == 'gated', biased=variant != 'axial')
    rng = np.random.default_rng(100 * list(SHAPES).index(shape) + 10 * VARIANTS.index(variant) + [F32, BF16, F16].index(dtype))
    c = dict(N=N, C=C, H=H, B=B, L=L, counts=counts, dtype=dtype, variant=variant, dropout=dropout,
             fused=rnd(rng, B, N, N, L.width).to(dtype).cuda(),
             mask3=gu.additive_mask(counts, N, torch.float32).reshape(B, N, N).cuda(),
             nc=torch.tensor(counts, dtype=torch.int32, device='cuda'),
             d_out=rnd(rng, B, N, N, 2 * C).to(dtype).cuda() * real_mask(counts, N).to(dtype))
    c['R'] = run(c, None, c['d_out'])
    _cases[key] = c
    return c


def check_contract(c, out, grad, what):
    R_out, R_grad = c['R']
    assert torch.isfinite(out).all() and torch.isfinite(grad).all(), what
    for b, n in enumerate(c['counts']):
        assert torch.equal(out[b, :n, :n], R_out[b, :n, :n]), (what, 'real block', b, n)
        assert float(out[b, :, n:].float().abs().sum()) == 0, (what, 'padded columns', b, n)
        assert float(out[b, n32(n):].float().abs().sum()) == 0, (what, 'padded query tiles', b, n)
    assert torch.equal(grad, R_grad), (what, 'd_fused', float((grad.float() - R_grad.float()).abs().max()))


def oracle_out(c):
    """float64 oracle of the forward in the kernels' channel order (tests/test_hip_triplet_kb.py::oracle_run), with the kernels'
    own keep pattern when the case has dropout"""
    from tgt_amd import layout
    B, N, C, H = c['B'], c['N'], c['C'], c['H']
    gated, biased = c['variant'] == 'gated', c['variant'] != 'axial'
    f64 = c['fused'].double().cpu()
    idx, oidx = layout.head_major_index(C, H), layout.va_cols_head_major(C, H)

    def to_ref(x_hm):
        out = torch.empty_like(x_hm)
        out[..., idx] = x_hm
        return out

    def blk(lo):
        return torch.cat([to_ref(f64[..., lo + p * C: lo + (p + 1) * C]) for p in range(3)], -1)
    nb = (2 if gated else 1) * H
    eg_in = f64[..., 6 * C: 6 * C + nb] if biased else None
    eg_out = f64[..., 6 * C + nb: 6 * C + 2 * nb] if biased else None
    kw = {}
    if c['dropout'][0] > 0:
        units = (((np.arange(B)[:, None, None, None] * 2 + np.arange(2)[None, :, None, None]) * H +
                  np.arange(H)[None, None, :, None]) * N + np.arange(N)[None, None, None, :]).reshape(-1)
        keep, scale = ku.triplet_dropout_keep(c['dropout'][1], c['dropout'][0], units, N)
        keep = torch.from_numpy(keep.reshape(B, 2, H, N, N, N))            # (b, dir, h, j, i, k)
        kw['dropout'] = (*[keep[:, d].permute(0, 3, 2, 4, 1).contiguous() for d in (0, 1)], scale)
    mask = gu.additive_mask(c['counts'], N, torch.float64)
    return core.triplet_attention_core(blk(0), eg_in, blk(3 * C), eg_out, mask, H, gated, biased, **kw)[..., oidx]


def check_everything(c, what):
    out, grad = run(c, c['nc'], c['d_out'])
    check_contract(c, out, grad, what)
    # the real block against the float64 oracle
    real = real_mask(c['counts'], c['N'])
    want = oracle_out(c) * real.cpu()
    got = (out * real).double().cpu()
    err = float((got - want).norm() / (want.norm() + 1e-30))
    print(what, c['dtype'], c['variant'], 'real block vs float64 oracle: rel-L2', err)
    assert err < TOL[c['dtype']], err
    # the padded columns of d_out are not read
    poisoned = torch.where(col_mask(c['counts'], c['N']).expand_as(c['d_out']), c['d_out'], torch.full_like(c['d_out'], BIG))
    assert float((poisoned - c['d_out']).abs().max()) == BIG
    out_p, grad_p = run(c, c['nc'], poisoned)
    assert torch.equal(out_p, out) and torch.equal(grad_p, grad), (what, 'poisoned d_out')
    # counts = N: the run without counts, everywhere
    out_f, grad_f = run(c, torch.full((c['B'],), c['N'], dtype=torch.int32, device='cuda'), c['d_out'])
    assert torch.equal(out_f, c['R'][0]) and torch.equal(grad_f, c['R'][1]), (what, 'counts = N')
    # counts outside [0, N] are clamped in the kernel
    wild = c['nc'].clone()
    wild[0], wild[1] = 1000, -5
    out_w, grad_w = run(c, wild, c['d_out'] * (torch.arange(c['B'], device='cuda') != 1).view(-1, 1, 1, 1).to(c['dtype']))
    assert torch.equal(out_w[0], c['R'][0][0]) and torch.equal(grad_w[0], c['R'][1][0])
    assert float(out_w[1].float().abs().sum()) == 0 and float(grad_w[1].float().abs().sum()) == 0
    assert torch.equal(out_w[2:], out[2:]) and torch.equal(grad_w[2:], grad[2:])


@pytest.mark.parametrize('shape,dtype,variant', CASES, ids=IDS)
def test_counts_skip_padded_units_tiles_and_key_blocks_bit_exactly(shape, dtype, variant):
    c = make_case(shape, dtype, variant)
    assert c['R'][0][1, :, c['counts'][1]:].float().abs().max() > 0          # (without counts the padded columns are computed)
    check_everything(c, shape)


def test_dropout_pattern_of_computed_elements_does_not_move():
    """attention dropout p = 0.25: N keeps the unit and word indices, so the whole contract holds unchanged"""
    c = make_case('n72h4', BF16, 'gated', dropout=(0.25, 0x1234567))
    plain = make_case('n72h4', BF16, 'gated')
    assert torch.equal(c['fused'], plain['fused']) and not torch.equal(c['R'][0], plain['R'][0])      # (the dropout is on)
    check_everything(c, 'dropout')


def test_graph_scale_wins_over_the_count(monkeypatch):
    """graph 1 (0 < n < N) dropped by DropPath: all zeros for it whatever its count, the other graphs as with counts alone"""
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_TRI_SKIP_BWD', True)
    c = make_case('n72h4', BF16, 'gated')
    assert 0 < c['counts'][1] < c['N']
    sc = torch.ones(c['B'], dtype=torch.float32, device='cuda')
    sc[1] = 0
    d_out = c['d_out'].clone()
    d_out[1] = 0                                                # what a dropped graph receives
    out, grad = run(c, c['nc'], d_out, graph_scale=sc)
    want_out, want_grad = run(c, c['nc'], d_out)
    assert float(out[1].float().abs().sum()) == 0 and float(grad[1].float().abs().sum()) == 0
    assert float(want_out[1].float().abs().sum()) > 0
    keep = [b for b in range(c['B']) if b != 1]
    assert torch.equal(out[keep], want_out[keep])
    assert torch.isfinite(grad).all() and torch.equal(grad, want_grad)


@pytest.mark.parametrize('split', [False, True], ids=['fused', 'split'])
def test_projected_triplet_attention_hands_the_counts_down(split, monkeypatch):
    """projected_triplet_attention at N = 72 (library GEMMs + the key-blocked kernels): the same contract through the projection
    node -- real block equal, padded columns and query tiles zero, x / weight / bias gradients equal"""
    from tgt_amd import ops
    if split:
        monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 1)
    N, C, H, counts = 72, 64, 4, [72, 40, 9]
    B, dtype = len(counts), BF16
    L = ops.TripletLayout(C, H)
    rng = np.random.default_rng(7)
    x = rnd(rng, B, N, N, C).to(dtype).cuda()
    w = (rnd(rng, L.width, C) * C ** -0.5).to(dtype)
    b = (rnd(rng, L.width) * 0.1).to(dtype)
    w[L.used:] = 0
    b[L.used:] = 0
    m3 = gu.additive_mask(counts, N, torch.float32).reshape(B, N, N).cuda()
    d_out = rnd(rng, B, N, N, 2 * C).to(dtype).cuda() * real_mask(counts, N).to(dtype)
    nc = torch.tensor(counts, dtype=torch.int32, device='cuda')
    assert ops._split_projection_ok(x, L) == split

    def go(node_counts):
        ins = [t.clone().cuda().requires_grad_(True) for t in (x, w, b)]
        out = ops.projected_triplet_attention(*ins, m3, L, node_counts=node_counts)
        out.backward(d_out)
        torch.cuda.synchronize()
        return out.detach(), [t.grad for t in ins]
    want, want_grads = go(None)
    out, grads = go(nc)
    assert float(want[1, :, counts[1]:].float().abs().max()) > 0
    for g, n in enumerate(counts):
        assert torch.equal(out[g, :n, :n], want[g, :n, :n])
        assert float(out[g, :, n:].float().abs().sum()) == 0 and float(out[g, n32(n):].float().abs().sum()) == 0
    assert torch.isfinite(out).all()
    for k, (g, r) in enumerate(zip(grads, want_grads)):
        assert torch.isfinite(g).all() and torch.equal(g, r), ('gradient', k)


# ---- a whole model: the 2-layer TGT-At of tests/test_hip_model_ragged.py on a batch padded to 72 nodes
GEOM = dict(B=3, N=72, num_nodes=[72, 40, 9])
CFG = dict(gu.MODEL_CASES['multi_at_tiny'][1], model_height=2, node_width=64, edge_width=256, num_heads=4, triplet_heads=16)


def _step(model, batch, autocast):
    from tgt_amd.training.step import pretrain_loss, StepConfig
    cfg = StepConfig(num_dist_bins=CFG['num_dist_bins'], mixed_precision=None)
    model.zero_grad(set_to_none=True)
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
        out = model(batch)
        loss = pretrain_loss(out, batch, cfg)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), [o.detach() for o in out], {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('autocast', [False, True], ids=['fp32', 'bf16'])
def test_training_step_is_bit_identical_with_both_switches_on(autocast, monkeypatch):
    """TGT_TRI_RAGGED (the model computes and hands down the counts) + TGT_TRI_RAGGED_KB (the kernels for N > 64 use them) against
    both off: the loss, every parameter gradient and the outputs on real nodes and edges"""
    from tgt_amd import ops, _lib
    from tgt_amd.pcqm import TGT_Multi
    from tgt_amd.tgt import stack
    model = gu.fill_params(TGT_Multi(**CFG), seed=31).cuda().train()
    batch = {k: v.cuda() for k, v in gu.model_batch(GEOM, seed=32).items()}
    flags = []
    real_launch = ops._launch

    def spy(entry, *args, prof=None):
        # (the triplet attention launches: counts given = the _counts entry, the flag = TRI_COUNTS_KB on the argument block)
        if entry.startswith(('tgt_triplet_attention_fwd', 'tgt_triplet_attention_bwd')):
            flags.append((entry, entry.endswith('_counts'), bool(args[0]._obj.flags & _lib.TRI_COUNTS_KB)))
        return real_launch(entry, *args, prof=prof)
    monkeypatch.setattr(ops, '_launch', spy)
    monkeypatch.setattr(stack, '_TRI_RAGGED', False)
    monkeypatch.setattr(ops, '_TRI_RAGGED_KB', False)
    loss0, out0, grads0 = _step(model, batch, autocast)
    assert len(flags) == 2 * CFG['model_height'] and not any(f[1] or f[2] for f in flags)
    del flags[:]
    monkeypatch.setattr(stack, '_TRI_RAGGED', True)
    monkeypatch.setattr(ops, '_TRI_RAGGED_KB', True)
    loss1, out1, grads1 = _step(model, batch, autocast)
    assert len(flags) == 2 * CFG['model_height'] and all(f[1] and f[2] for f in flags)        # forward and backward alike
    assert torch.equal(loss1, loss0), (float(loss1), float(loss0))
    em = batch['edge_mask'].bool()
    assert torch.equal(out1[0], out0[0])                                                # gap: one value per graph
    assert torch.equal(out1[1][em], out0[1][em])                                        # distance logits on the real edges
    assert grads1.keys() == grads0.keys() and len(grads0) > 20
    bad = [k for k in grads0 if not torch.equal(grads1[k], grads0[k])]
    assert not bad, bad
    assert any('tria' in k for k in grads0)
