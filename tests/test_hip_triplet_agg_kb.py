"""Triplet aggregate at 65 <= N <= 128 (csrc/triplet_aggregate_kb.hip: one query tile per workgroup forward, A sweep + V sweep
backward) against the float64 oracle on the CPU, on the GPU.

Bars: those of tests/test_hip_ops.py::test_triplet_aggregate, unchanged: rel-L2 against float64 of 2e-6 / 8e-3 / 1e-3 for
fp32 / bf16 / fp16 on the output, twice that for dV and for dE / dG separately, everything finite.
"""
import functools

import numpy as np
import pytest
import torch

import golden_util as gu
import triplet_kb_util as ku
from oracle import core

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-6, torch.bfloat16: 8e-3, torch.float16: 1e-3}
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16

CASES = {
    'C65': (1, 65, (65,), 32, 2),            # one key past two tiles
    'C80': (2, 80, (80, 71), 64, 4),         # ragged batch
    'C96': (2, 96, (96, 33), 32, 2),         # whole key tiles masked, query tiles fully padded
    'C72': (1, 72, (72,), 128, 8),           # two head groups
    'C70': (1, 70, (70,), 48, 3),            # H not a multiple of 4
    'C128': (1, 128, (128,), 32, 2),         # the limit, every tile full
    'D80': (2, 80, (80, 71), 32, 2),         # the dropout tests' ragged batch
}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rnd(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape))


def to_ref(x_hm, idx):
    out = torch.empty_like(x_hm)
    out[..., idx] = x_hm
    return out


def keep_pattern(case, p_drop, seed):
    """the kernels' keep decisions in the oracle's layouts: inward (b, i, k, h), outward (b, k, i, h), and the scale"""
    B, N, _, _, H = CASES[case]
    units = ((np.arange(B)[:, None, None] * 2 + np.arange(2)[None, :, None]) * H + np.arange(H)[None, None, :]).reshape(-1)
    keep, scale = ku.triplet_dropout_keep(seed, p_drop, units, N)
    keep = torch.from_numpy(keep.reshape(B, 2, H, N, N))                # (b, dir, h, i, k)
    keep_in = keep[:, 0].permute(0, 2, 3, 1).contiguous()
    keep_out = keep[:, 1].permute(0, 3, 2, 1).contiguous()              # the kernel's (i, k) is A_out[k, i]
    return keep, (keep_in, keep_out, scale)


@functools.lru_cache(maxsize=None)
def reference(case, dtype, gated, seed=0, dropout=None):
    """inputs (as the kernel sees them, rounded to dtype) and the float64 oracle's output and gradient, computed once"""
    from tgt_amd import ops, layout
    B, N, nn_, C, H = CASES[case]
    L = ops.AggregateLayout(C, H, gated=gated)
    rng = np.random.default_rng(seed + hash((B, N, C, H, 1)) % 1000)
    fused = rnd(rng, B, N, N, L.width).to(dtype)
    d_out = rnd(rng, B, N, N, 2 * C).to(dtype)
    mask = gu.additive_mask(list(nn_), N, torch.float32)
    f64 = fused.double().requires_grad_(True)
    idx, oidx = layout.head_major_index(C, H), layout.va_cols_head_major(C, H)
    v_both = torch.cat([to_ref(f64[..., q * C:(q + 1) * C], idx) for q in range(2)], -1)
    kw = {}
    if dropout is not None:
        kw['dropout'] = keep_pattern(case, *dropout)[1]
    va_ref = core.triplet_aggregate_core(v_both, f64[..., 2 * C:L.used], mask.double(), H, gated, **kw)[..., oidx]
    (va_ref * d_out.double()).sum().backward()
    return L, fused, d_out, mask.reshape(B, N, N), va_ref.detach(), f64.grad


def run_and_check(case, dtype, gated, seed=0, dropout=None):
    from tgt_amd import ops
    C = CASES[case][3]
    L, fused, d_out, mask, va_ref, g_ref = reference(case, dtype, gated, seed, dropout)
    fx = fused.cuda().requires_grad_(True)
    kw = {} if dropout is None else dict(dropout=dropout)
    va = ops.triplet_aggregate(fx, mask.cuda(), L, **kw)
    va.backward(d_out.cuda())
    torch.cuda.synchronize()
    g, tol = fx.grad, TOL[dtype]
    errs = dict(fwd=rel(va, va_ref), dv=rel(g[..., :2 * C], g_ref[..., :2 * C]), deg=rel(g[..., 2 * C:L.used], g_ref[..., 2 * C:L.used]))
    print('rel-L2', case, str(dtype), 'gated' if gated else 'ungated', errs)
    assert torch.isfinite(va).all() and torch.isfinite(g).all()
    assert errs['fwd'] < tol, errs
    assert errs['dv'] < 2 * tol, errs
    assert errs['deg'] < 2 * tol, errs


PARITY = ([(c, dt) for dt in (F32, BF16) for c in ('C65', 'C80', 'C96', 'C72', 'C70', 'C128')] +
          [(c, F16) for c in ('C65', 'C80', 'C128')])


@pytest.mark.parametrize('gated', [True, False], ids=['gated', 'ungated'])
@pytest.mark.parametrize('case,dtype', PARITY, ids=lambda v: str(v).replace('torch.', ''))
def test_triplet_aggregate_kb(case, dtype, gated):
    run_and_check(case, dtype, gated)


@pytest.mark.parametrize('gated', [True, False], ids=['gated', 'ungated'])
@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('case', ['D80', 'C128'])
def test_triplet_aggregate_kb_dropout(case, dtype, gated):
    """forward and backward against the oracle given the SAME keep pattern (tests/triplet_kb_util.py with the aggregate's
    units (b*2 + dir)*H + h), plus the keep rate"""
    p_drop, seed = 0.3, 0x1234567890ABCDEF
    keep, _ = keep_pattern(case, p_drop, seed)
    rate = float(keep.float().mean())
    assert abs(rate - (1 - p_drop)) < 0.02, rate
    run_and_check(case, dtype, gated, seed=13, dropout=(p_drop, seed))


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
def test_triplet_aggregate_kb_is_deterministic(dtype):
    from tgt_amd import ops
    L, fused, d_out, mask, _, _ = reference('C80', dtype, True)
    m3, d_out = mask.cuda(), d_out.cuda()
    outs, grads = [], []
    for _ in range(2):
        fx = fused.cuda().requires_grad_(True)
        va = ops.triplet_aggregate(fx, m3, L, dropout=(0.3, 99))
        va.backward(d_out)
        outs.append(va.detach())
        grads.append(fx.grad)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(grads[0], grads[1])


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
def test_registered_op_equals_the_ctypes_path_at_80_nodes(dtype):
    """torch.ops.tgt.triplet_aggregate: same kernels behind both bindings, outputs and gradients bit-identical"""
    from tgt_amd import ops, torch_ops
    t = torch_ops.load()
    B, N, nn_, C, H = CASES['C80']
    L, fused, d_out, mask, _, _ = reference('C80', dtype, True)
    m3, d_out, fa = mask.cuda(), d_out.cuda(), fused.cuda()
    a1 = fa.clone().requires_grad_(True)
    o1 = ops.triplet_aggregate(a1, m3, L)
    o1.backward(d_out)
    ap = [fa[..., :C], fa[..., 2 * C:2 * C + 2 * H], fa[..., C:2 * C], fa[..., 2 * C + 2 * H:2 * C + 4 * H]]
    ap = [p.clone().requires_grad_(True) for p in ap]
    o2 = t.triplet_aggregate(ap[0], ap[1], ap[2], ap[3], m3, H, False)
    o2.backward(d_out)
    torch.cuda.synchronize()
    g = a1.grad
    assert torch.equal(o1, o2)
    assert torch.equal(g[..., :C], ap[0].grad) and torch.equal(g[..., C:2 * C], ap[2].grad)
    assert torch.equal(g[..., 2 * C:2 * C + 2 * H], ap[1].grad) and torch.equal(g[..., 2 * C + 2 * H:2 * C + 4 * H], ap[3].grad)


def test_tgt_multi_with_aggregate_triplets_trains_a_step_at_72_nodes():
    """a 2-layer TGT_Multi with triplet_type='aggregate' on a ragged batch padded to 72 nodes, fp32: loss, outputs and EVERY
    parameter gradient against oracle.modules.TGT_Multi on the CPU with the same parameters.  Bars of
    tests/test_hip_triplet_kb.py::test_tgt_multi_trains_a_step_at_72_nodes: 3e-4 outputs / loss, 2e-3 gradients."""
    from oracle import modules as om
    from tgt_amd.pcqm import TGT_Multi
    from tgt_amd.training.step import pretrain_loss, StepConfig
    kwargs = dict(gu.MODEL_CASES['multi_at_tiny'][1])
    kwargs.update(model_height=2, edge_width=32, triplet_heads=2, triplet_type='aggregate')
    geom = dict(B=2, N=72, num_nodes=[72, 66])
    model = gu.fill_params(TGT_Multi(**kwargs), seed=41).cuda().train()
    ref = gu.fill_params(om.TGT_Multi(**kwargs), seed=41).train()
    cpu = gu.model_batch(geom, seed=42)
    batch = {k: v.cuda() for k, v in cpu.items()}
    cfg = StepConfig(num_dist_bins=kwargs['num_dist_bins'], mixed_precision=None)
    out = model(batch)
    loss = pretrain_loss(out, batch, cfg)
    loss.backward()
    g_ref, l_ref = ref(cpu)
    loss_ref = torch.nn.functional.l1_loss(g_ref, cpu['target']) + 0.1 * core.binned_distance_xent(
        l_ref, core.pairwise_dist(cpu['dft_coords']), cpu['edge_mask'], kwargs['num_dist_bins'], 8)
    loss_ref.backward()
    assert rel(out[0], g_ref) < 3e-4 and rel(out[1], l_ref) < 3e-4, (rel(out[0], g_ref), rel(out[1], l_ref))
    assert abs(float(loss) - float(loss_ref)) < 3e-4 * abs(float(loss_ref)), (float(loss), float(loss_ref))
    pm, pr = dict(model.named_parameters()), dict(ref.named_parameters())
    assert set(pm) == set(pr)
    checked = 0
    for k, p in pr.items():
        if p.grad is None:
            continue
        assert pm[k].grad is not None, k
        assert torch.isfinite(pm[k].grad).all(), k
        assert rel(pm[k].grad, p.grad) < 2e-3, (k, rel(pm[k].grad, p.grad))
        checked += 1
    assert checked > 20


def test_triplet_aggregate_refuses_more_than_128_nodes():
    from tgt_amd import ops
    L = ops.AggregateLayout(32, 2)
    fused = torch.zeros(1, 129, 129, L.width, device='cuda')
    with pytest.raises(RuntimeError, match='128'):
        ops.triplet_aggregate(fused, torch.zeros(1, 129, 129, device='cuda'), L)
