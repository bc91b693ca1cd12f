"""Triplet attention at 65 <= N <= 128 (csrc/triplet_attention_kb.hip: key-blocked forward with an online softmax, three-sweep
backward) against the float64 oracle on the CPU, on the GPU.

Bars: the project's own (tests/test_hip_ops.py): rel-L2 against float64 of 2e-6 / 8e-3 / 1e-3 for fp32 / bf16 / fp16, twice
that for gradients.  They were set from errors measured at N <= 64 and are used here unchanged.
"""
import numpy as np
import pytest
import torch

import golden_util as gu
import triplet_kb_util as ku
from oracle import core

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-6, torch.bfloat16: 8e-3, torch.float16: 1e-3}
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16

C65 = (1, 65, [65], 32, 2)            # one key past two blocks: a last block with a single live key
C80 = (2, 80, [80, 71], 64, 4)        # ragged batch, padded query rows and keys
C96 = (2, 96, [96, 33], 32, 2)        # second graph: whole key blocks fully masked, query tiles fully padded
C72 = (1, 72, [72], 128, 8)           # more than one head group
C128 = (1, 128, [128], 32, 2)         # the upper limit, every block full


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rnd(rng, *shape, scale=1.0):
    return torch.from_numpy(rng.standard_normal(shape) * scale)


def to_ref(x_hm, idx):
    out = torch.empty_like(x_hm)
    out[..., idx] = x_hm
    return out


def oracle_run(fused, d_out, mask, C, H, gated, biased, dropout=None):
    """float64 oracle in the reference layout on the values as the kernel sees them: (output head-major, gradient of fused)"""
    from tgt_amd import layout
    f64 = fused.double().requires_grad_(True)
    idx, oidx = layout.head_major_index(C, H), layout.va_cols_head_major(C, H)
    blk = lambda lo: torch.cat([to_ref(f64[..., lo + q * C: lo + (q + 1) * C], idx) for q in range(3)], -1)
    nb = (2 if gated else 1) * H
    eg_in = f64[..., 6 * C: 6 * C + nb] if biased else None
    eg_out = f64[..., 6 * C + nb: 6 * C + 2 * nb] if biased else None
    kw = {} if dropout is None else dict(dropout=dropout)
    va = core.triplet_attention_core(blk(0), eg_in, blk(3 * C), eg_out, mask.double(), H, gated, biased, **kw)[..., oidx]
    (va * d_out.double()).sum().backward()
    return va.detach(), f64.grad


def make(case, dtype, variant, seed=0):
    from tgt_amd import ops
    B, N, nn_, C, H = case
    gated, biased = variant == 'gated', variant != 'axial'
    L = ops.TripletLayout(C, H, gated=gated, biased=biased)
    rng = np.random.default_rng(seed + hash((B, N, C, H)) % 1000)
    fused = rnd(rng, B, N, N, L.width).to(dtype)
    d_out = rnd(rng, B, N, N, 2 * C).to(dtype)
    mask = gu.additive_mask(nn_, N, torch.float32)
    return L, fused, d_out, mask, gated, biased


def check(va, g, va_ref, g_ref, L, C, biased, dtype):
    tol = TOL[dtype]
    errs = dict(fwd=rel(va, va_ref), dqkv=rel(g[..., :6 * C], g_ref[..., :6 * C]))
    if biased:
        errs['deg'] = rel(g[..., 6 * C:L.used], g_ref[..., 6 * C:L.used])
    print('rel-L2', str(dtype), errs)
    assert torch.isfinite(va).all() and torch.isfinite(g).all()
    assert errs['fwd'] < tol, errs
    assert errs['dqkv'] < 2 * tol, errs
    if biased:
        assert errs['deg'] < 2 * tol, errs


PARITY = ([(c, F32, 'gated') for c in (C65, C80, C96, C72, C128)] + [(c, BF16, 'gated') for c in (C65, C80, C96, C72, C128)] +
          [(c, F16, 'gated') for c in (C65, C80, C128)] +
          [(C80, F32, 'ungated'), (C65, F32, 'axial'), (C96, BF16, 'axial'), (C72, BF16, 'ungated'), (C96, F16, 'ungated'), (C80, F16, 'axial')])


@pytest.mark.parametrize('case,dtype,variant', PARITY, ids=lambda v: str(v).replace('torch.', '') if not isinstance(v, tuple) else f'N{v[1]}H{v[4]}')
def test_triplet_attention_kb(case, dtype, variant):
    from tgt_amd import ops
    B, N, nn_, C, H = case
    L, fused, d_out, mask, gated, biased = make(case, dtype, variant)
    va_ref, g_ref = oracle_run(fused, d_out, mask, C, H, gated, biased)
    fx = fused.cuda().requires_grad_(True)
    va = ops.triplet_attention(fx, mask.reshape(B, N, N).cuda(), L)
    va.backward(d_out.cuda())
    torch.cuda.synchronize()
    check(va, fx.grad, va_ref, g_ref, L, C, biased, dtype)


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('variant', ['gated', 'axial'])
@pytest.mark.parametrize('case', [(2, 80, [80, 71], 32, 2), C128], ids=['N80', 'N128'])
def test_triplet_attention_kb_dropout(case, dtype, variant):
    """forward and backward against the oracle given the SAME keep pattern (tests/triplet_kb_util.py), plus the keep rate"""
    from tgt_amd import ops
    B, N, nn_, C, H = case
    L, fused, d_out, mask, gated, biased = make(case, dtype, variant, seed=11)
    p_drop, seed = 0.3, 0x1234567890ABCDEF
    units = (((np.arange(B)[:, None, None, None] * 2 + np.arange(2)[None, :, None, None]) * H +
              np.arange(H)[None, None, :, None]) * N + np.arange(N)[None, None, None, :]).reshape(-1)
    keep, scale = ku.triplet_dropout_keep(seed, p_drop, units, N)
    keep = torch.from_numpy(keep.reshape(B, 2, H, N, N, N))            # (b, dir, h, j, i, k)
    rate = float(keep.float().mean())
    assert abs(rate - (1 - p_drop)) < 0.02, rate
    keep_dirs = [keep[:, d].permute(0, 3, 2, 4, 1).contiguous() for d in (0, 1)]      # (b, i, j, k, h)
    va_ref, g_ref = oracle_run(fused, d_out, mask, C, H, gated, biased, dropout=(keep_dirs[0], keep_dirs[1], scale))
    fx = fused.cuda().requires_grad_(True)
    va = ops.triplet_attention(fx, mask.reshape(B, N, N).cuda(), L, dropout=(p_drop, seed))
    va.backward(d_out.cuda())
    torch.cuda.synchronize()
    check(va, fx.grad, va_ref, g_ref, L, C, biased, dtype)


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
def test_triplet_attention_kb_skips_dropped_graphs(dtype, monkeypatch):
    """graph_scale: the dropped graph's output and gradient rows are exactly zero, the others bit-equal to a run without it"""
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_TRI_SKIP_BWD', True)
    case = (3, 80, [80, 66, 70], 32, 2)
    B, N, nn_, C, H = case
    L, fused, d_out, mask, _, _ = make(case, dtype, 'gated', seed=5)
    m3 = mask.reshape(B, N, N).cuda()
    sc = torch.tensor([1.25, 0.0, 1.25], dtype=torch.float32, device='cuda')
    live = (sc != 0).view(B, 1, 1, 1).to(dtype)
    d_out = d_out.cuda() * live
    full, skip = fused.cuda().requires_grad_(True), fused.cuda().requires_grad_(True)
    va_full = ops.triplet_attention(full, m3, L)
    va_full.backward(d_out)
    va_skip = ops.triplet_attention(skip, m3, L, graph_scale=sc)
    va_skip.backward(d_out)
    torch.cuda.synchronize()
    assert float(va_full[1].abs().max()) > 0
    assert float(va_skip[1].abs().max()) == 0 and float(skip.grad[1].abs().max()) == 0
    assert torch.isfinite(skip.grad).all()
    for b in (0, 2):
        assert torch.equal(va_skip[b], va_full[b])
        assert torch.equal(skip.grad[b], full.grad[b])


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
def test_triplet_attention_kb_backward_is_deterministic(dtype):
    from tgt_amd import ops
    B, N, nn_, C, H = C80
    L, fused, d_out, mask, _, _ = make(C80, dtype, 'gated', seed=3)
    m3, d_out = mask.reshape(B, N, N).cuda(), d_out.cuda()
    grads = []
    for _ in range(2):
        fx = fused.cuda().requires_grad_(True)
        ops.triplet_attention(fx, m3, L, dropout=(0.3, 99)).backward(d_out)
        grads.append(fx.grad)
    torch.cuda.synchronize()
    assert torch.equal(grads[0], grads[1])


@pytest.mark.parametrize('dtype', [F32, BF16, F16], ids=['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('split', [False, True], ids=['fused', 'split'])
def test_projected_triplet_attention_kb(dtype, split, monkeypatch):
    """projection + core as one autograd node at N > 64 (library GEMM + the key-blocked kernels, bias gradient by the
    column-sum op) against triplet_attention(linear(...)); split: Q/K/V and E/G in two tensors, ONE fused gradient row
    (ld_dqkv / ld_deg).  Bars of tests/test_hip_ops.py::test_triplet_attention_dropout for the same comparison."""
    from tgt_amd import ops
    if split:
        monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 1)
    B, N, nn_, C, H = C80
    L = ops.TripletLayout(C, H)
    rng = np.random.default_rng(7)
    x = rnd(rng, B, N, N, C).to(dtype).cuda()
    w = (rnd(rng, L.width, C) * C ** -0.5).to(dtype).cuda().requires_grad_(True)
    b = (rnd(rng, L.width) * 0.1).to(dtype).cuda().requires_grad_(True)
    d_out = rnd(rng, B, N, N, 2 * C).to(dtype).cuda()
    m3 = gu.additive_mask(nn_, N, torch.float32).reshape(B, N, N).cuda()
    assert ops._split_projection_ok(x, L) == split
    y1 = ops.projected_triplet_attention(x, w, b, m3, L)
    g1 = torch.autograd.grad(y1, (w, b), d_out)
    y0 = ops.triplet_attention(ops.linear(x, w, b), m3, L)
    g0 = torch.autograd.grad(y0, (w, b), d_out)
    torch.cuda.synchronize()
    tol = TOL[dtype]
    errs = (rel(y1, y0), rel(g1[0], g0[0]), rel(g1[1][:L.used], g0[1][:L.used]))
    print('projected', str(dtype), errs)
    assert torch.isfinite(y1).all() and torch.isfinite(g1[0]).all() and torch.isfinite(g1[1]).all()
    assert errs[0] < tol and errs[1] < 2 * tol, errs
    assert errs[2] < (1e-5 if dtype == torch.float32 else 2e-2), errs


def test_tgt_multi_trains_a_step_at_72_nodes():
    """a 2-layer TGT_Multi with triplet_type='attention' on a ragged batch padded to 72 nodes, fp32: loss and EVERY parameter
    gradient against oracle.modules.TGT_Multi on the CPU with the same parameters.  Bars of
    tests/test_hip_model.py::test_task_model_matches_reference_golden for its fp32 tiny models: 3e-4 outputs / loss, 2e-3 gradients."""
    from oracle import modules as om
    from tgt_amd.pcqm import TGT_Multi
    from tgt_amd.training.step import pretrain_loss, StepConfig
    kwargs = dict(gu.MODEL_CASES['multi_at_tiny'][1])
    kwargs.update(model_height=2, edge_width=32, triplet_heads=2, triplet_type='attention')
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


def test_triplet_attention_refuses_more_than_128_nodes():
    from tgt_amd import ops
    L = ops.TripletLayout(32, 2)
    fused = torch.zeros(1, 129, 129, L.width, device='cuda')
    with pytest.raises(RuntimeError, match='128'):
        ops.triplet_attention(fused, torch.zeros(1, 129, 129, device='cuda'), L)
