"""Loss, outputs and EVERY parameter gradient of a 2-layer TGT-At at BASELINE widths on the benchmark batch size (B = 256,
N = 32: 262144 edge rows, so every persistent tgt_edge_linear workgroup walks 32 row tiles, the LayerNorm backwards fold all
their partial rows and the weight gradients go through their row chunks + plane sums), on the HIP path under bf16 / fp16
autocast, against the oracle run in float64 on the GPU.  All 256 graphs (ragged, one of them a single node) contribute to the
loss.  Bound, per tensor: 2x the oracle's own drift under the same autocast (fp32 parameters) against its float64 run -- the
convention of gu.bf16_drift, measured here on this batch.

Trainer-only modes (node side stream, flat gradient destinations, graph replay) are held equal to a plain backward by
tests/test_hip_trainer.py; a plain loss.backward() is used here."""
import numpy as np
import pytest
import torch

import golden_util as gu
import parity_log
from oracle import core, modules as om

pytestmark = pytest.mark.gpu

CFG = {**gu.FULL_AT_CFG, 'model_height': 2}
SEED = 2604
# ragged: graph 0 full, graph 1 a single node, every fourth graph full, the rest 2..32 nodes
_NN = np.random.default_rng(17).integers(2, 33, size=256)
_NN[::4] = 32
_NN[1] = 1
GEOM = dict(B=256, N=32, num_nodes=[int(n) for n in _NN])
# fp16: the loss is scaled by a fixed 2^12 (in the HIP run and the oracle's drift run alike) and the gradients divided back;
# unscaled, per-element gradients of ~1 / (256 * 1024) underflow in fp16
LOSS_SCALE = {torch.bfloat16: 1.0, torch.float16: 2.0 ** 12}


def rel(a, b):
    """rel-L2 in float64 on the device (the logits are 262144 x 512)"""
    a, b = a.detach().double(), b.detach().double()
    return parity_log.record(float((a - b).norm() / (b.norm() + 1e-30)))


def _ref_loss(gap, logits, batch, dist):
    return torch.nn.functional.l1_loss(gap, batch['target']) + 0.1 * core.binned_distance_xent(
        logits, dist, batch['edge_mask'], CFG['num_dist_bins'], 8)


def _oracle_run(batch, dist, dtype=None):
    """(loss, gap, logits, {name: grad}) of the oracle; dtype None: float64 parameters and inputs, else fp32 under autocast(dtype)"""
    model = gu.fill_params(om.TGT_Multi(**CFG), seed=SEED).cuda().train()
    if dtype is None:
        model = model.double()
        b = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
        with torch.autocast('cuda', enabled=False):
            gap, logits = model(b)
            loss = _ref_loss(gap, logits, b, dist.double())
        loss.backward()
        scale = 1.0
    else:
        scale = LOSS_SCALE[dtype]
        with torch.autocast('cuda', dtype=dtype):
            gap, logits = model(batch)
            loss = _ref_loss(gap, logits, batch, dist)
        (loss * scale).backward()
    grads = {k: (None if p.grad is None else p.grad / scale) for k, p in model.named_parameters()}
    out = (loss.detach(), gap.detach(), logits.detach(), grads)
    del model, gap, logits, loss
    return out


@pytest.fixture(scope='module')
def setting():
    """the batch on the device, the fp32 distance target (the bins of all runs come from the same fp32 distances) and the
    float64 oracle run, shared by both dtypes"""
    batch = {k: v.cuda() for k, v in gu.model_batch(GEOM, seed=SEED + 1).items()}
    dist = core.pairwise_dist(batch['dft_coords'].float())
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ref64 = _oracle_run(batch, dist)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f'\nfloat64 oracle at B = 256: peak device memory {peak / 2 ** 30:.2f} GiB')
    yield batch, dist, ref64
    del batch, dist, ref64
    torch.cuda.empty_cache()


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_batch_256_gradients_vs_float64_oracle(setting, dtype):
    from tgt_amd import gemm, ops
    from tgt_amd.pcqm import TGT_Multi
    from tgt_amd.training.step import StepConfig, pretrain_loss
    batch, dist, (loss64, gap64, logits64, g64) = setting
    parity_log.Tol.last = f'{str(dtype).replace("torch.", "")}-size-model'

    # the oracle's own drift under this autocast, per tensor
    loss_a, gap_a, logits_a, g_a = _oracle_run(batch, dist, dtype)
    drift = dict(loss=rel(loss_a, loss64), gap=rel(gap_a, gap64), logits=rel(logits_a, logits64))
    for k, g in g64.items():
        if g is not None and g_a[k] is not None:
            drift[k] = rel(g_a[k], g)
    del loss_a, gap_a, logits_a, g_a
    torch.cuda.empty_cache()

    # the HIP path, as the benchmark runs it
    model = gu.fill_params(TGT_Multi(**CFG), seed=SEED).cuda().train()
    cfg = StepConfig(num_dist_bins=CFG['num_dist_bins'], mixed_precision=None)
    before = (ops._lazy_dgrads[1], ops._colsum_handoffs[1], gemm.stats['own'])
    prof = ops.profile_kernels(True)
    try:
        with torch.autocast('cuda', dtype=dtype):
            gap, logits = model(batch)
            loss = pretrain_loss((gap, logits), batch, cfg)
        (loss * LOSS_SCALE[dtype]).backward()
        torch.cuda.synchronize()
    finally:
        ops.profile_kernels(False)
    # the benchmark's routes ran (no pass on an unfused fallback)
    for name in ('tgt_edge_linear', 'tgt_triplet_attention_proj_fwd'):
        assert len(prof.get(name, ())) > 0, (name, sorted(prof))
    assert ops._lazy_dgrads[1] > before[0], 'the LayerNorm backward was not fused into a consumer data gradient'
    assert ops._colsum_handoffs[1] > before[1], 'no bias gradient was handed over from a LayerNorm backward'
    assert gemm.stats['own'] > before[2], 'no GEMM went through the own kernels'
    del prof

    errs = {}
    for name, got, want in (('loss', loss, loss64), ('gap', gap, gap64), ('logits', logits, logits64)):
        errs[name] = rel(got, want)
    pm = dict(model.named_parameters())
    assert sorted(pm) == sorted(g64), 'parameter names differ from the oracle'
    for k, want in g64.items():
        got = pm[k].grad
        assert (got is None) == (want is None), (k, 'None pattern')
        if want is None:
            continue
        if float(want.abs().max()) == 0:
            assert float(got.abs().max()) == 0, (k, 'zero pattern')
            continue
        errs[k] = rel(got.float() / LOSS_SCALE[dtype], want)
    for k, e in errs.items():
        print(f'{str(dtype)[6:]} {k}: rel-L2 {e:.3e}  bound {2 * drift[k]:.3e}')
    bad = {k: (e, 2 * drift[k]) for k, e in errs.items() if not e <= 2 * drift[k]}
    del model, gap, logits, loss, pm
    torch.cuda.empty_cache()
    assert not bad, f'{len(bad)} of {len(errs)} tensors over 2x the oracle drift: {bad}'
