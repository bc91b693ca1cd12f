"""TriangularUpdate (`triplet_type: tiangular_update`, the reference factory's spelling) inside TGT layers and task models, on
the GPU, against the oracle model of the same parameters in float64.

  fp32   tests/test_hip_model.py's bars: 3e-4 outputs and loss, 2e-3 probed parameter gradients.
  bf16   per tensor 2 x the ORACLE's own drift on this very case -- its rel-L2 under torch.autocast('cpu', bfloat16) against its
         float64 run, computed here (the quantity tools/make_golden.py::bf16_drift_cases records for the existing cases) -- with
         the absolute floors of tests/test_hip_model.py for `gap` (3e-2) and `loss` (1e-3).  The same bars for the fused path
         (tiled core + gated output stage) and for the compositions (both knobs off).
profiles/parity_errors_triupd.json records the measured errors (TGT_PARITY_LOG)."""
import pytest
import torch

import golden_util as gu
import parity_log
from oracle import core, modules as om

pytestmark = pytest.mark.gpu

TRIUPD = 'tiangular_update'
TINY_MULTI = dict(gu.MODEL_CASES['multi_at_tiny'][1], triplet_type=TRIUPD)
TINY_DIST = dict(gu.MODEL_CASES['dist_agx2_tiny'][1], triplet_type=TRIUPD)
TINY_GEOM = gu.MODEL_CASES['multi_at_tiny'][2]
# two layers at the edge width and head count the fused kernels take (C = 256, 2H = 32), N = 12: 432 edge rows = 14 row tiles
WIDE = dict(TINY_MULTI, model_height=2, edge_width=256, triplet_heads=16)
WIDE_GEOM = dict(B=3, N=12, num_nodes=[12, 9, 5])
PROBES = gu.GRAD_PROBE_KEYS + ['encoder.TGT_layers.0.tria.lin_E.weight', 'encoder.TGT_layers.0.tria.lin_V.bias',
                               'encoder.TGT_layers.0.tria.lin_O.bias', 'encoder.TGT_layers.1.tria.lin_V.weight']
NEW_ENTRIES = {'tgt_triangular_update_tiled_fwd', 'tgt_triangular_update_tiled_bwd', 'tgt_edge_gated_out_fwd', 'tgt_edge_gated_out_bwd'}
FLOORS = dict(gap=3e-2, loss=1e-3)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return parity_log.record(float((a - b).norm() / (b.norm() + 1e-30)))


def oracle_run(cls_name, kwargs, cpu, seed, autocast=False):
    """{gap, logits, loss, pgrad.*} of the oracle model: float64, or float32 parameters under CPU bf16 autocast"""
    model = gu.fill_params(getattr(om, cls_name)(**kwargs), seed=seed).train()
    if not autocast:
        model = model.double()
        cpu = {k: (v.double() if v.is_floating_point() else v) for k, v in cpu.items()}
    bins = kwargs['num_dist_bins']
    with torch.autocast('cpu', dtype=torch.bfloat16, enabled=autocast):
        out = model(cpu)
        if cls_name == 'TGT_Multi':
            res = dict(gap=out[0], logits=out[1])
            loss = torch.nn.functional.l1_loss(out[0], cpu['target']) + 0.1 * core.binned_distance_xent(
                out[1], core.pairwise_dist(cpu['dft_coords']), cpu['edge_mask'], bins, 8)
        else:
            res = dict(logits=out)
            loss = core.binned_distance_xent(out, core.pairwise_dist(cpu['dft_coords']), cpu['edge_mask'], bins, 8)
    res['loss'] = loss
    loss.backward()
    named = dict(model.named_parameters())
    res.update({'pgrad.' + k: named[k].grad for k in PROBES if k in named and named[k].grad is not None})
    return {k: v.detach().clone() for k, v in res.items()}


def product_run(cls_name, kwargs, cpu, seed, autocast_dtype=None):
    from tgt_amd import pcqm
    from tgt_amd.training.step import pretrain_loss, binned_distance_loss, coords2dist, StepConfig
    model = gu.fill_params(getattr(pcqm, cls_name)(**kwargs), seed=seed).cuda().train()
    batch = {k: v.cuda() for k, v in cpu.items()}
    cfg = StepConfig(num_dist_bins=kwargs['num_dist_bins'], range_dist_bins=8, dist_loss_weight=0.1)
    ctx = torch.autocast('cuda', dtype=autocast_dtype) if autocast_dtype is not None else torch.autocast('cuda', enabled=False)
    with ctx:
        out = model(batch)
        if cls_name == 'TGT_Multi':
            res = dict(gap=out[0], logits=out[1])
            loss = pretrain_loss(out, batch, cfg)
        else:
            res = dict(logits=out)
            loss = binned_distance_loss(out, coords2dist(batch['dft_coords']), batch['edge_mask'], cfg.num_dist_bins, 8)
    res['loss'] = loss
    loss.backward()
    torch.cuda.synchronize()
    named = dict(model.named_parameters())
    res.update({'pgrad.' + k: named[k].grad for k in PROBES if k in named and named[k].grad is not None})
    return res


def test_layer_type_is_the_module():
    from tgt_amd.tgt.layers import blocks, triplet
    layer = blocks.TGT_Layer(node_width=48, edge_width=32, num_heads=4, triplet_heads=4, triplet_type=TRIUPD)
    assert type(layer.tria) is triplet.TriangularUpdate


@pytest.mark.parametrize('cls_name,kwargs', [('TGT_Multi', TINY_MULTI), ('TGT_Distance', TINY_DIST)], ids=['multi', 'distance_x2'])
def test_tiny_model_fp32_matches_the_oracle(cls_name, kwargs):
    """three layers (TGT_Distance: a weight-shared stack applied twice), fp32, through the compositions and the existing kernel"""
    cpu = gu.model_batch(TINY_GEOM, seed=711)
    ref = oracle_run(cls_name, kwargs, cpu, seed=710)
    got = product_run(cls_name, kwargs, cpu, seed=710)
    assert set(got) == set(ref) and any(k.startswith('pgrad.encoder.TGT_layers.1.tria') for k in ref)
    parity_log.Tol.last = 'fp32-model'
    for k, t in got.items():
        tol = 2e-3 if k.startswith('pgrad.') else 3e-4
        assert torch.isfinite(t).all(), k
        assert rel(t, ref[k]) < tol, (k, rel(t, ref[k]), tol)


_wide = {}


def wide_case():
    """(batch on the CPU, float64 oracle results, the oracle's bf16-autocast drift per tensor): computed once, shared"""
    if not _wide:
        cpu = gu.model_batch(WIDE_GEOM, seed=721)
        exact = oracle_run('TGT_Multi', WIDE, cpu, seed=720)
        low = oracle_run('TGT_Multi', WIDE, cpu, seed=720, autocast=True)
        drift = {k: float((low[k].double() - exact[k]).norm() / (exact[k].norm() + 1e-30)) for k in exact}
        print('oracle bf16-autocast drift:', {k[-36:]: f'{v:.2e}' for k, v in drift.items()})
        _wide.update(cpu=cpu, exact=exact, drift=drift)
    return _wide['cpu'], _wide['exact'], _wide['drift']


@pytest.fixture
def small_rows(monkeypatch):
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)
    monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 1)


@pytest.mark.parametrize('knobs_on', [True, False], ids=['fused', 'composed'])
def test_wide_model_bf16_within_twice_the_oracles_drift(knobs_on, small_rows, monkeypatch):
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_TRIUPD_TILED', knobs_on)
    monkeypatch.setattr(ops, '_TRIUPD_GATED', knobs_on)
    cpu, exact, drift = wide_case()
    prof = ops.profile_kernels(True)
    try:
        got = product_run('TGT_Multi', WIDE, cpu, seed=720, autocast_dtype=torch.bfloat16)
    finally:
        ops.profile_kernels(False)
    ran = NEW_ENTRIES & set(prof)
    assert ran == (NEW_ENTRIES if knobs_on else set()), ran
    if knobs_on:
        assert all(len(prof[k]) == 2 for k in NEW_ENTRIES), {k: len(prof[k]) for k in NEW_ENTRIES}      # once per layer
    assert set(got) == set(exact)
    parity_log.Tol.last = 'bf16-model'
    errs = {}
    for k, t in got.items():
        assert torch.isfinite(t).all(), k
        errs[k] = (rel(t, exact[k]), max(2.0 * drift[k], FLOORS.get(k, 0.0)))
    print('fused' if knobs_on else 'composed', {k[-36:]: f'{e:.2e} < {b:.2e}' for k, (e, b) in errs.items()})
    bad = {k: v for k, v in errs.items() if not v[0] < v[1]}
    assert not bad, bad


def trainer_grads(knobs_on, monkeypatch):
    from tgt_amd import ops, pcqm
    from tgt_amd.training.step import Trainer, StepConfig, preprocess_batch
    from tgt_amd.training.synthetic import make_batch
    monkeypatch.setattr(ops, '_TRIUPD_TILED', knobs_on)
    monkeypatch.setattr(ops, '_TRIUPD_GATED', knobs_on)
    cfg = StepConfig(num_dist_bins=WIDE['num_dist_bins'], mixed_precision='bf16', coords_noise=0.0)
    model = gu.fill_params(pcqm.TGT_Multi(**WIDE), seed=730).cuda().train()
    tr = Trainer(model, cfg)
    batch = preprocess_batch(make_batch(3, 12, seed=731, ragged=True), 'cuda', cfg, add_noise=False)
    prof = ops.profile_kernels(True)
    try:
        _, loss = tr.compute_gradients(batch)
        torch.cuda.synchronize()
    finally:
        ops.profile_kernels(False)
    index = {id(p): i for i, p in enumerate(tr.flat.params)}
    grads = {k: tr.flat.grad_views[index[id(p)]].clone() for k, p in model.named_parameters()}
    return float(loss), grads, set(prof)


def test_trainer_step_with_the_knobs_on(small_rows, monkeypatch):
    """one Trainer step (bf16, flat gradient buffer): every parameter gets a finite gradient, and those of the module's three
    Linears agree with the knobs-off step within the gradient bar (twice the bf16 bar of 8e-3)"""
    loss_on, on, ran_on = trainer_grads(True, monkeypatch)
    loss_off, off, ran_off = trainer_grads(False, monkeypatch)
    assert NEW_ENTRIES <= ran_on and not (NEW_ENTRIES & ran_off)
    assert abs(loss_on - loss_off) < 1e-3 * abs(loss_off) + 1e-3, (loss_on, loss_off)
    assert set(on) == set(off)
    for k, g in on.items():
        assert torch.isfinite(g).all(), k
    tria = [k for k in on if '.tria.lin_' in k]
    assert len(tria) == 2 * 3 * 2                   # 2 layers x (lin_E, lin_V, lin_O) x (weight, bias)
    parity_log.Tol.last = 'bfloat16'
    for k in tria:
        assert float(on[k].abs().max()) > 0, k
        assert rel(on[k], off[k]) < 2 * 8e-3, (k, rel(on[k], off[k]))


def test_graphed_forward_replays_the_eager_forward(small_rows, monkeypatch):
    from tgt_amd import ops, pcqm
    from tgt_amd.pcqm.graphed import GraphedForward
    monkeypatch.setattr(ops, '_TRIUPD_TILED', True)
    monkeypatch.setattr(ops, '_TRIUPD_GATED', True)
    model = gu.fill_params(pcqm.TGT_Multi(**WIDE), seed=740).cuda().eval()
    b0 = {k: v.cuda() for k, v in gu.model_batch(WIDE_GEOM, seed=741).items()}
    b1 = {k: v.cuda() for k, v in gu.model_batch(WIDE_GEOM, seed=742).items()}
    gf = GraphedForward(model, b0, autocast_dtype=torch.bfloat16, warmup=1)
    for b in (b1, b0):
        prof = ops.profile_kernels(True)
        try:
            with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
                want = model(b)
        finally:
            ops.profile_kernels(False)
        assert {'tgt_triangular_update_tiled_fwd', 'tgt_edge_gated_out_fwd'} <= set(prof)
        got = gf(b)
        torch.cuda.synchronize()
        assert all(torch.isfinite(w_).all() for w_ in want)
        assert all(torch.equal(g, w_) for g, w_ in zip(got, want))
