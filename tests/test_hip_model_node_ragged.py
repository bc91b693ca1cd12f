"""TGT_NODE_RAGGED (tgt_amd/tgt/stack.py: the per-graph node counts also go to node attention, and bound the rows of the mask as
well as its columns) on a whole model, on the GPU.  The model and batch of tests/test_hip_model_ragged.py: a 2-layer TGT-At at
edge width 256 / 16 triplet heads on a 4-graph batch padded to 12 nodes with num_nodes = [12, 5, 9, 1], fp32 and bf16 autocast.
At its 4 node heads node attention runs the lane-per-head kernels, which take the count and ignore it: the case `heads32` is the
same model at node width 256 / 32 heads, whose bf16 node attention runs the families that honour it (key-blocked forward, MFMA32
backward).
With TGT_TRI_RAGGED + TGT_NODE_RAGGED on, H_hat at padded pairs is zero instead of a finite value; everything a user reads -- the
loss, every parameter gradient, the outputs on real nodes and real edges -- must equal the run with both off bit for bit, because
a padded position reaches a real one only through keys the mask closes and receives a cotangent of exactly zero."""
import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu

GEOM = dict(B=4, N=12, num_nodes=[12, 5, 9, 1])
CFG = dict(gu.MODEL_CASES['multi_at_tiny'][1], model_height=2, node_width=64, edge_width=256, num_heads=4, triplet_heads=16)
CFG_H32 = dict(CFG, node_width=256, num_heads=32)


@pytest.fixture(autouse=True)
def small_rows(monkeypatch):
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_TRI_PROJ', True)
    monkeypatch.setattr(ops, '_TRI_PROJ_INFER', True)
    monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 1)            # (the projection-fused kernel also below 65536 edge rows)


class _Spy:
    """the node counts every node attention launch and every triplet attention launch of a forward was given"""

    def __init__(self, monkeypatch):
        from tgt_amd import ops
        self.node, self.tri = [], []
        real_node, real_tri = ops.node_attention, ops.projected_triplet_attention

        def node(*args, **kw):
            self.node.append(kw.get('node_counts'))
            return real_node(*args, **kw)

        def tri(*args, **kw):
            self.tri.append(kw.get('node_counts'))
            return real_tri(*args, **kw)
        monkeypatch.setattr(ops, 'node_attention', node)
        monkeypatch.setattr(ops, 'projected_triplet_attention', tri)


def _switch(monkeypatch, on):
    from tgt_amd.tgt import stack
    monkeypatch.setattr(stack, '_TRI_RAGGED', on)
    monkeypatch.setattr(stack, '_NODE_RAGGED', on)


def _model(train, cfg=CFG, cls='TGT_Multi'):
    from tgt_amd import pcqm
    m = gu.fill_params(getattr(pcqm, cls)(**cfg), seed=31).cuda()
    return m.train() if train else m.eval()


def _batch(seed=32):
    return {k: v.cuda() for k, v in gu.model_batch(GEOM, seed=seed).items()}


def _pretrain_loss(out, batch):
    from tgt_amd.training.step import pretrain_loss, StepConfig
    return pretrain_loss(out, batch, StepConfig(num_dist_bins=CFG['num_dist_bins'], mixed_precision=None))


def _step(model, batch, autocast, loss_of=_pretrain_loss):
    model.zero_grad(set_to_none=True)
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
        out = model(batch)
        loss = loss_of(out, batch)
    loss.backward()
    torch.cuda.synchronize()
    out = out if isinstance(out, (tuple, list)) else [out]
    return loss.detach(), [o.detach() for o in out], {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('cfg,autocast', [(CFG, False), (CFG, True), (CFG_H32, True)], ids=['fp32', 'bf16', 'bf16-heads32'])
def test_training_step_is_bit_identical_with_the_switches_on(cfg, autocast, monkeypatch):
    model, batch = _model(True, cfg), _batch()
    spy = _Spy(monkeypatch)
    layers = cfg['model_height']
    _switch(monkeypatch, False)
    loss0, out0, grads0 = _step(model, batch, autocast)
    assert spy.node == [None] * layers and spy.tri == [None] * layers
    _switch(monkeypatch, True)
    loss1, out1, grads1 = _step(model, batch, autocast)
    given = spy.node[layers:]
    assert len(given) == layers and all(c is given[0] for c in given)                   # ONE count tensor per forward, at every layer
    assert given[0].dtype == torch.int32 and given[0].tolist() == GEOM['num_nodes']
    assert all(c is given[0] for c in spy.tri[layers:])                                 # ... and the triplet modules get the same one
    assert torch.equal(loss1, loss0), (float(loss1), float(loss0))
    em = batch['edge_mask'].bool()
    assert torch.equal(out1[0], out0[0])                                                # gap: one value per graph
    assert torch.equal(out1[1][em], out0[1][em])                                        # distance logits on the real edges
    assert grads1.keys() == grads0.keys() and len(grads0) > 20
    bad = [k for k in grads0 if not torch.equal(grads1[k], grads0[k])]
    assert not bad, bad
    assert any('update.lin_EG' in k for k in grads0)


def test_heads32_model_runs_the_families_that_honour_the_count():
    """the `heads32` model's node attention call, as ops.node_attention describes it: key-blocked forward, MFMA32 backward"""
    import node_family_cases as nfc
    B, N, W, H = GEOM['B'], GEOM['N'], CFG_H32['node_width'], CFG_H32['num_heads']
    got = (nfc.shape_family((B, N, W, H), torch.bfloat16, 0), nfc.shape_family((B, N, W, H), torch.bfloat16, 1))
    assert got == (nfc.family_id('KB_FWD'), nfc.family_id('MFMA32'))


def test_a_callers_own_counts_are_used_as_given(monkeypatch):
    model, batch = _model(False), _batch()
    own = torch.tensor(GEOM['num_nodes'], dtype=torch.int32, device='cuda')
    spy = _Spy(monkeypatch)
    _switch(monkeypatch, True)
    with torch.no_grad():
        model(dict(batch, node_counts=own))
    torch.cuda.synchronize()
    assert all(c is not None and c.data_ptr() == own.data_ptr() for c in spy.node + spy.tri)


def test_node_ragged_needs_tri_ragged(monkeypatch):
    from tgt_amd.tgt import stack
    model, batch = _model(False), _batch()
    spy = _Spy(monkeypatch)
    monkeypatch.setattr(stack, '_TRI_RAGGED', False)
    monkeypatch.setattr(stack, '_NODE_RAGGED', True)
    with torch.no_grad():
        model(batch)
    torch.cuda.synchronize()
    assert spy.node == [None] * CFG['model_height']


def test_the_aggregate_family_gets_no_counts_in_node_attention(monkeypatch):
    """TGT-Agx2 (triplet aggregate: its gated outward direction is unmasked, padded edge rows reach real outputs, and H_hat at padded
    pairs is such a row): the knob has no effect -- node attention gets no counts, one notice says so, and the step is the knob-off
    step bit for bit, padded positions included"""
    from tgt_amd import ops
    name, kwargs, _ = gu.MODEL_CASES['dist_agx2_tiny']
    cfg = dict(kwargs, model_height=2, node_width=64, edge_width=256, num_heads=4, triplet_heads=16)
    model, batch = _model(True, cfg, name), _batch()

    def loss_of(out, batch):
        o = out[-1] if isinstance(out, (tuple, list)) else out
        return (o.float() * batch['edge_mask'].reshape(o.shape[:3] + (1,) * (o.ndim - 3)).float()).square().mean()
    _switch(monkeypatch, False)
    loss0, out0, grads0 = _step(model, batch, True, loss_of)
    _switch(monkeypatch, True)
    monkeypatch.setattr(ops, '_slow_path_said', set())
    spy = _Spy(monkeypatch)
    with pytest.warns(RuntimeWarning, match='TGT_NODE_RAGGED has no effect'):
        loss1, out1, grads1 = _step(model, batch, True, loss_of)
    assert spy.node and all(c is None for c in spy.node)
    assert torch.equal(loss1, loss0) and all(torch.equal(a, b) for a, b in zip(out1, out0))
    assert all(torch.equal(grads1[k], grads0[k]) for k in grads0)


def test_eval_forward_and_graphed_replay(monkeypatch):
    """eval mode, no_grad, bf16 autocast on the `heads32` model: switches on = switches off on the real positions; and the captured
    forward (GraphedForward: the count launches are part of the graph) replays to the eager result with the switches on."""
    from tgt_amd.pcqm.graphed import GraphedForward
    model = _model(False, CFG_H32)
    b0, b1 = _batch(32), _batch(33)

    def eager(b):
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            out = model(b)
        torch.cuda.synchronize()
        return [o.clone() for o in out]
    _switch(monkeypatch, False)
    off = eager(b0)
    _switch(monkeypatch, True)
    spy = _Spy(monkeypatch)
    on = eager(b0)
    assert len(spy.node) == CFG_H32['model_height'] and all(c is not None for c in spy.node)
    em = b0['edge_mask'].bool()
    assert torch.equal(on[0], off[0]) and torch.equal(on[1][em], off[1][em])
    gf = GraphedForward(model, b0, autocast_dtype=torch.bfloat16, warmup=1)
    assert all(c is not None for c in spy.node)
    for b in (b1, b0):
        want = eager(b)
        got = gf(b)
        torch.cuda.synchronize()
        assert all(torch.equal(g, w) for g, w in zip(got, want))
