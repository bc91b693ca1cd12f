"""TriangularUpdate models on ragged batches, on the GPU: TGT_TRI_RAGGED hands the per-graph node counts to the tiled core, and
TGT_EDGE_RAGGED / TGT_NODE_RAGGED on top of it now act on such a model (its triplet module takes node counts), the gated output
stage included (tgt_edge_gated_out_fwd_live / _bwd_live).

The model: the WIDE two-layer triangular-update TGT_Multi of tests/test_hip_model_triupd.py (C = 256, 16 triplet heads) on B = 4,
N = 12, num_nodes = [12, 5, 9, 1] (576 edge rows = 18 row tiles, some of them dead), _EDGE_MIN_ROWS = 1 as the existing ragged tests
set it.  What a user reads -- the loss, the outputs on real nodes and edges, every parameter gradient -- must not change:
  * TGT_TRI_RAGGED on against off: torch.equal throughout (a pair with a padded node contributes exact zeros with and without
    counts);
  * TGT_EDGE_RAGGED + TGT_NODE_RAGGED on top: the same, except the gradients that are summed over rows per workgroup and so
    regrouped by the list -- COLSUM_GRADS of tests/test_hip_edge_live.py and lin_O of `tria` (dw_partial / db_partial of the gated
    stage) -- held at that file's 2e-5 * max|off| + 2e-6 (fp32 summation order)."""
import warnings

import pytest
import torch

import golden_util as gu
import parity_log
from test_hip_edge_live import COLSUM_GRADS, _live_tiles_np
from test_hip_model_triupd import WIDE

from tgt_amd import _lib, ops

pytestmark = pytest.mark.gpu

GEOM = dict(B=4, N=12, num_nodes=[12, 5, 9, 1])
ROWS = GEOM['B'] * GEOM['N'] ** 2
REGROUPED = COLSUM_GRADS + ('tria.lin_O.',)
GATED_LIVE = ('tgt_edge_gated_out_fwd_live', 'tgt_edge_gated_out_bwd_live')
GATED_PLAIN = ('tgt_edge_gated_out_fwd', 'tgt_edge_gated_out_bwd')


@pytest.fixture(autouse=True)
def small_rows(monkeypatch):
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)             # the edge row kernels and the gated stage at 576 rows
    monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 1)
    monkeypatch.setattr(ops, '_TRIUPD_TILED', True)
    monkeypatch.setattr(ops, '_TRIUPD_GATED', True)


def _switch(monkeypatch, tri, edge_node=False):
    from tgt_amd.tgt import stack
    monkeypatch.setattr(stack, '_TRI_RAGGED', tri)
    monkeypatch.setattr(stack, '_EDGE_RAGGED', edge_node)
    monkeypatch.setattr(stack, '_NODE_RAGGED', edge_node)


class _Spy:
    """what the launches of a step were given: the node counts of every core call, the list of every edge_linear_raw call, the
    list pointer of every gated launch, and every notice said"""

    def __init__(self, monkeypatch):
        self.core, self.row_lists, self.gated, self.node = [], [], [], []
        real_core, real_raw, real_launch, real_node = ops.triangular_update_packed, ops.edge_linear_raw, ops._launch, ops.node_attention

        def core(ev, mask3, num_heads, node_counts=None):
            self.core.append(node_counts)
            return real_core(ev, mask3, num_heads, node_counts=node_counts)

        def raw(a, w, bias=None, epilogue=_lib.EPI_BIAS, **kw):
            self.row_lists.append((a.shape[0], kw.get('live')))
            return real_raw(a, w, bias, epilogue, **kw)

        def launch(entry, *args, **kw):
            if entry in GATED_LIVE:
                self.gated.append((entry, args[1].value))
            elif entry in GATED_PLAIN:
                self.gated.append((entry, None))
            return real_launch(entry, *args, **kw)

        def node(*args, **kw):
            self.node.append(kw.get('node_counts'))
            return real_node(*args, **kw)
        monkeypatch.setattr(ops, 'triangular_update_packed', core)
        monkeypatch.setattr(ops, 'edge_linear_raw', raw)
        monkeypatch.setattr(ops, '_launch', launch)
        monkeypatch.setattr(ops, 'node_attention', node)

    def clear(self):
        for l in (self.core, self.row_lists, self.gated, self.node):
            l.clear()


def _model(train, cfg=WIDE, cls='TGT_Multi'):
    from tgt_amd import pcqm
    m = gu.fill_params(getattr(pcqm, cls)(**cfg), seed=31).cuda()
    return m.train() if train else m.eval()


def _batch(seed=32):
    return {k: v.cuda() for k, v in gu.model_batch(GEOM, seed=seed).items()}


def _pretrain_loss(out, batch):
    from tgt_amd.training.step import pretrain_loss, StepConfig
    return pretrain_loss(out, batch, StepConfig(num_dist_bins=WIDE['num_dist_bins'], mixed_precision=None))


def _step(model, batch, autocast, loss_of=_pretrain_loss):
    """-> (loss, outputs, parameter gradients, notices said)"""
    model.zero_grad(set_to_none=True)
    before = set(ops._slow_path_said)
    ops._slow_path_said.clear()                               # (a notice is said once per process: let this step say its own)
    try:
        with warnings.catch_warnings(record=True) as said:
            warnings.simplefilter('always')
            with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
                out = model(batch)
                loss = loss_of(out, batch)
            loss.backward()
            torch.cuda.synchronize()
    finally:
        ops._slow_path_said.update(before)
    out = out if isinstance(out, (tuple, list)) else [out]
    return (loss.detach(), [o.detach() for o in out], {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None},
            [str(w.message) for w in said])


def _same_for_the_user(batch, a, b, regrouped=()):
    """loss, outputs on real nodes / edges and parameter gradients of step a against step b (the switches-off step)"""
    (loss1, out1, grads1, _), (loss0, out0, grads0, _) = a, b
    assert torch.isfinite(loss0) and torch.equal(loss1, loss0), (float(loss1), float(loss0))
    em = batch['edge_mask'].bool()
    assert torch.equal(out1[0], out0[0])                                                # gap: one value per graph
    assert torch.equal(out1[1][em], out0[1][em])                                        # distance logits on the real edges
    assert grads1.keys() == grads0.keys() and len(grads0) > 20
    assert any('tria.lin_E' in k for k in grads0) and any('tria.lin_O.weight' in k for k in grads0)
    bad, held = [], 0
    for k in grads0:
        assert bool(torch.isfinite(grads0[k]).all()) and float(grads0[k].abs().max()) >= 0
        if any(s in k for s in regrouped):
            held += 1
            top = float(grads0[k].abs().max())
            err = float((grads1[k].double() - grads0[k].double()).abs().max())
            parity_log.record(err / (top + 1e-30))
            print(f'{k}: |on - off| max {err:.3e}, max|off| {top:.3e}')
            if not err <= 2e-5 * top + 2e-6:
                bad.append((k, err, top))
        elif not torch.equal(grads1[k], grads0[k]):
            bad.append(k)
    assert not bad, bad
    return held


@pytest.mark.parametrize('autocast', [False, True], ids=['fp32', 'bf16'])
def test_training_step_with_the_switches_on(autocast, monkeypatch):
    model, batch = _model(True), _batch()
    layers = WIDE['model_height']
    spy = _Spy(monkeypatch)
    _switch(monkeypatch, False)
    off = _step(model, batch, autocast)
    assert spy.core == [None] * layers and all(l is None for _, l in spy.row_lists) and spy.node == [None] * layers
    plain = [(GATED_PLAIN[0], None)] * layers + [(GATED_PLAIN[1], None)] * layers      # forwards, then backwards
    assert spy.gated == (plain if autocast else [])
    n_rows_calls = len(spy.row_lists)

    # TGT_TRI_RAGGED alone: the core gets the counts, nothing else changes, every value stays
    spy.clear()
    _switch(monkeypatch, True)
    tri = _step(model, batch, autocast)
    assert len(spy.core) == layers and all(c is spy.core[0] for c in spy.core)          # ONE count tensor per forward
    assert spy.core[0].dtype == torch.int32 and spy.core[0].tolist() == GEOM['num_nodes']
    assert all(l is None for _, l in spy.row_lists) and all(p is None for _, p in spy.gated) and spy.node == [None] * layers
    assert not [m for m in tri[3] if 'has no effect' in m], tri[3]
    _same_for_the_user(batch, tri, off)

    # ... with TGT_EDGE_RAGGED and TGT_NODE_RAGGED on top
    spy.clear()
    _switch(monkeypatch, True, True)
    full = _step(model, batch, autocast)
    assert not [m for m in full[3] if 'has no effect' in m], full[3]                    # the switches act on this model
    assert len(spy.core) == layers and all(c is spy.core[0] for c in spy.core) and spy.core[0].tolist() == GEOM['num_nodes']
    assert len(spy.node) == layers and all(c is spy.core[0] for c in spy.node)          # node attention: the same count tensor
    assert len(spy.row_lists) == n_rows_calls                                           # the same row launches, no other
    if autocast:
        given = [l for _, l in spy.row_lists if l is not None]
        assert given and all(l is given[0] for l in given)                              # ONE list object, forward and backward
        assert isinstance(given[0], ops.EdgeLiveTiles) and given[0].rows == ROWS
        want = _live_tiles_np(GEOM['B'], GEOM['N'], GEOM['num_nodes'])
        assert int(given[0].tiles[0]) == int(want.sum()) < want.size
        # the gated launches: the _live entries, once per layer each way, with the list the row kernels got
        assert sorted(e for e, _ in spy.gated) == sorted(GATED_LIVE * layers), spy.gated
        assert all(p == given[0].tiles.data_ptr() for _, p in spy.gated)
    else:
        assert not spy.gated                                                            # fp32: the compositions, no 16-bit row kernel
    held = _same_for_the_user(batch, full, off, REGROUPED if autocast else ())
    if autocast:
        parity_log.Tol({torch.bfloat16: 2e-5})[torch.bfloat16]
        assert held >= 12


def test_eval_forward_and_graphed_replay(monkeypatch):
    """eval mode, no_grad, bf16 autocast: switches on = switches off on the real positions; and the captured forward
    (GraphedForward: the count and list launches are part of the graph) replays to the eager result with the switches on"""
    from tgt_amd.pcqm.graphed import GraphedForward
    model = _model(train=False)
    b0, b1 = _batch(32), _batch(33)

    def eager(b):
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            out = model(b)
        torch.cuda.synchronize()
        return [o.clone() for o in out]
    _switch(monkeypatch, False)
    off = eager(b0)
    _switch(monkeypatch, True, True)
    spy = _Spy(monkeypatch)
    on = eager(b0)
    assert spy.core and all(c is not None for c in spy.core)
    assert spy.gated and all(e == GATED_LIVE[0] and p is not None for e, p in spy.gated)
    em = b0['edge_mask'].bool()
    assert torch.equal(on[0], off[0]) and torch.equal(on[1][em], off[1][em])
    gf = GraphedForward(model, b0, autocast_dtype=torch.bfloat16, warmup=1)
    for b in (b1, b0):
        want = eager(b)
        got = gf(b)
        torch.cuda.synchronize()
        em = b['edge_mask'].bool()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1][em], want[1][em])


def test_a_callers_own_counts_are_used_as_given(monkeypatch):
    model, batch = _model(False), _batch()
    own = torch.tensor(GEOM['num_nodes'], dtype=torch.int32, device='cuda')
    spy = _Spy(monkeypatch)
    _switch(monkeypatch, True, True)
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        model(dict(batch, node_counts=own))
    torch.cuda.synchronize()
    assert spy.core and all(c is not None and c.data_ptr() == own.data_ptr() for c in spy.core + spy.node)


def test_the_aggregate_family_still_computes_everything(monkeypatch):
    """an aggregate-family model under the three switches: both notices, no list, no counts anywhere, and the step is the
    switches-off step bit for bit"""
    name, kwargs, _ = gu.MODEL_CASES['dist_agx2_tiny']
    cfg = dict(kwargs, model_height=2, node_width=64, edge_width=256, num_heads=4, triplet_heads=16)
    model, batch = _model(True, cfg, name), _batch()

    def loss_of(out, batch):
        o = out[-1] if isinstance(out, (tuple, list)) else out
        return (o.float() * batch['edge_mask'].reshape(o.shape[:3] + (1,) * (o.ndim - 3)).float()).square().mean()
    _switch(monkeypatch, False)
    loss0, out0, grads0, _ = _step(model, batch, True, loss_of)
    _switch(monkeypatch, True, True)
    spy = _Spy(monkeypatch)
    loss1, out1, grads1, said = _step(model, batch, True, loss_of)
    assert any('TGT_EDGE_RAGGED has no effect' in m for m in said) and any('TGT_NODE_RAGGED has no effect' in m for m in said), said
    assert spy.row_lists and all(l is None for _, l in spy.row_lists) and not spy.core and all(c is None for c in spy.node)
    assert torch.equal(loss1, loss0) and all(torch.equal(a, b) for a, b in zip(out1, out0))
    assert grads1.keys() == grads0.keys() and all(torch.equal(grads1[k], grads0[k]) for k in grads0)
