"""MC-dropout prediction as hipGraph replays (tgt_amd/pcqm/graphed.py: GraphedForward(stochastic=True), GraphedSampler; the
`graphed=` forms of tgt_amd/pcqm/predict.py) and the captured training step with attention dropout
(GraphedTrainingStep(attention_dropout=True)).

Every comparison is bitwise: a replay runs the kernels of the eager graph-safe forward with the same arguments, the same device
counter value and the same state of torch's generator (both runs start from one torch.manual_seed and perform the same number of
warm-up forwards) -- the recipe of tests/test_hip_trainer.py::_graphed_equals_eager."""
import gc

import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu

GEOM = dict(B=3, N=7, num_nodes=[7, 5, 3])
NOISE = dict(source_dropout=0.3, drop_path=0.1, node_act_dropout=0.1, edge_act_dropout=0.1, triplet_dropout=0.1)
BF16 = torch.bfloat16
WARMUP = 2


def _model(name, seed=32, **kw):
    from tgt_amd import pcqm
    cls, kwargs, _ = gu.MODEL_CASES[name]
    return gu.fill_params(getattr(pcqm, cls)(**dict(kwargs, **NOISE, **kw)), seed=seed).cuda().train()


def _batch(seed, geom=GEOM):
    b = {k: v.cuda() for k, v in gu.model_batch(geom, seed=seed).items()}
    b['num_nodes'] = torch.tensor(geom['num_nodes']).cuda()
    return b


def _clone(out):
    return tuple(t.clone() for t in out) if isinstance(out, (tuple, list)) else (out.clone(),)


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _start():
    from tgt_amd import ops
    torch.manual_seed(77)
    ops.reset_random_pools()


class _EagerGraphSafe:
    """the eager side of a comparison: graph-safe mode with a counter of its own, WARMUP forwards, then model-like calls"""

    def __init__(self, model, example, autocast_dtype=BF16):
        self.model, self.dt, self.example = model, autocast_dtype, example

    def __enter__(self):
        from tgt_amd import ops
        self.counter = torch.zeros(1, dtype=torch.int64, device='cuda')
        ops.graph_safe_rng(True)
        ops.set_seed_counter(self.counter)
        for _ in range(WARMUP):
            self(self.example)
        return self

    def __call__(self, batch):
        from tgt_amd.pcqm.graphed import eager_graph_safe_forward
        with torch.no_grad(), torch.autocast('cuda', dtype=self.dt):
            return eager_graph_safe_forward(self.model, self.counter, batch)

    def __exit__(self, *exc):
        from tgt_amd import ops
        ops.set_seed_counter(None)
        ops.graph_safe_rng(False)
        return False


def _restore():
    from tgt_amd import ops
    ops.set_seed_counter(None)
    ops.graph_safe_rng(False)


@pytest.mark.parametrize('name', ['dist_agx2_tiny', 'multi_at_tiny'])
def test_replays_equal_the_eager_graph_safe_forward_and_differ_from_each_other(name):
    """three sample() calls on one batch and one on a second batch == the eager graph-safe sequence, bit for bit; the three
    replays of one batch are pairwise different (every replay draws anew)"""
    from tgt_amd.pcqm.graphed import GraphedForward
    b0, b1 = _batch(41), _batch(42)
    runs = []
    try:
        for graphed in (False, True):
            _start()
            m = _model(name)
            if graphed:
                with GraphedForward(m, b0, autocast_dtype=BF16, warmup=WARMUP, stochastic=True) as gf:
                    gf.load(b0)
                    outs = [_clone(gf.sample()) for _ in range(3)] + [_clone(gf(b1))]
                    assert int(gf.counter) == WARMUP + 4
            else:
                with _EagerGraphSafe(m, b0) as eager:
                    outs = [_clone(eager(b)) for b in (b0, b0, b0, b1)]
            runs.append(outs)
    finally:
        _restore()
    assert all(torch.isfinite(t).all() for o in runs[0] for t in o)
    for want, got in zip(*runs):
        assert _same(want, got)
    a, b, c = runs[1][:3]
    assert not _same(a, b) and not _same(a, c) and not _same(b, c)


def test_mode_bookkeeping(monkeypatch):
    """the mode flags while open and after close(); a second stochastic owner raises; a capture that raises gives the mode back; a
    dropped owner gives it back; stochastic=False on the same model still refuses"""
    from tgt_amd import ops
    from tgt_amd.pcqm import graphed
    b0 = _batch(41)
    m = _model('dist_agx2_tiny')
    try:
        with pytest.raises(RuntimeError, match='train mode'):
            graphed.GraphedForward(m, b0)
        with pytest.raises(RuntimeError, match='train mode'):
            graphed.GraphedForward(m, b0, stochastic=False)
        assert not ops._GRAPH_SAFE[0] and ops._seed_counter[0] is None
        with graphed.GraphedForward(m, b0, autocast_dtype=BF16, warmup=1, stochastic=True) as gf:
            assert ops._GRAPH_SAFE[0] and ops._seed_counter[0] is gf.counter
            with pytest.raises(RuntimeError, match='already has an owner'):
                graphed.GraphedForward(m, b0, autocast_dtype=BF16, warmup=1, stochastic=True)
            assert ops._GRAPH_SAFE[0] and ops._seed_counter[0] is gf.counter         # (not taken over, not switched off)
            with pytest.raises(RuntimeError):                                          # the shape checks of load()
                gf.load({k: (v[:2] if k == 'node_mask' else v) for k, v in b0.items()})
            with pytest.raises(RuntimeError, match='keys'):
                gf.load({k: v for k, v in b0.items() if k != 'node_mask'})
            gf(b0)
        assert not ops._GRAPH_SAFE[0] and ops._seed_counter[0] is None
        with pytest.raises(RuntimeError, match='closed'):
            gf.sample()

        calls = [0]
        real = graphed.GraphedForward._body

        def failing(self):
            calls[0] += 1
            if calls[0] == 2:                         # the warm-up forward passes, the capture raises
                raise RuntimeError('boom inside the capture')
            return real(self)
        monkeypatch.setattr(graphed.GraphedForward, '_body', failing)
        with pytest.raises(RuntimeError, match='boom'):
            graphed.GraphedForward(m, b0, autocast_dtype=BF16, warmup=1, stochastic=True)
        assert not ops._GRAPH_SAFE[0] and ops._seed_counter[0] is None
        monkeypatch.setattr(graphed.GraphedForward, '_body', real)
        torch.cuda.synchronize()

        gf = graphed.GraphedForward(m, b0, autocast_dtype=BF16, warmup=1, stochastic=True)
        assert ops._GRAPH_SAFE[0]
        del gf                                        # dropped without close()
        gc.collect()
        assert not ops._GRAPH_SAFE[0] and ops._seed_counter[0] is None
    finally:
        _restore()


@pytest.mark.parametrize('kind', ['bins', 'probs'])
def test_graphed_predict_bins_and_probs_equal_the_eager_graph_safe_form(kind):
    from tgt_amd.pcqm import predict as pp
    from tgt_amd.pcqm.graphed import GraphedSampler
    S = 3
    b0, b1 = _batch(41), _batch(42)
    call = (lambda model, b, **kw: pp.predict_bins(model, b, S, **kw)) if kind == 'bins' else \
        (lambda model, b, **kw: pp.predict_probs(model, b, S, **kw))
    runs = []
    try:
        for graphed in (False, True):
            _start()
            m = _model('dist_agx2_tiny')
            if graphed:
                with GraphedSampler(m, b0, S, kind, autocast_dtype=BF16, warmup=WARMUP) as gs:
                    outs = [call(m, b1, graphed=gs), call(m, b0, graphed=gs)]        # (one capture, two batches)
                    assert int(gs.counter) == WARMUP + 2 * S and int(gs.state[0]) == S
                    with pytest.raises(RuntimeError, match='captured for'):
                        pp.predict_bins(m, b0, S + 1, graphed=gs)
            else:
                with _EagerGraphSafe(m, b0) as eager:
                    outs = [call(eager, b1), call(eager, b0)]
            runs.append(outs)
    finally:
        _restore()
    for want, got in zip(*runs):
        assert want.shape == got.shape and want.dtype == got.dtype
        assert torch.equal(want, got)
    out = runs[1][0]
    if kind == 'bins':
        assert out.shape == (3, S, 7, 7) and out.dtype == torch.uint8
        assert (out == out.transpose(-1, -2)).all()                                   # symmetrised probabilities
        assert len({out[:, s].cpu().numpy().tobytes() for s in range(S)}) == S        # every sample drew anew
    else:
        assert out.shape == (3, 7, 7, 24) and torch.isfinite(out).all()
        assert torch.equal(out, out.transpose(1, 2))
    assert not torch.equal(runs[1][0], runs[1][1])


def test_graphed_gap_prediction_step_equals_eager_and_cycles_the_inputs():
    """(B, 2, N, N) dist_input at S = 3: the graphed gap_pred == the eager graph-safe one, and sample v used input v % 2 -- the
    same run on the three inputs (d0, d1, d0), where sample v uses input v, gives the same predictions"""
    from tgt_amd.pcqm import predict as pp
    from tgt_amd.pcqm.graphed import GraphedSampler
    S = 3
    base = _batch(41)
    d = base['dist_input']
    two = dict(base, dist_input=torch.stack([d, d * 1.25 + 0.1], 1))
    three = dict(base, dist_input=torch.stack([d, d * 1.25 + 0.1, d], 1))
    runs = []
    try:
        for mode in ('eager', 'graphed', 'eager3'):
            _start()
            m = _model('gap_at_tiny', seed=33)
            if mode == 'graphed':
                with GraphedSampler(m, two, S, 'gap', autocast_dtype=BF16, warmup=WARMUP) as gs:
                    res = pp.gap_prediction_step(m, two, S, graphed=gs)
                    assert int(gs.state[0]) == S and int(gs.state[2]) == S
            else:
                b = two if mode == 'eager' else three
                # (which input a warm-up forward runs on does not matter: it only advances the counter and torch's generator)
                with _EagerGraphSafe(m, dict(b, dist_input=b['dist_input'][:, 0])) as eager:
                    res = pp.gap_prediction_step(eager, b, S)
            assert res['gap_pred'].shape == (3, S) and torch.isfinite(res['gap_pred']).all()
            assert torch.equal(res['gap_target'], base['target'])
            runs.append(res['gap_pred'].clone())
    finally:
        _restore()
    assert torch.equal(runs[0], runs[1])
    assert torch.equal(runs[0], runs[2])
    assert not torch.equal(runs[1][:, 0], runs[1][:, 2])          # same input, another draw


def test_graphed_two_stage_predict_fp16():
    """the shapes of tests/test_hip_predict.py::test_two_stage_inference_on_models_fp16 with both stages as graph replays (two
    samplers on one counter)"""
    from tgt_amd import ops
    from tgt_amd.pcqm import TGT_Distance, TGT_Gap, predict as pp
    from tgt_amd.pcqm.graphed import GraphedSampler
    dk = dict(gu.MODEL_CASES['dist_agx2_tiny'][1], **NOISE)
    gk = dict(gu.MODEL_CASES['gap_at_tiny'][1], **NOISE)
    gk.update(embed_3d_type='gaussian', triplet_type='aggregate', layer_multiplier=2)
    geom = dict(B=4, N=9, num_nodes=[9, 6, 9, 4])
    batch = _batch(31, geom)
    d_hip = gu.fill_params(TGT_Distance(**dk), seed=32).cuda().train()
    g_hip = gu.fill_params(TGT_Gap(**gk), seed=33).cuda().train()
    S, nbins = 3, dk['num_dist_bins']
    try:
        with GraphedSampler(d_hip, batch, S, 'bins', autocast_dtype=torch.float16, warmup=1) as g_bins:
            gap_example = dict(batch, dist_input=batch['dist_input'].float().unsqueeze(1).repeat(1, S, 1, 1))
            with GraphedSampler(g_hip, gap_example, S, 'gap', autocast_dtype=torch.float16, warmup=1, counter=g_bins.counter) as g_gap:
                assert ops._seed_counter[0] is g_bins.counter
                bins, gap = pp.two_stage_predict(d_hip, g_hip, batch, S, nbins, 8, autocast_dtype=torch.float16,
                                                 graphed=(g_bins, g_gap))
                with pytest.raises(RuntimeError, match='autocast'):
                    pp.two_stage_predict(d_hip, g_hip, batch, S, nbins, 8, autocast_dtype=BF16, graphed=(g_bins, g_gap))
            assert ops._seed_counter[0] is g_bins.counter and ops._GRAPH_SAFE[0]      # the borrower does not hand the mode back
        assert ops._seed_counter[0] is None and not ops._GRAPH_SAFE[0]
    finally:
        _restore()
    assert bins.shape == (4, S, 9, 9) and gap.shape == (4, S) and torch.isfinite(gap).all()
    assert (bins == bins.transpose(-1, -2)).all()
    assert len({bins[:, s].cpu().numpy().tobytes() for s in range(S)}) > 1


def test_graphed_training_step_with_attention_dropout_equals_eager():
    """FULL_AT_CFG at two layers with triplet_dropout = 0.1: parameters after 3 warm-up steps and 3 replays == the eager graph-safe
    trainer, bit for bit; two replays of one batch give different losses"""
    from tgt_amd import ops
    from tgt_amd.pcqm import TGT_Multi
    from tgt_amd.training.step import Trainer, StepConfig, preprocess_batch
    from tgt_amd.training.synthetic import make_batch
    from tgt_amd.training.graphed import GraphedTrainingStep, GraphedStepCache
    kwargs = dict(gu.FULL_AT_CFG, model_height=2, source_dropout=0.3, drop_path=0.2, node_act_dropout=0.1, edge_act_dropout=0.1,
                  triplet_dropout=0.1)
    cfg = StepConfig(num_dist_bins=512, mixed_precision='bf16', coords_noise=0.0, lr_warmup_steps=4, lr_total_steps=100)
    batches = [preprocess_batch(make_batch(3, 7, seed=40 + s, ragged=True), 'cuda', cfg, add_noise=False) for s in range(2)]
    order = [batches[1], batches[0], batches[0]]
    runs, losses = [], []
    try:
        for graphed in (False, True):
            _start()
            m = gu.fill_params(TGT_Multi(**kwargs), seed=3).cuda().train()
            with Trainer(m, cfg) as tr:
                if graphed:
                    with pytest.raises(RuntimeError, match='attention dropout'):      # the default stays the refusal
                        GraphedTrainingStep(tr, batches[0], warmup=1)
                    with pytest.raises(RuntimeError, match='attention dropout'):
                        GraphedStepCache(tr, warmup=1)
                    with GraphedTrainingStep(tr, batches[0], warmup=3, attention_dropout=True) as gs:
                        for b in order:
                            losses.append(float(gs.step(b)[1]))
                        assert gs.replays == 3 and int(gs.counter) == 6
                else:
                    ctr = torch.zeros(1, dtype=torch.int64, device='cuda')
                    ops.graph_safe_rng(True)
                    ops.set_seed_counter(ctr)
                    tr.set_device_lr(True)
                    for b in [batches[0]] * 3 + order:
                        tr.global_step += 1
                        tr.write_device_lr()
                        ctr.add_(1)
                        tr.compute_gradients(b)
                        tr.apply_gradients()
                    ops.set_seed_counter(None)
                    ops.graph_safe_rng(False)
                runs.append(torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone())
    finally:
        _restore()
    assert torch.isfinite(runs[0]).all()
    assert torch.equal(runs[0], runs[1])
    assert losses[1] != losses[2]                     # one batch, two replays: the drop patterns moved on
