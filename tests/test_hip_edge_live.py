"""Live tile lists of the persistent edge row kernels on the GPU (csrc/edge_live.hip, tgt_edge_linear_live).

The list: tgt_edge_live_tiles against a numpy statement of the predicate (row r = (b, i, j) is dead when i or j is at or past
clamp(node_counts[b], 0, N); a 32-row tile is dead when all its rows are dead or past M).

The kernels: every launch the three 32-row-tile kernels serve (the SIZE_CASES of test_hip_edge_gemm.py that run on them, the
GELU_BWD / LN_BWD epilogues with their column-sum planes, the GLU form) at M = 3 * 20^2 rows with node counts [20, 7, 0]: 38
tiles, 17 live -- tiles straddle node rows and graph boundaries, the uncapped grid has workgroups without a live tile, grid caps
1 and 3 make a workgroup walk many live and many dead tiles.  The operands of the dead tiles are NaN: a single read shows.
  * rows of live tiles: bit-identical to the launch without a list on clean operands (the computation is row-wise; dropout draws
    by absolute element);  rows of dead tiles: zeros in every output;  nothing NaN anywhere (the outputs start as NaN).
  * column sums: colsum_partial regroups rows over workgroups, so the totals are held to the float64 sum of THE SAME TERMS at
    _colsum_close (1e-5 max|want| + 1e-6, the fp32 summation bar of test_hip_edge_gemm.py).  The terms are what the kernel
    adds: GELU_BWD the result as stored; LN_BWD plane 2 the x-gradient as stored, planes 0 / 1 dy * xhat and dy with dy as the
    row kernel holds it -- the GEMM result rounded to the storage type, read back from a residual launch (res = 0) of the same
    k-loop.  (dy from a float64 GEMM differs from that by one 16-bit rounding in a few elements: 2^-8 of one term is far above
    the bar, which is about summation order, not about the GEMM.)  Two runs are torch.equal.

The model: a 2-layer TGT-At with edge width 256 as in test_hip_model_ragged.py, TGT_TRI_RAGGED on, TGT_EDGE_RAGGED on versus off."""
import math

import numpy as np
import pytest
import torch

import golden_util as gu
import parity_log
from test_hip_edge_gemm import SIZE_CASES, _colsum_close, _ln64, _mk

from tgt_amd import _lib, ops

pytestmark = pytest.mark.gpu

B_, N_, COUNTS = 3, 20, [20, 7, 0]
M_ = B_ * N_ * N_
RPS = N_ * N_


def _live_rows_np(B, N, counts):
    """(B N^2,) bool: the numpy statement of the row predicate"""
    n = np.clip(np.asarray(counts, dtype=np.int64), 0, N)
    i = np.arange(N)
    ok = (i[None, :, None] < n[:, None, None]) & (i[None, None, :] < n[:, None, None])
    return ok.reshape(-1)


def _live_tiles_np(B, N, counts):
    """(T,) bool: a tile is live when one of its rows (below M) is"""
    rows = _live_rows_np(B, N, counts)
    T = (rows.size + 31) // 32
    return np.pad(rows, (0, T * 32 - rows.size)).reshape(T, 32).any(1)


def _list(counts, N=N_):
    return ops.edge_live_tiles(torch.tensor(counts, dtype=torch.int32, device='cuda'), N)


@pytest.mark.parametrize('B,N,counts', [(3, 20, [20, 7, 0]), (4, 32, [32, 17, 1, 40]), (2, 48, [33, -3])])
def test_live_tile_list_against_the_numpy_predicate(B, N, counts):
    live = _list(counts, N)
    got = live.tiles.cpu().numpy()
    want = _live_tiles_np(B, N, counts)
    T = want.size
    assert live.rows == B * N * N and got.shape == (1 + T,) and got.dtype == np.int32
    n_live = int(got[0])
    assert n_live == int(want.sum())
    head, tail = got[1:1 + n_live], got[1 + n_live:]
    assert (np.diff(head) > 0).all() and (np.diff(tail) > 0).all()            # both halves ascending
    assert np.array_equal(np.sort(got[1:]), np.arange(T))                       # their union: every tile exactly once
    assert np.array_equal(head, np.nonzero(want)[0]) and np.array_equal(tail, np.nonzero(~want)[0])
    again = _list(counts, N).tiles
    assert torch.equal(again, live.tiles)


# name: (K, N, kind, options) -- the SIZE_CASES of the three kernels by their own names, then the backward epilogues and the GLU form
CASES = {name: c for name, c in SIZE_CASES.items() if c[1] in (256, 512)}
EXTRA = {
    'gelu_bwd': (256, 256, 'gelu_bwd', dict(p=0.0, scaled=False)),
    'gelu_bwd scaled p=0.1': (256, 256, 'gelu_bwd', dict(p=0.1, scaled=True)),
    'ln_bwd K=256': (256, 256, 'ln_bwd', {}),
    'ln_bwd K=128': (128, 256, 'ln_bwd', {}),
    'glu geglu': (256, 512, 'glu', dict(kind='geglu', p=0.0, scaled=False)),
    'glu glu p=0.1': (256, 512, 'glu', dict(kind='glu', p=0.1, scaled=False)),
    'glu swiglu scaled p=0.1': (256, 512, 'glu', dict(kind='swiglu', p=0.1, scaled=True)),
}
ALL_CASES = list(CASES) + list(EXTRA)


def test_the_cases_are_the_ones_of_the_three_kernels():
    assert set(CASES) == {k for k, c in SIZE_CASES.items() if 'slice' not in k} and len(CASES) == 8
    g = _lib.EdgeLinearArgs()
    for name, (K, N, epi, *_r) in SIZE_CASES.items():
        g.M, g.K, g.N, g.dtype = M_, K, N, _lib.TGT_BF16
        g.epilogue = {'bias': _lib.EPI_BIAS, 'gelu': _lib.EPI_GELU, 'resid': _lib.EPI_RESID}[epi]
        g.gamma = g.beta = g.y = (16 if epi == 'resid' else None)
        assert bool(_lib.lib().tgt_edge_linear_live_supported(g)) == (name in CASES), name


class _Inputs:
    def __init__(self, K, N, dtype, counts=COUNTS, seed=53):
        a, w, b, g = _mk(M_, K, N, dtype, seed)
        self.a, self.w, self.b = a, w, b
        self.res = (torch.randn(M_, 256, device='cuda', generator=g) * 1.3 + 0.2).to(dtype)       # residual / pre-activation / LN input
        self.ds = torch.randn(M_, 256, device='cuda', generator=g).to(dtype)
        self.sc = torch.tensor([1.25, 0.0, 1.25], device='cuda') if counts == COUNTS else (torch.rand(B_, device='cuda', generator=g) + 0.5)
        self.sc_bwd = torch.rand(B_, device='cuda', generator=g) + 0.5
        self.gamma = torch.rand(256, device='cuda', generator=g) + 0.5
        self.beta = torch.randn(256, device='cuda', generator=g) * 0.2
        _, mu, rs = _ln64(self.res, self.gamma, torch.zeros_like(self.gamma), 1e-5)
        self.mean, self.rstd = mu.float(), rs.float()
        self.dtype = dtype

    def poisoned(self, dead_rows):
        """the same operands with NaN in the rows of dead tiles (A, res, ds_in -- and the saved statistics)"""
        o = object.__new__(_Inputs)
        o.__dict__.update(self.__dict__)
        for name in ('a', 'res', 'ds', 'mean', 'rstd'):
            t = getattr(self, name).clone()
            t[dead_rows] = float('nan')
            setattr(o, name, t)
        return o


def _nan(*shape, dtype):
    return torch.full(shape, float('nan'), dtype=dtype, device='cuda')


def _run(case, I, live):
    """-> (outputs, colsum_partial or None); every output starts as NaN"""
    dt = I.dtype
    if case in CASES:
        K, N, epi, pres, ln, with_sc = CASES[case]
        scale = I.sc if with_sc else None
        if epi == 'bias':
            return [ops.edge_linear_raw(I.a, I.w, I.b, out=_nan(M_, N, dtype=dt), live=live)], None
        if epi == 'gelu':
            pre = _nan(M_, N, dtype=dt)
            act = ops.edge_linear_raw(I.a, I.w, I.b, _lib.EPI_GELU, out=_nan(M_, N, dtype=dt), out2=pre, dropout=(0.1, 0x5eed77),
                                      row_scale=scale, rows_per_sample=RPS, live=live)
            return [act, pre], None
        mean, rstd, y = _nan(M_, dtype=torch.float32), _nan(M_, dtype=torch.float32), _nan(M_, N, dtype=dt)
        out = ops.edge_linear_raw(I.a, I.w, I.b, _lib.EPI_RESID, out=_nan(M_, N, dtype=dt), res=I.res, row_scale=scale, rows_per_sample=RPS,
                                  ln=(I.gamma, I.beta, 1e-5), stats=(mean, rstd), y=y, flags=_lib.EDGE_BIAS_SCALED if pres else 0, live=live)
        return [out, y, mean, rstd], None
    K, N, kind, o = EXTRA[case]
    L = _lib.lib()
    if kind == 'gelu_bwd':
        cs = _nan(L.tgt_edge_linear_parts(M_, 256), 256, dtype=torch.float32)
        out = ops.edge_linear_raw(I.a, I.w, None, _lib.EPI_GELU_BWD, out=_nan(M_, 256, dtype=dt), res=I.res,
                                  out_scale=I.sc_bwd if o['scaled'] else None, rows_per_sample=RPS if o['scaled'] else 0,
                                  dropout=(o['p'], 0x9e1b5eed if o['p'] else 0), colsum_partial=cs, live=live)
        return [out], cs
    if kind == 'ln_bwd':
        cs = _nan(L.tgt_edge_linear_parts(M_, 256), 3 * 256, dtype=torch.float32)
        dres, dx = _nan(M_, 256, dtype=dt), _nan(M_, 256, dtype=dt)
        ops.edge_linear_raw(I.a, I.w, None, _lib.EPI_LN_BWD, ln=(I.gamma, None, 1e-5), stats=(I.mean, I.rstd), res=I.res, ds_in=I.ds,
                            out=dres, out2=dx, row_scale=I.sc_bwd, rows_per_sample=RPS, colsum_partial=cs, live=live)
        return [dres, dx], cs
    pre = _nan(M_, 512, dtype=dt)
    act = ops.edge_linear_raw(I.a, I.w, I.b, _lib.EPI_GLU, out=_nan(M_, 256, dtype=dt), out2=pre, dropout=(o['p'], 0x61c0ffee if o['p'] else 0),
                              row_scale=I.sc_bwd if o['scaled'] else None, rows_per_sample=RPS if o['scaled'] else 0,
                              flags=_lib.GLU_KINDS[o['kind']] << _lib.EDGE_GLU_KIND_SHIFT, live=live)
    return [act, pre], None


def _shape(case):
    return (CASES[case] if case in CASES else EXTRA[case])[:2]


def _colsum_want(case, I, outs, live_rows):
    """float64 sums of the terms the kernel adds (module docstring), over the rows of live tiles"""
    kind = EXTRA[case][2]
    if kind == 'gelu_bwd':
        return outs[0].double().sum(0)
    # dy as the row kernel holds it: the same k-loop, rounded to the storage type, through a residual launch with res = 0
    dy = ops.edge_linear_raw(I.a, I.w, None, _lib.EPI_RESID, res=torch.zeros(M_, 256, dtype=I.dtype, device='cuda')).double()
    dy = dy * live_rows[:, None]
    xh = (I.res.double() - I.mean.double()[:, None]) * I.rstd.double()[:, None]
    return torch.cat([(dy * xh).sum(0), dy.sum(0), outs[1].double().sum(0)])


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('cap', [0, 1, 3])
@pytest.mark.parametrize('case', ALL_CASES)
def test_row_kernels_walk_the_live_list(case, cap, dtype):
    K, N = _shape(case)
    parity_log.Tol({torch.bfloat16: 1e-5, torch.float16: 1e-5})[dtype]           # (files the column-sum errors under this dtype)
    clean = _Inputs(K, N, dtype)
    tile_live = torch.from_numpy(np.repeat(_live_tiles_np(B_, N_, COUNTS), 32)[:M_]).cuda()      # per ROW: is its tile live
    dirty = clean.poisoned(~tile_live)
    live = _list(COUNTS)
    L = _lib.lib()
    try:
        L.tgt_edge_linear_set_grid_cap(cap)
        ref, _ = _run(case, clean, None)
        got, cs = _run(case, dirty, live)
        again, cs2 = _run(case, dirty, live)
        torch.cuda.synchronize()
    finally:
        L.tgt_edge_linear_set_grid_cap(0)
    assert int(live.tiles[0]) == 17 and live.tiles.numel() == 39
    for r_, g_, a_ in zip(ref, got, again):
        assert not bool(torch.isnan(g_.float()).any()), case                   # every row written, no poisoned operand read
        assert torch.equal(g_[tile_live], r_[tile_live]), case                  # live tiles: the launch without a list, bit for bit
        assert bool((g_[~tile_live] == 0).all()), case                          # dead tiles: zeros
        assert torch.equal(g_, a_), case
    if cs is not None:
        assert bool(torch.isfinite(cs).all()) and torch.equal(cs, cs2)
        want = _colsum_want(case, clean, got, tile_live)
        ok, err = _colsum_close(cs.double().sum(0), want)
        print(f'{case} cap={cap} {dtype}: column sums off by {err:.3e} of max|want|')
        assert ok, ('colsum', case, err)
        if cap == 0:                                                            # 38 workgroups, 17 live tiles: the others wrote zeros
            assert cs.shape[0] == 38 and bool((cs[17:] == 0).all()) and bool((cs[:17] != 0).any(1).all())


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('case', ALL_CASES)
def test_a_batch_of_empty_graphs_is_all_zeros(case, dtype):
    K, N = _shape(case)
    I = _Inputs(K, N, dtype, counts=[0, 0, 0]).poisoned(torch.ones(M_, dtype=torch.bool, device='cuda'))
    live = _list([0, 0, 0])
    outs, cs = _run(case, I, live)
    torch.cuda.synchronize()
    assert int(live.tiles[0]) == 0
    for t in outs:
        assert bool((t == 0).all()), case
    if cs is not None:
        assert bool((cs == 0).all()), case


def test_a_list_is_a_permission_not_an_obligation():
    """edge_linear_raw(live=) makes the plain call when the list describes another row count or the launch is one
    tgt_edge_linear_live does not take (the slice kernel): the result is the plain one, every row computed"""
    dtype = torch.bfloat16
    a, w, b, _ = _mk(M_, 256, 128, dtype, 59)
    live = _list(COUNTS)
    want = ops.edge_linear_raw(a, w, b)
    assert torch.equal(ops.edge_linear_raw(a, w, b, live=live), want)                       # N = 128: the slice kernel
    a2, w2, b2, _ = _mk(M_ - 32, 256, 512, dtype, 61)
    assert torch.equal(ops.edge_linear_raw(a2, w2, b2, live=live), ops.edge_linear_raw(a2, w2, b2))      # other row count
    g = _lib.EdgeLinearArgs()
    g.M, g.K, g.N, g.dtype, g.epilogue = M_, 256, 128, _lib.TGT_BF16, _lib.EPI_BIAS
    g.a, g.lda, g.w, g.ldw, g.out, g.ldo = a.data_ptr(), 256, w.data_ptr(), 256, want.data_ptr(), 128
    assert _lib.lib().tgt_edge_linear_live(g, live.tiles.data_ptr(), None) == 2             # the C entry itself refuses


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
GEOM = dict(B=4, N=12, num_nodes=[12, 5, 9, 1])
CFG = dict(gu.MODEL_CASES['multi_at_tiny'][1], model_height=2, node_width=64, edge_width=256, num_heads=4, triplet_heads=16)
# gradients that come through colsum_partial (regrouped over workgroups by the list): the LayerNorms of the edge channel whose
# backward is the LN_BWD epilogue, and the biases of the edge Linears in front of them / in front of the activation
COLSUM_GRADS = ('update.mha_ln_e.', 'tria.tri_ln_e.', 'edge_ffn.ffn_ln.', 'update.lin_O_e.bias', 'tria.lin_O.bias',
                'edge_ffn.lin_W1.bias', 'edge_ffn.lin_W2.bias')


@pytest.fixture
def small_rows(monkeypatch):
    monkeypatch.setattr(ops, '_TRI_PROJ', True)
    monkeypatch.setattr(ops, '_TRI_PROJ_INFER', True)
    monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 1)            # (the projection-fused kernel also below 65536 edge rows)
    monkeypatch.setattr(ops, '_EDGE_MIN_ROWS', 1)             # (... and the edge row kernels: 4 * 12 * 12 = 576 rows, 18 tiles)
    from tgt_amd.tgt import stack
    monkeypatch.setattr(stack, '_TRI_RAGGED', True)


class _Spy:
    """(rows, epilogue, live) of every edge_linear_raw launch"""

    def __init__(self, monkeypatch):
        self.calls = []
        real = ops.edge_linear_raw

        def spy(a, w, bias=None, epilogue=_lib.EPI_BIAS, **kw):
            self.calls.append((a.shape[0], epilogue, kw.get('live')))
            return real(a, w, bias, epilogue, **kw)
        monkeypatch.setattr(ops, 'edge_linear_raw', spy)


def _model(train, cfg=CFG, cls='TGT_Multi'):
    from tgt_amd import pcqm
    m = gu.fill_params(getattr(pcqm, cls)(**cfg), seed=31).cuda()
    return m.train() if train else m.eval()


def _batch(seed=32):
    return {k: v.cuda() for k, v in gu.model_batch(GEOM, seed=seed).items()}


def _step(model, batch, loss_of):
    model.zero_grad(set_to_none=True)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out = model(batch)
        loss = loss_of(out, batch)
    loss.backward()
    torch.cuda.synchronize()
    out = out if isinstance(out, (tuple, list)) else [out]
    return loss.detach(), [o.detach() for o in out], {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def _pretrain_loss(out, batch):
    from tgt_amd.training.step import pretrain_loss, StepConfig
    return pretrain_loss(out, batch, StepConfig(num_dist_bins=CFG['num_dist_bins'], mixed_precision=None))


def test_training_step_with_the_switch_on(small_rows, monkeypatch):
    from tgt_amd.tgt import stack
    model, batch = _model(train=True), _batch()
    rows = GEOM['B'] * GEOM['N'] ** 2
    spy = _Spy(monkeypatch)
    monkeypatch.setattr(stack, '_EDGE_RAGGED', False)
    loss0, out0, grads0 = _step(model, batch, _pretrain_loss)
    assert spy.calls and all(c[2] is None for c in spy.calls)
    n_off = len(spy.calls)
    monkeypatch.setattr(stack, '_EDGE_RAGGED', True)
    loss1, out1, grads1 = _step(model, batch, _pretrain_loss)
    on = spy.calls[n_off:]
    assert [c[:2] for c in on] == [c[:2] for c in spy.calls[:n_off]]                     # the same launches, no other
    given = [c[2] for c in on if c[2] is not None]
    assert given and all(l is given[0] for l in given)                                   # ONE list object, forward and backward
    assert isinstance(given[0], ops.EdgeLiveTiles) and given[0].rows == rows
    want = _live_tiles_np(GEOM['B'], GEOM['N'], GEOM['num_nodes'])
    assert int(given[0].tiles[0]) == int(want.sum()) < want.size
    with_list = {c[1] for c in on if c[2] is not None and c[0] == rows}
    assert {_lib.EPI_RESID, _lib.EPI_GELU, _lib.EPI_GELU_BWD, _lib.EPI_LN_BWD, _lib.EPI_BIAS} <= with_list, with_list
    assert all(c[2] is not None for c in on if c[0] == rows and c[1] != _lib.EPI_BIAS)   # every whole-row epilogue on the edge rows
    assert torch.equal(loss1, loss0), (float(loss1), float(loss0))
    em = batch['edge_mask'].bool()
    assert torch.equal(out1[0], out0[0])                                                # gap: one value per graph
    assert torch.equal(out1[1][em], out0[1][em])                                        # distance logits on the real edges
    assert grads1.keys() == grads0.keys() and len(grads0) > 20
    parity_log.Tol({torch.bfloat16: 2e-5})[torch.bfloat16]
    bad, worst = [], 0.0
    for k in grads0:
        if any(s in k for s in COLSUM_GRADS):
            top = float(grads0[k].abs().max())
            err = float((grads1[k].double() - grads0[k].double()).abs().max())
            worst = max(worst, parity_log.record(err / (top + 1e-30)))
            print(f'{k}: |on - off| max {err:.3e}, max|off| {top:.3e}')
            if not err <= 2e-5 * top + 2e-6:
                bad.append((k, err, top))
        elif not torch.equal(grads1[k], grads0[k]):
            bad.append(k)
    assert not bad, bad
    assert any('tria' in k for k in grads0) and sum(any(s in k for s in COLSUM_GRADS) for k in grads0) >= 12


def test_eval_forward_and_graphed_replay(small_rows, monkeypatch):
    """eval mode, no_grad, bf16 autocast: switch on = switch off on the real positions; and the captured forward (GraphedForward:
    the list launch is part of the graph) replays to the eager result with the switch on."""
    from tgt_amd.tgt import stack
    from tgt_amd.pcqm.graphed import GraphedForward
    model = _model(train=False)
    b0, b1 = _batch(32), _batch(33)

    def eager(b):
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            out = model(b)
        torch.cuda.synchronize()
        return [o.clone() for o in out]
    monkeypatch.setattr(stack, '_EDGE_RAGGED', False)
    off = eager(b0)
    monkeypatch.setattr(stack, '_EDGE_RAGGED', True)
    spy = _Spy(monkeypatch)
    on = eager(b0)
    assert any(c[2] is not None for c in spy.calls)
    em = b0['edge_mask'].bool()
    assert torch.equal(on[0], off[0]) and torch.equal(on[1][em], off[1][em])
    gf = GraphedForward(model, b0, autocast_dtype=torch.bfloat16, warmup=1)
    for b in (b1, b0):
        want = eager(b)
        got = gf(b)
        torch.cuda.synchronize()
        em = b['edge_mask'].bool()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1][em], want[1][em])


def test_the_aggregate_family_computes_everything(small_rows, monkeypatch):
    """TGT-Agx2 (triplet aggregate: its gated outward direction is unmasked, padded rows reach real outputs): the knob has no
    effect -- no launch gets a list, one notice says so, and the step is the knob-off step bit for bit, padded positions included"""
    from tgt_amd.tgt import stack
    name, kwargs, _ = gu.MODEL_CASES['dist_agx2_tiny']
    cfg = dict(kwargs, model_height=2, node_width=64, edge_width=256, num_heads=4, triplet_heads=16)
    model, batch = _model(True, cfg, name), _batch()

    def loss_of(out, batch):
        o = out[-1] if isinstance(out, (tuple, list)) else out
        return (o.float() * batch['edge_mask'].reshape(o.shape[:3] + (1,) * (o.ndim - 3)).float()).square().mean()
    monkeypatch.setattr(stack, '_EDGE_RAGGED', False)
    loss0, out0, grads0 = _step(model, batch, loss_of)
    monkeypatch.setattr(stack, '_EDGE_RAGGED', True)
    monkeypatch.setattr(ops, '_slow_path_said', set())
    spy = _Spy(monkeypatch)
    with pytest.warns(RuntimeWarning, match='TGT_EDGE_RAGGED has no effect'):
        loss1, out1, grads1 = _step(model, batch, loss_of)
    assert spy.calls and all(c[2] is None for c in spy.calls)
    assert torch.equal(loss1, loss0) and all(torch.equal(a, b) for a, b in zip(out1, out0))
    assert grads1.keys() == grads0.keys() and all(torch.equal(grads1[k], grads0[k]) for k in grads0)
