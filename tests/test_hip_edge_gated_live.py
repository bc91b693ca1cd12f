"""The gated output stage of TriangularUpdate on a live tile list (tgt_edge_gated_out_fwd_live / _bwd_live; include/tgt_hip.h),
on the GPU.

M = 4 * 12^2 = 576 rows (18 tiles of 32), K = 32, C = 256, bf16 / fp16, node counts [12, 5, 9, 1]: the last graph leaves whole
tiles dead, and live tiles hold padded rows (checked on the CPU against the numpy predicate of tests/test_hip_edge_live.py).  A
second case has all counts 0.  Grid caps 1, 3 and none: a workgroup walks many live and many dead tiles, or -- uncapped -- some
workgroups have no live tile.  The operands of the dead tiles are NaN: a single read shows.
  * live tiles: s, y, mean, rstd and d_a bit-identical to the plain launch on clean operands; dead tiles: zeros; no NaN anywhere
    (every output starts as NaN);
  * the summed dw / db: the list regroups rows over workgroups, so they are held to the float64 sum of THE SAME TERMS at
    _colsum_close of tests/test_hip_edge_gemm.py (1e-5 max|want| + 1e-6, the project's fp32 summation bar).  The terms: the
    per-tile sums dz^T a and colsum(dz) of the plain launch with one workgroup per tile (uncapped grid: 18 workgroups, 18 tiles),
    on the clean operands with the rows of dead tiles zeroed -- dz is then exactly 0 there, which is what a dead tile adds;
    summed over the tiles in float64;
  * two runs are torch.equal; a NULL list equals the plain entry point bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import parity_log
from test_hip_edge_gemm import _colsum_close
from test_hip_edge_live import _live_rows_np, _live_tiles_np

from tgt_amd import _lib, ops

pytestmark = pytest.mark.gpu

B_, N_, K_, CH = 4, 12, 32, 256
M_ = B_ * N_ * N_
T_ = (M_ + 31) // 32
RPS = N_ * N_
COUNTS = [12, 5, 9, 1]
SCALES = [1 / 0.9, 1 / 0.9, 0.0, 1 / 0.9]
NAN = float('nan')


def test_the_geometry_is_the_one_the_checks_need():
    """on the CPU: at least 3 dead tiles, and at least one live tile that holds padded rows"""
    rows, tiles = _live_rows_np(B_, N_, COUNTS), _live_tiles_np(B_, N_, COUNTS)
    assert tiles.size == T_ == 18 and int((~tiles).sum()) >= 3
    per_tile = np.pad(rows, (0, T_ * 32 - rows.size)).reshape(T_, 32)
    assert any(tiles[t] and not per_tile[t].all() for t in range(T_))
    assert not _live_tiles_np(B_, N_, [0] * B_).any()


class _Inputs:
    def __init__(self, dtype, seed=71):
        g = torch.Generator(device='cuda').manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, device='cuda', generator=g)
        self.a = rnd(M_, K_).to(dtype)
        self.w = (rnd(2 * CH, K_) * (2.0 / K_ ** 0.5)).to(dtype)
        self.bias = (rnd(2 * CH) * 0.5).to(dtype)
        self.res = (rnd(M_, CH) * 1.3 + 0.2).to(dtype)
        self.gamma, self.beta = 1 + 0.3 * rnd(CH), 0.3 * rnd(CH)
        self.scale = torch.tensor(SCALES, device='cuda')
        self.dt = rnd(M_, CH).to(dtype)                      # (nonzero in every row: every live tile adds to dw / db)
        self.dtype = dtype

    def with_rows(self, rows, value):
        """the same operands with `value` in the given rows of a, res and dt"""
        o = object.__new__(_Inputs)
        o.__dict__.update(self.__dict__)
        for name in ('a', 'res', 'dt'):
            t = getattr(self, name).clone()
            t[rows] = value
            setattr(o, name, t)
        return o


def _run(I, tiles, cap=0, parts=None):
    """both launches; tiles: None (the plain entry points), 'null' (the _live entry points with a NULL list) or an EdgeLiveTiles.
    Every output starts as NaN.  -> (dict of s, y, mean, rstd, d_a; dw_partial; db_partial)"""
    L = _lib.lib()
    nan = lambda *s, dtype=I.dtype: torch.full(s, NAN, dtype=dtype, device='cuda')
    o = dict(s=nan(M_, CH), y=nan(M_, CH), mean=nan(M_, dtype=torch.float32), rstd=nan(M_, dtype=torch.float32), d_a=nan(M_, K_))
    L.tgt_edge_linear_set_grid_cap(cap)
    try:
        parts = parts or L.tgt_edge_gated_out_parts(M_)
        assert parts == (cap or T_)
        dw_part, db_part = nan(parts, 2 * CH, K_, dtype=torch.float32), nan(parts, 2 * CH, dtype=torch.float32)
        g = ops._gated_args(I.a, I.w, I.bias, CH)
        g.res, g.s, g.y, g.gamma, g.beta, g.eps = I.res.data_ptr(), o['s'].data_ptr(), o['y'].data_ptr(), I.gamma.data_ptr(), I.beta.data_ptr(), 1e-5
        g.mean, g.rstd = o['mean'].data_ptr(), o['rstd'].data_ptr()
        g.row_scale, g.rows_per_sample = I.scale.data_ptr(), RPS
        g.parts, g.dt, g.d_a, g.ld_da = parts, I.dt.data_ptr(), o['d_a'].data_ptr(), K_
        g.dw_partial, g.db_partial = dw_part.data_ptr(), db_part.data_ptr()
        if tiles is None:
            ops._launch('tgt_edge_gated_out_fwd', C.byref(g))
            ops._launch('tgt_edge_gated_out_bwd', C.byref(g))
        else:
            lst = None if isinstance(tiles, str) else ops._ptr(tiles.tiles)
            ops._launch('tgt_edge_gated_out_fwd_live', C.byref(g), lst)
            ops._launch('tgt_edge_gated_out_bwd_live', C.byref(g), lst)
        torch.cuda.synchronize()
    finally:
        L.tgt_edge_linear_set_grid_cap(0)
    return o, dw_part, db_part


def _list(counts):
    return ops.edge_live_tiles(torch.tensor(counts, dtype=torch.int32, device='cuda'), N_)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('cap', [0, 1, 3])
def test_gated_stage_walks_the_live_list(cap, dtype):
    parity_log.Tol({torch.bfloat16: 1e-5, torch.float16: 1e-5})[dtype]           # (files the summation errors under this dtype)
    clean = _Inputs(dtype)
    tile_live_np = _live_tiles_np(B_, N_, COUNTS)
    tile_live = torch.from_numpy(np.repeat(tile_live_np, 32)[:M_]).cuda()        # per ROW: is its tile live
    dirty = clean.with_rows(~tile_live, NAN)
    live = _list(COUNTS)
    assert int(live.tiles[0]) == int(tile_live_np.sum()) and live.tiles.numel() == 1 + T_
    ref, _, _ = _run(clean, None, cap)
    got, dw_part, db_part = _run(dirty, live, cap)
    again, dw2, db2 = _run(dirty, live, cap)
    for k in got:
        assert not bool(torch.isnan(got[k].float()).any()), k                    # every row written, no poisoned operand read
        assert torch.equal(got[k][tile_live], ref[k][tile_live]), k              # live tiles: the plain launch, bit for bit
        assert bool((got[k][~tile_live] == 0).all()), k                          # dead tiles: zeros
        assert torch.equal(got[k], again[k]), k
    # every plane and row of the partials written, reproducibly
    assert bool(torch.isfinite(dw_part).all()) and bool(torch.isfinite(db_part).all())
    assert torch.equal(dw_part, dw2) and torch.equal(db_part, db2)
    n_live = int(tile_live_np.sum())
    if cap == 0:                                                                 # 18 workgroups, the first n_live have one live tile each
        assert dw_part.shape[0] == T_ and bool((dw_part[n_live:] == 0).all()) and bool((db_part[n_live:] == 0).all())
        assert bool((db_part[:n_live] != 0).any(1).all())
    # the same terms in float64: one workgroup per tile on the operands with the dead tiles' rows ZEROED gives each live tile's
    # own partial sums (a dead tile's are exact zeros: a = 0 and dt = 0 make dz = 0); their float64 sum is the want
    per_tile, dw_t, db_t = _run(clean.with_rows(~tile_live, 0.0), None, 0)
    assert bool((dw_t[~torch.from_numpy(tile_live_np).cuda()] == 0).all())
    want_dw, want_db = dw_t.double().sum(0), db_t.double().sum(0)
    for name, have, want in (('dw', dw_part.double().sum(0), want_dw), ('db', db_part.double().sum(0), want_db)):
        ok, err = _colsum_close(have, want)
        print(f'gated live cap={cap} {dtype}: {name} partial sums off by {err:.3e} of max|want|')
        assert ok, (name, err)
    # ... and the sums as the op forms them (tgt_sum_planes / tgt_sum_rows, fp32)
    dw = ops.sum_planes(dw_part, torch.empty(2 * CH, K_, dtype=torch.float32, device='cuda'), defer=False)
    db = ops.sum_rows(db_part, defer=False)
    torch.cuda.synchronize()
    for name, have, want in (('dw', dw.double(), want_dw), ('db', db.double(), want_db)):
        ok, err = _colsum_close(have, want)
        print(f'gated live cap={cap} {dtype}: summed {name} off by {err:.3e} of max|want|')
        assert ok, (name, err)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('cap', [0, 1, 3])
def test_a_batch_of_empty_graphs_is_all_zeros(cap, dtype):
    I = _Inputs(dtype).with_rows(torch.ones(M_, dtype=torch.bool, device='cuda'), NAN)
    live = _list([0] * B_)
    assert int(live.tiles[0]) == 0
    got, dw_part, db_part = _run(I, live, cap)
    for k, t in got.items():
        assert bool((t == 0).all()), k
    assert bool((dw_part == 0).all()) and bool((db_part == 0).all())


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
def test_a_null_list_is_the_plain_entry_point(dtype):
    I = _Inputs(dtype)
    for cap in (0, 3):
        ref, dw0, db0 = _run(I, None, cap)
        got, dw1, db1 = _run(I, 'null', cap)
        for k in ref:
            assert torch.equal(got[k], ref[k]), k
        assert torch.equal(dw1, dw0) and torch.equal(db1, db0)


def test_a_full_list_is_the_plain_launch_bit_for_bit():
    """every graph full: the list names every tile in order, so the dealing is the plain one -- partials included"""
    I = _Inputs(torch.bfloat16)
    live = _list([N_] * B_)
    assert int(live.tiles[0]) == T_
    for cap in (0, 3):
        ref, dw0, db0 = _run(I, None, cap)
        got, dw1, db1 = _run(I, live, cap)
        for k in ref:
            assert torch.equal(got[k], ref[k]), k
        assert torch.equal(dw1, dw0) and torch.equal(db1, db0)


def test_a_wild_list_stays_inside_the_tensors():
    """entries are clamped where they are read: a count above the number of tiles is the number of tiles (every entry is then
    walked as live), and an entry outside [0, tiles) is a tile past the last row, which loads nothing and stores nothing"""
    I = _Inputs(torch.bfloat16)
    good = _list(COUNTS)
    wild = ops.EdgeLiveTiles(good.tiles.clone(), good.rows)
    wild.tiles[0] = 1000                                   # clamped to the 18 tiles: every entry is walked as live
    wild.tiles[3] = -5                                     # -> a tile past the last row: loads nothing, stores nothing
    wild.tiles[4] = 1 << 20
    got, dw_part, db_part = _run(I, wild, 3)
    ref, _, _ = _run(I, None, 3)
    skipped = {int(good.tiles[3]), int(good.tiles[4])}
    rows = torch.ones(M_, dtype=torch.bool, device='cuda')
    for t in skipped:
        rows[32 * t:32 * t + 32] = False
    for k in ref:
        assert torch.equal(got[k][rows], ref[k][rows]), k  # every other tile computed, bit for bit
        assert bool(torch.isnan(got[k][~rows].float()).all()), k      # the two dropped entries: their tiles were never written
    assert bool(torch.isfinite(dw_part).all()) and bool(torch.isfinite(db_part).all())
