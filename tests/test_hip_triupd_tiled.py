"""The TriangularUpdate core on staged matrix-core tiles (tgt_triangular_update_tiled_*, ops.triangular_update_packed) against the
float64 oracle on the inputs of tests/triplet_hard_inputs.py (non-symmetric pair masks, saturated gates), on the GPU.

Shapes: N = 5 (one partial 32-tile, H = 8: two head groups), 20 (ragged, H = 16), 33 (the first N on 64-wide planes: a 32-tile
with one live row / column), 40 (ragged inside the second tile, H = 32), 64 (the upper limit, ragged).  Both 16-bit types; the
contiguous form (two tensors, row stride 4H) and the packed form (the halves of one (B,N,N,8H) buffer, gradients into one buffer).

Bars: the project's own (tests/test_hip_triplet_hard_inputs.py): rel-L2 against float64 on the values as the kernel sees them,
bf16 8e-3 / fp16 1e-3 forward, twice that for gradients.  The gated operands are rounded to the element type before the matrix
core sees them: a CPU simulation of that rounding gave bf16 2.2-2.9e-3, fp16 2.9-3.9e-4.
profiles/parity_errors_triupd.json records the measured errors (TGT_PARITY_LOG)."""
import ctypes as C

import pytest
import torch

import parity_log
import test_triplet_hard_inputs as hc
import triplet_hard_inputs as hi

pytestmark = pytest.mark.gpu

TOL = parity_log.Tol({torch.bfloat16: 8e-3, torch.float16: 1e-3})
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
CASES = {'N5': (2, 5, [5, 3], 8), 'N20': (2, 20, [20, 13], 16), 'N33': (1, 33, [33], 16), 'N40': (1, 40, [33], 32),
         'N64': (1, 64, [50], 16)}          # B, N, num_nodes, H
PARAMS = [(c, dt) for c in CASES for dt in (BF16, F16)]

_cache = {}


def inputs_and_oracle(case, dtype):
    """(e4, v4, d_out, mask) on the CPU and the float64 oracle's {fwd, de, dv} on them: computed once, shared, never written to"""
    key = (case, dtype)
    if key not in _cache:
        e4, v4, d_out, mask = hi.triangular_inputs(CASES[case], dtype)
        ref = hc.triangular_oracle(e4, v4, d_out, mask, CASES[case][3])
        assert all(torch.isfinite(t).all() for t in ref.values())
        # the mask is not symmetric, so an index swap in either direction shows -- except at N = 5, where pair_mask's leading
        # blocks close rows and columns 1, 2, 4 alike and what is left happens to be symmetric (that case is about the partial tile)
        assert case == 'N5' or not torch.equal(mask, mask.transpose(1, 2))
        _cache[key] = (e4, v4, d_out, mask, ref)
    return _cache[key]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return parity_log.record(float((a - b).norm() / (b.norm() + 1e-30)))


def check(got, ref, tol, what):
    for k, t in got.items():
        assert torch.isfinite(t).all(), (what, k, 'not finite')
    errs = {k: rel(got[k], ref[k]) for k in ref}
    limit = {k: tol * (1 if k == 'fwd' else 2) for k in ref}
    print(what, 'rel-L2', {k: f'{v:.3e}' for k, v in errs.items()}, 'bars', limit)
    bad = {k: (errs[k], limit[k]) for k in ref if not errs[k] < limit[k]}
    assert not bad, (what, bad)


def run_contiguous(e4, v4, d_out, mask, H):
    """the C entries on two contiguous tensors (row stride 4H); gradient buffers pre-filled with NaN: every element must be written"""
    from tgt_amd import _lib, ops
    B, N = e4.shape[0], e4.shape[1]
    e, v, g, m = e4.cuda(), v4.cuda(), d_out.cuda(), mask.cuda()
    dt = ops._DT[e.dtype]
    out = torch.full((B, N, N, 2 * H), float('nan'), dtype=e.dtype, device='cuda')
    de, dv = torch.full_like(e, float('nan')), torch.full_like(v, float('nan'))
    p = ops._ptr
    ops._launch('tgt_triangular_update_tiled_fwd', p(e), 4 * H, p(v), 4 * H, p(m), p(out), B, N, H, dt)
    ops._launch('tgt_triangular_update_tiled_bwd', p(e), 4 * H, p(v), 4 * H, p(m), p(g), p(de), 4 * H, p(dv), 4 * H, B, N, H, dt)
    torch.cuda.synchronize()
    return dict(fwd=out, de=de, dv=dv)


def run_packed(e4, v4, d_out, mask, H, monkeypatch, tiled=True):
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_TRIUPD_TILED', tiled)
    ev = torch.cat((e4, v4), dim=-1).cuda().requires_grad_(True)
    prof = ops.profile_kernels(True)
    try:
        out = ops.triangular_update_packed(ev, mask.cuda(), H)
        out.backward(d_out.cuda())
        torch.cuda.synchronize()
    finally:
        ops.profile_kernels(False)
    ran = {'tgt_triangular_update_tiled_fwd', 'tgt_triangular_update_tiled_bwd'} <= set(prof)
    return dict(fwd=out.detach(), de=ev.grad[..., :4 * H], dv=ev.grad[..., 4 * H:]), ran


@pytest.mark.parametrize('case,dtype', PARAMS, ids=hc.case_id)
def test_tiled_core_contiguous(case, dtype):
    H = CASES[case][3]
    e4, v4, d_out, mask, ref = inputs_and_oracle(case, dtype)
    tol = TOL[dtype]
    got = run_contiguous(e4, v4, d_out, mask, H)
    check(got, ref, tol, f'tiled triangular update {case} {dtype} contiguous')
    again = run_contiguous(e4, v4, d_out, mask, H)
    for k in got:
        assert torch.equal(got[k], again[k]), (k, 'two runs differ')


@pytest.mark.parametrize('case,dtype', PARAMS, ids=hc.case_id)
def test_tiled_core_packed(case, dtype, monkeypatch):
    H = CASES[case][3]
    e4, v4, d_out, mask, ref = inputs_and_oracle(case, dtype)
    tol = TOL[dtype]
    got, ran = run_packed(e4, v4, d_out, mask, H, monkeypatch)
    assert ran, 'the tiled entries did not run'
    check(got, ref, tol, f'tiled triangular update {case} {dtype} packed')
    again, _ = run_packed(e4, v4, d_out, mask, H, monkeypatch)
    for k in got:
        assert torch.equal(got[k], again[k]), (k, 'two runs differ')
    # the same bits as the contiguous form: the row stride changes no arithmetic
    plain = run_contiguous(e4, v4, d_out, mask, H)
    for k in got:
        assert torch.equal(got[k], plain[k]), (k, 'packed and contiguous forms differ')


@pytest.mark.parametrize('case,dtype', [((2, 20, [20, 13], 16), F32), ((1, 40, [33], 3), BF16), ((1, 65, [60], 4), BF16),
                                        ((2, 20, [20, 13], 16), BF16)], ids=hc.case_id)
def test_unsupported_shapes_and_the_knob_off_stay_on_the_old_kernel(case, dtype, monkeypatch):
    """fp32, H = 3 and N = 65 with the knob on, and a supported shape with the knob off: ops.triangular_update's kernel, bit for bit"""
    from tgt_amd import ops
    B, N, nn_, H = case
    e4, v4, d_out, mask = hi.triangular_inputs(case, dtype)
    supported = dtype is not F32 and H % 4 == 0 and N <= 64
    got, ran = run_packed(e4, v4, d_out, mask, H, monkeypatch, tiled=not supported)
    assert not ran
    ex, vx = e4.cuda().requires_grad_(True), v4.cuda().requires_grad_(True)
    out = ops.triangular_update(ex, vx, mask.cuda(), H)
    out.backward(d_out.cuda())
    torch.cuda.synchronize()
    assert torch.equal(got['fwd'], out.detach()) and torch.equal(got['de'], ex.grad) and torch.equal(got['dv'], vx.grad)
    if not supported:
        from tgt_amd import _lib
        e = ex.detach()
        code = _lib.lib().tgt_triangular_update_tiled_fwd(ops._ptr(e), 4 * H, ops._ptr(vx.detach()), 4 * H, ops._ptr(mask.cuda()),
                                                          ops._ptr(out.detach()), B, N, H, ops._DT[dtype], None)
        assert code == 2, _lib.lib().tgt_last_error()


def test_stale_lds_cannot_reach_a_result():
    """rows and columns of the planes past N are written as zeros: a NaN-producing neighbour launch before the call changes nothing,
    and padded pairs of closed gates with huge linear parts contribute exactly 0"""
    from tgt_amd import ops
    case = (1, 5, [3], 8)
    B, N, nn_, H = case
    e4, v4, d_out, mask = hi.triangular_inputs(case, BF16)
    ref = hc.triangular_oracle(e4, v4, d_out, mask, H)
    poison = torch.full((1, 32, 32, 4 * H), float('nan'), dtype=BF16)
    run_contiguous(poison, poison, torch.zeros(1, 32, 32, 2 * H, dtype=BF16), torch.zeros(1, 32, 32), H)     # leaves NaN planes in LDS
    got = run_contiguous(e4, v4, d_out, mask, H)
    check(got, ref, TOL[BF16], 'tiled triangular update after a NaN launch')
    closed = mask == hi.LO
    assert closed.any()
    assert (got['de'].cpu()[closed] == 0).all() and (got['dv'].cpu()[closed] == 0).all()
