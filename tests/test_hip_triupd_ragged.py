"""The tiled TriangularUpdate core with per-graph node counts (tgt_triangular_update_tiled_fwd_counts / _bwd_counts,
ops.triangular_update_packed(node_counts=); include/tgt_hip.h), on the GPU.

Cases (B, N, counts, H), bf16 and fp16, prefix masks that close exactly the pairs with a node >= n_b:
  N12   4, 12, [12, 5, 9, 1], 4       planes of 32
  N40   4, 40, [40, 33, 32, 17], 4    planes of 64: counts either side of the 16-chunk and the 32-tile edges
  N64   3, 64, [64, 16, 0], 16        the upper limit, four head groups, an empty graph
What is held:
  * with counts == without counts by torch.equal at EVERY position, forward and backward (value equality: a padded pair is an
    exact zero of either sign without counts, +0 with them), d_out finite and random everywhere;
  * poison: ev, d_out and the mask NaN at every pair with a node >= n_b -- with counts the results equal the clean run's and hold
    no NaN (outputs start as NaN: an unwritten element shows);
  * two runs are torch.equal; counts above N / below 0 behave as N / 0;
  * the float64 oracle, at the bars of tests/test_hip_triupd_tiled.py (rel-L2 bf16 8e-3 / fp16 1e-3 forward, twice that for
    gradients)."""
import pytest
import torch

import parity_log
import test_triplet_hard_inputs as hc
import triplet_hard_inputs as hi

pytestmark = pytest.mark.gpu

TOL = parity_log.Tol({torch.bfloat16: 8e-3, torch.float16: 1e-3})
BF16, F16 = torch.bfloat16, torch.float16
CASES = {'N12': (4, 12, [12, 5, 9, 1], 4), 'N40': (4, 40, [40, 33, 32, 17], 4), 'N64': (3, 64, [64, 16, 0], 16)}
PARAMS = [(c, dt) for c in CASES for dt in (BF16, F16)]
NAN = float('nan')

_cache = {}


def inputs(case, dtype):
    """(e4, v4, d_out, mask, padded) on the GPU, the float64 oracle's {fwd, de, dv} and the plain (no counts) results: computed
    once, shared, never written to.  padded (B,N,N) bool: the pairs with a node >= n_b"""
    key = (case, dtype)
    if key not in _cache:
        B, N, counts, H = CASES[case]
        e4, v4, d_out, mask = hi.triangular_inputs(CASES[case], dtype, hard=False)
        padded = mask != 0
        real = torch.arange(N)[None, :] < torch.tensor(counts)[:, None]
        assert torch.equal(~padded, real[:, :, None] & real[:, None, :])          # the mask closes exactly the padded pairs
        assert torch.isfinite(d_out.float()).all() and bool((d_out[padded] != 0).any())
        ref = hc.triangular_oracle(e4, v4, d_out, mask, H)
        dev = [t.cuda() for t in (e4, v4, d_out, mask, padded)]
        _cache[key] = (*dev, ref, run(*dev[:4], H, None))
    return _cache[key]


def run(e, v, g, m, H, counts):
    """the C entries on two contiguous tensors; counts None: the plain entry points.  Every output starts as NaN"""
    from tgt_amd import ops
    B, N = e.shape[0], e.shape[1]
    dt = ops._DT[e.dtype]
    out = torch.full((B, N, N, 2 * H), NAN, dtype=e.dtype, device='cuda')
    de, dv = torch.full_like(e, NAN), torch.full_like(v, NAN)
    p = ops._ptr
    if counts is None:
        ops._launch('tgt_triangular_update_tiled_fwd', p(e), 4 * H, p(v), 4 * H, p(m), p(out), B, N, H, dt)
        ops._launch('tgt_triangular_update_tiled_bwd', p(e), 4 * H, p(v), 4 * H, p(m), p(g), p(de), 4 * H, p(dv), 4 * H, B, N, H, dt)
    else:
        nc = torch.tensor(counts, dtype=torch.int32, device='cuda')
        ops._launch('tgt_triangular_update_tiled_fwd_counts', p(e), 4 * H, p(v), 4 * H, p(m), p(out), B, N, H, dt, p(nc))
        ops._launch('tgt_triangular_update_tiled_bwd_counts', p(e), 4 * H, p(v), 4 * H, p(m), p(g), p(de), 4 * H, p(dv), 4 * H, B, N, H, dt,
                    p(nc))
    torch.cuda.synchronize()
    return dict(fwd=out, de=de, dv=dv)


def same(a, b, what):
    for k in a:
        assert not bool(torch.isnan(a[k].float()).any()), (what, k, 'NaN')
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize('case,dtype', PARAMS, ids=hc.case_id)
def test_counts_change_no_value(case, dtype):
    B, N, counts, H = CASES[case]
    e, v, g, m, padded, ref, plain = inputs(case, dtype)
    got = run(e, v, g, m, H, counts)
    same(got, plain, 'with counts against without')
    for k in got:                                              # padded pairs: zeros both ways
        assert bool((got[k][padded] == 0).all()) and bool((plain[k][padded] == 0).all()), k
    same(run(e, v, g, m, H, counts), got, 'two runs')


@pytest.mark.parametrize('case,dtype', PARAMS, ids=hc.case_id)
def test_nothing_of_a_padded_pair_is_read(case, dtype):
    B, N, counts, H = CASES[case]
    e, v, g, m, padded, ref, plain = inputs(case, dtype)
    assert bool(padded.any())
    pe, pv, pg, pm = e.clone(), v.clone(), g.clone(), m.clone()
    for t in (pe, pv, pg, pm):
        t[padded] = NAN
    got = run(pe, pv, pg, pm, H, counts)
    same(got, plain, 'poisoned padding')


@pytest.mark.parametrize('case,dtype', PARAMS, ids=hc.case_id)
def test_counts_are_clamped(case, dtype):
    B, N, counts, H = CASES[case]
    e, v, g, m, padded, ref, plain = inputs(case, dtype)
    wild = [N + 7 if n == N else n for n in counts]           # above N: N
    assert wild != counts
    same(run(e, v, g, m, H, wild), plain, 'counts above N')
    # below 0: 0 -- the graph's results are zeros wherever its mask says so; an all-closed mask makes that the plain result too
    closed = torch.full_like(m, hi.LO)
    zero = run(e, v, g, closed, H, None)
    assert all(bool((t == 0).all()) for t in zero.values())
    same(run(e, v, g, closed, H, [-3] * B), zero, 'counts below 0')
    same(run(e, v, g, closed, H, [0] * B), zero, 'counts 0')


@pytest.mark.parametrize('case,dtype', PARAMS, ids=hc.case_id)
def test_against_the_float64_oracle(case, dtype):
    B, N, counts, H = CASES[case]
    e, v, g, m, padded, ref, plain = inputs(case, dtype)
    got = run(e, v, g, m, H, counts)
    tol = TOL[dtype]
    errs = {}
    for k in ref:
        a, b = got[k].double().cpu(), ref[k].double()
        errs[k] = (parity_log.record(float((a - b).norm() / (b.norm() + 1e-30))), tol * (1 if k == 'fwd' else 2))
    print(f'tiled triangular update with counts {case} {dtype} rel-L2', {k: f'{e_:.3e} < {b_:.3e}' for k, (e_, b_) in errs.items()})
    bad = {k: v_ for k, v_ in errs.items() if not v_[0] < v_[1]}
    assert not bad, bad


@pytest.mark.parametrize('case,dtype', PARAMS, ids=hc.case_id)
def test_packed_op_with_node_counts(case, dtype, monkeypatch):
    """ops.triangular_update_packed(node_counts=): forward + backward equal the call without counts; both launches got the counts"""
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_TRIUPD_TILED', True)
    B, N, counts, H = CASES[case]
    e, v, g, m, padded, ref, plain = inputs(case, dtype)
    nc = torch.tensor(counts, dtype=torch.int32, device='cuda')
    seen = []
    real = ops._launch

    def spy(entry, *args, **kw):
        seen.append((entry, args))
        return real(entry, *args, **kw)
    monkeypatch.setattr(ops, '_launch', spy)
    res = {}
    for key, kw in (('plain', {}), ('counts', dict(node_counts=nc))):
        ev = torch.cat((e, v), dim=-1).requires_grad_(True)
        out = ops.triangular_update_packed(ev, m, H, **kw)
        out.backward(g)
        torch.cuda.synchronize()
        res[key] = dict(fwd=out.detach(), de=ev.grad[..., :4 * H], dv=ev.grad[..., 4 * H:])
    same(res['counts'], res['plain'], 'packed op')
    same(res['plain'], plain, 'packed against contiguous')
    names = [s[0] for s in seen]
    assert names == ['tgt_triangular_update_tiled_fwd', 'tgt_triangular_update_tiled_bwd',
                     'tgt_triangular_update_tiled_fwd_counts', 'tgt_triangular_update_tiled_bwd_counts'], names
    assert seen[2][1][-1].value == nc.data_ptr() and seen[3][1][-1].value == nc.data_ptr()      # the backward: the forward's counts


def test_packed_op_checks_the_counts_and_the_lane_route_drops_them(monkeypatch):
    from tgt_amd import ops
    B, N, counts, H = CASES['N12']
    e, v, g, m, padded, ref, plain = inputs('N12', BF16)
    ev = torch.cat((e, v), dim=-1)
    for bad in (torch.tensor(counts, dtype=torch.int64, device='cuda'), torch.tensor(counts[:3], dtype=torch.int32, device='cuda')):
        with pytest.raises(RuntimeError, match='node_counts'):
            ops.triangular_update_packed(ev, m, H, node_counts=bad)
    nc = torch.tensor(counts, dtype=torch.int32, device='cuda')
    monkeypatch.setattr(ops, '_TRIUPD_TILED', False)          # the lane-per-head kernel: counts accepted and ignored
    a = ops.triangular_update_packed(ev, m, H, node_counts=nc)
    b = ops.triangular_update_packed(ev, m, H)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
