"""The triplet kernels on pairwise masks and large logits (tests/triplet_hard_inputs.py), against the float64 oracle on the CPU, on
the GPU: triplet attention at N <= 32, 33..64 and 65..128, triplet aggregate, the projection-fused forwards, the triangular update
and the count-skipping kernels.  What a symmetric prefix mask and unit-variance logits cannot show (tests/test_triplet_hard_inputs.py
demonstrates it on the CPU): the mask read with its indices swapped in one direction, an online softmax whose LEADING key blocks
are closed (running maximum of finfo.min size, then rescaled away), a row maximum that moves by tens of units between key blocks,
saturated gates, and node counts taken from a mask that is not a prefix mask.

Bars (rel-L2 against float64 on the values as the kernel sees them; gradients twice the forward bar):
  16-bit  the project's own, unchanged (tests/test_hip_ops.py): bf16 8e-3, fp16 1e-3 -- storage rounding dominates and does not grow
          with the size of the logits.
  fp32    per compared quantity 2e-6 * max(1, e32_hard / e32_plain), where e32 is the rel-L2 of the FLOAT32 CPU oracle against the
          float64 oracle, on the test's inputs (hard) and on standard-normal inputs with the prefix mask at the same shape (plain):
          the reference's own float32 error grows on these inputs, and the bar keeps the ratio to it that 2e-6 has on plain inputs.
          Both are computed here (test_triplet_hard_inputs.f32_factors); nothing comes from a kernel's measured error.
profiles/parity_errors_hard_inputs.json records the measured errors (TGT_PARITY_LOG)."""
import numpy as np
import pytest
import torch

import parity_log
import test_hip_triplet_agg_proj as agg_proj
import test_triplet_hard_inputs as hc
import triplet_hard_inputs as hi

pytestmark = pytest.mark.gpu

TOL = parity_log.Tol({torch.float32: 2e-6, torch.bfloat16: 8e-3, torch.float16: 1e-3})
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return parity_log.record(float((a - b).norm() / (b.norm() + 1e-30)))


def rnd(rng, *shape, scale=1.0):
    return torch.from_numpy(rng.standard_normal(shape) * scale)


_factors = {}


def bars(dtype, key, oracle, hard_args, plain_args):
    """{quantity: forward-level bar}.  fp32: 2e-6 * max(1, e32_hard / e32_plain) (module docstring); hard_args / plain_args are
    callables returning the oracle's arguments, evaluated for fp32 only, once per key"""
    tol = TOL[dtype]
    if dtype is not F32:
        return None, tol
    if key not in _factors:
        _factors[key] = hc.f32_factors(oracle, hard_args(), plain_args())
    factors, e_hard, e_plain = _factors[key]
    print(f'float32 oracle vs float64 {key}: hard {e_hard} plain {e_plain}')
    return factors, tol


def check(got, ref, factors, tol, what):
    """finite; forward below its bar, every gradient below twice its bar"""
    for k, t in got.items():
        assert torch.isfinite(t).all(), (what, k, 'not finite')
    errs = {k: rel(got[k], ref[k]) for k in ref}
    limit = {k: tol * (1.0 if factors is None else max(1.0, factors[k])) * (1 if k == 'fwd' else 2) for k in ref}
    print(what, 'rel-L2', {k: f'{v:.3e}' for k, v in errs.items()}, 'bars', {k: f'{v:.3e}' for k, v in limit.items()},
          '' if factors is None else {k: f'x{max(1.0, v):.2f}' for k, v in factors.items()})
    bad = {k: (errs[k], limit[k]) for k in ref if not errs[k] < limit[k]}
    assert not bad, (what, bad)
    return errs


# ------------------------------------------------------------------------------------------------------------ 1. triplet attention
def run_attention(fused, d_out, mask, L, used, node_counts=None):
    from tgt_amd import ops
    C = L.C
    fx = fused.cuda().requires_grad_(True)
    va = ops.triplet_attention(fx, mask.cuda(), L, node_counts=node_counts)
    va.backward(d_out.cuda())
    torch.cuda.synchronize()
    got = dict(fwd=va.detach(), dqkv=fx.grad[..., :6 * C])
    if L.biased:
        got['deg'] = fx.grad[..., 6 * C:used]
    return got


@pytest.mark.parametrize('case,dtype,variant', hc.ATTENTION, ids=hc.case_id)
def test_triplet_attention(case, dtype, variant):
    from tgt_amd import ops
    B, N, nn_, C, H = hi.CASES[case]
    L = ops.TripletLayout(C, H, gated=variant == 'gated', biased=variant != 'axial')
    fused, d_out, mask, used = hi.attention_inputs(hi.CASES[case], dtype, variant)
    assert (L.width, L.used) == (fused.shape[-1], used)
    ref = hc.attention_oracle(fused, d_out, mask, C, H, variant)
    mk = lambda hard: (lambda: hi.attention_inputs(hi.CASES[case], F32, variant, hard=hard)[:3] + (C, H, variant))
    factors, tol = bars(dtype, ('attention', case, variant), hc.attention_oracle, mk(True), mk(False))
    check(run_attention(fused, d_out, mask, L, used), ref, factors, tol, f'attention {case} {variant} {dtype}')


# ------------------------------------------------------------------------------------------------------------ 2. triplet aggregate
@pytest.mark.parametrize('case,dtype,gated', hc.AGGREGATE, ids=hc.case_id)
def test_triplet_aggregate(case, dtype, gated):
    """gated: the outward direction is unmasked (reference quirk); ungated: both directions masked (TGT_TRI_MASK_OUT)"""
    from tgt_amd import ops
    B, N, nn_, C, H = hi.CASES[case]
    L = ops.AggregateLayout(C, H, gated=gated)
    fused, d_out, mask, used = hi.aggregate_inputs(hi.CASES[case], dtype, gated)
    assert (L.width, L.used) == (fused.shape[-1], used)
    ref = hc.aggregate_oracle(fused, d_out, mask, C, H, gated)
    mk = lambda hard: (lambda: hi.aggregate_inputs(hi.CASES[case], F32, gated, hard=hard)[:3] + (C, H, gated))
    factors, tol = bars(dtype, ('aggregate', case, gated), hc.aggregate_oracle, mk(True), mk(False))
    fx = fused.cuda().requires_grad_(True)
    va = ops.triplet_aggregate(fx, mask.cuda(), L)
    va.backward(d_out.cuda())
    torch.cuda.synchronize()
    got = dict(fwd=va.detach(), dv=fx.grad[..., :2 * C], deg=fx.grad[..., 2 * C:used])
    check(got, ref, factors, tol, f'aggregate {case} gated={gated} {dtype}')


# ------------------------------------------------------------------------------------------------------------ 3. projection-fused paths
PROJ_CASE = (2, 17, [17, 9], 256, 16)
INFER_CASE = (2, 32, [32, 20], 256, 16)        # (the predicates of both inference kernels stop at 32 nodes: no 65..128 case exists)


def projection_inputs(case, dtype, variant, seed, hard_rows):
    """x, w, b in dtype (w, b: the fused projection in kernel order), d_out, pair_mask; hard_rows: the E rows of w * 6, the G rows * 4"""
    from tgt_amd import ops
    B, N, nn_, C, H = case
    gated, biased = variant == 'gated', variant != 'axial'
    L = ops.TripletLayout(C, H, gated=gated, biased=biased)
    assert L.width == L.used
    rng = np.random.default_rng(seed)
    x = rnd(rng, B, N, N, C)
    w = rnd(rng, L.width, C) * C ** -0.5
    b = rnd(rng, L.width) * 0.1
    d_out = rnd(rng, B, N, N, 2 * C)
    mask = hi.pair_mask(nn_, N, rng)
    if hard_rows and biased:
        nb = (2 if gated else 1) * H
        for d in (0, 1):
            lo = 6 * C + d * nb
            w[lo:lo + H] *= 6.0
            if gated:
                w[lo + H:lo + nb] *= 4.0
    return L, x.to(dtype), w.to(dtype), b.to(dtype), d_out.to(dtype), mask


def projected_attention_oracle(x, w, b, d_out, mask, C, H, variant):
    """float64: linear -> attention_oracle's arithmetic; {fwd, dx, dw, db}"""
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    f64 = torch.nn.functional.linear(x64, w64, b64)
    r = hc.attention_oracle(f64.detach(), d_out, mask, C, H, variant)
    used = w.shape[0]
    g = torch.zeros_like(f64)
    g[..., :6 * C] = r['dqkv']
    if 'deg' in r:
        g[..., 6 * C:used] = r['deg']
    f64.backward(g)
    return dict(fwd=r['fwd'], dx=x64.grad, dw=w64.grad, db=b64.grad)


@pytest.mark.parametrize('dtype', [BF16, F16], ids=hc.case_id)
@pytest.mark.parametrize('variant', hc.VARIANTS)
def test_projection_fused_training(dtype, variant, monkeypatch):
    """tgt_triplet_attention_proj_fwd and its backward (tests/test_hip_ops.py::test_projection_fused_triplet_attention_vs_oracle) on
    pair_mask, with the E rows of the projection * 6 and the G rows * 4: forward, dx, dw, db"""
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_TRI_PROJ', True)
    monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 1)
    B, N, nn_, C, H = PROJ_CASE
    L, x, w, b, d_out, mask = projection_inputs(PROJ_CASE, dtype, variant, 1700 + hc.VARIANTS.index(variant), hard_rows=True)
    assert ops._proj_fused_ok(torch.empty(B, N, N, C), N, L, dtype), 'shape must be one the projection-fused kernel takes'
    ref = projected_attention_oracle(x, w, b, d_out, mask, C, H, variant)
    xin, win, bin_ = (t.cuda().requires_grad_(True) for t in (x, w, b))
    va = ops.projected_triplet_attention(xin, win, bin_, mask.cuda(), L)
    va.backward(d_out.cuda())
    torch.cuda.synchronize()
    got = dict(fwd=va.detach(), dx=xin.grad, dw=win.grad, db=bin_.grad)
    check(got, ref, None, TOL[dtype], f'projection-fused training {variant} {dtype}')


@pytest.mark.parametrize('variant', hc.VARIANTS)
def test_projection_fused_attention_inference(variant, monkeypatch):
    """the forward without Q/K/V stores (tests/test_hip_triplet_proj_infer.py: TGT_TRI_PROJ_INFER under no_grad) on pair_mask, bf16"""
    from tgt_amd import ops, _lib
    monkeypatch.setattr(ops, '_TRI_PROJ', True)
    monkeypatch.setattr(ops, '_TRI_PROJ_INFER', True)
    monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 1)
    B, N, nn_, C, H = INFER_CASE
    L, x, w, b, d_out, mask = projection_inputs(INFER_CASE, BF16, variant, 3200 + hc.VARIANTS.index(variant), hard_rows=False)
    assert ops._proj_fused_ok(torch.empty(B, N, N, C), N, L, BF16), 'shape must be one the projection-fused kernel takes'
    calls, real = [], ops._tri_args

    def spy(fused, *args, **kw):
        a = real(fused, *args, **kw)
        calls.append((fused, int(a.flags)))
        return a
    monkeypatch.setattr(ops, '_tri_args', spy)
    with torch.no_grad():
        out = ops.projected_triplet_attention(x.cuda(), w.cuda(), b.cuda(), mask.cuda(), L)
    torch.cuda.synchronize()
    assert len(calls) == 1 and calls[0][0] is None and calls[0][1] & _lib.TRI_NO_QKV_STORE      # the kernel that keeps Q/K/V on chip
    ref = projected_attention_oracle(x, w, b, d_out, mask, C, H, variant)
    check(dict(fwd=out), dict(fwd=ref['fwd']), None, TOL[BF16], f'projection-fused attention inference {variant}')


@pytest.mark.parametrize('gated', [True, False], ids=['gated', 'ungated'])
def test_projection_fused_aggregate_inference(gated, monkeypatch):
    """tgt_triplet_aggregate_proj_fwd called as tests/test_hip_triplet_agg_proj.py calls it (V = NULL: no other kernel can answer)
    on pair_mask, bf16"""
    from tgt_amd import ops, layout
    from oracle import core
    B, N, nn_, C, H = INFER_CASE
    assert (C, H) == (agg_proj.CW, agg_proj.H)
    L = ops.AggregateLayout(C, H, gated=gated)
    rng = np.random.default_rng(3300 + int(gated))
    x = rnd(rng, B, N, N, C).to(BF16)
    w = (rnd(rng, L.width, C) * C ** -0.5).to(BF16)
    b = (rnd(rng, L.width) * 0.1).to(BF16)
    mask = hi.pair_mask(nn_, N, rng)
    c = dict(B=B, N=N, L=L, dtype=BF16, gated=gated, x=x.cuda(), w=w.cuda(), b=b.cuda(), mask3=mask.cuda())
    monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 1)            # (the fused kernel also below 65536 edge rows)
    assert ops._agg_proj_ok(c['x'], N, L, BF16), 'shape must be one the projection-fused aggregate kernel takes'
    c['eg'] = torch.addmm(c['b'][2 * C:], c['x'].view(-1, C), c['w'][2 * C:].t()).view(B, N, N, L.used - 2 * C)
    code, out = agg_proj._proj_fwd(c)
    assert code == 0 and not torch.isnan(out).any()
    f64 = torch.nn.functional.linear(x.double(), w.double(), b.double())
    idx, oidx = layout.head_major_index(C, H), layout.va_cols_head_major(C, H)
    v_both = torch.cat([hc.to_ref(f64[..., p * C:(p + 1) * C], idx) for p in range(2)], -1)
    ref = core.triplet_aggregate_core(v_both, f64[..., 2 * C:L.used], mask.double().unsqueeze(-1), H, gated)[..., oidx]
    check(dict(fwd=out), dict(fwd=ref), None, TOL[BF16], f'projection-fused aggregate inference gated={gated}')


# ------------------------------------------------------------------------------------------------------------ 4. triangular update
@pytest.mark.parametrize('case,dtype', hc.TRIANGULAR, ids=hc.case_id)
def test_triangular_update(case, dtype):
    """M sits inside four sigmoids; gate chunks * 4.  (The first fp16 comparison of this kernel.)"""
    from tgt_amd import ops
    B, N, nn_, H = hi.TRIANGULAR_CASES[case]
    e4, v4, d_out, mask = hi.triangular_inputs(hi.TRIANGULAR_CASES[case], dtype)
    ref = hc.triangular_oracle(e4, v4, d_out, mask, H)
    mk = lambda hard: (lambda: hi.triangular_inputs(hi.TRIANGULAR_CASES[case], F32, hard=hard) + (H,))
    factors, tol = bars(dtype, ('triangular', case), hc.triangular_oracle, mk(True), mk(False))
    ex, vx = e4.cuda().requires_grad_(True), v4.cuda().requires_grad_(True)
    out = ops.triangular_update(ex, vx, mask.cuda(), H)
    out.backward(d_out.cuda())
    torch.cuda.synchronize()
    check(dict(fwd=out.detach(), de=ex.grad, dv=vx.grad), ref, factors, tol, f'triangular update {case} {dtype}')


# ------------------------------------------------------------------------------------------------------------ 5. counts on a non-prefix mask
COUNTS = [('M', F32), ('M', BF16), ('M', F16), ('K80', F32), ('K80', BF16)]


@pytest.mark.parametrize('case,dtype', COUNTS, ids=hc.case_id)
def test_node_counts_from_a_pair_mask(case, dtype, monkeypatch):
    """tgt_mask_node_counts on a mask that is not a prefix mask, and the count-skipping kernels behind it (N <= 64: TGT_TRI_RAGGED's
    entry points; K80: TGT_TRI_COUNTS_KB).  The random closings are inside the real block and the open diagonal keeps column n - 1
    open, so the counts are num_nodes; the run with them equals the run without on the real block bit for bit and meets the oracle
    there; one open entry in the last column makes the count N, and then the two runs are equal everywhere."""
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_TRI_RAGGED_KB', True)
    B, N, nn_, C, H = hi.CASES[case]
    L = ops.TripletLayout(C, H)
    real = (hi.prefix_mask(nn_, N) == 0).unsqueeze(-1)                  # (B,N,N,1): the real block of every graph
    assert not real.all()

    def inputs(dt, hard=True):
        fused, d_out, mask, used = hi.attention_inputs(hi.CASES[case], dt, 'gated', hard=hard)
        return fused, d_out * real.to(dt), mask, used                   # the cotangent of every padded row and column is zero
    fused, d_out, mask, used = inputs(dtype)
    counts = ops.mask_node_counts(mask.cuda())
    assert counts.dtype == torch.int32 and counts.tolist() == nn_
    plain = run_attention(fused, d_out, mask, L, used)
    skipping = run_attention(fused, d_out, mask, L, used, node_counts=counts)
    for b, n in enumerate(nn_):
        for k in plain:
            assert torch.equal(skipping[k][b, :n, :n], plain[k][b, :n, :n]), (k, 'real block', b)
    ref = hc.attention_oracle(fused, d_out, mask, C, H, 'gated')
    mk = lambda hard: (lambda: inputs(F32, hard)[:3] + (C, H, 'gated'))
    factors, tol = bars(dtype, ('counts', case), hc.attention_oracle, mk(True), mk(False))
    realc = real.cuda()
    check({k: v * realc for k, v in skipping.items()}, {k: v * real for k, v in ref.items()}, factors, tol, f'counts {case} {dtype}')
    # one open entry in the last column of graph 1: nothing may be skipped any more
    opened = mask.clone()
    assert opened[1, 0, N - 1] == hi.LO
    opened[1, 0, N - 1] = 0.0
    counts = ops.mask_node_counts(opened.cuda())
    assert counts.tolist() == [nn_[0], N]
    plain = run_attention(fused, d_out, opened, L, used)
    skipping = run_attention(fused, d_out, opened, L, used, node_counts=counts)
    for k in plain:
        assert torch.isfinite(plain[k]).all() and torch.equal(skipping[k], plain[k]), (k, 'count = N')
