"""The conditions tests/test_hip_triplet_hard_inputs.py relies on, on the CPU: what tests/triplet_hard_inputs.py builds has the
properties that make a kernel error visible, the float64 oracle is finite on every GPU case, and three mutants of the oracle --
the mask read with its two node indices swapped -- are far from the oracle on pair_mask while a prefix mask
(golden_util.additive_mask) cannot tell them apart at all.

Also home of the oracle wrappers the GPU tests share: the oracle in the kernels' row layout, in float64 (the reference of every
comparison) or in float32 (the reference's OWN rounding error, which sets the fp32 bars)."""
import numpy as np
import pytest
import torch

import golden_util as gu
import triplet_hard_inputs as hi
from oracle import core

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
VARIANTS = ['gated', 'ungated', 'axial']

# ---- the GPU cases (tests/test_hip_triplet_hard_inputs.py parametrises over exactly these lists)
ATTENTION = ([(c, dt, 'gated') for c in ('S8', 'S1', 'M', 'K80', 'K128') for dt in (F32, BF16, F16)] +
             [(c, dt, v) for c in ('S8', 'M', 'K80') for dt in (F32, BF16) for v in ('ungated', 'axial')])
AGGREGATE = ([(c, dt, g) for c in ('S8', 'M', 'K80', 'K128') for dt in (F32, BF16) for g in (True, False)] +
             [(c, F16, g) for c in ('M', 'K80') for g in (True, False)])
TRIANGULAR = [(c, dt) for c in ('T20', 'T40') for dt in (F32, BF16, F16)]


def case_id(v):
    return str(v).replace('torch.', '')


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def to_ref(x_hm, idx):
    out = torch.empty_like(x_hm)
    out[..., idx] = x_hm
    return out


# ---- oracle wrappers: kernel row layout in, kernel channel order out, at precision `prec`
def attention_oracle(fused, d_out, mask3, C, H, variant, prec=torch.float64, mutant=False):
    """tests/test_hip_triplet_kb.py::oracle_run with a precision: {fwd, dqkv, deg} of ops.triplet_attention on `fused`.
    mutant: the OUTWARD direction reads the mask with its indices swapped (M[b,i,k] for M[b,k,i])."""
    from tgt_amd import layout
    gated, biased = variant == 'gated', variant != 'axial'
    f = fused.to(prec).requires_grad_(True)
    idx, oidx = layout.head_major_index(C, H), layout.va_cols_head_major(C, H)
    blk = lambda lo: torch.cat([to_ref(f[..., lo + q * C: lo + (q + 1) * C], idx) for q in range(3)], -1)
    nb = ((2 if gated else 1) * H) if biased else 0
    used = 6 * C + 2 * nb
    eg_in = f[..., 6 * C: 6 * C + nb] if biased else None
    eg_out = f[..., 6 * C + nb: used] if biased else None
    m = mask3.to(prec).unsqueeze(-1)
    if not mutant:
        va = core.triplet_attention_core(blk(0), eg_in, blk(3 * C), eg_out, m, H, gated, biased)
    else:
        outs = []
        for qkv, eg, inward in ((blk(0), eg_in, True), (blk(3 * C), eg_out, False)):
            q, k, v = (core.heads_minor(t, H) for t in qkv.split(C, dim=-1))
            bias, gate = (eg.split(H, dim=-1) if gated else (eg, None)) if biased else (None, None)
            outs.append(core._triplet_dir(q * (C // H) ** -0.5, k, v, bias, gate, m if inward else m.transpose(1, 2), inward))
        va = torch.cat(outs, dim=-1).reshape(*fused.shape[:3], 2 * C)
    va = va[..., oidx]
    (va * d_out.to(prec)).sum().backward()
    res = dict(fwd=va.detach(), dqkv=f.grad[..., :6 * C])
    if biased:
        res['deg'] = f.grad[..., 6 * C:used]
    return res


def aggregate_oracle(fused, d_out, mask3, C, H, gated, prec=torch.float64, mutant=False):
    """{fwd, dv, deg} of ops.triplet_aggregate on `fused` (tests/test_hip_ops.py::test_triplet_aggregate).  mutant: mask transposed."""
    from tgt_amd import layout
    f = fused.to(prec).requires_grad_(True)
    used = 2 * C + (4 if gated else 2) * H
    idx, oidx = layout.head_major_index(C, H), layout.va_cols_head_major(C, H)
    v_both = torch.cat([to_ref(f[..., p * C:(p + 1) * C], idx) for p in range(2)], -1)
    m = mask3.to(prec).unsqueeze(-1)
    va = core.triplet_aggregate_core(v_both, f[..., 2 * C:used], m.transpose(1, 2) if mutant else m, H, gated)[..., oidx]
    (va * d_out.to(prec)).sum().backward()
    return dict(fwd=va.detach(), dv=f.grad[..., :2 * C], deg=f.grad[..., 2 * C:used])


def triangular_oracle(e4, v4, d_out, mask3, H, prec=torch.float64, mutant=False):
    """{fwd, de, dv} of ops.triangular_update.  mutant: mask transposed."""
    e, v = e4.to(prec).requires_grad_(True), v4.to(prec).requires_grad_(True)
    m = mask3.to(prec).unsqueeze(-1)
    out = core.triangular_update_core(v, e, m.transpose(1, 2) if mutant else m, H)
    out.backward(d_out.to(prec))
    return dict(fwd=out.detach(), de=e.grad, dv=v.grad)


def f32_factors(oracle, hard_args, plain_args):
    """per compared quantity: e32_hard / e32_plain, the rel-L2 of the float32 oracle against the float64 oracle on the test's
    inputs over the same on standard-normal inputs with the prefix mask (same shape) -- how much the REFERENCE's own float32
    error grows on these inputs.  The fp32 bar of a quantity is 2e-6 * max(1, factor): the project's bar keeps its ratio to
    the reference's own float32 error.  Returns (factors, e32_hard, e32_plain)."""
    errs = []
    for args in (hard_args, plain_args):
        r64, r32 = oracle(*args, prec=torch.float64), oracle(*args, prec=torch.float32)
        errs.append({k: rel(r32[k], r64[k]) for k in r64})
    return {k: errs[0][k] / errs[1][k] for k in errs[0]}, errs[0], errs[1]


# ---- the mask
ALL_MASK_CASES = [(nn_, N) for _, N, nn_, _, _ in hi.CASES.values()] + [(nn_, N) for _, N, nn_, _ in hi.TRIANGULAR_CASES.values()] + \
                 [([17, 9], 17), ([32, 20], 32)]


@pytest.mark.parametrize('nn_,N', ALL_MASK_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_pair_mask_conditions(nn_, N):
    m = hi.pair_mask(nn_, N, np.random.default_rng(N))
    assert m.shape == (len(nn_), N, N) and m.dtype == torch.float32
    assert bool(((m == 0) | (m == hi.LO)).all())                            # values in {0, finfo.min}: never -inf
    open_ = m == 0
    blocks = hi.leading_blocks(N)
    assert len(blocks) == 2 + (N > 64) + (N > 96)
    for b, n in enumerate(nn_):
        assert not open_[b, n:].any() and not open_[b, :, n:].any()         # padded rows and columns wholly closed
        real = open_[b, :n, :n]
        assert bool(real.any(1).all()), 'a real row without an open key (inward)'
        assert bool(real.any(0).all()), 'a real column without an open key (outward)'
        assert 0.1 < float((~real).float().mean()) < 1.0
        if n > 2:
            assert not torch.equal(real, real.t()), 'the mask is symmetric'
        for start, step, width in blocks:
            rows = [i for i in range(start, n, step)]
            assert rows, (n, start, step)
            w = min(width, n)
            # the leading block wholly closed (but for the reopened diagonal entry, where it falls inside the block) ...
            for i in rows:
                closed_in, closed_out = ~open_[b, i, :w], ~open_[b, :w, i]
                if i < w:
                    closed_in[i] = closed_out[i] = True
                assert bool(closed_in.all()) and bool(closed_out.all()), (b, i, width)
            # ... and for at least one real row / column WHOLLY: the first live key lies behind the block
            if width < n:
                assert any(i >= width and not open_[b, i, :width].any() and open_[b, i, width:n].any() for i in rows), (b, width)
                assert any(i >= width and not open_[b, :width, i].any() and open_[b, width:n, i].any() for i in rows), (b, width)


def test_pair_mask_is_reproducible_and_counts_are_the_node_counts():
    nn_, N = [80, 71], 80
    a, b = hi.pair_mask(nn_, N, np.random.default_rng(3)), hi.pair_mask(nn_, N, np.random.default_rng(3))
    assert torch.equal(a, b)
    # the rule of tgt_mask_node_counts: 1 + the last column with an open entry
    cols = (a == 0).any(1)
    assert [1 + int(torch.nonzero(c).max()) for c in cols] == nn_


def test_hard_logits():
    H, N = 3, 10
    rng = np.random.default_rng(0)
    for gated in (True, False):
        nb = (2 if gated else 1) * H
        eg = torch.from_numpy(rng.standard_normal((2, N, N, 2 * nb)))
        out = hi.hard_logits(eg, H, N, gated)
        want = eg.clone()
        want[..., :H] = eg[..., :H] * 6
        want[:, :, N // 2:, :H] += 12
        want[..., nb:nb + H] = eg[..., nb:nb + H] * 6
        want[:, N // 2:, :, nb:nb + H] += 12
        if gated:
            want[..., H:nb] = eg[..., H:nb] * 4
            want[..., nb + H:] = eg[..., nb + H:] * 4
        assert torch.equal(out, want) and out is not eg


# ---- the float64 oracle is finite on every GPU case
@pytest.mark.parametrize('case,dtype,variant', ATTENTION, ids=case_id)
def test_attention_oracle_is_finite(case, dtype, variant):
    B, N, nn_, C, H = hi.CASES[case]
    fused, d_out, mask, used = hi.attention_inputs(hi.CASES[case], dtype, variant)
    assert torch.isfinite(fused.float()).all()
    r = attention_oracle(fused, d_out, mask, C, H, variant)
    assert all(torch.isfinite(t).all() for t in r.values())
    assert float(r['fwd'].norm()) > 0 and float(r['dqkv'].norm()) > 0


@pytest.mark.parametrize('case,dtype,gated', AGGREGATE, ids=case_id)
def test_aggregate_oracle_is_finite(case, dtype, gated):
    B, N, nn_, C, H = hi.CASES[case]
    fused, d_out, mask, used = hi.aggregate_inputs(hi.CASES[case], dtype, gated)
    r = aggregate_oracle(fused, d_out, mask, C, H, gated)
    assert all(torch.isfinite(t).all() for t in r.values())
    assert float(r['fwd'].norm()) > 0 and float(r['deg'].norm()) > 0


@pytest.mark.parametrize('case,dtype', TRIANGULAR, ids=case_id)
def test_triangular_oracle_is_finite(case, dtype):
    e4, v4, d_out, mask = hi.triangular_inputs(hi.TRIANGULAR_CASES[case], dtype)
    r = triangular_oracle(e4, v4, d_out, mask, hi.TRIANGULAR_CASES[case][3])
    assert all(torch.isfinite(t).all() for t in r.values())
    assert float(r['fwd'].norm()) > 0


def test_hard_inputs_peak_the_softmax_and_saturate_the_gates():
    """what `hard_logits` is for: on the live keys of M's inward direction the largest softmax weight of a row is mostly close to 1
    (never so with unit-variance logits at N = 40), the row maximum lies in the upper half of the keys, and gates reach both ends"""
    B, N, nn_, C, H = hi.CASES['M']
    stats = {}
    for hard in (True, False):
        fused, _, mask, used = hi.attention_inputs(hi.CASES['M'], torch.float64, 'gated', hard=hard)
        e, g = fused[..., 6 * C:6 * C + H], fused[..., 6 * C + H:6 * C + 2 * H]
        p = torch.softmax(e + mask.unsqueeze(-1), dim=2)[0]                      # graph 0: every node real
        gate = torch.sigmoid(g)[0][mask[0] == 0]
        stats[hard] = (float(p.max(1).values.median()), float((p.argmax(1) >= N // 2).float().mean()),
                       float((gate < 1e-3).float().mean()), float((gate > 1 - 1e-3).float().mean()))
    assert stats[True][0] > 0.5 > 0.3 > stats[False][0], stats
    assert stats[True][1] > 0.9, stats
    assert stats[True][2] > 0.02 and stats[True][3] > 0.02 and stats[False][2] == 0 and stats[False][3] == 0, stats


# ---- the mutants: what a prefix mask cannot see
def _mutant_distances(oracle, args_of):
    out = {}
    for name, hard_mask in (('pair', True), ('prefix', False)):
        args = args_of(hard_mask)
        out[name] = rel(oracle(*args, mutant=True)['fwd'], oracle(*args)['fwd'])
    return out


def test_mutant_outward_direction_sees_the_transposed_mask():
    """core._triplet_dir's outward direction given M[b,i,k] instead of M[b,k,i] (B = 2, N = 40, C = 64, H = 4): more than 0.1 away
    from the oracle on pair_mask (a condition that the inputs discriminate, not a tolerance), exactly 0 on additive_mask"""
    case = hi.CASES['M']
    B, N, nn_, C, H = case

    def args_of(hard_mask):
        fused, d_out, mask, _ = hi.attention_inputs(case, torch.float64, 'gated')
        m = mask if hard_mask else gu.additive_mask(nn_, N, torch.float32).reshape(B, N, N)
        return fused, d_out, m, C, H, 'gated'
    d = _mutant_distances(attention_oracle, args_of)
    print('outward direction sees the transposed mask:', d)
    assert d['pair'] > 0.1 and d['prefix'] == 0.0, d


def test_mutant_ungated_aggregate_with_the_mask_transposed():
    case = hi.CASES['M']
    B, N, nn_, C, H = case

    def args_of(hard_mask):
        fused, d_out, mask, _ = hi.aggregate_inputs(case, torch.float64, False)
        m = mask if hard_mask else gu.additive_mask(nn_, N, torch.float32).reshape(B, N, N)
        return fused, d_out, m, C, H, False
    d = _mutant_distances(aggregate_oracle, args_of)
    print('ungated aggregate, mask transposed:', d)
    assert d['pair'] > 0.1 and d['prefix'] == 0.0, d


def test_mutant_triangular_update_with_the_mask_transposed():
    B, N, nn_, H = 2, 40, [40, 33], 4

    def args_of(hard_mask):
        e4, v4, d_out, mask = hi.triangular_inputs((B, N, nn_, H), torch.float64)
        m = mask if hard_mask else gu.additive_mask(nn_, N, torch.float32).reshape(B, N, N)
        return e4, v4, d_out, m, H
    d = _mutant_distances(triangular_oracle, args_of)
    print('triangular update, mask transposed:', d)
    assert d['pair'] > 0.1 and d['prefix'] == 0.0, d


def test_f32_factors_are_the_reference_s_own_error_growth():
    """the fp32 bars of the GPU tests come from here: the float32 oracle's error against the float64 oracle, hard over plain, at
    N = 40 -- of the order of 1 to a few, never from a kernel's measured error"""
    case = hi.CASES['M']
    B, N, nn_, C, H = case
    mk = lambda hard: hi.attention_inputs(case, F32, 'gated', hard=hard)[:3] + (C, H, 'gated')
    factors, hard, plain = f32_factors(attention_oracle, mk(True), mk(False))
    print('float32 oracle vs float64, N = 40: hard', hard, 'plain', plain, 'factors', factors)
    assert all(0.3 < f < 30 for f in factors.values()), factors
    assert all(5e-9 < e < 2e-6 for e in list(hard.values()) + list(plain.values())), (hard, plain)
