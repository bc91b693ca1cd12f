"""The attention dropout inside the triplet kernels honours the registered device step counter (tgt_set_seed_counter,
csrc/common.hpp step_seed): with the counter at c a call equals the call without a counter and with the seed
(seed + c * 0x9E3779B97F4A7C15) mod 2^64, forward and backward; no counter = c = 0 = today's result; p = 0 never looks at it.
Every comparison is bitwise (same kernel, same arguments but the seed): no tolerance is involved.

One N per kernel family: 8 (32-wide tiles), 40 (33..64 nodes), 72 (key-blocked kernels, second key block partly filled); the
projection-fused aggregate kernels at C = 256, H = 16: N = 8 (tgt_triplet_aggregate_proj_fwd) and 40 (..._proj64_fwd)."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
P, SEED = 0.5, 0x243F6A8885A308D3                # p = 0.5: two patterns cannot coincide by chance; a 63-bit seed
B, H, D = 2, 2, 16
NODES = {8: [8, 5], 40: [40, 33], 72: [72, 67]}

ATT = [(v, n, BF16) for v in ('gated', 'ungated', 'axial') for n in (8, 40, 72)] + [('gated', 40, F16)]
AGG = [(g, n, BF16) for g in (True, False) for n in (8, 40, 72)] + [(True, 72, F16)]
PROJ = [(g, n, BF16) for g in (True, False) for n in (8, 40)] + [(True, 8, F16)]


def _rnd(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape))


def _att_case(variant, N, dtype):
    from tgt_amd import ops
    L = ops.TripletLayout(H * D, H, gated=variant == 'gated', biased=variant != 'axial')
    rng = np.random.default_rng(N)
    fused, d_out = _rnd(rng, B, N, N, L.width).to(dtype).cuda(), _rnd(rng, B, N, N, 2 * H * D).to(dtype).cuda()
    mask3 = gu.additive_mask(NODES[N], N, torch.float32).reshape(B, N, N).cuda()

    def run(p, seed):
        x = fused.clone().requires_grad_(True)
        out = ops.triplet_attention(x, mask3, L, dropout=(p, seed))
        out.backward(d_out)
        return out.detach(), x.grad[..., :L.used]
    return run


def _agg_case(gated, N, dtype):
    from tgt_amd import ops
    L = ops.AggregateLayout(H * D, H, gated=gated)
    rng = np.random.default_rng(100 + N)
    fused, d_out = _rnd(rng, B, N, N, L.width).to(dtype).cuda(), _rnd(rng, B, N, N, 2 * H * D).to(dtype).cuda()
    mask3 = gu.additive_mask(NODES[N], N, torch.float32).reshape(B, N, N).cuda()

    def run(p, seed):
        x = fused.clone().requires_grad_(True)
        out = ops.triplet_aggregate(x, mask3, L, dropout=(p, seed))
        out.backward(d_out)
        return out.detach(), x.grad[..., :L.used]
    return run


def _proj_case(gated, N, dtype):
    """the inference entry points that project V inside the aggregate kernel (no autograd): the argument block of
    ops.projected_triplet_aggregate's fused path, with the narrow E/G rows in a tensor of their own"""
    from tgt_amd import ops, _lib
    CW, HP = 256, 16
    L = ops.AggregateLayout(CW, HP, gated=gated)
    assert L.width == L.used
    rng = np.random.default_rng(200 + N)
    x = _rnd(rng, B, N, N, CW).to(dtype).cuda()
    w, b = (_rnd(rng, L.width, CW) * CW ** -0.5).to(dtype).cuda(), (_rnd(rng, L.width) * 0.1).to(dtype).cuda()
    mask3 = gu.additive_mask(NODES[N], N, torch.float32).reshape(B, N, N).cuda()
    eg = torch.addmm(b[2 * CW:], x.view(-1, CW), w[2 * CW:].t()).view(B, N, N, L.used - 2 * CW)
    entry = 'tgt_triplet_aggregate_proj_fwd' if N <= 32 else 'tgt_triplet_aggregate_proj64_fwd'

    def run(p, seed):
        out = torch.full((B, N, N, 2 * CW), float('nan'), dtype=dtype, device='cuda')
        a = ops._agg_proj_args(eg, mask3, out, L, (p, seed))
        assert a.dropout_seed == seed                      # the argument block carries all 64 bits, unsigned
        code = getattr(_lib.lib(), entry)(C.byref(a), ops._ptr(x), CW, ops._ptr(w), ops._ptr(b), ops._stream())
        torch.cuda.synchronize()
        assert code == 0 and not torch.isnan(out).any()
        return (out,)
    return run


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _check(run):
    from tgt_amd import ops

    def with_counter(c, p=P, seed=SEED):
        ctr = torch.full((1,), c, dtype=torch.int64, device='cuda')
        ops.set_seed_counter(ctr)
        try:
            res = run(p, seed)
            torch.cuda.synchronize()
            assert int(ctr) == c                           # the kernels only read it
            return res
        finally:
            ops.set_seed_counter(None)

    try:
        plain = run(P, SEED)
        stepped = ops.step_seed(SEED, 3)
        assert stepped >= 2 ** 63                          # the unsigned half of the range: a narrowing argument path would show
        # 1. counter at 3 == no counter, seed + 3 * golden (mod 2^64): output and every gradient
        assert _same(with_counter(3), run(P, stepped))
        # 2. counter at 0 == no counter
        c0 = with_counter(0)
        assert _same(c0, plain)
        # 3. the patterns of successive counter values differ, in the output and in every gradient
        c1, c2 = with_counter(1), with_counter(2)
        for x, y in ((c0, c1), (c0, c2), (c1, c2)):
            assert not any(torch.equal(s, t) for s, t in zip(x, y))
        # 4. p = 0: independent of the counter
        assert _same(with_counter(3, p=0.0), run(0.0, SEED))
        assert all(torch.isfinite(t).all() for t in plain + c1)
    finally:
        ops.set_seed_counter(None)
        ops.graph_safe_rng(False)


@pytest.mark.parametrize('variant,N,dtype', ATT)
def test_triplet_attention_dropout_follows_the_counter(variant, N, dtype):
    _check(_att_case(variant, N, dtype))


@pytest.mark.parametrize('gated,N,dtype', AGG)
def test_triplet_aggregate_dropout_follows_the_counter(gated, N, dtype):
    _check(_agg_case(gated, N, dtype))


@pytest.mark.parametrize('gated,N,dtype', PROJ)
def test_projection_fused_aggregate_dropout_follows_the_counter(gated, N, dtype):
    _check(_proj_case(gated, N, dtype))
