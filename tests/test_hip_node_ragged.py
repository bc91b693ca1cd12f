"""Node attention with per-graph node counts (tgt_node_attention_fwd_counts / _bwd_counts, include/tgt_hip.h), on the GPU.

Families that honour the count: the key-blocked forward (KB_FWD), the MFMA32 and TILES16 backwards.  Everything else accepts and
ignores it.  Each case asserts with tgt_node_attention_family that it takes the family it names, before anything is launched.

The entry points are called as ops.node_attention calls them (ops._node_args), straight on the library, so that the statistics,
the output buffers (filled with NaN before every call: a zero must have been WRITTEN) and the cotangents are in the test's hands.

Masks are prefix masks built from the clamped counts, closed value finfo.min; the variant 'dropped' adds what source dropout
adds (another finfo.min on whole key columns): column 1 of graph 0, and every real column of the smallest non-empty graph, whose
real rows then have no open key at all.  Every mask is checked on the CPU against the premise of the contract (closed wherever
l >= n or m >= n).

Exactness is torch.equal on the real block [0, n) x [0, n) against the call without counts, whose cotangents are zero on the
padding; the call with counts gets random finite cotangents there (or NaN: `poison`).  lse and gsum are compared on every real
row, the rows without an open key included.  Oracle bars: those of tests/test_hip_node_families.py, unchanged."""
import ctypes as C
import functools

import pytest
import torch

import node_family_cases as nfc
from oracle import core

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
TOL = {F32: 2e-6, BF16: 8e-3, F16: 1e-3}

# (B, N, counts, H, D), forward family, backward family
HONOUR = [
    ((3, 32, (32, 17, 5), 32, 8), 'KB_FWD', 'MFMA32'),       # a full graph, a partial second block, a skipped query block and key block
    ((2, 20, (20, 7), 32, 12), 'KB_FWD', 'MFMA32'),          # N below the tile
    ((2, 48, (48, 16), 32, 12), 'KB_FWD', 'TILES16'),        # a count exactly on a block edge
    ((3, 64, (64, 33, 1), 32, 16), 'KB_FWD', 'TILES16'),     # a one-node graph
]
CLAMP = ((3, 32, (0, 40, -3), 32, 8), 'KB_FWD', 'MFMA32')    # an all-zero graph, counts above N and below 0
IGNORE = [
    ((1, 80, (41,), 32, 8), BF16, 'KB_FWD', 'KB_BWD'),       # (the backward is the family under test; the forward honours)
    ((2, 12, (12, 5), 4, 8), F32, 'LANE', 'LANE'),
]


def _id(p):
    if isinstance(p, torch.dtype):
        return str(p).replace('torch.', '')
    if isinstance(p, tuple) and isinstance(p[0], tuple):
        return '-'.join(map(str, p[0][:2])) + '-c' + '_'.join(map(str, p[0][2])) + '-' + p[-1]
    return None


def clamped(case):
    return [min(max(c, 0), case[1]) for c in case[2]]


@functools.lru_cache(maxsize=None)
def host_inputs(case, dtype, variant):
    """qkv, eg, d_vatt, d_hhat (CPU, dtype), the (B,N,N) float32 mask, and the real-pair / real-row indicator"""
    B, N, counts, H, D = case
    qkv, eg, d_v, d_h, _ = nfc.inputs((B, N, H * D, H), dtype, 'plain')
    n = torch.tensor(clamped(case))
    real = torch.arange(N)[None, :] < n[:, None]                          # (B,N)
    pair = real[:, :, None] & real[:, None, :]
    lo = torch.finfo(torch.float32).min
    mask = (~pair).float() * lo
    if variant == 'dropped':
        drop = torch.zeros(B, 1, N)
        if n[0] > 1:
            drop[0, 0, 1] = lo
        small = min((c, b) for b, c in enumerate(n.tolist()) if c > 0)[1]
        drop[small, 0, :n[small]] = lo
        mask = mask + drop                                                # (finfo.min + finfo.min = -inf on the padding of those columns)
    # the premise of the contract: every pair with l >= n or m >= n is closed
    assert bool((mask[~pair] <= lo / 2).all())
    if variant == 'dropped':
        open_row = ((mask > lo / 2) & pair).any(-1)
        assert bool((real & ~open_row).any())                             # some real row has no open key at all
    return qkv, eg, d_v, d_h, mask, pair, real


class Call:
    """one forward + backward through the library's entry points on device tensors"""

    def __init__(self, case, qkv, eg, mask, d_v, d_h, counts=None, hhat_scale=None, fwd_counts=True, scale_degree=True):
        from tgt_amd import ops
        B, N, _, H, D = case
        self.qkv, self.eg, self.mask, self.H = qkv, eg, mask, H
        W = H * D
        nan = float('nan')
        self.vatt = torch.full((B, N, W), nan, dtype=qkv.dtype, device='cuda')
        self.hhat = torch.full((B, N, N, H), nan, dtype=qkv.dtype, device='cuda')
        self.lse = torch.full((B, N, H), nan, dtype=F32, device='cuda')
        self.gsum = torch.full((B, N, H), nan, dtype=F32, device='cuda')
        self.d_qkv, self.d_eg = torch.full_like(qkv, nan), torch.full_like(eg, nan)
        a, _ = ops._node_args(qkv, eg, mask, H, scale_degree, False)
        a.vatt, a.hhat, a.lse, a.gsum = self.vatt.data_ptr(), self.hhat.data_ptr(), self.lse.data_ptr(), self.gsum.data_ptr()
        a.hhat_scale = ops._ptr(hhat_scale)
        self.family = (nfc.family(qkv, eg, mask, H, 0), nfc.family(qkv, eg, mask, H, 1))
        if counts is None or not fwd_counts:
            ops._launch('tgt_node_attention_fwd', C.byref(a))
        else:
            ops._launch('tgt_node_attention_fwd_counts', C.byref(a), ops._ptr(counts))
        a.d_vatt, a.d_hhat, a.d_qkv, a.d_eg = d_v.data_ptr(), d_h.data_ptr(), self.d_qkv.data_ptr(), self.d_eg.data_ptr()
        if counts is None:
            ops._launch('tgt_node_attention_bwd', C.byref(a))
        else:
            ops._launch('tgt_node_attention_bwd_counts', C.byref(a), ops._ptr(counts))
        torch.cuda.synchronize()


def assert_families(call, fwd, bwd):
    assert call.family == (nfc.family_id(fwd), nfc.family_id(bwd)), call.family


def device_inputs(case, dtype, variant):
    qkv, eg, d_v, d_h, mask, pair, real = host_inputs(case, dtype, variant)
    return [t.cuda() for t in (qkv, eg, d_v, d_h, mask, pair, real)]


def zero_padding(d_v, d_h, pair, real):
    return d_v * real[..., None].to(d_v.dtype), d_h * pair[..., None].to(d_h.dtype)


def check_real_block(got, ref, pair, real):
    """torch.equal on the real block, nothing NaN in it"""
    for name in ('vatt', 'lse', 'gsum'):
        g, r = getattr(got, name)[real], getattr(ref, name)[real]
        assert not torch.isnan(g.float()).any() and torch.equal(g, r), name
    for name in ('hhat', 'd_eg'):
        g, r = getattr(got, name)[pair], getattr(ref, name)[pair]
        assert not torch.isnan(g.float()).any() and torch.equal(g, r), name
    g, r = got.d_qkv[real], ref.d_qkv[real]
    assert not torch.isnan(g.float()).any() and torch.equal(g, r), 'd_qkv'


def check_zero_padding(got, pair, real):
    for name in ('vatt', 'lse', 'gsum', 'd_qkv'):
        assert (getattr(got, name)[~real] == 0).all(), name
    for name in ('hhat', 'd_eg'):
        assert (getattr(got, name)[~pair] == 0).all(), name


@pytest.mark.parametrize('variant', ['prefix', 'dropped'])
@pytest.mark.parametrize('dtype', [BF16, F16], ids=_id)
@pytest.mark.parametrize('case', HONOUR + [CLAMP], ids=_id)
def test_honouring_families_real_block_exact_padding_zero_and_never_used(case, dtype, variant):
    """(1) the real block equals the call without counts, (2) the padding is exact zeros, (3) the same with NaN at every padded
    position of the inputs and cotangents, (5) two calls give equal bits"""
    shape, fwd, bwd = case
    qkv, eg, d_v, d_h, mask, pair, real = device_inputs(shape, dtype, variant)
    counts = torch.tensor(shape[2], dtype=torch.int32, device='cuda')          # (unclamped: the kernels clamp)
    d_v0, d_h0 = zero_padding(d_v, d_h, pair, real)
    ref = Call(shape, qkv, eg, mask, d_v0, d_h0)
    assert_families(ref, fwd, bwd)
    got = Call(shape, qkv, eg, mask, d_v, d_h, counts)                           # random finite cotangents on the padding
    assert_families(got, fwd, bwd)
    check_real_block(got, ref, pair, real)
    check_zero_padding(got, pair, real)
    again = Call(shape, qkv, eg, mask, d_v, d_h, counts)
    for name in ('vatt', 'hhat', 'lse', 'gsum', 'd_qkv', 'd_eg'):
        assert torch.equal(getattr(again, name), getattr(got, name)), name
    # the padding is never used: NaN in the Q/K/V rows of padded nodes, E|G of padded pairs, d_vatt / d_hhat on the padding
    nan = float('nan')
    qkv_p = torch.where(real[..., None], qkv, torch.full_like(qkv, nan))
    eg_p = torch.where(pair[..., None], eg, torch.full_like(eg, nan))
    d_vp = torch.where(real[..., None], d_v, torch.full_like(d_v, nan))
    d_hp = torch.where(pair[..., None], d_h, torch.full_like(d_h, nan))
    poisoned = Call(shape, qkv_p, eg_p, mask, d_vp, d_hp, counts)
    check_real_block(poisoned, ref, pair, real)
    check_zero_padding(poisoned, pair, real)


@pytest.mark.parametrize('dtype', [BF16, F16], ids=_id)
@pytest.mark.parametrize('case', [HONOUR[0], HONOUR[2]], ids=_id)
def test_backward_does_not_need_a_forward_that_honoured_the_count(case, dtype):
    """the backward with counts behind a forward WITHOUT: the same real block, zeros on the padding of the gradients"""
    shape, fwd, bwd = case
    qkv, eg, d_v, d_h, mask, pair, real = device_inputs(shape, dtype, 'prefix')
    counts = torch.tensor(shape[2], dtype=torch.int32, device='cuda')
    d_v0, d_h0 = zero_padding(d_v, d_h, pair, real)
    ref = Call(shape, qkv, eg, mask, d_v0, d_h0)
    got = Call(shape, qkv, eg, mask, d_v, d_h, counts, fwd_counts=False)
    assert torch.equal(got.d_qkv[real], ref.d_qkv[real]) and torch.equal(got.d_eg[pair], ref.d_eg[pair])
    assert (got.d_qkv[~real] == 0).all() and (got.d_eg[~pair] == 0).all()


@pytest.mark.parametrize('dtype', [BF16, F16], ids=_id)
@pytest.mark.parametrize('case', [HONOUR[0], HONOUR[3]], ids=_id)
def test_hhat_scale_keeps_its_meaning(case, dtype):
    """one factor of 0: the dropped graph's H_hat is all zeros, the other graphs are bit-equal to a call without the factor"""
    shape, fwd, bwd = case
    B = shape[0]
    qkv, eg, d_v, d_h, mask, pair, real = device_inputs(shape, dtype, 'prefix')
    counts = torch.tensor(shape[2], dtype=torch.int32, device='cuda')
    hs = torch.ones(B, dtype=F32, device='cuda')
    hs[1] = 0.0
    plain = Call(shape, qkv, eg, mask, d_v, d_h, counts)
    scaled = Call(shape, qkv, eg, mask, d_v, d_h, counts, hhat_scale=hs)
    assert (scaled.hhat[1] == 0).all()
    keep = [b for b in range(B) if b != 1]
    for name in ('vatt', 'hhat', 'lse', 'gsum', 'd_qkv', 'd_eg'):
        assert torch.equal(getattr(scaled, name)[keep], getattr(plain, name)[keep]), name
    # the dropped graph: only d_hhat's way into dE goes (its factor is 0); everything else is what it was
    assert torch.equal(scaled.vatt[1], plain.vatt[1]) and torch.equal(scaled.d_eg[1][..., shape[3]:], plain.d_eg[1][..., shape[3]:])
    check_zero_padding(scaled, pair, real)


@pytest.mark.parametrize('case', IGNORE, ids=lambda c: '-'.join(map(str, c[0][:2])) + '-' + c[3])
def test_families_that_ignore_the_count_give_the_bits_of_the_call_without(case):
    """KB_BWD (65..128 nodes) and the lane-per-head kernels: whole tensors, the same (random everywhere) cotangents both ways"""
    shape, dtype, fwd, bwd = case
    qkv, eg, d_v, d_h, mask, pair, real = device_inputs(shape, dtype, 'prefix')
    counts = torch.tensor(shape[2], dtype=torch.int32, device='cuda')
    ref = Call(shape, qkv, eg, mask, d_v, d_h)
    assert_families(ref, fwd, bwd)
    got = Call(shape, qkv, eg, mask, d_v, d_h, counts, fwd_counts=(fwd != 'KB_FWD'))
    assert_families(got, fwd, bwd)
    for name in ('vatt', 'hhat', 'lse', 'gsum', 'd_qkv', 'd_eg'):
        assert torch.equal(getattr(got, name), getattr(ref, name)), name


def test_logits_only_calls_ignore_the_count():
    from tgt_amd import ops
    B, N, W, H = 2, 12, 32, 4
    qkv, eg, _, d_h, _ = nfc.inputs((B, N, W, H), BF16, 'plain')
    qk, eb, d_h = qkv[..., :2 * W].contiguous().cuda(), eg[..., :H].contiguous().cuda(), d_h.cuda()
    counts = torch.tensor([12, 5], dtype=torch.int32, device='cuda')
    out = []
    for nc in (None, counts):
        a, _ = ops._node_args(qk, eb, None, H, False, True)
        hhat, d_qk, d_e = torch.full((B, N, N, H), float('nan'), dtype=BF16, device='cuda'), torch.full_like(qk, float('nan')), torch.full_like(eb, float('nan'))
        a.hhat, a.d_hhat, a.d_qkv, a.d_eg = hhat.data_ptr(), d_h.data_ptr(), d_qk.data_ptr(), d_e.data_ptr()
        assert nfc.family(qk, eb, None, H, 0, logits_only=True) == nfc.family_id('LANE')
        if nc is None:
            ops._launch('tgt_node_attention_fwd', C.byref(a))
            ops._launch('tgt_node_attention_bwd', C.byref(a))
        else:
            ops._launch('tgt_node_attention_fwd_counts', C.byref(a), ops._ptr(nc))
            ops._launch('tgt_node_attention_bwd_counts', C.byref(a), ops._ptr(nc))
        torch.cuda.synchronize()
        out.append((hhat, d_qk, d_e))
    assert all(torch.equal(x, y) and not torch.isnan(x.float()).any() for x, y in zip(*out))


def test_autograd_surface_saves_the_counts_for_the_backward():
    """ops.node_attention(node_counts=): the same bits as the raw entry points, both directions, and a wrong count vector is refused"""
    from tgt_amd import ops
    shape, fwd, bwd = HONOUR[0]
    qkv, eg, d_v, d_h, mask, pair, real = device_inputs(shape, BF16, 'prefix')
    counts = torch.tensor(shape[2], dtype=torch.int32, device='cuda')
    raw = Call(shape, qkv, eg, mask, d_v, d_h, counts)
    qx, ex = qkv.clone().requires_grad_(True), eg.clone().requires_grad_(True)
    v, hh = ops.node_attention(qx, ex, mask, shape[3], True, True, node_counts=counts)
    torch.autograd.backward([v, hh], [d_v, d_h])
    torch.cuda.synchronize()
    assert torch.equal(v, raw.vatt) and torch.equal(hh, raw.hhat)
    assert torch.equal(qx.grad, raw.d_qkv) and torch.equal(ex.grad, raw.d_eg)
    with pytest.raises(RuntimeError, match='node_counts'):
        ops.node_attention(qkv, eg, mask, shape[3], node_counts=counts.long())
    with pytest.raises(RuntimeError, match='node_counts'):
        ops.node_attention(qkv, eg, mask, shape[3], node_counts=counts[:2])


@functools.lru_cache(maxsize=None)
def oracle(case, dtype):
    B, N, counts, H, D = case
    qkv, eg, d_v, d_h, mask, pair, real = host_inputs(case, dtype, 'prefix')
    d_v0, d_h0 = zero_padding(d_v, d_h, pair, real)
    q64, e64 = qkv.double().requires_grad_(True), eg.double().requires_grad_(True)
    v, h = core.egt_attention_core(q64, e64, mask.double().unsqueeze(-1), H, True)
    ((v * d_v0.double()).sum() + (h * d_h0.double()).sum()).backward()
    return v.detach(), h.detach(), q64.grad, e64.grad


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize('dtype', [BF16, F16], ids=_id)
@pytest.mark.parametrize('case', [HONOUR[0], HONOUR[2]], ids=_id)
def test_oracle_parity_on_the_real_block(case, dtype):
    """KB_FWD + MFMA32 backward, KB_FWD + TILES16 backward with counts against the float64 oracle, the bars of
    tests/test_hip_node_families.py: rel-L2 8e-3 (bf16) / 1e-3 (fp16) on outputs, twice that on gradients"""
    shape, fwd, bwd = case
    qkv, eg, d_v, d_h, mask, pair, real = device_inputs(shape, dtype, 'prefix')
    counts = torch.tensor(shape[2], dtype=torch.int32, device='cuda')
    got = Call(shape, qkv, eg, mask, d_v, d_h, counts)
    assert_families(got, fwd, bwd)
    v, h, dq, de = oracle(shape, dtype)
    pc, rc = pair.cpu(), real.cpu()
    errs = dict(vatt=rel(got.vatt[real], v[rc]), hhat=rel(got.hhat[pair], h[pc]), dqkv=rel(got.d_qkv[real], dq[rc]),
                deg=rel(got.d_eg[pair], de[pc]))
    print(shape, dtype, errs)
    tol = TOL[dtype]
    assert errs['vatt'] < tol and errs['hhat'] < tol, errs
    assert errs['dqkv'] < 2 * tol and errs['deg'] < 2 * tol, errs
