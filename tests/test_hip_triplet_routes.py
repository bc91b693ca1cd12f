"""Which libtgt_hip entry points ops.projected_triplet_attention / projected_triplet_aggregate launch, in order, forward and backward,
for every route of their host code: the N <= 32 and 33..64 projection-fused forwards with and without a backward, their node-count
and DropPath forms, and every way off them (dropout, N > 64, fp32, D != 16, the knob).  ops._launch is wrapped by a recorder that
calls through; only the tgt_triplet_* names are compared.  B = 2, C = 256, bf16, _SPLIT_MIN_ROWS = 1 unless the case says otherwise."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

ATT, AGG = 'tgt_triplet_attention', 'tgt_triplet_aggregate'
KNOBS_ON = ('_TRI_PROJ', '_TRI_PROJ_INFER', '_TRI_PROJ64_INFER', '_TRI_SPLIT', '_TRI_COLSUM', '_AGG_PROJ_INFER', '_AGG_PROJ64_INFER')


@pytest.fixture
def launches(monkeypatch):
    from tgt_amd import ops
    names, real = [], ops._launch

    def recorder(entry, *args, **kw):
        names.append(entry)
        return real(entry, *args, **kw)
    monkeypatch.setattr(ops, '_launch', recorder)
    monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 1)
    for name in KNOBS_ON:
        monkeypatch.setattr(ops, name, True)
    monkeypatch.setattr(ops, '_TRI_PROJ64_TRAIN', False)            # (its default: opt-in)
    monkeypatch.setattr(ops, '_TRI_SKIP_BWD', False)
    monkeypatch.setattr(ops, '_slow_path_said', set())              # (these shapes count as BASELINE-sized here: notices fire, and stay ours)
    return lambda: [n for n in names if n.startswith('tgt_triplet_')]


def _run(kind, N, grad, H=16, dtype=torch.bfloat16, p=0.0, counts=False, scale=False, B=2):
    """one forward (+ backward) of the module's attend() on random input"""
    from tgt_amd.tgt.layers import triplet
    cls = triplet.TripletAttention if kind == 'attention' else triplet.TripletAggregate
    g = torch.Generator(device='cuda').manual_seed(N)
    mod = cls(256, H, attention_dropout=p).cuda().to(dtype).train()
    x = (torch.randn(B, N, N, 256, device='cuda', generator=g) * 0.5).to(dtype).requires_grad_(grad)
    mask = torch.zeros(B, N, N, 1, device='cuda')
    extra = {}
    if counts:
        extra['node_counts'] = torch.tensor([N, max(1, N - 3)], dtype=torch.int32, device='cuda')
        mask[1, :, N - 3:] = torch.finfo(torch.float32).min
    if scale:
        extra['graph_scale'] = torch.tensor([0.0, 2.0], device='cuda')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)             # (the slow-path notices)
        with torch.enable_grad() if grad else torch.no_grad():
            out = mod.attend(x, mask, **extra)
        if grad:
            out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    assert out.shape == (B, N, N, 512) and bool(torch.isfinite(out.float()).all())
    return out


ATTENTION = [
    # id, arguments of _run, knobs patched, expected suffixes of tgt_triplet_attention
    ('n32_grad', dict(N=32, grad=True), {}, ['_proj_fwd', '_bwd']),
    ('n32_no_grad', dict(N=32, grad=False), {}, ['_proj_fwd']),
    ('n32_dropout_grad', dict(N=32, grad=True, p=0.1), {}, ['_fwd', '_bwd']),
    ('n33_no_grad', dict(N=33, grad=False), {}, ['_proj64_fwd']),
    ('n64_no_grad', dict(N=64, grad=False), {}, ['_proj64_fwd']),
    ('n48_grad', dict(N=48, grad=True), {}, ['_fwd', '_bwd']),
    ('n48_grad_train64', dict(N=48, grad=True), {'_TRI_PROJ64_TRAIN': True}, ['_proj64_train_fwd', '_bwd']),
    ('n65_no_grad', dict(N=65, grad=False), {}, ['_fwd']),
    ('fp32_n32', dict(N=32, grad=False, dtype=torch.float32), {}, ['_fwd']),
    ('h8', dict(N=32, grad=False, H=8), {}, ['_fwd']),
    ('proj_off_n32', dict(N=32, grad=False), {'_TRI_PROJ': False}, ['_fwd']),
    ('proj_off_n48', dict(N=48, grad=False), {'_TRI_PROJ': False}, ['_fwd']),
    # every fused case again with node counts
    ('n32_grad_counts', dict(N=32, grad=True, counts=True), {}, ['_proj_fwd_counts', '_bwd_counts']),
    ('n32_no_grad_counts', dict(N=32, grad=False, counts=True), {}, ['_proj_fwd_counts']),
    ('n33_no_grad_counts', dict(N=33, grad=False, counts=True), {}, ['_proj64_fwd_counts']),
    ('n64_no_grad_counts', dict(N=64, grad=False, counts=True), {}, ['_proj64_fwd_counts']),
    ('n48_grad_train64_counts', dict(N=48, grad=True, counts=True), {'_TRI_PROJ64_TRAIN': True}, ['_proj64_train_fwd_counts', '_bwd_counts']),
]


@pytest.mark.parametrize('kwargs,knobs,want', [c[1:] for c in ATTENTION], ids=[c[0] for c in ATTENTION])
def test_attention_launches(launches, monkeypatch, kwargs, knobs, want):
    from tgt_amd import ops
    for name, value in knobs.items():
        monkeypatch.setattr(ops, name, value)
    _run('attention', **kwargs)
    assert launches() == [ATT + s for s in want]


AGGREGATE = [
    ('n32_no_grad', dict(N=32, grad=False), ['_proj_fwd']),
    ('n32_no_grad_graph_scale', dict(N=32, grad=False, scale=True), ['_proj_fwd_skip']),
    ('n48_no_grad', dict(N=48, grad=False), ['_proj64_fwd']),
    ('n32_grad', dict(N=32, grad=True), ['_fwd', '_bwd']),
    ('n48_grad', dict(N=48, grad=True), ['_fwd', '_bwd']),
    ('n65_no_grad', dict(N=65, grad=False), ['_fwd']),
]


@pytest.mark.parametrize('kwargs,want', [c[1:] for c in AGGREGATE], ids=[c[0] for c in AGGREGATE])
def test_aggregate_launches(launches, kwargs, want):
    _run('aggregate', **kwargs)
    assert launches() == [AGG + s for s in want]
