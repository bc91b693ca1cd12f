"""ops._tri_forward_route against the routing of _ProjectedTripletAttention.forward as it stood before the route became one function,
written out here as tables (CPU only: the function reads x.numel(), the layout, the dtypes and the module-level knobs)."""
import itertools

import pytest
import torch

from tgt_amd import ops

BF16, F16, FP32 = torch.bfloat16, torch.float16, torch.float32
ANY = object()


class OnDevice:                                                 # (stands in for a CUDA tensor: is_cuda and numel are all that is read)
    is_cuda = True

    def __init__(self, rows):
        self.n = rows * 256

    def numel(self):
        return self.n


def _layouts():
    padded = ops.TripletLayout(256, 16)                         # (no H with D = 16 pads the row by itself: a stand-in that differs in this alone)
    padded.width = padded.used + 8
    return {'gated16': ops.TripletLayout(256, 16), 'axial': ops.TripletLayout(256, 16, gated=False, biased=False),
            'h8': ops.TripletLayout(256, 8), 'padded': padded}


# which layouts and dtypes the two fused kernels' shape terms admit (the old _proj_fused_ok / _proj64_fused_ok less N, knob and rows)
FUSABLE = {(lay, cd): lay in ('gated16', 'axial') and cd is not FP32
           for lay in ('gated16', 'axial', 'h8', 'padded') for cd in (BF16, F16, FP32)}
assert sum(FUSABLE.values()) == 4
# biased, unpadded, E/G row a multiple of 8 columns: two GEMMs instead of one once there are enough rows
SPLITTABLE = {'gated16': True, 'axial': False, 'h8': True, 'padded': False}

# the forward's branches, first match wins:
# (N range, fusable, p, no_backward, _TRI_PROJ, _TRI_PROJ_INFER, _TRI_PROJ64_INFER, _TRI_PROJ64_TRAIN) with enough rows
#    -> (kind, entry, stores_qkv)
FUSED_ROUTES = [
    (('<=32', True, 0.0, True, True, True, ANY, ANY), ('proj', 'tgt_triplet_attention_proj_fwd', False)),
    (('<=32', True, 0.0, ANY, True, ANY, ANY, ANY), ('proj', 'tgt_triplet_attention_proj_fwd', True)),
    (('33..64', True, 0.0, True, True, ANY, True, ANY), ('proj64', 'tgt_triplet_attention_proj64_fwd', False)),
    (('33..64', True, 0.0, False, True, ANY, ANY, True), ('proj64_train', 'tgt_triplet_attention_proj64_train_fwd', True)),
]
NRANGE = {8: '<=32', 32: '<=32', 33: '33..64', 64: '33..64', 65: '>64'}

# the word of the notice for a call that is off the fused forward, for N <= 32 and p = 0 (N and p come first: below)
WHY_SHAPE = {('gated16', FP32): 'fp32', ('axial', FP32): 'fp32',
             ('h8', BF16): 'head dim != 16', ('h8', F16): 'head dim != 16', ('h8', FP32): 'head dim != 16',
             ('padded', BF16): 'padded / unbiased layout', ('padded', F16): 'padded / unbiased layout', ('padded', FP32): 'fp32'}


def _expected(N, lay, cd, p, no_backward, enough_rows, proj, proj_infer, p64_infer, p64_train):
    if enough_rows:
        have = (NRANGE[N], FUSABLE[lay, cd], p, no_backward, proj, proj_infer, p64_infer, p64_train)
        for want, route in FUSED_ROUTES:
            if all(w is ANY or w == h for w, h in zip(want, have)):
                return route + (None,)
    kind = 'split' if (SPLITTABLE[lay] and enough_rows) else 'gemm'
    why = None
    if enough_rows and proj:
        why = 'N > 64' if N == 65 else 'N > 32' if N in (33, 64) else 'attention dropout > 0' if p else WHY_SHAPE[lay, cd]
    return (kind, 'tgt_triplet_attention_fwd', False, why)


@pytest.mark.parametrize('knobs', list(itertools.product((True, False), repeat=4)),
                         ids=lambda k: ''.join('01'[v] for v in k))
def test_route_table(monkeypatch, knobs):
    proj, proj_infer, p64_infer, p64_train = knobs
    monkeypatch.setattr(ops, '_TRI_PROJ', proj)
    monkeypatch.setattr(ops, '_TRI_PROJ_INFER', proj_infer)
    monkeypatch.setattr(ops, '_TRI_PROJ64_INFER', p64_infer)
    monkeypatch.setattr(ops, '_TRI_PROJ64_TRAIN', p64_train)
    monkeypatch.setattr(ops, '_TRI_SPLIT', True)
    layouts, seen = _layouts(), set()
    for N, lay, cd, p, no_backward, enough in itertools.product((8, 32, 33, 64, 65), layouts, (BF16, F16, FP32), (0.0, 0.1),
                                                                (True, False), (False, True)):
        x = OnDevice(ops._SPLIT_MIN_ROWS - (0 if enough else 1))
        got = ops._tri_forward_route(x, N, layouts[lay], cd, p, no_backward)
        want = _expected(N, lay, cd, p, no_backward, enough, *knobs)
        assert tuple(got) == want, (N, lay, cd, p, no_backward, enough, knobs)
        assert got.projection_fused is (want[0] in ('proj', 'proj64', 'proj64_train'))
        seen.add(want[0])
    assert seen >= {'split', 'gemm'} and (not proj or 'proj' in seen)


def test_every_kind_and_every_word_is_reached_at_the_default_knobs_or_one_step_from_them(monkeypatch):
    for name in ('_TRI_PROJ', '_TRI_PROJ_INFER', '_TRI_PROJ64_INFER', '_TRI_PROJ64_TRAIN', '_TRI_SPLIT'):
        monkeypatch.setattr(ops, name, True)
    L, x = _layouts(), OnDevice(ops._SPLIT_MIN_ROWS)
    kinds = {ops._tri_forward_route(x, N, L['gated16'], BF16, 0.0, nb).kind for N in (32, 48) for nb in (True, False)}
    assert kinds == {'proj', 'proj64', 'proj64_train'}
    words = {ops._tri_forward_route(x, N, L[lay], cd, p, False).why
             for N in (32, 48, 65) for lay in L for cd in (BF16, FP32) for p in (0.0, 0.1)}
    assert words == {None, 'N > 64', 'N > 32', 'attention dropout > 0', 'head dim != 16', 'fp32', 'padded / unbiased layout'}


def test_the_split_knob_and_the_row_threshold_are_read_per_call(monkeypatch):
    L, x = _layouts()['gated16'], OnDevice(4096)
    monkeypatch.setattr(ops, '_TRI_PROJ', False)
    assert ops._tri_forward_route(x, 32, L, BF16, 0.0, False) == ('gemm', 'tgt_triplet_attention_fwd', False, None)
    monkeypatch.setattr(ops, '_SPLIT_MIN_ROWS', 4096)
    assert ops._tri_forward_route(x, 32, L, BF16, 0.0, False).kind == 'split'
    monkeypatch.setattr(ops, '_TRI_SPLIT', False)
    assert ops._tri_forward_route(x, 32, L, BF16, 0.0, False).kind == 'gemm'
    monkeypatch.setattr(ops, '_TRI_PROJ', True)
    assert ops._tri_forward_route(x, 32, L, BF16, 0.0, False) == ('proj', 'tgt_triplet_attention_proj_fwd', True, None)


def test_notice_keys_and_texts(monkeypatch):
    """the keys put into _slow_path_said and the texts, from the route's word: what users and tests grep"""
    said = []
    monkeypatch.setattr(ops, '_slow_path_notice', lambda key, msg, stacklevel=3: said.append((key, msg)))
    R = ops._TriRoute
    ops._tri_route_notice(R('gemm', 'tgt_triplet_attention_fwd', False, None), 48, 0.0)
    assert said == []
    ops._tri_route_notice(R('split', 'tgt_triplet_attention_fwd', False, 'N > 64'), 65, 0.0)
    assert said[-1][0] == ('tri_proj', 'N > 64') and 'key-blocked attention kernels (65 <= N <= 128' in said[-1][1]
    ops._tri_route_notice(R('split', 'tgt_triplet_attention_fwd', False, 'N > 32'), 48, 0.0)
    assert said[-1][0] == ('tri_proj', 'N > 32')
    assert said[-1][1] == ('triplet attention: the projection-fused forward / round-4 backward do not take this shape (N > 32); running the '
                           'projection as library GEMMs + the general attention kernels (N in 33..64: 16-wide tiles at 0.39-0.45 of HBM '
                           'instead of 0.52; see DESIGN.md section 4)')
    for on in (True, False):
        monkeypatch.setattr(ops._knobs, 'library_flag_now', lambda name, on=on: {'tri_drop16': on}[name])
        ops._tri_route_notice(R('split', 'tgt_triplet_attention_fwd', False, 'N > 32'), 48, 0.1)
        assert said[-1][0] == ('tri_proj', 'N > 32', 'dropout', on) and 'see DESIGN.md 4.zj' in said[-1][1]
        assert ('TGT_TRI_DROP16=1; each direction' in said[-1][1]) is on
    for fast in (True, False):
        monkeypatch.setattr(ops, '_TRI_DROP_FAST', fast)
        ops._tri_route_notice(R('split', 'tgt_triplet_attention_fwd', False, 'attention dropout > 0'), 32, 0.1)
        assert said[-1][0] == ('tri_proj', 'attention dropout > 0')
        assert ('the backward stays on the round-4 kernel: DESIGN.md 4.zi' in said[-1][1]) is fast
