"""CPU-side checks of tests/node_family_cases.py: every case takes the kernel family it declares (tgt_node_attention_family() is host
logic on sizes, dtype, offsets, pointer nullness and alignment), and the table, together with the six hard-input cases the suite
already had, keeps a plain and a hard-input case on every family and direction the library routes to.  A change to an eligibility
rule that empties a family's coverage fails here, on a machine without a GPU."""
import pytest
import torch

import node_family_cases as nfc

ALL = nfc.CASES + nfc.EXISTING_HARD


def _ids(cases):
    return ['-'.join(map(str, c.shape)) + '-' + str(dt).replace('torch.', '') for c in cases for dt in c.dtypes]


@pytest.mark.parametrize('case,dtype', [(c, dt) for c in ALL for dt in c.dtypes], ids=_ids(ALL))
def test_declared_family(case, dtype):
    got = (nfc.shape_family(case.shape, dtype, 0), nfc.shape_family(case.shape, dtype, 1))
    assert got == (nfc.family_id(case.fwd), nfc.family_id(case.bwd)), (case, got)


def test_fake_addresses_route_like_tensors():
    """shape_family() describes the call that family() reads off real tensors"""
    for shape, dtype in [((2, 20, 192, 16), torch.bfloat16), ((2, 33, 128, 16), torch.float16), ((1, 7, 20, 5), torch.float32)]:
        qkv, eg, _, _, mask = nfc.inputs(shape, dtype, 'plain')
        for bwd in (0, 1):
            assert nfc.family(qkv, eg, mask, shape[3], bwd) == nfc.shape_family(shape, dtype, bwd)
    qk, eb = torch.zeros(1, 5, 128, dtype=torch.bfloat16), torch.zeros(1, 5, 5, 2, dtype=torch.bfloat16)
    for bwd in (0, 1):
        assert nfc.family(qk, eb, None, 2, bwd, logits_only=True) == nfc.shape_family((1, 5, 64, 2), torch.bfloat16, bwd, logits_only=True)


def test_table_is_keyed_by_shape_and_dtype():
    assert len(nfc.FAMILIES) == sum(len(c.dtypes) for c in nfc.CASES)                  # no (shape, dtype) declared twice
    assert nfc.FAMILIES[(1, 130, 256, 32, torch.bfloat16)] == ('KB_FWD', 'LANE')
    assert all(set(c.kinds) <= {'hard', 'plain'} and c.kinds for c in ALL)


def test_every_family_and_direction_has_a_plain_and_a_hard_case():
    seen = set()
    for c in ALL:
        for dt in c.dtypes:
            for bwd in (0, 1):
                fam = nfc.shape_family(c.shape, dt, bwd)                               # what the library says, not what the table says
                seen.update((fam, bwd, kind) for kind in c.kinds)
    missing = [(name, bwd, kind) for name, bwd in nfc.ROUTES for kind in ('plain', 'hard') if (nfc.family_id(name), bwd, kind) not in seen]
    assert not missing, missing


def test_routes_are_all_the_library_has():
    from tgt_amd import _lib
    names = {n[len('NODE_FAMILY_'):] for n in dir(_lib) if n.startswith('NODE_FAMILY_')} - {'NONE'}
    assert names == {name for name, _ in nfc.ROUTES}
    # the two one-directional families never take the other direction
    for c in ALL:
        for dt in c.dtypes:
            assert nfc.shape_family(c.shape, dt, 1) != _lib.NODE_FAMILY_KB_FWD and nfc.shape_family(c.shape, dt, 0) != _lib.NODE_FAMILY_KB_BWD


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('shape', nfc.LOGITS_CASES)
def test_logits_only_is_lane_per_head(shape, dtype):
    lane = nfc.family_id('LANE')
    assert nfc.shape_family(shape, dtype, 0, logits_only=True) == lane and nfc.shape_family(shape, dtype, 1, logits_only=True) == lane


@pytest.mark.parametrize('shape', sorted({c.shape for c in nfc.CASES if 'hard' in c.kinds}))
def test_hard_inputs_are_hard(shape):
    B, N, W, H = shape
    qkv, eg, d_v, d_h, m = nfc.inputs(shape, torch.float32, 'hard')
    dead = torch.isinf(m)
    assert set(m.unique().tolist()) == {0.0, -float('inf')}
    assert not dead[:, :, N - 1].any()                                                 # every query keeps a live key
    assert not torch.equal(dead, dead.transpose(1, 2))                                 # per (query, key), not symmetric
    lead = 16 if N > 16 else N // 2
    assert dead[:, 1::3, :lead].all() and (N <= 32 or dead[:, 2::5, :32].all())         # whole leading key blocks
    assert not dead[:, 0::3, :lead].all()                                              # ... for some queries only
    e = eg[..., :H]
    assert e.std() > 6 and e[:, :, N // 2:].mean() - e[:, :, :N // 2].mean() > 8       # spread logits, the maximum in the later keys
    assert torch.equal(qkv, nfc.inputs(shape, torch.float32, 'hard')[0])               # the same in every process
