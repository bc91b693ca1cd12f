"""oracle.modules.FFN with activation relu / silu / elu against the reference's own float64 outputs and gradients
(tests/golden/op_ffn_<kind>_small.npz, written by tools/make_golden.py `act`: the reference FFN on the inputs of op_ffn_geglu_small)."""
import pytest

import golden_util as gu
from oracle import modules as om
from test_oracle_golden import check, load

KINDS = ['relu', 'silu', 'elu']


def act_case_args(kind):
    """tools/make_golden.py act_case_args: geometry and seed of op_ffn_geglu_small, the activation swapped"""
    _, kwargs, geom = gu.OP_CASES['ffn_geglu_small']
    return dict(kwargs, activation=kind), geom, 100 + list(gu.OP_CASES).index('ffn_geglu_small')


@pytest.mark.parametrize('kind', KINDS)
def test_ffn_act_case_matches_reference(kind):
    kwargs, geom, seed = act_case_args(kind)
    res = gu.run_op_case(om.FFN, kwargs, geom, seed=seed)
    gold = load(f'op_ffn_{kind}_small')
    assert set(res) == set(gold), (sorted(res), sorted(gold))
    for k, t in res.items():
        check(t, gold[k], 1e-11, f'ffn_{kind}_small:{k}')
    assert float(res['out_e'].detach().abs().max()) > 0 and 'pgrad.lin_W1.weight' in res


def test_the_three_goldens_differ():
    outs = [load(f'op_ffn_{kind}_small')['out_e']['full'] for kind in KINDS]
    assert all(abs(a - b).max() > 1e-3 for i, a in enumerate(outs) for b in outs[i + 1:])
