"""Which launches offer themselves to ops.profile_kernels(True), and under which names: one training step each of the tiny
two-layer TGT-At of tests/test_hip_triplet_kb_ragged.py at N = 72 (library GEMMs + the key-blocked triplet kernels; fp32 and
bf16 autocast) and at N = 12 with every row-count threshold lowered to 1 (the row kernels, the split projection and the
projection-fused triplet forward; bf16 autocast).  The number of event pairs per name is compared with
tests/golden/profile_names.json.

The fixture is a RECORDING of the commit before the launches moved onto ops._launch (it pins the names the --profile-all
tables under profiles/ were made with); it is not regenerated from the code under test.  It was written by

    python tests/test_hip_profile_names.py tests/golden/profile_names.json

on an MI355X at that commit."""
import json
import os
import sys

import pytest
import torch

if __name__ == '__main__':
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]

import golden_util as gu

pytestmark = pytest.mark.gpu

CFG = dict(gu.MODEL_CASES['multi_at_tiny'][1], model_height=2, node_width=64, edge_width=256, num_heads=4, triplet_heads=16)
# name -> (batch geometry, bf16 autocast, row thresholds lowered)
STEPS = {
    'n72_fp32': (dict(B=3, N=72, num_nodes=[72, 40, 9]), False, False),
    'n72_bf16': (dict(B=3, N=72, num_nodes=[72, 40, 9]), True, False),
    'n12_bf16_row_kernels': (dict(B=2, N=12, num_nodes=[12, 9]), True, True),
}
FIXTURE = os.path.join(gu.GOLDEN_DIR, 'profile_names.json')


def record(name):
    """{kernel name: event pairs} of one forward + loss + backward under profile_kernels(True)"""
    from tgt_amd import ops
    from tgt_amd.pcqm import TGT_Multi
    from tgt_amd.training.step import pretrain_loss, StepConfig
    geom, autocast, lowered = STEPS[name]
    saved = ops._EDGE_MIN_ROWS, ops._SPLIT_MIN_ROWS
    if lowered:
        ops._EDGE_MIN_ROWS = ops._SPLIT_MIN_ROWS = 1
    try:
        model = gu.fill_params(TGT_Multi(**CFG), seed=31).cuda().train()
        batch = {k: v.cuda() for k, v in gu.model_batch(geom, seed=32).items()}
        cfg = StepConfig(num_dist_bins=CFG['num_dist_bins'], mixed_precision=None)
        prof = ops.profile_kernels(True)
        try:
            with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
                loss = pretrain_loss(model(batch), batch, cfg)
            loss.backward()
            torch.cuda.synchronize()
        finally:
            ops.profile_kernels(False)
        assert torch.isfinite(loss)
        assert ops.profile_launch_counts() == {}            # (stride 1: nothing is counted)
        return {k: len(v) for k, v in sorted(prof.items())}
    finally:
        ops._EDGE_MIN_ROWS, ops._SPLIT_MIN_ROWS = saved


@pytest.mark.parametrize('name', list(STEPS))
def test_timed_launches_and_their_names_are_those_of_the_recording(name):
    with open(FIXTURE) as fh:
        want = json.load(fh)[name]
    got = record(name)
    print(name, got)
    assert got == want, {k: (got.get(k), want.get(k)) for k in sorted(set(got) | set(want)) if got.get(k) != want.get(k)}


if __name__ == '__main__':
    out = {name: record(name) for name in STEPS}
    # the routes the recording is there for did run: the key-blocked triplet kernels, the row kernels, the projection-fused forward
    for name in ('n72_fp32', 'n72_bf16'):
        assert out[name]['tgt_triplet_attention_fwd'] == out[name]['tgt_triplet_attention_bwd'] == CFG['model_height']
    rows = out['n12_bf16_row_kernels']
    assert rows['tgt_triplet_attention_proj_fwd'] == CFG['model_height'] and rows['tgt_edge_linear'] > 0
    with open(sys.argv[1], 'w') as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(out, sort_keys=True))
