"""Host-side checks of the MC-dropout graph replay (no device): the Python restatement of the kernels' step_seed, the keyword
surface of the graphed classes and predict functions, and the header the kernels' contract is written in."""
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = 0x9E3779B97F4A7C15


def test_step_seed_wraps_like_the_kernels_uint64_arithmetic():
    """csrc/common.hpp: seed + *ctr * 0x9E3779B97F4A7C15 in uint64_t; the values below were computed by hand (hex long addition)"""
    from tgt_amd.ops import step_seed
    assert step_seed(0, 0) == 0
    assert step_seed(0x243F6A8885A308D3, 0) == 0x243F6A8885A308D3                  # c = 0: the seed as given
    assert step_seed(0, 1) == GOLDEN
    assert step_seed(5, 2) == 0x3C6EF372FE94F82F                                    # 2 * golden = 0x1_3C6EF372FE94F82A: wraps once
    assert step_seed(0xFFFFFFFFFFFFFFF0, 1) == 0x9E3779B97F4A7C05                   # a seed near 2^64: the sum wraps
    assert step_seed(0x243F6A8885A308D3, 3) == 0xFEE5D7B503827D12                   # the kernel tests' case: lands above 2^63
    assert step_seed(0x8000000000000001, 2 ** 64 - 1) == 0xE1C8864680B583EC        # counter = -1 as uint64: seed - golden
    for seed, c in ((0, 0), (1, 7), (2 ** 64 - 1, 2 ** 63), (0x0123456789ABCDEF, 123456789)):
        v = step_seed(seed, c)
        assert 0 <= v < 2 ** 64 and v == (seed + c * GOLDEN) % 2 ** 64


def test_host_seeds_fit_the_unsigned_argument():
    """the argument blocks take the seed through c_uint64 after `& (2^64 - 1)`: a stepped seed above 2^63 survives"""
    from tgt_amd import _lib
    for cls in (_lib.TripletAttentionArgs, _lib.TripletAggregateArgs):
        a = cls()
        a.dropout_seed = 0xFEE5D7B503827D12
        assert a.dropout_seed == 0xFEE5D7B503827D12


def test_keyword_surface():
    from tgt_amd.pcqm import graphed, predict
    from tgt_amd.training import graphed as tgraphed

    def default(fn, name):
        return inspect.signature(fn).parameters[name].default

    assert default(graphed.GraphedForward.__init__, 'stochastic') is False
    assert default(graphed.GraphedForward.__init__, 'allow_frozen_dropout') is False
    assert default(graphed.GraphedForward.__init__, 'counter') is None
    for name in ('load', 'sample', 'close', '__call__', '__enter__', '__exit__'):
        assert callable(getattr(graphed.GraphedForward, name))
    assert issubclass(graphed.GraphedSampler, graphed.GraphedForward)
    assert list(inspect.signature(graphed.GraphedSampler.__init__).parameters)[1:5] == ['model', 'example_batch', 'nb_samples', 'kind']
    assert default(tgraphed.GraphedTrainingStep.__init__, 'attention_dropout') is False      # the default stays the refusal
    assert default(tgraphed.GraphedStepCache.__init__, 'attention_dropout') is False
    for fn in (predict.predict_bins, predict.predict_probs, predict.gap_prediction_step, predict.prediction_step4eval,
               predict.prediction_step4savebins, predict.two_stage_predict):
        assert default(fn, 'graphed') is None, fn.__name__                                    # opt-in


def test_header_still_parses_and_the_abi_version_is_unchanged(tmp_path):
    from tgt_amd import _lib
    src = tmp_path / 't.c'
    src.write_text('#include "tgt_hip.h"\nint main(void) { return (int)sizeof(tgt_triplet_aggregate_args) == 0; }\n')
    subprocess.check_call(['gcc', '-fsyntax-only', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src)])
    assert _lib.ABI_VERSION == 32
    capi = open(os.path.join(ROOT, 'tgt_amd', 'csrc', 'capi.hip')).read()
    assert re.search(r'int tgt_abi_version\(void\)\s*\{\s*return 32;\s*\}', capi)
    text = open(os.path.join(ROOT, 'include', 'tgt_hip.h')).read()
    assert 'int tgt_set_seed_counter(const void* device_counter);' in text
