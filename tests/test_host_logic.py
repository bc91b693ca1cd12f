"""Host-side logic that needs no GPU: the row tables that assemble the kernel-order projections from
the reference's separate nn.Linear parameters, and the numpy restatement of the kernels'
attention-dropout generator."""
import numpy as np
import pytest
import torch

import golden_util as gu


def test_triplet_attention_param_table_matches_reference_channel_order():
    from tgt_amd import layout
    from tgt_amd.tgt.layers.triplet import TripletAttention, TripletAttentionUngated, AxialAttention
    C, H = 64, 8
    D = C // H
    for cls, nb in ((TripletAttention, 2 * H), (TripletAttentionUngated, H), (AxialAttention, 0)):
        mod = cls(C, H)
        t, L = mod._table, mod._layout
        src, idx = t.row_src.tolist(), t.row_idx.tolist()
        assert len(src) == L.width and t.n_cols == C
        for dir_ in (0, 1):
            for part, off in enumerate((L.q[dir_], L.k[dir_], L.v[dir_])):
                for h in range(H):
                    for d in range(D):
                        r = off + h * D + d                       # kernel row: head-major
                        assert src[r] == dir_                      # lin_QKV_in / lin_QKV_out
                        assert idx[r] == part * C + d * H + h      # reference channel: head-minor (triplet.py:213-215)
        if nb:
            for dir_ in (0, 1):
                for j in range(nb):
                    r = 6 * C + dir_ * nb + j
                    assert src[r] == 2 + dir_ and idx[r] == j
        assert all(s == -1 for s in src[L.used:])
        # the permutation really is one: every reference row of the QKV weights is used exactly once
        assert sorted(i for s_, i in zip(src, idx) if s_ == 0) == list(range(3 * C))
        assert torch.equal(torch.tensor(idx[:3 * C]), layout.qkv_rows_head_major(C, H).to(torch.int64))


def test_triplet_aggregate_param_table():
    from tgt_amd.tgt.layers.triplet import TripletAggregate, TripletAggregateUngated
    C, H = 32, 4
    D = C // H
    for cls, nb in ((TripletAggregate, 4 * H), (TripletAggregateUngated, 2 * H)):
        mod = cls(C, H)
        src, idx = mod._table.row_src.tolist(), mod._table.row_idx.tolist()
        for dir_ in (0, 1):
            for h in range(H):
                for d in range(D):
                    r = dir_ * C + h * D + d
                    assert src[r] == 0 and idx[r] == dir_ * C + d * H + h
        assert src[2 * C:2 * C + nb] == [1] * nb and idx[2 * C:2 * C + nb] == list(range(nb))


def test_dropout_generator_restatement_is_deterministic_and_calibrated():
    units = np.arange(40)
    keep, scale = gu.triplet_dropout_keep(0xDEADBEEF12345678, 0.2, units, 32)
    keep2, _ = gu.triplet_dropout_keep(0xDEADBEEF12345678, 0.2, units, 32)
    other, _ = gu.triplet_dropout_keep(0xDEADBEEF12345679, 0.2, units, 32)
    assert keep.shape == (40, 32, 32) and keep.dtype == bool
    assert (keep == keep2).all() and (keep != other).any()
    assert abs(keep.mean() - 0.8) < 0.01 and abs(scale - 1.25) < 1e-6
    # neighbouring keys share one hash word but not their decision
    assert (keep[:, :, 0::2] != keep[:, :, 1::2]).mean() > 0.2


def test_knobs_are_read_once_in_one_place(monkeypatch):
    """tgt_amd/knobs.py: every host-side A/B switch in one record; flags that default on go off with "0", flags that default off go
    on with "1", and non_default() names exactly what differs (bench.py prints it)"""
    from tgt_amd import knobs
    for var, *_ in knobs._SPEC.values():
        monkeypatch.delenv(var, raising=False)
    for var in knobs.ENV_OF_LIBRARY:
        monkeypatch.delenv(var, raising=False)
    base = knobs.Knobs.from_env()
    assert base.non_default() == {}
    assert base.tri_proj and base.node_stream and not base.defer_sums and base.side_prio == -1 and base.tri_skip == 1
    monkeypatch.setenv('TGT_TRI_PROJ', '0')
    monkeypatch.setenv('TGT_DEFER_SUMS', '1')
    monkeypatch.setenv('TGT_WGRAD_STREAM', '0')          # a default-off flag set to its default: not reported
    monkeypatch.setenv('TGT_TRI_SKIP', '2')
    monkeypatch.setenv('TGT_TRI_BWD2_DMA', '0')          # read by the library, listed in the report
    k = knobs.Knobs.from_env()
    assert k.non_default() == {'TGT_TRI_PROJ': False, 'TGT_DEFER_SUMS': True, 'TGT_TRI_SKIP': 2, 'TGT_TRI_BWD2_DMA': '0'}
    import dataclasses
    with pytest.raises(dataclasses.FrozenInstanceError):
        k.tri_proj = True


def test_no_environment_switch_outside_knobs():
    """every host-side switch is a field of knobs.K (so that bench.py's knobs_not_default names it); the
    work-skipping timing probes are not in the product at all (tools/probes/skip_probes.py, bench.py --timing-probe)"""
    import os
    import re
    import tgt_amd
    root = os.path.dirname(tgt_amd.__file__)
    allowed = {'knobs.py': None, '_lib.py': ('TGT_HIP_LIB', 'HIPCC', 'TGT_KEEP_ISA'), 'torch_ops.py': ('CXX',),
               os.path.join('training', 'gemm_tuning.py'): ('TGT_TUNING_FILE',)}
    for d, _, files in os.walk(root):
        for f in files:
            if not f.endswith('.py'):
                continue
            rel = os.path.relpath(os.path.join(d, f), root)
            src = open(os.path.join(d, f)).read()
            assert 'PROBE_SKIP' not in src, rel
            names = re.findall(r"os\.environ(?:\.get)?[\[(]\s*'([A-Z_0-9]+)'", src)
            if rel in allowed:
                assert allowed[rel] is None or set(names) <= set(allowed[rel]), (rel, names)
            else:
                assert not [n for n in names if n.startswith('TGT_')], (rel, names)
    from tgt_amd import knobs
    assert knobs._SPEC['wgrad_maxp'][0] == 'TGT_WGRAD_MAXP' and knobs._SPEC['embed_gemm'][0] == 'TGT_EMBED_GEMM'


def test_parameter_reuse_is_found_in_the_graph():
    """the forked parameter-gradient stream / deferred closing sums are only safe when every parameter that one of the
    package's own autograd Functions differentiates enters the graph once; the Trainer looks for reuse of ANY kind in the graph
    of its first step (not only layer_multiplier > 1)"""
    import torch
    from tgt_amd.training.step import _parameter_reused

    class Lin(torch.autograd.Function):                 # stands for the package's Functions (a Python-defined node)
        @staticmethod
        def forward(ctx, x, w):
            ctx.save_for_backward(x, w)
            return x @ w.t()

        @staticmethod
        def backward(ctx, dy):
            x, w = ctx.saved_tensors
            return dy @ w, dy.t() @ x

    lin, other = torch.nn.Linear(4, 4), torch.nn.Linear(4, 4)
    params = list(lin.parameters()) + list(other.parameters())
    x = torch.randn(3, 4)
    assert not _parameter_reused(Lin.apply(Lin.apply(x, lin.weight), other.weight).sum(), params)
    assert _parameter_reused(Lin.apply(Lin.apply(x, lin.weight), lin.weight).sum(), params)     # a module applied twice
    assert _parameter_reused((Lin.apply(x, lin.weight) @ lin.weight).sum(), params)             # a tied weight, one own edge
    assert not _parameter_reused(lin(lin(x)).sum(), params)            # library nodes only: autograd orders those itself
    assert not _parameter_reused(x.sum().requires_grad_(), params)     # no graph at all


def test_numa_affinity_helper_parses_and_declines_gracefully():
    """bench.py binds a rank to the CPUs of its GPU's NUMA node (tgt_amd/training/affinity.py); without the topology it must
    leave the process alone and say why"""
    import os
    from tgt_amd.training import affinity
    assert affinity._cpulist('0-3,8,10-11\n') == {0, 1, 2, 3, 8, 10, 11}
    assert affinity._cpulist('') == set()
    assert affinity.bind_to_gpu_numa(0, enabled=False) == {'bound': False, 'why': 'disabled'}
    before = os.sched_getaffinity(0)
    real = affinity.gpu_numa_node
    try:
        affinity.gpu_numa_node = lambda i: None              # a container that hides the PCI topology
        rep = affinity.bind_to_gpu_numa(0)
        assert rep['bound'] is False and 'NUMA' in rep['why']
        affinity.gpu_numa_node = lambda i: 10 ** 6           # a node without a cpulist
        rep = affinity.bind_to_gpu_numa(0)
        assert rep['bound'] is False
    finally:
        affinity.gpu_numa_node = real
    assert os.sched_getaffinity(0) == before


def test_graph_safe_host_seeds_are_a_function_of_the_call_position():
    """training/graphed.py: a captured step bakes its host-drawn dropout seeds into the graph, so in graph-safe mode they are a fixed
    function of the call's position inside the step (the step enters through the device counter instead): every step draws the
    same sequence, every call of a step another seed; outside the mode seeds come from torch's CPU generator again"""
    import torch
    from tgt_amd import ops
    try:
        ops.graph_safe_rng(True)
        ops.begin_step()
        a = [ops.draw_dropout(0.1, True)[1] for _ in range(50)]
        ops.begin_step()
        b = [ops.draw_dropout(0.1, True)[1] for _ in range(50)]
        assert a == b and len(set(a)) == 50 and all(0 <= s < 2 ** 63 for s in a)
        assert ops.draw_dropout(0.1, False) == (0.0, 0)            # not training: no dropout, no position consumed
        assert ops.draw_dropout(0.0, True) == (0.0, 0)
        ops.begin_step()
        assert ops.draw_dropout(0.1, True)[1] == a[0]
    finally:
        ops.graph_safe_rng(False)
    torch.manual_seed(5)
    c = ops.draw_dropout(0.1, True)[1]
    torch.manual_seed(5)
    assert ops.draw_dropout(0.1, True)[1] == c and c not in a


def test_flat_gradient_destination_refuses_a_second_gradient_for_one_parameter():
    """inside one Trainer backward a parameter's slice of the flat gradient buffer is handed out ONCE; a graph
    that starts re-using a parameter after the first step (which is the only one the Trainer walks) is an error, not a silent
    double write"""
    import pytest
    import torch
    from tgt_amd import ops
    v = torch.zeros(4, 3)
    ops.register_flat_grads([v], [v])
    try:
        assert ops._grad_dst(v.data_ptr(), (4, 3), torch.float32) is None          # outside a Trainer backward: ordinary tensors
        with ops.trainer_backward():
            a = ops._grad_dst(v.data_ptr(), (4, 3), torch.float32)
            assert a is not None and a.data_ptr() == v.data_ptr()
            with pytest.raises(RuntimeError, match='second weight gradient'):
                ops._grad_dst(v.data_ptr(), (4, 3), torch.float32)
        with ops.trainer_backward():                                                # the next backward starts clean
            assert ops._grad_dst(v.data_ptr(), (4, 3), torch.float32) is not None
    finally:
        ops.unregister_flat_grads([v.data_ptr()])


def test_affinity_binds_every_thread_of_the_process():
    """sched_setaffinity(0, ..) binds the calling thread only; torch's thread pools exist before bench.py binds"""
    import os
    import threading
    import pytest
    from tgt_amd.training import affinity
    if not hasattr(os, 'sched_setaffinity'):
        pytest.skip('no sched_setaffinity')
    before = os.sched_getaffinity(0)
    if len(before) < 2:
        pytest.skip('one CPU')
    stop = threading.Event()
    seen = {}

    def worker():
        stop.wait()
        seen['mask'] = os.sched_getaffinity(0)
    t = threading.Thread(target=worker)
    t.start()
    target = set(sorted(before)[:1])
    try:
        done, total = affinity._bind_all_threads(target)
        assert done >= 2 and total >= 2
        stop.set()
        t.join()
        assert seen['mask'] == target and os.sched_getaffinity(0) == target
    finally:
        stop.set()
        affinity.restore_affinity(before)
    assert os.sched_getaffinity(0) == before


def test_slow_kernel_family_is_announced_once():
    """a BASELINE-sized call that falls off the hot kernels says so, once per reason"""
    import warnings
    from tgt_amd import ops
    ops._slow_path_said.discard(('x', 'y'))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        ops._slow_path_notice(('x', 'y'), 'first')
        ops._slow_path_notice(('x', 'y'), 'second')
    assert len(w) == 1 and 'first' in str(w[0].message) and issubclass(w[0].category, RuntimeWarning)


# ---- ops._launch, the one way a kernel is enqueued, and the skip record of the triplet ops.  As in the binding tests nothing is
# launched and no pointer is dereferenced: the argument blocks are refused, or done (an empty batch), before memory is touched
def _aggregate_block(B=2, N=20):
    from tgt_amd import _lib
    a = _lib.TripletAggregateArgs()
    a.B, a.N, a.H, a.D, a.dtype, a.flags = B, N, 16, 16, _lib.TGT_BF16, _lib.TRI_BIASED | _lib.TRI_GATED
    return a


def test_launcher_labels_an_error_with_the_entry_it_called(monkeypatch):
    import ctypes as C
    from tgt_amd import ops
    monkeypatch.setattr(ops, '_stream', lambda: None)
    a = _aggregate_block(N=-1)
    for entry in ('tgt_triplet_aggregate_fwd', 'tgt_triplet_aggregate_bwd'):
        with pytest.raises(RuntimeError, match=entry + r' failed \(code 1\).*bad sizes'):
            ops._launch(entry, C.byref(a), prof='tgt_triplet_aggregate_fwd')
    with pytest.raises(RuntimeError, match=r'tgt_triplet_aggregate_fwd_skip failed \(code 1\).*bad sizes'):
        ops._launch('tgt_triplet_aggregate_fwd_skip', C.byref(a), None, prof='tgt_triplet_aggregate_fwd')
    assert ops._launch('tgt_triplet_aggregate_fwd', C.byref(_aggregate_block(B=0))) is None      # an empty batch: done, cleanly
    with pytest.raises(AttributeError):
        ops._launch('tgt_no_such_entry')


def test_launcher_samples_counts_and_records_under_the_one_name_it_is_given(monkeypatch):
    import ctypes as C
    from tgt_amd import ops
    recorded = []

    class FakeEvent:
        def __init__(self, enable_timing=False):
            assert enable_timing

        def record(self):
            recorded.append(self)
    monkeypatch.setattr(torch.cuda, 'Event', FakeEvent)
    monkeypatch.setattr(ops, '_stream', lambda: None)
    empty = _aggregate_block(B=0)

    def launch(prof):
        ops._launch('tgt_triplet_aggregate_fwd', C.byref(empty), prof=prof)
    try:
        prof = ops.profile_kernels(True, only={'tgt_layer_norm_bwd'}, stride=2)
        for name in ['tgt_layer_norm_bwd', 'tgt_colsum', None] * 3 + ['tgt_layer_norm_bwd'] * 2:
            launch(name)
        assert list(prof) == ['tgt_layer_norm_bwd'] and len(prof['tgt_layer_norm_bwd']) == 3         # launches 0, 2 and 4 of five
        assert all(isinstance(ev, FakeEvent) for pair in prof['tgt_layer_norm_bwd'] for ev in pair) and len(recorded) == 6
        assert ops.profile_launch_counts() == {'tgt_layer_norm_bwd': 5}                               # (no None key, no other name)
        # every name, one launch in two: counted and sampled per name; prof=None stays out of both
        prof = ops.profile_kernels(True, stride=2)
        for name in ('tgt_colsum', None, 'tgt_colsum', 'tgt_colsum', 'tgt_layer_norm_fwd', None):
            launch(name)
        assert {k: len(v) for k, v in prof.items()} == {'tgt_colsum': 2, 'tgt_layer_norm_fwd': 1}
        assert ops.profile_launch_counts() == {'tgt_colsum': 3, 'tgt_layer_norm_fwd': 1}
        # stride 1: everything named is recorded, nothing is counted
        prof = ops.profile_kernels(True)
        for name in ('tgt_colsum', None, 'tgt_colsum'):
            launch(name)
        assert {k: len(v) for k, v in prof.items()} == {'tgt_colsum': 2} and ops.profile_launch_counts() == {}
    finally:
        ops.profile_kernels(False)
    n = len(recorded)
    launch('tgt_colsum')
    assert len(recorded) == n and ops._PROFILE is None


class _PerGraph:
    """stands in for a per-graph device tensor: only what the check asks"""

    def __init__(self, dtype, n, contiguous=True, is_cuda=True):
        self.dtype, self.n, self.contiguous, self.is_cuda = dtype, n, contiguous, is_cuda

    def numel(self):
        return self.n

    def is_contiguous(self):
        return self.contiguous


def test_per_graph_vectors_of_the_triplet_ops_are_checked_in_one_place():
    from tgt_amd import ops
    B = 3
    counts, scale = _PerGraph(torch.int32, B), _PerGraph(torch.float32, B)
    assert ops._check_per_graph(None, B, torch.int32, 'x') is None and ops._check_per_graph(counts, B, torch.int32, 'x') is counts
    bad_counts = [_PerGraph(torch.int64, B), _PerGraph(torch.int32, B + 1), _PerGraph(torch.int32, B, contiguous=False),
                  _PerGraph(torch.int32, B, is_cuda=False), torch.zeros(B, dtype=torch.int32)]
    bad_scale = [_PerGraph(torch.float16, B), _PerGraph(torch.float32, B - 1), _PerGraph(torch.float32, B, contiguous=False),
                 _PerGraph(torch.float32, B, is_cuda=False), torch.ones(B)]
    for t in bad_counts:
        with pytest.raises(RuntimeError) as err:
            ops._TriSkip.of('triplet attention', B, 20, node_counts=t)
        assert str(err.value) == 'triplet attention: node_counts must be a contiguous int32 device tensor with one value per graph'
        if t.numel() == B:                  # (edge_live_tiles takes the batch size FROM the counts)
            with pytest.raises(RuntimeError, match='triplet attention: node_counts must be a contiguous int32 device tensor'):
                ops.edge_live_tiles(t, 20)
    for op in ('triplet attention', 'triplet aggregate'):
        for t in bad_scale:
            with pytest.raises(RuntimeError) as err:
                ops._TriSkip.of(op, B, 20, graph_scale=t)
            assert str(err.value) == op + ': graph_scale must be a contiguous float32 device tensor with one value per graph'
    assert ops._TriSkip.of('triplet attention', B, 20, counts, scale) == (counts, False, scale)


def test_skip_record_decides_what_a_triplet_backward_skips(monkeypatch):
    from tgt_amd import ops
    B = 3
    counts, scale = _PerGraph(torch.int32, B), _PerGraph(torch.float32, B)
    # counts_kb: N > 64, counts given, the switch on -- all three
    for ragged_kb in (False, True):
        monkeypatch.setattr(ops, '_TRI_RAGGED_KB', ragged_kb)
        for N in (64, 65, 128):
            for nc in (None, counts):
                skip = ops._TriSkip.of('triplet attention', B, N, nc, scale)
                assert skip.counts_kb is (ragged_kb and N > 64 and nc is not None), (ragged_kb, N, nc)
                assert skip.node_counts is nc and skip.graph_scale is scale
    # the backward's factors: with TGT_TRI_SKIP=2, or behind a projection-fused forward; its counts and flag: always the forward's
    skip = ops._TriSkip.of('triplet attention', B, 72, counts, scale)
    assert skip.counts_kb
    for skip_bwd in (False, True):
        monkeypatch.setattr(ops, '_TRI_SKIP_BWD', skip_bwd)
        for fused in (False, True):
            bwd = skip.for_backward(projection_fused=fused)
            assert bwd.graph_scale is (scale if (skip_bwd or fused) else None), (skip_bwd, fused)
            assert bwd.node_counts is counts and bwd.counts_kb is True
        assert skip.for_backward().graph_scale is (scale if skip_bwd else None)
        assert ops._TriSkip.of('triplet aggregate', B, 20).for_backward(True) == (None, False, None)
    # decided once: what the forward stored does not move with the switches
    monkeypatch.setattr(ops, '_TRI_SKIP_BWD', False)
    monkeypatch.setattr(ops, '_TRI_RAGGED_KB', False)
    assert bwd.graph_scale is scale and bwd.counts_kb is True
    with pytest.raises(AttributeError):
        skip.graph_scale = None
    assert not hasattr(skip, '__dict__')


def test_compute_dtype_keeps_both_spellings_of_its_call_sites(monkeypatch):
    from tgt_amd import ops
    x = torch.zeros(2, dtype=torch.float32)                    # a CPU tensor: where the two spellings differ
    assert ops._compute_dtype(x) is torch.float32 and ops._compute_dtype(x, on_cpu=True) is torch.float32
    assert ops._compute_dtype(x, otherwise=torch.float64) is torch.float64
    # CUDA autocast on (torch switches it off by itself where there is no GPU: its state is stood in for)
    monkeypatch.setattr(torch, 'is_autocast_enabled', lambda device: device == 'cuda')
    monkeypatch.setattr(torch, 'get_autocast_dtype', lambda device: torch.bfloat16)
    assert ops._compute_dtype(x) is torch.float32
    assert ops._compute_dtype(x, otherwise=torch.float64) is torch.float64
    assert ops._compute_dtype(x, on_cpu=True) is torch.bfloat16
    assert ops._compute_dtype(_PerGraph(torch.float32, 2)) is torch.bfloat16
    assert ops._compute_dtype(_PerGraph(torch.float32, 2), otherwise=torch.float64) is torch.bfloat16
    monkeypatch.undo()
    p = torch.zeros(2, requires_grad=True)
    assert ops._no_backward(x, None) and not ops._no_backward(x, None, p)
    with torch.no_grad():
        assert ops._no_backward(x, p)


def test_timing_probes_accept_every_parameter_of_what_they_replace(monkeypatch):
    """tools/probes/skip_probes.py replaces functions of tgt_amd.ops that the autograd Functions call with keywords: a replacement
    that lacks a parameter of the real function (as _ln_backward's lacked `live`) raises TypeError on the first backward of
    bench.py --timing-probe.  Every replacement takes every parameter of the function it replaces, under the same name."""
    import importlib.util
    import inspect
    import os
    from tgt_amd import ops
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'probes', 'skip_probes.py')
    spec = importlib.util.spec_from_file_location('skip_probes', path)
    skip_probes = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(skip_probes)
    replaced = {'skip_sums': 'sum_planes', 'skip_proj_ln': '_ln_backward', 'skip_wgrad': '_wgrad_into'}
    assert set(replaced) == set(skip_probes.PROBES)
    for probe, name in replaced.items():
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, real)                # (registers the real function for restoration: install() overwrites it)
        monkeypatch.setattr(ops, 'torch', ops.torch)        # (skip_wgrad also wraps the module's view of torch)
        skip_probes.install(probe)
        probe_fn = getattr(ops, name)
        assert probe_fn is not real, (probe, name)
        have = inspect.signature(probe_fn).parameters
        for pname, par in inspect.signature(real).parameters.items():
            assert pname in have and have[pname].kind == par.kind, (probe, name, pname)
        monkeypatch.undo()
        assert getattr(ops, name) is real and ops.torch is torch
