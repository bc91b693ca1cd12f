"""`python bench.py --gpus 2 --share-device`: the multi-rank branch of bench.py end to end on ONE GPU.
RCCL with more than one rank has never run on the boxes this repo is built on (1 GPU each); the first 8-GPU contact is the
driver's.  This walks everything of that branch that does not need a second device: self-launch of the ranks
(reference lib/training/execute.py:91-107), rendezvous on 127.0.0.1, rank-0 parameter broadcast, bucketed gradient exchange from
the autograd hooks, the settle-step count that must not depend on a rank's own allocator, per-rank NUMA binding, per-rank
TunableOp files, the all_gather of the timings, and the JSON line of rank 0."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *args], capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]               # rank 0 only
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize('launcher', ['self', 'torchrun', 'self_sharded'])
def test_bench_two_ranks_share_one_gpu(launcher):
    common = ['--gpus', '2', '--share-device', '--batch', '16', '--steps', '3', '--warmup', '1', '--settle-steps', '3',
              '--full', '--roofline-steps', '1', '--no-cpu-baseline']
    if launcher == 'self_sharded':                          # the sharded-optimizer exchange (StepConfig.shard_optimizer) through the same branch
        out = _bench(common + ['--grad-exchange', 'reduce_scatter_sharded'])
        assert out['grad_exchange']['optimizer_sharded'] is True and out['grad_exchange']['mode'] == 'reduce_scatter'
    elif launcher == 'self':
        out = _bench(common)
    else:
        # the driver's form: python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py ...
        import socket
        with socket.socket() as s:
            s.bind(('127.0.0.1', 0))
            port = s.getsockname()[1]
        env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
        env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr',
                            '127.0.0.1', '--master-port', str(port), os.path.join(ROOT, 'bench.py'), *common],
                           capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
        assert len(lines) == 1, r.stdout[-2000:]
        out = json.loads(lines[0])
    assert out['world'] == 2 and out['n_gpus'] == 2 and out['rccl_ranks'] == 0            # gloo: a rehearsal, and the line says so
    assert 'REHEARSAL' in out['config']['parallelism'] and out['config']['global_batch'] == 32
    assert len(out['ms_per_step_by_rank']) == 2 and all(v > 0 for v in out['ms_per_step_by_rank'])
    assert len(out['comm_exposed_ms_by_rank']) == 2
    assert out['grad_exchange']['buckets'] >= 2 and sorted(out['grad_exchange']['launch_order_last_step']) == \
        list(range(out['grad_exchange']['buckets']))[:16] or out['grad_exchange']['buckets'] > 16
    assert out['allocator_settle_steps'] == 3              # every rank ran the same count (it drives collectives)
    assert out['value'] > 0 and abs(out['value'] - 32 * 3 / (out['ms_per_step'] * 3e-3)) < 1e-3 * out['value'] + 1
    assert out['roofline'] is not None and out['final_loss'] == out['final_loss']        # a number, not NaN


@pytest.mark.gpu
def test_plain_run_dumps_its_last_step(tmp_path):
    """`bench.py --gpus 1` without --full: --steps timed steps, ms_per_step, no roofline / CPU baseline; --dump-outputs writes the
    last timed step's arrays as float32 / float64 .npy files (64 MB at most), and they do not depend on how many allocator settle
    steps ran before the warm-up (the state before them is restored)"""
    import numpy as np
    common = ['--gpus', '1', '--batch', '16', '--steps', '3', '--warmup', '1', '--no-gemm-tuning']     # (16 x 32 x 32 x 512 logits: sampled)
    dumps = []
    for k, settle in enumerate(('4', '2')):
        d = tmp_path / str(k)
        out = _bench(common + ['--settle-steps', settle, '--dump-outputs', str(d)], timeout=600)
        assert out['steps'] == 3 and out['allocator_settle_steps'] == int(settle)
        assert out['ms_per_step'] > 0 and abs(out['value'] - 16 * 3 / (out['ms_per_step'] * 3e-3)) < 1e-3 * out['value'] + 1
        assert out['roofline'] is None and 'cpu_baseline' not in out
        files = sorted(os.listdir(d))
        assert files == ['dist_logits_sample.npy', 'gap.npy', 'loss.npy', 'params_sample.npy'], files
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        dumps.append({f: np.load(d / f) for f in files})
    assert dumps[0]['gap.npy'].shape == (16,) and dumps[0]['loss.npy'].shape == ()
    for f, a in dumps[0].items():
        b = dumps[1][f]
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape and np.isfinite(a).all(), f
        # the step is not bitwise reproducible (bf16 outputs move by a few units in the last place between runs); another
        # dropout / DropPath stream or another parameter state moves most elements by far more than this
        diff = np.abs(b.astype(np.float64) - a)
        assert diff.max() <= 0.1 * np.abs(a).max() + 1e-6 and diff.mean() <= 2e-2 * np.abs(a).mean() + 1e-6, \
            (f, float(diff.max()), float(diff.mean()))
