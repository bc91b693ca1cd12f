"""A/B of the triplet aggregate forward kernels with and without the per-graph DropPath factor (tgt_triplet_aggregate_fwd_skip /
_proj_fwd_skip), in ONE process, the settings alternating round by round:

    no_factor    tgt_triplet_aggregate_fwd / _proj_fwd of this tree (the kernels' instantiations without the argument)
    all_kept     the _skip entry points, every factor non-zero (the instantiations with the argument, nothing to skip)
    dropped      the _skip entry points, every `--every`-th graph at factor 0 (10 % at the default)
    parent       tgt_triplet_aggregate_fwd / _proj_fwd of a SECOND build of the library (`--parent-lib`, e.g. of the parent commit
                 built in another checkout): loaded beside this tree's, same inputs, same process.  Several paths may be given
                 (parent, parent_2, ...): a byte-for-byte COPY of one build under another file name is loaded as a library of its
                 own, and the difference between the two copies is what code placement alone is worth

Kernels: tri_agg_fwd_kernel (fused V | E/G rows from memory) and tri_agg_proj_fwd_kernel (V projected in the kernel), called through
the C ABI on fixed random inputs; HIP events around `--iters` back-to-back launches, `--rounds` rounds, median (min - max) per
setting; every setting writes the SAME output buffer and the order of the settings rotates from round to round.  The run-to-run
spread to judge a difference by is that of the parent's own rounds.  The outputs of `parent` and `no_factor` are compared bit for
bit, and `dropped` is checked against `no_factor` (kept graphs equal, dropped graphs zeros), in a pass of their own.

    python tools/agg_skip_bench.py [--parent-lib PATH [PATH ...]] [--batch 256] [--nodes 32] [--every 10] [--iters 20] [--warmup 5]
                                   [--rounds 7] [--dtype bf16|fp16] [--seed 0]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CW, H = 256, 16         # what tri_agg_proj_fwd_kernel takes


def stats(xs):
    xs = sorted(xs)
    return {'median': round(xs[len(xs) // 2], 4), 'min': round(xs[0], 4), 'max': round(xs[-1], 4)}


def timeit(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def load_second(path):
    """a second build of the library beside the tree's: its own symbols first (RTLD_DEEPBIND), the binding's signatures"""
    from tgt_amd import _lib
    L = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
    for name in ('tgt_abi_version', 'tgt_last_error', 'tgt_triplet_aggregate_fwd', 'tgt_triplet_aggregate_proj_fwd'):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _lib.SYMBOLS[name]
    assert L.tgt_abi_version() == _lib.ABI_VERSION
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', nargs='*', default=[])
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--nodes', type=int, default=32)
    ap.add_argument('--every', type=int, default=10, help='graphs b with b %% every == every - 1 are dropped')
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp16'])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    from tgt_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit('agg_skip_bench: needs the GPU (nothing is measured without one)')
    dt = torch.bfloat16 if a.dtype == 'bf16' else torch.float16
    B, N = a.batch, a.nodes
    new = _lib.lib()
    libs = {'new': new}
    for i, path in enumerate(a.parent_lib):
        libs['parent' if i == 0 else f'parent_{i + 1}'] = load_second(path)
    L = ops.AggregateLayout(CW, H, gated=True)
    torch.manual_seed(a.seed)
    n_nodes = torch.randint(max(1, N // 2), N + 1, (B,))
    nm = torch.arange(N)[None, :] < n_nodes[:, None]
    mask3 = ((~(nm[:, :, None] & nm[:, None, :])).float() * torch.finfo(torch.float32).min).cuda().contiguous()
    x = torch.randn(B, N, N, CW, device='cuda', dtype=dt)
    w = (torch.randn(L.width, CW, device='cuda') * CW ** -0.5).to(dt)
    b = (torch.randn(L.width, device='cuda') * 0.1).to(dt)
    fused = torch.addmm(b, x.view(-1, CW), w.t()).view(B, N, N, L.width)
    eg = fused[..., 2 * CW:L.used].contiguous()
    kept = torch.full((B,), 1.0 / 0.9, dtype=torch.float32, device='cuda')
    dropped = kept.clone()
    dropped[a.every - 1::a.every] = 0
    dead = (dropped == 0).cpu()
    stream = ops._stream

    def plain(lib, out, gs=None):
        args = ops._agg_args(fused, mask3, out, L)
        if gs is None:
            return lambda: _lib.check(lib.tgt_triplet_aggregate_fwd(C.byref(args), stream()), 'fwd')
        return lambda: _lib.check(lib.tgt_triplet_aggregate_fwd_skip(C.byref(args), ops._ptr(gs), stream()), 'fwd_skip')

    def proj(lib, out, gs=None):
        args = ops._agg_proj_args(eg, mask3, out, L)
        px, pw, pb = ops._ptr(x), ops._ptr(w), ops._ptr(b)
        if gs is None:
            return lambda: _lib.check(lib.tgt_triplet_aggregate_proj_fwd(C.byref(args), px, CW, pw, pb, stream()), 'proj_fwd')
        return lambda: _lib.check(lib.tgt_triplet_aggregate_proj_fwd_skip(C.byref(args), ops._ptr(gs), px, CW, pw, pb, stream()), 'proj_fwd_skip')

    result = {'B': B, 'N': N, 'C': CW, 'H': H, 'dtype': a.dtype, 'dropped_graphs': int(dead.sum()), 'iters': a.iters, 'rounds': a.rounds,
              'mean_nodes': round(float(n_nodes.double().mean()), 2)}
    for kernel, make in (('tri_agg_fwd_kernel', plain), ('tri_agg_proj_fwd_kernel', proj)):
        out = torch.empty(B, N, N, 2 * CW, dtype=dt, device='cuda')
        settings = {'no_factor': make(new, out), 'all_kept': make(new, out, kept), 'dropped': make(new, out, dropped)}
        for k, lib in libs.items():
            if k != 'new':
                settings[k] = make(lib, out)
        names = list(settings)
        outs = {}
        for k in names:                                         # the checks' pass: one launch each, results kept
            out.fill_(float('nan'))
            settings[k]()
            torch.cuda.synchronize()
            outs[k] = out.clone()
        times = {k: [] for k in names}
        for r in range(a.rounds):
            for k in names[r % len(names):] + names[:r % len(names)]:
                times[k].append(timeit(settings[k], a.iters, a.warmup))
        torch.cuda.synchronize()
        ref = outs['no_factor']
        checks = {'all_kept_equals_no_factor': bool(torch.equal(outs['all_kept'], ref)),
                  'dropped_kept_graphs_equal': bool(torch.equal(outs['dropped'][~dead], ref[~dead])),
                  'dropped_graphs_zero': bool((outs['dropped'][dead] == 0).all())}
        for k in names:
            if k.startswith('parent'):
                checks[k + '_equals_no_factor_bitwise'] = bool(torch.equal(outs[k].view(torch.int16), ref.view(torch.int16)))
        result[kernel] = {'ms': {k: stats(v) for k, v in times.items()}, 'rounds_ms': {k: [round(t, 4) for t in v] for k, v in times.items()},
                          'checks': checks}
        del outs, out
    print(json.dumps(result))
    if not all(v for k in ('tri_agg_fwd_kernel', 'tri_agg_proj_fwd_kernel') for v in result[k]['checks'].values()):
        raise SystemExit('agg_skip_bench: an output check failed')


if __name__ == '__main__':
    main()
