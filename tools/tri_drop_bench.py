"""A/B of triplet attention with attention dropout: forward + backward of ops.projected_triplet_attention in ONE process, the arms
alternating round by round.  At the headline shape (`--nodes` <= 32):

    new_p        this tree, dropout p: library GEMMs + tri_att_fwd_kernel, backward on tri_att_bwd2_kernel's dropout instantiation
    new_p_off    this tree with TGT_TRI_DROP_FAST=0 (the library asks per call): the backward on tri_att_bwd_kernel, as the parent has it
    new_0        this tree, p = 0: the projection-fused forward + tri_att_bwd2_kernel
    parent_p     a SECOND build of the library (`--parent-lib`, the parent commit built in another checkout), dropout p
    parent_0     the same, p = 0

At 33..64 nodes (`--nodes 48 --batch 128`) the switch of the arms is TGT_TRI_DROP16, which the library also asks per call:

    new_p        TGT_TRI_DROP16=1: library GEMMs + the DROP instantiations of tri_att16_fwd_kernel / tri_att16_bwd_kernel
    new_p_off    TGT_TRI_DROP16=0, the default: library GEMMs + the general 32-wide kernels, which is the parent's code
    new_0        p = 0: library GEMMs + the p = 0 kernels of the 16-wide tiles

The host code of the arms is this tree's: the parent's differs from it in the wording of a notice only, so `parent_*` swaps the
LIBRARY under it (loaded beside this tree's, RTLD_DEEPBIND).  Time: HIP events around `--iters` forward + backward pairs after
`--warmup`, `--rounds` rounds, median (min - max) per arm; the order of the arms rotates from round to round.  The run-to-run spread to
judge a difference by is that of one arm's own rounds.  A pass of its own takes the per-kernel times (ops.profile_kernels /
ops.kernel_times_ms, median per launch) and compares the results: new_p_off against parent_p and new_0 against parent_0 bit for
bit (same kernels), new_p against parent_p within the gradient bar of the tests.

    python tools/tri_drop_bench.py [--parent-lib PATH] [--batch 256] [--nodes 32] [--p 0.1] [--iters 10] [--warmup 3] [--rounds 7]
                                   [--dtype bf16|fp16] [--seed 0]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CW, H = 256, 16
SEED = 0x1234567890ABCDEF


def stats(xs):
    xs = sorted(xs)
    return {'median': round(xs[len(xs) // 2], 4), 'min': round(xs[0], 4), 'max': round(xs[-1], 4)}


def load_second(path):
    """a second build of the library beside the tree's: its own symbols first (RTLD_DEEPBIND), the binding's signatures for every
    symbol it has (an older build lacks the newest ones)"""
    from tgt_amd import _lib
    L = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
    for name, (res, args) in _lib.SYMBOLS.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    assert L.tgt_abi_version() == _lib.ABI_VERSION
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--nodes', type=int, default=32)
    ap.add_argument('--p', type=float, default=0.1)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp16'])
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    from tgt_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit('tri_drop_bench: needs the GPU (nothing is measured without one)')
    dt = torch.bfloat16 if a.dtype == 'bf16' else torch.float16
    B, N = a.batch, a.nodes
    new = _lib.lib()
    parent = load_second(a.parent_lib) if a.parent_lib else None
    L = ops.TripletLayout(CW, H, gated=True, biased=True)
    torch.manual_seed(a.seed)
    n_nodes = torch.randint(max(1, N // 2), N + 1, (B,))
    nm = torch.arange(N)[None, :] < n_nodes[:, None]
    mask3 = ((~(nm[:, :, None] & nm[:, None, :])).float() * torch.finfo(torch.float32).min).cuda().contiguous()
    x = torch.randn(B, N, N, CW, device='cuda', dtype=dt).requires_grad_(True)
    w = (torch.randn(L.width, CW, device='cuda') * CW ** -0.5).to(dt).requires_grad_(True)
    b = (torch.randn(L.width, device='cuda') * 0.1).to(dt).requires_grad_(True)
    d_out = torch.randn(B, N, N, 2 * CW, device='cuda', dtype=dt)

    def arm(lib, p, fast):
        def run():
            _lib._lib = lib
            os.environ['TGT_TRI_DROP_FAST'] = os.environ['TGT_TRI_DROP16'] = '1' if fast else '0'
            try:
                out = ops.projected_triplet_attention(x, w, b, mask3, L, dropout=(p, SEED if p else 0))
                grads = torch.autograd.grad(out, (x, w, b), d_out)
            finally:
                _lib._lib = new
                os.environ.pop('TGT_TRI_DROP_FAST', None)
                os.environ.pop('TGT_TRI_DROP16', None)
            return (out,) + grads
        return run

    arms = {'new_p': arm(new, a.p, True), 'new_p_off': arm(new, a.p, False), 'new_0': arm(new, 0.0, True)}
    if parent is not None:
        arms['parent_p'] = arm(parent, a.p, True)
        arms['parent_0'] = arm(parent, 0.0, True)
    names = list(arms)

    def timeit(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.iters

    import warnings
    warnings.simplefilter('ignore', RuntimeWarning)           # (the slow-path notice of the dropout forward)
    results, kernels = {}, {}
    for k in names:                                            # the checks' and the per-kernel pass
        arms[k]()
        prof = ops.profile_kernels(True)
        try:
            for _ in range(5):
                res = arms[k]()
            torch.cuda.synchronize()
        finally:
            ops.profile_kernels(False)
        results[k] = [t.detach().clone() for t in res]
        kernels[k] = {name: round(sorted(v)[len(v) // 2], 4) for name, v in ops.kernel_times_ms(prof).items() if name.startswith('tgt_triplet')}
        del res
    times = {k: [] for k in names}
    for r in range(a.rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            times[k].append(timeit(arms[k]))

    def same(p, q):
        return all(bool(torch.equal(s, t)) for s, t in zip(results[p], results[q]))

    def rel(p, q):
        return [round(float((s.double() - t.double()).norm() / (t.double().norm() + 1e-30)), 6) for s, t in zip(results[p], results[q])]

    checks = {'new_p_vs_new_p_off_rel': rel('new_p', 'new_p_off')}
    if parent is not None:
        checks.update({'new_p_off_equals_parent_p_bitwise': same('new_p_off', 'parent_p'), 'new_0_equals_parent_0_bitwise': same('new_0', 'parent_0'),
                       'new_p_vs_parent_p_rel': rel('new_p', 'parent_p')})
    fam = {}
    for k, on in (('new_p', '1'), ('new_p_off', '0')):         # which kernel family the attention core of the two dropout arms is
        os.environ['TGT_TRI_DROP_FAST'] = os.environ['TGT_TRI_DROP16'] = on
        fused = torch.empty(1, N, N, L.width, dtype=dt, device='cuda')
        out1 = torch.empty(1, N, N, 2 * CW, dtype=dt, device='cuda')
        cs = ops._colsum_workspace(1, L.width, L.used, fused.device)
        fam[k] = [new.tgt_triplet_attention_family(C.byref(ops._tri_args(fused, mask3[:1], out1, L, dropout=(a.p, SEED))), 0),
                  new.tgt_triplet_attention_family(C.byref(ops._tri_args(fused, mask3[:1], out1, L, out1, fused, cs, dropout=(a.p, SEED))), 1)]
        os.environ.pop('TGT_TRI_DROP_FAST', None)
        os.environ.pop('TGT_TRI_DROP16', None)
    print(json.dumps({'B': B, 'N': N, 'family_fwd_bwd': fam, 'C': CW, 'H': H, 'dtype': a.dtype, 'p': a.p, 'iters': a.iters, 'rounds': a.rounds,
                      'mean_nodes': round(float(n_nodes.double().mean()), 2), 'fwd_bwd_ms': {k: stats(v) for k, v in times.items()},
                      'rounds_ms': {k: [round(t, 4) for t in v] for k, v in times.items()}, 'kernel_ms': kernels, 'checks': checks}))
    bad = [k for k, v in checks.items() if k.endswith('bitwise') and not v]
    if bad:
        raise SystemExit('tri_drop_bench: ' + ', '.join(bad) + ' failed')


if __name__ == '__main__':
    main()
