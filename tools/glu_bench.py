#!/usr/bin/env python
"""A/B of FFN.hidden with a gated activation on the edge rows (M = B*N*N rows, 256 -> 512 -> 256 channels, 16-bit autocast,
activation dropout and a per-graph DropPath factor), HIP events on the launch stream, the two sides ALTERNATED:
  (a) the composition this path ran before the GLU kernels: library GEMM, chunk, F.gelu / sigmoid / silu, multiply, nn.Dropout,
      multiply by the per-graph factor (autograd keeps every intermediate);
  (b) FFN.hidden: one tgt_edge_linear launch (TGT_EPI_GLU) forward; tgt_glu_dropout_bwd + the Linear's gradients backward.
Then the streaming kernels tgt_glu_dropout_fwd / _bwd next to tgt_gelu_dropout_* at the same OUTPUT element count, in algorithmic
GB/s (forward: x in + y out; backward: x and dy in, dx out).  Prints a table; --out FILE also writes it."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tgt_amd import ops  # noqa: E402
from tgt_amd.tgt.layers.blocks import FFN  # noqa: E402


def timeit(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def composition(ffn, x, sample_scale):
    """FFN.hidden as it ran for the GLU names before the kernels (blocks.py, last branch)"""
    y = ffn.dropout(ffn.ffn_fn(ffn.lin_W1(x)))
    return y * sample_scale.view([-1] + [1] * (y.ndim - 1)).to(y.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=256)
    ap.add_argument('--N', type=int, default=32)
    ap.add_argument('--p', type=float, default=0.1)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--activation', default='geglu')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    dt = {'bf16': torch.bfloat16, 'fp16': torch.float16}[a.dtype]
    B, N, C = a.B, a.N, 256
    M = B * N * N
    torch.manual_seed(0)
    lines = [f'FFN.hidden A/B, activation={a.activation}, M = {M} rows, C = {C}, {a.dtype} autocast, p = {a.p}, per-graph scale; '
             f'{a.rounds} alternating rounds x {a.iters} iterations, ms per call (HIP events)']
    ffn = FFN(C, 1., act_dropout=a.p, activation=a.activation).cuda().train()
    x = torch.randn(B, N, N, C, device='cuda', dtype=dt).requires_grad_(True)
    scale = (torch.rand(B, device='cuda') > 0.2).float() / 0.8
    dy = torch.randn(B, N, N, C, device='cuda', dtype=dt)
    with torch.autocast('cuda', dtype=dt):
        assert ops.linear_glu_dropout_ok(x, ffn.lin_W1.weight, scale), 'the fused launch does not take this shape'
        sides = {'a_composition': lambda: composition(ffn, x, scale), 'b_kernels': lambda: ffn.hidden(x, scale)}

        def fwd_bwd(f):
            y = f()
            torch.autograd.grad(y, [x, ffn.lin_W1.weight, ffn.lin_W1.bias], dy)
        for f in sides.values():                             # warm-up: code objects, GEMM plans, allocator
            for _ in range(3):
                fwd_bwd(f)
        torch.cuda.synchronize()
        res = {k: dict(fwd=[], fwd_bwd=[]) for k in sides}
        for _ in range(a.rounds):
            for k, f in sides.items():
                with torch.no_grad():
                    res[k]['fwd'].append(timeit(f, a.iters))
                res[k]['fwd_bwd'].append(timeit(lambda: fwd_bwd(f), a.iters))
    lines.append(f'{"side":16s} {"fwd min":>9s} {"fwd med":>9s} {"fwd max":>9s} {"f+b min":>9s} {"f+b med":>9s} {"f+b max":>9s}')
    for k, r in res.items():
        fw, fb = sorted(r['fwd']), sorted(r['fwd_bwd'])
        lines.append(f'{k:16s} {fw[0]:9.4f} {fw[len(fw) // 2]:9.4f} {fw[-1]:9.4f} {fb[0]:9.4f} {fb[len(fb) // 2]:9.4f} {fb[-1]:9.4f}')

    # the streaming kernels alone, next to the GELU pair at the same output element count
    n_out = M * C
    lines.append('')
    lines.append(f'streaming kernels, {n_out} output elements, {a.dtype}, p = {a.p}, per-graph scale: ms and algorithmic GB/s')
    esz = 2
    xg = torch.randn(M, C, device='cuda', dtype=dt).requires_grad_(True)
    xx = torch.randn(M, 2 * C, device='cuda', dtype=dt).requires_grad_(True)
    dyo = torch.randn(M, C, device='cuda', dtype=dt)
    scale_m = scale
    cases = {'gelu': (lambda: ops.gelu_dropout(xg.view(B, -1, C), a.p, True, scale_m), xg, 2, 3)}
    for kind in ('geglu', 'glu', 'swiglu'):
        cases[kind] = ((lambda kind=kind: ops.glu_dropout(xx.view(B, -1, 2 * C), kind, a.p, True, scale_m)), xx, 3, 5)
    for name, (f, inp, pass_f, pass_b) in cases.items():
        g = dyo.view(B, -1, C)
        for _ in range(3):
            torch.autograd.grad(f(), inp, g)
        torch.cuda.synchronize()
        with torch.no_grad():
            tf = min(timeit(f, a.iters) for _ in range(a.rounds))
        tfb = min(timeit(lambda: torch.autograd.grad(f(), inp, g), a.iters) for _ in range(a.rounds))
        tb = tfb - tf
        lines.append(f'{name:8s} fwd {tf:7.4f} ms {pass_f * n_out * esz / tf / 1e6:7.0f} GB/s   bwd {tb:7.4f} ms '
                     f'{pass_b * n_out * esz / tb / 1e6:7.0f} GB/s')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or '.', exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
