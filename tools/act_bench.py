#!/usr/bin/env python
"""A/B of the FFN block with a plain activation (relu / silu / elu) on the edge rows (M = B*N*N rows, 256 -> 256 -> 256 channels,
16-bit autocast, activation dropout), as TGT_Layer runs it: hidden = dropout(act(lin_W1(x))), then lin_W2 + residual add + the next
LayerNorm (ops.linear_residual_layer_norm).  HIP events on the launch stream, the three sides ALTERNATED in one process:
  (a) knob on   TGT_EPI_ACT forward, TGT_EPI_ACT_BWD as the epilogue of lin_W2's data gradient;
  (b) knob off  library GEMM + tgt_act_dropout_fwd / _bwd;
  (c) eager     the composition this path ran before the kernels: library GEMM, F.relu / F.silu / F.elu, nn.Dropout (stored mask).
Then the node FFN (rows x 768, FFN.forward_normed): the streaming pair against the eager composition.
Prints a table; --out FILE also writes it (appending with --append)."""
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


def eager_hidden(ffn, x):
    """FFN.hidden as it ran for these names before the kernels (blocks.py, last branch)"""
    return ffn.dropout(ffn.ffn_fn(ffn.lin_W1(x)))


def table(lines, res):
    lines.append(f'{"side":12s} {"fwd min":>9s} {"fwd med":>9s} {"fwd max":>9s} {"f+b min":>9s} {"f+b med":>9s} {"f+b max":>9s}')
    for k, r in res.items():
        fw, fb = sorted(r['fwd']), sorted(r['fwd_bwd'])
        lines.append(f'{k:12s} {fw[0]:9.4f} {fw[len(fw) // 2]:9.4f} {fw[-1]:9.4f} {fb[0]:9.4f} {fb[len(fb) // 2]:9.4f} {fb[-1]:9.4f}')


def measure(sides, params, dy, rounds, iters, setup):
    def fwd_bwd(k):
        setup(k)
        torch.autograd.grad(sides[k](), params, dy)
    for k in sides:                                          # warm-up: code objects, GEMM plans, allocator
        for _ in range(3):
            fwd_bwd(k)
    torch.cuda.synchronize()
    res = {k: dict(fwd=[], fwd_bwd=[]) for k in sides}
    for _ in range(rounds):
        for k in sides:
            setup(k)
            with torch.no_grad():
                res[k]['fwd'].append(timeit(sides[k], iters))
            res[k]['fwd_bwd'].append(timeit(lambda: fwd_bwd(k), iters))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=256)
    ap.add_argument('--N', type=int, default=32)
    ap.add_argument('--node-rows', type=int, default=8192)
    ap.add_argument('--p', type=float, default=0.1)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--activations', default='relu,silu,elu')
    ap.add_argument('--out', default='')
    ap.add_argument('--append', action='store_true')
    a = ap.parse_args()
    dt = {'bf16': torch.bfloat16, 'fp16': torch.float16}[a.dtype]
    B, N, C = a.B, a.N, 256
    M = B * N * N
    torch.manual_seed(0)
    lines = []
    for act in a.activations.split(','):
        lines.append(f'edge FFN block A/B, activation={act}, M = {M} rows, C = {C}, {a.dtype} autocast, p = {a.p}; '
                     f'{a.rounds} alternating rounds x {a.iters} iterations, ms per call (HIP events)')
        ffn = FFN(C, 1., act_dropout=a.p, activation=act).cuda().train()
        ln = torch.nn.LayerNorm(C).cuda()
        x = torch.randn(B, N, N, C, device='cuda', dtype=dt).requires_grad_(True)
        res_in = torch.randn(B, N, N, C, device='cuda', dtype=dt).requires_grad_(True)
        dy = torch.randn(B, N, N, C, device='cuda', dtype=dt)
        params = [x, res_in, ffn.lin_W1.weight, ffn.lin_W1.bias, ffn.lin_W2.weight, ffn.lin_W2.bias]

        def block(hidden):
            s, y = ops.linear_residual_layer_norm(hidden(x), ffn.lin_W2.weight, ffn.lin_W2.bias, res_in, None, ln.weight, ln.bias, ln.eps)
            return s + y                                     # (both outputs carry a gradient, as in the layer)

        def setup(k):
            ops._FFN_ACT_EPI = k == 'a_knob_on'
        with torch.autocast('cuda', dtype=dt):
            ops._FFN_ACT_EPI = True
            assert ops.linear_act_dropout_ok(x, ffn.lin_W1.weight), 'the fused launch does not take this shape'
            sides = {'a_knob_on': lambda: block(ffn.hidden), 'b_knob_off': lambda: block(ffn.hidden),
                     'c_eager': lambda: block(lambda t: eager_hidden(ffn, t))}
            table(lines, measure(sides, params, dy, a.rounds, a.iters, setup))
        lines.append('')
        del x, res_in, dy

        R, W = a.node_rows, 768
        lines.append(f'node FFN (forward_normed), activation={act}, {R} rows x {W}, {a.dtype} autocast, p = {a.p}: ms per call')
        nffn = FFN(W, 1., act_dropout=a.p, activation=act).cuda().train()
        xn = torch.randn(R // 32, 32, W, device='cuda', dtype=dt).requires_grad_(True)
        dyn = torch.randn(R // 32, 32, W, device='cuda', dtype=dt)
        nparams = [xn, nffn.lin_W1.weight, nffn.lin_W1.bias, nffn.lin_W2.weight, nffn.lin_W2.bias]
        with torch.autocast('cuda', dtype=dt):
            nsides = {'kernels': lambda: nffn.forward_normed(xn), 'c_eager': lambda: nffn.lin_W2(eager_hidden(nffn, xn))}
            table(lines, measure(nsides, nparams, dyn, a.rounds, a.iters, lambda k: None))
        lines.append('')
    ops._FFN_ACT_EPI = ops.K.ffn_act_epi
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or '.', exist_ok=True)
        with open(a.out, 'a' if a.append else 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
