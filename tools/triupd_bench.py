#!/usr/bin/env python
"""A/B of the triplet branch of ONE TGT layer with `triplet_type: tiangular_update` on the edge rows (M = B*N*N rows, C = 256,
H = 16 heads, 16-bit autocast), from the LayerNorm'd edge rows to (s, y) = the residual stream and the edge FFN's LayerNorm
output: lin_E / lin_V, the TriangularUpdate core, lin_O + gate, DropPath-less residual add, LayerNorm.  HIP events on the launch
stream, the sides ALTERNATED in one process:
  parent       what the parent commit's layer code could run for this module: TriangularUpdate.forward_normed (two narrow GEMMs,
               the lane-per-head core, library lin_O, eager gate) + ops.add_layer_norm                       -- THE BASELINE
  both_off     attend + out_proj_residual_ln with both knobs off (one fused projection, the same core on the halves, composition)
  tiled        TGT_TRIUPD_TILED on  (core on matrix-core tiles), gated off
  gated        TGT_TRIUPD_GATED on  (lin_O + gate + residual + LayerNorm as one launch each way), tiled off
  both_on      both knobs on
Forward alone (no_grad) and forward + backward (gradients of x, the residual and every parameter).  A knob earns its default only
if its gain over `both_off` exceeds the spread (max - min over the rounds) of `both_off` in the same session.
Prints a table; --out FILE also writes it (appending with --append)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tgt_amd import ops  # noqa: E402
from tgt_amd.tgt.layers.triplet import TriangularUpdate  # noqa: E402

SIDES = {'parent': None, 'both_off': (False, False), 'tiled': (True, False), 'gated': (False, True), 'both_on': (True, True)}


def timeit(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def table(lines, res):
    lines.append(f'{"side":10s} {"fwd min":>9s} {"fwd med":>9s} {"fwd max":>9s} {"f+b min":>9s} {"f+b med":>9s} {"f+b max":>9s}')
    for k, r in res.items():
        fw, fb = sorted(r['fwd']), sorted(r['fwd_bwd'])
        lines.append(f'{k:10s} {fw[0]:9.4f} {fw[len(fw) // 2]:9.4f} {fw[-1]:9.4f} {fb[0]:9.4f} {fb[len(fb) // 2]:9.4f} {fb[-1]:9.4f}')
    off = res['both_off']
    for leg in ('fwd', 'fwd_bwd'):
        base = sorted(off[leg])
        spread = base[-1] - base[0]
        for k in ('tiled', 'gated', 'both_on', 'parent'):
            med = sorted(res[k][leg])[len(res[k][leg]) // 2]
            gain = base[len(base) // 2] - med
            lines.append(f'  {leg:7s} {k:8s} median gain over both_off {gain:+.4f} ms ({100 * gain / base[len(base) // 2]:+.1f} %), '
                         f'spread of both_off {spread:.4f} ms -> {"faster by more than" if gain > spread else ("slower by more than" if -gain > spread else "within")} the spread')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='256x32,128x48', help='BxN, comma separated')
    ap.add_argument('--heads', type=int, default=16)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--out', default='')
    ap.add_argument('--append', action='store_true')
    a = ap.parse_args()
    dt = {'bf16': torch.bfloat16, 'fp16': torch.float16}[a.dtype]
    C, H = 256, a.heads
    torch.manual_seed(0)
    lines = []
    for shape in a.shapes.split(','):
        B, N = (int(v) for v in shape.split('x'))
        lines.append(f'TriangularUpdate branch of one layer, B = {B}, N = {N} (M = {B * N * N} rows), C = {C}, H = {H}, {a.dtype} autocast; '
                     f'{a.rounds} alternating rounds x {a.iters} iterations, ms per call (HIP events)')
        tria = TriangularUpdate(C, H).cuda().train()
        ln = torch.nn.LayerNorm(C).cuda()
        x = torch.randn(B, N, N, C, device='cuda', dtype=dt).requires_grad_(True)
        res_in = torch.randn(B, N, N, C, device='cuda', dtype=dt).requires_grad_(True)
        dy = torch.randn(B, N, N, C, device='cuda', dtype=dt)
        nodes = torch.randint(N // 2, N + 1, (B,), device='cuda')
        real = torch.arange(N, device='cuda')[None, :] < nodes[:, None]
        mask = ((~(real[:, :, None] & real[:, None, :])).float() * torch.finfo(torch.float32).min).unsqueeze(-1)
        params = [x, res_in, ln.weight, ln.bias] + list(tria.lin_E.parameters()) + list(tria.lin_V.parameters()) + list(tria.lin_O.parameters())

        def run(k):
            if SIDES[k] is None:
                s, y = ops.add_layer_norm(tria.forward_normed(x, mask), res_in, None, ln.weight, ln.bias, ln.eps)
            else:
                ops._TRIUPD_TILED, ops._TRIUPD_GATED = SIDES[k]
                s, y = tria.out_proj_residual_ln(tria.attend(x, mask), res_in, None, ln)
            return s + y                                     # (both outputs carry a gradient, as in the layer)

        def fwd_bwd(k):
            torch.autograd.grad(run(k), params, dy)

        with torch.autocast('cuda', dtype=dt):
            for k in SIDES:                                  # warm-up: code objects, GEMM plans, allocator
                for _ in range(3):
                    fwd_bwd(k)
            torch.cuda.synchronize()
            res = {k: dict(fwd=[], fwd_bwd=[]) for k in SIDES}
            for _ in range(a.rounds):
                for k in SIDES:
                    with torch.no_grad():
                        res[k]['fwd'].append(timeit(lambda: run(k), a.iters))
                    res[k]['fwd_bwd'].append(timeit(lambda: fwd_bwd(k), a.iters))
        table(lines, res)
        lines.append('')
        del x, res_in, dy, mask
        torch.cuda.empty_cache()
    ops._TRIUPD_TILED, ops._TRIUPD_GATED = ops.K.triupd_tiled, ops.K.triupd_gated
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or '.', exist_ok=True)
        with open(a.out, 'a' if a.append else 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
