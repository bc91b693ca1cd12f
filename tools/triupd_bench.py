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
--ragged: instead, both knobs on and the ragged stack (node counts to the core, the live tile list to the row kernels and the
gated stage) on against off, on drawn node counts and on full graphs (see ragged()).
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


def ragged(a, dt, lines):
    """--ragged: the branch with both knobs on, with and without the ragged stack (TGT_TRI_RAGGED: node counts to the tiled core;
    TGT_EDGE_RAGGED on top: the live tile list to the fused projection's row kernel and to the gated output stage), alternating in
    one process.  Two arms per shape: `ragged` -- node counts numpy default_rng(0).integers(N // 4, N, endpoint=True), printed --
    and `full` -- every count N, where the list names every tile and the counts skip nothing: what the switches cost when
    there is nothing to skip.  The counts and the list are built outside the timed region (a model builds them once per forward,
    for all its layers).  `off` is the parent's code path."""
    import numpy as np
    C, H = 256, a.heads
    ops._TRIUPD_TILED, ops._TRIUPD_GATED = True, True
    for shape in a.shapes.split(','):
        B, N = (int(v) for v in shape.split('x'))
        drawn = np.random.default_rng(0).integers(N // 4, N, size=B, endpoint=True)
        lines.append(f'TriangularUpdate branch of one layer on ragged batches, B = {B}, N = {N} (M = {B * N * N} rows), C = {C}, H = {H}, '
                     f'{a.dtype} autocast; {a.rounds} alternating rounds x {a.iters} iterations, ms per call (HIP events)')
        tria = TriangularUpdate(C, H).cuda().train()
        ln = torch.nn.LayerNorm(C).cuda()
        x = torch.randn(B, N, N, C, device='cuda', dtype=dt).requires_grad_(True)
        res_in = torch.randn(B, N, N, C, device='cuda', dtype=dt).requires_grad_(True)
        dy = torch.randn(B, N, N, C, device='cuda', dtype=dt)
        params = [x, res_in, ln.weight, ln.bias] + list(tria.lin_E.parameters()) + list(tria.lin_V.parameters()) + list(tria.lin_O.parameters())
        for arm, counts in (('ragged', drawn), ('full', np.full(B, N))):
            nodes = torch.from_numpy(np.asarray(counts, dtype=np.int32)).cuda()
            real = torch.arange(N, device='cuda')[None, :] < nodes[:, None]
            mask = ((~(real[:, :, None] & real[:, None, :])).float() * torch.finfo(torch.float32).min).unsqueeze(-1)
            live = ops.edge_live_tiles(nodes, N)
            tiles = live.tiles.cpu()
            lines.append(f'arm {arm}: node counts {counts.tolist()}')
            lines.append(f'arm {arm}: real pairs {int((nodes.long() ** 2).sum())} of {B * N * N} '
                         f'({100.0 * float((nodes.double() ** 2).sum()) / (B * N * N):.1f} %), live 32-row tiles {int(tiles[0])} of {tiles.numel() - 1}')

            def run(on):
                with ops.edge_live(live if on else None):
                    s, y = tria.out_proj_residual_ln(tria.attend(x, mask, node_counts=nodes if on else None), res_in, None, ln)
                return s + y

            def fwd_bwd(on):
                torch.autograd.grad(run(on), params, dy)

            with torch.autocast('cuda', dtype=dt):
                for on in (False, True):
                    for _ in range(3):
                        fwd_bwd(on)
                torch.cuda.synchronize()
                res = {on: dict(fwd=[], fwd_bwd=[]) for on in (False, True)}
                for _ in range(a.rounds):
                    for on in (False, True):
                        with torch.no_grad():
                            res[on]['fwd'].append(timeit(lambda: run(on), a.iters))
                        res[on]['fwd_bwd'].append(timeit(lambda: fwd_bwd(on), a.iters))
            lines.append(f'{"side":10s} {"fwd min":>9s} {"fwd med":>9s} {"fwd max":>9s} {"f+b min":>9s} {"f+b med":>9s} {"f+b max":>9s}')
            for on in (False, True):
                fw, fb = sorted(res[on]['fwd']), sorted(res[on]['fwd_bwd'])
                lines.append(f'{"on" if on else "off":10s} {fw[0]:9.4f} {fw[len(fw) // 2]:9.4f} {fw[-1]:9.4f} {fb[0]:9.4f} {fb[len(fb) // 2]:9.4f} {fb[-1]:9.4f}')
            for leg in ('fwd', 'fwd_bwd'):
                base, got = sorted(res[False][leg]), sorted(res[True][leg])
                spread = base[-1] - base[0]
                gain = base[len(base) // 2] - got[len(got) // 2]
                verdict = 'faster by more than' if gain > spread else ('SLOWER by more than' if -gain > spread else 'within')
                lines.append(f'  {arm:6s} {leg:7s} on: median gain over off {gain:+.4f} ms ({100 * gain / base[len(base) // 2]:+.1f} %), '
                             f'min-max spread of off {spread:.4f} ms -> {verdict} the spread')
            del mask
        lines.append('')
        del x, res_in, dy
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='256x32,128x48', help='BxN, comma separated')
    ap.add_argument('--heads', type=int, default=16)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--out', default='')
    ap.add_argument('--append', action='store_true')
    ap.add_argument('--ragged', action='store_true',
                    help='the ragged A/B instead: node counts (numpy default_rng(0) integers in [N/4, N], printed) and an arm with every '
                         'count N, the ragged stack on against off')
    a = ap.parse_args()
    dt = {'bf16': torch.bfloat16, 'fp16': torch.float16}[a.dtype]
    C, H = 256, a.heads
    torch.manual_seed(0)
    lines = []
    for shape in ([] if a.ragged else a.shapes.split(',')):
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
    if a.ragged:
        ragged(a, dt, lines)
    ops._TRIUPD_TILED, ops._TRIUPD_GATED = ops.K.triupd_tiled, ops.K.triupd_gated
    text ='\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or '.', exist_ok=True)
        with open(a.out, 'a' if a.append else 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
