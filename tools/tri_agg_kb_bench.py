"""Stand-alone timing of the key-blocked triplet aggregate kernels (65 <= N <= 128, csrc/triplet_aggregate_kb.hip) at
C = 256, H = 16 in 16-bit: N = 96 at B = 32 and N = 128 at B = 16.

Prints, per shape and direction of autograd, the HIP-event time of the kernels behind tgt_triplet_aggregate_fwd / _bwd, their
algorithmic bytes as a fraction of 8 TB/s (V, E / G and mask read, O written; the backward's counterparts), and the time and
peak memory of the plain torch composition of the same math on the device (softmax / sigmoid / einsum in the same dtype).

    python tools/tri_agg_kb_bench.py [--dtype bf16|fp16] [--iters 5] [--no-torch] [--out profiles/tri_agg_kb_bench.txt]
Every timed step runs under --step-limit seconds (checked after each synchronize; the run stops at the first step over it).
"""
import argparse
import ctypes as C
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 8e12


def timed(fn, iters, limit):
    fn()
    torch.cuda.synchronize()
    best = float('inf')
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.time()
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        if time.time() - t0 > limit:
            raise SystemExit(f'step over the limit of {limit} s')
        best = min(best, s.elapsed_time(e))
    return best


def torch_composition(fused, mask3, Lyt):
    """the reference's chain (lib/tgt/layers/triplet.py:56-70) on head-major operands, gated: the outward direction unmasked"""
    B, N = fused.shape[:2]
    C_, H, D = Lyt.C, Lyt.H, Lyt.D
    m = mask3.to(fused.dtype)[..., None]
    outs = []
    for d in (0, 1):
        v = fused[..., Lyt.v[d]:Lyt.v[d] + C_].view(B, N, N, H, D)
        e, g = fused[..., Lyt.e[d]:Lyt.e[d] + H], fused[..., Lyt.g[d]:Lyt.g[d] + H]
        if d == 0:
            a = torch.softmax(e + m, 2) * torch.sigmoid(g + m)
            outs.append(torch.einsum('bikh,bjkhd->bijhd', a, v))
        else:
            a = torch.softmax(e, 1) * torch.sigmoid(g)
            outs.append(torch.einsum('bkih,bkjhd->bijhd', a, v))
    return torch.cat([o.reshape(B, N, N, C_) for o in outs], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp16'])
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--step-limit', type=float, default=20.0)
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    from tgt_amd import ops, _lib
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    dt = torch.bfloat16 if args.dtype == 'bf16' else torch.float16
    Lyt = ops.AggregateLayout(256, 16)
    say(f'{torch.cuda.get_device_name(0)}; best of {args.iters} HIP-event timings per step')
    for B, N in ((32, 96), (16, 128)):
        torch.manual_seed(0)
        fused = torch.randn(B, N, N, Lyt.width, device='cuda', dtype=dt)
        d_out = torch.randn(B, N, N, 2 * Lyt.C, device='cuda', dtype=dt)
        mask3 = torch.zeros(B, N, N, device='cuda')
        out = torch.empty(B, N, N, 2 * Lyt.C, device='cuda', dtype=dt)
        d_fused = torch.empty_like(fused)
        L = _lib.lib()
        a_f = ops._agg_args(fused, mask3, out, Lyt)
        a_b = ops._agg_args(fused, mask3, out, Lyt, d_out, d_fused)
        t_f = timed(lambda: _lib.check(L.tgt_triplet_aggregate_fwd(C.byref(a_f), ops._stream()), 'fwd'), args.iters, args.step_limit)
        t_b = timed(lambda: _lib.check(L.tgt_triplet_aggregate_bwd(C.byref(a_b), ops._stream()), 'bwd'), args.iters, args.step_limit)
        rows, esz = B * N * N, fused.element_size()
        v, eg, o, msk = rows * 2 * Lyt.C * esz, rows * 4 * Lyt.H * esz, rows * 2 * Lyt.C * esz, rows * 4
        by_f = v + eg + msk + o
        by_b = v + eg + msk + o + v + eg              # sources + d_out read, d_v + d_eg written
        say(f'B={B} N={N} C=256 H=16 {args.dtype}')
        say(f'  tgt_triplet_aggregate_fwd  {t_f:8.3f} ms   {by_f / 1e9:6.3f} GB algorithmic = {by_f / (t_f * 1e-3) / HBM:.3f} of 8 TB/s')
        say(f'  tgt_triplet_aggregate_bwd  {t_b:8.3f} ms   {by_b / 1e9:6.3f} GB algorithmic = {by_b / (t_b * 1e-3) / HBM:.3f} of 8 TB/s')
        if not args.no_torch:
            try:
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                fr = fused.clone().requires_grad_(True)
                t_tf = timed(lambda: torch_composition(fr.detach(), mask3, Lyt), max(1, args.iters // 2), args.step_limit)

                def fb():
                    fr.grad = None
                    torch_composition(fr, mask3, Lyt).backward(d_out)
                t_tfb = timed(fb, max(1, args.iters // 2), args.step_limit)
                peak = (torch.cuda.max_memory_allocated() - base) / 1e9
                say(f'  torch composition          fwd {t_tf:8.3f} ms, fwd+bwd {t_tfb:8.3f} ms (kernels fwd+bwd {t_f + t_b:.3f} ms), '
                    f'peak memory above the operands {peak:.2f} GB (kernels: out + d_fused = {(o + d_fused.numel() * esz) / 1e9:.2f} GB)')
                del fr
            except torch.cuda.OutOfMemoryError:
                say('  torch composition          out of memory')
        del fused, d_out, out, d_fused
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
