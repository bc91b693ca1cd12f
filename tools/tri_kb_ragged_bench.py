"""Stand-alone timing of the key-blocked triplet attention kernels (csrc/triplet_attention_kb.hip, 65 <= N <= 128) on a ragged
batch, with the node counts ignored (TGT_TRI_COUNTS_KB clear: the kernels every caller runs by default) or used (`--counts-kb`:
the bit set, padded units, query tiles and key blocks skipped).

One process = one setting: the forward and forward + backward of ops.triplet_attention under HIP events, `--repeats` times each,
median (min - max) in one JSON line.  `--full-counts` gives every graph N nodes: the with-counts kernels with nothing to skip.
For an A/B, alternate the two settings in fresh processes (the caller's job script).

    python tools/tri_kb_ragged_bench.py --nodes 96 --batch 32 [--counts-kb] [--full-counts] [--width 256] [--heads 16]
                                        [--dtype bf16|fp16] [--iters 10] [--warmup 3] [--repeats 5] [--seed 0]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def stats(xs):
    xs = sorted(xs)
    return {'median': round(xs[len(xs) // 2], 4), 'min': round(xs[0], 4), 'max': round(xs[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, default=96)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--width', type=int, default=256)
    ap.add_argument('--heads', type=int, default=16)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp16'])
    ap.add_argument('--counts-kb', action='store_true', help='set TGT_TRI_COUNTS_KB: the kernels use the counts')
    ap.add_argument('--full-counts', action='store_true', help='every graph has N nodes (nothing to skip)')
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    from tgt_amd import ops
    dt = torch.bfloat16 if a.dtype == 'bf16' else torch.float16
    B, N, C, H = a.batch, a.nodes, a.width, a.heads
    g = torch.Generator().manual_seed(a.seed)
    counts = torch.full((B,), N) if a.full_counts else torch.randint(N // 2, N + 1, (B,), generator=g)      # U{N/2..N}
    ops._TRI_RAGGED_KB = bool(a.counts_kb)
    L = ops.TripletLayout(C, H)
    torch.manual_seed(a.seed)
    nm = torch.arange(N)[None, :] < counts[:, None]
    real = (nm[:, :, None] & nm[:, None, :]).cuda()
    mask3 = ((~real).float() * torch.finfo(torch.float32).min).contiguous()
    fused = torch.randn(B, N, N, L.width, device='cuda', dtype=dt).requires_grad_(True)
    d_out = torch.randn(B, N, N, 2 * C, device='cuda', dtype=dt) * real.unsqueeze(-1).to(dt)      # zero at padded rows and columns
    nc = counts.to(torch.int32).cuda()

    def fwd():
        return ops.triplet_attention(fused, mask3, L, node_counts=nc)

    def fwd_bwd():
        torch.autograd.grad(fwd(), fused, d_out)

    t_f, t_fb = [], []
    for _ in range(a.repeats):
        t_f.append(timeit(fwd, a.iters, a.warmup))
        t_fb.append(timeit(fwd_bwd, a.iters, a.warmup))
    n = counts.double()
    share = float((n / N * (torch.ceil(n / 32) / ((N + 31) // 32)) ** 2).mean())      # work left by arithmetic
    print(json.dumps({'kernel': 'tri_att_kb', 'B': B, 'N': N, 'C': C, 'H': H, 'dtype': a.dtype, 'counts_kb': bool(a.counts_kb),
                      'full_counts': bool(a.full_counts), 'mean_count': round(float(n.mean()), 2), 'work_share': round(share, 3),
                      'fwd_ms': stats(t_f), 'fwd_bwd_ms': stats(t_fb)}))


if __name__ == '__main__':
    main()
