"""Stand-alone timing of the node attention BACKWARD (tgt_node_attention_bwd) at 65 <= N <= 128 -- the key-blocked kernel of
csrc/node_attention_kb_bwd.hip, or with TGT_NODE_KB_BWD=0 in the environment the lane-per-head pair it replaces (same library).

The backward is timed alone as tools/kernel_bench.py does it: HIP events around (forward + backward) minus events around the
forward.  Prints one JSON line: ms, algorithmic GB/s and its fraction of 8 TB/s -- bytes: E, G, dH_hat read and dE, dG written
(5 H halves per pair), plus the node rows (qkv, V_att, dV_att read, d_qkv written: 8 W per node) -- and the value of
tgt_node_attention_family for the backward call (5 = key-blocked backward, 1 = lane per head; include/tgt_hip.h).

    python tools/node_att_kb_bench.py --nodes 80 --batch 64 [--heads 64] [--width 768] [--dtype bf16|fp16] [--iters 20] [--repeats 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 8e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, default=80)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--heads', type=int, default=64)
    ap.add_argument('--width', type=int, default=768)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp16'])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=5, help='(forward, forward + backward) pairs; the median difference is reported')
    a = ap.parse_args()
    from tgt_amd import _lib, ops
    dt = torch.bfloat16 if a.dtype == 'bf16' else torch.float16
    B, N, H, W = a.batch, a.nodes, a.heads, a.width
    torch.manual_seed(0)
    qkv = torch.randn(B, N, 3 * W, device='cuda', dtype=dt).requires_grad_(True)
    eg = torch.randn(B, N, N, 2 * H, device='cuda', dtype=dt).requires_grad_(True)
    gv, gh = torch.randn(B, N, W, device='cuda', dtype=dt), torch.randn(B, N, N, H, device='cuda', dtype=dt)
    mask = torch.zeros(B, N, N, device='cuda')

    args, _ = ops._node_args(qkv, eg, mask, H, True, False)
    for f in ('vatt', 'hhat', 'lse', 'gsum', 'd_vatt', 'd_hhat', 'd_qkv', 'd_eg'):      # (only looked at: nullness and alignment)
        setattr(args, f, qkv.data_ptr())
    family = _lib.lib().tgt_node_attention_family(C.byref(args), 1)

    def fwd():
        return ops.node_attention(qkv, eg, mask, H)

    def fwd_bwd():
        v, h = fwd()
        torch.autograd.grad([v, h], [qkv, eg], [gv, gh])

    diffs = []
    for _ in range(a.repeats):
        t_f = timeit(fwd, a.iters, a.warmup)
        t_fb = timeit(fwd_bwd, a.iters, a.warmup)
        diffs.append(t_fb - t_f)
    diffs.sort()
    ms = diffs[len(diffs) // 2]
    esz = 2
    nbytes = B * (N * N * 5 * H + N * 8 * W) * esz
    print(json.dumps({'kernel': 'node_att_bwd', 'B': B, 'N': N, 'H': H, 'W': W, 'dtype': a.dtype, 'family': family,
                      'TGT_NODE_KB_BWD': os.environ.get('TGT_NODE_KB_BWD', '1'), 'ms': round(ms, 4),
                      'ms_min': round(diffs[0], 4), 'ms_max': round(diffs[-1], 4), 'GBs': round(nbytes / ms / 1e6, 1),
                      'of_8TBs': round(nbytes / (ms * 1e-3) / HBM, 3)}))


if __name__ == '__main__':
    main()
