#!/usr/bin/env python3
"""Node attention with and without per-graph node counts, kernel level (tgt_node_attention_fwd_counts / _bwd_counts).

bf16, H = 64, D = 12 at (B = 256, N = 32) and (B = 128, N = 48); counts ~ U{N/2..N} and U{4..N}, seed 0; prefix masks built from
the counts.  Forward and backward, each timed with HIP events around 20 launches, 7 alternating rounds (without, with, without,
...) in one process; reported as median (min - max) microseconds per launch.  One line per (shape, distribution, direction).

    python tools/node_ragged_bench.py [--rounds 7] [--launches 20]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tgt_amd import _lib, ops  # noqa: E402

H, D = 64, 12
SHAPES = [(256, 32), (128, 48)]
FAMILY = {v: k[len('NODE_FAMILY_'):] for k, v in vars(_lib).items() if k.startswith('NODE_FAMILY_')}


def build(B, N, counts):
    g = torch.Generator(device='cuda').manual_seed(0)
    W = H * D
    bf = torch.bfloat16
    qkv = torch.randn(B, N, 3 * W, generator=g, device='cuda').to(bf)
    eg = torch.randn(B, N, N, 2 * H, generator=g, device='cuda').to(bf)
    d_v = torch.randn(B, N, W, generator=g, device='cuda').to(bf)
    d_h = torch.randn(B, N, N, H, generator=g, device='cuda').to(bf)
    real = torch.arange(N, device='cuda')[None, :] < counts[:, None]
    pair = real[:, :, None] & real[:, None, :]
    mask = (~pair).float() * torch.finfo(torch.float32).min
    d_v, d_h = d_v * real[..., None].to(bf), d_h * pair[..., None].to(bf)
    a, _ = ops._node_args(qkv, eg, mask, H, True, False)
    out = dict(vatt=torch.empty(B, N, W, dtype=bf, device='cuda'), hhat=torch.empty(B, N, N, H, dtype=bf, device='cuda'),
               lse=torch.empty(B, N, H, device='cuda'), gsum=torch.empty(B, N, H, device='cuda'),
               d_qkv=torch.empty_like(qkv), d_eg=torch.empty_like(eg))
    for k, t in out.items():
        setattr(a, k, t.data_ptr())
    a.d_vatt, a.d_hhat = d_v.data_ptr(), d_h.data_ptr()
    keep = (qkv, eg, d_v, d_h, mask, out)
    return a, keep


def timed(entry, a, counts, launches):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    args = (C.byref(a),) if counts is None else (C.byref(a), ops._ptr(counts))
    s.record()
    for _ in range(launches):
        ops._launch(entry, *args)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000.0 / launches


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--launches', type=int, default=20)
    opt = ap.parse_args()
    rng = np.random.default_rng(0)
    for B, N in SHAPES:
        for dist, lo in (('U{N/2..N}', N // 2), ('U{4..N}', 4)):
            host = rng.integers(lo, N + 1, size=B)
            counts = torch.tensor(host, dtype=torch.int32, device='cuda')
            a, keep = build(B, N, counts)
            real_pairs = float((host.astype(np.float64) ** 2).mean() / N ** 2)
            for direction, bwd in (('fwd', 0), ('bwd', 1)):
                plain, ragged = f'tgt_node_attention_{direction}', f'tgt_node_attention_{direction}_counts'
                family = FAMILY[_lib.lib().tgt_node_attention_family(C.byref(a), bwd)]
                if bwd:
                    ops._launch('tgt_node_attention_fwd', C.byref(a))          # (statistics for the backward)
                for entry, nc in ((plain, None), (ragged, counts)):            # warm-up
                    timed(entry, a, nc, 3)
                t = {'without': [], 'with': []}
                for _ in range(opt.rounds):
                    t['without'].append(timed(plain, a, None, opt.launches))
                    t['with'].append(timed(ragged, a, counts, opt.launches))
                line = dict(B=B, N=N, H=H, D=D, counts=dist, real_pairs=round(real_pairs, 3), direction=direction, family=family)
                for k, v in t.items():
                    line[k + '_us'] = dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))
                line['ratio'] = round(statistics.median(t['with']) / statistics.median(t['without']), 3)
                print(json.dumps(line), flush=True)
            del keep


if __name__ == '__main__':
    main()
