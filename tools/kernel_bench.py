#!/usr/bin/env python
"""Micro-benchmark of the hand-written kernels at the BASELINE shapes
(B=256, N=32, C=256, Ht=16; W=768, Hn=64), HIP events on the launch stream.
Prints algorithmic GB/s per kernel (bytes as in DESIGN.md §4)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tgt_amd import ops  # noqa: E402


def timeit(fn, iters):
    for _ in range(3):
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
    ap.add_argument('--B', type=int, default=None, help='graphs (default 256; --only aggproj: 512, the config-5 inference batch)')
    ap.add_argument('--N', type=int, default=32)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--only', default='')
    a = ap.parse_args()
    # ('aggproj' / 'triproj64' name their own blocks only, not the 'agg', 'tri' and 'proj' ones)
    rest = a.only.replace('aggproj', '').replace('triproj64_train', '').replace('triproj64', '')
    agg_b = a.B or 512
    a.B = a.B or 256
    dt = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}[a.dtype]
    esz = 4 if a.dtype == 'fp32' else 2
    B, N, C, Ht, W, Hn = a.B, a.N, 256, 16, 768, 64
    dev = 'cuda'
    torch.manual_seed(0)
    mask = torch.zeros(B, N, N, device=dev)
    out = {}
    n2 = N * N

    if not a.only or 'tri' in rest:
        L = ops.TripletLayout(C, Ht)
        fused = torch.randn(B, N, N, L.width, device=dev, dtype=dt).requires_grad_(True)
        va = ops.triplet_attention(fused, mask, L)
        g = torch.randn_like(va)
        fb = B * (2 * (4 * n2 * C + 2 * n2 * Ht) * esz + n2 * 4)
        bb = B * (2 * (7 * n2 * C + 4 * n2 * Ht) * esz + n2 * 4)
        t = timeit(lambda: ops.triplet_attention(fused, mask, L), a.iters)
        out['tri_att_fwd'] = dict(ms=round(t, 4), GBs=round(fb / t / 1e6, 1))
        t2 = timeit(lambda: torch.autograd.grad(ops.triplet_attention(fused, mask, L), fused, g), a.iters)
        out['tri_att_bwd'] = dict(ms=round(t2 - t, 4), GBs=round(bb / (t2 - t) / 1e6, 1))
        del fused, va, g

    if 'tricol' in a.only:
        # the backward as the training step runs it: projection + attention as one autograd node,
        # bias gradient accumulated inside the backward kernel (CS variant)
        L = ops.TripletLayout(C, Ht)
        x = torch.randn(B, N, N, C, device=dev, dtype=dt).requires_grad_(True)
        w = (torch.randn(L.width, C, device=dev) * C ** -0.5).to(dt).requires_grad_(True)
        bias = torch.randn(L.width, device=dev).to(dt).requires_grad_(True)
        g = torch.randn(B, N, N, 2 * C, device=dev, dtype=dt)
        prof = ops.profile_kernels(True)
        for _ in range(a.iters):
            torch.autograd.grad(ops.projected_triplet_attention(x, w, bias, mask, L), (x, w, bias), g)
        torch.cuda.synchronize()
        ops.profile_kernels(False)
        out['tricol'] = {k: round(sum(v[1:]) / max(1, len(v) - 1), 4) for k, v in ops.kernel_times_ms(prof).items()}
        del x, w, bias, g

    if 'proj' in rest:
        # projection + attention forward as the training step runs it: fused kernel (TGT_TRI_PROJ=1, default) or GEMM + GEMM + attention
        L = ops.TripletLayout(C, Ht)
        x = torch.randn(B, N, N, C, device=dev, dtype=dt)
        w = (torch.randn(L.width, C, device=dev) * C ** -0.5).to(dt)
        bias = torch.randn(L.width, device=dev).to(dt)
        with torch.no_grad():
            t = timeit(lambda: ops.projected_triplet_attention(x, w, bias, mask, L), a.iters)
        out['proj+tri_att_fwd'] = dict(ms=round(t, 4), fused=bool(ops._TRI_PROJ))

    if 'projflag' in a.only:
        # tgt_triplet_attention_proj_fwd itself (the C entry point, no host work around it) with the Q/K/V rows written (training)
        # and without (TGT_TRI_NO_QKV_STORE: inference), alternating rounds in one process; algorithmic bytes = X once + O out
        # (+ Q, K, V out): DESIGN.md section 4
        import ctypes
        import statistics
        from tgt_amd import _lib
        L = ops.TripletLayout(C, Ht)
        x = torch.randn(B, N, N, C, device=dev, dtype=dt)
        w = (torch.randn(L.width, C, device=dev) * C ** -0.5).to(dt)
        bias = torch.randn(L.width, device=dev).to(dt)
        eg = torch.addmm(bias[6 * C:], x.view(-1, C), w[6 * C:].t()).view(B, N, N, L.used - 6 * C)
        o = torch.empty(B, N, N, 2 * C, device=dev, dtype=dt)
        qkv = torch.empty(B, N, N, 6 * C, device=dev, dtype=dt)
        args = {False: ops._tri_args(qkv, mask, o, L, eg=eg), True: ops._tri_args(None, mask, o, L, eg=eg)}
        fn = _lib.lib().tgt_triplet_attention_proj_fwd

        def run(flag):
            _lib.check(fn(ctypes.byref(args[flag]), ops._ptr(x), C, ops._ptr(w), ops._ptr(bias), ops._stream()), 'tgt_triplet_attention_proj_fwd')
        times = {False: [], True: []}
        for _ in range(7):
            for flag in (False, True):
                times[flag].append(timeit(lambda: run(flag), a.iters))
        nbytes = {False: B * n2 * (C + 2 * C + 6 * C) * esz, True: B * n2 * (C + 2 * C) * esz}
        for flag, name in ((False, 'proj_fwd_store'), (True, 'proj_fwd_no_qkv_store')):
            med = statistics.median(times[flag])
            out[name] = dict(ms=round(med, 4), min=round(min(times[flag]), 4), max=round(max(times[flag]), 4),
                             GBs=round(nbytes[flag] / med / 1e6, 1), rounds=[round(t, 4) for t in times[flag]])

    if not a.only or 'agg' in rest:
        L = ops.AggregateLayout(C, Ht)
        fused = torch.randn(B, N, N, L.width, device=dev, dtype=dt).requires_grad_(True)
        g = torch.randn(B, N, N, 2 * C, device=dev, dtype=dt)
        fb = B * (2 * (2 * n2 * C + 2 * n2 * Ht) * esz + n2 * 4)
        t = timeit(lambda: ops.triplet_aggregate(fused, mask, L), a.iters)
        out['tri_agg_fwd'] = dict(ms=round(t, 4), GBs=round(fb / t / 1e6, 1))
        t2 = timeit(lambda: torch.autograd.grad(ops.triplet_aggregate(fused, mask, L), fused, g), a.iters)
        bb = B * (2 * (3 * n2 * C + 4 * n2 * Ht) * esz + n2 * 4)
        out['tri_agg_bwd'] = dict(ms=round(t2 - t, 4), GBs=round(bb / (t2 - t) / 1e6, 1))
        del fused, g

    if 'aggproj' in a.only:
        # tgt_triplet_aggregate_proj_fwd itself (the C entry point on pre-projected E/G rows, a.v = NULL) + the narrow E/G Linear it
        # needs, against what it replaces: the library GEMM of the fused row [V_in | V_out | E | G] + tgt_triplet_aggregate_fwd.
        # fp16 and bf16, 7 alternating rounds in one process; algorithmic bytes of both paths from the shapes
        # --N above 32: tgt_triplet_aggregate_proj64_fwd (33..64 nodes); the plain kernel it is compared with then
        # walks the graph once per 32-row query tile and reads every V slab twice
        import ctypes
        import statistics
        from tgt_amd import _lib
        Bp = agg_b
        L = ops.AggregateLayout(C, Ht)
        ne, rows = L.used - 2 * C, Bp * n2
        maskp = torch.zeros(Bp, N, N, device=dev)
        v_reads = 1 if N <= 32 else 2
        byts = dict(unfused=rows * (C + L.width + L.width + (v_reads - 1) * 2 * C + 2 * C) * 2, fused=rows * (C + ne + 2 * C + ne + 2 * C) * 2,
                    kernel=rows * (2 * C + ne + 2 * C) * 2)
        out['aggproj_bytes'] = dict(byts, B=Bp, N=N, H=Ht)
        cases = {}
        for name, dtp in (('fp16', torch.float16), ('bf16', torch.bfloat16)):
            x = torch.randn(Bp, N, N, C, device=dev, dtype=dtp)
            w = (torch.randn(L.width, C, device=dev) * C ** -0.5).to(dtp)
            bias = torch.randn(L.width, device=dev).to(dtp)
            x2, we, be = x.view(-1, C), w[2 * C:], bias[2 * C:].contiguous()
            o = torch.empty(Bp, N, N, 2 * C, device=dev, dtype=dtp)
            own_eg = ops._edge_kernel_ok(x2, ne, dtp)

            egv, _ = ops._agg_proj_eg_view(o, L)                 # (as ops.projected_triplet_aggregate: E/G inside the result's own columns)

            def narrow(x2=x2, we=we, be=be, own_eg=own_eg, egv=egv):
                return ops.edge_linear_raw(x2, we, be, out=egv) if own_eg else torch.addmm(be, x2, we.t(), out=egv)
            ap_ = ops._agg_proj_args(o, maskp, o, L)
            entry = 'tgt_triplet_aggregate_proj_fwd' if N <= 32 else 'tgt_triplet_aggregate_proj64_fwd'
            fn = getattr(_lib.lib(), entry)

            def kernel(ap_=ap_, x=x, w=w, bias=bias):
                _lib.check(fn(ctypes.byref(ap_), ops._ptr(x), C, ops._ptr(w), ops._ptr(bias), ops._stream()), entry)

            def fused(narrow=narrow, kernel=kernel):
                narrow()
                kernel()
            narrow()                 # ('kernel' alone then runs on whatever the previous launch left in those columns: finite, same work)

            def unfused(x2=x2, w=w, bias=bias, o=o):
                f = torch.addmm(bias, x2, w.t()).view(Bp, N, N, L.width)
                au = ops._agg_args(f, maskp, o, L)
                _lib.check(_lib.lib().tgt_triplet_aggregate_fwd(ctypes.byref(au), ops._stream()), 'tgt_triplet_aggregate_fwd')
            cases[name] = dict(kernel=kernel, fused=fused, unfused=unfused, keep=(x, w, bias, o))
        times = {(n_, k): [] for n_ in cases for k in ('kernel', 'fused', 'unfused')}
        for _ in range(7):
            for key in times:
                times[key].append(timeit(cases[key[0]][key[1]], a.iters))
        for (n_, k), ts in times.items():
            med = statistics.median(ts)
            out[f'aggproj_{k}_{n_}'] = dict(ms=round(med, 4), min=round(min(ts), 4), max=round(max(ts), 4),
                                           GBs=round(byts[k] / med / 1e6, 1), share_of_8TBs=round(byts[k] / med / 1e6 / 8000, 3),
                                           rounds=[round(t, 4) for t in ts])
        del cases

    if 'triproj64' in a.only.replace('triproj64_train', ''):
        # tgt_triplet_attention_proj64_fwd itself (the C entry point on pre-projected E/G rows, a.qkv = NULL), the same + the narrow
        # E/G Linear it needs, and what the pair replaces: the split GEMMs (Q/K/V 1536 wide, E/G narrow) + tgt_triplet_attention_fwd
        # (tri_att16_fwd_kernel at these node counts).  fp16 and bf16, 7 alternating rounds in one process; algorithmic bytes per edge
        # row as in DESIGN.md 4.w-64 (16-bit, gated, C = 256)
        import ctypes
        import statistics
        from tgt_amd import _lib
        assert 33 <= N <= 64, '--only triproj64 needs --N in 33..64'
        Bp = a.B
        L = ops.TripletLayout(C, Ht)
        ne, rows = L.used - 6 * C, Bp * n2
        maskp = torch.zeros(Bp, N, N, device=dev)
        # kernel: X 3 x C (row j and column j inward, column j outward), E/G, O out (2C); fused: + the narrow Linear (X in, E/G out);
        # unfused: GEMMs (X in, Q/K/V 6C and E/G out) + kernel (Q/K/V and E/G in, O out)
        byts = dict(kernel=rows * (3 * C + ne + 2 * C) * 2, fused=rows * (C + ne + 3 * C + ne + 2 * C) * 2,
                    unfused=rows * (C + 6 * C + ne + 6 * C + ne + 2 * C) * 2)
        out['triproj64_bytes'] = dict(byts, B=Bp, N=N, H=Ht, per_row={k: v // rows for k, v in byts.items()})
        cases = {}
        for name, dtp in (('fp16', torch.float16), ('bf16', torch.bfloat16)):
            x = torch.randn(Bp, N, N, C, device=dev, dtype=dtp)
            w = (torch.randn(L.width, C, device=dev) * C ** -0.5).to(dtp)
            bias = torch.randn(L.width, device=dev).to(dtp)
            x2, wq, bq, we, be = x.view(-1, C), w[:6 * C], bias[:6 * C], w[6 * C:L.used], bias[6 * C:L.used]
            o = torch.empty(Bp, N, N, 2 * C, device=dev, dtype=dtp)

            def narrow(x2=x2, we=we, be=be, dtp=dtp):
                return ops._narrow_linear(x2, we, be, dtp).view(Bp, N, N, ne)
            ap_ = ops._tri_args(None, maskp, o, L, eg=narrow())
            fn = _lib.lib().tgt_triplet_attention_proj64_fwd

            def kernel(ap_=ap_, x=x, w=w, bias=bias):
                _lib.check(fn(ctypes.byref(ap_), ops._ptr(x), C, ops._ptr(w), ops._ptr(bias), ops._stream()), 'tgt_triplet_attention_proj64_fwd')

            def fused(narrow=narrow, x=x, w=w, bias=bias, o=o):
                af = ops._tri_args(None, maskp, o, L, eg=narrow())
                _lib.check(fn(ctypes.byref(af), ops._ptr(x), C, ops._ptr(w), ops._ptr(bias), ops._stream()), 'tgt_triplet_attention_proj64_fwd')

            def unfused(narrow=narrow, x2=x2, wq=wq, bq=bq, o=o):
                f = torch.addmm(bq, x2, wq.t()).view(Bp, N, N, 6 * C)
                au = ops._tri_args(f, maskp, o, L, eg=narrow())
                _lib.check(_lib.lib().tgt_triplet_attention_fwd(ctypes.byref(au), ops._stream()), 'tgt_triplet_attention_fwd')
            cases[name] = dict(kernel=kernel, fused=fused, unfused=unfused, keep=(x, w, bias, o, ap_))
        times = {(n_, k): [] for n_ in cases for k in ('kernel', 'fused', 'unfused')}
        for _ in range(7):
            for key in times:
                times[key].append(timeit(cases[key[0]][key[1]], a.iters))
        for (n_, k), ts in times.items():
            med = statistics.median(ts)
            out[f'triproj64_{k}_{n_}'] = dict(ms=round(med, 4), min=round(min(ts), 4), max=round(max(ts), 4),
                                             GBs=round(byts[k] / med / 1e6, 1), share_of_8TBs=round(byts[k] / med / 1e6 / 8000, 3),
                                             rounds=[round(t, 4) for t in ts])
        del cases

    if 'triproj64_train' in a.only:
        # tgt_triplet_attention_proj64_train_fwd: the kernel alone (pre-projected E/G rows, a preallocated Q/K/V
        # tensor), the same + the narrow E/G Linear and the allocation as ops runs it, the inference kernel for scale, and what the
        # training forward is without it: the split GEMMs + tgt_triplet_attention_fwd.  Rounds and bytes as the triproj64 block
        import ctypes
        import statistics
        from tgt_amd import _lib
        assert 33 <= N <= 64, '--only triproj64_train needs --N in 33..64'
        Bp = a.B
        L = ops.TripletLayout(C, Ht)
        ne, rows = L.used - 6 * C, Bp * n2
        maskp = torch.zeros(Bp, N, N, device=dev)
        byts = dict(kernel=rows * (3 * C + ne + 2 * C + 6 * C) * 2, fused=rows * (C + ne + 3 * C + ne + 2 * C + 6 * C) * 2,
                    infer=rows * (3 * C + ne + 2 * C) * 2, unfused=rows * (C + 6 * C + ne + 6 * C + ne + 2 * C) * 2)
        out['triproj64_train_bytes'] = dict(byts, B=Bp, N=N, H=Ht, per_row={k: v // rows for k, v in byts.items()})
        cases = {}
        for name, dtp in (('fp16', torch.float16), ('bf16', torch.bfloat16)):
            x = torch.randn(Bp, N, N, C, device=dev, dtype=dtp)
            w = (torch.randn(L.width, C, device=dev) * C ** -0.5).to(dtp)
            bias = torch.randn(L.width, device=dev).to(dtp)
            x2, wq, bq, we, be = x.view(-1, C), w[:6 * C], bias[:6 * C], w[6 * C:L.used], bias[6 * C:L.used]
            o = torch.empty(Bp, N, N, 2 * C, device=dev, dtype=dtp)
            qkv = torch.empty(Bp, N, N, 6 * C, device=dev, dtype=dtp)

            def narrow(x2=x2, we=we, be=be, dtp=dtp):
                return ops._narrow_linear(x2, we, be, dtp).view(Bp, N, N, ne)
            at_, ai_ = ops._tri_args(qkv, maskp, o, L, eg=narrow()), ops._tri_args(None, maskp, o, L, eg=narrow())
            fn, fi = _lib.lib().tgt_triplet_attention_proj64_train_fwd, _lib.lib().tgt_triplet_attention_proj64_fwd

            def kernel(at_=at_, x=x, w=w, bias=bias):
                _lib.check(fn(ctypes.byref(at_), ops._ptr(x), C, ops._ptr(w), ops._ptr(bias), ops._stream()), 'tgt_triplet_attention_proj64_train_fwd')

            def infer(ai_=ai_, x=x, w=w, bias=bias):
                _lib.check(fi(ctypes.byref(ai_), ops._ptr(x), C, ops._ptr(w), ops._ptr(bias), ops._stream()), 'tgt_triplet_attention_proj64_fwd')

            def fused(narrow=narrow, x=x, w=w, bias=bias, o=o, dtp=dtp):
                f = torch.empty(Bp, N, N, 6 * C, device=dev, dtype=dtp)
                af = ops._tri_args(f, maskp, o, L, eg=narrow())
                _lib.check(fn(ctypes.byref(af), ops._ptr(x), C, ops._ptr(w), ops._ptr(bias), ops._stream()), 'tgt_triplet_attention_proj64_train_fwd')

            def unfused(narrow=narrow, x2=x2, wq=wq, bq=bq, o=o):
                f = torch.addmm(bq, x2, wq.t()).view(Bp, N, N, 6 * C)
                au = ops._tri_args(f, maskp, o, L, eg=narrow())
                _lib.check(_lib.lib().tgt_triplet_attention_fwd(ctypes.byref(au), ops._stream()), 'tgt_triplet_attention_fwd')
            cases[name] = dict(kernel=kernel, infer=infer, fused=fused, unfused=unfused, keep=(x, w, bias, o, qkv, at_, ai_))
        times = {(n_, k): [] for n_ in cases for k in ('kernel', 'infer', 'fused', 'unfused')}
        for _ in range(7):
            for key in times:
                times[key].append(timeit(cases[key[0]][key[1]], a.iters))
        for (n_, k), ts in times.items():
            med = statistics.median(ts)
            out[f'triproj64_train_{k}_{n_}'] = dict(ms=round(med, 4), min=round(min(ts), 4), max=round(max(ts), 4),
                                                   GBs=round(byts[k] / med / 1e6, 1), share_of_8TBs=round(byts[k] / med / 1e6 / 8000, 3),
                                                   rounds=[round(t, 4) for t in ts])
        del cases

    if not a.only or 'node' in a.only:
        qkv = torch.randn(B, N, 3 * W, device=dev, dtype=dt).requires_grad_(True)
        eg = torch.randn(B, N, N, 2 * Hn, device=dev, dtype=dt).requires_grad_(True)
        gv = torch.randn(B, N, W, device=dev, dtype=dt)
        gh = torch.randn(B, N, N, Hn, device=dev, dtype=dt)
        fb = B * ((4 * N * W + 3 * n2 * Hn) * esz + n2 * 4)
        bb = B * ((7 * N * W + 5 * n2 * Hn) * esz + n2 * 4)
        t = timeit(lambda: ops.node_attention(qkv, eg, mask, Hn), a.iters)
        out['node_att_fwd'] = dict(ms=round(t, 4), GBs=round(fb / t / 1e6, 1))

        def fb_():
            v, h = ops.node_attention(qkv, eg, mask, Hn)
            torch.autograd.grad([v, h], [qkv, eg], [gv, gh])
        t2 = timeit(fb_, a.iters)
        out['node_att_bwd'] = dict(ms=round(t2 - t, 4), GBs=round(bb / (t2 - t) / 1e6, 1))
        del qkv, eg

    if not a.only or 'ln' in a.only:
        x = torch.randn(B * n2, C, device=dev, dtype=dt).requires_grad_(True)
        w, b = torch.ones(C, device=dev, requires_grad=True), torch.zeros(C, device=dev, requires_grad=True)
        g = torch.randn(B * n2, C, device=dev, dtype=dt)
        t = timeit(lambda: ops.layer_norm(x, w, b, 1e-5, dt), a.iters)
        out['ln_fwd_edge'] = dict(ms=round(t, 4), GBs=round(2 * x.numel() * esz / t / 1e6, 1))
        t2 = timeit(lambda: torch.autograd.grad(ops.layer_norm(x, w, b, 1e-5, dt), [x, w, b], g), a.iters)
        out['ln_bwd_edge'] = dict(ms=round(t2 - t, 4), GBs=round(3 * x.numel() * esz / (t2 - t) / 1e6, 1))
        res = torch.randn(B, N, N, C, device=dev, dtype=dt)
        x4 = x.detach().view(B, N, N, C)
        sc = torch.ones(B, device=dev)
        t = timeit(lambda: ops.add_layer_norm(x4, res, sc, w, b, 1e-5, dt), a.iters)
        out['add_ln_fwd_edge'] = dict(ms=round(t, 4), GBs=round(4 * x.numel() * esz / t / 1e6, 1))
        xr, rr = x4.clone().requires_grad_(True), res.clone().requires_grad_(True)
        g4 = g.view(B, N, N, C)

        def add_ln_fb():
            s_, y_ = ops.add_layer_norm(xr, rr, sc, w, b, 1e-5, dt)
            return torch.autograd.grad([s_, y_], [xr, rr], [g4, g4])
        t2 = timeit(add_ln_fb, a.iters)
        out['add_ln_bwd_edge'] = dict(ms=round(t2 - t, 4), GBs=round(5 * x.numel() * esz / (t2 - t) / 1e6, 1))
        t = timeit(lambda: ops.gelu_dropout(x4, 0.1, True), a.iters)
        out['gelu_dropout_fwd'] = dict(ms=round(t, 4), GBs=round(2 * x.numel() * esz / t / 1e6, 1))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
