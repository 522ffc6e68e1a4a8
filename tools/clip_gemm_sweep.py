"""Sweep forced GEMM plans for the text tower's four linears against the planner's own choice.

python tools/clip_gemm_sweep.py > profiles/clip_gemm_sweep.log

The q|k|v, out-proj, c_fc (GELU) and c_proj GEMMs of a width-1024 block at M = 77 (B = 1) and M = 616 (B = 8): the
planner's plan, then every built 64 / 128-row tile with 1 ... 16 K slices.  Each plan runs as one captured graph of
24+ launches over distinct weight copies (>= 300 MB in all, so the weights come from HBM as in the tower, not from
the caches), replayed 3 times; one JSON line per plan with us per launch, and the best forced plan per GEMM.
"""
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tair_amd import _lib  # noqa: E402

L = _lib.lib()
dev = "cuda"
part = torch.empty(6 * 640 * 4096 * 4, device=dev)
sem = torch.zeros(1 << 16, device=dev, dtype=torch.int32)


def run(M, N, K, act, res, force, copies):
    A = torch.randn(M, K, device=dev).to(torch.bfloat16)
    Ws = [(torch.randn(N, K, device=dev) / K ** 0.5).to(torch.bfloat16) for _ in range(copies)]
    bias = torch.randn(N, device=dev)
    out = torch.zeros(M, 2 * N if res else N, device=dev, dtype=torch.bfloat16)
    descs = []
    for W in Ws:
        d = _lib.GemmDesc()
        d.M, d.N, d.K, d.amode, d.alpha, d.act, d.rows_per_b = M, N, K, 0, 1.0, act, 1
        d.A, d.lda, d.Wt, d.ldw, d.bias = A.data_ptr(), K, W.data_ptr(), K, bias.data_ptr()
        d.out, d.ldo = out.data_ptr(), out.stride(0)
        if res:
            d.res, d.ld_res, d.res_lo, d.out_lo = out.data_ptr(), 2 * N, N, N
        d.partial, d.partial_cap = part.data_ptr(), part.numel()
        d.tile_sem, d.sem_cap = sem.data_ptr(), sem.numel()
        d.force_bm, d.force_bn, d.force_splits = force
        descs.append(d)
    o = [ctypes.c_int() for _ in range(4)]
    if L.tair_k_gemm_plan(ctypes.byref(descs[0]), *[ctypes.byref(x) for x in o]) != 0:
        return None, None
    plan = [x.value for x in o]

    def launch_all():
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for d in descs:
            assert L.tair_k_gemm(ctypes.byref(d), st) == 0, L.tair_last_error()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch_all()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch_all()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (3 * copies), plan


SHAPES = [("qkv", 3072, 1024, 0, False), ("out", 1024, 1024, 0, True), ("fc", 4096, 1024, 3, False),
          ("proj", 1024, 4096, 0, True)]
for M in (77, 616):
    for name, N, K, act, res in SHAPES:
        copies = max(24, int(3e8 // (N * K * 2)))
        cands = [(0, 0, 0)] + [(bm, bn, s) for bm in (64, 128) for bn in (64, 128) for s in (1, 2, 3, 4, 6, 8, 12, 16)
                               if s <= K // 64 and (M < 200 or s <= 4)]
        best = None
        for f in cands:
            us, plan = run(M, N, K, act, res, f, copies)
            if us is None:
                continue
            print(json.dumps({"M": M, "gemm": name, "force": f, "plan": plan, "us": round(us, 2)}), flush=True)
            if f != (0, 0, 0) and (best is None or us < best[0]):
                best = (us, f)
        print(json.dumps({"M": M, "gemm": name, "best": best}), flush=True)
n = ctypes.c_int(0)
L.tair_fault_count(1, ctypes.byref(n))
print("faults", n.value)
