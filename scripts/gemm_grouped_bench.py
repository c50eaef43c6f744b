"""Time the grouped MoE GEMM (csrc/gemm_grouped.hip) against E separate edge-kernel calls, and the gather / combine
passes against the HBM rate, on the GPU.  One JSON line per measurement.

    python scripts/gemm_grouped_bench.py [--P 32768 --E 8 --d 768 --ff 3072 --iters 50]

The separate calls get their sizes as host integers (what a host read of the router's counts would give them; the
read itself is not timed, nor is the capture it breaks).  Tables: balanced, a 2:1 skew, one empty expert.  Bytes and
FLOPs are computed from the shapes."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from polyaxon_amd.ops import gemm, moe  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak


def timed(fn, iters):
    for _ in range(5):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters * 1e3  # us


def edge(a, b, out, M, N, K, a_kmajor, b_kmajor):
    """one csrc/gemm_edge.hip call, also for shapes gemm.gemm would give to the 256-tile kernel"""
    return gemm._gemm_edge(a, b, out, M, N, K, a_kmajor, b_kmajor, 1.0, False, None)


def tables(P, E):
    r8 = lambda v: v // 8 * 8  # noqa: E731 -- the edge kernel takes multiples of 8; P is one, so the remainders are
    even = [P // E] * E
    skew = [r8(2 * P // (3 * (E // 2)))] * (E // 2) + [r8(P // (3 * (E // 2)))] * (E // 2)
    skew[0] += P - sum(skew)
    empty = [0] + [r8(P // (E - 1))] * (E - 1)
    empty[1] += P - sum(empty)
    return {"balanced": even, "skew_2_1": skew, "one_empty": empty}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=32768)
    ap.add_argument("--E", type=int, default=8)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--ff", type=int, default=3072)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    P, E, bf = a.P, a.E, torch.bfloat16
    x = torch.randn(P, a.d, device=dev).to(bf)
    h = torch.randn(P, a.ff, device=dev).to(bf)
    w = torch.randn(E, a.ff, a.d, device=dev).to(bf)
    flops = 2.0 * P * a.ff * a.d
    for name, counts in tables(P, E).items():
        offs = torch.tensor([0] + counts).cumsum(0).to(torch.int32).to(dev)
        o = offs.tolist()
        live = [e for e in range(E) if counts[e]]  # the edge kernel takes M > 0 and multiples of 8 (these tables are)
        out = torch.empty(P, a.ff, dtype=bf, device=dev)
        dx = torch.empty(P, a.d, dtype=bf, device=dev)
        dw = torch.empty(E, a.ff, a.d, dtype=bf, device=dev)
        seg = [slice(o[e], o[e + 1]) for e in range(E)]
        cases = {
            "rows_fwd": (lambda: gemm.grouped_rows(x, w, offs, a.ff, a.d, True, out=out),
                         lambda: [edge(x[seg[e]], w[e], out[seg[e]], counts[e], a.ff, a.d, True, True) for e in live]),
            "rows_dgrad": (lambda: gemm.grouped_rows(h, w, offs, a.d, a.ff, False, out=dx),
                           lambda: [edge(h[seg[e]], w[e], dx[seg[e]], counts[e], a.d, a.ff, True, False) for e in live]),
            "reduce_wgrad": (lambda: gemm.grouped_wgrad(h, x, offs, E, out=dw),
                             lambda: [edge(h[seg[e]], x[seg[e]], dw[e], a.ff, a.d, counts[e], False, False)
                                      for e in live]),
        }
        for case, (grouped, separate) in cases.items():
            tg, ts = timed(grouped, a.iters), timed(separate, a.iters)
            print(json.dumps({"case": case, "table": name, "P": P, "E": E, "d": a.d, "ff": a.ff,
                              "grouped_us": round(tg, 1), "separate_us": round(ts, 1), "ratio": round(ts / tg, 3),
                              "grouped_tflops": round(flops / tg / 1e6, 1)}), flush=True)
    # the routing passes: T tokens, k choices each
    T = P // a.k
    ids = torch.stack([torch.randperm(E, device=dev)[:a.k] for _ in range(64)]).repeat(T // 64, 1)
    offs, token_of, slot_of = moe.plan(ids, E)
    gates = torch.rand(T, a.k, device=dev)
    xt = torch.randn(T, a.d, device=dev).to(bf)
    for case, fn, nbytes in (
            ("gather", lambda: moe._gather_rows(xt, token_of, None, P), 2 * P * a.d * 2 + 4 * P),
            ("combine", lambda: moe._combine_rows(x, slot_of, gates), (P + T) * a.d * 2 + 8 * P)):
        t = timed(fn, a.iters)
        print(json.dumps({"case": case, "P": P, "T": T, "d": a.d, "us": round(t, 1), "bytes": nbytes,
                          "hbm_fraction": round(nbytes / (t * 1e-6) / HBM_BYTES_PER_S, 3)}), flush=True)
    print(json.dumps({"case": "plan", "P": P, "E": E, "us": round(timed(lambda: moe.plan(ids, E), a.iters), 1)}))


if __name__ == "__main__":
    main()
