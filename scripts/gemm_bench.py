"""Time the 256x256 MFMA GEMM (csrc/gemm256.hip) against torch (hipBLASLt) on the LM linears' shapes.

    python scripts/gemm_bench.py [--models gpt2,llama] [--reps 20] [--waves 8,4]

One JSON line per (model, linear, pass): ms and TFLOP/s of both, and the max |diff| relative to the output scale.
``--waves 8,4`` times both kernel schedules (ops/gemm.py FORCE_SCHEDULE) in the same process, interleaved per shape;
``--waves table`` times the per-shape table (ops/gemm.py SCHEDULE).
Passes: fwd (x . W^T), dgrad (dy . W), wgrad (dy^T . x, K = tokens).

``--models ragged`` (or any name of ``RAGGED``) times the shapes only the edge-tile kernel (csrc/gemm_edge.hip) takes:
``gemm.gemm`` runs it for them.  ``--edge`` also times that kernel on each 256-multiple shape, beside gemm256
(``edge_ms``, ``edge_vs_native``).  ``--rounds R`` alternates R timings of torch and of each kernel and reports the
medians (``*_spread``: max / min over the rounds).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from polyaxon_amd.ops import gemm  # noqa: E402

# (model, tokens, [(linear, in, out)])
MODELS = {
    "gpt2": (16 * 1024, [("qkv", 768, 2304), ("proj", 768, 768), ("up", 768, 3072), ("down", 3072, 768),
                        ("head", 768, 50432)]),
    "llama": (4096, [("qkv", 4096, 6144), ("proj", 4096, 4096), ("up", 4096, 28672), ("down", 14336, 4096)]),
}
# shapes with a dimension that is not a multiple of 256 (or K of 64): another token count, d_model 1600 (GPT-2 XL) and
# 896, the tiny test configs, the ResNet-50 head (its three roles are 256 x 1000 x 2048 and its transposes)
RAGGED = {
    "gpt2_12x1000": (12 * 1000, MODELS["gpt2"][1]),
    "d1600": (4096, [("qkv", 1600, 4800), ("proj", 1600, 1600), ("up", 1600, 6400), ("down", 6400, 1600)]),
    "d896": (4096, [("qkv", 896, 2688), ("proj", 896, 896), ("up", 896, 3584), ("down", 3584, 896)]),
    "tiny": (8 * 64, [("qkv", 64, 192), ("up", 64, 128), ("down", 128, 64)]),
    "resnet_head": (256, [("fc", 2048, 1000)]),
}


def timed(fn, reps):
    for _ in range(3):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="gpt2,llama")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--waves", default="8")
    ap.add_argument("--groups", default="", help="tile-group sizes to A/B (plx_gemm256_set_group), e.g. 1,4,8")
    ap.add_argument("--cold", type=int, default=0,
                    help="rotate each call through this many operand copies (>= 1 GB in total defeats the 256 MB "
                         "infinity cache: the operands stream from HBM as in a training step)")
    ap.add_argument("--edge", action="store_true", help="also time the edge-tile kernel on 256-multiple shapes")
    ap.add_argument("--rounds", type=int, default=1, help="alternating timing rounds of torch and each kernel")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    tot = {"torch": 0.0}
    waves = [0 if w == "table" else int(w) for w in args.waves.split(",")]
    groups = [int(g) for g in args.groups.split(",")] if args.groups else [0]
    names = [n for m in args.models.split(",") for n in (RAGGED if m == "ragged" else [m])]
    lib = gemm._native.lib("plx_gemm") if any(n in MODELS for n in names) else None
    for model in names:
        T, linears = MODELS[model] if model in MODELS else RAGGED[model]
        for name, fin, fout in linears:
            x = torch.randn(T, fin, device=dev).to(torch.bfloat16)
            w = (torch.randn(fout, fin, device=dev) * 0.02).to(torch.bfloat16)
            dy = torch.randn(T, fout, device=dev).to(torch.bfloat16)
            n = max(1, args.cold)
            xs, ws, dys = [x] + [x.clone() for _ in range(n - 1)], [w] + [w.clone() for _ in range(n - 1)], \
                [dy] + [dy.clone() for _ in range(n - 1)]
            it = {"i": 0}

            def nxt():  # the operand copy of this call (round robin)
                it["i"] = (it["i"] + 1) % n
                return xs[it["i"]], ws[it["i"]], dys[it["i"]]

            def op(f):
                def run():
                    a_, b_, c_ = nxt()
                    return f(a_, b_, c_)
                return run
            # the kernel itself (gemm.gemm), not gemm.forward / dgrad / wgrad: those dispatch through ``auto``, which
            # sends the shapes outside ops/gemm.py's table to hipBLASLt (round 4's per-shape numbers for the forward
            # and most data gradients were hipBLASLt against itself)
            cases = [
                ("fwd", T, fout, fin, op(lambda x, w, dy: gemm.gemm(x, w, T, fout, fin, True, True)),
                 op(lambda x, w, dy: x @ w.t())),
                ("dgrad", T, fin, fout, op(lambda x, w, dy: gemm.gemm(dy, w, T, fin, fout, True, False)),
                 op(lambda x, w, dy: dy @ w)),
                ("wgrad", fout, fin, T, op(lambda x, w, dy: gemm.gemm(dy, x, fout, fin, T, False, False)),
                 op(lambda x, w, dy: dy.t() @ x)),
            ]
            lay = {"fwd": (True, True), "dgrad": (True, False), "wgrad": (False, False)}
            for pas, M, N, K, nat, ref in cases:
                b = ref()
                fl = 2.0 * M * N * K
                full = gemm.supported(M, N, K)  # gemm.gemm runs gemm256 (else the edge-tile kernel)
                rec = {"model": model, "linear": name, "pass": pas, "M": M, "N": N, "K": K,
                       "kernel": "gemm256" if full else "gemm_edge",
                       "splits": gemm._native.size("plx_gemm", "plx_gemm256_splits", M, N, K) if full
                       else gemm._native.size("plx_gemm_edge", "plx_gemm_edge_splits", M, N, K)}
                # (suffix, schedule, group, callable): every kernel variant timed on this shape
                runs = [(("" if len(waves) == 1 else f"_w{wv}") + (f"_g{grp}" if grp else ""), wv, grp, nat)
                        for grp in groups for wv in waves] if full else [("", 0, 0, nat)]
                if full and args.edge:
                    eo = torch.empty(M, N, dtype=torch.bfloat16, device=dev)

                    def edge_run(pas=pas, M=M, N=N, K=K, eo=eo):
                        x_, w_, dy_ = nxt()
                        a_, b_ = {"fwd": (x_, w_), "dgrad": (dy_, w_), "wgrad": (dy_, x_)}[pas]
                        return gemm._gemm_edge(a_, b_, eo, M, N, K, *lay[pas], 1.0, False, None)
                    runs.append(("_edge", 0, 0, edge_run))
                tts, tns = [], {sfx: [] for sfx, *_ in runs}
                for _ in range(max(1, args.rounds)):  # alternating: torch, then each kernel variant
                    tts.append(timed(ref, args.reps))
                    for sfx, wv, grp, fn in runs:
                        gemm.FORCE_SCHEDULE = wv
                        if grp:
                            lib.plx_gemm256_set_group(grp)
                        tns[sfx].append(timed(fn, args.reps))
                tt = sorted(tts)[len(tts) // 2]
                tot["torch"] += tt
                rec.update({"torch_ms": round(tt, 4), "torch_tflops": round(fl / tt / 1e9, 1),
                            "torch_spread": round(max(tts) / min(tts), 3)})
                for sfx, wv, grp, fn in runs:
                    gemm.FORCE_SCHEDULE = wv
                    a = fn()
                    err = ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-6)).item()
                    tn = sorted(tns[sfx])[len(tns[sfx]) // 2]
                    key = "edge" if sfx == "_edge" else "native" + sfx
                    tot[key] = tot.get(key, 0.0) + tn
                    rec.update({f"{key}_ms": round(tn, 4), f"{key}_tflops": round(fl / tn / 1e9, 1),
                                f"{key}_spread": round(max(tns[sfx]) / min(tns[sfx]), 3),
                                ("edge_vs_torch" if sfx == "_edge" else f"speedup{sfx}"): round(tt / tn, 3),
                                f"rel_err{'_edge' if sfx == '_edge' else sfx}": round(err, 5)})
                if full and args.edge:
                    rec["edge_vs_native"] = round(rec["native" + runs[0][0] + "_ms"] / rec["edge_ms"], 3)
                print(json.dumps(rec), flush=True)
            del x, w, dy, xs, ws, dys
    gemm.FORCE_SCHEDULE = 0
    print(json.dumps({f"total_{k}_ms": round(v, 3) for k, v in tot.items()}))


if __name__ == "__main__":
    main()
