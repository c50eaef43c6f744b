"""The BatchNorm-dx data gradient and the weight gradient of ResNet-50 layer 1's Cin = 64 -> Cout = 256 1x1 convolutions
(bs 256: M = 802816, K = 256, N = 64), alone on one stream, alternating:

  (a) plx_gemm_nt_bndx (stores dy) + plx_gemm_tn (reads dy and x_in back, float atomics), back to back
  (b) plx_gemm_nt_bndx_wgrad: one persistent kernel, dy never stored
  (c) plx_gemm_nt_bndx alone -- what the data-gradient chain's stream pays today

with and without the epilogue addend.  All three carry the BnBwd epilogue.  Every repetition uses the next of several
buffer sets (>= 1 GB in total), so the 256 MiB Infinity Cache cannot hold what the previous repetition touched.  Times
are per-repetition device-event times; bytes are counted from the shapes.  One JSON line per addend setting.

    python scripts/dgrad_wgrad_micro.py [reps] [warmup]
"""
import ctypes
import json
import statistics
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))

from polyaxon_amd.ops import _native  # noqa: E402

M, K, N = 802816, 256, 64
HBM_TBS = 6.3  # achievable HBM bandwidth (measuring-on-mi355x)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    dev = torch.device("cuda", 0)
    conv = _native.lib("plx_conv")
    st = torch.cuda.current_stream().cuda_stream
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    f32 = dict(dtype=torch.float32, device=dev)
    act, out = M * K * 2, M * N * 2
    coef = torch.cat([torch.rand(K, **f32) + 0.5, 0.3 * torch.randn(K, **f32), 0.1 * torch.randn(K, **f32)])
    mean2, invstd2 = 0.1 * torch.randn(N, **f32), torch.rand(N, **f32) + 0.5
    wt = (torch.randn(N, K, device=dev) / K ** 0.5).to(torch.bfloat16)
    nblk2 = -(-M // 256)
    part2 = torch.empty(2 * nblk2 * N, **f32)
    dw = torch.zeros(K, N, **f32)
    ws = torch.empty(conv.plx_gemm_tn_workspace(M, K, N, cus), **f32)
    nsets = 2
    sets = []
    for _ in range(nsets):
        s = {name: torch.randn(M, c, device=dev).to(torch.bfloat16)
             for name, c in (("g", K), ("x", K), ("x2", N), ("x_in", N), ("add", N))}
        s["mask"] = torch.randint(0, 256, (M * K // 8,), device=dev, dtype=torch.uint8)
        s["mask2"] = torch.randint(0, 256, (M * N // 8,), device=dev, dtype=torch.uint8)
        s["dy"] = torch.empty(M, K, device=dev, dtype=torch.bfloat16)
        s["c"] = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        s["bnr"] = _native.GemmBnBwdArgs(s["x2"].data_ptr(), s["mask2"].data_ptr(), mean2.data_ptr(),
                                         invstd2.data_ptr(), part2.data_ptr(), nblk2, 0)
        sets.append(s)
    for with_add in (False, True):
        # g, x, mask | C written, the BnBwd epilogue's x and mask (| the addend) | the weight
        base = 2 * act + act // 16 + out + out + out // 16 + (out if with_add else 0) + N * K * 2
        nbytes = {"dgrad_then_wgrad": base + act + act + out, "fused": base + out, "dgrad_alone": base + act}

        def dgrad(s):
            rc = conv.plx_gemm_nt_bndx(s["g"].data_ptr(), s["x"].data_ptr(), s["mask"].data_ptr(), coef.data_ptr(),
                                       s["dy"].data_ptr(), wt.data_ptr(), s["c"].data_ptr(), M, N, K, K, N,
                                       s["add"].data_ptr() if with_add else None, N if with_add else 0, None,
                                       ctypes.addressof(s["bnr"]), st)
            assert rc == 0

        def dgrad_then_wgrad(s):
            dgrad(s)
            rc = conv.plx_gemm_tn(s["dy"].data_ptr(), s["x_in"].data_ptr(), dw.data_ptr(), ws.data_ptr(), M, K, N, K, N,
                                  N, cus, 1, st)
            assert rc == 0

        def fused(s):
            rc = conv.plx_gemm_nt_bndx_wgrad(s["g"].data_ptr(), s["x"].data_ptr(), s["mask"].data_ptr(),
                                             coef.data_ptr(), s["dy"].data_ptr(), wt.data_ptr(), s["c"].data_ptr(), M, N,
                                             K, K, N, s["add"].data_ptr() if with_add else None, N if with_add else 0,
                                             None, ctypes.addressof(s["bnr"]), s["x_in"].data_ptr(), dw.data_ptr(), N, 0,
                                             st)
            assert rc == 0

        variants = {"dgrad_then_wgrad": dgrad_then_wgrad, "fused": fused, "dgrad_alone": dgrad}
        times = {name: [] for name in variants}
        for rep in range(-warmup, reps):
            for j, (name, fn) in enumerate(variants.items()):
                s = sets[(3 * rep + j) % nsets]
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn(s)
                b.record()
                b.synchronize()
                if rep >= 0:
                    times[name].append(a.elapsed_time(b) * 1e3)
        rec = {"shape": f"M{M} K{K} N{N}", "add": with_add, "reps": reps, "buffer_sets": nsets}
        for name, t in times.items():
            med = statistics.median(t)
            rec[name] = {"mbytes": round(nbytes[name] / 1e6, 1), "us_median": round(med, 1), "us_min": round(min(t), 1),
                         "us_max": round(max(t), 1), "tbs": round(nbytes[name] / med / 1e6, 2),
                         "of_hbm": round(nbytes[name] / med / 1e6 / HBM_TBS, 2)}
        a_, b_, c_ = rec["dgrad_then_wgrad"], rec["fused"], rec["dgrad_alone"]
        rec["bar1_pair_minus_fused_us"] = round(a_["us_median"] - b_["us_median"], 1)
        rec["bar1_pair_spread_us"] = round(a_["us_max"] - a_["us_min"], 1)
        rec["bar1"] = bool(a_["us_median"] - b_["us_median"] > a_["us_max"] - a_["us_min"])
        rec["bar2_alone_minus_fused_us"] = round(c_["us_median"] - b_["us_median"], 1)
        rec["bar2_alone_spread_us"] = round(c_["us_max"] - c_["us_min"], 1)
        rec["bar2"] = bool(c_["us_median"] - b_["us_median"] > c_["us_max"] - c_["us_min"])
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
