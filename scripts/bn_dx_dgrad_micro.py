"""bn3's backward dx + conv3's data gradient of the ResNet-50 bottlenecks (bs 256): today's two kernels (the
BatchNorm dx pass, then plx_gemm_nt reading its output) against the fused GEMM that produces dx itself
(plx_gemm_nt_bndx), alternating, one JSON line per shape.

Both variants start from the same per-block partials and run the same reduce / finalize launch first, as the training
step does (plx_bn_backward from external partials, with and without its dx pass), and both GEMMs carry the BnBwd
epilogue that serves bn2.  Every repetition uses the next of several buffer sets (>= 1 GB in total per shape), so the
256 MiB Infinity Cache cannot hold what the previous repetition touched.  Times are per-repetition device-event
times; bytes are counted from the shapes (activations, masks and the weight once).

    python scripts/bn_dx_dgrad_micro.py [reps] [warmup]
"""
import ctypes
import json
import statistics
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))

from polyaxon_amd.ops import _native  # noqa: E402
from polyaxon_amd.ops.bn_fused import _counters, bn_backward  # noqa: E402
from polyaxon_amd.ops.conv1x1 import nt_stats_rows  # noqa: E402

SHAPES = [(802816, 256, 64), (200704, 512, 128), (50176, 1024, 256), (12544, 2048, 512)]  # (M, K, N) of conv3's dgrad
HBM_TBS = 6.3  # achievable HBM bandwidth (measuring-on-mi355x)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    dev = torch.device("cuda", 0)
    conv = _native.lib("plx_conv")
    st = torch.cuda.current_stream().cuda_stream
    cnt = _counters(dev)
    f32 = dict(dtype=torch.float32, device=dev)
    for m, k, n in SHAPES:
        act, out = m * k * 2, m * n * 2
        common = 2 * act + act // 16 + act + out + out // 16 + out + n * k * 2  # g, x, mask, dy written | y2, mask2, C, W
        nbytes = {"two_kernels": common + act, "fused": common}
        nsets = max(2, -(-(1 << 30) // nbytes["two_kernels"]))
        gamma, mean, invstd = torch.rand(k, **f32) + 0.5, 0.1 * torch.randn(k, **f32), torch.rand(k, **f32) + 0.5
        mean2, invstd2 = 0.1 * torch.randn(n, **f32), torch.rand(n, **f32) + 0.5
        wt = (torch.randn(n, k, device=dev) / k ** 0.5).to(torch.bfloat16)
        nblk = -(-m // 128)
        part = torch.randn(2 * nblk * k, **f32)
        l2 = torch.empty(_native.size("plx_bn", "plx_bn_l2_workspace", nblk, k), **f32)
        dgb, coef = torch.empty(2 * k, **f32), torch.empty(3 * k, **f32)
        nblk2 = -(-m // nt_stats_rows(n))
        part2 = torch.empty(2 * nblk2 * n, **f32)
        sets = []
        for _ in range(nsets):
            s = {name: torch.randn(m, c, device=dev).to(torch.bfloat16) for name, c in (("g", k), ("x", k), ("x2", n))}
            s["mask"] = torch.randint(0, 256, (m * k // 8,), device=dev, dtype=torch.uint8)
            s["mask2"] = torch.randint(0, 256, (m * n // 8,), device=dev, dtype=torch.uint8)
            s["dy"] = torch.empty(m, k, device=dev, dtype=torch.bfloat16)
            s["c"] = torch.empty(m, n, device=dev, dtype=torch.bfloat16)
            s["bnr"] = _native.GemmBnBwdArgs(s["x2"].data_ptr(), s["mask2"].data_ptr(), mean2.data_ptr(),
                                             invstd2.data_ptr(), part2.data_ptr(), nblk2, 0)
            sets.append(s)

        def two_kernels(s):
            bn_backward(x=s["x"], mask=s["mask"], dy=s["g"], dx=s["dy"], m=m, c=k, gamma=gamma, save_mean=mean,
                        save_invstd=invstd, dgamma=dgb, dbeta=dgb[k:], coef=coef, ext_part=part, ext_nblk=nblk,
                        workspace=l2, relu=True, accumulate=0, counters=cnt, stream=st)
            rc = conv.plx_gemm_nt(s["dy"].data_ptr(), wt.data_ptr(), s["c"].data_ptr(), m, n, k, k, k, n, None, None,
                                  0, None, ctypes.addressof(s["bnr"]), st)
            assert rc == 0

        def fused(s):
            bn_backward(x=s["x"], mask=s["mask"], dy=s["g"], dx=None, m=m, c=k, gamma=gamma, save_mean=mean,
                        save_invstd=invstd, dgamma=dgb, dbeta=dgb[k:], coef=coef, ext_part=part, ext_nblk=nblk,
                        workspace=l2, relu=True, accumulate=0, counters=cnt, stream=st)
            rc = conv.plx_gemm_nt_bndx(s["g"].data_ptr(), s["x"].data_ptr(), s["mask"].data_ptr(), coef.data_ptr(),
                                       s["dy"].data_ptr(), wt.data_ptr(), s["c"].data_ptr(), m, n, k, k, n, None, 0, None,
                                       ctypes.addressof(s["bnr"]), st)
            assert rc == 0

        variants = {"two_kernels": two_kernels, "fused": fused}
        times = {name: [] for name in variants}
        for rep in range(-warmup, reps):
            for j, (name, fn) in enumerate(variants.items()):
                s = sets[(2 * rep + j) % nsets]
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn(s)
                b.record()
                b.synchronize()
                if rep >= 0:
                    times[name].append(a.elapsed_time(b) * 1e3)
        rec = {"shape": f"M{m} K{k} N{n}", "reps": reps, "buffer_sets": nsets}
        for name, t in times.items():
            med = statistics.median(t)
            rec[name] = {"mbytes": round(nbytes[name] / 1e6, 1), "us_median": round(med, 1), "us_min": round(min(t), 1),
                         "us_max": round(max(t), 1), "tbs": round(nbytes[name] / med / 1e6, 2),
                         "of_hbm": round(nbytes[name] / med / 1e6 / HBM_TBS, 2)}
        gain = rec["two_kernels"]["us_median"] - rec["fused"]["us_median"]
        spread = max(r["us_max"] - r["us_min"] for r in (rec["two_kernels"], rec["fused"]))
        rec.update(gain_us=round(gain, 1), spread_us=round(spread, 1), fused_wins=bool(gain > spread))
        print(json.dumps(rec), flush=True)
        del sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
