"""bn3's apply + residual + ReLU and the next block's conv1 of the ResNet-50 bottlenecks (bs 256): today's two kernels
(the apply pass, then plx_gemm_nt reading its output) against the fused GEMM that produces the block output itself
(plx_gemm_nt_bnapply), alternating, one JSON line per shape.  The first two shapes are the engaged ones (layers 1 and
2); the third (layer 3, two N tiles per row panel) is the control that the shape rule keeps on the two kernels.

Both GEMMs carry the channel-stats epilogue, as in the training step.  Every repetition uses the next of several buffer
sets (>= 1 GB in total per shape), so the 256 MiB Infinity Cache cannot hold what the previous repetition touched.
Times are per-repetition device-event times; bytes are counted from the shapes (activations, mask and the weight once).

    python scripts/bn_apply_conv1_micro.py [reps] [warmup] [rsb]
"""
import json
import statistics
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))

from polyaxon_amd.ops import _native  # noqa: E402
from polyaxon_amd.ops.conv1x1 import nt_stats_rows  # noqa: E402

SHAPES = [(802816, 256, 64), (200704, 512, 128), (50176, 1024, 256)]  # (M, K, N) of conv1's forward
HBM_TBS = 6.3  # achievable HBM bandwidth (measuring-on-mi355x)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    with_rsb = len(sys.argv) > 3 and sys.argv[3] == "rsb"
    dev = torch.device("cuda", 0)
    conv, bn = _native.lib("plx_conv"), _native.lib("plx_bn")
    st = torch.cuda.current_stream().cuda_stream
    f32 = dict(dtype=torch.float32, device=dev)
    for m, k, n in SHAPES:
        act, y = m * k * 2, m * n * 2
        common = 2 * act + act + act // 16 + y + n * k * 2      # x, res read | out, mask written | y written, W
        nbytes = {"two_kernels": common + act, "fused": common}  # the GEMM's re-read of out
        nsets = max(2, -(-(1 << 30) // nbytes["two_kernels"]))
        sb = torch.cat([torch.rand(k, **f32) + 0.5, 0.2 * torch.randn(k, **f32)]).contiguous()
        rsb = torch.cat([torch.rand(k, **f32) + 0.5, 0.2 * torch.randn(k, **f32)]).contiguous() if with_rsb else None
        rsp = rsb.data_ptr() if with_rsb else None
        w = (torch.randn(n, k, device=dev) / k ** 0.5).to(torch.bfloat16)
        nblk = -(-m // nt_stats_rows(n))
        stats = torch.empty(2 * nblk * n, **f32)
        sets = []
        for _ in range(nsets):
            s = {name: torch.randn(m, k, device=dev).to(torch.bfloat16) for name in ("x", "res")}
            s["out"] = torch.empty(m, k, device=dev, dtype=torch.bfloat16)
            s["mask"] = torch.empty(m * k // 8, device=dev, dtype=torch.uint8)
            s["y"] = torch.empty(m, n, device=dev, dtype=torch.bfloat16)
            sets.append(s)

        def two_kernels(s):
            rc = bn.plx_bn_apply_res_relu(s["x"].data_ptr(), s["res"].data_ptr(), s["out"].data_ptr(), m, k,
                                          sb.data_ptr(), s["mask"].data_ptr(), rsp, st)
            assert rc == 0
            rc = conv.plx_gemm_nt(s["out"].data_ptr(), w.data_ptr(), s["y"].data_ptr(), m, n, k, k, k, n,
                                  stats.data_ptr(), None, 0, None, None, st)
            assert rc == 0

        def fused(s):
            rc = conv.plx_gemm_nt_bnapply(s["x"].data_ptr(), s["res"].data_ptr(), sb.data_ptr(), rsp,
                                          s["out"].data_ptr(), s["mask"].data_ptr(), w.data_ptr(), s["y"].data_ptr(), m,
                                          n, k, k, n, stats.data_ptr(), st)
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
        rec = {"shape": f"M{m} K{k} N{n}", "rsb": with_rsb, "reps": reps, "buffer_sets": nsets}
        for name, t in times.items():
            med = statistics.median(t)
            rec[name] = {"mbytes": round(nbytes[name] / 1e6, 1), "us_median": round(med, 1), "us_min": round(min(t), 1),
                         "us_max": round(max(t), 1), "tbs": round(nbytes[name] / med / 1e6, 2),
                         "of_hbm": round(nbytes[name] / med / 1e6 / HBM_TBS, 2)}
        gain = rec["two_kernels"]["us_median"] - rec["fused"]["us_median"]
        spread = rec["two_kernels"]["us_max"] - rec["two_kernels"]["us_min"]  # the two-kernel spread the gain must beat
        rec.update(gain_us=round(gain, 1), two_kernel_spread_us=round(spread, 1), fused_wins=bool(gain > spread))
        print(json.dumps(rec), flush=True)
        del sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
