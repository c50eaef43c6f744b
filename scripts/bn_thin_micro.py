"""The thinned BatchNorm kernels (PLX_BN_THIN=1) against their predecessors (=0) at the ResNet-50 shapes (bs 256),
alone, alternating off / on in one process through plx_bn_set_thin, one JSON line per case:

  stem_fwd    plx_stem_bn_pool_forward from given channel sums: finalize (a few us) + the apply/pool kernel
  stem_bwd    plx_stem_bn_pool_backward: partials pass + finalize + dx pass (a kernel trace of this script splits
              the two passes: `rocprofv3 --kernel-trace --stats -- python scripts/bn_thin_micro.py 5 2`)
  res_dx_L    plx_bn_backward from given partials with a ResBn (ReLU on, residual BatchNorm without ReLU, as the first
              block of each ResNet-50 stage runs it): finalize + the dx pass that also reduces the residual's partials.
              Not in the default list: that pass's thinned kernel missed the bar (profiles/bn_thin.md) and was
              removed, so both settings run the same kernel today; the cases are kept for a later attempt.

Every repetition uses the next of several buffer sets (>= 1 GB in total per case), so the 256 MiB Infinity Cache cannot
hold what the previous repetition touched.  Times are per-repetition device-event times; bytes are counted from the
shapes.  The bar: the gain (difference of the medians) must exceed the old kernels' own max - min.

    python scripts/bn_thin_micro.py [reps] [warmup] [case ...]
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from polyaxon_amd.ops import _native  # noqa: E402
from polyaxon_amd.ops.bn_fused import _counters, bn_backward  # noqa: E402

STEM = (256, 112, 112, 64)
RES = {"res_dx_1": (802816, 256), "res_dx_2": (200704, 512), "res_dx_3": (50176, 1024), "res_dx_4": (12544, 2048)}


def stem_case(lib, dev, st, backward):
    n, h, w, c = STEM
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    f32 = dict(dtype=torch.float32, device=dev)
    bf = dict(dtype=torch.bfloat16, device=dev)
    big, small = n * h * w * c * 2, n * oh * ow * c * 2
    nbytes = (2 * (big + small + small // 2) + big) if backward else (big + small + small // 2)
    nsets = max(2, -(-(1 << 30) // nbytes))
    gamma, beta = torch.rand(c, **f32) + 0.5, torch.randn(c, **f32) * 0.2
    cnt = _counters(dev)
    sets = []
    for _ in range(nsets):
        s = {"x": torch.randn(n, h, w, c, device=dev).to(torch.bfloat16), "y": torch.empty(n, oh, ow, c, **bf),
             "idx": torch.empty(n * oh * ow * c, dtype=torch.uint8, device=dev), "stats": torch.empty(4 * c, **f32)}
        xf = s["x"].view(-1, c).float()
        s["part"] = torch.cat([xf.sum(0), (xf * xf).sum(0)]).contiguous()  # level-1 partials [2][1][C]
        del xf
        s["l2"] = torch.empty(int(lib.plx_bn_l2_workspace(1, c)), **f32)
        s["rm"], s["rv"] = torch.zeros(c, **f32), torch.ones(c, **f32)
        if backward:
            s["dy"] = torch.randn(n, oh, ow, c, device=dev).to(torch.bfloat16)
            s["dx"] = torch.empty(n, h, w, c, **bf)
            s["dgb"], s["coef"] = torch.zeros(2 * c, **f32), torch.empty(3 * c, **f32)
            s["ws"] = torch.empty(int(lib.plx_stem_bn_pool_bwd_workspace(n, h, w, c)), **f32)
        sets.append(s)

    def fwd(s):
        rc = lib.plx_stem_bn_pool_forward(s["x"].data_ptr(), s["y"].data_ptr(), s["idx"].data_ptr(), n, h, w, c,
                                          gamma.data_ptr(), beta.data_ptr(), 1e-5, 0.1, s["rm"].data_ptr(),
                                          s["rv"].data_ptr(), s["stats"].data_ptr(), s["stats"][c:].data_ptr(),
                                          s["stats"][2 * c:].data_ptr(), s["l2"].data_ptr(), s["part"].data_ptr(), 1,
                                          cnt, st)
        assert rc == 0

    def bwd(s):
        rc = lib.plx_stem_bn_pool_backward(s["dy"].data_ptr(), s["idx"].data_ptr(), s["x"].data_ptr(),
                                           s["dx"].data_ptr(), n, h, w, c, gamma.data_ptr(), s["stats"].data_ptr(),
                                           s["stats"][c:].data_ptr(), s["stats"][2 * c:].data_ptr(),
                                           s["dgb"].data_ptr(), s["dgb"][c:].data_ptr(), s["coef"].data_ptr(),
                                           s["ws"].data_ptr(), 0, cnt, st)
        assert rc == 0

    if backward:  # the forward's idx and statistics are the backward's inputs
        for s in sets:
            fwd(s)
        torch.cuda.synchronize()
    return (bwd if backward else fwd), sets, nbytes


def res_case(lib, dev, st, m, c):
    f32 = dict(dtype=torch.float32, device=dev)
    act = m * c * 2
    nbytes = 5 * act + act // 16  # x, dy, x2 read | dx, d_residual written | the ReLU mask
    nsets = max(2, -(-(1 << 30) // nbytes))
    nblk2 = int(lib.plx_bn_dx_blocks(m, c))
    gamma, mean, invstd = torch.rand(c, **f32) + 0.5, torch.randn(c, **f32) * 0.2, torch.rand(c, **f32) + 0.5
    mean2, invstd2 = torch.randn(c, **f32) * 0.2, torch.rand(c, **f32) + 0.5
    part_in = torch.randn(2 * c, **f32)  # level-1 partials [2][1][C] of this BatchNorm
    l2 = torch.empty(int(lib.plx_bn_l2_workspace(1, c)), **f32)
    dgb, coef = torch.zeros(2 * c, **f32), torch.empty(3 * c, **f32)
    cnt = _counters(dev)
    sets = []
    for _ in range(nsets):
        s = {k: torch.randn(m, c, device=dev).to(torch.bfloat16) for k in ("x", "dy", "x2")}
        s["dx"], s["dres"] = torch.empty_like(s["x"]), torch.empty_like(s["x"])
        s["mask"] = torch.randint(0, 256, (m * c // 8,), device=dev, dtype=torch.int32).to(torch.uint8)
        s["part"] = torch.empty(2 * nblk2 * c, **f32)
        s["rb"] = _native.ResBnArgs(s["x2"].data_ptr(), None, mean2.data_ptr(), invstd2.data_ptr(), s["part"].data_ptr())
        sets.append(s)

    def run(s):
        bn_backward(x=s["x"], mask=s["mask"], dy=s["dy"], dx=s["dx"], dres=s["dres"], m=m, c=c, gamma=gamma,
                    save_mean=mean, save_invstd=invstd, dgamma=dgb, dbeta=dgb[c:], coef=coef, ext_part=part_in,
                    ext_nblk=1, workspace=l2, relu=True, accumulate=0, resbn=s["rb"], counters=cnt, stream=st)

    return run, sets, nbytes


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    cases = sys.argv[3:] or ["stem_fwd", "stem_bwd"]
    dev = torch.device("cuda", 0)
    lib = _native.lib("plx_bn")
    st = torch.cuda.current_stream().cuda_stream
    for case in cases:
        if case.startswith("stem"):
            fn, sets, nbytes = stem_case(lib, dev, st, case == "stem_bwd")
        else:
            fn, sets, nbytes = res_case(lib, dev, st, *RES[case])
        times = {"off": [], "on": []}
        for rep in range(-warmup, reps):
            for j, name in enumerate(times):
                lib.plx_bn_set_thin(j)
                s = sets[(2 * rep + j) % len(sets)]
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn(s)
                b.record()
                b.synchronize()
                if rep >= 0:
                    times[name].append(a.elapsed_time(b) * 1e3)
        lib.plx_bn_set_thin(1)
        rec = {"case": case, "reps": reps, "buffer_sets": len(sets), "mbytes": round(nbytes / 1e6, 1)}
        for name, t in times.items():
            med = statistics.median(t)
            rec[name] = {"us_median": round(med, 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1),
                         "tbs": round(nbytes / med / 1e6, 2)}
        gain = rec["off"]["us_median"] - rec["on"]["us_median"]
        spread = rec["off"]["us_max"] - rec["off"]["us_min"]
        rec.update(gain_us=round(gain, 1), off_spread_us=round(spread, 1), thin_wins=bool(gain > spread))
        print(json.dumps(rec), flush=True)
        del sets, fn
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
