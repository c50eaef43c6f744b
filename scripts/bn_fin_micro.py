"""The single-workgroup BatchNorm reduce + finalize (PLX_BN_FIN_SINGLE=1) against the ticket kernels (=0), alone, at
partial-row counts and channel counts around those of ResNet-50 (bs 256), alternating off / on in one process through
plx_bn_set_fin_single, one JSON line per (nblk, C, direction):

    python scripts/bn_fin_micro.py [reps] [warmup] [launches]

A call is plx_bn_forward / plx_bn_backward from given level-1 partials (ext_part) with no apply / dx pass: exactly the
reduce + finalize launch.  These launches take a few microseconds, less than a pair of events resolves and less than
the host needs to issue one, so per setting `launches` (default 16) calls, each on the next of 8 sets of partials and
outputs, are captured into a graph once; a repetition replays that graph between two device events and its time is
divided by `launches`: the figure is the stream's cost per launch, start to start, as the captured training step
pays it.  Above 512 rows both settings run the ticket kernels (the single-workgroup kernels hold at
most 512 rows in flight), so those lines measure the ticket kernels twice and show the noise.  The bar: the gain
(difference of the medians) must exceed the off runs' own max - min.
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from polyaxon_amd.ops import _native  # noqa: E402
from polyaxon_amd.ops.bn_fused import bn_backward, bn_forward  # noqa: E402

NBLKS = (98, 392, 512, 784, 1568, 3136, 6272)
CS = (64, 256, 512, 1024, 2048)
NSETS = 8


def make_case(lib, dev, nblk, c, backward, cnt):
    f32 = dict(dtype=torch.float32, device=dev)
    gamma, beta = torch.rand(c, **f32) + 0.5, torch.randn(c, **f32) * 0.2
    mean, invstd = torch.randn(c, **f32) * 0.2, torch.rand(c, **f32) + 0.5
    sets = []
    for _ in range(NSETS):
        s = {"part": torch.cat([torch.randn(nblk, c, **f32), torch.rand(nblk, c, **f32) + 1.0]).contiguous(),
             "l2": torch.empty(int(lib.plx_bn_l2_workspace(nblk, c)), **f32), "stats": torch.empty(4 * c, **f32),
             "run": torch.zeros(2 * c, **f32), "dgb": torch.zeros(2 * c, **f32), "coef": torch.empty(3 * c, **f32)}
        sets.append(s)

    def fwd(s):
        bn_forward(x=None, m=nblk * 128, c=c, gamma=gamma, beta=beta, eps=1e-5, momentum=0.1, save_mean=s["stats"],
                   save_invstd=s["stats"][c:], scale_bias=s["stats"][2 * c:], workspace=s["l2"],
                   running_mean=s["run"], running_var=s["run"][c:], ext_part=s["part"], ext_nblk=nblk, counters=cnt)

    def bwd(s):
        bn_backward(x=None, dy=None, m=nblk * 128, c=c, gamma=gamma, save_mean=mean, save_invstd=invstd,
                    dgamma=s["dgb"], dbeta=s["dgb"][c:], coef=s["coef"], workspace=s["l2"], ext_part=s["part"],
                    ext_nblk=nblk, accumulate=1, counters=cnt)

    return (bwd if backward else fwd), sets


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    launches = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    dev = torch.device("cuda", 0)
    lib = _native.lib("plx_bn")
    cnt = torch.zeros(64, dtype=torch.int32, device=dev)
    for nblk in NBLKS:
        for c in CS:
            for backward in (False, True):
                fn, sets = make_case(lib, dev, nblk, c, backward, cnt)
                times = {"off": [], "on": []}
                graphs = []
                for j in range(2):  # the host picks the kernels at capture time
                    lib.plx_bn_set_fin_single(j)
                    fn(sets[0])
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        for k in range(launches):
                            fn(sets[k % NSETS])
                    graphs.append(g)
                for rep in range(-warmup, reps):
                    for j, name in enumerate(times):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        graphs[j].replay()
                        b.record()
                        b.synchronize()
                        if rep >= 0:
                            times[name].append(a.elapsed_time(b) * 1e3 / launches)
                lib.plx_bn_set_fin_single(1)
                rec = {"nblk": nblk, "C": c, "dir": "bwd" if backward else "fwd", "reps": reps, "launches": launches,
                       "path_on": int(lib.plx_bn_fin_path(nblk, c))}
                for name, t in times.items():
                    rec[name] = {"us_median": round(statistics.median(t), 2), "us_min": round(min(t), 2),
                                 "us_max": round(max(t), 2)}
                gain = rec["off"]["us_median"] - rec["on"]["us_median"]
                spread = rec["off"]["us_max"] - rec["off"]["us_min"]
                rec.update(gain_us=round(gain, 2), off_spread_us=round(spread, 2), single_wins=bool(gain > spread))
                print(json.dumps(rec), flush=True)
                del graphs, sets, fn
    assert int(cnt.abs().sum()) == 0


if __name__ == "__main__":
    main()
