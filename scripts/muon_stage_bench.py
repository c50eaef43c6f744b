"""Muon on GPT-2 125M's 48 hidden matrices on one MI355X: per-stage kernel times with achieved TFLOP/s (stages 1 and 2
with the upper-triangle tile table and with every tile), and the optimizer step with and without ``muon=`` on the
model's real flat layout.  Device events around launches that end in a synchronise; prints one JSON line."""
import argparse
import json

import torch

from polyaxon_amd.models.transformer import Transformer, gpt2_125m, muon_parameter_names
from polyaxon_amd.ops.flat import FlatParams
from polyaxon_amd.ops.optim import FusedAdamW


def timed(fn, reps, before=None):
    total = 0.0
    for _ in range(reps):
        if before is not None:
            before()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        total += t0.elapsed_time(t1)
    return total / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {}
    step_ms = {}
    for name in ("adamw", "muon"):
        torch.manual_seed(0)
        with torch.device(dev):
            model = Transformer(gpt2_125m())
        flat = FlatParams(model, dev, channels_last=False, lp_dtype=torch.bfloat16)
        opt = FusedAdamW(flat, muon=muon_parameter_names(model) if name == "muon" else None)

        def fill():
            flat.lp_grads.normal_(0, 0.02)
            flat.grads.normal_(0, 0.02)

        timed(opt.step_, 3, fill)
        step_ms[name] = timed(opt.step_, a.reps, fill)
        if name == "muon":
            plan = opt._mu.plan
            st = torch.cuda.current_stream().cuda_stream
            full = {1: sum(2 * min(r, c) ** 2 * max(r, c) for r, c in plan.shapes),
                    2: sum(2 * min(r, c) ** 3 for r, c in plan.shapes)}
            full[3] = full[1]
            for stage in (1, 2, 3):
                for tri in ((True, False) if stage < 3 else (True,)):
                    fn = lambda: plan.stage(stage, False, 0, st, triangle=tri)  # noqa: E731
                    timed(fn, 3)
                    ms = timed(fn, a.reps)
                    key = f"stage{stage}_{'triangle' if tri else 'all_tiles'}" if stage < 3 else "stage3"
                    out[key] = {"ms": round(ms, 4), "tflops_of_full_product": round(full[stage] / ms / 1e9, 1),
                                "tiles": int((plan.tiles_rect if stage == 3 else plan.tiles_sym if tri
                                              else plan.tiles_full).shape[0])}
            out["iteration_tflop_full_products"] = round(5 * sum(full.values()) / 1e12, 3)
        del opt, flat, model
    out["optimizer_step_ms"] = {k: round(v, 3) for k, v in step_ms.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
