"""One training step through the stage-level autograd nodes (`autograd: true` on the three stages: the glue calls encoder, aggregator
and decoder, torch evaluates [L2, DiffBCE, SoftTargetCrossEntropyLoss] on their outputs, `loss.backward()`) against the model-level
`training_step(...).backward()` on the same loss set, batch and noise, with `cotangent_support` all and winner.  A step here is
forward + loss + backward, gradients into `.grad` (no optimizer).  The four routes alternate call by call on one device, timed with HIP
events after a warm-up, in `--rounds` rounds whose medians are reported one by one; then the two DLDG producers alone (k_diff_cot of
the stage route, k_diffbce of the model-level one) from the library's event profiler.

    python tools/stage_autograd_bench.py                     # config2 (64 scenes x 128 agents, K = 6, T = 20) and config4 (128 x 48, K = 10, T = 60)
    python tools/stage_autograd_bench.py --config config2 --iters 10
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
ROUTES = ("model_all", "model_winner", "stage_all", "stage_winner")
CUSTOM = ["L2", "DiffBCE", "SoftTargetCrossEntropyLoss"]
WEIGHTS = [1.0, 0.5, 0.7]


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def run_config(name, iters, warmup, rounds):
    import yaml
    from trajsde_amd import _lib, driver
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import CONFIGS, synth
    spec = CONFIGS[name]
    with open(os.path.join(ROOT, "trajsde_amd/configs/mi355x_sde_encoder_decoder.yml")) as f:
        base = yaml.safe_load(f)
    K, T = spec["num_modes"], spec["future_steps"]
    dev = torch.device("cuda:0")
    models = {}
    for r in ROUTES:
        level, support = r.split("_")
        cfg = json.loads(json.dumps(base))
        cfg["model_specific"]["kwargs"].update(num_modes=K, future_steps=T, cotangent_support=support)
        cfg["aggregator"]["kwargs"]["num_modes"] = K
        cfg["decoder"]["kwargs"].update(num_modes=K, future_steps=T, max_fut_t=spec["max_fut_t"])
        if level == "stage":
            for s in ("encoder", "aggregator", "decoder"):
                cfg[s]["kwargs"]["autograd"] = True
            cfg["decoder"]["kwargs"]["cotangent_support"] = support
        cfg["losses"] = ["trajsde_amd/losses.py"] * len(CUSTOM)
        cfg["losses_module"], cfg["loss_weights"] = list(CUSTOM), list(WEIGHTS)
        cfg["loss_args"] = [{"reduction": "mean"} for _ in CUSTOM]
        models[r] = driver.build_model(cfg, None, dev, init_seed=0).train()
    batch = synth(**spec["synth"]).to(dev)
    y0 = batch.y.clone()

    def step(r, i):
        model = models[r]
        for p in model.parameters():
            p.grad = None
        batch.y = y0
        noise = NoiseSpec(seed=100 + i)
        if r.startswith("model"):
            model.training_step(batch, i, noise=noise).backward()
            return
        model._ensure_rotated(batch)                         # the stage-level glue: what the reference's own model class does
        local, diff_in, diff_out, label_in, label_out = model.encoder(data=batch, noise=noise)
        glob = model.aggregator(data=batch, local_embed=local, noise=noise)
        out = model.decoder(data=batch, local_embed=local, global_embed=glob, noise=noise)
        out["diff_in"], out["diff_out"], out["label_in"], out["label_out"] = diff_in, diff_out, label_in, label_out
        sum(w * fn(batch, out) for fn, w in zip(model.losses, model.loss_weights)).backward()

    for i in range(warmup):
        for r in ROUTES:
            step(r, i)
    torch.cuda.synchronize()
    t = {r: [] for r in ROUTES}
    for i in range(iters * rounds):
        order = ROUTES[i % len(ROUTES):] + ROUTES[:i % len(ROUTES)]
        for r in order:
            t[r].append(_timed(lambda: step(r, warmup + i)))
    models["stage_winner"].check_cotangent_support(models["stage_winner"].decoder.last_support_status)   # winner's premise held
    models["model_winner"].check_cotangent_support()
    kernels = {}
    L = _lib.lib()
    for r in ("model_all", "stage_all"):
        L.trajsde_profile_mode(2)
        for i in range(3):
            step(r, i)
        torch.cuda.synchronize()
        L.trajsde_profile_mode(0)
        kernels[r] = {tag: round(ms / n * 1e3, 1) for tag, (n, ms, _) in _lib.profile_report().items() if "k_diff" in tag}
    _lib.check_range()
    by_round = {r: [round(statistics.median(v[k * iters:(k + 1) * iters]), 1) for k in range(rounds)] for r, v in t.items()}
    med = {r: round(statistics.median(v), 1) for r, v in t.items()}
    return {"config": name, "K": K, "T": T, "agents": int(batch.num_nodes), "iters": iters, "rounds": rounds,
            "step_us_round_medians": by_round, "step_us_median": med, "step_us_min": {r: round(min(v), 1) for r, v in t.items()},
            "stage_over_model_all": round(med["stage_all"] / med["model_all"], 3),
            "stage_over_model_winner": round(med["stage_winner"] / med["model_winner"], 3),
            "dldg_kernel_us": kernels}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", help="synth.CONFIGS name (repeatable); default: config2 and config4")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="rounds of --iters alternating calls; every round's median is reported")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    a = ap.parse_args()
    lines = []
    for name in a.config or ["config2", "config4"]:
        r = run_config(name, a.iters, a.warmup, a.rounds)
        print(json.dumps(r), flush=True)
        lines.append(r)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
