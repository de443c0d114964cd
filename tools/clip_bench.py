"""What global-norm clipping adds to the end of a training step: trajsde_grad_norm_clip + trajsde_adamw_step_clipped (three launches)
against the single trajsde_adamw_step they replace and against torch.nn.utils.clip_grad_norm_ over the ~150 `.grad` slices followed by
that launch, at the model's real flat size; the variants alternate group by group on one device and are timed with HIP events after a
warm-up (GPU time of `--group` back-to-back calls, per call).  Then the three kernels alone (the library's event profiler) and the
whole training step of a BASELINE configuration with and without `gradient_clip_val`, alternating step by step.

    python tools/clip_bench.py                               # config2: 64 scenes x 128 agents, K = 6, T = 20
    python tools/clip_bench.py --config config2 --iters 30 --steps 20
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def _timed(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _model(name, clip, dev):
    import yaml
    from trajsde_amd import driver
    from trajsde_amd.synth import CONFIGS
    spec = CONFIGS[name]
    with open(os.path.join(ROOT, "trajsde_amd/configs/mi355x_sde_encoder_decoder.yml")) as f:
        cfg = yaml.safe_load(f)
    K, T = spec["num_modes"], spec["future_steps"]
    cfg["model_specific"]["kwargs"].update(num_modes=K, future_steps=T)
    cfg["aggregator"]["kwargs"]["num_modes"] = K
    cfg["decoder"]["kwargs"].update(num_modes=K, future_steps=T, max_fut_t=spec["max_fut_t"])
    model = driver.build_model(cfg, None, dev, init_seed=0).train()
    model.gradient_clip_val = clip
    return model, driver.FlatTraining(model)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="config2")
    ap.add_argument("--iters", type=int, default=30, help="timed groups per variant")
    ap.add_argument("--group", type=int, default=10, help="back-to-back calls between two events")
    ap.add_argument("--steps", type=int, default=20, help="timed training steps per variant")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--clip", type=float, default=1.0)
    args = ap.parse_args()
    from trajsde_amd import _lib
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import CONFIGS, synth
    dev = torch.device("cuda:0")
    L = _lib.lib()
    models = {k: _model(args.config, c, dev) for k, c in (("plain", None), ("clipped", args.clip))}
    ft = models["plain"][1]
    n = ft.flat_param.numel()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    grad0 = (1e-2 * torch.randn(n, generator=g)).to(dev)
    bufs = [torch.randn(n, generator=g).to(dev), grad0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)]
    ws = torch.empty(int(L.trajsde_grad_norm_ws_bytes(n)) // 8, dtype=torch.float64, device=dev)
    out = torch.empty(2, device=dev)
    sc = (1 - 1e-3 * 1e-4, 0.1, 0.999, 0.001, (1 - 0.999 ** 3) ** 0.5, 1, 1e-8, -(1e-3 / (1 - 0.9 ** 3)))
    ptrs = [t.data_ptr() for t in bufs]
    slices = [p for p in ft.params]                       # the ~150 parameters whose .grad are slices of one buffer: torch's clip over them
    ft.grads.flat.copy_(grad0)

    def plain():
        _lib.check(L.trajsde_adamw_step(*ptrs, n, *sc, st), "adamw")

    def norm_only():
        _lib.check(L.trajsde_grad_norm_clip(ptrs[1], n, args.clip, ws.data_ptr(), ws.numel() * 8, out.data_ptr(), st), "norm")

    def step_only():
        _lib.check(L.trajsde_adamw_step_clipped(*ptrs, n, *sc, out.data_ptr() + 4, st), "clipped")

    def pair():
        norm_only()
        step_only()

    def torch_clip():
        torch.nn.utils.clip_grad_norm_(slices, args.clip)
        plain()

    variants = {"adamw_step": plain, "norm_clip+adamw_step_clipped": pair, "norm_clip": norm_only, "adamw_step_clipped": step_only,
                "torch_clip_grad_norm+adamw_step": torch_clip}
    times = {k: [] for k in variants}
    for it in range(args.warmup + args.iters):
        for k, fn in variants.items():
            bufs[1].copy_(grad0)                          # (the clipped step scales the gradient in place: start every group alike)
            ft.grads.flat.copy_(grad0)
            t = _timed(fn, args.group)
            if it >= args.warmup:
                times[k].append(t)
    res = {"config": args.config, "flat_elements": n, "tensors": len(slices), "group": args.group,
           "us_per_call_median": {k: round(statistics.median(v), 2) for k, v in times.items()},
           "us_per_call_min": {k: round(min(v), 2) for k, v in times.items()}}
    # the kernels alone
    L.trajsde_profile_mode(2)
    _lib.profile_report()
    for _ in range(args.iters):
        pair()
        plain()
    torch.cuda.synchronize()
    res["kernel_us"] = {tag: round(ms * 1e3 / cnt, 2) for tag, (cnt, ms, _) in _lib.profile_report().items()}
    L.trajsde_profile_mode(0)
    # the whole training step, with and without the clip value
    spec = CONFIGS[args.config]
    batch = synth(**spec["synth"]).to(dev)
    y0 = batch.y.clone()

    def train_step(k, i):
        model, flat = models[k]
        flat.zero()
        batch.y = y0
        model.training_step(batch, i, noise=NoiseSpec(seed=100 + i)).backward()
        flat.step()

    steps = {k: [] for k in models}
    for i in range(args.warmup + args.steps):
        for k in models:
            t = _timed(lambda: train_step(k, i))
            if i >= args.warmup:
                steps[k].append(t / 1e3)
    res["train_step_ms_median"] = {k: round(statistics.median(v), 3) for k, v in steps.items()}
    res["train_step_ms_min"] = {k: round(min(v), 3) for k, v in steps.items()}
    res["last_grad_norm"] = [float(x) for x in models["clipped"][1].last_grad_norm.cpu()]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
