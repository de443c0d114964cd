"""The welded decoder backward against the backward from cotangents: decoder_l2_backward (the N winning paths) against
decoder_cotangent_backward fed the same loss's dL/dloc, once over all K * N paths (`support="all"`) and once over each actor's supported
mode (`support="winner"`), and the whole training step (training_step + backward + FlatTraining's AdamW) under [L2, DiffBCE] against
[L2, DiffBCE, SoftTargetCrossEntropyLoss] with `cotangent_support: all` and `winner`; the three routes alternating call by call on one
device, timed with HIP events after a warm-up, in `--rounds` rounds whose medians are reported one by one (the spread of a route's own
round medians is what a difference between two routes has to exceed); the three workspace queries; then the replay, sweep and
weight-gradient kernels alone (the library's event profiler).

    python tools/cotangent_bench.py                          # config2 (64 scenes x 128 agents, K = 6, T = 20) and config4 (128 x 48, K = 10, T = 60)
    python tools/cotangent_bench.py --config config2 --iters 10
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
METHODS = ("welded", "cotangent", "winner")
CUSTOM = ["L2", "DiffBCE", "SoftTargetCrossEntropyLoss"]
LOSS_SETS = {"welded": ["L2", "DiffBCE"], "cotangent": CUSTOM, "winner": CUSTOM}


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def run_config(name, iters, warmup, rounds):
    import yaml
    from trajsde_amd import _lib, driver, runtime
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import CONFIGS, synth
    spec = CONFIGS[name]
    with open(os.path.join(ROOT, "trajsde_amd/configs/mi355x_sde_encoder_decoder.yml")) as f:
        base = yaml.safe_load(f)
    K, T = spec["num_modes"], spec["future_steps"]
    dev = torch.device("cuda:0")
    models, flats = {}, {}
    for m in METHODS:
        cfg = json.loads(json.dumps(base))
        cfg["model_specific"]["kwargs"].update(num_modes=K, future_steps=T, cotangent_support="winner" if m == "winner" else "all")
        cfg["aggregator"]["kwargs"]["num_modes"] = K
        cfg["decoder"]["kwargs"].update(num_modes=K, future_steps=T, max_fut_t=spec["max_fut_t"])
        cfg["losses"] = ["trajsde_amd/losses.py"] * len(LOSS_SETS[m])
        cfg["losses_module"], cfg["loss_weights"] = list(LOSS_SETS[m]), [1.0] * len(LOSS_SETS[m])
        cfg["loss_args"] = [{"reduction": "mean"} for _ in LOSS_SETS[m]]
        models[m] = driver.build_model(cfg, None, dev, init_seed=0).train()
        flats[m] = driver.FlatTraining(models[m])
    batch = synth(**spec["synth"]).to(dev)
    y0 = batch.y.clone()

    def step(m, i):
        flats[m].zero()
        batch.y = y0
        models[m].training_step(batch, i, noise=NoiseSpec(seed=100 + i)).backward()
        flats[m].step()

    # the decoder stage alone on the same embeddings; the cotangent is the L2 loss's own, built by torch once
    from trajsde_amd import losses
    stage = {}
    for m in METHODS:
        model = models[m]
        data = synth(**spec["synth"]).to(dev)               # (a batch of its own: the training steps rotate theirs)
        rot, y_rot = runtime.rotate_inputs(data)
        data.y, data["rotate_mat"] = y_rot, rot
        noise = NoiseSpec(seed=5)
        with torch.no_grad():
            local, *_ = model.encoder(data=data, noise=noise)
            glob = model.aggregator(data=data, local_embed=local)
            out = model.decoder(data=data, local_embed=local, global_embed=glob, noise=noise)
        loc = out["loc"].detach().clone().requires_grad_(True)
        with torch.enable_grad():
            (d_loc,) = torch.autograd.grad(losses.L2()(data, {"loc": loc, "reg_mask": out["reg_mask"]}), [loc])
        stage[m] = (model.decoder._rt, data, local, glob, out, noise, d_loc)

    def dec_bwd(m):
        rt, data, local, glob, out, noise, d_loc = stage[m]
        if m == "welded":
            rt.decoder_l2_backward(data, local, glob, out, noise)
        else:
            rt.decoder_cotangent_backward(data, local, glob, out, noise, d_loc, None, support="winner" if m == "winner" else "all")

    for i in range(warmup):
        for m in METHODS:
            dec_bwd(m)
            step(m, i)
    torch.cuda.synchronize()
    t_bwd, t_step = {m: [] for m in METHODS}, {m: [] for m in METHODS}
    for i in range(iters * rounds):
        order = METHODS[i % len(METHODS):] + METHODS[:i % len(METHODS)]
        for m in order:
            t_bwd[m].append(_timed(lambda: dec_bwd(m)))
        for m in order:
            t_step[m].append(_timed(lambda: step(m, warmup + i)))
    models["winner"].check_cotangent_support()
    sched = stage["winner"][0]._decoder_tables(T, dev)[0]
    N = int(batch.num_nodes)
    ws = {m: int(getattr(_lib.lib(), q)(N, K, T, sched.n_euler))
          for m, q in (("welded", "trajsde_decoder_backward_ws_bytes"), ("welded_nll", "trajsde_decoder_nll_backward_ws_bytes"),
                       ("cotangent", "trajsde_decoder_cotangent_backward_ws_bytes"),
                       ("winner", "trajsde_decoder_cotangent_backward_sel_ws_bytes"))}
    kernels = {}
    L = _lib.lib()
    for m in METHODS:
        L.trajsde_profile_mode(2)
        for _ in range(3):
            dec_bwd(m)
        torch.cuda.synchronize()
        L.trajsde_profile_mode(0)
        tab = _lib.profile_report()
        kernels[m] = {tag: round(ms / n * 1e3, 1) for tag, (n, ms, _) in tab.items() if "k_sde" in tag or "wgrad" in tag or "cot" in tag or "pi_head" in tag or "init" in tag or "support" in tag}
    _lib.check_range()
    med = lambda d: {m: round(statistics.median(v), 1) for m, v in d.items()}
    by_round = lambda d: {m: [round(statistics.median(v[r * iters:(r + 1) * iters]), 1) for r in range(rounds)] for m, v in d.items()}
    spread = lambda v: round(max(v) - min(v), 1)
    rb, rs = by_round(t_bwd), by_round(t_step)
    return {"config": name, "K": K, "T": T, "agents": int(batch.num_nodes), "iters": iters, "rounds": rounds, "n_euler": sched.n_euler,
            "workspace_bytes": ws,
            "decoder_backward_us_round_medians": rb, "train_step_us_round_medians": rs,
            # the acceptance rule of the winner route: below the dense route by more than the spread of the dense route's own round medians
            "winner_vs_cotangent_decoder_backward": {"gain_us": round(statistics.median(t_bwd["cotangent"]) - statistics.median(t_bwd["winner"]), 1),
                                                     "cotangent_spread_us": spread(rb["cotangent"])},
            "winner_vs_cotangent_train_step": {"gain_us": round(statistics.median(t_step["cotangent"]) - statistics.median(t_step["winner"]), 1),
                                               "cotangent_spread_us": spread(rs["cotangent"])},
            "decoder_backward_us_median": med(t_bwd), "train_step_us_median": med(t_step),
            "decoder_backward_us_min": {m: round(min(v), 1) for m, v in t_bwd.items()},
            "train_step_us_min": {m: round(min(v), 1) for m, v in t_step.items()},
            "ratio_decoder_backward": round(statistics.median(t_bwd["cotangent"]) / statistics.median(t_bwd["welded"]), 3),
            "ratio_train_step": round(statistics.median(t_step["cotangent"]) / statistics.median(t_step["welded"]), 3),
            "ratio_decoder_backward_winner": round(statistics.median(t_bwd["winner"]) / statistics.median(t_bwd["welded"]), 3),
            "ratio_train_step_winner": round(statistics.median(t_step["winner"]) / statistics.median(t_step["welded"]), 3),
            "kernel_us": kernels}


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
