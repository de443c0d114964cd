"""Monte-Carlo decoding against R forwards: PredictionModelSDENet.predict_samples(batch, R) -- graph stage, encoder and interactor once,
R sample paths per (mode, actor) in one decode launch -- and R back-to-back model(batch, noise=...) calls on the same box, in the same
process, alternating run by run; then the decode kernels alone (k_sde_decode_mc against k_sde_decode, from the library's per-launch
events).  One stream of work, host clock around a window that ends in a device synchronise, medians of `--iters` runs after a warm-up.

    python tools/mc_decode_bench.py                              # metric256 (32 x 256) and config2 (64 x 128), R = 4, 16, 64
    python tools/mc_decode_bench.py --workload metric256 --samples 16 --iters 30 --out profiles/mc.jsonl

The forward is untouched by the sampling feature, so `forward_ms` of this tree is the figure of the commit before it; run the tool in
a checkout of that commit to see so (it then reports the forwards alone: there is no predict_samples to time).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _window(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def run_workload(name, samples, iters, warmup):
    import helpers as H
    from trajsde_amd import _lib
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import CONFIGS, synth
    dev = torch.device("cuda:0")
    spec = CONFIGS[name]
    K, T = spec["num_modes"], spec["future_steps"]
    model = PredictionModelSDENet(**H.our_cfg(K, T, spec["max_fut_t"]), init_seed=0).eval().to(dev)
    batch = synth(**spec["synth"]).to(dev)
    N = batch.num_nodes
    y0 = batch.y.clone()
    L = _lib.lib()
    have_mc = hasattr(model, "predict_samples")
    seed = [1000]

    def forwards(R):
        for _ in range(R):
            seed[0] += 1
            batch.y = y0                                        # the forward rotates y in place (as bench.py's Workload.step)
            model(batch, noise=NoiseSpec(seed=seed[0]))

    def mc(R, keep):
        seed[0] += 1
        batch.y = y0
        model.predict_samples(batch, R, noise=NoiseSpec(seed=seed[0]), return_samples=keep)

    res = {"workload": name, "N": N, "K": K, "T": T, "paths": K * N, "iters": iters, "rows": []}
    with torch.no_grad():
        for R in samples:
            variants = {"forwards": lambda R=R: forwards(R)}
            if have_mc:
                variants["mc"] = lambda R=R: mc(R, False)
                variants["mc_samples"] = lambda R=R: mc(R, True)
            for _ in range(warmup):
                for fn in variants.values():
                    fn()
            times = {k: [] for k in variants}
            order = list(variants)
            for i in range(iters):
                for k in (order if i % 2 == 0 else order[::-1]):
                    times[k].append(_window(variants[k]))
            row = {"R": R, **{k + "_ms": round(statistics.median(v), 3) for k, v in times.items()},
                   **{k + "_ms_min_max": [round(min(v), 3), round(max(v), 3)] for k, v in times.items()}}
            row["forward_ms"] = round(row["forwards_ms"] / R, 3)
            if have_mc:
                row["speedup"] = round(row["forwards_ms"] / row["mc_ms"], 2)
                # the kernels alone: the library's events around every launch (serialises nothing: one stream)
                kern = {}
                for tag, fn, n in (("plain", lambda: forwards(1), 5), ("mc", lambda R=R: mc(R, False), 5)):
                    _lib.profile_report()
                    L.trajsde_profile_mode(2)
                    for _ in range(n):
                        fn()
                    torch.cuda.synchronize()
                    L.trajsde_profile_mode(0)
                    tab = _lib.profile_report()
                    want = "k_sde_decode_mc" if tag == "mc" else "k_sde_decode<"
                    kern[tag] = {t: ms / cnt for t, (cnt, ms, _) in tab.items() if want in t}
                    if tag == "mc":
                        kern["combine"] = {t: ms / cnt for t, (cnt, ms, _) in tab.items() if "k_mc_combine" in t}
                plain_ms, mc_ms = sum(kern["plain"].values()), sum(kern["mc"].values())
                row.update(k_sde_decode_ms=round(plain_ms, 4), k_sde_decode_mc_ms=round(mc_ms, 4),
                           k_mc_combine_ms=round(sum(kern["combine"].values()), 4),
                           per_path_ratio=round(mc_ms / (R * plain_ms), 3) if plain_ms else None, kernel_tags=sorted(kern["mc"]) + sorted(kern["plain"]))
            res["rows"].append(row)
            torch.cuda.empty_cache()
    _lib.check_range()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="append", help="synth.CONFIGS key (repeatable); default: metric256 and config2")
    ap.add_argument("--samples", default="4,16,64", help="comma-separated R")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mc_decode_bench needs a GPU: a time taken elsewhere says nothing")
    lines = []
    for name in (a.workload or ["metric256", "config2"]):
        r = run_workload(name, [int(x) for x in a.samples.split(",")], a.iters, a.warmup)
        print(json.dumps(r), flush=True)
        lines.append(r)
        if a.out:
            with open(a.out, "w") as f:
                for x in lines:
                    f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
