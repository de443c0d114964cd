"""The vanilla HiVT variant's welded decoder backward against its backward from cotangents: mlp_decoder_nll_backward (the N winning
rows, the loss fused in) against mlp_decoder_cotangent_backward fed the same loss's dL/dloc (all K * N rows and the pi head), on the
embeddings of one forward; the two alternating call by call on one device, timed with HIP events after a warm-up.  Also prints the
workspace queries of the two entry points and the library's per-kernel event profile of the new one.

    python tools/grid_cotangent_bench.py                     # 64 scenes x 128 agents, K = 6, T = 30
    python tools/grid_cotangent_bench.py --scenes 32 --agents 48 --iters 20
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
METHODS = ("welded", "cotangent")


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def run(scenes, agents, K, T, iters, warmup):
    import yaml
    from trajsde_amd import _lib, driver, losses
    from trajsde_amd.synth import synth
    with open(os.path.join(ROOT, "trajsde_amd/configs/mi355x_trmenc_mlpdec.yml")) as f:
        cfg = yaml.safe_load(f)
    cfg["model_specific"]["kwargs"].update(num_modes=K, future_steps=T)
    cfg["aggregator"]["kwargs"]["num_modes"] = K
    cfg["decoder"]["kwargs"].update(num_modes=K, future_steps=T)
    dev = torch.device("cuda:0")
    model = driver.build_model(cfg, None, dev, init_seed=0).eval()
    data = synth(S=scenes, n=agents, L=64, F=T, box=200.0, seed=2, mixed_source=True).to(dev)
    with torch.no_grad():
        out = model(data)                                    # rotates data.y
    local, glob = out["local_embed"], out["global_embed"]
    loc = out["loc"].detach().clone().requires_grad_(True)
    with torch.enable_grad():
        (d_loc,) = torch.autograd.grad(losses.LaplaceNLLLoss(eps=1e-6)(data, {"loc": loc, "reg_mask": out["reg_mask"]}), [loc])
    d_pi = torch.randn(out["pi"].shape, device=dev) * 1e-3
    rt = model.decoder._rt

    def dec_bwd(m):
        if m == "welded":
            rt.mlp_decoder_nll_backward(data, local, glob, out, eps=1e-6)
        else:
            rt.mlp_decoder_cotangent_backward(data, local, glob, out, d_loc, d_pi)

    for _ in range(warmup):
        for m in METHODS:
            dec_bwd(m)
    torch.cuda.synchronize()
    t = {m: [] for m in METHODS}
    for i in range(iters):
        for m in (METHODS if i % 2 == 0 else METHODS[::-1]):
            t[m].append(_timed(lambda: dec_bwd(m)))
    L = _lib.lib()
    L.trajsde_profile_mode(2)
    for _ in range(3):
        dec_bwd("cotangent")
    torch.cuda.synchronize()
    L.trajsde_profile_mode(0)
    kernels = {tag: round(ms / n * 1e3, 1) for tag, (n, ms, _) in _lib.profile_report().items()}
    _lib.check_range()
    N = int(local.shape[0])
    return {"scenes": scenes, "agents": N, "K": K, "T": T, "iters": iters,
            "decoder_backward_us_median": {m: round(statistics.median(v), 1) for m, v in t.items()},
            "decoder_backward_us_min": {m: round(min(v), 1) for m, v in t.items()},
            "ratio": round(statistics.median(t["cotangent"]) / statistics.median(t["welded"]), 3),
            "workspace_bytes": {"welded": int(L.trajsde_mlp_decoder_nll_backward_ws_bytes(N)),
                                "cotangent": int(L.trajsde_mlp_decoder_cotangent_backward_ws_bytes(N, K, T))},
            "cotangent_kernel_us": kernels}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=64)
    ap.add_argument("--agents", type=int, default=128, help="agents per scene")
    ap.add_argument("--modes", type=int, default=6)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    a = ap.parse_args()
    r = run(a.scenes, a.agents, a.modes, a.steps, a.iters, a.warmup)
    print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
