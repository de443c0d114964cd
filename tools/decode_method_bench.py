"""Euler against Milstein decode: trajsde_decoder_forward and trajsde_decoder_forward_milstein on the same inputs, timed with HIP events
after a warm-up, the two entry points alternating call by call on one device; then the fused decode kernel alone (k_sde_decode,
from the library's event profiler).

    python tools/decode_method_bench.py                        # the metric's shape (32 scenes x 256 agents, K = 6, 20 steps) and K = 10, T = 60
    python tools/decode_method_bench.py --shape 8192,6,20 --iters 50
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def run_shape(N, K, T, iters, warmup):
    import helpers as H
    from trajsde_amd import _lib, runtime
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    from trajsde_amd.schedule import decoder_schedule
    dev = torch.device("cuda:0")
    max_t = T / 10.0
    cfg = H.our_cfg(K, T, max_t)
    cfg["decoder"]["kwargs"]["method"] = "milstein"
    dec = PredictionModelSDENet(**cfg, init_seed=0).eval().decoder.to(dev)
    rt, L = dec._rt, _lib.lib()
    sched = decoder_schedule(T, max_t, float(dec.min_stepsize))
    step_tab = torch.from_numpy(sched.step_table()).to(dev).contiguous()
    out_tab = torch.from_numpy(sched.out_table()).to(dev).contiguous()
    g = torch.Generator().manual_seed(0)
    local, glob = torch.randn(N, 64, generator=g).to(dev), torch.randn(K, N, 64, generator=g).to(dev)
    loc = torch.empty(K, N, T, 4, device=dev)
    pi = torch.empty(N, K, device=dev)
    ws_bytes = L.trajsde_decoder_ws_bytes(N, K)
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    blobs = {"euler": rt.blob(_lib.STAGE_DECODER), "milstein": rt.blob(_lib.STAGE_DECODER_MILSTEIN)}
    entry = {"euler": L.trajsde_decoder_forward, "milstein": L.trajsde_decoder_forward_milstein}
    noise = _lib.Noise(C.c_uint64(7), None, None, None)
    stream = torch.cuda.current_stream().cuda_stream

    def call(m):
        _lib.check(entry[m](N, K, T, blobs[m].data_ptr(), local.data_ptr(), glob.data_ptr(), step_tab.data_ptr(), sched.n_euler,
                            out_tab.data_ptr(), float(dec.min_scale), C.byref(noise), ws.data_ptr(), ws_bytes, loc.data_ptr(),
                            pi.data_ptr(), stream), m)

    for _ in range(warmup):
        call("euler")
        call("milstein")
    torch.cuda.synchronize()
    times = {"euler": [], "milstein": []}
    for i in range(iters):
        for m in (("euler", "milstein") if i % 2 == 0 else ("milstein", "euler")):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(m)
            e1.record()
            e1.synchronize()
            times[m].append(e0.elapsed_time(e1) * 1e3)
    kernel = {}
    for m in ("euler", "milstein"):                      # the fused decode kernel alone (the library's per-launch events)
        L.trajsde_profile_mode(2)
        for _ in range(5):
            call(m)
        torch.cuda.synchronize()
        L.trajsde_profile_mode(0)
        tab = _lib.profile_report()
        kernel[m] = {tag: ms / n * 1e3 for tag, (n, ms, _) in tab.items() if "k_sde_decode" in tag}
    _lib.check_range()
    med = {m: statistics.median(v) for m, v in times.items()}
    kd = {m: sum(kernel[m].values()) for m in kernel}
    return {"N": N, "K": K, "T": T, "n_euler": sched.n_euler, "iters": iters,
            "call_us_median": {m: round(v, 1) for m, v in med.items()},
            "call_us_min": {m: round(min(v), 1) for m, v in times.items()},
            "decode_kernel_us": {m: round(v, 1) for m, v in kd.items()},
            "decode_kernel_tags": kernel,
            "ratio_call": round(med["milstein"] / med["euler"], 3),
            "ratio_kernel": round(kd["milstein"] / kd["euler"], 3) if kd["euler"] else None,
            "sync_free_forward": runtime.sync_free()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="N,K,T (repeatable); default: 8192,6,20 and 8192,10,60")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split(",")) for s in (a.shape or ["8192,6,20", "8192,10,60"])]
    lines = []
    for N, K, T in shapes:
        r = run_shape(N, K, T, a.iters, a.warmup)
        print(json.dumps(r), flush=True)
        lines.append(r)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
