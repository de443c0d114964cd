"""Time the graph stage alone (trajsde_graph_prepare_async + trajsde_graph_compact through runtime.GraphContext) on the metric
workload, with HIP events, and print the library's per-kernel table for it.

    python tools/graph_stage_bench.py [--workload metric256] [--iters 50] [--exact]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from trajsde_amd import _lib, runtime
    from trajsde_amd.runtime import GraphContext, NoiseSpec
    from trajsde_amd.synth import CONFIGS, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="metric256")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--exact", action="store_true")
    ap.add_argument("--edges", default="dataset", choices=("dataset", "shuffled", "swapped"),
                    help="the actor edge list as the datasets emit it, randomly permuted, or with ONE pair of neighbouring edges exchanged "
                         "(the last two are the same graph, not in dataset order: the device-decided general path, caught early / late)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    batch = synth(**CONFIGS[a.workload]["synth"])
    ei = batch["edge_index"]
    if a.edges == "shuffled":
        batch["edge_index"] = ei[:, torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(1))].contiguous()
    elif a.edges == "swapped":
        j = ei.shape[1] // 2
        ei[:, [j, j + 1]] = ei[:, [j + 1, j]]
    batch = batch.to(dev)
    rot, y_rot = runtime.rotate_inputs(batch)
    batch["rotate_mat"] = rot

    def once(i):
        if GraphContext.KEY in batch:
            del batch[GraphContext.KEY]
        return GraphContext.get(batch, 50.0, 21, NoiseSpec(seed=i), exact=a.exact)
    for i in range(5):
        gc = once(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(a.iters):
        gc = once(10 + i)
    e1.record()
    torch.cuda.synchronize()
    print(f"graph stage ({'exact' if a.exact else 'sync-free'}, {a.edges} edge order): {e0.elapsed_time(e1) / a.iters * 1e3:.1f} us per batch, counts {gc.true_counts()}, "
          f"actor CSR path: {gc.graph_path()}")
    _lib.lib().trajsde_profile_mode(2)
    for i in range(3):
        once(1000 + i)
    torch.cuda.synchronize()
    _lib.lib().trajsde_profile_mode(0)
    tab = _lib.profile_report()
    for tag, (n, ms, dom) in sorted(tab.items(), key=lambda kv: -kv[1][1]):
        print(f"   {tag:24s} {ms / 3 * 1e3:8.1f} us")


if __name__ == "__main__":
    main()
