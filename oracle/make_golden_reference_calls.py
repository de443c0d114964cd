"""Generate tests/golden/reference_calls/*.npz: what two of the REFERENCE's own functions return, so that the CPU tests that
hold ours against them need no reference tree.  Build container only.

    python oracle/make_golden_reference_calls.py

* laplace_nll.npz -- losses/laplace_nll_loss.py LaplaceNLLLoss(eps=1e-6) on the oracle's forward of the mixed_k6_t20 case
  (the inputs it saw, `in.*`, and its value, `out.value`), for tests/test_host_logic.py.
* leave_only_agent.npz -- the model class's static `leave_only_agent` (MODEL:168-202) on helpers.leave_only_agent_case():
  the batch fields and outputs it leaves (`data.*`, `out.*`) and `num_nodes`, for tests/test_lightning_boundary.py.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE, os.path.join(ROOT, "tests")]

import helpers as H                                            # noqa: E402
import ref_loader as R                                        # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reference_calls")


def laplace_nll():
    from importlib.machinery import SourceFileLoader
    batch, meta, _, _ = H.load_fixture("mixed_k6_t20")
    model, cfg = H.build_model(meta)
    o = H.oracle_forward(model, cfg, batch, meta["noise_seed"], want_intermediates=False)
    inputs = {"y": o["y"], "loc": o["loc"], "reg_mask": o["reg_mask"]}
    path = os.path.join(R.REFERENCE_ROOT, "losses", "laplace_nll_loss.py")
    ref = SourceFileLoader("ref_laplace", path).load_module("ref_laplace").LaplaceNLLLoss(eps=1e-6)
    value = float(ref({"y": inputs["y"].clone()}, {k: v.clone() for k, v in inputs.items()}))
    fx = {f"in.{k}": v.numpy() for k, v in inputs.items()}
    fx["out.value"] = np.float64(value)
    print("laplace_nll", value)
    return fx


def leave_only_agent():
    batch, out = H.leave_only_agent_case()
    data = R.to_reference_data(batch)
    R.reference_model_class().leave_only_agent(data, out)
    fx = {f"data.{k}": data[k].numpy() for k in H.LEAVE_ONLY_AGENT_KEYS}
    fx.update({f"out.{k}": out[k].numpy() for k in ("loc", "pi", "reg_mask")})
    fx["num_nodes"] = np.int64(data.num_nodes)
    print("leave_only_agent", {k: v.shape for k, v in fx.items()})
    return fx


def main():
    if not R.reference_available():
        sys.exit("reference tree not found")
    os.makedirs(OUT, exist_ok=True)
    for name, make in (("laplace_nll", laplace_nll), ("leave_only_agent", leave_only_agent)):
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **make())
        print(f"-> {path} {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
