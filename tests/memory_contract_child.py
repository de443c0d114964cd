"""child process of test_gpu_memory_contract.py: the memory contract under the kernel forms the environment selects (run-time switches
and TRAJSDE_LIB are read once per process) or, with `bf16`, under trajsde_state_storage(1).  `forms`: one mixed and one degenerate
batch, inference forward and training step; `bf16`: the inference forward of both and trajsde_sde_step on bf16 states (the mode is
inference only).  Prints one JSON verdict line; an assertion that fails ends the process with its traceback."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(os.path.dirname(HERE), "oracle")]


def main():
    import test_gpu_memory_contract as M
    from trajsde_amd import runtime
    what = sys.argv[1]
    dev = torch.device("cuda:0")
    M.spy_on_library()
    K, T = 6, 12
    model = M.sde_model(K, T).to(dev)
    batches = (("nt61_k10_t12", M._case_batch("nt61_k10_t12")), ("isolated", M.degenerate_batch("isolated", T)))
    runs = 0
    if what == "bf16":
        assert runtime.set_state_storage("bf16") == "fp32"
        for name, batch in batches:
            M.forward_contract(f"bf16 forward {name}", model, batch, dev, K)
            runs += len(M.FILL_RUNS)
        M.sde_step_contract(model, dev, True)
        runs += 8 * len(M.FILL_RUNS)
    else:
        for name, batch in batches:
            M.forward_contract(f"forward {name}", model, batch, dev, K)
            M.training_contract(f"training {name}", model, batch, dev, K)
            runs += 2 * len(M.FILL_RUNS)
    print(json.dumps({"ok": True, "runs": runs, "what": what, "called": len(M.CALLED)}))


if __name__ == "__main__":
    main()
