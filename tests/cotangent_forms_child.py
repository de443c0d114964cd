"""child process of test_gpu_cotangent.py::test_both_kernel_forms_match_float64_autograd: the cotangent entry point once, at the
test's own case (test_gpu_cotangent._forms_case), with the library's run-time switches taken from the environment (they are read once
per process); saves {name: gradient} with torch.save to the path given as the only argument."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(out_path):
    import test_gpu_cotangent as M
    from trajsde_amd import _lib, runtime
    dev = torch.device("cuda:0")
    model, cfg, batch, sched, t = M._forms_case(dev)
    noise = runtime.NoiseSpec(seed=M.FORMS_SEED)
    data, local, glob = batch.to(dev), t["local"].to(dev), t["glob"].to(dev)
    rt = model.decoder._rt
    with torch.no_grad():
        out = rt.decoder_forward(data, local, glob, noise)
    res = rt.decoder_cotangent_backward(data, local, glob, out, noise, t["d_loc"].to(dev), t["d_pi"].to(dev))
    torch.cuda.synchronize()
    _lib.check_range()
    torch.save({k: v.detach().cpu() for k, v in M._all(res).items()}, out_path)


if __name__ == "__main__":
    main(sys.argv[1])
