"""child process of test_gpu_cotangent_sel.py::test_one_wave_kernel_forms_match_float64_autograd: trajsde_decoder_cotangent_backward_sel
once, at the test's own case (test_gpu_cotangent_sel.build_case("n17")) under seeded noise, with the library's run-time switches taken
from the environment (they are read once per process); saves the gradients, the cotangents they belong to and the two status words
with torch.save to the path given as the only argument."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(out_path):
    import test_gpu_cotangent_sel as S
    from trajsde_amd import _lib, runtime
    dev = torch.device("cuda:0")
    c = S.build_case("n17", dev, noise=runtime.NoiseSpec(seed=S.FORMS_SEED))
    res = S.run(c, "winner")
    torch.cuda.synchronize()
    _lib.check_range()
    torch.save({"grads": {k: v.detach().cpu() for k, v in S._all(res).items()}, "d_loc": c["d_loc"].cpu(), "d_pi": c["d_pi"].cpu(),
                "status": res["support_status"].tolist()}, out_path)


if __name__ == "__main__":
    main(sys.argv[1])
