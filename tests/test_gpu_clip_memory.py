"""trajsde_grad_norm_clip and trajsde_adamw_step_clipped inside the red-zone arenas of tests/guarded_memory.py (-m gpu): the accounting
of tests/test_gpu_cotangent_memory.py for `_lib.CLIP_EXT_SIGNATURES`.  Every buffer in an arena of its own; `out` and the workspace
routed into arenas that start as NaN, as zeros or as random bits.  For n one below, at and one above a wave and one above a
workgroup's share: every guard byte intact, the inputs unwritten, `out` and the step's four outputs overwritten in full, and the
results bit-identical under the three poisons and equal to the same calls on plain tensors."""
import pytest
import torch

import guarded_memory as GM

pytestmark = pytest.mark.gpu
MAX_NORM = 0.05
SCALARS = (1 - 3e-3 * 1e-2, 0.1, 0.999, 0.001, (1 - 0.999 ** 2) ** 0.5, 1, 1e-8, -(3e-3 / (1 - 0.9 ** 2)))     # step 2, the dividing form


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    return torch.device("cuda:0")


def test_every_clip_entry_point_is_a_size_query_or_runs_in_these_arenas():
    from trajsde_amd import _lib
    assert {n for n in _lib.CLIP_EXT_SIGNATURES if n.endswith("_bytes")} == {"trajsde_grad_norm_ws_bytes"}
    launches = {n for n in _lib.CLIP_EXT_SIGNATURES if not n.endswith("_bytes")}
    assert launches == {"trajsde_grad_norm_clip", "trajsde_adamw_step_clipped"}


def _run(L, t, n, out, ws, ws_bytes):
    """the two launches on the tensors of `t`; -> nothing (the caller synchronises)"""
    from trajsde_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L.trajsde_grad_norm_clip(t["grad_in"].data_ptr(), n, MAX_NORM, ws.data_ptr(), ws_bytes, out.data_ptr(), st), "norm")
    _lib.check(L.trajsde_adamw_step_clipped(t["param"].data_ptr(), t["grad"].data_ptr(), t["exp_avg"].data_ptr(), t["exp_avg_sq"].data_ptr(),
                                            n, *SCALARS, out.data_ptr() + 4, st), "step")


@pytest.mark.parametrize("n", [63, 64, 65, "share+1"])
def test_clip_entry_points_stay_inside_their_buffers(n, dev):
    from trajsde_amd import _lib
    L = _lib.lib()
    n = _lib.CLIP_WG_FLOATS + 1 if n == "share+1" else n
    g = torch.Generator().manual_seed(60 + n)
    grad = torch.randn(n, generator=g)
    grad = grad + torch.where(grad < 0, -0.5, 0.5)                            # |g| >= 0.5, no element near zero: every output moves
    host = dict(grad_in=grad, grad=grad.clone(), param=torch.randn(n, generator=g), exp_avg=0.1 * torch.randn(n, generator=g),
                exp_avg_sq=0.01 * torch.rand(n, generator=g))
    need = int(L.trajsde_grad_norm_ws_bytes(n))
    assert need == 8 * ((n + _lib.CLIP_WG_FLOATS - 1) // _lib.CLIP_WG_FLOATS)
    # the same calls on plain tensors: what the arenas must reproduce
    plain = {k: v.clone().to(dev) for k, v in host.items()}
    plain_out = torch.empty(2, device=dev)
    _run(L, plain, n, plain_out, torch.empty(need // 8, dtype=torch.float64, device=dev), need)
    torch.cuda.synchronize()
    assert 0.0 < float(plain_out[1]) < 1.0 and abs(float(plain_out[0]) - float(grad.double().norm())) < 1e-5 * float(plain_out[0])
    for k in ("grad", "param", "exp_avg", "exp_avg_sq"):                      # overwritten in full: no element kept its value
        assert bool((plain[k] != host[k].to(dev)).all()), k
    assert torch.equal(plain["grad_in"], host["grad_in"].to(dev))
    for fill, poison in (("A", "nan"), ("B", "zero"), ("A", 7)):
        gm = GM.GuardedMemory(poison=poison)
        t = {k: gm.placed(v.to(dev), fill, label=k, const=(k == "grad_in")) for k, v in host.items()}
        with gm:
            out = torch.empty(2, dtype=torch.float32, device=dev)             # poisoned: the call overwrites both words
            ws = torch.empty(need // 8, dtype=torch.float64, device=dev)      # poisoned: may hold anything on entry
        assert gm.routed == 2 and gm.owns(out) and gm.owns(ws)
        _lib.check(L.trajsde_grad_norm_clip(t["grad_in"].data_ptr(), n, MAX_NORM, ws.data_ptr(), need, out.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "norm")
        torch.cuda.synchronize()
        pair = out.clone()                                                    # `coef` is an input of the step: it must come back unchanged
        _lib.check(L.trajsde_adamw_step_clipped(t["param"].data_ptr(), t["grad"].data_ptr(), t["exp_avg"].data_ptr(),
                                                t["exp_avg_sq"].data_ptr(), n, *SCALARS, out.data_ptr() + 4,
                                                torch.cuda.current_stream().cuda_stream), "step")
        torch.cuda.synchronize()
        rep = gm.check()
        assert rep.ok, f"n={n} poison={poison}\n{rep}"                        # guards intact, grad_in unchanged
        assert torch.equal(out.view(torch.int32), pair.view(torch.int32)), poison
        assert torch.equal(out.view(torch.int32), plain_out.view(torch.int32)), (poison, out, plain_out)
        for k in ("grad", "param", "exp_avg", "exp_avg_sq"):
            assert torch.equal(t[k].view(torch.int32), plain[k].view(torch.int32)), (poison, k)
