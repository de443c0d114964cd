"""trajsde_mlp_decoder_cotangent_backward inside the red-zone arenas of tests/guarded_memory.py (-m gpu): every input in an arena of
its own, every output, gradient buffer and the workspace routed into arenas.  For K * N one below, at and one above a multiple of 16
rows (N = 15, 16, 17 with K = 3, T = 12) and for 2T = 66 outputs a head (T = 33): every guard byte intact, the inputs unwritten, and the
results bit-identical whether the workspace and the outputs started as NaN, as zeros or as random bits."""
import pytest
import torch

import guarded_memory as GM
import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    return torch.device("cuda:0")


def test_every_grid_extension_entry_point_is_a_size_query_or_runs_in_these_arenas():
    """the accounting of tests/test_gpu_memory_contract.py for `_lib.GRID_EXT_SIGNATURES`: every symbol is a `*_bytes` size query or
    the one launch entry point the arenas below are built around"""
    from trajsde_amd import _lib
    launches = {n for n in _lib.GRID_EXT_SIGNATURES if not n.endswith("_bytes")}
    assert launches == {"trajsde_mlp_decoder_cotangent_backward"}


@pytest.mark.parametrize("N,T", [(15, 12), (16, 12), (17, 12), (17, 33)])
def test_mlp_cotangent_backward_stays_inside_its_buffers(N, T, dev):
    from trajsde_amd import _lib
    from trajsde_amd.models.model_base_mix import PredictionModel
    from trajsde_amd.synth import synth
    K = 3
    model = PredictionModel(**H.grid_cfg(K, T, 4, 2), init_seed=21).eval()
    H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
    model = model.to(dev)
    rt = model.decoder._rt
    batch = synth(S=1, n=N, L=4, F=T, box=60.0, seed=40 + N).to(dev)
    g = torch.Generator().manual_seed(7 + N + T)
    host = dict(local=torch.randn(N, 64, generator=g), glob=torch.randn(K, N, 64, generator=g), d_loc=torch.randn(K, N, T, 4, generator=g),
                d_pi=torch.randn(N, K, generator=g))
    with torch.no_grad():
        fwd = rt.mlp_decoder_forward(batch, host["local"].to(dev), host["glob"].to(dev))
    rt.blob(_lib.STAGE_DECODER_MLP_COT_BWD)                               # the weight image is packed outside the arenas, once
    torch.cuda.synchronize()
    base = None
    for fill, poison in (("A", "nan"), ("B", "zero"), ("A", 7)):
        gm = GM.GuardedMemory(poison=poison)
        t = {k: gm.placed(v.to(dev), fill, label=k) for k, v in host.items()}
        out = {"loc": gm.placed(fwd["loc"], fill, label="loc"), "reg_mask": fwd["reg_mask"]}
        calls = []
        real = _lib.lib().trajsde_mlp_decoder_cotangent_backward
        _lib.lib().trajsde_mlp_decoder_cotangent_backward = lambda *a: (calls.append(1), real(*a))[1]
        try:
            with gm:
                res = rt.mlp_decoder_cotangent_backward(batch, t["local"], t["glob"], out, t["d_loc"], t["d_pi"])
        finally:
            _lib.lib().trajsde_mlp_decoder_cotangent_backward = real
        assert calls == [1]
        torch.cuda.synchronize()
        outs = dict(res["grads"])
        outs.update(d_local_embed=res["d_local_embed"], d_global_embed=res["d_global_embed"])
        assert gm.routed >= 4                                            # gradient buffers, d_local, d_global, the workspace
        assert gm.owns(res["d_local_embed"]) and gm.owns(res["d_global_embed"]) and gm.owns(res["grads"].flat)
        rep = gm.check()
        assert rep.ok, f"N={N} T={T} poison={poison}\n{rep}"             # guards intact, placed inputs unchanged
        assert all(bool(torch.isfinite(v).all()) for v in outs.values()), poison
        cur = {k: v.clone() for k, v in outs.items()}
        if base is None:
            base = cur
            assert float(cur["pi.6.weight"].abs().max()) > 0 and float(cur["d_local_embed"].abs().max()) > 0
        else:
            assert [k for k in base if not torch.equal(base[k], cur[k])] == [], poison
