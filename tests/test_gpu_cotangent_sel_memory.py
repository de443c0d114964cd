"""trajsde_decoder_cotangent_backward_sel inside the red-zone arenas of tests/guarded_memory.py (-m gpu), as
tests/test_gpu_cotangent_memory.py holds the dense entry point: every input in an arena of its own, every output, gradient buffer, the
two status words and the workspace routed into arenas.  For K * N = 45, 48, 51 (N = 15, 16, 17 with K = 3), T = 5: every guard byte
intact, the inputs unwritten, and the results bit-identical whether the workspace, the outputs and `status` started as NaN, as zeros or
as random bits -- and once more with a cotangent that breaks the one-mode-per-actor premise."""
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


def test_every_entry_point_of_the_table_is_a_size_query_or_runs_in_these_arenas():
    from trajsde_amd import _lib
    launches = {n for n in _lib.COT_SEL_EXT_SIGNATURES if not n.endswith("_bytes")}
    assert launches == {"trajsde_decoder_cotangent_backward_sel"}


@pytest.mark.parametrize("N", [15, 16, 17])
def test_winner_backward_stays_inside_its_buffers(N, dev):
    import test_gpu_cotangent_sel as S
    from trajsde_amd import _lib, runtime
    from trajsde_amd.schedule import decoder_schedule
    from trajsde_amd.synth import synth
    K, T, max_t = 3, 5, 0.5
    model, _ = H.build_model(K, T, max_t, init_seed=21)
    H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
    model = model.to(dev)
    rt = model.decoder._rt
    batch = synth(S=1, n=N, L=4, F=T, box=60.0, seed=40 + N).to(dev)
    g = torch.Generator().manual_seed(7 + N)
    sched = decoder_schedule(T, max_t, 0.1)
    host = dict(local=torch.randn(N, 64, generator=g), glob=torch.randn(K, N, 64, generator=g),
                z=torch.randn(sched.n_euler, K * N, 64, generator=g), d_pi=torch.randn(N, K, generator=g))
    with torch.no_grad():
        fwd = rt.decoder_forward(batch, host["local"].to(dev), host["glob"].to(dev), runtime.NoiseSpec(z_dec=host["z"].to(dev)))
    d_loc, best, valid = S.wta_cotangent(batch, fwd, "nll", seed=9 + N)    # one mode per actor, loc and scale channels
    assert bool(valid.all())
    case = dict(d_loc=d_loc, best=best, valid=valid)
    broken, actor, lowest = S.violate(case, actor=N - 1)                   # the last row of the last tile: two supported modes
    rt.blob()                                                             # the weight images are packed outside the arenas, once
    rt.blob(_lib.STAGE_DECODER_COT_BWD)
    torch.cuda.synchronize()
    base = None
    for fill, poison, cot in (("A", "nan", d_loc), ("B", "zero", d_loc), ("A", 7, d_loc), ("B", "nan", broken)):
        gm = GM.GuardedMemory(poison=poison)
        t = {k: gm.placed(v.to(dev), fill, label=k) for k, v in dict(host, d_loc=cot).items()}
        out = {"loc": gm.placed(fwd["loc"], fill, label="loc"), "reg_mask": fwd["reg_mask"]}
        calls = []
        real = _lib.lib().trajsde_decoder_cotangent_backward_sel
        _lib.lib().trajsde_decoder_cotangent_backward_sel = lambda *a: (calls.append(1), real(*a))[1]
        try:
            with gm:
                res = rt.decoder_cotangent_backward(batch, t["local"], t["glob"], out, runtime.NoiseSpec(z_dec=t["z"]), t["d_loc"], t["d_pi"],
                                                    support="winner")
        finally:
            _lib.lib().trajsde_decoder_cotangent_backward_sel = real
        assert calls == [1]
        torch.cuda.synchronize()
        outs = dict(res["grads"])
        outs.update(d_local_embed=res["d_local_embed"], d_global_embed=res["d_global_embed"], status=res["support_status"],
                    mode=res["support_mode"])
        assert gm.routed >= 5                                            # gradient buffers, d_local, d_global, status, the workspace
        assert gm.owns(res["d_local_embed"]) and gm.owns(res["d_global_embed"]) and gm.owns(res["grads"].flat)
        assert gm.owns(res["support_status"]) and gm.owns(res["support_mode"])
        rep = gm.check()
        assert rep.ok, f"N={N} poison={poison}\n{rep}"                   # guards intact, placed inputs unchanged
        assert all(bool(torch.isfinite(v).all()) for v in outs.values() if v.is_floating_point()), poison
        cur = {k: v.clone() for k, v in outs.items()}
        if cot is broken:
            assert cur["status"].tolist() == [1, N] and int(cur["mode"][actor]) == lowest
        elif base is None:
            base = cur
            assert cur["status"].tolist() == [0, N] and torch.equal(cur["mode"].long(), best)
            assert float(cur["pi.3.weight"].abs().max()) > 0 and float(cur["scale.3.weight"].abs().max()) > 0
            assert float(cur["d_local_embed"].abs().max()) > 0
        else:
            assert [k for k in base if not torch.equal(base[k], cur[k])] == [], poison
