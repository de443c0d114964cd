"""CPU suite of training the decoder's `method: milstein` (trajsde_decoder_*_backward_milstein, csrc/decoder_mil_bwd.hip): the
float64 gradient oracle (tests/milstein_grad_restate.py) against the forward restatement and finite differences, the reverse sweep's
closed form against autograd, how far the Milstein gradients lie from the Euler ones at the GPU tests' weights, the new C-ABI
entries and stage tables, and the new kernels' listing (no scratch)."""
import os
import re
import subprocess

import pytest
import torch

import helpers as H
import milstein_grad_restate as MG
import milstein_restate as MR

DEC_SHAPES = MG.DEC_SHAPES
G_TENSORS = ("lsde_func.g_func.net.0.weight", "lsde_func.g_func.net.2.weight", "lsde_func.g_func.net.4.weight")


def _random_gfunc(seed, rows=9):
    g = torch.Generator().manual_seed(seed)
    d = torch.float64
    P = {"g.net.0.weight": torch.randn(64, 66, generator=g, dtype=d) * 0.3, "g.net.0.bias": torch.randn(64, generator=g, dtype=d) * 0.2,
         "g.net.2.weight": torch.randn(64, 64, generator=g, dtype=d) * 0.3, "g.net.2.bias": torch.randn(64, generator=g, dtype=d) * 0.2,
         "g.net.4.weight": torch.randn(1, 64, generator=g, dtype=d) * 0.5, "g.net.4.bias": torch.randn(1, generator=g, dtype=d) * 0.2}
    y, u, I = (torch.randn(rows, 64, generator=g, dtype=d) for _ in range(3))
    return P, y, u, 0.3 * I


def test_closed_form_of_the_gdg_vjp_matches_autograd():
    """section 1 of the design (decoder_mil_bwd.hip k_sde_bwd_mil): the gradient of Psi = u . gdg w.r.t. y and GFunc's six tensors,
    u held fixed, against double backward through torchsde's create_graph vjp"""
    for seed in (3, 4):
        P, y, u, I = _random_gfunc(seed)
        dt = 0.1
        got = MG.closed_form_step_vjp(P, "g", y, u, I, dt, 0.3, -0.9)
        for v in P.values():
            v.requires_grad_(True)
        yy = y.clone().requires_grad_(True)
        _, gdg = MG.gdg_graph(P, "g", yy, 0.3, -0.9, 0.5 * (I ** 2 - dt))
        names = [k for k in got if k != "y"]
        want = torch.autograd.grad((u * gdg).sum(), [yy] + [P["g." + k] for k in names])
        assert float((want[0] - got["y"]).abs().max()) <= 1e-12
        for k, w in zip(names, want[1:]):
            assert w.shape == got[k].shape, k
            assert float((w - got[k]).abs().max()) <= 1e-12 * max(1.0, float(w.abs().max())), k


def _stage_case(S, n, K, T, max_t, kw, strength, seed=300, init_seed=11, noise_seed=91):
    """(model, cfg, batch, local, glob, y_rot) of a stage case on the host: the oracle's fp32 encoder and interactor outputs"""
    from trajsde_amd.synth import synth
    batch = synth(S=S, n=n, L=6, F=T, box=80.0, seed=seed + n, **kw)
    model, cfg = H.build_model(K, T, max_t, init_seed=init_seed)
    if strength:
        H.trained_like_parameters(model, H.TRAINED_SEED, strength)
    out = H.oracle_forward(model, cfg, batch, noise_seed=noise_seed, want_intermediates=True)
    return model, cfg, batch, out["local_embed"], out["global_embed"], out["y"]


def test_grad_restatement_forward_equals_the_milstein_restatement():
    import restate
    from trajsde_amd.schedule import decoder_schedule
    for (S, n, K, T, max_t, kw) in DEC_SHAPES[:2]:
        model, cfg, batch, local, glob, _ = _stage_case(S, n, K, T, max_t, kw, 1.0)
        c = restate.flat_cfg(cfg)
        P = {k: v.detach().double() for k, v in model.state_dict().items() if v.is_floating_point()}
        sched = decoder_schedule(T, max_t, c["min_stepsize"])
        noise = H.NoiseAs(restate.PhiloxNoise(91), torch.float64)
        want = MR.sde_decoder(P, c, batch, local.double(), glob.double(), noise, sched)
        got = {k: v.detach() for k, v in MG.sde_decoder(P, c, batch, local.double(), glob.double(), noise, sched).items()}
        assert float((got["loc"] - want["loc"]).abs().max()) <= 1e-12
        assert float((got["pi"] - want["pi"]).abs().max()) <= 1e-12
        euler = MG.sde_decoder(P, c, batch, local.double(), glob.double(), noise, sched, method="euler")
        ref = restate.sde_decoder({k: v for k, v in P.items()}, c, batch, local.double(), glob.double(), noise, sched)
        assert float((euler["loc"] - ref["loc"]).abs().max()) <= 1e-12


def test_grad_restatement_passes_a_finite_difference_check():
    """torch.autograd.gradcheck (float64) of a tiny Milstein decode w.r.t. GFunc's six tensors and local_embed"""
    import restate
    from trajsde_amd.schedule import decoder_schedule
    K, T, max_t = 2, 5, 0.5
    model, cfg = H.build_model(K, T, max_t, init_seed=3)
    H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
    c = restate.flat_cfg(cfg)
    P = {k: v.detach().double() for k, v in model.state_dict().items() if v.is_floating_point()}
    with torch.no_grad():
        P["decoder.lsde_func.g_func.net.4.weight"] *= 4.0                   # a gdg term well above the finite differences' noise
    sched = decoder_schedule(T, max_t, c["min_stepsize"])
    g = torch.Generator().manual_seed(8)
    local, glob = torch.randn(3, 64, generator=g, dtype=torch.float64), torch.randn(K, 3, 64, generator=g, dtype=torch.float64)
    noise = H.NoiseAs(restate.PhiloxNoise(5), torch.float64)
    names = [k for k in P if k.startswith("decoder.lsde_func.g_func.")]
    assert len(names) == 6

    def fn(lo, *tensors):
        Q = dict(P)
        Q.update(zip(names, tensors))
        return MG.sde_decoder(Q, c, None, lo, glob, noise, sched)["loc"]
    inputs = [local.clone().requires_grad_(True)] + [P[k].clone().requires_grad_(True) for k in names]
    assert torch.autograd.gradcheck(fn, inputs, eps=1e-6, atol=1e-7, rtol=1e-5, fast_mode=True)


@pytest.mark.parametrize("strength", MG.STRENGTHS)
@pytest.mark.parametrize("S,n,K,T,max_t,kw", DEC_SHAPES)
def test_milstein_gradients_are_far_from_euler_at_the_gpu_tests_weights(S, n, K, T, max_t, kw, strength):
    """at the GPU stage tests' weights the float64 Milstein gradients of GFunc's three matrices and of local_embed lie at least
    20 x the backward bound (helpers.BACKWARD_REL of the tensor's max) from those of the Euler decoder (same noise) and from those of
    the Milstein decoder with the gdg term cut from the graph: a backward that ran Euler's sweep, or ignored the second-order term,
    fails those tests"""
    model, cfg, batch, local, glob, y_rot = _stage_case(S, n, K, T, max_t, kw, strength)
    _, best_m, mil, dl_m, _ = MG.oracle_decoder_grads(model, cfg, batch, local, glob, y_rot, 91)
    _, _, eul, dl_e, _ = H.oracle_decoder_grads(model, cfg, batch, local, glob, y_rot, 91)
    _, best_d, det, dl_d, _ = MG.oracle_decoder_grads(model, cfg, batch, local, glob, y_rot, 91, gdg_detached=True)
    assert torch.equal(best_m, best_d)                                         # (the same forward)
    mil["d_local_embed"], eul["d_local_embed"], det["d_local_embed"] = dl_m, dl_e, dl_d
    for k in G_TENSORS + ("d_local_embed",):
        bound = H.BACKWARD_REL * float(mil[k].abs().max())
        assert float((eul[k] - mil[k]).abs().max()) >= 20 * bound, k
        assert float((det[k] - mil[k]).abs().max()) >= 20 * bound, k


def test_milstein_backward_symbols_are_exported_and_declared():
    from trajsde_amd import _lib
    header = open(os.path.join(H.ROOT, "include", "trajsde_hip.h")).read()
    lib = _lib.lib()
    for name in ("trajsde_decoder_milstein_backward_ws_bytes", "trajsde_decoder_l2_backward_milstein",
                 "trajsde_decoder_nll_backward_milstein"):
        assert name in _lib.SIGNATURES and re.search(r"\b" + name + r"\s*\(", header), name
        assert getattr(lib, name) is not None
    assert "TRAJSDE_STAGE_DECODER_MILSTEIN_BWD = 13" in header and "TRAJSDE_STAGE_DECODER_MILSTEIN_NLL_BWD = 14" in header
    assert (_lib.STAGE_DECODER_MILSTEIN_BWD, _lib.STAGE_DECODER_MILSTEIN_NLL_BWD) == (13, 14)
    for N, K, T, n_euler in ((37, 6, 20, 20), (500, 10, 60, 60)):
        mil = lib.trajsde_decoder_milstein_backward_ws_bytes(N, K, T, n_euler)
        assert mil > lib.trajsde_decoder_nll_backward_ws_bytes(N, K, T, n_euler) > lib.trajsde_decoder_backward_ws_bytes(N, K, T, n_euler)


def test_milstein_backward_stage_tables_are_the_euler_tables():
    from trajsde_amd import _lib
    lib = _lib.lib()

    def names(stage):
        return [lib.trajsde_param_name(stage, i, 0, 6).decode() for i in range(lib.trajsde_param_count(stage, 0, 6))]
    for mil, euler in ((_lib.STAGE_DECODER_MILSTEIN_BWD, _lib.STAGE_DECODER_BWD),
                       (_lib.STAGE_DECODER_MILSTEIN_NLL_BWD, _lib.STAGE_DECODER_NLL_BWD)):
        assert names(mil) == names(euler) and len(names(mil)) > 0
        assert lib.trajsde_blob_floats(mil, 0, 6) == lib.trajsde_blob_floats(euler, 0, 6) + 2 * 64 * 64


@pytest.mark.parametrize("extra", [[], ["-DTSDE_SPLIT_H3=0"]])
def test_milstein_backward_kernels_compile_without_scratch(tmp_path, extra):
    """the Milstein replay and sweep (fp16x3 and bf16x6 builds) hold their state, GFunc's activations and the tangent pass in registers"""
    from trajsde_amd import build
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    out = tmp_path / "decoder_mil_bwd.s"
    src = os.path.join(H.ROOT, "trajsde_amd", "csrc", "decoder_mil_bwd.hip")
    subprocess.check_call([build.HIPCC, *flags, *extra, "--cuda-device-only", "-S", "-o", str(out), src],
                          stderr=subprocess.DEVNULL)
    text = out.read_text()
    kernels = re.findall(r"^(_ZN4tsde\d+k_(?:sde_replay_mil|sde_bwd_mil|add_mil_wgrad)\w+):.*?; ScratchSize: (\d+)", text,
                         flags=re.S | re.M)
    assert len(kernels) == 3, kernels
    assert all(int(sz) == 0 for _, sz in kernels), kernels
