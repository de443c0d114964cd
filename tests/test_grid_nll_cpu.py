"""The vanilla HiVT variant under the Laplace NLL (losses/laplace_nll_loss.py), the parts that need no GPU: the parameter table and
image size of TRAJSDE_STAGE_DECODER_MLP_NLL_BWD, the parameters the loss reaches, the loss routing of `training_step`, and the
float64 yardstick of the GPU tests (tests/grid_nll_restate.py) against the reference's own training step
(tests/golden/train_grid_nll, tools/make_golden_grid_nll.py)."""
import pytest
import torch

import grid_nll_restate as G
import helpers as H

SCALE = ["scale.0.weight", "scale.0.bias", "scale.1.weight", "scale.1.bias", "scale.3.weight", "scale.3.bias"]


def _names(lib, stage, nl, K):
    return [lib.trajsde_param_name(stage, i, nl, K).decode() for i in range(lib.trajsde_param_count(stage, nl, K))]


@pytest.mark.parametrize("T", [12, 30, 64])
def test_mlp_nll_stage_is_the_l2_table_plus_the_scale_head(T):
    from trajsde_amd import _lib
    from trajsde_amd.models.model_base_mix import PredictionModel
    lib = _lib.lib()
    assert _lib.STAGE_DECODER_MLP_NLL_BWD == 12
    l2 = _names(lib, _lib.STAGE_DECODER_MLP_BWD, T, 6)
    nll = _names(lib, _lib.STAGE_DECODER_MLP_NLL_BWD, T, 6)
    assert nll == l2 + SCALE
    model = PredictionModel(**H.grid_cfg(6, T, 4, 2), init_seed=0)
    dec = dict(model.decoder.named_parameters())
    assert all(n in dec for n in nll) and not any(n.startswith("pi.") for n in nll)
    image = lib.trajsde_blob_floats(_lib.STAGE_DECODER_MLP_NLL_BWD, T, 6) - lib.trajsde_blob_floats(_lib.STAGE_DECODER_MLP_BWD, T, 6)
    # one MlpHeadBwdL image: the forward fields (W0, b0, gamma, beta, W3 and b3 padded to 128 outputs) + W3^T (64 x 128) + W0^T
    assert image == 64 * 64 + 3 * 64 + 128 * 64 + 128 + 64 * 128 + 64 * 64 == 24896


def test_params_with_gradient_follow_the_configured_loss():
    from trajsde_amd.models.model_base_mix import PredictionModel
    l2 = PredictionModel(**H.grid_cfg(3, 12, 4, 2), init_seed=0)
    nll = PredictionModel(**G.nll_cfg(3, 12, 4, 2), init_seed=0)
    name_of = {}
    for m in (l2, nll):
        name_of.update({id(p): n for n, p in m.named_parameters()})
    got_l2 = [name_of[id(p)] for p in l2.params_with_gradient()]
    got_nll = [name_of[id(p)] for p in nll.params_with_gradient()]
    # L2: what it was -- every parameter but the decoder's pi and scale heads (and the AL encoder's unused embeddings)
    assert not any(n.startswith(("decoder.pi.", "decoder.scale.")) for n in got_l2)
    assert any(n.startswith("decoder.loc.") for n in got_l2)
    # Laplace NLL: the same list plus every scale-head parameter, in named_parameters() order; pi still unreached
    assert set(got_nll) == set(got_l2) | {"decoder." + n for n in SCALE}
    assert got_nll == [n for n, _ in nll.named_parameters() if n in set(got_nll)]
    assert not any(n.startswith("decoder.pi.") for n in got_nll)


@pytest.mark.parametrize("modules", [["L2", "LaplaceNLLLoss"], ["LaplaceNLLLoss", "L2"], ["DiffBCE"], ["L2", "DiffBCE"]])
def test_training_step_refuses_other_loss_sets_before_any_gpu_work(modules):
    from trajsde_amd.models.model_base_mix import PredictionModel
    from trajsde_amd.synth import synth
    cfg = H.grid_cfg(3, 12, 4, 2)
    cfg["losses"] = ["trajsde_amd/losses.py"] * len(modules)
    cfg["losses_module"] = list(modules)
    cfg["loss_weights"] = [1] * len(modules)
    cfg["loss_args"] = [{} for _ in modules]
    model = PredictionModel(**cfg, init_seed=0)
    model.ts_drop = 0.3
    batch = synth(S=2, n=6, L=4, F=12, box=70.0, seed=5, mixed_source=True)
    x0, pad0 = batch.x.clone(), batch.padding_mask.clone()
    with pytest.raises(NotImplementedError, match="ONE regression loss"):
        model.training_step(batch, 0)                          # CPU tensors: any kernel launch would fail differently
    assert torch.equal(batch.x, x0) and torch.equal(batch.padding_mask, pad0)       # refused before touching the batch


def test_nll_yardstick_matches_the_reference_loss_class_and_the_kernels_closed_form():
    """the yardstick's loss (helpers.reference_laplace_nll) against what losses/laplace_nll_loss.py returned
    (tests/golden/reference_calls/laplace_nll.npz), and its gradient against the closed form the kernels use"""
    ref = H.load_reference_call("laplace_nll")
    y, loc4, mask = ref["in.y"].double(), ref["in.loc"].double(), ref["in.reg_mask"].bool()
    val, best = H.reference_laplace_nll(y, loc4, mask)
    assert abs(float(val) - float(ref["out.value"])) <= 1e-6 * max(1.0, abs(float(ref["out.value"])))
    loc4 = loc4.clone().requires_grad_(True)
    H.reference_laplace_nll(y, loc4, mask)[0].backward()
    rows = torch.arange(best.numel())
    l, s = loc4.detach()[best, rows, :, :2], loc4.detach()[best, rows, :, 2:].clamp(min=1e-6)
    n = 2 * int(mask.sum())
    m = mask.unsqueeze(-1).double()
    want_l = -torch.sign(y - l) / s / n * m
    want_s = (1 / s - (y - l).abs() / s ** 2) / n * m
    got = loc4.grad[best, rows]
    assert torch.allclose(got[..., :2], want_l, rtol=1e-12, atol=1e-15) and torch.allclose(got[..., 2:], want_s, rtol=1e-12, atol=1e-15)
    others = torch.ones(loc4.shape[:2], dtype=torch.bool)
    others[best, rows] = False
    assert float(loc4.grad[others].abs().max()) == 0.0         # only the winning mode carries gradient


def test_oracle_autograd_matches_the_reference_nll_training_step_of_the_vanilla_variant():
    """the float64 yardstick of tests/test_gpu_grid_nll.py against the reference's own model, Laplace NLL module and torch.autograd"""
    from trajsde_amd.models.model_base_mix import PredictionModel
    batch, meta, losses, weights, grads, digests = G.load_fixture()
    assert set(losses) == {"LaplaceNLLLoss", "total"} and weights == {"LaplaceNLLLoss": 1.0}
    assert any(k.startswith("decoder.scale.") for k in digests) and not any(k.startswith("decoder.pi.") for k in digests)
    cfg = G.nll_cfg(int(meta["num_modes"]), int(meta["future_steps"]), int(meta["num_heads"]), int(meta["num_temporal_layers"]))
    model = PredictionModel(**cfg, init_seed=int(meta["init_seed"]))
    H.perturb_parameters(model, int(meta["perturb_seed"]))
    checksum = float(sum(v.double().abs().sum() for v in model.state_dict().values() if torch.isfinite(v).all()))   # (the generator's)
    assert abs(checksum - meta["state_checksum"]) <= 1e-6 * meta["state_checksum"]
    total, got = G.oracle_grid_nll_grads(model, cfg, batch, float(meta["nll_eps"]))
    assert abs(total - losses["total"]) <= 2e-6 * max(1.0, abs(losses["total"]))
    assert all(got["decoder." + n] is not None and float(got["decoder." + n].abs().max()) > 0 for n in SCALE)
    bad = H.check_grads_against_train_fixture(got, grads, digests, rel=2e-5)
    assert not bad, bad[:8]


def test_nll_backward_refuses_a_decoder_without_scale_head():
    """`uncertain: False` builds no scale head: the Laplace NLL has nothing to read its scales from (refused before any GPU work)"""
    from trajsde_amd import _lib
    from trajsde_amd.models.model_base_mix import PredictionModel
    model = PredictionModel(**H.grid_cfg(3, 12, 4, 2, uncertain=False), init_seed=0)
    with pytest.raises(_lib.TrajsdeError, match="uncertain: False"):
        model.decoder._rt.mlp_decoder_nll_backward({}, torch.zeros(5, 64), torch.zeros(3, 5, 64), {})
