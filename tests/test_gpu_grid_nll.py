"""GPU parity (-m gpu) of the vanilla HiVT variant trained under the Laplace NLL (losses/laplace_nll_loss.py): the MLP decoder's
backward entry point (trajsde_mlp_decoder_nll_backward, both heads) against float64 autograd, the whole training step against
whole-model float64 autograd and against the reference's own training step (tests/golden/train_grid_nll), reproducibility in
train mode, and a short training run.  Tolerances as in tests/test_gpu_grid.py."""
import pytest
import torch

import grid_nll_restate as G
import helpers as H

pytestmark = pytest.mark.gpu
SCALE = ["scale.0.weight", "scale.0.bias", "scale.1.weight", "scale.1.bias", "scale.3.weight", "scale.3.bias"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _close(got, want, what):
    scale = float(want.abs().max())
    err = float((got.detach().cpu().double() - want.double()).abs().max())
    assert err <= 2e-4 * scale + 1e-7, (what, err, scale)


def _pad_future(batch, T, seed, empty_every=0):
    """pad a quarter of the future steps at random (reg_mask = ~padding_mask[:, -T:]); `empty_every`: every that many actors lose
    all their future steps"""
    g = torch.Generator().manual_seed(seed)
    batch.padding_mask[:, -T:] |= torch.rand(batch.padding_mask.shape[0], T, generator=g) < 0.25
    if empty_every:
        batch.padding_mask[::empty_every, -T:] = True
    return batch


def _decoder_case(dev, S, n, K, T, seed, empty_every=0):
    """a perturbed vanilla model's forward on a mixed-source batch with padded history and future steps"""
    from trajsde_amd.models.model_base_mix import PredictionModel
    from trajsde_amd.synth import synth
    batch = _pad_future(synth(S=S, n=n, L=5, F=T, box=80.0, seed=seed, mixed_source=True, history_dropout=0.3), T, seed, empty_every)
    cfg = G.nll_cfg(K, T, 4, 2)
    model = PredictionModel(**cfg, init_seed=3)
    H.perturb_parameters(model, 500 + seed)
    model = model.to(dev)
    data = batch.to(dev)
    with torch.no_grad():
        out = model(data)                                           # rotates data.y
    return model, cfg, batch, data, out


@pytest.mark.parametrize("S,n,K,T,empty", [(3, 14, 3, 12, 0), (2, 21, 6, 30, 0), (2, 21, 10, 60, 0), (2, 9, 4, 64, 0),
                                           (3, 12, 6, 30, 4)])
def test_mlp_decoder_nll_backward_matches_autograd(S, n, K, T, empty, dev):
    import restate_grid
    model, cfg, batch, data, out = _decoder_case(dev, S, n, K, T, 810 + n + K, empty)
    local, glob = out["local_embed"], out["global_embed"]
    reg_mask = out["reg_mask"].cpu()
    assert bool((~reg_mask).any()) and (not empty or bool((~reg_mask.any(-1)).any()))       # padded steps; actors with none valid
    res = model.decoder._rt.mlp_decoder_nll_backward(data, local, glob, out)
    torch.cuda.synchronize()
    c = restate_grid.flat_cfg(cfg)
    P = {k: v.detach().cpu().double().clone() for k, v in model.state_dict().items()}
    names = [k for k in P if k.startswith("decoder.")]
    for k in names:
        P[k].requires_grad_(True)
    lo = local.detach().cpu().double().clone().requires_grad_(True)
    gl = glob.detach().cpu().double().clone().requires_grad_(True)
    with torch.enable_grad():
        o = restate_grid.mlp_decoder(P, c, batch, lo, gl)
        loss, best = H.reference_laplace_nll(data.y.cpu().double(), o["loc"], reg_mask, 1e-6)
        loss.backward()
    assert torch.equal(res["best_mode"].cpu().long(), best)
    assert abs(float(res["loss"]) - float(loss.detach())) <= 1e-5 * max(1.0, abs(float(loss.detach())))
    got = res["grads"]
    from trajsde_amd import _lib
    assert list(got) == model.decoder._rt.param_names(_lib.STAGE_DECODER_MLP_NLL_BWD) and len(got) == 16
    assert not any(k.startswith("pi.") for k in got)
    for k in names:
        short = k[len("decoder."):]
        want = P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])
        if short not in got:
            assert short.startswith("pi.") and float(want.abs().max()) == 0.0, k
            continue
        _close(got[short], want, k)
    for s in SCALE:
        assert float(got[s].abs().max()) > 0, s
    _close(res["d_local_embed"], lo.grad, "d_local_embed")
    _close(res["d_global_embed"], gl.grad, "d_global_embed")


@pytest.mark.parametrize("empty", [False, True])
def test_mlp_nll_loss_convention_is_the_sde_decoders(empty, dev):
    """the loss of trajsde_mlp_decoder_nll_backward and of trajsde_decoder_nll_backward on the same loc, y and mask tensors is the same
    number; with no valid step at all both give 0 and the MLP decoder's gradients are all zero"""
    from trajsde_amd import runtime
    K, T = 6, 30
    model, cfg, batch, data, out = _decoder_case(dev, 2, 15, K, T, 77)
    if empty:
        out["reg_mask"][:] = False
    local, glob = out["local_embed"], out["global_embed"]
    mlp = model.decoder._rt.mlp_decoder_nll_backward(data, local, glob, out)
    sde_model, _ = H.build_model(K, T, 3.0, init_seed=1)
    sde_model = sde_model.to(dev)
    sde = sde_model.decoder._rt.decoder_nll_backward(data, local, glob, out, runtime.NoiseSpec(seed=0))
    torch.cuda.synchronize()
    assert float(mlp["loss"]) == float(sde["loss"])
    assert torch.equal(mlp["best_mode"], sde["best_mode"])
    if empty:
        assert float(mlp["loss"]) == 0.0
        for k, g in mlp["grads"].items():
            assert float(g.abs().max()) == 0.0, k
        assert float(mlp["d_local_embed"].abs().max()) == 0.0 and float(mlp["d_global_embed"].abs().max()) == 0.0
    else:
        assert float(mlp["loss"]) != 0.0


def test_nll_training_step_matches_end_to_end_autograd(dev):
    from trajsde_amd.losses import LaplaceNLLLoss
    from trajsde_amd.models.model_base_mix import PredictionModel
    from trajsde_amd.synth import synth
    K, T = 3, 12
    batch = _pad_future(synth(S=3, n=11, L=6, F=T, box=70.0, seed=91, mixed_source=True, history_dropout=0.3), T, 91)
    cfg = G.nll_cfg(K, T, 4, 2)
    model = PredictionModel(**cfg, init_seed=7)
    # a perturbation whose ReLU inputs all keep >= 3e-6 from zero (float64 oracle): one within float32 rounding of zero is a kink
    # whose two one-sided gradients differ by that unit's whole contribution (oracle/make_golden_train.py GRID_KINK_MARGIN)
    H.perturb_parameters(model, 4335)
    model = model.to(dev).train()
    data = batch.to(dev)
    loss = model.training_step(data, 0)
    loss.backward()
    torch.cuda.synchronize()
    assert set(model.last_losses) == {"LaplaceNLLLoss"} and "train/LaplaceNLLLoss" in model.logged
    value = float(LaplaceNLLLoss(eps=1e-6)(data, model.last_output))
    assert abs(float(loss.detach()) - value) <= 1e-5 * max(1.0, abs(value))
    want_loss, want = G.oracle_grid_nll_grads(model, cfg, batch)
    assert abs(float(loss.detach()) - want_loss) <= 1e-5 * max(1.0, abs(want_loss))
    reached = {id(p) for p in model.params_with_gradient()}
    bad = []
    for n, p in model.named_parameters():
        if id(p) not in reached:
            assert p.grad is None, n
            assert want[n] is None or float(want[n].abs().max()) == 0.0, n
            continue
        w = want[n]
        scale = float(w.abs().max())
        err = float((p.grad.cpu().double() - w).abs().max())
        zero_by_symmetry = n.endswith("lin_k.bias") or n.endswith("lin_k_node.bias") or n.endswith("lin_k_edge.bias")
        if (err > 5e-5 or scale > 5e-5) if zero_by_symmetry else (err > 2e-4 * scale + 1e-7):
            bad.append((n, err, scale))
    assert not bad, bad
    for s in SCALE:
        assert float(dict(model.named_parameters())["decoder." + s].grad.abs().max()) > 0, s
    assert all(p.grad is None for n, p in model.named_parameters() if n.startswith("decoder.pi."))


def test_nll_training_step_matches_the_reference_training_step(dev):
    """loss and parameter-gradient digests of the HIP training step against the REFERENCE's vanilla model, losses/laplace_nll_loss.py
    and torch.autograd (tests/golden/train_grid_nll/grid_nll_k3_t12_h4.npz, tools/make_golden_grid_nll.py; dropout off)"""
    from trajsde_amd.models.model_base_mix import PredictionModel
    batch, meta, losses, weights, grads, digests = G.load_fixture()
    cfg = G.nll_cfg(int(meta["num_modes"]), int(meta["future_steps"]), int(meta["num_heads"]), int(meta["num_temporal_layers"]),
                    eps=float(meta["nll_eps"]))
    model = PredictionModel(**cfg, init_seed=int(meta["init_seed"]))
    H.perturb_parameters(model, int(meta["perturb_seed"]))
    model = model.to(dev).train()
    loss = model.training_step(batch.to(dev), 0)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - losses["total"]) <= 1e-5 * max(1.0, abs(losses["total"]))
    got = {n: p.grad for n, p in model.named_parameters()}
    assert all(got["decoder." + s] is not None for s in SCALE)
    bad = H.check_grads_against_train_fixture(got, grads, digests, rel=2e-4)
    assert not bad, bad[:8]


def test_nll_training_step_in_train_mode_repeated_is_bitwise_identical(dev):
    """dropout 0.1 and ts_drop on, one batch of 24 scenes x 64 agents, the same keys (and the same ts_drop draw): the same loss bits,
    output and gradient words on every call -- test_vanilla_training_step_repeated_is_bitwise_identical under the Laplace NLL"""
    from trajsde_amd import runtime
    from trajsde_amd.models.model_base_mix import PredictionModel
    from trajsde_amd.synth import synth
    K, T = 6, 30
    base = synth(S=24, n=64, L=24, F=T, box=120.0, seed=17, mixed_source=True, history_dropout=0.2)
    model = PredictionModel(**G.nll_cfg(K, T, 8, 4, dropout=0.1), init_seed=3)
    model.ts_drop = 0.2
    H.perturb_parameters(model, 77)
    model = model.to(dev).train()
    ref = None
    for call in range(3):
        model.zero_grad(set_to_none=True)
        data = H.clone_batch(base).to(dev)
        torch.manual_seed(11)                                           # the ts_drop draw (torch's global generator, as the reference's)
        loss = model.training_step(data, 0, noise=runtime.NoiseSpec(seed=5, dropout_seed=6))
        loss.backward()
        torch.cuda.synchronize()
        cur = (loss.detach().clone(), model.last_output["loc"].clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
        if ref is None:
            ref = cur
            assert bool(torch.isfinite(cur[0])) and all(bool(torch.isfinite(g).all()) for g in cur[2].values())
            assert all("decoder." + s in cur[2] and float(cur[2]["decoder." + s].abs().max()) > 0 for s in SCALE)
            assert not any(n.startswith("decoder.pi.") for n in cur[2])
            continue
        assert torch.equal(cur[0], ref[0]) and torch.equal(cur[1], ref[1]), call
        bad = [n for n in ref[2] if not torch.equal(cur[2][n], ref[2][n])]
        assert not bad and set(cur[2]) == set(ref[2]), (call, bad[:6])


def test_nll_driver_training_lowers_the_loss_and_trains_the_scale_head_only(dev):
    from trajsde_amd import driver
    from trajsde_amd.models.model_base_mix import PredictionModel
    from trajsde_amd.synth import synth
    K, T = 3, 12
    batch = synth(S=3, n=11, L=6, F=T, box=70.0, seed=91, mixed_source=True, history_dropout=0.3)
    model = PredictionModel(**G.nll_cfg(K, T, 4, 2), init_seed=7).to(dev)
    model.lr, model.weight_decay, model.T_max = 2e-3, 1e-4, 10
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    data = batch.to(dev)
    y0 = data.y.clone()

    def fresh(epoch):
        for _ in range(6):
            data.y = y0                                                 # (each forward rotates the targets in place)
            yield data
    hist = driver.train(model, fresh, epochs=2)
    torch.cuda.synchronize()
    assert len(hist) == 12 and sum(hist[-3:]) < sum(hist[:3]), hist
    after = dict(model.named_parameters())
    for s in SCALE:
        assert not torch.equal(after["decoder." + s], before["decoder." + s]), s
    for n, p in after.items():
        if n.startswith("decoder.pi."):
            assert torch.equal(p, before[n]), n
