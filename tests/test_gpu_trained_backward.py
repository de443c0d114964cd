"""The backward kernels (-m gpu) against float64 autograd over the oracle at trained-like weights (helpers.trained_like_parameters,
strengths 1 and 2).

Every other gradient test runs at the initial weights (biases 0, LayerNorms the identity) or 0.02 away from them.  There a dropped
or misplaced bias or gamma in a backward weight image (csrc/pack.hip recipe_*_bwd), in a backward-side forward recompute
(k_sde_replay, the encoder backward) or in tile_bwd.hpp ln_backward is zero or nearly so; ReLU masks, softmax peaks, saturated
sigmoid / tanh units and small NLL scales stay where the initial weights put them.  Here they do not:
tests/test_trained_grad_profile_cpu.py shows that every folded tensor moves its stage's backward by at least 10 x REL at this
profile, and that float32 autograd over the oracle lands within REL / 10 of float64, so the bound below is the kernels' own.

Each stage is tested alone on the fp32 inputs the kernel was given, then the whole training step end to end.  The rule is
helpers.compare_grads: max|got - want| <= REL x max|want| + 1e-7 per tensor; key biases 5e-5 absolute; the encoder's and the
aggregator's tensors may also use 2 x the float32 oracle's own deviation.  Each test prints its worst error ("[trained-backward] ...") and ends with the
fp16-range check quiet."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
REL = H.BACKWARD_REL
STRENGTHS = H.TRAINED_STRENGTHS


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    return torch.device("cuda:0")


def _trained(model, strength):
    H.trained_like_parameters(model, H.TRAINED_SEED, strength)
    return model


def _check_range():
    from trajsde_amd import _lib
    torch.cuda.synchronize()
    _lib.check_range()                           # no fp16x3 operand left the fp16 range at these weights


def _rotated(batch, dev):
    from trajsde_amd import runtime
    data = batch.to(dev)
    rot, y_rot = runtime.rotate_inputs(data)
    data.y, data["rotate_mat"] = y_rot, rot
    return data, y_rot


# ------------------------------------------------------------------ SDE decoder
def _decoder_case(S, n, K, T, max_t, kw, strength, dev, seed, init_seed, noise_seed, batch=None):
    from trajsde_amd import runtime
    from trajsde_amd.synth import synth
    if batch is None:
        batch = synth(S=S, n=n, L=6, F=T, box=80.0, seed=seed + n, **kw)
    model, cfg = H.build_model(K, T, max_t, init_seed=init_seed)
    model = _trained(model, strength).to(dev)
    data, y_rot = _rotated(batch, dev)
    noise = runtime.NoiseSpec(seed=noise_seed)
    with torch.no_grad():
        local, *_ = model.encoder(data=data, noise=noise)
        glob = model.aggregator(data=data, local_embed=local)
        out = model.decoder(data=data, local_embed=local, global_embed=glob, noise=noise)
    return model, cfg, batch, data, y_rot, noise, local, glob, out


def _decoder_check(tag, res, model, cfg, batch, local, glob, y_rot, seed, nll_eps, loss_tol):
    want_loss, want_best, want, d_local, d_glob = H.oracle_decoder_grads(model, cfg, batch, local, glob, y_rot, seed, nll_eps=nll_eps)
    assert torch.equal(res["best_mode"].cpu().long(), want_best)
    assert abs(float(res["loss"]) - want_loss) <= loss_tol * max(1.0, abs(want_loss))
    got = dict(res["grads"])
    for k in set(want) - set(got):
        assert float(want[k].abs().max()) == 0.0, k               # pi head (and the scale head under L2): no gradient path
    got.update(d_local_embed=res["d_local_embed"], d_global_embed=res["d_global_embed"])
    want.update(d_local_embed=d_local, d_global_embed=d_glob)
    bad = H.compare_grads(tag, got, want)
    assert not bad, bad
    return got


DEC_SHAPES = [(3, 20, 4, 20, 2.0, dict(mixed_source=True, history_dropout=0.3)),
              (2, 13, 3, 30, 3.0, dict(source=1)),            # T=30: the solver's extra micro-step, outputs interpolated
              (2, 9, 1, 5, 0.5, dict(nus_sparsity=True))]     # a single mode, ragged masks


@pytest.mark.parametrize("strength", STRENGTHS)
@pytest.mark.parametrize("S,n,K,T,max_t,kw", DEC_SHAPES)
def test_decoder_l2_backward_at_trained_weights(S, n, K, T, max_t, kw, strength, dev):
    """the shapes of test_decoder_l2_backward_matches_autograd: winner, loss, every decoder gradient, d local_embed, d global_embed"""
    model, cfg, batch, data, y_rot, noise, local, glob, out = _decoder_case(S, n, K, T, max_t, kw, strength, dev, 300, 11, 91)
    res = model.decoder._rt.decoder_l2_backward(data, local, glob, out, noise)
    _check_range()
    _decoder_check(f"decoder L2 K={K} T={T} s={strength}", res, model, cfg, batch, local, glob, y_rot, 91, None, 1e-5)


# measured on MI355X: lsde_func.g_func.net.4.bias (the diffusion head's output bias, one scalar) 8.5e-7 from float64 against a max
# of 1.2e-3, i.e. 7.2e-4 of it; every other tensor of the case within 5e-6.  That gradient is a sum over every (actor, mode, step) of
# the reverse sweep that cancels to 1e-3 of its terms; float32 autograd lands 6e-8 from float64 there, the kernels (22-bit split
# operands, decoder_bwd.hip reverse sweep) 14 times further
_SWEEP_BIAS = pytest.mark.xfail(strict=True, reason="g_func.net.4.bias 7.2e-4 of its max (8.5e-7 abs): cancelling sum in the "
                                                   "decoder's reverse sweep (decoder_bwd.hip), 22-bit operands")
NLL_CASES = [pytest.param(*shape, s, marks=_SWEEP_BIAS if (shape[3] == 30 and s == 1.0) else ())
             for shape in DEC_SHAPES[:2] for s in STRENGTHS]


@pytest.mark.parametrize("S,n,K,T,max_t,kw,strength", NLL_CASES)
def test_decoder_nll_backward_at_trained_weights(S, n, K, T, max_t, kw, strength, dev):
    """trajsde_decoder_nll_backward: both heads (the scale head's ELU and 1/s^2 terms at the scales these weights give)"""
    model, cfg, batch, data, y_rot, noise, local, glob, out = _decoder_case(S, n, K, T, max_t, kw, strength, dev, 400, 12, 92)
    res = model.decoder._rt.decoder_nll_backward(data, local, glob, out, noise, eps=1e-6)
    _check_range()
    got = _decoder_check(f"decoder NLL K={K} T={T} s={strength}", res, model, cfg, batch, local, glob, y_rot, 92, 1e-6, 2e-5)
    for k in ("scale.0.weight", "scale.0.bias", "scale.1.weight", "scale.1.bias", "scale.3.weight", "scale.3.bias"):
        assert k in got and float(got[k].abs().max()) > 0.0, k


# ------------------------------------------------------------------ aggregator
def _aggregator_oracle(model, cfg, batch, loc, d_glob, heads):
    """float64 (grads, d_local) and the smallest |input| of the ReLUs on node rows (the interactor's FFNs: they move with `loc`)"""
    import restate
    relu, seen, n = restate.F.relu, [], loc.shape[0]

    def spy(x, *a, **kw):
        if x.dim() == 2 and x.shape[0] == n:
            seen.append(float(x.detach().abs().min()))
        return relu(x, *a, **kw)
    restate.F.relu = spy
    try:
        want, d_local = H.oracle_aggregator_grads(model, cfg, batch, loc, d_glob, heads)
    finally:
        restate.F.relu = relu
    return want, d_local, min(seen, default=float("inf"))


def _away_from_relu_kinks(model, cfg, batch, local, d_glob, heads, margin=2e-6):
    """(local', float64 grads, float64 d_local) with local' = local scaled by 1 + eps for the first eps of a short list at which no
    FFN ReLU input of the float64 interactor lies within `margin` of zero and the float64 d_local does not move when the input
    moves by another 2e-6 (test_gpu_backward._aggregator_point_away_from_relu_kinks).  On a kink the two one-sided gradients
    differ by the unit's whole contribution and fp32 rounding picks the side: at strength 2 the unmoved input of the first and the
    last case put such a unit within rounding of zero and the kernels landed 2e-2 and 4e-2 (of the tensors' max) away"""
    for eps in (0.0, 1e-5, 2e-5, 4e-5, 8e-5, 1.6e-4, 3.2e-4, 6.4e-4):
        loc = (local * (1.0 + eps)).contiguous()
        want, d_local, nearest = _aggregator_oracle(model, cfg, batch, loc, d_glob, heads)
        if nearest < margin:
            continue
        _, d_near = H.oracle_aggregator_grads(model, cfg, batch, loc * (1.0 + 2e-6), d_glob, heads)
        if H.maxdiff(d_near, d_local) <= 5e-5 * float(d_local.abs().max()):
            return loc, want, d_local
    raise AssertionError("no kink-free point near the test input")


AGG_CASES = [(3, 20, 4, 8, dict(mixed_source=True, history_dropout=0.3)),
             (2, 33, 2, 8, dict(source=1)),
             (2, 1, 3, 8, dict()),                            # single-actor scenes: no global edges at all
             (3, 18, 3, 4, dict(mixed_source=True)),          # the vanilla configuration's head count
             (0, 0, 3, 8, None)]                              # helpers._cache_edge_batch: scenes of 32, 33, 256, 257 and 1 actors


# measured on MI355X: global_interactor_layers.1.lin_k_node.bias 6.3e-5 against the key biases' absolute bound of 5e-5 (float64:
# 8e-15); every other tensor of the case within 2 x the float32 oracle's deviation.  A key bias's gradient is zero in exact
# arithmetic; the aggregator backward (aggregator_bwd.hip) sums it over every edge of a target, and with 257-actor scenes at
# strength 2 that rounding residue outgrows the bound
_KEY_BIAS_NOISE = pytest.mark.xfail(strict=True, reason="layers.1.lin_k_node.bias 6.3e-5 > 5e-5: the key-bias gradient's rounding "
                                                       "residue over 257-actor scenes (aggregator_bwd.hip)")
AGG_PARAMS = [pytest.param(*case, s, marks=_KEY_BIAS_NOISE if (case[4] is None and s == 2.0) else ())
              for case in AGG_CASES for s in STRENGTHS]


@pytest.mark.parametrize("S,n,K,heads,kw,strength", AGG_PARAMS)
def test_aggregator_backward_at_trained_weights(S, n, K, heads, kw, strength, dev):
    """each case runs at a point the float64 gradients are locally stable at (_away_from_relu_kinks): the 8 / 4 head kernels, the
    single-actor batch and the scene-cached global attention's chunk and capacity edges"""
    from trajsde_amd import runtime
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    from trajsde_amd.synth import synth
    T = 5
    batch = H._cache_edge_batch(T) if kw is None else synth(S=S, n=n, L=6, F=T, box=80.0, seed=400 + n, **kw)
    _aggregator_backward_check(batch, K, heads, strength, dev)


def _aggregator_backward_check(batch, K, heads, strength, dev, T=5):
    from trajsde_amd import runtime
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    cfg = H.our_cfg(K, T, 0.5)
    cfg["aggregator"]["kwargs"]["num_heads"] = heads
    model = _trained(PredictionModelSDENet(**cfg, init_seed=13).eval(), strength).to(dev)
    data, _ = _rotated(batch, dev)
    with torch.no_grad():
        local, *_ = model.encoder(data=data, noise=runtime.NoiseSpec(seed=17))
    d_glob = torch.randn(K, local.shape[0], 64, generator=torch.Generator().manual_seed(3))
    local, want, d_local = _away_from_relu_kinks(model, cfg, batch, local, d_glob, heads)
    res = model.aggregator._rt.aggregator_backward(data, local, d_glob.to(dev))
    _check_range()
    got = dict(res["grads"])
    assert set(got) == set(want)
    want32, _ = H.oracle_aggregator_grads(model, cfg, batch, local, d_glob, heads, dt=torch.float32)
    noise32 = H.deviation(want32, want)                       # (the edge embedding's ReLUs do not move with `local`)
    got["d_local_embed"], want["d_local_embed"] = res["d_local_embed"], d_local
    bad = H.compare_grads(f"aggregator N={batch.num_nodes} heads={heads} s={strength}", got, want, noise32=noise32)
    assert not bad, bad
    return got


# ------------------------------------------------------------------ SDE encoder
@pytest.mark.parametrize("strength", STRENGTHS)
@pytest.mark.parametrize("S,n,kw,diff_weight", [
    (3, 14, dict(mixed_source=True, history_dropout=0.4), 1.0),
    (2, 9, dict(source=1, history_dropout=0.2), 0.5),
    (2, 6, dict(nus_sparsity=True), 0.0),
])
def test_encoder_backward_at_trained_weights(S, n, kw, diff_weight, strength, dev):
    """every encoder gradient and d aa_out (the AA block's output: the encoder's recurrence backward ends there); the tensor bound
    may be widened only to 2 x the float32 oracle's own deviation from float64 (test_encoder_backward_matches_autograd)"""
    from trajsde_amd import runtime
    from trajsde_amd.synth import synth
    _encoder_backward_check(synth(S=S, n=n, L=6, F=5, box=60.0, seed=500 + n, **kw), diff_weight, strength, dev)


def _encoder_backward_check(batch, diff_weight, strength, dev, tag="encoder"):
    from trajsde_amd import runtime
    model, cfg = H.build_model(2, 5, 0.5, init_seed=17)
    model = _trained(model, strength).to(dev)
    data, _ = _rotated(batch, dev)
    d_local = torch.randn(batch.num_nodes, 64, generator=torch.Generator().manual_seed(5))
    res = model.encoder._rt.encoder_backward(data, d_local.to(dev), runtime.NoiseSpec(seed=23), diff_weight=diff_weight,
                                             want_boundaries=True)
    _check_range()
    want, bce, d_aa = H.oracle_encoder_grads(model, cfg, batch, d_local, 23, diff_weight)
    want32, _, _ = H.oracle_encoder_grads(model, cfg, batch, d_local, 23, diff_weight, dt=torch.float32)
    assert abs(float(res["diff_loss"]) - diff_weight * bce) <= 1e-5 * max(1.0, bce)
    got = dict(res["grads"])
    for k in set(want) - set(got):
        assert float(want[k].abs().max()) == 0.0, k
    noise32 = H.deviation(want32, want)
    got["d_aa_out"], want["d_aa_out"] = res["d_aa_out"], d_aa
    bad = H.compare_grads(f"{tag} diff_weight={diff_weight} s={strength}", got, want, noise32=noise32)
    assert not bad, bad
    return res, got


# ------------------------------------------------------------------ vanilla variant: grid encoder, MLP decoder
@pytest.mark.parametrize("strength", STRENGTHS)
@pytest.mark.parametrize("S,n,heads,layers,kw", [
    (3, 12, 4, 2, dict(mixed_source=True, history_dropout=0.4)),
    (2, 9, 8, 1, dict(source=1, history_dropout=0.2)),
])
def test_vanilla_encoder_backward_at_trained_weights(S, n, heads, layers, kw, strength, dev):
    from trajsde_amd.models.model_base_mix import PredictionModel
    from trajsde_amd.synth import synth
    _vanilla_encoder_backward_check(synth(S=S, n=n, L=6, F=5, box=60.0, seed=900 + n, **kw), heads, layers, strength, dev)


def _vanilla_encoder_backward_check(batch, heads, layers, strength, dev, tag="vanilla encoder"):
    from trajsde_amd.models.model_base_mix import PredictionModel
    cfg = H.grid_cfg(2, 5, heads, layers)
    model = _trained(PredictionModel(**cfg, init_seed=5), strength).to(dev)
    data, _ = _rotated(batch, dev)
    with torch.no_grad():
        local = model.encoder(data=data)
    d_local = torch.randn(local.shape, generator=torch.Generator().manual_seed(2))
    res = model.encoder._rt.encoder_grid_backward(data, d_local.to(dev))
    _check_range()
    _, want = H.oracle_grid_full_grads(model, cfg, batch, d_local)
    want = {k[len("encoder."):]: w for k, w in want.items() if k.startswith("encoder.")}
    for k in set(want) - set(res["grads"]):
        assert want[k] is None or float(want[k].abs().max()) == 0.0, k
    bad = H.compare_grads(f"{tag} heads={heads} layers={layers} s={strength}", res["grads"], want)
    assert not bad, bad
    return res["grads"]


def _pad_future(batch, T, seed, empty_every=0):
    """pad a quarter of the future steps at random; `empty_every`: every that many actors lose all their future steps"""
    g = torch.Generator().manual_seed(seed)
    batch.padding_mask[:, -T:] |= torch.rand(batch.padding_mask.shape[0], T, generator=g) < 0.25
    if empty_every:
        batch.padding_mask[::empty_every, -T:] = True
    return batch


@pytest.mark.parametrize("strength", STRENGTHS)
@pytest.mark.parametrize("loss,S,n,K,T,empty", [("l2", 3, 14, 4, 30, 0), ("l2", 2, 9, 1, 64, 0), ("l2", 2, 21, 10, 60, 0),
                                                ("nll", 3, 14, 3, 12, 0), ("nll", 2, 21, 6, 30, 0), ("nll", 3, 12, 6, 30, 4)])
def test_mlp_decoder_backward_at_trained_weights(loss, S, n, K, T, empty, strength, dev):
    """trajsde_mlp_decoder_l2_backward / _nll_backward (grid_bwd.hip) on padded future steps: winner, loss, both heads' gradients
    under the NLL, d local_embed, d global_embed"""
    import grid_nll_restate as G
    import restate_grid
    from trajsde_amd.models.model_base_mix import PredictionModel
    from trajsde_amd.synth import synth
    seed = 800 + n + K
    batch = _pad_future(synth(S=S, n=n, L=5, F=T, box=80.0, seed=seed, mixed_source=True, history_dropout=0.3), T, seed, empty)
    _mlp_decoder_backward_check(batch, loss, K, T, strength, dev)


def _mlp_decoder_backward_check(batch, loss, K, T, strength, dev, tag="MLP decoder"):
    import grid_nll_restate as G
    import restate_grid
    from trajsde_amd.models.model_base_mix import PredictionModel
    cfg = G.nll_cfg(K, T, 4, 2) if loss == "nll" else H.grid_cfg(K, T, 4, 2)
    model = _trained(PredictionModel(**cfg, init_seed=3), strength).to(dev)
    data = batch.to(dev)
    with torch.no_grad():
        out = model(data)                                           # rotates data.y
    local, glob = out["local_embed"], out["global_embed"]
    rt = model.decoder._rt
    res = rt.mlp_decoder_nll_backward(data, local, glob, out) if loss == "nll" else rt.mlp_decoder_l2_backward(data, local, glob, out)
    _check_range()
    dt = torch.float64
    P, names = H.params_as(model, dt, "decoder.")
    lo = local.detach().cpu().to(dt).requires_grad_(True)
    gl = glob.detach().cpu().to(dt).requires_grad_(True)
    with torch.enable_grad():
        o = restate_grid.mlp_decoder(P, restate_grid.flat_cfg(cfg), batch, lo, gl)
        y = data.y.cpu().to(dt)
        if loss == "nll":
            value, best = H.reference_laplace_nll(y, o["loc"], out["reg_mask"].cpu(), 1e-6)
        else:
            value, best = H.reference_l2(y, o["loc"][..., :2], out["reg_mask"].cpu())
        value.backward()
    assert torch.equal(res["best_mode"].cpu().long(), best)
    assert abs(float(res["loss"]) - float(value.detach())) <= 1e-5 * max(1.0, abs(float(value.detach())))
    want = H.stage_grads(P, names, "decoder.")
    got = dict(res["grads"])
    for k in set(want) - set(got):
        assert float(want[k].abs().max()) == 0.0, k
    if loss == "nll":
        assert all(float(got[k].abs().max()) > 0 for k in got if k.startswith("scale."))
    got.update(d_local_embed=res["d_local_embed"], d_global_embed=res["d_global_embed"])
    want.update(d_local_embed=lo.grad, d_global_embed=gl.grad)
    bad = H.compare_grads(f"{tag} {loss} K={K} T={T} s={strength}", got, want)
    assert not bad, bad
    return got


# ------------------------------------------------------------------ whole training step
def _compare_step(tag, model, want):
    """every parameter's .grad against the float64 gradient; params_with_gradient() is exactly the set float64 says is nonzero, and
    the others keep .grad None"""
    reached = {id(p) for p in model.params_with_gradient()}
    named = dict(model.named_parameters())
    nonzero = {n for n in named if want.get(n) is not None and float(want[n].abs().max()) > 0}
    assert {n for n, p in named.items() if id(p) in reached} == nonzero
    assert all(p.grad is None for n, p in named.items() if id(p) not in reached)
    bad = H.compare_grads(tag, {n: p.grad for n, p in named.items() if id(p) in reached}, want)
    assert not bad, bad


@pytest.mark.parametrize("strength", STRENGTHS)
@pytest.mark.parametrize("mode", H.TRAINED_STEP_MODES)
@pytest.mark.parametrize("name", H.TRAINED_STEP_CASES)
def test_training_step_at_trained_weights(name, mode, strength, dev):
    """`training_step(...).backward()` against float64 autograd over the whole oracle: eval; train mode with the YAML's dropout 0.1
    (the Philox masks, restate.PhiloxDropout on the host); and with losses_module [LaplaceNLLLoss, DiffBCE]"""
    _training_step_check(name, mode, strength, dev)


def _training_step_check(name, mode, strength, dev):
    from trajsde_amd import runtime
    model, cfg, batch, kw = H.trained_step_case(name, mode, strength)
    model = model.to(dev)
    if mode == "dropout":
        model.train()
    loss = model.training_step(H.clone_batch(batch).to(dev), 0, noise=runtime.NoiseSpec(seed=H.TRAINED_STEP_SEED))
    loss.backward()
    _check_range()
    want_loss, want = H.oracle_full_grads(model, cfg, batch, H.TRAINED_STEP_SEED, 1.0, 0.5, **kw)
    assert abs(float(loss) - want_loss) <= (2e-5 if mode == "nll" else 1e-5) * max(1.0, abs(want_loss))
    _compare_step(f"training step {name} {mode} s={strength}", model, want)
    return model


@pytest.mark.parametrize("strength", STRENGTHS)
@pytest.mark.parametrize("loss", ["l2", "nll"])
def test_vanilla_training_step_at_trained_weights(loss, strength, dev):
    import grid_nll_restate as G
    from trajsde_amd.models.model_base_mix import PredictionModel
    from trajsde_amd.synth import synth
    K, T = 3, 12
    batch = _pad_future(synth(S=3, n=11, L=6, F=T, box=70.0, seed=91, mixed_source=True, history_dropout=0.3), T, 91)
    _vanilla_training_step_check(batch, loss, K, T, strength, dev)


def _vanilla_training_step_check(batch, loss, K, T, strength, dev, tag="vanilla training step"):
    import grid_nll_restate as G
    from trajsde_amd.models.model_base_mix import PredictionModel
    cfg = G.nll_cfg(K, T, 4, 2) if loss == "nll" else H.grid_cfg(K, T, 4, 2)
    model = _trained(PredictionModel(**cfg, init_seed=7), strength).to(dev).train()
    value = model.training_step(H.clone_batch(batch).to(dev), 0)
    value.backward()
    _check_range()
    want_loss, want = G.oracle_grid_nll_grads(model, cfg, batch) if loss == "nll" else H.oracle_grid_full_grads(model, cfg, batch)
    assert abs(float(value.detach()) - want_loss) <= 1e-5 * max(1.0, abs(want_loss))
    _compare_step(f"{tag} {loss} s={strength}", model, want)
    return model


def test_training_step_at_strength_2_repeats_bit_for_bit(dev):
    """the whole training step (train mode, dropout 0.1) three times on 32 scenes x 96 agents at strength 2: the same loss bits and
    gradient words every time (test_whole_training_step_repeated_is_bitwise_identical runs 0.02 from the initial weights)"""
    from trajsde_amd import runtime
    from trajsde_amd.synth import synth
    K, T = 6, 20
    batch = synth(S=32, n=96, L=24, F=T, box=120.0, seed=19, mixed_source=True, history_dropout=0.2)
    model, _ = H.build_model(K, T, 2.0, init_seed=4)
    model = _trained(model, 2.0).to(dev).train()
    ref = None
    for call in range(3):
        model.zero_grad(set_to_none=True)
        loss = model.training_step(H.clone_batch(batch).to(dev), 0, noise=runtime.NoiseSpec(seed=7, dropout_seed=8))
        loss.backward()
        torch.cuda.synchronize()
        cur = (loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
        if ref is None:
            ref = cur
            assert len(cur[1]) > 200 and all(bool(torch.isfinite(g).all()) for g in cur[1].values())
            continue
        assert torch.equal(cur[0], ref[0]), call
        bad = [n for n in ref[1] if not torch.equal(cur[1][n], ref[1][n])]
        assert not bad and set(cur[1]) == set(ref[1]), (call, bad[:6])
    _check_range()


# ------------------------------------------------------------------ irregular observation masks
# trajsde_amd/synth.py irregular_masks: gaps and several bos per row, rows unobserved at step 20 or never, step 20 alone, agents with
# an interior gap, ragged and empty futures -- dealt round-robin, so that the kinds share tiles and waves.  Masked GRU steps come
# BEFORE the kept iteration here (the "masked rows pass the state through" path of encoder_bwd.hip is live and differs row by row),
# and the agents padded at step 20 are targets of empty global segments.  The checks and the bounds are those above.
def _finite(grads):
    bad = [k for k, g in grads.items() if g is not None and not bool(torch.isfinite(g).all())]
    assert not bad, bad


def _irregular(F, seed=61, n=13):
    from trajsde_amd.synth import irregular
    return irregular(S=3, n=n, L=6, F=F, box=60.0, seed=seed, mixed_source=True)


@pytest.mark.parametrize("strength", STRENGTHS)
@pytest.mark.parametrize("diff_weight", [1.0, 0.0])
def test_encoder_backward_under_irregular_masks(diff_weight, strength, dev):
    res, got = _encoder_backward_check(_irregular(5), diff_weight, strength, dev, tag="encoder, irregular masks,")
    _finite(got)


@pytest.mark.parametrize("strength", STRENGTHS)
@pytest.mark.parametrize("heads", [8, 4])
def test_aggregator_backward_under_irregular_masks(heads, strength, dev):
    _finite(_aggregator_backward_check(_irregular(5, seed=62), 3, heads, strength, dev))


@pytest.mark.parametrize("strength", STRENGTHS)
@pytest.mark.parametrize("loss", ["l2", "nll"])
def test_decoder_backward_under_irregular_masks(loss, strength, dev):
    """ragged futures, actors without any valid future step (observed at step 20 or not) under the SDE decoder's L2 and NLL"""
    K, T = 4, 20
    case = _decoder_case(3, 13, K, T, 2.0, None, strength, dev, 0, 11, 93, batch=_irregular(T, seed=63))
    model, cfg, batch, data, y_rot, noise, local, glob, out = case
    rt = model.decoder._rt
    if loss == "nll":
        res = rt.decoder_nll_backward(data, local, glob, out, noise, eps=1e-6)
    else:
        res = rt.decoder_l2_backward(data, local, glob, out, noise)
    _check_range()
    _finite(_decoder_check(f"decoder {loss}, irregular masks, K={K} T={T} s={strength}", res, model, cfg, batch, local, glob, y_rot, 93,
                           1e-6 if loss == "nll" else None, 2e-5 if loss == "nll" else 1e-5))


@pytest.mark.parametrize("strength", STRENGTHS)
def test_vanilla_encoder_backward_under_irregular_masks(strength, dev):
    """padding_mask is the temporal transformer's key-padding mask: gaps inside the history, rows padded everywhere"""
    _finite(_vanilla_encoder_backward_check(_irregular(5, seed=64), 4, 2, strength, dev, tag="vanilla encoder, irregular masks,"))


@pytest.mark.parametrize("strength", STRENGTHS)
@pytest.mark.parametrize("loss", ["l2", "nll"])
def test_mlp_decoder_backward_under_irregular_masks(loss, strength, dev):
    _finite(_mlp_decoder_backward_check(_irregular(12, seed=65), loss, 3, 12, strength, dev, tag="MLP decoder, irregular masks,"))


@pytest.mark.parametrize("strength", STRENGTHS)
@pytest.mark.parametrize("mode", H.TRAINED_STEP_MODES)
def test_training_step_under_irregular_masks(mode, strength, dev):
    model = _training_step_check("irregular_k6_t20", mode, strength, dev)
    _finite({n: p.grad for n, p in model.named_parameters()})


@pytest.mark.parametrize("strength", STRENGTHS)
@pytest.mark.parametrize("loss", ["l2", "nll"])
def test_vanilla_training_step_under_irregular_masks(loss, strength, dev):
    model = _vanilla_training_step_check(_irregular(12, seed=66), loss, 3, 12, strength, dev,
                                         tag="vanilla training step, irregular masks,")
    _finite({n: p.grad for n, p in model.named_parameters()})


def test_training_step_under_irregular_masks_repeats_bit_for_bit(dev):
    """train mode (dropout 0.1) twice on the irregular batch at strength 2: the same loss bits and gradient words"""
    from trajsde_amd import runtime
    model, cfg, batch, _ = H.trained_step_case("irregular_k6_t20", "dropout", 2.0)
    model = model.to(dev).train()
    ref = None
    for call in range(2):
        model.zero_grad(set_to_none=True)
        loss = model.training_step(H.clone_batch(batch).to(dev), 0, noise=runtime.NoiseSpec(seed=7, dropout_seed=8))
        loss.backward()
        torch.cuda.synchronize()
        cur = (loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
        if ref is None:
            ref = cur
            assert len(cur[1]) > 200
            _finite(cur[1])
            continue
        assert torch.equal(cur[0], ref[0])
        bad = [n for n in ref[1] if not torch.equal(cur[1][n], ref[1][n])]
        assert not bad and set(cur[1]) == set(ref[1]), bad[:6]
    _check_range()
