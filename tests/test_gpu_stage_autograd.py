"""The three stages as torch.autograd nodes (`autograd: true`, trajsde_amd/stage_autograd.py; -m gpu): a torch loss on the stage outputs,
`loss.backward()`, and every parameter's `.grad` against float64 autograd over the oracle (oracle/restate.py) at the same Philox noise
and dropout masks -- the whole path, each stage alone, a loss on the diffusion outputs that only this route can train, the agreement
with the model-level `training_step`, the exact properties and the refusals.

The rule is the backward tests' own (helpers.compare_grads): max|got - want| <= 2e-4 x max|want| + 1e-7 per tensor."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
CUSTOM = ["L2", "DiffBCE", "SoftTargetCrossEntropyLoss"]
WEIGHTS = (1.0, 0.5, 0.7)
STAGES = ("encoder", "aggregator", "decoder")
SEED = H.TRAINED_STEP_SEED


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    return torch.device("cuda:0")


def _check_range():
    from trajsde_amd import _lib
    torch.cuda.synchronize()
    _lib.check_range()


def _synth(**kw):
    from trajsde_amd.synth import synth
    return synth(**kw)


# name -> (K, T, max_fut_t, batch maker): the tile edges of the row-on-lane kernels
CASES = {
    "n1_k1_t5": (1, 5, 0.5, lambda: _synth(S=1, n=1, L=2, F=5, box=30.0, seed=60)),                         # one actor, no edges
    "n15_k3_t5": (3, 5, 0.5, lambda: _synth(S=1, n=15, L=4, F=5, box=60.0, seed=55)),
    "n16_k3_t5": (3, 5, 0.5, lambda: _synth(S=1, n=16, L=4, F=5, box=60.0, seed=56)),
    "n17_k3_t5": (3, 5, 0.5, lambda: _synth(S=1, n=17, L=4, F=5, box=60.0, seed=57)),
    "mixed3x9_k6_t20": (6, 20, 2.0, lambda: _synth(S=3, n=9, L=6, F=20, box=70.0, seed=12, mixed_source=True)),   # g_nus and g_argo
    "irregular_k6_t20": H.TRAINED_CASES["irregular_k6_t20"],
}


def _model(K, T, max_t, autograd=True, **decoder_kw):
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    cfg = H.our_cfg(K, T, max_t)
    cfg["losses"] = ["trajsde_amd/losses.py"] * len(CUSTOM)
    cfg["losses_module"] = list(CUSTOM)
    cfg["loss_weights"] = list(WEIGHTS)
    cfg["loss_args"] = [{"reduction": "mean"} for _ in CUSTOM]
    for s in STAGES:
        cfg[s]["kwargs"]["autograd"] = autograd
    cfg["decoder"]["kwargs"].update(decoder_kw)
    model = PredictionModelSDENet(**cfg, init_seed=2).eval()
    H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
    return model, cfg


def _configured_loss(model):
    return lambda data, out: sum(float(w) * fn(data, out) for fn, w in zip(model.losses, model.loss_weights))


def _stages(model, data, noise, upto="decoder"):
    """the test glue: what any glue module around the three stages does"""
    model._ensure_rotated(data)
    local, diff_in, diff_out, label_in, label_out = model.encoder(data=data, noise=noise)
    out = dict(local_embed=local, diff_in=diff_in, diff_out=diff_out, label_in=label_in, label_out=label_out)
    if upto == "decoder":
        glob = model.aggregator(data=data, local_embed=local, noise=noise)
        out.update(model.decoder(data=data, local_embed=local, global_embed=glob, noise=noise))
        out["global_embed"] = glob
    return out


def _step(model, batch_cpu, dev, loss_fn, seed=SEED, upto="decoder"):
    """stages -> torch loss -> loss.backward(): (loss, {parameter name: .grad} of the parameters that got one, stage outputs)"""
    from trajsde_amd.runtime import NoiseSpec
    for p in model.parameters():
        p.grad = None
    data = H.clone_batch(batch_cpu).to(dev)
    out = _stages(model, data, NoiseSpec(seed=seed), upto)
    loss = loss_fn(data, out)
    loss.backward()
    return loss.detach(), {n: p.grad for n, p in model.named_parameters() if p.grad is not None}, out


def _oracle(model, cfg, batch_cpu, loss_fn, seed=SEED, drop=None, upto="decoder"):
    """float64 autograd over the oracle's stages under `loss_fn(data, out)`, the normals of Philox seed `seed` and (train mode) the
    masks of `drop`: (loss value, {parameter name: gradient, None without a path})"""
    import restate
    from trajsde_amd.schedule import decoder_schedule, encoder_schedule
    dt = torch.float64
    c = restate.flat_cfg(cfg)
    es = encoder_schedule(c["historical_steps"], c["max_past_t"], c["minimum_step"])
    ds = decoder_schedule(c["future_steps"], c["max_fut_t"], c["min_stepsize"])
    P = {k: (v.detach().cpu().to(dt) if v.is_floating_point() else v.detach().cpu().clone()) for k, v in model.state_dict().items()}
    names = [k for k in P if P[k].is_floating_point()]
    for k in names:
        P[k].requires_grad_(True)
    b = H.batch_as(batch_cpu, dt)
    noise = H.NoiseAs(restate.PhiloxNoise(seed), dt)
    torch.set_default_dtype(dt)
    try:
        rot, y_rot = restate.rotate_inputs(b)
        with torch.enable_grad():
            local, diff_in, diff_out, _ = restate.local_encoder(P, c, b, rot, noise, es, False, drop)
            out = dict(local_embed=local, diff_in=diff_in, diff_out=diff_out, label_in=torch.zeros_like(diff_in),
                       label_out=torch.ones_like(diff_out))
            if upto == "decoder":
                glob = restate.global_interactor(P, c, b, rot, local, None, drop)
                out.update(restate.sde_decoder(P, c, b, local, glob, noise, ds))
                out["global_embed"] = glob
            total = loss_fn({"y": y_rot}, out)
            total.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return float(total.detach()), {k: P[k].grad for k in names}


def _drop(mode, seed=SEED):
    import restate
    return restate.PhiloxDropout(seed, 0.1) if mode == "train" else None


def _reached(model):
    own = {id(p) for p in model.params_with_gradient()}
    return {n for n, p in model.named_parameters() if id(p) in own}


# ------------------------------------------------------------------ 1. the whole path
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("name", list(CASES))
def test_whole_path_matches_float64_autograd(name, mode, dev):
    """encoder -> aggregator -> decoder through the stage nodes under 1.0 L2 + 0.5 DiffBCE + 0.7 SoftTargetCrossEntropyLoss evaluated by
    torch on the stage outputs; train mode: dropout 0.1 with the masks of the host Philox twin.  (Without the feature the outputs have
    no grad_fn and loss.backward() raises.)"""
    K, T, max_t, make = CASES[name]
    model, cfg = _model(K, T, max_t)
    batch = make()
    if name == "mixed3x9_k6_t20":
        assert set(batch["source"].tolist()) == {0, 1}
    assert cfg["encoder"]["kwargs"]["dropout"] == cfg["aggregator"]["kwargs"]["dropout"] == 0.1
    model = model.to(dev)
    model.train() if mode == "train" else model.eval()
    loss_fn = _configured_loss(model)
    loss, got, out = _step(model, batch, dev, loss_fn)
    _check_range()
    for k in ("loc", "pi", "diff_in", "diff_out", "local_embed", "global_embed"):
        assert out[k].grad_fn is not None, k
    assert out["reg_mask"].grad_fn is None and out["label_in"].grad_fn is None and out["label_out"].grad_fn is None
    assert set(got) == _reached(model)
    want_loss, want = _oracle(model, cfg, batch, loss_fn, drop=_drop(mode))
    assert abs(float(loss) - want_loss) <= 2e-5 * max(1.0, abs(want_loss))
    assert {n for n, w in want.items() if w is not None and float(w.abs().max()) > 0} <= set(got)
    bad = H.compare_grads(f"stage autograd, whole path {name} {mode}", got, want)
    assert not bad, bad


# ------------------------------------------------------------------ 2. each stage alone
def _cotangent_loss(cots):
    return lambda data, out: sum((out[k] * v.to(out[k].device, out[k].dtype)).sum() for k, v in cots.items() if v is not None)


@pytest.mark.parametrize("which", ["all", "local_embed", "diff_in", "diff_out"])
def test_encoder_node_vjp(which, dev):
    """random cotangents on the encoder's three differentiable outputs, and each of them alone (the other two None)"""
    K, T, max_t, make = CASES["n17_k3_t5"]
    model, cfg = _model(K, T, max_t)
    batch = make()
    N, A = batch.num_nodes, int(batch["agent_index"].numel())
    g = torch.Generator().manual_seed(8)
    cots = dict(local_embed=torch.randn(N, 64, generator=g), diff_in=torch.randn(A, 64, generator=g), diff_out=torch.randn(A, 64, generator=g))
    if which != "all":
        cots = {k: (v if k == which else None) for k, v in cots.items()}
    model = model.to(dev)
    loss_fn = _cotangent_loss(cots)
    _, got, _ = _step(model, batch, dev, loss_fn, upto="encoder")
    _check_range()
    assert set(got) == {n for n in _reached(model) if n.startswith("encoder.")}
    _, want = _oracle(model, cfg, batch, loss_fn, upto="encoder")
    assert any(float(v.abs().max()) > 0 for v in got.values())
    bad = H.compare_grads(f"encoder node vjp, cotangents: {which}", got, want)
    assert not bad, bad


def test_aggregator_node_vjp(dev):
    from trajsde_amd.runtime import NoiseSpec
    K, T, max_t, make = CASES["n17_k3_t5"]
    model, cfg = _model(K, T, max_t)
    batch = make()
    N = batch.num_nodes
    g = torch.Generator().manual_seed(9)
    local, d_glob = torch.randn(N, 64, generator=g), torch.randn(K, N, 64, generator=g)
    model = model.to(dev)
    data = H.clone_batch(batch).to(dev)
    model._ensure_rotated(data)
    leaf = local.to(dev).requires_grad_(True)
    glob = model.aggregator(data=data, local_embed=leaf, noise=NoiseSpec(seed=SEED))
    assert glob.grad_fn is not None
    glob.backward(d_glob.to(dev))
    _check_range()
    want, d_local = H.oracle_aggregator_grads(model, cfg, batch, local, d_glob)
    got = {n[len("aggregator."):]: p.grad for n, p in model.named_parameters() if p.grad is not None}
    assert set(got) == {n[len("aggregator."):] for n in _reached(model) if n.startswith("aggregator.")}
    got["d_local_embed"], want["d_local_embed"] = leaf.grad, d_local
    bad = H.compare_grads("aggregator node vjp", got, want)
    assert not bad, bad


@pytest.mark.parametrize("support", ["all", "winner"])
def test_decoder_node_vjp(support, dev):
    """random cotangents on loc and pi (`winner`: dL/dloc kept in one mode per actor, as the switch asks)"""
    import restate
    import test_gpu_cotangent as TC
    from trajsde_amd import runtime
    N, K, T = 17, 3, 5
    _, _, batch, sched, t = TC._stage_case(N, K, T, torch.device("cpu"))
    model, cfg = _model(K, T, T / 10.0, cotangent_support=support)
    if support == "winner":
        keep = torch.randint(0, K, (N,), generator=torch.Generator().manual_seed(3))
        t["d_loc"] = t["d_loc"] * torch.nn.functional.one_hot(keep, K).t()[:, :, None, None]
    model = model.to(dev)
    data = batch.to(dev)
    lo, gl = t["local"].to(dev).requires_grad_(True), t["glob"].to(dev).requires_grad_(True)
    out = model.decoder(data=data, local_embed=lo, global_embed=gl, noise=runtime.NoiseSpec(z_dec=t["z"].to(dev)))
    assert out["loc"].grad_fn is not None and out["pi"].grad_fn is not None and out["reg_mask"].grad_fn is None
    torch.autograd.backward([out["loc"], out["pi"]], [t["d_loc"].to(dev), t["d_pi"].to(dev)])
    _check_range()
    want = TC._oracle_vjp(model, cfg, batch, sched, t, restate.InjectedNoise(None, None, t["z"]))
    got = {n[len("decoder."):]: p.grad for n, p in model.named_parameters() if p.grad is not None}
    assert set(got) == {n[len("decoder."):] for n in _reached(model) if n.startswith("decoder.")}
    assert all(float(got[k].abs().max()) > 0 for k in TC.PI + TC.SCALE)
    got.update(d_local_embed=lo.grad, d_global_embed=gl.grad)
    if support == "winner":
        assert model.decoder.last_support_status.tolist() == [0, N]
    bad = H.compare_grads(f"decoder node vjp, support {support}", got, want)
    assert not bad, bad


# ------------------------------------------------------------------ 3. a loss only this route can train
def test_a_loss_on_the_diffusion_outputs_trains_the_encoder(dev):
    K, T, max_t, make = CASES["mixed3x9_k6_t20"]
    model, cfg = _model(K, T, max_t)
    batch = make()
    model = model.to(dev)
    loss_fn = lambda data, out: ((out["diff_in"] - 0.3) ** 2).mean() + out["diff_out"].sum(-1).mean()
    loss, got, _ = _step(model, batch, dev, loss_fn, upto="encoder")
    _check_range()
    want_loss, want = _oracle(model, cfg, batch, loss_fn, upto="encoder")
    assert abs(float(loss) - want_loss) <= 2e-5 * max(1.0, abs(want_loss))
    assert float(got["encoder.lsde_func.g_nus.net.4.weight"].abs().max()) > 0 and float(got["encoder.lsde_func.g_argo.net.4.weight"].abs().max()) > 0
    assert all(n.startswith("encoder.") for n in got)
    bad = H.compare_grads("a loss on diff_in / diff_out", got, want)
    assert not bad, bad


# ------------------------------------------------------------------ 4. agreement with the model-level route
@pytest.fixture(scope="module")
def both_routes(dev):
    """the same batch, noise and loss set through training_step (`cotangent_support: all`) and through the stage nodes (`all`, `winner`)"""
    from trajsde_amd.runtime import NoiseSpec
    K, T, max_t, make = CASES["mixed3x9_k6_t20"]
    batch = make()
    model, _ = _model(K, T, max_t)
    model = model.to(dev)
    assert model._cotangent_route() and model.cotangent_support == "all"
    for p in model.parameters():
        p.grad = None
    level = model.training_step(H.clone_batch(batch).to(dev), 0, noise=NoiseSpec(seed=SEED))
    level.backward()
    res = {"model": (level.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})}
    loss, got, _ = _step(model, batch, dev, _configured_loss(model))
    res["all"] = (loss, {n: g.clone() for n, g in got.items()})
    model.decoder.cotangent_support = "winner"
    loss, got, _ = _step(model, batch, dev, _configured_loss(model))
    res["winner"] = (loss, {n: g.clone() for n, g in got.items()})
    res["status"] = model.decoder.last_support_status.tolist()
    _check_range()
    return res


def test_stage_nodes_agree_with_the_model_level_route(both_routes):
    (want_loss, want), (loss, got) = both_routes["model"], both_routes["all"]
    assert abs(float(loss) - float(want_loss)) <= 2e-5 * max(1.0, abs(float(want_loss)))
    assert set(got) == set(want)
    bad = H.compare_grads("stage nodes against training_step", got, want)
    assert not bad, bad


def test_winner_support_on_the_decoder_stage_matches_all(both_routes):
    """under the winner-takes-all set dL/dloc is non-zero in one mode per actor: the stage's `cotangent_support: winner` replays that
    mode only and says so in its status words"""
    (_, want), (_, got) = both_routes["all"], both_routes["winner"]
    assert both_routes["status"][0] == 0 and both_routes["status"][1] > 0
    assert set(got) == set(want)
    bad = H.compare_grads("decoder stage, winner against all", got, want)
    assert not bad, bad


# ------------------------------------------------------------------ 5. exact properties
def test_identical_passes_give_identical_gradients_and_a_retained_graph_recomputes(dev):
    from trajsde_amd.runtime import NoiseSpec
    K, T, max_t, make = CASES["mixed3x9_k6_t20"]
    model, _ = _model(K, T, max_t)
    batch = make()
    model = model.to(dev).train()
    loss_fn = _configured_loss(model)
    _, a, _ = _step(model, batch, dev, loss_fn)
    a = {n: g.clone() for n, g in a.items()}
    _, b, _ = _step(model, batch, dev, loss_fn)
    torch.cuda.synchronize()
    assert set(a) == set(b) and [n for n in a if not torch.equal(a[n], b[n])] == []
    # a second backward over a retained graph: the tapes are gone, the stages recompute their forward at the node's noise
    for p in model.parameters():
        p.grad = None
    data = H.clone_batch(batch).to(dev)
    loss = loss_fn(data, _stages(model, data, NoiseSpec(seed=SEED)))
    loss.backward(retain_graph=True)
    first = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    for p in model.parameters():
        p.grad = None
    loss.backward()
    torch.cuda.synchronize()
    second = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    assert [n for n in a if not torch.equal(first[n], a[n])] == []
    assert set(second) == set(first) and [n for n in first if not torch.equal(first[n], second[n])] == []


def test_no_grad_is_the_inference_path_bit_for_bit(dev):
    from trajsde_amd.runtime import NoiseSpec
    K, T, max_t, make = CASES["mixed3x9_k6_t20"]
    batch = make()
    on, _ = _model(K, T, max_t)
    off, _ = _model(K, T, max_t, autograd=False)
    on, off = on.to(dev), off.to(dev)
    keys = ("loc", "pi", "diff_in", "diff_out", "reg_mask")
    with torch.no_grad():
        a = on(H.clone_batch(batch).to(dev), noise=NoiseSpec(seed=SEED))
    b = off(H.clone_batch(batch).to(dev), noise=NoiseSpec(seed=SEED))          # (the switch off: no node even with grad mode on)
    with torch.inference_mode():
        c = on(H.clone_batch(batch).to(dev), noise=NoiseSpec(seed=SEED))
    torch.cuda.synchronize()
    for k in keys:
        assert a[k].grad_fn is None and b[k].grad_fn is None and not a[k].requires_grad, k
        assert torch.equal(a[k], b[k]) and torch.equal(c[k], b[k]), k
    # ... and with grad mode on, the model's forward hands out differentiable outputs
    d = on(H.clone_batch(batch).to(dev), noise=NoiseSpec(seed=SEED))
    assert all(d[k].grad_fn is not None for k in ("loc", "pi", "diff_in", "diff_out"))
    assert H.maxdiff(d["loc"], b["loc"]) <= 1e-4 and H.maxdiff(d["pi"], b["pi"]) <= 1e-4


# ------------------------------------------------------------------ 6. refusals and misuse
def test_milstein_and_uncertain_false_are_refused(dev):
    with pytest.raises(NotImplementedError, match="Euler-only cotangent route"):
        _model(3, 20, 2.0, method="milstein")
    with pytest.raises(NotImplementedError, match="uncertain"):
        _model(3, 5, 0.5, uncertain=False)
    plain, _ = _model(3, 20, 2.0, autograd=False, method="milstein")           # the switch off: a Milstein decoder is built as before
    assert plain.decoder.method == "milstein"


def test_a_parameter_updated_between_forward_and_backward_trips_the_version_check(dev):
    from trajsde_amd.runtime import NoiseSpec
    K, T, max_t, make = CASES["n17_k3_t5"]
    model, _ = _model(K, T, max_t)
    model = model.to(dev)
    for stage in STAGES:
        data = H.clone_batch(make()).to(dev)
        loss = _configured_loss(model)(data, _stages(model, data, NoiseSpec(seed=SEED)))
        with torch.no_grad():
            next(getattr(model, stage).parameters()).mul_(1.0001)
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            loss.backward()
    torch.cuda.synchronize()
