"""The vanilla HiVT stages as torch.autograd nodes (`autograd: true` among the kwargs of LocalEncoder / GlobalInteractor / MLPDecoder,
trajsde_amd/stage_autograd.py; -m gpu): a torch loss on the stage outputs, `loss.backward()`, and every parameter's `.grad` against
float64 autograd over the oracle (oracle/restate_grid.py) under the same loss and dropout masks -- the whole path, each stage alone, the
agreement with the model-level `training_step`, the exact properties and the refusals.

The rule is the backward tests' own (helpers.compare_grads): max|got - want| <= 2e-4 x max|want| + 1e-7 per tensor."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
CUSTOM = ["L2", "SoftTargetCrossEntropyLoss"]
WEIGHTS = (1.0, 0.7)
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


# name -> (K, T, temporal layers, batch maker): one actor without edges; one below, at and above a 16-row tile; both sources; irregular masks
CASES = {
    "n1_k3_t5": (3, 5, 1, lambda: _synth(S=1, n=1, L=2, F=5, box=30.0, seed=60)),
    "n15_k3_t5": (3, 5, 1, lambda: _synth(S=1, n=15, L=4, F=5, box=60.0, seed=55)),
    "n16_k3_t5": (3, 5, 1, lambda: _synth(S=1, n=16, L=4, F=5, box=60.0, seed=56)),
    "n17_k3_t5": (3, 5, 1, lambda: _synth(S=1, n=17, L=4, F=5, box=60.0, seed=57)),
    "mixed3x9_k6_t20": (6, 20, 2, lambda: _synth(S=3, n=9, L=6, F=20, box=70.0, seed=12, mixed_source=True)),
    "irregular_k6_t20": (6, 20, 2, H.TRAINED_CASES["irregular_k6_t20"][3]),
}


def _model(K, T, layers, autograd=True, **decoder_kw):
    from trajsde_amd.models.model_base_mix import PredictionModel
    cfg = H.grid_cfg(K, T, 4, layers, dropout=0.1)
    cfg["losses"] = ["trajsde_amd/losses.py"] * len(CUSTOM)
    cfg["losses_module"] = list(CUSTOM)
    cfg["loss_weights"] = list(WEIGHTS)
    cfg["loss_args"] = [{"reduction": "mean"} for _ in CUSTOM]
    for s in STAGES:
        cfg[s]["kwargs"]["autograd"] = autograd
    cfg["decoder"]["kwargs"].update(decoder_kw)
    model = PredictionModel(**cfg, init_seed=2).eval()
    H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
    return model, cfg


def _configured_loss(model):
    return lambda data, out: sum(float(w) * fn(data, out) for fn, w in zip(model.losses, model.loss_weights))


def _stages(model, data, noise, upto="decoder"):
    """the test glue: what any glue module around the three stages does (rotate -> encoder -> aggregator -> decoder)"""
    model._ensure_rotated(data)
    local = model.encoder(data=data, noise=noise)
    out = dict(local_embed=local)
    if upto == "decoder":
        glob = model.aggregator(data=data, local_embed=local, noise=noise)
        out.update(model.decoder(data=data, local_embed=local, global_embed=glob))
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


def _oracle(model, cfg, batch_cpu, loss_fn, drop=None, upto="decoder"):
    """float64 autograd over the oracle's stages under `loss_fn(data, out)` and (train mode) the masks of `drop`:
    (loss value, {parameter name: gradient, None without a path})"""
    import restate
    import restate_grid
    dt = torch.float64
    c = restate_grid.flat_cfg(cfg)
    P = {k: (v.detach().cpu().to(dt) if v.is_floating_point() else v.detach().cpu().clone()) for k, v in model.state_dict().items()}
    names = [k for k in P if P[k].is_floating_point() and not k.endswith("attn_mask")]
    for k in names:
        P[k].requires_grad_(True)
    b = H.batch_as(batch_cpu, dt)
    torch.set_default_dtype(dt)
    try:
        rot, y_rot = restate.rotate_inputs(b)
        with torch.enable_grad():
            local = restate_grid.local_encoder_grid(P, c, b, rot, drop)
            out = dict(local_embed=local)
            if upto == "decoder":
                glob = restate.global_interactor(P, c, b, rot, local, None, drop)
                out.update(restate_grid.mlp_decoder(P, c, b, local, glob))
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
    """encoder -> aggregator (4 heads) -> decoder through the stage nodes under 1.0 L2 + 0.7 SoftTargetCrossEntropyLoss evaluated by torch
    on the stage outputs; train mode: dropout 0.1 with the masks of the host Philox twin.  (Without the feature the outputs have no
    grad_fn and loss.backward() raises.)"""
    K, T, layers, make = CASES[name]
    model, cfg = _model(K, T, layers)
    batch = make()
    if name == "mixed3x9_k6_t20":
        assert set(batch["source"].tolist()) == {0, 1}
    assert model.aggregator.num_heads == model.encoder.num_heads == 4
    model = model.to(dev)
    model.train() if mode == "train" else model.eval()
    loss_fn = _configured_loss(model)
    loss, got, out = _step(model, batch, dev, loss_fn)
    _check_range()
    for k in ("loc", "pi", "local_embed", "global_embed"):
        assert out[k].grad_fn is not None, k
    assert out["reg_mask"].grad_fn is None
    assert model._cotangent_route() and set(got) == _reached(model)
    assert {"decoder.pi.6.weight", "decoder.scale.3.weight"} <= set(got)
    want_loss, want = _oracle(model, cfg, batch, loss_fn, drop=_drop(mode))
    assert abs(float(loss) - want_loss) <= 2e-5 * max(1.0, abs(want_loss))
    assert {n for n, w in want.items() if w is not None and float(w.abs().max()) > 0} <= set(got)
    bad = H.compare_grads(f"grid stage autograd, whole path {name} {mode}", got, want)
    assert not bad, bad


# ------------------------------------------------------------------ 2. each stage alone
def test_encoder_node_vjp(dev):
    """a random cotangent on local_embed, train mode (the node's dropout key is replayed by its backward)"""
    K, T, layers, make = CASES["n17_k3_t5"]
    model, cfg = _model(K, T, 2)
    batch = make()
    cot = torch.randn(batch.num_nodes, 64, generator=torch.Generator().manual_seed(8))
    model = model.to(dev).train()
    loss_fn = lambda data, out: (out["local_embed"] * cot.to(out["local_embed"].device, out["local_embed"].dtype)).sum()
    _, got, _ = _step(model, batch, dev, loss_fn, upto="encoder")
    _check_range()
    assert set(got) == {n for n in _reached(model) if n.startswith("encoder.")}
    _, want = _oracle(model, cfg, batch, loss_fn, drop=_drop("train"), upto="encoder")
    assert any(float(v.abs().max()) > 0 for v in got.values())
    bad = H.compare_grads("grid encoder node vjp", got, want)
    assert not bad, bad


def test_aggregator_node_vjp_at_four_heads(dev):
    """GlobalInteractor's node under this glue: a leaf local_embed, a random cotangent on global_embed, 4 heads"""
    import restate
    import restate_grid
    from trajsde_amd.runtime import NoiseSpec
    K, T, layers, make = CASES["n17_k3_t5"]
    model, cfg = _model(K, T, layers)
    batch = make()
    N = batch.num_nodes
    g = torch.Generator().manual_seed(9)
    local, d_glob = torch.randn(N, 64, generator=g), torch.randn(K, N, 64, generator=g)
    model = model.to(dev)
    data = H.clone_batch(batch).to(dev)
    model._ensure_rotated(data)
    with torch.no_grad():
        model.encoder(data=data)                                          # the glue's graph: no fake agents, sync-free until the node asks
    gc = data["_trajsde_graph"]
    assert gc.batch.A == 0 and not gc.graph.exact
    leaf = local.to(dev).requires_grad_(True)
    glob = model.aggregator(data=data, local_embed=leaf, noise=NoiseSpec(seed=SEED))
    assert glob.grad_fn is not None and data["_trajsde_graph"] is gc and gc.graph.exact
    glob.backward(d_glob.to(dev))
    _check_range()
    dt = torch.float64
    P, names = H.params_as(model, dt, "aggregator.")
    lo = local.to(dt).requires_grad_(True)
    b = H.batch_as(batch, dt)
    torch.set_default_dtype(dt)
    try:
        rot, _ = restate.rotate_inputs(b)
        with torch.enable_grad():
            (restate.global_interactor(P, restate_grid.flat_cfg(cfg), b, rot, lo) * d_glob.to(dt)).sum().backward()
    finally:
        torch.set_default_dtype(torch.float32)
    want = H.stage_grads(P, names, "aggregator.")
    got = {n[len("aggregator."):]: p.grad for n, p in model.named_parameters() if p.grad is not None}
    assert set(got) == {n[len("aggregator."):] for n in _reached(model) if n.startswith("aggregator.")}
    got["d_local_embed"], want["d_local_embed"] = leaf.grad, lo.grad
    bad = H.compare_grads("aggregator node vjp, 4 heads, A = 0", got, want)
    assert not bad, bad


def test_decoder_node_vjp(dev):
    """random cotangents on loc and pi, leaf embeddings"""
    import test_gpu_grid_cotangent as TC
    N, K, T = 17, 3, 12
    model, cfg, batch, t = TC._stage_case(N, K, T, dev)
    model.decoder.autograd = True
    data = batch.to(dev)
    lo, gl = t["local"].to(dev).requires_grad_(True), t["glob"].to(dev).requires_grad_(True)
    out = model.decoder(data=data, local_embed=lo, global_embed=gl)
    assert out["loc"].grad_fn is not None and out["pi"].grad_fn is not None and out["reg_mask"].grad_fn is None
    assert out["local_embed"] is lo and out["global_embed"] is gl
    torch.autograd.backward([out["loc"], out["pi"]], [t["d_loc"].to(dev), t["d_pi"].to(dev)])
    _check_range()
    want = TC._oracle_vjp(model, cfg, batch, t)
    got = {n[len("decoder."):]: p.grad for n, p in model.named_parameters() if p.grad is not None}
    assert len(got) == 26 and all(float(got[k].abs().max()) > 0 for k in TC.PI + TC.SCALE)
    got.update(d_local_embed=lo.grad, d_global_embed=gl.grad)
    bad = H.compare_grads("grid decoder node vjp", got, want)
    assert not bad, bad


# ------------------------------------------------------------------ 3. agreement with the model-level route
def test_stage_nodes_agree_with_the_model_level_route(dev):
    """the same batch, dropout key and loss set through training_step (one node over the three backward entry points) and through the
    stage nodes"""
    from trajsde_amd.runtime import NoiseSpec
    K, T, layers, make = CASES["mixed3x9_k6_t20"]
    batch = make()
    model, _ = _model(K, T, layers)
    model = model.to(dev).train()
    for p in model.parameters():
        p.grad = None
    level = model.training_step(H.clone_batch(batch).to(dev), 0, noise=NoiseSpec(seed=SEED))
    level.backward()
    want_loss, want = level.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    loss, got, _ = _step(model, batch, dev, _configured_loss(model))
    _check_range()
    assert abs(float(loss) - float(want_loss)) <= 2e-5 * max(1.0, abs(float(want_loss)))
    assert set(got) == set(want)
    bad = H.compare_grads("grid stage nodes against training_step", got, want)
    assert not bad, bad


# ------------------------------------------------------------------ 4. exact properties
def test_identical_passes_give_identical_gradients_and_a_retained_graph_recomputes(dev):
    from trajsde_amd.runtime import NoiseSpec
    K, T, layers, make = CASES["mixed3x9_k6_t20"]
    model, _ = _model(K, T, layers)
    batch = make()
    model = model.to(dev).train()
    loss_fn = _configured_loss(model)
    _, a, _ = _step(model, batch, dev, loss_fn)
    a = {n: g.clone() for n, g in a.items()}
    _, b, _ = _step(model, batch, dev, loss_fn)
    torch.cuda.synchronize()
    assert set(a) == set(b) and [n for n in a if not torch.equal(a[n], b[n])] == []
    # a second backward over a retained graph: the stages recompute their forward under the node's dropout key
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


def test_no_grad_and_the_switch_off_are_the_inference_path_bit_for_bit(dev):
    K, T, layers, make = CASES["mixed3x9_k6_t20"]
    batch = make()
    on, _ = _model(K, T, layers)
    off, _ = _model(K, T, layers, autograd=False)
    on, off = on.to(dev), off.to(dev)
    keys = ("loc", "pi", "local_embed", "global_embed", "reg_mask")
    data = H.clone_batch(batch).to(dev)
    with torch.no_grad():
        a = on(data)
    assert not data["_trajsde_graph"].graph.exact                         # the inference path: sync-free
    b = off(H.clone_batch(batch).to(dev))                                 # (the switch off: no node even with grad mode on)
    with torch.inference_mode():
        c = on(H.clone_batch(batch).to(dev))
    torch.cuda.synchronize()
    for k in keys:
        assert a[k].grad_fn is None and b[k].grad_fn is None and not a[k].requires_grad, k
        assert torch.equal(a[k], b[k]) and torch.equal(c[k], b[k]), k
    # ... and with grad mode on, the model's forward hands out differentiable outputs of the same values (eval mode: no dropout)
    d = on(H.clone_batch(batch).to(dev))
    assert all(d[k].grad_fn is not None for k in ("loc", "pi", "local_embed", "global_embed"))
    assert H.maxdiff(d["loc"], b["loc"]) <= 1e-4 and H.maxdiff(d["pi"], b["pi"]) <= 1e-4
    _check_range()


# ------------------------------------------------------------------ 5. refusals and misuse
def test_uncertain_false_and_host_tensors_are_refused(dev):
    from trajsde_amd import _lib
    with pytest.raises(NotImplementedError, match="uncertain"):
        _model(3, 5, 1, uncertain=False)
    plain, _ = _model(3, 5, 1, autograd=False, uncertain=False)               # the switch off: built as before
    assert plain.decoder.uncertain is False
    K, T, layers, make = CASES["n17_k3_t5"]
    model, _ = _model(K, T, layers)
    model = model.to(dev)
    with pytest.raises(_lib.TrajsdeError, match="GPU"):
        model.encoder(data=make())
    with pytest.raises(_lib.TrajsdeError, match="GPU"):
        model.decoder(data=make().to(dev), local_embed=torch.zeros(17, 64), global_embed=torch.zeros(K, 17, 64))


def test_a_parameter_updated_between_forward_and_backward_trips_the_version_check(dev):
    from trajsde_amd.runtime import NoiseSpec
    K, T, layers, make = CASES["n17_k3_t5"]
    model, _ = _model(K, T, layers)
    model = model.to(dev)
    for stage in STAGES:
        data = H.clone_batch(make()).to(dev)
        loss = _configured_loss(model)(data, _stages(model, data, NoiseSpec(seed=SEED)))
        with torch.no_grad():
            next(getattr(model, stage).parameters()).mul_(1.0001)
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            loss.backward()
    torch.cuda.synchronize()


def test_a_train_eval_flip_between_forward_and_backward_is_refused(dev):
    from trajsde_amd import _lib
    from trajsde_amd.runtime import NoiseSpec
    K, T, layers, make = CASES["n17_k3_t5"]
    model, _ = _model(K, T, layers)
    model = model.to(dev).train()
    data = H.clone_batch(make()).to(dev)
    loss = (_stages(model, data, NoiseSpec(seed=SEED), upto="encoder")["local_embed"] ** 2).sum()
    model.eval()
    with pytest.raises(_lib.TrajsdeError, match="switched between train"):
        loss.backward()
    torch.cuda.synchronize()
