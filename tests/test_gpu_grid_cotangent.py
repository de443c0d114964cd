"""trajsde_mlp_decoder_cotangent_backward (-m gpu): the vanilla HiVT variant's MLPDecoder differentiated from caller-supplied dL/dloc
and dL/dpi -- against float64 autograd over the oracle (oracle/restate_grid.py), against the welded L2 / Laplace NLL entry points, its
repeatability, and `PredictionModel.training_step` under loss sets the welded entry points do not differentiate.

The rule is the backward tests' own (helpers.compare_grads): max|got - want| <= 2e-4 x max|want| + 1e-7 per tensor."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
PI = ["pi.0.weight", "pi.0.bias", "pi.1.weight", "pi.1.bias", "pi.3.weight", "pi.3.bias", "pi.4.weight", "pi.4.bias", "pi.6.weight",
      "pi.6.bias"]
SCALE = ["scale.0.weight", "scale.0.bias", "scale.1.weight", "scale.1.bias", "scale.3.weight", "scale.3.bias"]
SETS = {"l2_ce": (["L2", "SoftTargetCrossEntropyLoss"], (1.0, 0.7)), "nll_ce": (["LaplaceNLLLoss", "SoftTargetCrossEntropyLoss"], (1.0, 0.5))}


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


def _all(res):
    d = dict(res["grads"])
    d.update(d_local_embed=res["d_local_embed"], d_global_embed=res["d_global_embed"])
    return d


def _cfg(K, T, modules=None, weights=None, dropout=0.0):
    cfg = H.grid_cfg(K, T, 4, 2, dropout=dropout)
    if modules is not None:
        cfg["losses"] = ["trajsde_amd/losses.py"] * len(modules)
        cfg["losses_module"] = list(modules)
        cfg["loss_weights"] = list(weights)
        cfg["loss_args"] = [{"eps": 1e-6, "reduction": "mean"} if m == "LaplaceNLLLoss" else {"reduction": "mean"} for m in modules]
    return cfg


# ------------------------------------------------------------------ 1. vjp parity, stage level
def _stage_case(N, K, T, dev):
    """seeded random embeddings and cotangents for an MLP decoder at trained-like weights"""
    from trajsde_amd.models.model_base_mix import PredictionModel
    from trajsde_amd.synth import synth
    cfg = _cfg(K, T)
    model = PredictionModel(**cfg, init_seed=21).eval()
    H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
    model = model.to(dev)
    batch = synth(S=1, n=N, L=4, F=T, box=60.0, seed=40 + N)
    assert batch.num_nodes == N
    g = torch.Generator().manual_seed(300 + N + T)
    t = dict(local=torch.randn(N, 64, generator=g), glob=torch.randn(K, N, 64, generator=g), d_loc=torch.randn(K, N, T, 4, generator=g),
             d_pi=torch.randn(N, K, generator=g))
    return model, cfg, batch, t


def _oracle_vjp(model, cfg, batch, t):
    """float64 autograd of (loc . d_loc).sum() + (pi . d_pi).sum() through the oracle's MLP decoder"""
    import restate_grid
    dt = torch.float64
    c = restate_grid.flat_cfg(cfg)
    P = {k: v.detach().cpu().to(dt).clone() for k, v in model.state_dict().items() if v.is_floating_point()}
    names = [k for k in P if k.startswith("decoder.")]
    for k in names:
        P[k].requires_grad_(True)
    lo = t["local"].to(dt).requires_grad_(True)
    gl = t["glob"].to(dt).requires_grad_(True)
    torch.set_default_dtype(dt)
    try:
        with torch.enable_grad():
            out = restate_grid.mlp_decoder(P, c, batch, lo, gl)
            ((out["loc"] * t["d_loc"].to(dt)).sum() + (out["pi"] * t["d_pi"].to(dt)).sum()).backward()
    finally:
        torch.set_default_dtype(torch.float32)
    want = {k[len("decoder."):]: P[k].grad for k in names}
    want.update(d_local_embed=lo.grad, d_global_embed=gl.grad)
    return want


@pytest.mark.parametrize("N,K,T", [(1, 1, 5), (15, 3, 12), (16, 3, 12), (17, 6, 30), (17, 3, 33), (33, 2, 64)])
def test_vjp_matches_float64_autograd(N, K, T, dev):
    """one row; K * N and N one below, at and above a 16-row tile; a third tile; 2T below 16, below 64, across 64 (66) and at the full
    128 outputs of a head.  Every one of the 26 gradients, d_local and d_global"""
    from trajsde_amd import _lib
    model, cfg, batch, t = _stage_case(N, K, T, dev)
    data = batch.to(dev)
    local, glob = t["local"].to(dev), t["glob"].to(dev)
    rt = model.decoder._rt
    with torch.no_grad():
        out = rt.mlp_decoder_forward(data, local, glob)
    res = rt.mlp_decoder_cotangent_backward(data, local, glob, out, t["d_loc"].to(dev), t["d_pi"].to(dev))
    _check_range()
    want = _oracle_vjp(model, cfg, batch, t)
    got = dict(res["grads"])
    assert list(got) == rt.param_names(_lib.STAGE_DECODER_MLP_COT_BWD) and len(got) == 26
    assert set(got) <= set(want)
    for k in set(want) - set(got) - {"d_local_embed", "d_global_embed"}:
        assert want[k] is None or float(want[k].abs().max()) == 0.0, k   # decoder tensors the forward never reads
    for k in PI + SCALE:
        assert float(got[k].abs().max()) > 0.0, k
    got.update(d_local_embed=res["d_local_embed"], d_global_embed=res["d_global_embed"])
    bad = H.compare_grads(f"grid cotangent vjp N={N} K={K} T={T}", got, want)
    assert not bad, bad


# ------------------------------------------------------------------ 2. agreement with the welded entry points
@pytest.fixture(scope="module")
def fixture_cases(dev):
    """two golden fixtures of the vanilla variant run once through the model; the welded backward results beside them"""
    import numpy as np
    import os
    from trajsde_amd.data import TemporalData
    from trajsde_amd.models.model_base_mix import PredictionModel
    cases = {}
    for name in ("grid_k3_t12_h4", "grid_k6_t30_h8"):
        z = np.load(os.path.join(H.ROOT, "tests", "golden_grid", name + ".npz"))
        batch = TemporalData(**{k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in.")})
        K, T, heads, layers = (int(z["meta." + k]) for k in ("num_modes", "future_steps", "num_heads", "num_temporal_layers"))
        model = PredictionModel(**H.grid_cfg(K, T, heads, layers), init_seed=int(z["meta.init_seed"])).eval()
        H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
        model = model.to(dev)
        data = batch.to(dev)
        with torch.no_grad():
            out = model(data)                                        # rotates data.y
        local, glob = out["local_embed"], out["global_embed"]
        rt = model.decoder._rt
        welded = {"l2": rt.mlp_decoder_l2_backward(data, local, glob, out),
                  "nll": rt.mlp_decoder_nll_backward(data, local, glob, out, eps=1e-6)}
        cases[name] = (model, data, local, glob, out, welded)
    return cases


@pytest.mark.parametrize("loss", ["l2", "nll"])
@pytest.mark.parametrize("name", ["grid_k3_t12_h4", "grid_k6_t30_h8"])
def test_reproduces_the_welded_entry_points(name, loss, fixture_cases):
    """the cotangent of the winner-takes-all L2 (of the Laplace NLL), built by torch from the forward's loc, through the new entry
    point: the welded entry point's grads, d_local and d_global; pi.* exactly zero, scale.* exactly zero under L2"""
    from trajsde_amd import losses
    model, data, local, glob, out, welded = fixture_cases[name]
    loc = out["loc"].detach().clone().requires_grad_(True)
    fn = losses.L2() if loss == "l2" else losses.LaplaceNLLLoss(eps=1e-6)
    with torch.enable_grad():
        value = fn(data, {"loc": loc, "reg_mask": out["reg_mask"]})
        (d_loc,) = torch.autograd.grad(value, [loc])
    assert abs(float(value) - float(welded[loss]["loss"])) <= 2e-5 * max(1.0, abs(float(value)))
    res = model.decoder._rt.mlp_decoder_cotangent_backward(data, local, glob, out, d_loc, None)
    _check_range()
    got, want = dict(res["grads"]), dict(welded[loss]["grads"])
    for k in PI + (SCALE if loss == "l2" else []):
        assert float(got[k].abs().max()) == 0.0 and bool(torch.isfinite(got[k]).all()), k
    if loss == "nll":
        assert all(float(got[k].abs().max()) > 0.0 for k in SCALE)
    got.update(d_local_embed=res["d_local_embed"], d_global_embed=res["d_global_embed"])
    want.update(d_local_embed=welded[loss]["d_local_embed"], d_global_embed=welded[loss]["d_global_embed"])
    assert set(want) <= set(got)
    bad = H.compare_grads(f"grid cotangent vs welded {loss} {name}", got, want)
    assert not bad, bad


# ------------------------------------------------------------------ 3. zero and repeat
def test_zero_cotangents_and_repeat(dev):
    N, K, T = 17, 3, 12
    model, cfg, batch, t = _stage_case(N, K, T, dev)
    rt, data = model.decoder._rt, batch.to(dev)
    local, glob = t["local"].to(dev), t["glob"].to(dev)
    with torch.no_grad():
        out = rt.mlp_decoder_forward(data, local, glob)
    zero = _all(rt.mlp_decoder_cotangent_backward(data, local, glob, out, None, None))
    for k, v in zero.items():
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) == 0.0, k
    d_loc, d_pi = t["d_loc"].to(dev), t["d_pi"].to(dev)
    a = _all(rt.mlp_decoder_cotangent_backward(data, local, glob, out, d_loc, d_pi))
    b = _all(rt.mlp_decoder_cotangent_backward(data, local, glob, out, d_loc, d_pi))
    _check_range()
    assert float(a["pi.6.weight"].abs().max()) > 0
    assert [k for k in a if not torch.equal(a[k], b[k])] == []


# ------------------------------------------------------------------ 4. end to end
def _step_case(key, train):
    """two scenes of 7 actors, K = 3, T = 12, padded history steps; the model on the host"""
    from trajsde_amd.models.model_base_mix import PredictionModel
    from trajsde_amd.synth import synth
    modules, weights = SETS[key]
    K, T = 3, 12
    batch = synth(S=2, n=7, L=6, F=T, box=70.0, seed=93, mixed_source=True, history_dropout=0.3)
    cfg = _cfg(K, T, modules, weights, dropout=0.1 if train else 0.0)
    model = PredictionModel(**cfg, init_seed=8)
    H.perturb_parameters(model, 1234)
    return (model.train() if train else model.eval()), cfg, batch, modules, weights


def _oracle_step(model, cfg, batch_cpu, modules, weights, drop=None):
    """float64 autograd over the whole oracle (helpers.oracle_grid_full_grads, with the configured set in place of L2): L2 and the
    Laplace NLL as helpers spell them out, the soft-target cross-entropy as the torch class it is"""
    import restate
    import restate_grid
    from trajsde_amd import losses
    c = restate_grid.flat_cfg(cfg)
    dt = torch.float64
    P = {k: (v.detach().cpu().to(dt) if v.is_floating_point() else v.detach().cpu().clone()) for k, v in model.state_dict().items()}
    names = [k for k in P if P[k].is_floating_point() and not k.endswith("attn_mask")]
    for k in names:
        P[k].requires_grad_(True)
    b = H.clone_batch(batch_cpu)
    for k in b.keys:
        if torch.is_tensor(b[k]) and b[k].is_floating_point():
            b[k] = b[k].to(dt)
    torch.set_default_dtype(dt)
    try:
        rot, y_rot = restate.rotate_inputs(b)
        with torch.enable_grad():
            local = restate_grid.local_encoder_grid(P, c, b, rot, drop)
            glob = restate.global_interactor(P, c, b, rot, local, None, drop)
            out = restate_grid.mlp_decoder(P, c, b, local, glob)
            parts = {"L2": lambda: H.reference_l2(y_rot, out["loc"][..., :2], out["reg_mask"])[0],
                     "LaplaceNLLLoss": lambda: H.reference_laplace_nll(y_rot, out["loc"], out["reg_mask"], 1e-6)[0],
                     "SoftTargetCrossEntropyLoss": lambda: losses.SoftTargetCrossEntropyLoss()({"y": y_rot}, out)}
            values = {m: parts[m]() for m in modules}
            total = sum(w * values[m] for m, w in zip(modules, weights))
            total.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return float(total.detach()), {k: P[k].grad for k in names}, {m: float(v.detach()) for m, v in values.items()}


@pytest.mark.parametrize("key,train", [("l2_ce", False), ("nll_ce", False), ("l2_ce", True)])
def test_training_step_under_a_custom_loss_set(key, train, dev):
    """`training_step(...).backward()` sets .grad exactly on params_with_gradient(), decoder.pi.* and decoder.scale.* included, to the
    float64 gradients of the whole oracle; in train mode with the masks of the Philox host twin.  (The parent commit raises
    NotImplementedError for both sets.)"""
    import restate
    from trajsde_amd import runtime
    model, cfg, batch, modules, weights = _step_case(key, train)
    model = model.to(dev)
    loss = model.training_step(H.clone_batch(batch).to(dev), 0, noise=runtime.NoiseSpec(seed=1, dropout_seed=99))
    loss.backward()
    _check_range()
    drop = restate.PhiloxDropout(99, 0.1) if train else None
    want_loss, want, values = _oracle_step(model, cfg, batch, modules, weights, drop)
    print(f"[grid-cotangent] {key} train={train}: loss {float(loss):.8f} want {want_loss:.8f}; "
          + ", ".join(f"{m} {float(model.last_losses[m]):.8f} want {values[m]:.8f}" for m in modules))
    assert abs(float(loss) - want_loss) <= 2e-5 * max(1.0, abs(want_loss))
    assert list(model.last_losses) == modules and all("train/" + m in model.logged for m in modules)
    for m in modules:
        assert abs(float(model.last_losses[m]) - values[m]) <= 2e-5 * max(1.0, abs(values[m])), m
    reached = {id(p) for p in model.params_with_gradient()}
    named = dict(model.named_parameters())
    got = {n: p.grad for n, p in named.items() if id(p) in reached}
    assert all(g is not None for g in got.values())
    assert {"decoder." + k for k in PI + SCALE} <= set(got)
    assert all(p.grad is None for n, p in named.items() if id(p) not in reached)
    assert {n for n in named if want.get(n) is not None and float(want[n].abs().max()) > 0} <= set(got)
    assert all(float(got["decoder." + k].abs().max()) > 0 for k in PI)
    bad = H.compare_grads(f"grid training step {modules} train={train}", got, want)
    assert not bad, bad


# ------------------------------------------------------------------ 5. the old route is the old route
def test_each_route_calls_its_own_decoder_backward(dev):
    from trajsde_amd import runtime
    from trajsde_amd.models.model_base_mix import PredictionModel
    from trajsde_amd.synth import synth
    batch = synth(S=2, n=7, L=4, F=12, box=70.0, seed=12, mixed_source=True)
    for modules, weights, expect in ((["L2"], (1.0,), "mlp_decoder_l2_backward"), (*SETS["l2_ce"], "mlp_decoder_cotangent_backward")):
        model = PredictionModel(**_cfg(3, 12, modules, weights), init_seed=8).eval().to(dev)
        rt = model.decoder._rt
        calls = []
        for name in ("mlp_decoder_l2_backward", "mlp_decoder_nll_backward", "mlp_decoder_cotangent_backward"):
            real = getattr(rt, name)
            setattr(rt, name, (lambda real, name: lambda *a, **kw: (calls.append(name), real(*a, **kw))[1])(real, name))
        model.training_step(H.clone_batch(batch).to(dev), 0, noise=runtime.NoiseSpec(seed=3)).backward()
        torch.cuda.synchronize()
        assert calls == [expect], (modules, calls)


# ------------------------------------------------------------------ 6. optimizer
def test_flat_training_steps_move_the_pi_head(dev):
    from trajsde_amd import driver
    from trajsde_amd.models.model_base_mix import PredictionModel
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import synth
    model = PredictionModel(**_cfg(3, 12, *SETS["l2_ce"]), init_seed=8).eval()
    model.lr, model.weight_decay, model.T_max = 1e-3, 1e-4, 4
    model = model.to(dev)
    batch = synth(S=2, n=7, L=4, F=12, box=70.0, seed=12, mixed_source=True).to(dev)
    y0 = batch.y.clone()
    before = dict(model.named_parameters())["decoder.pi.6.weight"].detach().clone()
    ft = driver.FlatTraining(model)
    for i in range(2):
        ft.zero()
        batch.y = y0.clone()
        model.training_step(batch, i, noise=NoiseSpec(seed=50 + i)).backward()
        ft.step()
    _check_range()
    assert not torch.equal(dict(model.named_parameters())["decoder.pi.6.weight"].detach(), before)
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
