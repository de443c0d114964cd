"""trajsde_decoder_cotangent_backward (-m gpu): the decoder stage's vector-Jacobian product from caller-supplied dL/dloc and dL/dpi
against float64 autograd over the oracle (oracle/restate.py), its agreement with the welded L2 / Laplace NLL entry points, its
repeatability, and `training_step` under loss sets the welded entry points do not differentiate.

The rule is the backward tests' own (helpers.compare_grads): max|got - want| <= 2e-4 x max|want| + 1e-7 per tensor."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
PI = ["pi.0.weight", "pi.0.bias", "pi.1.weight", "pi.1.bias", "pi.3.weight", "pi.3.bias"]
SCALE = ["scale.0.weight", "scale.0.bias", "scale.1.weight", "scale.1.bias", "scale.3.weight", "scale.3.bias"]
CUSTOM = ["L2", "DiffBCE", "SoftTargetCrossEntropyLoss"]
BOTH = ["L2", "LaplaceNLLLoss", "DiffBCE"]


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


def _rotated(batch, dev):
    from trajsde_amd import runtime
    data = batch.to(dev)
    rot, y_rot = runtime.rotate_inputs(data)
    data.y, data["rotate_mat"] = y_rot, rot
    return data, y_rot


# ------------------------------------------------------------------ 1. vjp parity, stage level
def _stage_case(N, K, T, dev, max_t=None, batch=None):
    """seeded random embeddings, cotangents and injected normals for a decoder at trained-like weights"""
    from trajsde_amd.schedule import decoder_schedule
    from trajsde_amd.synth import synth
    max_t = T / 10.0 if max_t is None else max_t
    model, cfg = H.build_model(K, T, max_t, init_seed=21)
    H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
    model = model.to(dev)
    if batch is None:
        batch = synth(S=1, n=N, L=4, F=T, box=60.0, seed=40 + N)
    assert batch.num_nodes == N
    g = torch.Generator().manual_seed(100 + N)
    sched = decoder_schedule(T, max_t, 0.1)
    t = dict(local=torch.randn(N, 64, generator=g), glob=torch.randn(K, N, 64, generator=g),
             z=torch.randn(sched.n_euler, K * N, 64, generator=g), d_loc=torch.randn(K, N, T, 4, generator=g),
             d_pi=torch.randn(N, K, generator=g))
    return model, cfg, batch, sched, t


def _oracle_vjp(model, cfg, batch, sched, t, noise):
    """float64 autograd of (loc . d_loc).sum() + (pi . d_pi).sum() through the oracle decoder"""
    import restate
    dt = torch.float64
    c = restate.flat_cfg(cfg)
    P, names = H.params_as(model, dt, "decoder.")
    lo = t["local"].to(dt).requires_grad_(True)
    gl = t["glob"].to(dt).requires_grad_(True)
    torch.set_default_dtype(dt)
    try:
        with torch.enable_grad():
            out = restate.sde_decoder(P, c, H.batch_as(batch, dt), lo, gl, H.NoiseAs(noise, dt), sched)
            ((out["loc"] * t["d_loc"].to(dt)).sum() + (out["pi"] * t["d_pi"].to(dt)).sum()).backward()
    finally:
        torch.set_default_dtype(torch.float32)
    want = H.stage_grads(P, names, "decoder.")
    want.update(d_local_embed=lo.grad, d_global_embed=gl.grad)
    return want


@pytest.mark.parametrize("N,K,T", [(1, 1, 5), (15, 3, 5), (16, 3, 5), (17, 6, 5), (33, 6, 20)])
def test_vjp_matches_float64_autograd(N, K, T, dev):
    """one row, one below / at / one above a 16-row tile, a third tile; every gradient of the table, d_local and d_global"""
    import restate
    from trajsde_amd import _lib, runtime
    model, cfg, batch, sched, t = _stage_case(N, K, T, dev)
    noise = runtime.NoiseSpec(z_dec=t["z"].to(dev))
    data = batch.to(dev)
    local, glob = t["local"].to(dev), t["glob"].to(dev)
    rt = model.decoder._rt
    with torch.no_grad():
        out = rt.decoder_forward(data, local, glob, noise)
    res = rt.decoder_cotangent_backward(data, local, glob, out, noise, t["d_loc"].to(dev), t["d_pi"].to(dev))
    _check_range()
    want = _oracle_vjp(model, cfg, batch, sched, t, restate.InjectedNoise(None, None, t["z"]))
    got = dict(res["grads"])
    assert list(got) == rt.param_names(_lib.STAGE_DECODER_COT_BWD) and set(got) <= set(want)
    for k in set(want) - set(got) - {"d_local_embed", "d_global_embed"}:
        assert float(want[k].abs().max()) == 0.0, k               # decoder parameters the forward never reads
    for k in PI + SCALE:
        assert float(got[k].abs().max()) > 0.0, k
    got.update(d_local_embed=res["d_local_embed"], d_global_embed=res["d_global_embed"])
    bad = H.compare_grads(f"cotangent vjp N={N} K={K} T={T}", got, want)
    assert not bad, bad


def test_vjp_under_irregular_masks(dev):
    """the cotangent entry point on trajsde_amd/synth.py irregular_masks rows, with the cotangent of loc zero wherever reg_mask is
    off, as any masked loss hands it over: ragged futures, whole rows of zero cotangent next to live ones in a tile"""
    import restate
    from trajsde_amd import runtime
    from trajsde_amd.synth import irregular
    N, K, T = 39, 6, 20
    model, cfg, batch, sched, t = _stage_case(N, K, T, dev, batch=irregular(S=3, n=13, L=6, F=T, box=60.0, seed=68, mixed_source=True))
    noise = runtime.NoiseSpec(z_dec=t["z"].to(dev))
    data = batch.to(dev)
    local, glob = t["local"].to(dev), t["glob"].to(dev)
    rt = model.decoder._rt
    with torch.no_grad():
        out = rt.decoder_forward(data, local, glob, noise)
    reg = out["reg_mask"].cpu()
    assert torch.equal(reg, ~batch["padding_mask"][:, 21:]) and int((~reg.any(1)).sum()) >= 10
    t["d_loc"] = t["d_loc"] * reg[None, :, :, None]
    res = rt.decoder_cotangent_backward(data, local, glob, out, noise, t["d_loc"].to(dev), t["d_pi"].to(dev))
    _check_range()
    want = _oracle_vjp(model, cfg, batch, sched, t, restate.InjectedNoise(None, None, t["z"]))
    got = dict(res["grads"])
    got.update(d_local_embed=res["d_local_embed"], d_global_embed=res["d_global_embed"])
    assert all(bool(torch.isfinite(g).all()) for g in got.values())
    bad = H.compare_grads(f"cotangent vjp, irregular masks, N={N} K={K} T={T}", got, want)
    assert not bad, bad


# ------------------------------------------------------------------ 2. agreement with the welded entry points
@pytest.fixture(scope="module")
def fixture_cases(dev):
    """the two golden fixtures run once through encoder, aggregator and decoder; the welded backward results beside them"""
    from trajsde_amd import runtime
    cases = {}
    for name in ("mixed_k6_t20", "nus_k1_t5"):
        batch, meta, _, _ = H.load_fixture(name)
        model, cfg = H.build_model(meta)
        H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
        model = model.to(dev)
        data, y_rot = _rotated(batch, dev)
        noise = runtime.NoiseSpec(seed=int(meta["noise_seed"]))
        with torch.no_grad():
            local, *_ = model.encoder(data=data, noise=noise)
            glob = model.aggregator(data=data, local_embed=local)
            out = model.decoder(data=data, local_embed=local, global_embed=glob, noise=noise)
        rt = model.decoder._rt
        welded = {"l2": rt.decoder_l2_backward(data, local, glob, out, noise),
                  "nll": rt.decoder_nll_backward(data, local, glob, out, noise, eps=1e-6)}
        cases[name] = (model, data, noise, local, glob, out, welded)
    return cases


@pytest.mark.parametrize("loss", ["l2", "nll"])
@pytest.mark.parametrize("name", ["mixed_k6_t20", "nus_k1_t5"])
def test_reproduces_the_welded_entry_points(name, loss, fixture_cases):
    """the cotangent of the winner-takes-all L2 (of the Laplace NLL), built by torch from the forward's loc, through the new entry
    point: the welded entry point's grads, d_local and d_global; pi.* exactly zero, scale.* exactly zero under L2"""
    from trajsde_amd import losses
    model, data, noise, local, glob, out, welded = fixture_cases[name]
    loc = out["loc"].detach().clone().requires_grad_(True)
    fn = losses.L2() if loss == "l2" else losses.LaplaceNLLLoss(eps=1e-6)
    with torch.enable_grad():
        value = fn(data, {"loc": loc, "reg_mask": out["reg_mask"]})
        (d_loc,) = torch.autograd.grad(value, [loc])
    assert abs(float(value) - float(welded[loss]["loss"])) <= 2e-5 * max(1.0, abs(float(value)))
    res = model.decoder._rt.decoder_cotangent_backward(data, local, glob, out, noise, d_loc, None)
    _check_range()
    got, want = dict(res["grads"]), dict(welded[loss]["grads"])
    for k in PI + (SCALE if loss == "l2" else []):
        assert float(got[k].abs().max()) == 0.0 and bool(torch.isfinite(got[k]).all()), k
    if loss == "nll":
        assert all(float(got[k].abs().max()) > 0.0 for k in SCALE)
    got.update(d_local_embed=res["d_local_embed"], d_global_embed=res["d_global_embed"])
    want.update(d_local_embed=welded[loss]["d_local_embed"], d_global_embed=welded[loss]["d_global_embed"])
    bad = H.compare_grads(f"cotangent vs welded {loss} {name}", got, want)
    assert not bad, bad


# ------------------------------------------------------------------ 3. zero and repeat
def _all(res):
    d = dict(res["grads"])
    d.update(d_local_embed=res["d_local_embed"], d_global_embed=res["d_global_embed"])
    return d


def test_zero_cotangents_repeat_and_noise_sources(dev):
    import restate
    from trajsde_amd import runtime
    N, K, T = 17, 3, 5
    model, cfg, batch, sched, t = _stage_case(N, K, T, dev)
    rt, data = model.decoder._rt, batch.to(dev)
    local, glob = t["local"].to(dev), t["glob"].to(dev)
    by_seed = runtime.NoiseSpec(seed=77)
    with torch.no_grad():
        out = rt.decoder_forward(data, local, glob, by_seed)
    zero = _all(rt.decoder_cotangent_backward(data, local, glob, out, by_seed, None, None))
    for k, v in zero.items():
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) == 0.0, k
    d_loc, d_pi = t["d_loc"].to(dev), t["d_pi"].to(dev)
    a = _all(rt.decoder_cotangent_backward(data, local, glob, out, by_seed, d_loc, d_pi))
    b = _all(rt.decoder_cotangent_backward(data, local, glob, out, by_seed, d_loc, d_pi))
    torch.cuda.synchronize()
    assert [k for k in a if not torch.equal(a[k], b[k])] == []
    # the host twin's stream handed in as injected normals: the same paths
    twin = restate.PhiloxNoise(77)
    z = torch.stack([twin.decoder(k, (K * N, 64)) for k in range(sched.n_euler)]).to(dev)
    by_z = runtime.NoiseSpec(z_dec=z)
    with torch.no_grad():
        out_z = rt.decoder_forward(data, local, glob, by_z)
    assert H.maxdiff(out_z["loc"], out["loc"]) <= 1e-5
    c = _all(rt.decoder_cotangent_backward(data, local, glob, out_z, by_z, d_loc, d_pi))
    _check_range()
    bad = H.compare_grads("cotangent seed vs injected z", c, a, rel=2e-5)
    assert not bad, bad


# ------------------------------------------------------------------ 3b. both forms of the replay and the sweep
FORMS_SEED = 77


def _forms_case(dev):
    """K * N = 3 * 17 = 51 paths (three full 16-row tiles and a ragged one; 17 actors: a full tile and a ragged one), T = 5 output steps over
    n_euler = 6 Euler steps (max_fut_t 0.6 at step 0.1): the smallest case with a partial tile, more than one mode and n_euler != T"""
    case = _stage_case(17, 3, 5, dev, max_t=0.6)
    assert case[3].n_euler == 6
    return case


def test_both_kernel_forms_match_float64_autograd(dev, tmp_path):
    """The cotangent route reaches the replay and the sweep through the host helpers it shares with the welded entry points
    (csrc/decoder_bwd_host.hpp), on the row domain (K * N, 1).  Once with the default switches (the cooperative kernels in the fp16x3
    build) and once with TRAJSDE_REPLAY_COOP=0 TRAJSDE_SWEEP_COOP=0 (the one-wave kernels), each in a fresh process since the switches
    are read once; seeded noise; every gradient against float64 autograd over the oracle under the file's rule."""
    import os
    import subprocess
    import sys

    import restate
    model, cfg, batch, sched, t = _forms_case(torch.device("cpu"))
    want = _oracle_vjp(model, cfg, batch, sched, t, restate.PhiloxNoise(FORMS_SEED))
    for tag, switches in (("default", {}), ("one-wave", {"TRAJSDE_REPLAY_COOP": "0", "TRAJSDE_SWEEP_COOP": "0"})):
        env = {k: v for k, v in os.environ.items() if k not in ("TRAJSDE_REPLAY_COOP", "TRAJSDE_SWEEP_COOP")}
        env.update(switches)
        out = str(tmp_path / (tag + ".pt"))
        r = subprocess.run([sys.executable, os.path.join(H.ROOT, "tests", "cotangent_forms_child.py"), out], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, (tag, r.stdout[-2000:], r.stderr[-2000:])
        got = torch.load(out)
        assert set(got) <= set(want) and all(float(got[k].abs().max()) > 0.0 for k in PI + SCALE), tag
        bad = H.compare_grads(f"cotangent forms {tag}", got, want)
        assert not bad, (tag, bad)


# ------------------------------------------------------------------ 4. end to end
def _step_model(modules, weights, strength=1.0):
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    K, T, max_t, make = H.TRAINED_CASES["mixed_k6_t20"]
    cfg = H.our_cfg(K, T, max_t)
    cfg["losses"] = ["trajsde_amd/losses.py"] * len(modules)
    cfg["losses_module"] = list(modules)
    cfg["loss_weights"] = list(weights)
    cfg["loss_args"] = [{"eps": 1e-6, "reduction": "mean"} if m == "LaplaceNLLLoss" else {"reduction": "mean"} for m in modules]
    model = PredictionModelSDENet(**cfg, init_seed=2).eval()
    H.trained_like_parameters(model, H.TRAINED_SEED, strength)
    return model, cfg, make()


def _oracle_step(model, cfg, batch_cpu, seed, modules, weights):
    """float64 autograd over the whole oracle under the configured set: L2 and the Laplace NLL as helpers spell them out, the soft-target
    cross-entropy as the torch class it is (it has no reference counterpart), DiffBCE on the encoder's diffusion outputs"""
    import restate
    import torch.nn.functional as F
    from trajsde_amd import losses
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
            local, diff_in, diff_out, _ = restate.local_encoder(P, c, b, rot, noise, es, False, None)
            glob = restate.global_interactor(P, c, b, rot, local, None, None)
            out = restate.sde_decoder(P, c, b, local, glob, noise, ds)
            parts = {"L2": lambda: H.reference_l2(y_rot, out["loc"][..., :2], out["reg_mask"])[0],
                     "LaplaceNLLLoss": lambda: H.reference_laplace_nll(y_rot, out["loc"], out["reg_mask"], 1e-6)[0],
                     "SoftTargetCrossEntropyLoss": lambda: losses.SoftTargetCrossEntropyLoss()({"y": y_rot}, out),
                     "DiffBCE": lambda: (F.binary_cross_entropy(diff_in, torch.zeros_like(diff_in)) +
                                         F.binary_cross_entropy(diff_out, torch.ones_like(diff_out)))}
            values = {m: parts[m]() for m in modules}
            total = sum(w * values[m] for m, w in zip(modules, weights))
            total.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return float(total.detach()), {k: P[k].grad for k in names}, {m: float(v.detach()) for m, v in values.items()}


@pytest.mark.parametrize("modules,weights", [(CUSTOM, (1.0, 0.5, 0.7)), (BOTH, (1.0, 0.3, 0.5))])
def test_training_step_under_a_custom_loss_set(modules, weights, dev):
    """`training_step(...).backward()` fills .grad of every parameter of params_with_gradient(), decoder.pi.* included, with the
    float64 gradients of the whole oracle.  (The parent commit raises NotImplementedError for both sets.)"""
    from trajsde_amd import runtime
    model, cfg, batch = _step_model(modules, weights)
    model = model.to(dev)
    loss = model.training_step(H.clone_batch(batch).to(dev), 0, noise=runtime.NoiseSpec(seed=H.TRAINED_STEP_SEED))
    loss.backward()
    _check_range()
    want_loss, want, values = _oracle_step(model, cfg, batch, H.TRAINED_STEP_SEED, modules, weights)
    assert abs(float(loss) - want_loss) <= 2e-5 * max(1.0, abs(want_loss))
    assert set(model.last_losses) == set(modules)
    for m in modules:
        assert abs(float(model.last_losses[m]) - values[m]) <= 2e-5 * max(1.0, abs(values[m])), m
    reached = {id(p) for p in model.params_with_gradient()}
    named = dict(model.named_parameters())
    got = {n: p.grad for n, p in named.items() if id(p) in reached}
    assert all(g is not None for g in got.values())
    assert {"decoder." + k for k in PI + SCALE} <= set(got)
    assert all(p.grad is None for n, p in named.items() if id(p) not in reached)
    assert {n for n in named if want.get(n) is not None and float(want[n].abs().max()) > 0} <= set(got)
    if "SoftTargetCrossEntropyLoss" in modules:
        assert all(float(got["decoder." + k].abs().max()) > 0 for k in PI)
    bad = H.compare_grads(f"training step {modules}", got, want)
    assert not bad, bad


# ------------------------------------------------------------------ 5. the old route is the old route
def test_each_route_calls_its_own_decoder_backward(dev):
    from trajsde_amd import runtime
    from trajsde_amd.synth import synth
    batch = synth(S=2, n=9, L=4, F=20, box=70.0, seed=12, mixed_source=True)
    for modules, expect in ((["L2", "DiffBCE"], "decoder_l2_backward"), (CUSTOM, "decoder_cotangent_backward")):
        model, _, _ = _step_model(modules, [1.0] * len(modules))
        model = model.to(dev)
        rt = model.decoder._rt
        calls = []
        for name in ("decoder_l2_backward", "decoder_nll_backward", "decoder_cotangent_backward"):
            real = getattr(rt, name)
            setattr(rt, name, (lambda real, name: lambda *a, **kw: (calls.append(name), real(*a, **kw))[1])(real, name))
        model.training_step(H.clone_batch(batch).to(dev), 0, noise=runtime.NoiseSpec(seed=3)).backward()
        torch.cuda.synchronize()
        assert calls == [expect], (modules, calls)


# ------------------------------------------------------------------ 6. optimizer
def test_flat_training_steps_move_the_pi_head(dev):
    from trajsde_amd import driver
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import synth
    model, _, _ = _step_model(CUSTOM, (1.0, 0.5, 0.7))
    model.lr, model.weight_decay, model.T_max = 1e-3, 1e-4, 4
    model = model.to(dev)
    batch = synth(S=2, n=9, L=4, F=20, box=70.0, seed=12, mixed_source=True).to(dev)
    y0 = batch.y.clone()
    before = dict(model.named_parameters())["decoder.pi.3.weight"].detach().clone()
    ft = driver.FlatTraining(model)
    for i in range(2):
        ft.zero()
        batch.y = y0.clone()
        model.training_step(batch, i, noise=NoiseSpec(seed=50 + i)).backward()
        ft.step()
    _check_range()
    assert not torch.equal(dict(model.named_parameters())["decoder.pi.3.weight"].detach(), before)
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_milstein_under_a_custom_set_raises(dev):
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import synth
    cfg = H.our_cfg(3, 20, 2.0)
    cfg["losses"], cfg["losses_module"] = ["trajsde_amd/losses.py"] * 3, list(CUSTOM)
    cfg["loss_weights"], cfg["loss_args"] = [1.0, 1.0, 1.0], [{}, {}, {}]
    cfg["decoder"]["kwargs"]["method"] = "milstein"
    model = PredictionModelSDENet(**cfg, init_seed=0).eval().to(dev)
    batch = synth(S=1, n=6, L=4, F=20, box=60.0, seed=2).to(dev)
    with pytest.raises(NotImplementedError, match="Euler"):
        model.training_step(batch, 0, noise=NoiseSpec(seed=1))
