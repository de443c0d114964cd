"""trajsde_decoder_cotangent_backward_sel (-m gpu): the decoder's vector-Jacobian product from a dL/dloc that is non-zero in one mode per
actor -- torch's gradient of a winner-takes-all loss on the forward's own `loc` -- and a dense dL/dpi, with only the supported path of
every actor replayed: against float64 autograd over the oracle (oracle/restate.py) at the same cotangents, against the dense entry
point, the selection itself, actors without support, repeatability, a violated premise, and `training_step` with
`cotangent_support: winner`.

The cases and the oracle are test_gpu_cotangent.py's (`_stage_case`, `_oracle_vjp`, `_oracle_step`); the rule is the backward tests' own
(helpers.compare_grads): max|got - want| <= 2e-4 x max|want| + 1e-7 per tensor."""
import pytest
import torch

import helpers as H
import test_gpu_cotangent as M

pytestmark = pytest.mark.gpu
PI, SCALE, CUSTOM = M.PI, M.SCALE, M.CUSTOM
SDE = ["lsde_func.f_func.net.0.weight", "lsde_func.f_func.net.2.weight", "lsde_func.f_func.net.4.weight", "lsde_func.g_func.net.0.weight",
       "lsde_func.g_func.net.2.weight", "lsde_func.g_func.net.4.weight", "decoder.0.weight", "aggr_embed.0.weight"]
# (N, K, T, loss): one below / at / one above a 16-row tile under L2 (the scale channels carry no cotangent); the last of them again
# under the Laplace NLL, whose cotangent reaches the scale head of the winning mode too; irregular_masks rows with K = 4, T = 20
CASES = {"n15": (15, 3, 5, "l2"), "n16": (16, 3, 5, "l2"), "n17": (17, 3, 5, "l2"), "n17_nll": (17, 3, 5, "nll"),
         "irregular": (39, 4, 20, "l2")}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    return torch.device("cuda:0")


def _all(res):
    return M._all(res)


def wta_cotangent(data, out, loss, seed):
    """(dL/dloc [K,N,T,4] of the winner-takes-all loss on the forward's `loc`, times a positive weight per (actor, step); the winner per
    actor as losses.L2 picks it; the actors with a valid future step)"""
    from trajsde_amd import losses
    loc = out["loc"].detach().clone().requires_grad_(True)
    fn = losses.L2() if loss == "l2" else losses.LaplaceNLLLoss(eps=1e-6)
    with torch.enable_grad():
        (d_loc,) = torch.autograd.grad(fn(data, {"loc": loc, "reg_mask": out["reg_mask"]}), [loc])
    N, T = loc.shape[1], loc.shape[2]
    g = torch.Generator().manual_seed(seed)
    d_loc = d_loc * (N * T * (0.5 + torch.rand(N, T, 1, generator=g))).to(d_loc.device)      # (magnitudes of order one)
    l2 = torch.norm(data["y"].unsqueeze(0) - out["loc"][..., :2], p=2, dim=-1)
    best = (l2 * out["reg_mask"].unsqueeze(0)).mean(-1).argmin(0)
    return d_loc, best, out["reg_mask"].any(1)


def build_case(key, dev, noise=None):
    """model, inputs, the forward and the winner-takes-all cotangent of one CASES entry (injected normals unless `noise` is given)"""
    from trajsde_amd import runtime
    from trajsde_amd.synth import irregular
    N, K, T, loss = CASES[key]
    if key == "irregular":
        batch = irregular(S=3, n=13, L=6, F=T, box=60.0, seed=68, mixed_source=True)
        model, cfg, batch, sched, t = M._stage_case(N, K, T, dev, batch=batch)
    else:
        model, cfg, batch, sched, t = M._stage_case(N, K, T, dev, max_t=0.6)
        assert sched.n_euler == 6
    noise = runtime.NoiseSpec(z_dec=t["z"].to(dev)) if noise is None else noise
    data, local, glob = batch.to(dev), t["local"].to(dev), t["glob"].to(dev)
    rt = model.decoder._rt
    with torch.no_grad():
        out = rt.decoder_forward(data, local, glob, noise)
    d_loc, best, valid = wta_cotangent(data, out, loss, seed=300 + N)
    t = dict(t, d_loc=d_loc.cpu())
    return dict(model=model, cfg=cfg, batch=batch, sched=sched, t=t, noise=noise, data=data, local=local, glob=glob, rt=rt, out=out,
                d_loc=d_loc, d_pi=t["d_pi"].to(dev), best=best, valid=valid)


def run(c, support, d_loc=None, d_pi=None, noise=None, out=None):
    return c["rt"].decoder_cotangent_backward(c["data"], c["local"], c["glob"], c["out"] if out is None else out,
                                              c["noise"] if noise is None else noise, c["d_loc"] if d_loc is None else d_loc,
                                              c["d_pi"] if d_pi is None else d_pi, support=support)


@pytest.fixture(scope="module")
def cases(dev):
    """every case once: both routes on the same inputs, the float64 reference computed on first use and left unchanged"""
    built = {}

    def get(key):
        if key not in built:
            c = build_case(key, dev)
            c["winner"], c["dense"] = run(c, "winner"), run(c, "all")
            M._check_range()
            built[key] = c
        return built[key]
    return get


def oracle(c):
    import restate
    if "want" not in c:
        c["want"] = M._oracle_vjp(c["model"], c["cfg"], c["batch"], c["sched"], c["t"], restate.InjectedNoise(None, None, c["t"]["z"]))
    return c["want"]


@pytest.mark.parametrize("key", list(CASES))
def test_vjp_matches_float64_autograd(key, cases):
    """every gradient of the table, d_local_embed and d_global_embed against float64 autograd over the oracle at the same cotangents"""
    from trajsde_amd import _lib
    c = cases(key)
    res, want = c["winner"], oracle(c)
    got = dict(res["grads"])
    assert list(got) == c["rt"].param_names(_lib.STAGE_DECODER_COT_BWD) and set(got) <= set(want)
    assert set(res) == {"grads", "d_local_embed", "d_global_embed", "support_status", "support_mode"}
    for k in PI + SDE + (SCALE if CASES[key][3] == "nll" else []):
        assert float(got[k].abs().max()) > 0.0, k
    if key == "irregular":
        assert int((~c["valid"]).sum()) >= 10                             # whole rows of zero cotangent next to live ones in a tile
    got.update(d_local_embed=res["d_local_embed"], d_global_embed=res["d_global_embed"])
    assert all(bool(torch.isfinite(g).all()) for g in got.values())
    bad = H.compare_grads(f"winner vjp {key}", got, want)
    assert not bad, bad


@pytest.mark.parametrize("key", list(CASES))
def test_agrees_with_the_dense_route(key, cases):
    c = cases(key)
    assert set(c["dense"]) == {"grads", "d_local_embed", "d_global_embed"}                    # today's dict
    bad = H.compare_grads(f"winner vs dense {key}", _all(c["winner"]), _all(c["dense"]))
    assert not bad, bad
    # rows of d_global outside the selected mode hold the pi head's part alone: the dense route's, whose aggr_embed part there is zero
    N, K = CASES[key][0], CASES[key][1]
    other = torch.ones(K, N, dtype=torch.bool, device=c["best"].device)
    other[c["winner"]["support_mode"].long(), torch.arange(N, device=other.device)] = False
    a, b = c["winner"]["d_global_embed"][other], c["dense"]["d_global_embed"][other]
    assert float((a - b).abs().max()) <= 2e-4 * float(b.abs().max()) + 1e-7


@pytest.mark.parametrize("key", list(CASES))
def test_selection_is_the_winner_torch_picked(key, cases):
    c = cases(key)
    sel, status = c["winner"]["support_mode"], c["winner"]["support_status"].tolist()
    valid = c["valid"]
    assert sel.dtype == torch.int32 and tuple(sel.shape) == (CASES[key][0],)
    assert torch.equal(sel[valid].long(), c["best"][valid])
    assert bool((sel[~valid] == 0).all())                                 # no valid future step: zero cotangent, mode 0
    assert status == [0, int(valid.sum())]
    c["model"].check_cotangent_support(c["winner"]["support_status"])      # premise kept: nothing raised


def test_rows_with_no_support(cases):
    """all-zero dL/dloc under a dense dL/dpi: the pi head's gradients are the dense route's, everything the SDE and the two heads feed
    is exactly zero, and no actor counts as supported"""
    c = cases("n17")
    zero = torch.zeros_like(c["d_loc"])
    res, dense = run(c, "winner", d_loc=zero), run(c, "all", d_loc=zero)
    M._check_range()
    assert res["support_status"].tolist() == [0, 0] and bool((res["support_mode"] == 0).all())
    got, want = _all(res), _all(dense)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
        if not k.startswith("pi.") and k not in ("d_local_embed", "d_global_embed"):
            assert float(v.abs().max()) == 0.0, k
    assert all(float(got[k].abs().max()) > 0.0 for k in PI)
    keep = PI + ["d_local_embed", "d_global_embed"]
    bad = H.compare_grads("winner vs dense, no support", {k: got[k] for k in keep}, {k: want[k] for k in keep})
    assert not bad, bad


def test_repeats_bitwise_and_noise_sources_agree(dev):
    """two identical calls give identical words; the Philox seed and the host twin's stream handed in as injected normals give the same
    paths (as test_gpu_cotangent.test_zero_cotangents_repeat_and_noise_sources holds the dense route to)"""
    import restate
    from trajsde_amd import runtime
    c = build_case("n17", dev, noise=runtime.NoiseSpec(seed=77))
    N, K = CASES["n17"][:2]
    a, b = run(c, "winner"), run(c, "winner")
    torch.cuda.synchronize()
    assert [k for k in _all(a) if not torch.equal(_all(a)[k], _all(b)[k])] == []
    assert torch.equal(a["support_status"], b["support_status"]) and torch.equal(a["support_mode"], b["support_mode"])
    twin = restate.PhiloxNoise(77)
    z = torch.stack([twin.decoder(k, (K * N, 64)) for k in range(c["sched"].n_euler)]).to(dev)
    by_z = runtime.NoiseSpec(z_dec=z)
    with torch.no_grad():
        out_z = c["rt"].decoder_forward(c["data"], c["local"], c["glob"], by_z)
    assert H.maxdiff(out_z["loc"], c["out"]["loc"]) <= 1e-5
    z_res = run(c, "winner", noise=by_z, out=out_z)
    M._check_range()
    assert torch.equal(z_res["support_mode"], a["support_mode"])
    bad = H.compare_grads("winner, seed vs injected z", _all(z_res), _all(a), rel=2e-5)
    assert not bad, bad


def violate(c, actor=None):
    """dL/dloc with one more supported mode for one supported actor: the rows of the mode after its winner, copied from the winner's"""
    actor = int(torch.nonzero(c["valid"])[0]) if actor is None else actor
    K = c["d_loc"].shape[0]
    k0 = int(c["best"][actor])
    d_loc = c["d_loc"].clone()
    d_loc[(k0 + 1) % K, actor] = d_loc[k0, actor]
    return d_loc, actor, min(k0, (k0 + 1) % K)


def test_violated_premise_completes_and_is_reported(cases):
    """an ordinary in-bounds run: the call returns, counts the actor, keeps its lowest supported mode, and the model's check raises"""
    from trajsde_amd import _lib
    c = cases("n17")
    d_loc, actor, lowest = violate(c)
    res = run(c, "winner", d_loc=d_loc)
    M._check_range()
    assert res["support_status"].tolist() == [1, int(c["valid"].sum())]
    assert int(res["support_mode"][actor]) == lowest
    assert all(bool(torch.isfinite(v).all()) for v in _all(res).values())
    model = c["model"]
    with pytest.raises(_lib.TrajsdeError, match="more than one mode"):
        model.check_cotangent_support(res["support_status"])
    model.last_support_status = res["support_status"]
    try:
        with pytest.raises(_lib.TrajsdeError, match="cotangent_support"):
            model.check_cotangent_support()
    finally:
        model.last_support_status = None
    # the gradients are those of the selected mode alone: the dense route on the cotangent with the other mode's rows taken out again
    only = d_loc.clone()
    for k in range(d_loc.shape[0]):
        if k != lowest:
            only[k, actor] = 0
    bad = H.compare_grads("violated premise vs its selected mode", _all(res), _all(run(c, "all", d_loc=only)))
    assert not bad, bad


# ------------------------------------------------------------------ the training step
def _winner_model(support):
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    weights = (1.0, 0.5, 0.7)
    K, T, max_t, make = H.TRAINED_CASES["mixed_k6_t20"]
    cfg = H.our_cfg(K, T, max_t)
    cfg["losses"] = ["trajsde_amd/losses.py"] * len(CUSTOM)
    cfg["losses_module"] = list(CUSTOM)
    cfg["loss_weights"] = list(weights)
    cfg["loss_args"] = [{"reduction": "mean"} for _ in CUSTOM]
    if support is not None:
        cfg["model_specific"]["kwargs"]["cotangent_support"] = support
    model = PredictionModelSDENet(**cfg, init_seed=2).eval()
    H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
    return model, cfg, make(), weights


def test_training_step_with_cotangent_support_winner(dev):
    """[L2, DiffBCE, SoftTargetCrossEntropyLoss] with `cotangent_support: winner`: the float64 gradients of the whole oracle, the
    parameters the dense route reaches, the dense route's loss values, through the new entry point and with the premise kept"""
    from trajsde_amd import _lib, runtime
    steps = {}
    for support in ("winner", None):
        model, cfg, batch, weights = _winner_model(support)
        model = model.to(dev)
        calls = []
        L = _lib.lib()
        real = {n: getattr(L, n) for n in ("trajsde_decoder_cotangent_backward", "trajsde_decoder_cotangent_backward_sel")}
        for n in real:
            setattr(L, n, (lambda n: lambda *a: (calls.append(n), real[n](*a))[1])(n))
        try:
            loss = model.training_step(H.clone_batch(batch).to(dev), 0, noise=runtime.NoiseSpec(seed=H.TRAINED_STEP_SEED))
        finally:
            for n in real:
                setattr(L, n, real[n])
        loss.backward()
        M._check_range()
        assert calls == ["trajsde_decoder_cotangent_backward" + ("_sel" if support else "")]
        steps[support] = (model, cfg, batch, weights, loss)
    model, cfg, batch, weights, loss = steps["winner"]
    dense_model, dense_loss = steps[None][0], steps[None][4]
    assert model.cotangent_support == "winner" and dense_model.cotangent_support == "all"
    model.check_cotangent_support()
    assert model.last_support_status.tolist()[0] == 0 and model.last_support_status.tolist()[1] > 0
    assert dense_model.last_support_status is None
    want_loss, want, values = M._oracle_step(model, cfg, batch, H.TRAINED_STEP_SEED, CUSTOM, weights)
    assert abs(float(loss) - want_loss) <= 2e-5 * max(1.0, abs(want_loss))
    assert abs(float(loss) - float(dense_loss)) <= 1e-6
    assert set(model.last_losses) == set(dense_model.last_losses) == set(CUSTOM)
    for m in CUSTOM:
        assert abs(float(model.last_losses[m]) - float(dense_model.last_losses[m])) <= 1e-6, m
    reached = {id(p) for p in model.params_with_gradient()}
    named = dict(model.named_parameters())
    got = {n: p.grad for n, p in named.items() if id(p) in reached}
    assert all(g is not None for g in got.values())
    assert set(got) == {n for n, p in dense_model.named_parameters() if p.grad is not None}
    assert all(p.grad is None for n, p in named.items() if id(p) not in reached)
    assert all(float(got["decoder." + k].abs().max()) > 0 for k in PI)
    bad = H.compare_grads("training step, cotangent_support: winner", got, want)
    assert not bad, bad


def test_flat_training_steps_move_the_pi_head(dev):
    from trajsde_amd import driver
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import synth
    model, _, _, _ = _winner_model("winner")
    model.lr, model.weight_decay, model.T_max = 1e-3, 1e-4, 4
    model = model.to(dev)
    batch = synth(S=2, n=9, L=4, F=20, box=70.0, seed=12, mixed_source=True).to(dev)
    y0 = batch.y.clone()
    before = {k: dict(model.named_parameters())["decoder." + k].detach().clone() for k in PI}
    ft = driver.FlatTraining(model)
    for i in range(3):
        ft.zero()
        batch.y = y0.clone()
        model.training_step(batch, i, noise=NoiseSpec(seed=50 + i)).backward()
        ft.step()
        model.check_cotangent_support()
    M._check_range()
    after = dict(model.named_parameters())
    assert all(not torch.equal(after["decoder." + k].detach(), before[k]) for k in PI)
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


# ------------------------------------------------------------------ the one-wave forms of the replay and the sweep
FORMS_SEED = 77


def test_one_wave_kernel_forms_match_float64_autograd(tmp_path):
    """The new entry point reaches the replay and the sweep through the welded route's helpers on the row domain (N, K, sel).  The tests
    above run their default (cooperative, fp16x3 build) forms; this one runs the case in a fresh process with TRAJSDE_REPLAY_COOP=0
    TRAJSDE_SWEEP_COOP=0 (the switches are read once), seeded noise, and compares with float64 autograd at the child's cotangents."""
    import os
    import subprocess
    import sys

    import restate
    env = dict(os.environ, TRAJSDE_REPLAY_COOP="0", TRAJSDE_SWEEP_COOP="0")
    out = str(tmp_path / "one_wave.pt")
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "tests", "cotangent_sel_forms_child.py"), out], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    saved = torch.load(out)
    N, K, T, _ = CASES["n17"]
    model, cfg, batch, sched, t = M._stage_case(N, K, T, torch.device("cpu"), max_t=0.6)
    t = dict(t, d_loc=saved["d_loc"], d_pi=saved["d_pi"])
    want = M._oracle_vjp(model, cfg, batch, sched, t, restate.PhiloxNoise(FORMS_SEED))
    assert saved["status"] == [0, N]
    got = saved["grads"]
    assert set(got) <= set(want) and all(float(got[k].abs().max()) > 0.0 for k in PI + SDE)
    bad = H.compare_grads("winner, one-wave forms", got, want)
    assert not bad, bad
