"""GPU suite of training the decoder's `method: milstein` (-m gpu): trajsde_decoder_l2_backward_milstein /
trajsde_decoder_nll_backward_milstein (csrc/decoder_mil_bwd.hip: the Milstein replay and the reverse sweep through the gdg term) against
float64 autograd over tests/milstein_grad_restate.py, which differentiates torchsde's create_graph vjp as the reference does.

The stage cases are those of test_gpu_trained_backward.py (DEC_SHAPES, init-like and trained-like weights) under the same per-tensor
rule, helpers.compare_grads.  At these weights the float64 Milstein gradients lie at least 20 x that bound from the Euler ones and from
those of a backward that ignores the second-order term (test_milstein_grad_cpu.py): either would fail here.  Then the whole training
step end to end, its repeatability, and three FlatTraining steps (the Milstein weight images re-packed after every AdamW step)."""
import os
import subprocess
import sys

import pytest
import torch

import helpers as H
import milstein_grad_restate as MG

pytestmark = pytest.mark.gpu
DEC_SHAPES, STRENGTHS = MG.DEC_SHAPES, MG.STRENGTHS


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
    _lib.check_range()                           # no fp16x3 operand left the fp16 range at these weights


def _milstein_model(cfg, init_seed, strength):
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    cfg["decoder"]["kwargs"]["method"] = "milstein"
    model = PredictionModelSDENet(**cfg, init_seed=init_seed).eval()
    if strength:
        H.trained_like_parameters(model, H.TRAINED_SEED, strength)
    return model


def _stage_case(S, n, K, T, max_t, kw, strength, dev, seed=300, init_seed=11, noise_seed=91, batch=None):
    """test_milstein_grad_cpu._stage_case with `method: milstein`, run on the GPU: the kernels' own embeddings and forward"""
    from trajsde_amd import runtime
    from trajsde_amd.synth import synth
    if batch is None:
        batch = synth(S=S, n=n, L=6, F=T, box=80.0, seed=seed + n, **kw)
    cfg = H.our_cfg(K, T, max_t)
    model = _milstein_model(cfg, init_seed, strength).to(dev)
    data = batch.to(dev)
    rot, y_rot = runtime.rotate_inputs(data)
    data.y, data["rotate_mat"] = y_rot, rot
    noise = runtime.NoiseSpec(seed=noise_seed)
    with torch.no_grad():
        local, *_ = model.encoder(data=data, noise=noise)
        glob = model.aggregator(data=data, local_embed=local)
        out = model.decoder(data=data, local_embed=local, global_embed=glob, noise=noise)
    return model, cfg, batch, data, y_rot, noise, local, glob, out


def _check(tag, res, model, cfg, batch, local, glob, y_rot, nll_eps, loss_tol):
    want_loss, want_best, want, d_local, d_glob = MG.oracle_decoder_grads(model, cfg, batch, local, glob, y_rot, 91, nll_eps=nll_eps)
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


@pytest.mark.parametrize("strength", STRENGTHS)
@pytest.mark.parametrize("S,n,K,T,max_t,kw", DEC_SHAPES)
def test_milstein_decoder_l2_backward(S, n, K, T, max_t, kw, strength, dev):
    model, cfg, batch, data, y_rot, noise, local, glob, out = _stage_case(S, n, K, T, max_t, kw, strength, dev)
    res = model.decoder._rt.decoder_l2_backward(data, local, glob, out, noise)
    _check_range()
    _check(f"Milstein decoder L2 K={K} T={T} s={strength}", res, model, cfg, batch, local, glob, y_rot, None, 1e-5)


@pytest.mark.parametrize("strength", STRENGTHS)
@pytest.mark.parametrize("S,n,K,T,max_t,kw", DEC_SHAPES)
def test_milstein_decoder_nll_backward(S, n, K, T, max_t, kw, strength, dev):
    model, cfg, batch, data, y_rot, noise, local, glob, out = _stage_case(S, n, K, T, max_t, kw, strength, dev)
    res = model.decoder._rt.decoder_nll_backward(data, local, glob, out, noise, eps=1e-6)
    _check_range()
    got = _check(f"Milstein decoder NLL K={K} T={T} s={strength}", res, model, cfg, batch, local, glob, y_rot, 1e-6, 2e-5)
    for k in ("scale.0.weight", "scale.0.bias", "scale.1.weight", "scale.1.bias", "scale.3.weight", "scale.3.bias"):
        assert k in got and float(got[k].abs().max()) > 0.0, k


@pytest.mark.parametrize("strength", STRENGTHS)
@pytest.mark.parametrize("loss", ["l2", "nll"])
def test_milstein_decoder_backward_under_irregular_masks(loss, strength, dev):
    """the Milstein pair on trajsde_amd/synth.py irregular_masks rows: ragged futures, actors without any valid future step"""
    from trajsde_amd.synth import irregular
    K, T = 4, 20
    batch = irregular(S=3, n=13, L=6, F=T, box=60.0, seed=67, mixed_source=True)
    model, cfg, batch, data, y_rot, noise, local, glob, out = _stage_case(3, 13, K, T, 2.0, None, strength, dev, batch=batch)
    rt = model.decoder._rt
    res = rt.decoder_nll_backward(data, local, glob, out, noise, eps=1e-6) if loss == "nll" else rt.decoder_l2_backward(data, local, glob, out, noise)
    _check_range()
    got = _check(f"Milstein decoder {loss}, irregular masks, K={K} T={T} s={strength}", res, model, cfg, batch, local, glob, y_rot,
                 1e-6 if loss == "nll" else None, 2e-5 if loss == "nll" else 1e-5)
    assert all(bool(torch.isfinite(g).all()) for g in got.values())


# ------------------------------------------------------------------ whole training step
def _step_case(name, mode, strength):
    """helpers.trained_step_case with `method: milstein` (the encoder runs Euler whatever its method: the reference's sdeint_dual)"""
    import restate
    K, T, max_t, make = H.TRAINED_CASES[name]
    cfg = H.our_cfg(K, T, max_t)
    kw = {}
    if mode == "nll":
        cfg["losses_module"] = ["LaplaceNLLLoss", "DiffBCE"]
        cfg["loss_args"] = [{"eps": 1e-6, "reduction": "mean"}, {"reduction": "mean"}]
        kw["nll_eps"] = 1e-6
    elif mode == "dropout":
        kw["drop"] = restate.PhiloxDropout(H.TRAINED_STEP_SEED, 0.1)
    model = _milstein_model(cfg, 2, 0.0)
    model.loss_weights = [1.0, 0.5]
    H.trained_like_parameters(model, H.TRAINED_SEED, strength)
    return model, cfg, make(), kw


def _compare_step(tag, model, want):
    reached = {id(p) for p in model.params_with_gradient()}
    named = dict(model.named_parameters())
    nonzero = {n for n in named if want.get(n) is not None and float(want[n].abs().max()) > 0}
    assert {n for n, p in named.items() if id(p) in reached} == nonzero
    assert all(p.grad is None for n, p in named.items() if id(p) not in reached)
    bad = H.compare_grads(tag, {n: p.grad for n, p in named.items() if id(p) in reached}, want)
    assert not bad, bad


@pytest.mark.parametrize("strength", H.TRAINED_STRENGTHS)
@pytest.mark.parametrize("mode", H.TRAINED_STEP_MODES)
def test_milstein_training_step(mode, strength, dev):
    """`training_step(...).backward()` with `method: milstein` against float64 autograd over the whole oracle: L2 + DiffBCE in eval
    and in train mode (dropout 0.1), LaplaceNLL + DiffBCE"""
    from trajsde_amd import runtime
    model, cfg, batch, kw = _step_case("mixed_k6_t20", mode, strength)
    model = model.to(dev)
    if mode == "dropout":
        model.train()
    loss = model.training_step(H.clone_batch(batch).to(dev), 0, noise=runtime.NoiseSpec(seed=H.TRAINED_STEP_SEED))
    loss.backward()
    _check_range()
    want_loss, want = MG.oracle_full_grads(model, cfg, batch, H.TRAINED_STEP_SEED, 1.0, 0.5, **kw)
    assert abs(float(loss) - want_loss) <= (2e-5 if mode == "nll" else 1e-5) * max(1.0, abs(want_loss))
    _compare_step(f"Milstein training step {mode} s={strength}", model, want)


@pytest.mark.parametrize("mode", ["eval", "nll"])
def test_milstein_training_step_repeats_bit_for_bit(mode, dev):
    """the same training step twice: the same loss bits and gradient words"""
    from trajsde_amd import runtime
    model, cfg, batch, _ = _step_case("shipped_k10_t60", mode, 2.0)
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
            assert len(cur[1]) > 200 and all(bool(torch.isfinite(g).all()) for g in cur[1].values())
            continue
        assert torch.equal(cur[0], ref[0])
        bad = [n for n in ref[1] if not torch.equal(cur[1][n], ref[1][n])]
        assert not bad and set(cur[1]) == set(ref[1]), bad[:6]
    _check_range()


@pytest.mark.parametrize("mode", ["eval", "nll"])
def test_milstein_flat_training_repacks_after_every_step(mode, dev):
    """three driver.FlatTraining steps under `method: milstein`: the gradients of step 3 are those of a fresh model loaded with the
    parameters after step 2, bit for bit -- the Milstein forward and backward images of the step's PackSet follow every AdamW update"""
    from trajsde_amd import driver
    from trajsde_amd.runtime import NoiseSpec
    model, cfg, batch, _ = _step_case("mixed_k6_t20", mode, 1.0)
    model.lr, model.weight_decay, model.T_max = 1e-3, 1e-4, 4
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(dev).train()
    data = batch.to(dev)
    y0 = data.y.clone()
    ft = driver.FlatTraining(model)
    for i in range(2):
        ft.zero()
        data.y = y0
        model.training_step(data, i, noise=NoiseSpec(seed=60 + i)).backward()
        ft.step()
    ft.zero()
    data.y = y0
    loss = model.training_step(data, 2, noise=NoiseSpec(seed=62))
    loss.backward()
    torch.cuda.synchronize()
    got = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    fresh, _, _, _ = _step_case("mixed_k6_t20", mode, 1.0)
    fresh.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    fresh = fresh.to(dev).train()
    data.y = y0
    loss2 = fresh.training_step(data, 2, noise=NoiseSpec(seed=62))
    loss2.backward()
    torch.cuda.synchronize()
    want = {n: p.grad for n, p in fresh.named_parameters() if p.grad is not None}
    assert torch.equal(loss.detach(), loss2.detach())
    assert set(got) == set(want) and len(got) > 200
    bad = [n for n in want if not torch.equal(got[n], want[n])]
    assert not bad, bad[:6]
    g_func = [n for n in start if n.startswith("decoder.lsde_func.g_func.")]
    assert len(g_func) == 6 and all(not torch.equal(start[n], fresh.state_dict()[n].cpu()) for n in g_func)   # (the steps moved them)


# ------------------------------------------------------------------ the bf16x6 twin (variants/libtrajsde_strict24.so)
_CHILD = (
    "import sys, torch; sys.path[:0] = [%r, %r, %r]\n"
    "import test_gpu_milstein_backward as M\n"
    "dev = torch.device('cuda:0')\n"
    "S, n, K, T, max_t, kw = M.DEC_SHAPES[0]\n"
    "model, cfg, batch, data, y_rot, noise, local, glob, out = M._stage_case(S, n, K, T, max_t, kw, 1.0, dev)\n"
    "rt, res = model.decoder._rt, {}\n"
    "for loss in ('l2', 'nll'):\n"
    "    r = rt.decoder_l2_backward(data, local, glob, out, noise) if loss == 'l2' else rt.decoder_nll_backward(data, local, glob, out, noise, eps=1e-6)\n"
    "    res[loss] = {'loss': r['loss'].cpu(), 'best_mode': r['best_mode'].cpu(), 'd_local_embed': r['d_local_embed'].cpu(),\n"
    "                 'd_global_embed': r['d_global_embed'].cpu(), 'grads': {k: v.cpu() for k, v in r['grads'].items()}}\n"
    "torch.cuda.synchronize()\n"
    "from trajsde_amd import _lib\n"
    "_lib.check_range()\n"
    "torch.save({'res': res, 'local': local.cpu(), 'glob': glob.cpu(), 'y_rot': y_rot.cpu()}, sys.argv[1])\n")


def test_strict_library_milstein_backward(dev, tmp_path):
    """the Milstein backward of the bf16x6 twin (24-bit operands, the one-wave kernels' fp32 products) under both losses against the
    float64 oracle, in a child process that loads that library"""
    from trajsde_amd import build
    if not os.path.isfile(build.STRICT_LIB):
        pytest.skip("variants/libtrajsde_strict24.so not built")
    path = str(tmp_path / "strict.pt")
    script = _CHILD % (H.ROOT, os.path.join(H.ROOT, "tests"), os.path.join(H.ROOT, "oracle"))
    subprocess.run([sys.executable, "-c", script, path], check=True, env={**os.environ, "TRAJSDE_LIB": build.STRICT_LIB}, timeout=600)
    got = torch.load(path)
    from trajsde_amd.synth import synth
    S, n, K, T, max_t, kw = DEC_SHAPES[0]
    batch = synth(S=S, n=n, L=6, F=T, box=80.0, seed=300 + n, **kw)
    cfg = H.our_cfg(K, T, max_t)
    model = _milstein_model(cfg, 11, 1.0)
    for loss, eps, tol in (("l2", None, 1e-5), ("nll", 1e-6, 2e-5)):
        _check(f"Milstein decoder {loss} strict24", got["res"][loss], model, cfg, batch, got["local"], got["glob"], got["y_rot"], eps, tol)
