"""The inference kernels (-m gpu) against the float64 oracle at trained-like weights (helpers.trained_like_parameters).

Every other inference parity test runs at the initial weights, where all biases are 0 and every LayerNorm is the identity affine
map.  The kernels do not apply those parameters where the reference does: csrc/pack.hip folds LayerNorm gamma into the next
matrix, beta and the bias into constants (W beta + b) that the kernels add back only where the algebra allows (non-empty
segments, the sum of the attention weights), centres bias vectors, drops the key biases and prescales tanh / sigmoid layers.
A wrong fold is invisible at the initial weights.  Here it is not (tests/test_trained_profile_cpu.py shows that every folded
tensor moves the outputs by at least 10 x TOL at this profile).  The oracle runs in float64 on the fp32 normals the kernels
draw, so the errors printed below are the kernels' own."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
TOL = 1e-4
KEYS = ("loc", "pi", "diff_in", "diff_out")
SEED = 6
CASES = [(name, s) for name in H.TRAINED_CASES for s in H.TRAINED_STRENGTHS]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    return torch.device("cuda:0")


def _model(name, strength, uncertain=True, method=None):
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    K, T, max_t, make = H.TRAINED_CASES[name]
    cfg = H.our_cfg(K, T, max_t, uncertain)
    if method is not None:
        cfg["decoder"]["kwargs"]["method"] = cfg["encoder"]["kwargs"]["method"] = method
    model = PredictionModelSDENet(**cfg, init_seed=2).eval()
    H.trained_like_parameters(model, H.TRAINED_SEED, strength)
    return model, cfg, make()


_ORACLE = {}


def _oracle(name, strength):
    """(model on the host, cfg, batch, float64 oracle with intermediates), computed once per case"""
    key = (name, strength)
    if key not in _ORACLE:
        model, cfg, batch = _model(name, strength)
        _ORACLE[key] = (model, cfg, batch, H.oracle_forward64(model, cfg, batch, noise_seed=SEED))
    model, cfg, batch, want = _ORACLE[key]
    m2, _, _ = _model(name, strength)            # a fresh copy for the device (the cached one stays on the host)
    return m2, cfg, H.clone_batch(batch), want


def _scaled(a, ref):
    """max-abs error over max(1, max|ref|): the bound for intermediates whose magnitude grows with the weights"""
    return H.maxdiff(a, ref) / max(1.0, float(ref.abs().max()))


def _report(tag, errs):
    print(f"[trained-weights] {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))


def _check_range():
    from trajsde_amd import _lib
    _lib.check_range()                           # no fp16x3 operand left the fp16 range at these weights


@pytest.mark.parametrize("name,strength", CASES)
def test_forward_matches_float64_oracle(name, strength, dev):
    from trajsde_amd.runtime import NoiseSpec
    model, cfg, batch, want = _oracle(name, strength)
    model = model.to(dev)
    model.encoder.capture_intermediates = True
    seen = {}
    hook = model.decoder.register_forward_hook(
        lambda mod, args, kw, out: seen.update(local=kw["local_embed"].clone(), glob=kw["global_embed"].clone()), with_kwargs=True)
    try:
        with torch.no_grad():
            o = model(batch.to(dev), noise=NoiseSpec(seed=SEED))
        torch.cuda.synchronize()
    finally:
        hook.remove()
    _check_range()
    im = model.encoder.last_intermediates
    assert im["E_aa"] == want["aa_edges"]
    errs = {k: H.maxdiff(o[k].cpu(), want[k]) for k in KEYS}
    rel = {"aa_out": _scaled(im["aa_out"].cpu(), want["aa_out"]), "latent_ys": _scaled(im["latent_ys"].cpu(), want["latent_ys"]),
           "local_embed": _scaled(seen["local"].cpu(), want["local_embed"]), "global_embed": _scaled(seen["glob"].cpu(), want["global_embed"])}
    _report(f"forward {name} s={strength}", {**errs, **rel})
    assert torch.equal(o["reg_mask"].cpu(), want["reg_mask"])
    for k, e in {**errs, **rel}.items():
        assert e <= TOL, (k, e)


def _stage_check(model, cfg, batch, want, dev, tag):
    """encoder; aggregator fed the oracle's local_embed; decoder fed the oracle's embeddings, with in-kernel Philox and with the
    same normals injected -- each against the float64 oracle of that stage on the same (fp32-rounded) inputs"""
    import restate
    from trajsde_amd import philox
    from trajsde_amd.runtime import NoiseSpec, rotate_inputs
    from trajsde_amd.schedule import decoder_schedule
    c = restate.flat_cfg(cfg)
    K, T, N = c["num_modes"], c["future_steps"], batch.num_nodes
    P = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in model.state_dict().items()}
    b64 = H.double_batch(batch)
    rot64, _ = restate.rotate_inputs(b64)
    model = model.to(dev)
    data = batch.to(dev)
    data["rotate_mat"], _ = rotate_inputs(data)
    errs = {}
    with torch.no_grad():
        local, di, do, _, _ = model.encoder(data=data, noise=NoiseSpec(seed=SEED))
        errs["encoder.local_embed"] = _scaled(local.cpu(), want["local_embed"])
        errs["encoder.diff_in"] = H.maxdiff(di.cpu(), want["diff_in"])
        errs["encoder.diff_out"] = H.maxdiff(do.cpu(), want["diff_out"])
        local32 = want["local_embed"].float()
        g = model.aggregator(data=data, local_embed=local32.to(dev))
        g_want = restate.global_interactor(P, c, b64, rot64, local32.double())
        errs["aggregator"] = _scaled(g.cpu(), g_want)
        gone = batch["padding_mask"][:, c["historical_steps"] - 1].cpu()     # targets of an empty global segment: written all the same
        if bool(gone.any()):
            assert bool(torch.isfinite(g.cpu()[:, gone]).all())
            errs["aggregator[padded at 20]"] = _scaled(g.cpu()[:, gone], g_want[:, gone])
        glob32 = want["global_embed"].float()
        sched = decoder_schedule(T, c["max_fut_t"], c["min_stepsize"])
        z = torch.from_numpy(np.stack([philox.normals(SEED, philox.STREAM_DECODER, k, np.arange(K * N), 64) for k in range(sched.n_euler)]))
        d_want = restate.sde_decoder(P, c, b64, local32.double(), glob32.double(), H.Float64Noise(restate.InjectedNoise(None, None, z)), sched)
        for tag_n, noise in (("philox", NoiseSpec(seed=SEED)), ("injected", NoiseSpec(seed=0, z_dec=z.to(dev)))):
            dec = model.decoder(data=data, local_embed=local32.to(dev), global_embed=glob32.to(dev), noise=noise)
            errs[f"decoder[{tag_n}].loc"] = H.maxdiff(dec["loc"].cpu(), d_want["loc"])
            errs[f"decoder[{tag_n}].pi"] = H.maxdiff(dec["pi"].cpu(), d_want["pi"])
    torch.cuda.synchronize()
    _check_range()
    _report(tag, errs)
    for k, e in errs.items():
        assert e <= TOL, (k, e)


@pytest.mark.parametrize("strength", H.TRAINED_STRENGTHS)
@pytest.mark.parametrize("name", ["mixed_k6_t20", "isolated_k6_t20"])
def test_stages_in_isolation_match_float64_oracle(name, strength, dev):
    """errors cannot cancel between stages"""
    model, cfg, batch, want = _oracle(name, strength)
    _stage_check(model, cfg, batch, want, dev, f"stages {name} s={strength}")


@pytest.mark.parametrize("strength", H.TRAINED_STRENGTHS)
@pytest.mark.parametrize("name", H.IRREGULAR_CASES)
def test_stages_in_isolation_under_irregular_masks(name, strength, dev):
    """_stage_check (diff_in / diff_out picked at eos[agent_index] of agents with a gap among its figures) with every device buffer
    the stages ask for starting as NaN (tests/guarded_memory.py): the aggregate rows of the agents padded at step 20, whom no global
    edge reaches, are the oracle's and not what the workspace held"""
    import guarded_memory as GM
    model, cfg, batch, want = _oracle(name, strength)
    assert int(batch["padding_mask"][:, 20].sum()) >= 4
    gm = GM.GuardedMemory(poison="nan")
    with gm:
        _stage_check(model, cfg, batch, want, dev, f"stages {name} s={strength}")
    assert gm.routed > 0
    rep = gm.check()
    assert rep.ok, str(rep)


@pytest.mark.parametrize("strength", H.TRAINED_STRENGTHS)
def test_aggregator_with_a_scene_beyond_agent_index(strength, dev):
    """a batch vector that names more scenes than agent_index has entries: the last scene's id equals A.  The scene-cached global
    attention's k_scene_ptr must hand such a batch to the gathering kernel, not leave that scene's aggregate rows unwritten"""
    import restate
    from trajsde_amd.data import collate
    from trajsde_amd.runtime import rotate_inputs
    from trajsde_amd.synth import synth
    model, cfg, _ = _model("mixed_k6_t20", strength)
    batch = collate([synth(S=1, n=n, L=4, F=20, box=80.0, seed=40 + n) for n in (9, 14, 11)])
    batch["agent_index"], batch["av_index"] = batch["agent_index"][:2].clone(), batch["av_index"][:2].clone()
    assert int(batch["batch"].max()) == batch["agent_index"].numel()
    c = restate.flat_cfg(cfg)
    P = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    local = torch.randn(batch.num_nodes, 64, generator=torch.Generator().manual_seed(3))
    b64 = H.double_batch(batch)
    rot64, _ = restate.rotate_inputs(b64)
    want = restate.global_interactor(P, c, b64, rot64, local.double())
    model = model.to(dev)
    data = batch.to(dev)
    data["rotate_mat"], _ = rotate_inputs(data)
    with torch.no_grad():
        g = model.aggregator(data=data, local_embed=local.to(dev))
    torch.cuda.synchronize()
    _check_range()
    err = _scaled(g.cpu(), want)
    _report(f"aggregator, scene id == A, s={strength}", {"global_embed": err})
    assert err <= TOL


_MODES = (("split", {}),
          ("fp32", {"TRAJSDE_EDGE_FP32": "1", "TRAJSDE_NODE_FP32": "1", "TRAJSDE_DECODE_FP32": "1", "TRAJSDE_RECUR_LEGACY": "1",
                    "TRAJSDE_GLOBAL_UNFUSED": "1"}),
          ("one_tile", {"TRAJSDE_EDGE_PAIR": "0"}),
          ("two_kernel", {"TRAJSDE_ATTN_FUSED": "0"}),
          ("gattn_vector", {"TRAJSDE_GATTN_F32MM": "0", "TRAJSDE_REL_SPLIT": "0"}),
          ("gattn_f32", {"TRAJSDE_REL_SPLIT": "0"}),
          ("rel_split", {"TRAJSDE_REL_SPLIT": "1"}),
          ("rel_split_scene_cache", {"TRAJSDE_REL_SPLIT": "2"}),
          ("fallbacks", {"TRAJSDE_RECUR_LEGACY": "1", "TRAJSDE_GLOBAL_UNFUSED": "1", "TRAJSDE_NODE_FP32": "0"}))

_CHILD = (
    "import sys, torch; sys.path[:0] = [%r, %r, %r]\n"
    "import helpers as H\n"
    "import test_gpu_trained_weights as W\n"
    "from trajsde_amd import _lib\n"
    "from trajsde_amd.runtime import NoiseSpec\n"
    "outs = {}\n"
    "for s in H.TRAINED_STRENGTHS:\n"
    "    m, cfg, b = W._model(sys.argv[2], s)\n"
    "    with torch.no_grad():\n"
    "        o = m.to('cuda')(b.to('cuda'), noise=NoiseSpec(seed=W.SEED))\n"
    "    _lib.check_range()\n"
    "    outs[s] = {k: o[k].cpu() for k in W.KEYS}\n"
    "torch.save(outs, sys.argv[1])\n")


def _child(tmp_path, mode, env, name="mixed_k6_t20"):
    path = str(tmp_path / (mode + ".pt"))
    script = _CHILD % (H.ROOT, os.path.join(H.ROOT, "tests"), os.path.join(H.ROOT, "oracle"))
    subprocess.run([sys.executable, "-c", script, path, name], check=True, env={**os.environ, **env}, timeout=600)
    return torch.load(path)


def _forms_against_oracle(tmp_path, modes, name="mixed_k6_t20"):
    want = {s: _oracle(name, s)[3] for s in H.TRAINED_STRENGTHS}
    bad = []
    for mode, env in modes:
        got = _child(tmp_path, mode, env, name)
        for s in H.TRAINED_STRENGTHS:
            errs = {k: H.maxdiff(got[s][k], want[s][k]) for k in KEYS}
            _report(f"kernel form {mode}{'' if name == 'mixed_k6_t20' else ' ' + name} s={s}", errs)
            bad += [(mode, s, k, e) for k, e in errs.items() if e > TOL]
    assert not bad, bad


def test_every_kernel_form_matches_float64_oracle(dev, tmp_path):
    """the switch matrix of test_gpu_parity.test_alternative_kernel_paths_agree at both strengths, one interpreter per mode (the
    switches are read once per process) -- each form against the float64 oracle, not only against the others"""
    _forms_against_oracle(tmp_path, _MODES)


def test_strict24_library_matches_float64_oracle(dev, tmp_path):
    """the bf16x6 twin (variants/libtrajsde_strict24.so, made by build()): exact-fp32 products on the plain images"""
    from trajsde_amd import build
    if not os.path.isfile(build.STRICT_LIB):
        pytest.skip("variants/libtrajsde_strict24.so not built")
    _forms_against_oracle(tmp_path, [("strict24", {"TRAJSDE_LIB": build.STRICT_LIB})])


def test_every_kernel_form_under_irregular_masks(dev, tmp_path):
    """the legacy and the cooperative recurrence, the gathering and the scene-cached global attention each carry mask code of their
    own: the same switch matrix on the irregular batch (masked GRU steps before the kept iteration, agents without global edges)"""
    _forms_against_oracle(tmp_path, _MODES, name="irregular_k6_t20")


def test_strict24_library_under_irregular_masks(dev, tmp_path):
    from trajsde_amd import build
    assert os.path.isfile(build.STRICT_LIB), "variants/libtrajsde_strict24.so not built"
    _forms_against_oracle(tmp_path, [("strict24", {"TRAJSDE_LIB": build.STRICT_LIB})], name="irregular_k6_t20")


@pytest.mark.parametrize("strength", H.TRAINED_STRENGTHS)
def test_decoder_without_scale_head(strength, dev):
    """`uncertain: False` (DEC:56): the decoder's plain head image, loc [K, N, T, 2]"""
    from trajsde_amd.runtime import NoiseSpec
    model, cfg, batch = _model("mixed_k6_t20", strength, uncertain=False)
    want = H.oracle_forward64(model, cfg, batch, noise_seed=SEED, want_intermediates=False)
    with torch.no_grad():
        o = model.to(dev)(batch.to(dev), noise=NoiseSpec(seed=SEED))
    torch.cuda.synchronize()
    _check_range()
    assert o["loc"].shape[-1] == 2
    errs = {k: H.maxdiff(o[k].cpu(), want[k]) for k in KEYS}
    _report(f"uncertain=False s={strength}", errs)
    for k, e in errs.items():
        assert e <= TOL, (k, e)


@pytest.mark.parametrize("strength", H.TRAINED_STRENGTHS)
def test_milstein_model(strength, dev):
    """`method: milstein` with the whole model at the profile: the oracle's float64 encoder and interactor, then the float64
    restatement of torchsde's MilsteinIto step (tests/milstein_restate.py)"""
    import milstein_restate as MR
    import restate
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.schedule import decoder_schedule, encoder_schedule
    _milstein_check("mixed_k6_t20", strength, dev, f"milstein s={strength}")


def _milstein_check(name, strength, dev, tag):
    import milstein_restate as MR
    import restate
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.schedule import decoder_schedule, encoder_schedule
    model, cfg, batch = _model(name, strength, method="milstein")
    c = restate.flat_cfg(cfg)
    P = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in model.state_dict().items()}
    b64 = H.double_batch(batch)
    noise = H.Float64Noise(restate.PhiloxNoise(SEED))
    with torch.no_grad():
        rot, _ = restate.rotate_inputs(b64)
        local, di, do, _ = restate.local_encoder(P, c, b64, rot, noise, encoder_schedule(c["historical_steps"], c["max_past_t"], c["minimum_step"]))
        glob = restate.global_interactor(P, c, b64, rot, local)
    want = MR.sde_decoder(P, c, b64, local, glob, noise, decoder_schedule(c["future_steps"], c["max_fut_t"], c["min_stepsize"]))
    want.update(diff_in=di, diff_out=do)
    with torch.no_grad():
        o = model.to(dev)(batch.to(dev), noise=NoiseSpec(seed=SEED))
    torch.cuda.synchronize()
    _check_range()
    errs = {k: H.maxdiff(o[k].cpu(), want[k]) for k in KEYS}
    _report(tag, errs)
    for k, e in errs.items():
        assert e <= TOL, (k, e)


@pytest.mark.parametrize("strength", H.TRAINED_STRENGTHS)
def test_forward_ood(strength, dev):
    """forward_ood (MODEL:89-98, ENC:204-370): no fake agents, ten stochastic encoder passes, per-actor std"""
    from trajsde_amd.runtime import NoiseSpec
    _ood_check("mixed_k6_t20", strength, dev, f"forward_ood s={strength}")


def _ood_check(name, strength, dev, tag):
    from trajsde_amd.runtime import NoiseSpec
    model, cfg, batch = _model(name, strength)
    want = H.oracle_forward64(model, cfg, batch, noise_seed=SEED, want_intermediates=False, ood=True)
    model = model.to(dev)
    model.ood = True
    with torch.no_grad():
        o = model(batch.to(dev), noise=NoiseSpec(seed=SEED))
    torch.cuda.synchronize()
    _check_range()
    errs = {k: H.maxdiff(o[k].cpu(), want[k]) for k in ("stds", "loc", "pi")}
    _report(tag, errs)
    for k, e in errs.items():
        assert e <= TOL, (k, e)


@pytest.mark.parametrize("strength", H.TRAINED_STRENGTHS)
def test_vanilla_grid_forward(strength, dev):
    """the vanilla HiVT variant (temporal transformer encoder, MLP decoder) at the profile against oracle/restate_grid.py"""
    import restate_grid
    from trajsde_amd.models.model_base_mix import PredictionModel
    from trajsde_amd.synth import synth
    K, T = 6, 30
    batch = synth(S=3, n=20, L=9, F=T, box=100.0, seed=720, mixed_source=True, history_dropout=0.4)
    _grid_check(batch, K, T, strength, dev, f"grid s={strength}")


def _grid_check(batch, K, T, strength, dev, tag):
    import restate_grid
    from trajsde_amd.models.model_base_mix import PredictionModel
    model = PredictionModel(**H.grid_cfg(K, T, 4, 4), init_seed=9).eval()
    H.trained_like_parameters(model, H.TRAINED_SEED, strength)
    P = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in model.state_dict().items()}
    want = restate_grid.forward(P, H.grid_cfg(K, T, 4, 4), H.double_batch(batch), True)
    with torch.no_grad():
        o = model.to(dev)(batch.to(dev))
    torch.cuda.synchronize()
    _check_range()
    errs = {k: H.maxdiff(o[k].cpu(), want[k]) for k in ("loc", "pi")}
    errs.update({k: _scaled(o[k].cpu(), want[k]) for k in ("local_embed", "global_embed")})
    _report(tag, errs)
    for k, e in errs.items():
        assert e <= TOL, (k, e)


@pytest.mark.parametrize("strength", H.TRAINED_STRENGTHS)
def test_training_forward(strength, dev):
    """the tape-keeping kernels of a training step (dropout 0) at the profile: their outputs against the oracle"""
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    from trajsde_amd.runtime import NoiseSpec
    _training_forward_check("mixed_k6_t20", strength, dev, f"training forward s={strength}")


def _training_forward_check(name, strength, dev, tag):
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    from trajsde_amd.runtime import NoiseSpec
    K, T, max_t, make = H.TRAINED_CASES[name]
    cfg = H.our_cfg(K, T, max_t)
    cfg["encoder"]["kwargs"]["dropout"] = cfg["aggregator"]["kwargs"]["dropout"] = 0.0
    model = PredictionModelSDENet(**cfg, init_seed=2)
    H.trained_like_parameters(model, H.TRAINED_SEED, strength)
    batch = make()
    want = H.oracle_forward64(model, cfg, batch, noise_seed=SEED)
    model = model.to(dev).train()
    assert float(model.encoder.dropout) == float(model.aggregator.dropout) == 0.0
    out, local, glob, enc_tape, agg_tape = model._forward_stages(batch.to(dev), NoiseSpec(seed=SEED), keep_tapes=True)
    torch.cuda.synchronize()
    _check_range()
    assert enc_tape is not None and agg_tape is not None
    errs = {k: H.maxdiff(out[k].detach().cpu(), want[k]) for k in KEYS}
    errs.update(local_embed=_scaled(local.detach().cpu(), want["local_embed"]), global_embed=_scaled(glob.detach().cpu(), want["global_embed"]))
    _report(tag, errs)
    for k, e in errs.items():
        assert e <= TOL, (k, e)


def test_weight_reload_and_graph_replay(dev):
    """a model run at its initial weights, then given a profile state by load_state_dict: the next forward re-packs and equals, bit
    for bit, a model built with those weights, and matches the oracle; the captured-graph forward at the profile is the eager one"""
    from trajsde_amd import runtime
    from trajsde_amd.runtime import NoiseSpec
    fresh, cfg, batch, want = _oracle("mixed_k6_t20", 2.0)
    reloaded, _ = H.build_model(6, 20, 2.0, init_seed=2)
    reloaded = reloaded.to(dev)
    with torch.no_grad():
        before = reloaded(batch.to(dev), noise=NoiseSpec(seed=SEED))["loc"].clone()
        reloaded.load_state_dict(fresh.state_dict())
        a = reloaded(batch.to(dev), noise=NoiseSpec(seed=SEED))
        fresh = fresh.to(dev)
        b = fresh(batch.to(dev), noise=NoiseSpec(seed=SEED))
    torch.cuda.synchronize()
    _check_range()
    assert not torch.equal(before, a["loc"])
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    errs = {k: H.maxdiff(a[k].cpu(), want[k]) for k in KEYS}
    _report("reloaded s=2.0", errs)
    for k, e in errs.items():
        assert e <= TOL, (k, e)
    data = batch.to(dev)
    gf = runtime.GraphedForward(fresh, data)
    got = {k: gf(seed=SEED)[k].clone() for k in KEYS}
    for k in KEYS:
        assert torch.equal(got[k], b[k]), k


# ----------------------------------------------------------------------------- irregular observation masks (synth.irregular_masks)
# test_forward_matches_float64_oracle runs both H.IRREGULAR_CASES through CASES; the entry points below have mask code of their own
@pytest.mark.parametrize("strength", H.TRAINED_STRENGTHS)
def test_forward_ood_under_irregular_masks(strength, dev):
    """forward_ood's own recurrence loop: masked steps before the kept iteration, rows without a bos"""
    _ood_check("irregular_k6_t20", strength, dev, f"forward_ood irregular_k6_t20 s={strength}")


@pytest.mark.parametrize("strength", H.TRAINED_STRENGTHS)
def test_training_forward_under_irregular_masks(strength, dev):
    _training_forward_check("irregular_k6_t20", strength, dev, f"training forward irregular_k6_t20 s={strength}")


@pytest.mark.parametrize("strength", H.TRAINED_STRENGTHS)
def test_milstein_model_under_irregular_masks(strength, dev):
    _milstein_check("irregular_k6_t20", strength, dev, f"milstein irregular_k6_t20 s={strength}")


@pytest.mark.parametrize("strength", H.TRAINED_STRENGTHS)
def test_vanilla_grid_forward_under_irregular_masks(strength, dev):
    """padding_mask as the temporal transformer's key-padding mask: gaps inside the history, rows padded at every step"""
    from trajsde_amd.synth import irregular
    _grid_check(irregular(S=3, n=13, L=6, F=12, box=80.0, seed=42, mixed_source=True), 3, 12, strength, dev, f"grid, irregular masks, s={strength}")


@pytest.mark.parametrize("strength", H.TRAINED_STRENGTHS)
def test_bf16_state_storage_under_irregular_masks(strength, dev):
    """`set_state_storage("bf16")` on the irregular batch at that storage form's own bound (test_gpu_parity.
    test_stress_shape_config5_fp32_and_bf16_state: finite, within 5e-2 of the fp32-state forward on positions and scales, really
    switched on, and the fp32 path bit for bit itself once the switch is back)"""
    from trajsde_amd import runtime
    from trajsde_amd.runtime import NoiseSpec
    model, cfg, batch, want = _oracle("irregular_k6_t20", strength)
    model = model.to(dev)
    with torch.no_grad():
        o32 = model(H.clone_batch(batch).to(dev), noise=NoiseSpec(seed=SEED))
        prev = runtime.set_state_storage("bf16")
        try:
            o16 = model(H.clone_batch(batch).to(dev), noise=NoiseSpec(seed=SEED))
            torch.cuda.synchronize()
        finally:
            runtime.set_state_storage(prev)
        again = model(H.clone_batch(batch).to(dev), noise=NoiseSpec(seed=SEED))
    assert torch.isfinite(o16["loc"]).all() and torch.isfinite(o16["pi"]).all()
    d_xy = H.maxdiff(o16["loc"][..., :2].cpu(), o32["loc"][..., :2].cpu())
    d_sc = H.maxdiff(o16["loc"][..., 2:].cpu(), o32["loc"][..., 2:].cpu())
    _report(f"bf16 state irregular_k6_t20 s={strength}", {"xy": d_xy, "scale": d_sc, "fp32 loc": H.maxdiff(o32["loc"].cpu(), want["loc"])})
    assert 0.0 < d_xy <= 5e-2, d_xy
    assert d_sc <= 5e-2, d_sc
    assert torch.equal(again["loc"], o32["loc"]) and torch.equal(again["pi"], o32["pi"])
