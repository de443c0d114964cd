"""GPU suite of the decoder's `method: milstein` (-m gpu): the fused Milstein decode (csrc/decoder.hip k_sde_decode<.., MIL = true>)
through trajsde_decoder_forward_milstein against the float64 restatement of torchsde's MilsteinIto (tests/milstein_restate.py)."""
import os
import subprocess
import sys

import pytest
import torch

import helpers as H
import milstein_restate as MR

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    return torch.device("cuda:0")


def _cfg(K, T, max_t, uncertain=True, dec="milstein", enc="milstein"):
    cfg = H.our_cfg(K, T, max_t, uncertain)
    cfg["decoder"]["kwargs"]["method"] = dec
    cfg["encoder"]["kwargs"]["method"] = enc
    return cfg


def _model(K, T, max_t, uncertain=True, init_seed=0, dec="milstein", enc="milstein"):
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    cfg = _cfg(K, T, max_t, uncertain, dec, enc)
    return PredictionModelSDENet(**cfg, init_seed=init_seed).eval(), cfg


def _g_last(decoder):
    return decoder.p("lsde_func.g_func.net.4.weight")


def _stage_inputs(K, T, N, seed, n_euler, dev):
    g = torch.Generator().manual_seed(seed)
    local, glob = torch.randn(N, 64, generator=g), torch.randn(K, N, 64, generator=g)
    z = torch.randn(n_euler, K * N, 64, generator=g)
    data = {"padding_mask": torch.zeros(N, 20 + T, dtype=torch.bool, device=dev)}
    return local, glob, z, data


def _restate_stage(decoder, cfg, local, glob, noise, T, max_t):
    import restate
    from trajsde_amd.schedule import decoder_schedule
    P = {k: v.detach().cpu().double() for k, v in decoder.state_dict().items()}
    sched = decoder_schedule(T, max_t, float(cfg["decoder"]["kwargs"]["min_stepsize"]))
    return MR.sde_decoder(P, restate.flat_cfg(cfg), None, local, glob, noise, sched, pre="")


def _run_stage(K, T, max_t, uncertain, g_last, dev, N=53, seed=1):
    import restate
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.schedule import decoder_schedule
    model, cfg = _model(K, T, max_t, uncertain, init_seed=4)
    dec = model.decoder
    with torch.no_grad():
        for name in dec.state_dict():
            if name.startswith("lsde_func."):
                p = dec.p(name)
                p.add_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())))
        _g_last(dec).mul_(g_last)
    dec = dec.to(dev)
    n_euler = decoder_schedule(T, max_t).n_euler
    local, glob, z, data = _stage_inputs(K, T, N, seed, n_euler, dev)
    out = dec(data=data, local_embed=local.to(dev), global_embed=glob.to(dev), noise=NoiseSpec(seed=0, z_dec=z.to(dev)))
    torch.cuda.synchronize()
    want = _restate_stage(dec, cfg, local, glob, restate.InjectedNoise(None, None, z), T, max_t)
    return dec, cfg, out, want, (local, glob, z, data)


@pytest.mark.parametrize("K,T,max_t", [(6, 20, 2.0), (10, 60, 6.0)])
@pytest.mark.parametrize("uncertain", [True, False])
def test_milstein_decoder_stage_matches_float64_restatement(K, T, max_t, uncertain, dev):
    from trajsde_amd import _lib
    dec, cfg, out, want, _ = _run_stage(K, T, max_t, uncertain, 1.0, dev)
    assert out["loc"].shape == want["loc"].shape
    err = H.maxdiff(out["loc"].cpu(), want["loc"])
    print(f"milstein K={K} T={T} uncertain={uncertain}: max |hip - float64| loc {err:.3e}")
    assert err <= TOL, err
    assert H.maxdiff(out["pi"].cpu(), want["pi"]) <= TOL
    _lib.check_range()


def test_milstein_differs_from_euler_and_still_matches_with_a_large_diffusion_gradient(dev):
    """teeth: GFunc's last layer enlarged (ds/dy not small) -- the Milstein output is far from the Euler one at the same noise, and
    still on the restatement"""
    from trajsde_amd.runtime import NoiseSpec
    dec, cfg, out, want, (local, glob, z, data) = _run_stage(6, 20, 2.0, True, 3.0, dev)
    err = H.maxdiff(out["loc"].cpu(), want["loc"])
    print(f"milstein, GFunc last layer x3: max |hip - float64| loc {err:.3e}")
    assert err <= TOL, err
    dec.method = "euler"
    try:
        eu = dec(data=data, local_embed=local.to(dev), global_embed=glob.to(dev), noise=NoiseSpec(seed=0, z_dec=z.to(dev)))
    finally:
        dec.method = "milstein"
    gap = H.maxdiff(out["loc"].cpu(), eu["loc"].cpu())
    print(f"milstein against euler at the same noise: max |diff| loc {gap:.3e}")
    assert gap > 100 * TOL, gap


def test_milstein_with_philox_noise_matches_restatement_fed_by_the_host_twin(dev):
    import restate
    from trajsde_amd.runtime import NoiseSpec
    K, T, max_t, N = 6, 20, 2.0, 41
    model, cfg = _model(K, T, max_t, init_seed=5)
    dec = model.decoder.to(dev)
    local, glob, _, data = _stage_inputs(K, T, N, 9, 1, dev)
    out = dec(data=data, local_embed=local.to(dev), global_embed=glob.to(dev), noise=NoiseSpec(seed=1234))
    want = _restate_stage(dec, cfg, local, glob, restate.PhiloxNoise(1234), T, max_t)
    assert H.maxdiff(out["loc"].cpu(), want["loc"]) <= TOL
    assert H.maxdiff(out["pi"].cpu(), want["pi"]) <= TOL


def _batch():
    from trajsde_amd.synth import synth
    return synth(S=3, n=20, L=8, F=20, box=90.0, seed=9, mixed_source=True)


def test_whole_model_from_a_milstein_yaml_matches_the_oracle_with_the_milstein_decoder(dev):
    """`method: milstein` in both stages: the decoder solves with Milstein, the encoder with Euler (as the reference's sdeint_dual) --
    diff_in / diff_out are bit for bit the Euler model's"""
    import restate
    from trajsde_amd.runtime import NoiseSpec
    batch = _batch()
    model, cfg = _model(6, 20, 2.0, init_seed=2)
    euler, _ = _model(6, 20, 2.0, init_seed=2, dec="euler", enc="euler")
    P = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    want = MR.forward(P, cfg, H.clone_batch(batch), restate.PhiloxNoise(6))
    with torch.no_grad():
        got = model.to(dev)(batch.to(dev), noise=NoiseSpec(seed=6))
        eu = euler.to(dev)(batch.to(dev), noise=NoiseSpec(seed=6))
    for key in ("loc", "pi", "diff_in", "diff_out"):
        assert H.maxdiff(got[key].cpu(), want[key]) <= TOL, key
    for key in ("diff_in", "diff_out", "pi"):
        assert torch.equal(got[key], eu[key]), key
    assert H.maxdiff(got["loc"].cpu(), eu["loc"].cpu()) > 10 * TOL


_CHILD = (
    "import sys, torch; sys.path[:0] = [%r, %r, %r]\n"
    "import test_gpu_milstein as M\n"
    "from trajsde_amd.runtime import NoiseSpec\n"
    "m, cfg = M._model(6, 20, 2.0, init_seed=2)\n"
    "with torch.no_grad():\n"
    "    o = m.to('cuda')(M._batch().to('cuda'), noise=NoiseSpec(seed=6))\n"
    "torch.save({k: v.cpu() for k, v in o.items() if k in ('loc', 'pi', 'diff_in', 'diff_out')}, sys.argv[1])\n")


def _child(tmp_path, name, env):
    path = str(tmp_path / (name + ".pt"))
    script = _CHILD % (H.ROOT, os.path.join(H.ROOT, "tests"), os.path.join(H.ROOT, "oracle"))
    subprocess.run([sys.executable, "-c", script, path], check=True, env={**os.environ, **env}, timeout=600)
    return torch.load(path)


def test_plain_image_form_agrees_with_the_default(dev, tmp_path):
    """TRAJSDE_DECODE_FP32=1 (the plain decode image DecSdeL + MilL) against the fp16x3 default (DecSdeL6 + MilL)"""
    a, b = _child(tmp_path, "split", {}), _child(tmp_path, "fp32", {"TRAJSDE_DECODE_FP32": "1"})
    for key in a:
        assert H.maxdiff(a[key], b[key]) <= 2e-5, key


def test_strict_library_matches_the_restatement(dev, tmp_path):
    """the bf16x6 twin (variants/libtrajsde_strict24.so, made by build()): its Milstein path takes the plain-image form"""
    import restate
    from trajsde_amd import build
    if not os.path.isfile(build.STRICT_LIB):
        pytest.skip("variants/libtrajsde_strict24.so not built")
    got = _child(tmp_path, "strict", {"TRAJSDE_LIB": build.STRICT_LIB})
    model, cfg = _model(6, 20, 2.0, init_seed=2)
    P = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    want = MR.forward(P, cfg, H.clone_batch(_batch()), restate.PhiloxNoise(6))
    for key in ("loc", "pi", "diff_in", "diff_out"):
        assert H.maxdiff(got[key], want[key]) <= TOL, key


def test_two_identical_milstein_calls_are_bitwise_identical(dev):
    from trajsde_amd.runtime import NoiseSpec
    dec, cfg, out, want, (local, glob, z, data) = _run_stage(10, 60, 6.0, True, 1.0, dev, N=97)
    again = dec(data=data, local_embed=local.to(dev), global_embed=glob.to(dev), noise=NoiseSpec(seed=0, z_dec=z.to(dev)))
    assert torch.equal(out["loc"], again["loc"]) and torch.equal(out["pi"], again["pi"])
    a = dec(data=data, local_embed=local.to(dev), global_embed=glob.to(dev), noise=NoiseSpec(seed=77))
    b = dec(data=data, local_embed=local.to(dev), global_embed=glob.to(dev), noise=NoiseSpec(seed=77))
    assert torch.equal(a["loc"], b["loc"])


def test_graph_replay_of_a_milstein_model_is_the_eager_forward(dev):
    from trajsde_amd import runtime
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import synth
    K, T = 3, 6
    batch = synth(S=4, n=40, L=12, F=T, box=80.0, seed=31, mixed_source=True)
    model, cfg = _model(K, T, 0.5, init_seed=6)
    model = model.to(dev).eval()
    gf = runtime.GraphedForward(model, batch.to(dev))
    for seed in (5, 77):
        got = {k: gf(seed=seed)[k].clone() for k in ("loc", "pi", "diff_in", "diff_out")}
        with torch.no_grad():
            want = model(batch.to(dev), noise=NoiseSpec(seed=seed))
        for k in got:
            assert torch.equal(got[k], want[k]), (seed, k)
