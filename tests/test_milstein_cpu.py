"""CPU suite of the decoder's `method: milstein` (csrc/decoder.hip k_sde_decode<.., MIL = true>): the float64 restatement and the
closed form the kernel implements, the stages' `method` handling, the refusal to train, and the kernels' listing (no scratch)."""
import os
import re
import subprocess

import pytest
import torch

import helpers as H
import milstein_restate as MR


def _random_gfunc(seed):
    g = torch.Generator().manual_seed(seed)
    P = {"g.net.0.weight": torch.randn(64, 66, generator=g, dtype=torch.float64) * 0.3,
         "g.net.0.bias": torch.randn(64, generator=g, dtype=torch.float64) * 0.2,
         "g.net.2.weight": torch.randn(64, 64, generator=g, dtype=torch.float64) * 0.3,
         "g.net.2.bias": torch.randn(64, generator=g, dtype=torch.float64) * 0.2,
         "g.net.4.weight": torch.randn(1, 64, generator=g, dtype=torch.float64) * 0.5,
         "g.net.4.bias": torch.randn(1, generator=g, dtype=torch.float64) * 0.2}
    y = torch.randn(37, 64, generator=g, dtype=torch.float64)
    return P, y, g


def test_closed_form_ds_dy_matches_autograd():
    """the formula of csrc/sde_funcs.hpp gfunc_input_grad, on random weights, against autograd of GFunc"""
    import restate
    P, y, _ = _random_gfunc(3)
    got, _ = MR.ds_dy_closed_form(P, "g", y, 0.4, -0.7)
    yy = y.clone().requires_grad_(True)
    s = restate.diffusion(P, "g", yy, 0.4, -0.7)
    (want,) = torch.autograd.grad(s.sum(), yy)                   # rows are independent: the sum's gradient is per-row ds/dy
    assert float((got - want).abs().max()) <= 1e-12


def test_restated_gdg_is_the_column_sum_of_the_broadcast_diffusion():
    """vjp(g.repeat(1, 64), y, g * v2) = s (sum_i v2_i) ds/dy -- torchsde's term for this module, not the textbook diagonal one"""
    P, y, g = _random_gfunc(5)
    v2 = 0.5 * (torch.randn(37, 64, generator=g, dtype=torch.float64) ** 2 * 0.1 - 0.1)
    gb, gdg = MR.gdg_autograd(P, "g", y, 0.1, 0.2, v2)
    dsdy, s = MR.ds_dy_closed_form(P, "g", y, 0.1, 0.2)
    assert torch.equal(gb, s.expand(-1, 64))
    want = s * v2.sum(1, keepdim=True) * dsdy
    assert float((gdg - want).abs().max()) <= 1e-12
    diagonal = s * v2 * dsdy                                     # the textbook term differs
    assert float((gdg - diagonal).abs().max()) > 1e-3


def _cfg(dec_method="euler", enc_method="euler", **enc):
    cfg = H.our_cfg(6, 20, 2.0)
    cfg["decoder"]["kwargs"]["method"] = dec_method
    cfg["encoder"]["kwargs"]["method"] = enc_method
    cfg["encoder"]["kwargs"].update(enc)
    return cfg


def _decoder(method, **kw):
    from trajsde_amd.models.decoders.dec_hivt_nusargo_sde import SDEDecoder
    k = dict(_cfg()["decoder"]["kwargs"])
    k.update(method=method, init_seed=0, **kw)
    return SDEDecoder(**k)


def test_decoder_accepts_milstein_with_the_euler_state_dict_keys():
    for uncertain in (True, False):
        a, b = _decoder("euler", uncertain=uncertain), _decoder("milstein", uncertain=uncertain)
        assert b.method == "milstein"
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb)
        assert all(torch.equal(sa[k], sb[k]) for k in sa)


def test_decoder_refuses_what_is_not_built_or_not_ito():
    with pytest.raises(NotImplementedError, match="srk"):
        _decoder("srk")
    with pytest.raises(NotImplementedError, match="srk"):
        _decoder(None)                                          # torchsde's default for this SDE is srk
    from trajsde_amd.models.decoders.dec_hivt_nusargo_sde import SDEDecoder
    k = {key: v for key, v in _cfg()["decoder"]["kwargs"].items() if key != "method"}
    with pytest.raises(NotImplementedError, match="srk"):
        SDEDecoder(**k)                                         # no `method` kwarg at all: None
    with pytest.raises(ValueError):
        _decoder("foo")
    for name in ("midpoint", "heun", "reversible_heun", "adjoint_reversible_heun", "log_ode", "euler_heun"):
        with pytest.raises(ValueError, match="Stratonovich"):
            _decoder(name)


def test_encoder_accepts_every_method_name_and_runs_euler():
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    from trajsde_amd.schedule import SDE_METHODS
    base = PredictionModelSDENet(**_cfg(), init_seed=0).encoder.state_dict()
    for name in (None,) + SDE_METHODS:
        enc = PredictionModelSDENet(**_cfg(enc_method=name), init_seed=0).encoder
        sd = enc.state_dict()
        assert list(sd) == list(base) and all(torch.equal(sd[k], base[k]) for k in sd)
    with pytest.raises(ValueError):
        PredictionModelSDENet(**_cfg(enc_method="foo"), init_seed=0)
    for bad in (dict(adaptive=True), dict(run_backwards=False), dict(sde_layers=3)):
        with pytest.raises(NotImplementedError):
            PredictionModelSDENet(**_cfg(enc_method="milstein", **bad), init_seed=0)


def test_milstein_model_builds_from_yaml_in_both_stages_and_refuses_training_on_cpu():
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import synth
    model = PredictionModelSDENet(**_cfg("milstein", "milstein"), init_seed=0).train()
    euler = PredictionModelSDENet(**_cfg(), init_seed=0)
    assert list(model.state_dict()) == list(euler.state_dict())
    batch = synth(S=1, n=8, L=4, F=20, box=60.0, seed=2)
    with pytest.raises(NotImplementedError, match="milstein"):
        model.training_step(batch, 0, noise=NoiseSpec(seed=1))
    with pytest.raises(NotImplementedError, match="milstein"):
        model.decoder._rt.decoder_l2_backward(batch, None, None, {}, NoiseSpec(seed=1))


def test_milstein_stage_table_is_the_decoder_table():
    """TRAJSDE_STAGE_DECODER_MILSTEIN packs the decoder's parameters, into the decoder blob + two 64x64 images"""
    from trajsde_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.lib()

    def names(stage):
        return [lib.trajsde_param_name(stage, i, 0, 6).decode() for i in range(lib.trajsde_param_count(stage, 0, 6))]
    assert names(_lib.STAGE_DECODER_MILSTEIN) == names(_lib.STAGE_DECODER)
    assert lib.trajsde_blob_floats(_lib.STAGE_DECODER_MILSTEIN, 0, 6) == lib.trajsde_blob_floats(_lib.STAGE_DECODER, 0, 6) + 2 * 64 * 64


@pytest.mark.parametrize("extra,expect", [([], 4), (["-DTSDE_SPLIT_H3=0"], 1)])
def test_milstein_decode_kernels_compile_without_scratch(tmp_path, extra, expect):
    """every Milstein instantiation (fp16x3: split and plain image, 512 and 768 threads; bf16x6: the plain image at 512 threads) holds
    its state, GFunc's activations and the input gradient in registers"""
    from trajsde_amd import build
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    out = tmp_path / "decoder.s"
    src = os.path.join(H.ROOT, "trajsde_amd", "csrc", "decoder.hip")
    subprocess.check_call([build.HIPCC, *flags, *extra, "--cuda-device-only", "-S", "-o", str(out), src],
                          stderr=subprocess.DEVNULL)
    text = out.read_text()
    kernels = re.findall(r"^(_ZN4tsde12k_sde_decodeILb[01]ELi\d+ELb1E\w+):.*?; ScratchSize: (\d+)", text, flags=re.S | re.M)
    assert len(kernels) == expect, kernels
    assert all(int(sz) == 0 for _, sz in kernels), kernels
