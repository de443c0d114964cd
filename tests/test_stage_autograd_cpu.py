"""The stages as torch.autograd nodes (`autograd: true`, trajsde_amd/stage_autograd.py) and the encoder backward from cotangents
(trajsde_encoder_cotangent_backward), the parts that need no GPU: the extension header against its `_lib` table, the exported symbol,
the stage kwarg on the host, and the reference's own glue class resolving our stage files with the switch among their kwargs."""
import copy
import os
import sys

import pytest
import torch

import helpers as H

NAME = "trajsde_encoder_cotangent_backward"
HEADER = "trajsde_hip_encoder_cotangent.h"
STAGES = ("encoder", "aggregator", "decoder")


def _cfg(K=3, T=5, max_t=0.5, **decoder_kw):
    cfg = H.our_cfg(K, T, max_t)
    for s in STAGES:
        cfg[s]["kwargs"]["autograd"] = True
    cfg["decoder"]["kwargs"].update(decoder_kw)
    return cfg


def test_the_symbol_is_exported_by_the_built_libraries():
    from trajsde_amd import _lib
    lib = _lib.lib()
    assert hasattr(lib, NAME)
    assert getattr(lib, NAME).argtypes == _lib.ENC_COT_EXT_SIGNATURES[NAME][1]
    assert lib.trajsde_abi_version() == 10


def test_extension_header_and_its_signature_table_agree(tmp_path):
    """include/trajsde_hip_encoder_cotangent.h against `_lib.ENC_COT_EXT_SIGNATURES`, by the rules tests/test_cotangent_cpu.py applies to
    trajsde_hip_cotangent.h; the table overlaps no other table, the header no other header; the arguments are trajsde_encoder_backward's
    with (float diff_weight, ..., float* diff_loss) replaced by the two cotangent pointers"""
    import re

    import test_cabi_cpu as CABI
    from trajsde_amd import _lib
    inc = os.path.join(H.ROOT, "include")
    text = open(os.path.join(inc, HEADER)).read()
    assert '#include "trajsde_hip.h"' in text
    body = text.replace('#include "trajsde_hip.h"', "")
    declared = set(re.findall(r"\b(trajsde_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", " ", body, flags=re.S)))
    assert declared == set(_lib.ENC_COT_EXT_SIGNATURES) == {NAME}
    for other in (_lib.SIGNATURES, _lib.EXT_SIGNATURES, _lib.COT_SEL_EXT_SIGNATURES, _lib.GRID_EXT_SIGNATURES, _lib.CLIP_EXT_SIGNATURES):
        assert not set(_lib.ENC_COT_EXT_SIGNATURES) & set(other)
    for h in sorted(os.listdir(inc)):
        if h != HEADER:
            assert not declared & set(re.findall(r"\b(trajsde_[a-z_0-9]+)\s*\(", open(os.path.join(inc, h)).read())), h
    protos = CABI._header_prototypes(body)
    assert set(protos) == declared
    assert CABI._check_against_header(_lib.ENC_COT_EXT_SIGNATURES, protos) == []
    swap = lambda tu: tu.replace('"trajsde_hip.h"', f'"{HEADER}"')
    r = CABI._compile_tu(swap(CABI._prototype_tu(_lib.ENC_COT_EXT_SIGNATURES, protos)), tmp_path, H.ROOT, "enc_cot")
    assert r.returncode == 0, r.stdout[-3000:]
    bad = dict(_lib.ENC_COT_EXT_SIGNATURES)                     # the check has teeth: one cotangent pointer fewer is caught both ways
    res, args = bad[NAME]
    bad[NAME] = (res, args[:9] + args[10:])
    assert CABI._check_against_header(bad, protos)
    assert CABI._compile_tu(swap(CABI._prototype_tu(bad, protos)), tmp_path, H.ROOT, "enc_cot_bad").returncode != 0
    welded = _lib.SIGNATURES["trajsde_encoder_backward"][1]
    assert welded[9] is _lib.F32 and welded[12] is _lib.P                  # diff_weight, diff_loss
    assert args == welded[:9] + [_lib.P, _lib.P] + welded[10:12] + welded[13:]


def test_the_stages_construct_with_the_switch_on_the_host_with_unchanged_keys():
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    plain = PredictionModelSDENet(**H.our_cfg(3, 5, 0.5), init_seed=0)
    model = PredictionModelSDENet(**_cfg(), init_seed=0)
    for s in STAGES:
        assert getattr(model, s).autograd is True and not getattr(getattr(plain, s), "autograd", False)
    assert list(model.state_dict()) == list(plain.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), plain.state_dict().values()))
    assert [n for n, _ in model.named_parameters()] == [n for n, _ in plain.named_parameters()]
    assert model.decoder.last_support_status is None
    assert PredictionModelSDENet(**_cfg(cotangent_support="winner"), init_seed=0).decoder.cotangent_support == "winner"


def test_the_node_is_taken_only_where_a_gradient_is_wanted():
    from trajsde_amd import stage_autograd
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    model = PredictionModelSDENet(**_cfg(), init_seed=0)
    plain = PredictionModelSDENet(**H.our_cfg(3, 5, 0.5), init_seed=0)
    x = torch.zeros(2, 64)
    assert stage_autograd.active(model.aggregator, x) and not stage_autograd.active(plain.aggregator, x.requires_grad_(True))
    with torch.no_grad():
        assert not stage_autograd.active(model.aggregator, x)
    with torch.inference_mode():
        assert not stage_autograd.active(model.encoder)
    for p in model.decoder.parameters():
        p.requires_grad_(False)
    assert not stage_autograd.active(model.decoder, x.detach(), None) and stage_autograd.active(model.decoder, x.detach(), x)


def test_host_tensors_are_refused_on_the_node_route():
    from trajsde_amd import _lib
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    from trajsde_amd.synth import synth
    model = PredictionModelSDENet(**_cfg(), init_seed=0)
    batch = synth(S=1, n=6, L=4, F=5, box=60.0, seed=2)
    with pytest.raises(_lib.TrajsdeError, match="GPU"):
        model.encoder(data=batch)
    with pytest.raises(_lib.TrajsdeError, match="GPU"):
        model.aggregator(data=batch, local_embed=torch.zeros(6, 64))
    with pytest.raises(_lib.TrajsdeError, match="GPU"):
        model.decoder(data=batch, local_embed=torch.zeros(6, 64), global_embed=torch.zeros(3, 6, 64))


def test_milstein_and_a_decoder_without_its_scale_head_are_refused():
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    with pytest.raises(NotImplementedError, match="Euler-only cotangent route"):
        PredictionModelSDENet(**_cfg(T=20, max_t=2.0, method="milstein"), init_seed=0)
    with pytest.raises(NotImplementedError, match="uncertain"):
        PredictionModelSDENet(**_cfg(uncertain=False), init_seed=0)
    with pytest.raises(ValueError, match="cotangent_support"):
        PredictionModelSDENet(**_cfg(cotangent_support="best"), init_seed=0)
    # the switch set on a built stage is checked where the node would be entered
    model = PredictionModelSDENet(**H.our_cfg(3, 20, 2.0), init_seed=0)
    model.decoder.method, model.decoder.autograd = "milstein", True
    with pytest.raises(NotImplementedError, match="Euler-only cotangent route"):
        model.decoder(data=None, local_embed=torch.zeros(6, 64), global_embed=torch.zeros(3, 6, 64))


def test_the_references_own_glue_resolves_our_stages_with_the_switch():
    """the stage-level swap: three `file_path` strings of the reference's YAML pointed at our stage files, `autograd: true` among their
    kwargs, inside the reference's own PredictionModelSDENet"""
    sys.path.insert(0, os.path.join(H.ROOT, "oracle"))
    import ref_loader as R
    if not R.reference_available():
        pytest.skip("the reference tree is not on this machine")
    ours = H.our_cfg(3, 5, 0.5)
    cfg = copy.deepcopy(R.load_reference_cfg(num_modes=3, future_steps=5, max_fut_t=0.5))
    for s in STAGES:
        cfg[s]["file_path"] = os.path.join(H.ROOT, ours[s]["file_path"])
        assert cfg[s]["module_name"] == ours[s]["module_name"]
        cfg[s]["kwargs"]["autograd"] = True
    ref = R.build_reference_model(cfg)
    assert type(ref).__module__ != "trajsde_amd.models.model_base_mix_sde"
    from trajsde_amd.models.params import ParamTree
    for s in STAGES:
        stage = getattr(ref, s)
        assert isinstance(stage, ParamTree) and stage.autograd is True and hasattr(stage, "_rt"), s
        assert os.path.samefile(sys.modules[type(stage).__module__].__file__, cfg[s]["file_path"]), s
    plain = H.build_model(3, 5, 0.5)[0]
    assert set(ref.state_dict()) == set(plain.state_dict())
