"""The vanilla HiVT stages as torch.autograd nodes (`autograd: true` among the kwargs of LocalEncoder / GlobalInteractor / MLPDecoder;
trajsde_amd/stage_autograd.py GridEncoderNode / MLPDecoderNode), the parts that need no GPU: the stage kwarg on the host, when the node is
taken, the refusals, and the reference's own PredictionModel resolving our three stage files with the switch among their kwargs."""
import copy
import os
import sys

import pytest
import torch
import yaml

import helpers as H

STAGES = ("encoder", "aggregator", "decoder")
REF_GRID_CFG = "configs/nusargo/hivt_nuSArgo_trmenc_mlpdec.yml"


def _cfg(K=3, T=5, heads=4, layers=1, **decoder_kw):
    cfg = H.grid_cfg(K, T, heads, layers, dropout=0.1)
    for s in STAGES:
        cfg[s]["kwargs"]["autograd"] = True
    cfg["decoder"]["kwargs"].update(decoder_kw)
    return cfg


def _model(cfg):
    from trajsde_amd.models.model_base_mix import PredictionModel
    return PredictionModel(**cfg, init_seed=0)


def test_the_vanilla_stages_construct_with_the_switch_on_the_host_with_unchanged_keys():
    from trajsde_amd import stage_autograd
    plain, model = _model(H.grid_cfg(3, 5, 4, 1, dropout=0.1)), _model(_cfg())
    for s in STAGES:
        assert getattr(model, s).autograd is True and not getattr(getattr(plain, s), "autograd", False)
    assert list(model.state_dict()) == list(plain.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), plain.state_dict().values()))
    assert [n for n, _ in model.named_parameters()] == [n for n, _ in plain.named_parameters()]
    assert issubclass(stage_autograd.GridEncoderNode, torch.autograd.Function)
    assert issubclass(stage_autograd.MLPDecoderNode, torch.autograd.Function)


def test_the_node_is_taken_only_where_a_gradient_is_wanted():
    from trajsde_amd import stage_autograd
    model, plain = _model(_cfg()), _model(H.grid_cfg(3, 5, 4, 1))
    x = torch.zeros(2, 64)
    assert stage_autograd.active(model.encoder) and not stage_autograd.active(plain.encoder)
    assert stage_autograd.active(model.decoder, x, None) and not stage_autograd.active(plain.decoder, x.requires_grad_(True), None)
    with torch.no_grad():
        assert not stage_autograd.active(model.encoder) and not stage_autograd.active(model.decoder, x, x)
    with torch.inference_mode():
        assert not stage_autograd.active(model.encoder)
    for p in model.parameters():
        p.requires_grad_(False)
    assert not stage_autograd.active(model.encoder)
    assert not stage_autograd.active(model.decoder, x.detach(), None) and stage_autograd.active(model.decoder, x.detach(), x)


def test_the_parameters_of_a_node_cover_its_backward_table():
    """what the nodes hand back per parameter is looked up by name in the stage's backward table: every name of the table is a
    parameter of the module, so no gradient is dropped on the way"""
    from trajsde_amd import _lib
    model = _model(_cfg(layers=2))
    for stage, sid in (("encoder", _lib.STAGE_ENCODER_GRID_BWD), ("aggregator", _lib.STAGE_AGGREGATOR_BWD),
                       ("decoder", _lib.STAGE_DECODER_MLP_COT_BWD)):
        m = getattr(model, stage)
        own = [n for n, _ in m.named_parameters()]
        table = m._rt.param_names(sid)
        assert set(table) <= set(own) and len(set(table)) == len(table), stage
    assert {"pi.6.weight", "scale.3.bias"} <= set(model.decoder._rt.param_names(_lib.STAGE_DECODER_MLP_COT_BWD))


def test_host_tensors_are_refused_on_the_node_route():
    from trajsde_amd import _lib
    from trajsde_amd.synth import synth
    model = _model(_cfg())
    batch = synth(S=1, n=6, L=4, F=5, box=60.0, seed=2)
    with pytest.raises(_lib.TrajsdeError, match="GPU"):
        model.encoder(data=batch)
    with pytest.raises(_lib.TrajsdeError, match="GPU"):
        model.aggregator(data=batch, local_embed=torch.zeros(6, 64))
    with pytest.raises(_lib.TrajsdeError, match="GPU"):
        model.decoder(data=batch, local_embed=torch.zeros(6, 64), global_embed=torch.zeros(3, 6, 64))


def test_a_decoder_without_its_scale_head_is_refused_with_the_switch():
    with pytest.raises(NotImplementedError, match="uncertain"):
        _model(_cfg(uncertain=False))
    cfg = H.grid_cfg(3, 5, 4, 1, uncertain=False)                 # the switch off: built as before
    assert _model(cfg).decoder.uncertain is False
    model = _model(cfg)                                            # the switch set on a built stage is checked where the node is entered
    model.decoder.autograd = True
    with pytest.raises(NotImplementedError, match="uncertain"):
        model.decoder(data=None, local_embed=torch.zeros(6, 64), global_embed=torch.zeros(3, 6, 64))


def test_forward_takes_the_exact_graph_request_as_a_keyword():
    """`training_step` asks for the exact graph by keyword (grad mode cannot tell it from an inference forward); the stage and the
    runtime pass it on"""
    import inspect
    from trajsde_amd import runtime
    from trajsde_amd.models.encoders.enc_hivt_nusargo_grid import LocalEncoder
    from trajsde_amd.models.model_base_mix import PredictionModel
    assert inspect.signature(PredictionModel.forward).parameters["exact_graph"].default is False
    assert inspect.signature(LocalEncoder.forward).parameters["exact_graph"].default is False
    assert inspect.signature(runtime.StageRuntime.encoder_grid_forward).parameters["exact"].default is False


def test_the_references_own_glue_resolves_our_vanilla_stages_with_the_switch():
    """the stage-level swap of the vanilla configuration: the three `file_path` strings of the reference's YAML pointed at our stage
    files, `autograd: true` among their kwargs, inside the reference's own PredictionModel"""
    sys.path.insert(0, os.path.join(H.ROOT, "oracle"))
    import ref_loader as R
    if not R.reference_available():
        pytest.skip("the reference tree is not on this machine")
    ours = H.grid_cfg(3, 5, 4, 1, dropout=0.1)
    with open(os.path.join(R.REFERENCE_ROOT, REF_GRID_CFG)) as f:
        cfg = copy.deepcopy(yaml.safe_load(f))
    cfg["model_specific"]["kwargs"].update(num_modes=3, future_steps=5)
    cfg["aggregator"]["kwargs"]["num_modes"] = 3
    cfg["decoder"]["kwargs"].update(num_modes=3, future_steps=5)
    cfg["encoder"]["kwargs"]["num_temporal_layers"] = 1
    for s in STAGES:
        cfg[s]["file_path"] = os.path.join(H.ROOT, ours[s]["file_path"])
        assert cfg[s]["module_name"] == ours[s]["module_name"]
        cfg[s]["kwargs"]["autograd"] = True
    ref = R.build_reference_model(cfg)
    assert type(ref).__name__ == "PredictionModel" and type(ref).__module__ != "trajsde_amd.models.model_base_mix"
    from trajsde_amd import stage_autograd
    from trajsde_amd.models.params import ParamTree
    for s in STAGES:
        stage = getattr(ref, s)
        assert isinstance(stage, ParamTree) and stage.autograd is True and hasattr(stage, "_rt"), s
        assert os.path.samefile(sys.modules[type(stage).__module__].__file__, cfg[s]["file_path"]), s
    assert stage_autograd.active(ref.encoder) and stage_autograd.active(ref.decoder, torch.zeros(2, 64), None)
    assert set(ref.state_dict()) == set(_model(ours).state_dict())
