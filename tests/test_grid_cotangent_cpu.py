"""The MLP decoder's backward from caller-supplied cotangents (trajsde_mlp_decoder_cotangent_backward), the parts that need no GPU:
the parameter table and image size of TRAJSDE_STAGE_DECODER_MLP_COT_BWD, the extension header against its ctypes table, the workspace
query and its refusals, the parameters the cotangent route reaches and the loss routing of `PredictionModel.training_step`."""
import pytest
import torch

import helpers as H

PI = ["pi.0.weight", "pi.0.bias", "pi.1.weight", "pi.1.bias", "pi.3.weight", "pi.3.bias", "pi.4.weight", "pi.4.bias", "pi.6.weight",
      "pi.6.bias"]
SCALE = ["scale.0.weight", "scale.0.bias", "scale.1.weight", "scale.1.bias", "scale.3.weight", "scale.3.bias"]
CUSTOM = ["L2", "SoftTargetCrossEntropyLoss"]


def _names(lib, stage, nl, K):
    return [lib.trajsde_param_name(stage, i, nl, K).decode() for i in range(lib.trajsde_param_count(stage, nl, K))]


def _model(modules, K=3, T=12, **kw):
    from trajsde_amd.models.model_base_mix import PredictionModel
    cfg = H.grid_cfg(K, T, 4, 2, **kw)
    cfg["losses"] = ["trajsde_amd/losses.py"] * len(modules)
    cfg["losses_module"] = list(modules)
    cfg["loss_weights"] = [1.0] * len(modules)
    cfg["loss_args"] = [{} for _ in modules]
    return PredictionModel(**cfg, init_seed=0).eval()


@pytest.mark.parametrize("T", [12, 30, 64])
def test_stage_16_table_is_the_mlp_nll_table_followed_by_the_pi_head(T):
    from trajsde_amd import _lib
    lib = _lib.lib()
    assert _lib.STAGE_DECODER_MLP_COT_BWD == 16
    with open(H.ROOT + "/include/trajsde_hip.h") as f:
        assert "TRAJSDE_STAGE_DECODER_MLP_COT_BWD = 16" in f.read()
    assert lib.trajsde_abi_version() == 10
    nll, cot = _names(lib, _lib.STAGE_DECODER_MLP_NLL_BWD, T, 6), _names(lib, _lib.STAGE_DECODER_MLP_COT_BWD, T, 6)
    assert len(cot) == 26 and cot[:16] == nll and cot[16:] == PI
    # every parameter of the decoder, each once
    dec = dict(_model(["L2"], K=6, T=T).decoder.named_parameters())
    assert set(cot) == set(dec) and len(set(cot)) == 26
    image = lib.trajsde_blob_floats(_lib.STAGE_DECODER_MLP_COT_BWD, T, 6) - lib.trajsde_blob_floats(_lib.STAGE_DECODER_MLP_NLL_BWD, T, 6)
    # one MlpPiBwdL image: pi.0 as two 64 x 64 halves, pi.3, their three transposes; b0, b3, two LayerNorm affines, w6 (seven vectors of 64); b6 padded to 4
    assert image == 6 * 64 * 64 + 7 * 64 + 4 == 25028


def test_workspace_query_is_positive_monotone_and_refuses():
    from trajsde_amd import _lib
    lib = _lib.lib()
    q = lib.trajsde_mlp_decoder_cotangent_backward_ws_bytes
    base = (17, 3, 12)
    b0 = q(*base)
    assert b0 > 0
    for arg in range(2):                                                  # (the workspace does not depend on T: the rows hold 128 outputs)
        prev = b0
        for step in (1, 2, 15, 16, 17, 100):
            args = list(base)
            args[arg] += step
            cur = q(*args)
            assert cur >= prev > 0, (arg, step, cur, prev)
            prev = cur
    assert q(17, 3, 64) == b0 == q(17, 3, 1)
    for bad in ((0, 3, 12), (17, 0, 12), (17, 3, 0), (17, 3, 65), (1 << 30, 4, 12)):
        assert q(*bad) < 0, bad                                           # refused, with a message
        assert b"mlp_decoder_cotangent_backward" in lib.trajsde_last_error()


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """null pointers, a wrong gradient count, future_steps outside 1..64, an empty or oversized problem and a short workspace: each
    refused with a message by the host-side checks (no GPU is touched: they come before the first launch)"""
    import ctypes as C
    from trajsde_amd import _lib
    lib = _lib.lib()
    f = lib.trajsde_mlp_decoder_cotangent_backward
    p = C.cast(C.create_string_buffer(64), C.c_void_p).value              # a non-null stand-in: never dereferenced by the checks
    grads = (C.c_void_p * 26)(*([p] * 26))
    ok = dict(N=17, K=3, T=12, blob=p, lo=p, gl=p, loc=p, ms=0.001, dloc=p, dpi=p, ws=p, wsb=1 << 40, grads=grads, n=26, dl=p, dg=p)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["N"], a["K"], a["T"], a["blob"], a["lo"], a["gl"], a["loc"], a["ms"], a["dloc"], a["dpi"], a["ws"], a["wsb"], a["grads"],
                 a["n"], a["dl"], a["dg"], None)
    for kw, msg in ((dict(blob=None), b"null pointer"), (dict(dpi=None), b"null pointer"), (dict(dg=None), b"null pointer"),
                    (dict(n=16), b"gradient count"), (dict(T=0), b"future_steps"), (dict(T=65), b"future_steps"),
                    (dict(N=0), b"empty or oversized"), (dict(N=1 << 30, K=4), b"empty or oversized"),
                    (dict(wsb=lib.trajsde_mlp_decoder_cotangent_backward_ws_bytes(17, 3, 12) - 1), b"workspace too small")):
        assert call(**kw) != 0, kw
        assert msg in lib.trajsde_last_error(), (kw, lib.trajsde_last_error())
    one_null = (C.c_void_p * 26)(*([p] * 25 + [None]))
    assert call(grads=one_null) != 0 and b"null gradient buffer" in lib.trajsde_last_error()


def test_grid_extension_header_and_its_signature_table_agree(tmp_path):
    """include/trajsde_hip_grid_cotangent.h against `_lib.GRID_EXT_SIGNATURES`, by the rules tests/test_cabi_cpu.py applies to
    trajsde_hip.h and `_lib.SIGNATURES` (its helpers, imported); the library exports the symbols; no table or header overlaps another"""
    import os
    import re

    import test_cabi_cpu as CABI
    from trajsde_amd import _lib
    inc = os.path.join(H.ROOT, "include")
    text = open(os.path.join(inc, "trajsde_hip_grid_cotangent.h")).read()
    body = text.replace('#include "trajsde_hip.h"', "")
    find = lambda s: set(re.findall(r"\b(trajsde_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", " ", s, flags=re.S)))
    declared = find(body)
    assert declared == set(_lib.GRID_EXT_SIGNATURES) == {"trajsde_mlp_decoder_cotangent_backward",
                                                         "trajsde_mlp_decoder_cotangent_backward_ws_bytes"}
    assert not set(_lib.GRID_EXT_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES))
    for other in ("trajsde_hip.h", "trajsde_hip_cotangent.h"):
        assert not declared & find(open(os.path.join(inc, other)).read()), other
    protos = CABI._header_prototypes(body)
    assert set(protos) == declared
    assert CABI._check_against_header(_lib.GRID_EXT_SIGNATURES, protos) == []
    swap = lambda tu: tu.replace('#include "trajsde_hip.h"', '#include "trajsde_hip_grid_cotangent.h"')
    r = CABI._compile_tu(swap(CABI._prototype_tu(_lib.GRID_EXT_SIGNATURES, protos)), tmp_path, H.ROOT, "gridcot")
    assert r.returncode == 0, r.stdout[-3000:]
    bad = dict(_lib.GRID_EXT_SIGNATURES)                        # the check has teeth: one argument fewer is caught both ways
    res, args = bad["trajsde_mlp_decoder_cotangent_backward"]
    bad["trajsde_mlp_decoder_cotangent_backward"] = (res, args[:-1])
    assert CABI._check_against_header(bad, protos)
    assert CABI._compile_tu(swap(CABI._prototype_tu(bad, protos)), tmp_path, H.ROOT, "gridcot_bad").returncode != 0
    lib = _lib.lib()
    for name in declared:
        assert hasattr(lib, name), name


def test_routes_and_reached_parameters():
    l2, nll = _model(["L2"]), _model(["LaplaceNLLLoss"])
    custom, custom_nll = _model(CUSTOM), _model(["SoftTargetCrossEntropyLoss", "LaplaceNLLLoss"])
    assert not l2._cotangent_route() and not nll._cotangent_route() and custom._cotangent_route() and custom_nll._cotangent_route()
    for refused in (["L2", "LaplaceNLLLoss"], ["L2", "LaplaceNLLLoss", "SoftTargetCrossEntropyLoss"], ["L2", "DiffBCE"],
                    ["L2", "DiffBCE", "SoftTargetCrossEntropyLoss"], ["SoftTargetCrossEntropyLoss"], ["DiffBCE"]):
        assert not _model(refused)._cotangent_route(), refused
    name_of = lambda m: [n for n, p in m.named_parameters() if any(p is q for q in m.params_with_gradient())]
    got_l2, got_nll, got_c = name_of(l2), name_of(nll), name_of(custom)
    # the fused sets: what they were
    assert not any(n.startswith(("decoder.pi.", "decoder.scale.")) for n in got_l2) and any(n.startswith("decoder.loc.") for n in got_l2)
    assert set(got_nll) == set(got_l2) | {"decoder." + n for n in SCALE}
    # the custom set: every pi.* and scale.* name on top, in named_parameters() order
    assert set(got_c) == set(got_l2) | {"decoder." + n for n in PI + SCALE}
    assert got_c == [n for n, _ in custom.named_parameters() if n in set(got_c)]
    assert name_of(custom_nll) == got_c


@pytest.mark.parametrize("modules", [["L2", "LaplaceNLLLoss", "SoftTargetCrossEntropyLoss"], ["L2", "DiffBCE", "SoftTargetCrossEntropyLoss"],
                                     ["SoftTargetCrossEntropyLoss"]])
def test_training_step_still_refuses_sets_without_exactly_one_regression_loss(modules):
    from trajsde_amd.synth import synth
    model = _model(modules)
    model.ts_drop = 0.3
    batch = synth(S=2, n=6, L=4, F=12, box=70.0, seed=5, mixed_source=True)
    x0, pad0 = batch.x.clone(), batch.padding_mask.clone()
    with pytest.raises(NotImplementedError, match="ONE regression loss"):
        model.training_step(batch, 0)
    assert torch.equal(batch.x, x0) and torch.equal(batch.padding_mask, pad0)


def test_training_step_on_cpu_under_a_custom_set_is_refused_before_the_batch_is_touched():
    from trajsde_amd import _lib
    from trajsde_amd.synth import synth
    model = _model(CUSTOM)
    model.ts_drop = 0.3                                        # (would mask history steps of the batch in place)
    batch = synth(S=2, n=6, L=4, F=12, box=70.0, seed=5, mixed_source=True)
    x0, pad0, y0 = batch.x.clone(), batch.padding_mask.clone(), batch.y.clone()
    with pytest.raises(_lib.TrajsdeError, match="must live on the GPU"):
        model.training_step(batch, 0)                          # CPU tensors: any kernel launch would fail differently
    assert torch.equal(batch.x, x0) and torch.equal(batch.padding_mask, pad0) and torch.equal(batch.y, y0)
    assert "rotate_mat" not in batch.as_dict() or batch.as_dict()["rotate_mat"] is None
    plain = _model(CUSTOM, uncertain=False)
    with pytest.raises(NotImplementedError, match="uncertain: False"):
        plain.training_step(batch, 0)
    assert torch.equal(batch.x, x0) and torch.equal(batch.padding_mask, pad0) and torch.equal(batch.y, y0)
    with pytest.raises(_lib.TrajsdeError, match="uncertain: False"):
        plain.decoder._rt.mlp_decoder_cotangent_backward({}, torch.zeros(5, 64), torch.zeros(3, 5, 64), {}, None, None)
