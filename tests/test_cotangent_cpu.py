"""The decoder backward from caller-supplied cotangents (trajsde_decoder_cotangent_backward), the parts that need no GPU: the
parameter table of TRAJSDE_STAGE_DECODER_COT_BWD, the workspace query, losses.SoftTargetCrossEntropyLoss against a hand-written
float64 formula, the parameters the cotangent route reaches and the loss routing of `training_step`."""
import math

import pytest
import torch

import helpers as H

PI = ["pi.0.weight", "pi.0.bias", "pi.1.weight", "pi.1.bias", "pi.3.weight", "pi.3.bias"]
CUSTOM = ["L2", "DiffBCE", "SoftTargetCrossEntropyLoss"]


def _names(lib, stage):
    return [lib.trajsde_param_name(stage, i, 0, 0).decode() for i in range(lib.trajsde_param_count(stage, 0, 0))]


def _model(modules, weights=None, K=3, T=5, method=None):
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    cfg = H.our_cfg(K, T, 0.5)
    cfg["losses"] = ["trajsde_amd/losses.py"] * len(modules)
    cfg["losses_module"] = list(modules)
    cfg["loss_weights"] = list(weights) if weights is not None else [1.0] * len(modules)
    cfg["loss_args"] = [{} for _ in modules]
    if method is not None:
        cfg["decoder"]["kwargs"]["method"] = method
    return PredictionModelSDENet(**cfg, init_seed=0).eval(), cfg


def test_stage_15_table_is_the_nll_table_followed_by_the_pi_head():
    from trajsde_amd import _lib
    lib = _lib.lib()
    assert _lib.STAGE_DECODER_COT_BWD == 15
    with open(H.ROOT + "/include/trajsde_hip.h") as f:
        assert "TRAJSDE_STAGE_DECODER_COT_BWD = 15" in f.read()
    assert lib.trajsde_abi_version() == 10
    nll, cot = _names(lib, _lib.STAGE_DECODER_NLL_BWD), _names(lib, _lib.STAGE_DECODER_COT_BWD)
    assert cot == nll + PI and len(set(cot)) == len(cot)
    assert lib.trajsde_blob_floats(_lib.STAGE_DECODER_COT_BWD, 0, 0) > lib.trajsde_blob_floats(_lib.STAGE_DECODER_NLL_BWD, 0, 0)
    # its name set: every decoder parameter the forward reads that requires a gradient
    model, _ = _model(CUSTOM)
    fwd = set(_names(lib, _lib.STAGE_DECODER))
    want = {n for n, p in model.decoder.named_parameters() if p.requires_grad and n in fwd}
    assert set(cot) == want
    assert any(n.startswith("pi.") for n in want) and any(n.startswith("scale.") for n in want)


def test_workspace_query_is_positive_and_monotone():
    from trajsde_amd import _lib
    q = _lib.lib().trajsde_decoder_cotangent_backward_ws_bytes
    base = (17, 3, 5, 6)
    b0 = q(*base)
    assert b0 > 0
    for arg in range(4):
        prev = b0
        for step in (1, 2, 15, 16, 17, 100):
            args = list(base)
            args[arg] += step
            cur = q(*args)
            assert cur >= prev > 0, (arg, step, cur, prev)
            prev = cur
    # one mode: the welded entry point's workspace fits
    assert q(64, 1, 20, 20) >= _lib.lib().trajsde_decoder_nll_backward_ws_bytes(64, 1, 20, 20)
    assert q(0, 3, 5, 6) < 0 and q(17, 0, 5, 6) < 0                      # refused, with a message
    assert b"decoder_cotangent_backward" in _lib.lib().trajsde_last_error()


def test_soft_target_cross_entropy_matches_hand_written_formula():
    """3 actors, K = 2, T = 3: actor 0 fully valid, actor 1 with a masked step, actor 2 fully masked (no term)"""
    from trajsde_amd.losses import SoftTargetCrossEntropyLoss
    g = torch.Generator().manual_seed(4)
    K, N, T = 2, 3, 3
    loc = torch.randn(K, N, T, 4, generator=g, dtype=torch.float64)
    y = torch.randn(N, T, 2, generator=g, dtype=torch.float64)
    pi = torch.randn(N, K, generator=g, dtype=torch.float64, requires_grad=True)
    mask = torch.tensor([[1, 1, 1], [1, 0, 1], [0, 0, 0]], dtype=torch.bool)
    got = SoftTargetCrossEntropyLoss()({"y": y}, {"loc": loc, "pi": pi, "reg_mask": mask})
    total, dpi = 0.0, torch.zeros(N, K, dtype=torch.float64)
    for n in range(2):                                                    # actor 2 has no valid step
        steps = [t for t in range(T) if mask[n, t]]
        d = [sum(math.hypot(float(loc[k, n, t, 0] - y[n, t, 0]), float(loc[k, n, t, 1] - y[n, t, 1])) for t in steps) / len(steps)
             for k in range(K)]
        e = [math.exp(-v) for v in d]
        soft = [v / sum(e) for v in e]
        lse = math.log(sum(math.exp(float(pi[n, k])) for k in range(K)))
        total += -sum(soft[k] * (float(pi[n, k]) - lse) for k in range(K))
        for k in range(K):                                                # d CE / d pi = softmax(pi) - soft
            dpi[n, k] = (math.exp(float(pi[n, k]) - lse) - soft[k]) / 2
    assert abs(float(got) - total / 2) <= 1e-12
    got.backward()
    assert float((pi.grad - dpi).abs().max()) <= 1e-12 and float(pi.grad[2].abs().max()) == 0.0
    loc.requires_grad_(True)                                              # the soft target is detached: no gradient into loc
    v = SoftTargetCrossEntropyLoss()({"y": y}, {"loc": loc, "pi": pi.detach().requires_grad_(True), "reg_mask": mask})
    assert torch.autograd.grad(v, loc, allow_unused=True)[0] is None
    none = SoftTargetCrossEntropyLoss()({"y": y}, {"loc": loc, "pi": pi, "reg_mask": torch.zeros(N, T, dtype=torch.bool)})
    assert float(none) == 0.0
    with pytest.raises(ValueError):
        SoftTargetCrossEntropyLoss(reduction="sum")


def test_routes_and_reached_parameters():
    welded, _ = _model(["L2", "DiffBCE"])
    custom, _ = _model(CUSTOM)
    both, _ = _model(["L2", "LaplaceNLLLoss", "DiffBCE"])
    assert not welded._cotangent_route() and custom._cotangent_route() and both._cotangent_route()
    assert not _model(["LaplaceNLLLoss", "DiffBCE"])[0]._cotangent_route()
    name_of = lambda m: [n for n, p in m.named_parameters() if any(p is q for q in m.params_with_gradient())]
    got_w, got_c = name_of(welded), name_of(custom)
    assert not any(n.startswith(("decoder.pi.", "decoder.scale.")) for n in got_w)
    scale = ["decoder.scale" + n[2:] for n in PI]
    assert set(got_c) == set(got_w) | {"decoder." + n for n in PI} | set(scale)
    assert name_of(both) == got_c


def test_training_step_on_cpu_under_a_custom_set_is_refused_before_the_batch_is_touched():
    from trajsde_amd import _lib
    from trajsde_amd.synth import synth
    model, _ = _model(CUSTOM)
    batch = synth(S=2, n=6, L=4, F=5, box=70.0, seed=5, mixed_source=True)
    x0, pad0, y0 = batch.x.clone(), batch.padding_mask.clone(), batch.y.clone()
    with pytest.raises(_lib.TrajsdeError, match="must live on the GPU"):
        model.training_step(batch, 0)                          # CPU tensors: any kernel launch would fail differently
    assert torch.equal(batch.x, x0) and torch.equal(batch.padding_mask, pad0) and torch.equal(batch.y, y0)
    assert "rotate_mat" not in batch.as_dict() or batch.as_dict()["rotate_mat"] is None


def test_milstein_under_a_custom_set_is_refused():
    from trajsde_amd.synth import synth
    model, _ = _model(CUSTOM, K=3, T=20, method="milstein")
    batch = synth(S=1, n=6, L=4, F=20, box=60.0, seed=2)
    with pytest.raises(NotImplementedError, match="Euler"):
        model.training_step(batch, 0)
    with pytest.raises(NotImplementedError, match="milstein"):
        model.decoder._rt.decoder_cotangent_backward(batch, None, None, {}, None, None, None)


def test_extension_header_and_its_signature_table_agree(tmp_path):
    """include/trajsde_hip_cotangent.h against `_lib.EXT_SIGNATURES`, by the rules tests/test_cabi_cpu.py applies to trajsde_hip.h and
    `_lib.SIGNATURES` (its helpers, imported): the same names; argument counts, scalar types, pointer-ness and pointed-to structs,
    compared in Python and by the C compiler; the library exports the symbols; the two tables and the two headers do not overlap"""
    import os
    import re

    import test_cabi_cpu as CABI
    from trajsde_amd import _lib
    text = open(os.path.join(H.ROOT, "include", "trajsde_hip_cotangent.h")).read()
    main = open(os.path.join(H.ROOT, "include", "trajsde_hip.h")).read()
    body = text.replace('#include "trajsde_hip.h"', "")
    declared = set(re.findall(r"\b(trajsde_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", " ", body, flags=re.S)))
    assert declared == set(_lib.EXT_SIGNATURES) == {"trajsde_decoder_cotangent_backward", "trajsde_decoder_cotangent_backward_ws_bytes"}
    assert not set(_lib.EXT_SIGNATURES) & set(_lib.SIGNATURES)
    assert not declared & set(re.findall(r"\b(trajsde_[a-z_0-9]+)\s*\(", main))
    protos = CABI._header_prototypes(body)
    assert set(protos) == declared
    assert CABI._check_against_header(_lib.EXT_SIGNATURES, protos) == []
    tu = CABI._prototype_tu(_lib.EXT_SIGNATURES, protos).replace('#include "trajsde_hip.h"', '#include "trajsde_hip_cotangent.h"')
    r = CABI._compile_tu(tu, tmp_path, H.ROOT, "cot")
    assert r.returncode == 0, r.stdout[-3000:]
    bad = dict(_lib.EXT_SIGNATURES)                             # the check has teeth: one argument fewer is caught both ways
    res, args = bad["trajsde_decoder_cotangent_backward"]
    bad["trajsde_decoder_cotangent_backward"] = (res, args[:-1])
    assert CABI._check_against_header(bad, protos)
    assert CABI._compile_tu(CABI._prototype_tu(bad, protos).replace('"trajsde_hip.h"', '"trajsde_hip_cotangent.h"'), tmp_path, H.ROOT,
                            "cot_bad").returncode != 0
    lib = _lib.lib()
    for name in declared:
        assert hasattr(lib, name), name
