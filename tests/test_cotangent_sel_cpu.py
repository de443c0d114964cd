"""The cotangent decoder backward over each actor's supported mode (trajsde_decoder_cotangent_backward_sel), the parts that need no GPU:
its extension header against its `_lib` table, the exported symbols, the workspace query against the dense route's, and the
`cotangent_support` switch of the model and the runtime."""
import pytest

import helpers as H

CUSTOM = ["L2", "DiffBCE", "SoftTargetCrossEntropyLoss"]
NAMES = {"trajsde_decoder_cotangent_backward_sel", "trajsde_decoder_cotangent_backward_sel_ws_bytes"}


def _model(modules, support=None, K=3, T=5, method=None):
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    cfg = H.our_cfg(K, T, 0.5)
    cfg["losses"] = ["trajsde_amd/losses.py"] * len(modules)
    cfg["losses_module"] = list(modules)
    cfg["loss_weights"] = [1.0] * len(modules)
    cfg["loss_args"] = [{} for _ in modules]
    if support is not None:
        cfg["model_specific"]["kwargs"]["cotangent_support"] = support
    if method is not None:
        cfg["decoder"]["kwargs"]["method"] = method
    return PredictionModelSDENet(**cfg, init_seed=0).eval()


def test_extension_header_and_its_signature_table_agree(tmp_path):
    """include/trajsde_hip_cotangent_sel.h against `_lib.COT_SEL_EXT_SIGNATURES`, by the rules tests/test_cotangent_cpu.py applies to
    trajsde_hip_cotangent.h: the same names; argument counts, scalar types, pointer-ness and pointed-to structs, compared in Python and by
    the C compiler; the library exports the symbols; the table overlaps no other table, the header no other header"""
    import os
    import re

    import test_cabi_cpu as CABI
    from trajsde_amd import _lib
    inc = os.path.join(H.ROOT, "include")
    text = open(os.path.join(inc, "trajsde_hip_cotangent_sel.h")).read()
    body = text.replace('#include "trajsde_hip_cotangent.h"', "")
    declared = set(re.findall(r"\b(trajsde_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", " ", body, flags=re.S)))
    assert declared == set(_lib.COT_SEL_EXT_SIGNATURES) == NAMES
    for other in (_lib.SIGNATURES, _lib.EXT_SIGNATURES, _lib.GRID_EXT_SIGNATURES, _lib.CLIP_EXT_SIGNATURES):
        assert not set(_lib.COT_SEL_EXT_SIGNATURES) & set(other)
    for h in ("trajsde_hip.h", "trajsde_hip_cotangent.h", "trajsde_hip_grid_cotangent.h", "trajsde_hip_clip.h"):
        assert not declared & set(re.findall(r"\b(trajsde_[a-z_0-9]+)\s*\(", open(os.path.join(inc, h)).read())), h
    protos = CABI._header_prototypes(body)
    assert set(protos) == declared
    assert CABI._check_against_header(_lib.COT_SEL_EXT_SIGNATURES, protos) == []
    tu = CABI._prototype_tu(_lib.COT_SEL_EXT_SIGNATURES, protos).replace('"trajsde_hip.h"', '"trajsde_hip_cotangent_sel.h"')
    r = CABI._compile_tu(tu, tmp_path, H.ROOT, "cot_sel")
    assert r.returncode == 0, r.stdout[-3000:]
    bad = dict(_lib.COT_SEL_EXT_SIGNATURES)                     # the check has teeth: without the status pointer it is caught both ways
    res, args = bad["trajsde_decoder_cotangent_backward_sel"]
    bad["trajsde_decoder_cotangent_backward_sel"] = (res, args[:-2] + args[-1:])
    assert CABI._check_against_header(bad, protos)
    assert CABI._compile_tu(CABI._prototype_tu(bad, protos).replace('"trajsde_hip.h"', '"trajsde_hip_cotangent_sel.h"'), tmp_path, H.ROOT,
                            "cot_sel_bad").returncode != 0
    # the dense entry point's arguments plus one pointer in front of the stream
    dense = _lib.EXT_SIGNATURES["trajsde_decoder_cotangent_backward"][1]
    assert _lib.COT_SEL_EXT_SIGNATURES["trajsde_decoder_cotangent_backward_sel"][1] == dense[:-1] + [_lib.P] + dense[-1:]
    lib = _lib.lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.trajsde_abi_version() == 10


def test_workspace_query_is_positive_monotone_and_below_the_dense_one():
    from trajsde_amd import _lib
    L = _lib.lib()
    q, dense, nll = (L.trajsde_decoder_cotangent_backward_sel_ws_bytes, L.trajsde_decoder_cotangent_backward_ws_bytes,
                     L.trajsde_decoder_nll_backward_ws_bytes)
    base = (17, 3, 5, 6)
    b0 = q(*base)
    assert b0 > 0
    for arg in (0, 2, 3):                                                 # N, T, n_euler
        prev = b0
        for step in (1, 2, 15, 16, 17, 100):
            args = list(base)
            args[arg] += step
            cur = q(*args)
            assert cur >= prev > 0, (arg, step, cur, prev)
            prev = cur
    for N, K0, T, n_euler in ((17, 3, 5, 6), (8192, 6, 20, 20), (6144, 10, 60, 61)):
        for K in range(2, 33):
            s, d = q(N, K, T, n_euler), dense(N, K, T, n_euler)
            assert 0 < s < d, (N, K, T, n_euler, s, d)
            grow_s, grow_d = q(N, 2 * K, T, n_euler) - s, dense(N, 2 * K, T, n_euler) - d
            assert 0 <= grow_s < grow_d, (N, K, grow_s, grow_d)
            # the SDE tape does not scale with K: what K adds is the pi head's delta rows, 256 bytes a path (+ alignment)
            assert grow_s <= K * N * 256 + 512
        # the welded carve over N rows, the pi head's K * N + N rows and two count words per 16 actors on top of it
        assert 0 < q(N, K0, T, n_euler) - nll(N, K0, T, n_euler) <= (K0 + 1) * N * 256 + N + 2048
    assert q(0, 3, 5, 6) < 0 and q(17, 0, 5, 6) < 0                      # refused, with a message
    assert b"decoder_cotangent_backward_sel" in L.trajsde_last_error()


def test_the_model_kwarg_and_its_default():
    assert _model(CUSTOM).cotangent_support == "all"
    assert _model(["L2", "DiffBCE"]).cotangent_support == "all"
    winner = _model(CUSTOM, support="winner")
    assert winner.cotangent_support == "winner" and winner._cotangent_route()
    winner.check_cotangent_support()                                      # no step yet: nothing to check, nothing raised
    # the switch changes neither the route nor the parameters it reaches
    name_of = lambda m: [n for n, p in m.named_parameters() if any(p is q for q in m.params_with_gradient())]
    assert name_of(winner) == name_of(_model(CUSTOM))
    assert not _model(["L2", "DiffBCE"], support="winner")._cotangent_route()


def test_a_bad_value_raises_value_error():
    from trajsde_amd.synth import synth
    batch = synth(S=1, n=6, L=4, F=5, box=60.0, seed=2)
    model = _model(CUSTOM)
    with pytest.raises(ValueError, match="support"):
        model.decoder._rt.decoder_cotangent_backward(batch, None, None, {}, None, None, None, support="best")
    x0, y0 = batch.x.clone(), batch.y.clone()
    import torch
    with pytest.raises(ValueError, match="cotangent_support"):
        _model(CUSTOM, support="best").training_step(batch, 0)
    assert torch.equal(batch.x, x0) and torch.equal(batch.y, y0)


def test_milstein_under_a_custom_set_is_refused_with_winner_too():
    from trajsde_amd.synth import synth
    model = _model(CUSTOM, support="winner", K=3, T=20, method="milstein")
    batch = synth(S=1, n=6, L=4, F=20, box=60.0, seed=2)
    with pytest.raises(NotImplementedError, match="Euler"):
        model.training_step(batch, 0)
    with pytest.raises(NotImplementedError, match="milstein"):
        model.decoder._rt.decoder_cotangent_backward(batch, None, None, {}, None, None, None, support="winner")


def test_the_driver_option():
    from trajsde_amd import driver
    ap = driver.arg_parser()
    assert ap.parse_args(["-c", "x.yml"]).cotangent_support is None
    assert ap.parse_args(["-c", "x.yml", "--cotangent-support", "winner"]).cotangent_support == "winner"
    assert ap.parse_args(["-c", "x.yml", "--cotangent_support", "all"]).cotangent_support == "all"
    with pytest.raises(SystemExit):
        ap.parse_args(["-c", "x.yml", "--cotangent-support", "best"])
