"""Global-norm gradient clipping in front of the flat AdamW step (include/trajsde_hip_clip.h, driver.FlatAdamW(max_grad_norm=...)), the
parts that need no GPU: the extension header against `_lib.CLIP_EXT_SIGNATURES`, the exported symbols, the size query and the
refusals of the host side, the coefficient formula against torch.nn.utils.clip_grad_norm_, the torch routes of the training handles
on CPU parameters, the command-line flag and the meaning of `gradient_clip_val`."""
import math
import os
import re

import numpy as np
import pytest
import torch

import helpers as H

NAMES = {"trajsde_grad_norm_ws_bytes", "trajsde_grad_norm_clip", "trajsde_adamw_step_clipped"}


def host_norm_and_coef(values, max_norm):
    """the host twin of k_grad_norm_finish (csrc/clip.hip): the float64 sum of exact squares, then torch's fp32 operations --
    total_norm + 1e-6, `max_norm / t` = t.reciprocal() * max_norm (torch/_tensor.py __rdiv__), clamp(max=1.0), which keeps a NaN"""
    total = math.fsum(float(v) * float(v) for v in values)
    with np.errstate(all="ignore"):
        norm = np.float32(math.sqrt(total)) if math.isfinite(total) else np.float32(total)
        c = (np.float32(1.0) / (norm + np.float32(1e-6))) * np.float32(max_norm)
    return norm, (np.float32(1.0) if c > np.float32(1.0) else c)


def test_clip_header_and_its_signature_table_agree(tmp_path):
    """include/trajsde_hip_clip.h against `_lib.CLIP_EXT_SIGNATURES` by the rules tests/test_cotangent_cpu.py applies to its header"""
    import test_cabi_cpu as CABI
    from trajsde_amd import _lib
    text = open(os.path.join(H.ROOT, "include", "trajsde_hip_clip.h")).read()
    main = open(os.path.join(H.ROOT, "include", "trajsde_hip.h")).read()
    body = text.replace('#include "trajsde_hip.h"', "")
    declared = set(re.findall(r"\b(trajsde_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", " ", body, flags=re.S)))
    assert declared == set(_lib.CLIP_EXT_SIGNATURES) == NAMES
    for other in (_lib.SIGNATURES, _lib.EXT_SIGNATURES, _lib.GRID_EXT_SIGNATURES):
        assert not set(_lib.CLIP_EXT_SIGNATURES) & set(other)
    assert not declared & set(re.findall(r"\b(trajsde_[a-z_0-9]+)\s*\(", main))
    protos = CABI._header_prototypes(body)
    assert set(protos) == declared
    assert CABI._check_against_header(_lib.CLIP_EXT_SIGNATURES, protos) == []
    tu = CABI._prototype_tu(_lib.CLIP_EXT_SIGNATURES, protos).replace('#include "trajsde_hip.h"', '#include "trajsde_hip_clip.h"')
    r = CABI._compile_tu(tu, tmp_path, H.ROOT, "clip")
    assert r.returncode == 0, r.stdout[-3000:]
    for name in ("trajsde_grad_norm_clip", "trajsde_adamw_step_clipped"):      # the check has teeth: one argument fewer is caught both ways
        bad = dict(_lib.CLIP_EXT_SIGNATURES)
        res, args = bad[name]
        bad[name] = (res, args[:-1])
        assert CABI._check_against_header(bad, protos)
        assert CABI._compile_tu(CABI._prototype_tu(bad, protos).replace('"trajsde_hip.h"', '"trajsde_hip_clip.h"'), tmp_path, H.ROOT,
                                "clip_bad").returncode != 0
    assert _lib.ABI_VERSION == 10 and _lib.lib().trajsde_abi_version() == 10   # an extension header: the ABI version did not move


def test_the_three_symbols_are_exported_by_the_built_libraries():
    from trajsde_amd import _lib
    lib = _lib.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.CLIP_EXT_SIGNATURES[name][1]


def test_workspace_query_is_eight_bytes_per_workgroup_of_the_documented_geometry():
    """ties `_lib.CLIP_WG_FLOATS` / `_lib.CLIP_MAX_WGS` (what the GPU tests pick their sizes from) to the library"""
    from trajsde_amd import _lib
    q = _lib.lib().trajsde_grad_norm_ws_bytes
    W, G = _lib.CLIP_WG_FLOATS, _lib.CLIP_MAX_WGS
    assert (W, G) == (2048, 512)
    assert q(1) == q(W - 1) == q(W) == 8 and q(W + 1) == 16
    assert q(W * G - 1) == q(W * G) == q(W * G + 1) == q(1 << 40) == 8 * G and q(W * (G - 1)) == 8 * (G - 1)
    assert q(0) < 0 and q(-5) < 0
    assert b"grad_norm_clip" in _lib.lib().trajsde_last_error()


def test_host_side_refuses_bad_arguments_before_any_launch():
    """n == 0, max_norm <= 0 or NaN, null pointers, a misaligned or short workspace: refused by the host side, which touches no pointer"""
    from trajsde_amd import _lib
    L = _lib.lib()
    p = 1 << 20                                       # never dereferenced: every call below is refused on the host
    assert L.trajsde_grad_norm_clip(p, 0, 1.0, p, 4096, p, None) == -1
    for bad in (0.0, -1.0, float("nan")):
        assert L.trajsde_grad_norm_clip(p, 100, bad, p, 4096, p, None) == -1
        assert b"max_norm" in L.trajsde_last_error()
    assert L.trajsde_grad_norm_clip(None, 100, 1.0, p, 4096, p, None) == -1
    assert L.trajsde_grad_norm_clip(p, 100, 1.0, None, 4096, p, None) == -1
    assert L.trajsde_grad_norm_clip(p, 100, 1.0, p, 4096, None, None) == -1
    assert L.trajsde_grad_norm_clip(p, 100, 1.0, p + 4, 4096, p, None) == -1
    assert L.trajsde_grad_norm_clip(p, 100, 1.0, p, 7, p, None) == -3
    assert L.trajsde_grad_norm_clip(p, 5000, 1.0, p, 16, p, None) == -3
    a = (p, p, p, p, 10, 0.99, 0.1, 0.999, 0.001, 0.5, 1, 1e-8, -1e-3)
    assert L.trajsde_adamw_step_clipped(*a, None, None) == -1
    assert L.trajsde_adamw_step_clipped(None, *a[1:], p, None) == -1
    assert L.trajsde_adamw_step_clipped(*a[:4], -1, *a[5:], p, None) == -1
    assert L.trajsde_adamw_step_clipped(*a[:9], 0.0, *a[10:], p, None) == -1
    assert L.trajsde_adamw_step_clipped(*a[:4], 0, *a[5:], p, None) == 0          # nothing to do, nothing launched


@pytest.mark.parametrize("values", [[3, 4], [1, 2, 2], [2, 3, 6], [0, 0, 0], [12, 15, 16], [1], [8, 9, 12, 0, 0]])
@pytest.mark.parametrize("max_norm", [0.3, 1.0, 4.0, 7.0, 100.0])
def test_host_twin_of_the_coefficient_is_torchs_scaling(values, max_norm):
    """integer gradients whose norm is an integer (5, 3, 7, 0, 25, 1, 17), so torch's fp32 norm is exact: the twin's norm is torch's
    total_norm and g * coef is what clip_grad_norm_ leaves in `.grad`, bit for bit"""
    from trajsde_amd import driver
    g = torch.tensor(values, dtype=torch.float32)
    norm, coef = host_norm_and_coef(values, max_norm)
    q = torch.nn.Parameter(torch.zeros_like(g))
    q.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_([q], max_norm)
    assert float(total) == float(norm)
    assert np.array_equal(q.grad.numpy(), g.numpy() * coef)
    p = torch.nn.Parameter(torch.zeros_like(g))
    p.grad = g.clone()
    pair = driver.torch_clip_grad_norm([p], max_norm)
    assert pair.dtype == torch.float32 and pair.shape == (2,)
    assert float(pair[0]) == float(norm) and float(pair[1]) == float(coef)


def test_host_twin_on_non_finite_norms_is_torchs():
    for values, want in (([1.0, float("inf")], 0.0), ([1.0, float("nan")], float("nan"))):
        norm, coef = host_norm_and_coef(values, 2.0)
        p = torch.nn.Parameter(torch.zeros(2))
        p.grad = torch.tensor(values)
        total = torch.nn.utils.clip_grad_norm_([p], 2.0)
        t = torch.clamp(2.0 / (total + 1e-6), max=1.0)
        assert (math.isnan(float(coef)) and math.isnan(float(t)) and math.isnan(want)) or float(coef) == float(t) == want


class _Net(torch.nn.Module):
    """what PlainTraining asks of a model: configure_optimizers, params_with_gradient, named_parameters"""

    def __init__(self, clip):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.a = torch.nn.Parameter(torch.randn(7, 5, generator=g))
        self.b = torch.nn.Parameter(torch.randn(11, generator=g))
        self.frozen = torch.nn.Parameter(torch.randn(3, generator=g), requires_grad=False)
        self.gradient_clip_val = clip

    def params_with_gradient(self):
        return [self.a, self.b]

    def configure_optimizers(self):
        opt = torch.optim.AdamW(self.parameters(), lr=1e-2, weight_decay=1e-2)
        return [opt], [torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)]


def _grads(step):
    g = torch.Generator().manual_seed(100 + step)
    return torch.randn(7, 5, generator=g) * 10.0 ** (step - 1), torch.randn(11, generator=g) * 10.0 ** (step - 1)


def _twin_steps(clip, steps=3):
    """torch's clip_grad_norm_ then AdamW.step(), spelled out"""
    net = _Net(None)
    (opt,), _ = net.configure_optimizers()
    norms = []
    for s in range(steps):
        net.a.grad, net.b.grad = _grads(s)
        if clip:
            norms.append(float(torch.nn.utils.clip_grad_norm_([net.a, net.b], clip)))
        opt.step()
    return net, norms


@pytest.mark.parametrize("clip", [0.5, 1e6])
def test_plain_training_clips_with_torch_before_its_step(clip):
    from trajsde_amd import driver
    net = _Net(clip)
    pt = driver.PlainTraining(net)
    assert pt.max_grad_norm == clip and pt.last_grad_norm is None
    twin, norms = _twin_steps(clip)
    for s in range(3):
        pt.zero()
        ga, gb = _grads(s)
        net.a.grad.copy_(ga)
        net.b.grad.copy_(gb)
        pt.step()
        assert float(pt.last_grad_norm[0]) == norms[s]
        assert float(pt.last_grad_norm[1]) == float(host_norm_and_coef([norms[s]], clip)[1])
    assert torch.equal(net.a.detach(), twin.a.detach()) and torch.equal(net.b.detach(), twin.b.detach())
    assert torch.equal(net.a.grad, twin.a.grad) and torch.equal(net.b.grad, twin.b.grad)
    assert (float(pt.last_grad_norm[1]) < 1.0) == (clip == 0.5)


@pytest.mark.parametrize("off", [None, 0, 0.0])
def test_gradient_clip_val_of_none_and_of_zero_are_both_off(off, monkeypatch):
    from trajsde_amd import driver
    assert driver.clip_value_of(_Net(off)) is None
    assert driver.clip_value_of(object()) is None                   # a model that never heard of the attribute
    assert driver.clip_value_of(_Net(2)) == 2.0
    with pytest.raises(ValueError):
        driver.clip_value_of(_Net(-1.0))
    calls = []
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", lambda *a, **k: calls.append(a))
    net = _Net(off)
    pt = driver.PlainTraining(net)
    twin, _ = _twin_steps(None)
    for s in range(3):
        pt.zero()
        ga, gb = _grads(s)
        net.a.grad.copy_(ga)
        net.b.grad.copy_(gb)
        pt.step()
    assert calls == [] and pt.max_grad_norm is None and pt.last_grad_norm is None
    assert torch.equal(net.a.detach(), twin.a.detach()) and torch.equal(net.b.detach(), twin.b.detach())


@pytest.mark.parametrize("form", ["foreach", "single"])
def test_flat_adamw_fallback_on_cpu_parameters_is_torchs_clip_then_torchs_step(form):
    """CPU tensors: the launch does not apply, so FlatAdamW(max_grad_norm=...) is clip_grad_norm_ over the group's parameters and
    torch's step; the clip value is in neither state_dict() nor param_groups"""
    from trajsde_amd import driver
    twin, norms = _twin_steps(0.5)
    net = _Net(None)
    opt = driver.FlatAdamW([net.a, net.b], lr=1e-2, weight_decay=1e-2, form=form, max_grad_norm=0.5)
    assert opt.last_grad_norm is None
    for s in range(3):
        net.a.grad, net.b.grad = _grads(s)
        opt.step()
        assert float(opt.last_grad_norm[0]) == norms[s]
    assert torch.equal(net.a.detach(), twin.a.detach()) and torch.equal(net.b.detach(), twin.b.detach())
    assert torch.equal(net.a.grad, twin.a.grad) and torch.equal(net.b.grad, twin.b.grad)
    plain = driver.FlatAdamW([torch.nn.Parameter(torch.zeros(3))], lr=1e-2, weight_decay=1e-2, form=form)
    assert plain.max_grad_norm is None
    assert opt.state_dict()["param_groups"][0].keys() == plain.state_dict()["param_groups"][0].keys()
    assert not any("norm" in k for k in opt.state_dict()["param_groups"][0])
    assert set(opt.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            driver.FlatAdamW([torch.nn.Parameter(torch.zeros(3))], max_grad_norm=bad)


def test_gradient_clip_val_flag_parses():
    from trajsde_amd import driver
    ap = driver.arg_parser()
    assert ap.parse_args(["-c", "x.yml", "--train"]).gradient_clip_val is None
    assert ap.parse_args(["-c", "x.yml", "--train", "--gradient-clip-val", "0.5"]).gradient_clip_val == 0.5
    assert ap.parse_args(["-c", "x.yml", "--train", "--gradient_clip_val", "2"]).gradient_clip_val == 2.0     # the reference's spelling
    with pytest.raises(SystemExit):
        ap.parse_args(["-c", "x.yml", "--gradient-clip-val", "much"])
