"""Global-norm gradient clipping inside the flat AdamW step (-m gpu): trajsde_grad_norm_clip and trajsde_adamw_step_clipped
(include/trajsde_hip_clip.h) against float64 and against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW, and the training loop
with `gradient_clip_val` set.

Sizes (`_lib.CLIP_WG_FLOATS` = W elements a workgroup and pass, `_lib.CLIP_MAX_WGS` = G workgroups): around one wave, one workgroup of
256 threads, one workgroup's share W, one pass of the whole grid W * G, several passes, and the model's own flat size.

Bounds.  Norm: the float64 sum of n exact squares is off by at most n * 2^-53 relative, far below an fp32 ulp, and is rounded once:
within ONE fp32 ulp of grad.double().norm().  Written-back gradient against float64: one ulp of the norm, one of norm + 1e-6, one of
the reciprocal, one of its product with max_norm, half of the product with g: under 8 ulp = 2^-20 relative."""
import functools

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
SMALL = [1, 63, 64, 65, 255, 256, 257]
MAX_NORM = 0.37                       # log-uniform magnitudes over 1e-9 .. 1 have a norm of ~0.155 sqrt(n): n <= 5 is not clipped, the rest is


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _real_flat_size():
    from trajsde_amd import driver
    model, _ = H.build_model(6, 20, 2.0, init_seed=0)
    model.lr, model.weight_decay, model.T_max = 1e-3, 1e-4, 4
    return int(driver.FlatTraining(model.to("cuda:0")).flat_param.numel())


def _sizes():
    from trajsde_amd import _lib
    W, G = _lib.CLIP_WG_FLOATS, _lib.CLIP_MAX_WGS
    return SMALL + [W - 1, W, W + 1, W * G - 1, W * G, W * G + 1, 2 * W * G + 4097]


# (n, pointer offset in floats): every size aligned and offset by one float; the two other misalignments where the paths differ
# ("real" = the model's flat size, resolved on the GPU box)
CASES = [(n, off) for n in _sizes() + ["real"] for off in (0, 1)] + [(n, off) for n in (1, 65, 257, 2049, "real") for off in (2, 3)]


@functools.lru_cache(maxsize=None)
def _gradient(n, scale=1.0):
    """n values with random signs and magnitudes drawn log-uniformly from 1e-9 .. 1 (what the adjoints span), on the host; shared"""
    g = torch.Generator().manual_seed(1000 + n % 9973)
    mag = 10.0 ** (-9.0 * torch.rand(n, generator=g, dtype=torch.float64))
    sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    return (mag * sign * scale).float()


def _offset_view(values, off, dev, pad=float("nan")):
    """`values` at `off` floats past a 512-byte boundary, NaN on both sides: a read outside the view poisons the sum"""
    buf = torch.full((values.numel() + 8,), pad, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + values.numel()]
    view.copy_(values)
    return view


def _norm_clip(grad, max_norm, ws=None):
    from trajsde_amd import _lib
    L = _lib.lib()
    n = grad.numel()
    need = int(L.trajsde_grad_norm_ws_bytes(n))
    assert need > 0
    if ws is None:
        ws = torch.empty(need // 8, dtype=torch.float64, device=grad.device)
    out = torch.full((2,), float("nan"), device=grad.device)
    _lib.check(L.trajsde_grad_norm_clip(grad.data_ptr(), n, max_norm, ws.data_ptr(), ws.numel() * 8, out.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream), "trajsde_grad_norm_clip")
    return out


def _torch_coef(norm32, max_norm):
    """min(max_norm / (norm + 1e-6), 1) evaluated by torch in fp32 on the fp32 norm, on the host"""
    return torch.clamp(max_norm / (norm32 + 1e-6), max=1.0)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


_NORM_SEEN = {}


@pytest.mark.parametrize("n,off", CASES)
def test_norm_is_within_one_ulp_of_float64_and_the_coefficient_is_torchs(n, off, dev):
    n = _real_flat_size() if n == "real" else n
    values = _gradient(n)
    grad = _offset_view(values, off, dev)
    out = _norm_clip(grad, MAX_NORM).cpu()
    want = float(values.to(dev).double().norm())
    got = float(out[0])
    ulp = float(np.spacing(np.float32(want)))
    print(f"n={n} off={off}: norm {got!r} float64 {want!r} diff {abs(got - want) / ulp:.3f} ulp, coef {float(out[1])!r}")
    assert abs(got - want) <= ulp, (n, off, got, want)
    assert torch.equal(_bits(out[1:]), _bits(_torch_coef(out[:1], MAX_NORM))), (n, off, out)
    assert (float(out[1]) == 1.0) == (got + 1e-6 <= MAX_NORM) or abs(got - MAX_NORM) < 1e-5
    # the order of the sum depends on n alone: the same words at every alignment of the pointer
    seen = _NORM_SEEN.setdefault(n, _bits(out).clone())
    assert torch.equal(seen, _bits(out)), (n, off)


def _scalars(lr, wd, beta1, beta2, eps, step, divide):
    bias1, bias2 = 1 - beta1 ** step, 1 - beta2 ** step
    return (1 - lr * wd, 1 - beta1, beta2, 1 - beta2, bias2 ** 0.5 if divide else 1.0 / (bias2 ** 0.5), int(divide), eps, -(lr / bias1))


@pytest.mark.parametrize("divide", [1, 0])
def test_clipped_step_below_above_and_at_zero(divide, dev):
    """norm below max_norm: the coefficient is exactly 1 and parameters, moments AND gradient are the bits trajsde_adamw_step leaves;
    far above: the gradient is scaled down to max_norm; an all-zero gradient: norm 0, coefficient 1"""
    from trajsde_amd import _lib
    L = _lib.lib()
    n = 5003
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(5)
    p0, m0 = torch.randn(n, generator=g).to(dev), (0.1 * torch.randn(n, generator=g)).to(dev)
    v0 = (0.01 * torch.rand(n, generator=g)).to(dev)
    sc = _scalars(3e-3, 1e-2, 0.9, 0.999, 1e-8, 3, divide)
    for name, values, max_norm in (("below", _gradient(n), 1e3), ("above", _gradient(n, 100.0), 0.01), ("zero", torch.zeros(n), 0.5)):
        grad = values.to(dev)
        out = _norm_clip(grad, max_norm)
        a = [t.clone() for t in (p0, grad, m0, v0)]
        b = [t.clone() for t in (p0, grad, m0, v0)]
        _lib.check(L.trajsde_adamw_step_clipped(*(t.data_ptr() for t in a), n, *sc, out.data_ptr() + 4, st), "clipped")
        _lib.check(L.trajsde_adamw_step(*(t.data_ptr() for t in b), n, *sc, st), "plain")
        torch.cuda.synchronize()
        norm, coef = float(out[0]), float(out[1])
        if name == "above":
            assert coef < 1e-3 and abs(float(a[1].double().norm()) / (max_norm * norm / (norm + 1e-6)) - 1) < 1e-5
            assert not torch.equal(a[0], b[0]) and torch.equal(a[1], grad * out[1])
        else:
            assert coef == 1.0 and (norm == 0.0) == (name == "zero")
            for x, y, what in zip(a, b, ("param", "grad", "exp_avg", "exp_avg_sq")):
                assert torch.equal(_bits(x), _bits(y)), (name, what)
            assert torch.equal(_bits(a[1]), _bits(grad))


@pytest.mark.parametrize("form", ["foreach", "single"])
@pytest.mark.parametrize("n,off", [(n, 0) for n in _sizes() + ["real"]] + [(n, 1) for n in (1, 65, 257, 2049)])
def test_clipped_update_is_torchs_clip_then_adamw_bit_for_bit(n, off, form, dev):
    """three steps of FlatAdamW(max_grad_norm=...) -- trajsde_grad_norm_clip + trajsde_adamw_step_clipped -- against torch: grad.mul_(coef)
    with the coefficient read back from the device, then torch.optim.AdamW(foreach=...).step().  Parameters, both moments and the
    written-back gradient bit-equal after every step; the written-back gradient also within 2^-20 relative of the float64 value
    g * min(max_norm / (||g|| + 1e-6), 1), which does not go through torch's or the kernel's fp32 norm.  off = 1: parameter and gradient
    one float past a 16-byte boundary (the kernel's element-wise path)"""
    from trajsde_amd import _lib, driver
    n = _real_flat_size() if n == "real" else n
    L = _lib.lib()
    calls = []
    real = L.trajsde_adamw_step_clipped
    L.trajsde_adamw_step_clipped = lambda *a: (calls.append(1), real(*a))[1]
    try:
        g = torch.Generator().manual_seed(n)
        p0 = torch.randn(n, generator=g)
        pa = torch.nn.Parameter(p0.clone().to(dev))
        pb = torch.nn.Parameter(_offset_view(p0, off, dev, pad=0.0))
        a = torch.optim.AdamW([pa], lr=3e-3, weight_decay=1e-2, foreach=form == "foreach")
        b = driver.FlatAdamW([pb], lr=3e-3, weight_decay=1e-2, form=form, max_grad_norm=MAX_NORM)
        for step in range(3):
            values = _gradient(n, 10.0 ** (step - 1))            # the third step is clipped at every n, the first at the larger ones
            pb.grad = _offset_view(values, off, dev)
            b.step()
            pair = b.last_grad_norm.cpu()
            pa.grad = values.clone().to(dev)
            pa.grad.mul_(float(pair[1]))
            a.step()
            assert torch.equal(_bits(pa.detach()), _bits(pb.detach())), (step, float((pa.detach() - pb.detach()).abs().max()))
            assert torch.equal(_bits(pa.grad), _bits(pb.grad)), step
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(_bits(a.state[pa][key]), _bits(b.state[pb][key])), (step, key)
            g64 = values.to(dev).double()
            want = g64 * min(MAX_NORM / (float(g64.norm()) + 1e-6), 1.0)
            rel = float(((pb.grad.double() - want).abs() / want.abs().clamp_min(1e-300)).max())
            print(f"n={n} off={off} {form} step {step}: coef {float(pair[1])!r}, written-back gradient max rel err {rel:.3e}")
            assert rel <= 2.0 ** -20, (step, rel)
        assert len(calls) == 3 and (n < 63 or float(pair[1]) < 1.0)      # (a handful of elements may all be tiny)
    finally:
        L.trajsde_adamw_step_clipped = real


@pytest.mark.parametrize("n", ["grid+1", "real"])
def test_identical_calls_over_different_garbage_give_identical_words(n, dev):
    from trajsde_amd import _lib
    n = _real_flat_size() if n == "real" else _lib.CLIP_WG_FLOATS * _lib.CLIP_MAX_WGS + 1
    grad = _gradient(n).to(dev)
    words = _lib.CLIP_MAX_WGS + 64                                        # a workspace larger than the query, too
    g = torch.Generator(device=dev).manual_seed(3)
    outs = []
    for fill in ("nan", "random", "random", "zero"):
        ws = torch.zeros(words, dtype=torch.float64, device=dev)
        if fill == "nan":
            ws.view(torch.uint8).fill_(0xFF)
        elif fill == "random":
            ws.view(torch.uint8).random_(0, 256, generator=g)
        outs.append(_bits(_norm_clip(grad, MAX_NORM, ws=ws)).cpu())
    assert all(torch.equal(outs[0], o) for o in outs[1:]), outs


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gradients_behave_as_torchs_clip_and_adamw(bad, dev):
    """error_if_nonfinite=False: an inf entry makes the norm inf and the coefficient 0 (0 * inf = NaN at that entry), a NaN entry makes
    both NaN and with them every element.  Same values, NaN for NaN, as clip_grad_norm_ + AdamW on the same tensors"""
    from trajsde_amd import driver
    n = 3000
    values = _gradient(n).clone()
    values[1234] = bad
    g = torch.Generator().manual_seed(8)
    p0 = torch.randn(n, generator=g)
    pa, pb = torch.nn.Parameter(p0.clone().to(dev)), torch.nn.Parameter(p0.clone().to(dev))
    a = torch.optim.AdamW([pa], lr=3e-3, weight_decay=1e-2)
    b = driver.FlatAdamW([pb], lr=3e-3, weight_decay=1e-2, max_grad_norm=MAX_NORM)
    pa.grad, pb.grad = values.clone().to(dev), values.clone().to(dev)
    total = torch.nn.utils.clip_grad_norm_([pa], MAX_NORM)
    a.step()
    b.step()
    pair = b.last_grad_norm

    def same(x, y):
        return torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x, nan=7.0), torch.nan_to_num(y, nan=7.0))
    assert same(pair[0], total) and same(pair[1], torch.clamp(MAX_NORM / (total + 1e-6), max=1.0))
    assert (float(pair[1]) == 0.0) if bad == float("inf") else bool(torch.isnan(pair).all())
    assert same(pa.grad, pb.grad) and same(pa.detach(), pb.detach())
    for key in ("exp_avg", "exp_avg_sq"):
        assert same(a.state[pa][key], b.state[pb][key]), key
    assert int(torch.isnan(pb.grad).sum()) == (1 if bad == float("inf") else n)


# ------------------------------------------------------------------ the training loop
def _loop(clip, steps=2, set_attribute=True):
    """FlatTraining on the small synthetic batch of tests/test_gpu_cotangent.py; -> (handle, model, per-step records, calls of
    trajsde_grad_norm_clip / trajsde_adamw_step_clipped / trajsde_adamw_step)"""
    import test_gpu_cotangent as TC
    from trajsde_amd import _lib, driver
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import synth
    dev = torch.device("cuda:0")
    model, _, _ = TC._step_model(TC.CUSTOM, (1.0, 0.5, 0.7))
    model.lr, model.weight_decay, model.T_max = 1e-3, 1e-4, 4
    if set_attribute:
        model.gradient_clip_val = clip
    model = model.to(dev)
    batch = synth(S=2, n=9, L=4, F=20, box=70.0, seed=12, mixed_source=True).to(dev)
    y0 = batch.y.clone()
    L = _lib.lib()
    names = ("trajsde_grad_norm_clip", "trajsde_adamw_step_clipped", "trajsde_adamw_step")
    calls, reals = [], {k: getattr(L, k) for k in names}
    for k in names:
        setattr(L, k, (lambda real, k: lambda *a: (calls.append(k), real(*a))[1])(reals[k], k))
    try:
        ft = driver.FlatTraining(model)
        assert isinstance(ft.optimizer, driver.FlatAdamW)
        records = []
        for i in range(steps):
            ft.zero()
            batch.y = y0.clone()
            model.training_step(batch, i, noise=NoiseSpec(seed=50 + i)).backward()
            before = ft.grads.flat.clone()
            ft.step()
            records.append((before, ft.grads.flat.clone(), ft.last_grad_norm))
        torch.cuda.synchronize()
    finally:
        for k in names:
            setattr(L, k, reals[k])
    return ft, model, records, calls


@pytest.fixture(scope="module")
def unclipped(dev):
    return _loop(None)


def test_without_a_clip_value_the_loop_is_the_loop_it_was(unclipped, dev):
    """gradient_clip_val None, 0 or absent: trajsde_grad_norm_clip and trajsde_adamw_step_clipped are never called, one
    trajsde_adamw_step a step, the gradient is left as it was, and the parameters of the three runs are the same words"""
    ft, model, records, calls = unclipped
    assert calls == ["trajsde_adamw_step"] * 2 and ft.last_grad_norm is None and ft.max_grad_norm is None
    assert all(torch.equal(before, after) and pair is None for before, after, pair in records)
    for kw in (dict(clip=0), dict(clip=None, set_attribute=False)):
        ft2, _, _, calls2 = _loop(**kw)
        assert calls2 == calls and ft2.max_grad_norm is None
        assert torch.equal(_bits(ft.flat_param), _bits(ft2.flat_param)), kw


def test_flat_training_clips_the_global_norm_inside_the_step(unclipped, dev):
    ft0, model0, records0, _ = unclipped
    observed = float(records0[0][0].double().norm())
    assert observed > 0
    clip = 0.1 * observed
    ft, model, records, calls = _loop(clip)
    assert calls == ["trajsde_grad_norm_clip", "trajsde_adamw_step_clipped"] * 2 and ft.max_grad_norm == clip
    for step, (before, after, pair) in enumerate(records):
        pair_h = pair.cpu()
        want = float(before.double().norm())
        ulp = float(np.spacing(np.float32(want)))
        print(f"step {step}: norm {float(pair_h[0])!r} float64 {want!r}, coef {float(pair_h[1])!r}")
        assert abs(float(pair_h[0]) - want) <= ulp
        assert float(pair_h[1]) < 1.0 and torch.equal(_bits(pair_h[1:]), _bits(_torch_coef(pair_h[:1], clip)))
        assert torch.equal(_bits(after), _bits(before * pair[1]))           # .grad holds the scaled gradient ...
        assert abs(float(after.double().norm()) / (clip * want / (want + 1e-6)) - 1) < 1e-5      # ... whose norm is the clip value
    assert ft.last_grad_norm is records[-1][2]
    assert all(p.grad.data_ptr() == ft.grads.flat.data_ptr() + 4 * o for p, o in zip(ft.grads.params, ft.grads.offsets))
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert torch.equal(_bits(records[0][0]), _bits(records0[0][0]))         # the same first gradient, another update
    assert not torch.equal(ft.flat_param.detach(), ft0.flat_param.detach())
    sd = ft.optimizer_state_dict()                                          # configuration, not state: the reference's layout
    assert sd["param_groups"][0].keys() == ft0.optimizer_state_dict()["param_groups"][0].keys()
    assert sd["state"].keys() == ft0.optimizer_state_dict()["state"].keys()
