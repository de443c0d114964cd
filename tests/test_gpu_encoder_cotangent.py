"""trajsde_encoder_cotangent_backward (-m gpu), the C-ABI call itself through runtime.StageRuntime.encoder_cotangent_backward: against
trajsde_encoder_backward, whose launches it shares behind the DLDG producer -- bit for bit where no cotangent reaches the diffusion
outputs, within the backward tests' bound (helpers.compare_grads: max|got - want| <= 2e-4 x max|want| + 1e-7 per tensor) where the
cotangent is torch's gradient of w x DiffBCE; with the tape handed over and recomputed; with a cotangent in a single channel."""
import ctypes as C

import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
SEED = 23


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def case(dev):
    """three mixed-source scenes of 14 actors (N + A = 45: two full row tiles and a ragged one), late first observations"""
    from trajsde_amd import runtime
    from trajsde_amd.synth import synth
    batch = synth(S=3, n=14, L=6, F=5, box=60.0, seed=514, mixed_source=True, history_dropout=0.4)
    model, _ = H.build_model(2, 5, 0.5, init_seed=17)
    H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
    model = model.to(dev)
    data = batch.to(dev)
    rot, y_rot = runtime.rotate_inputs(data)
    data.y, data["rotate_mat"] = y_rot, rot
    noise = runtime.NoiseSpec(seed=SEED)
    rt = model.encoder._rt
    with torch.no_grad():
        outs, _ = rt.encoder_forward_train(data, noise)
    N, A = batch.num_nodes, 3
    assert tuple(outs[1].shape) == tuple(outs[2].shape) == (A, 64)
    d_local = torch.randn(N, 64, generator=torch.Generator().manual_seed(5)).to(dev)
    return model, rt, data, noise, outs, d_local, N, A


def _all(res):
    d = dict(res["grads"])
    d.update(d_latent=res["d_latent"], d_aa_out=res["d_aa_out"])
    return d


def _tape(rt, data, noise, tape_valid):
    """a fresh tape of the training forward (tape_valid = 1), or None: the backward recomputes the forward (tape_valid = 0)"""
    return rt.encoder_forward_train(data, noise)[1] if tape_valid else None


@pytest.mark.parametrize("tape_valid", [0, 1])
def test_without_diffusion_cotangents_it_is_the_welded_call_at_weight_zero(tape_valid, case):
    model, rt, data, noise, outs, d_local, N, A = case
    want = _all(rt.encoder_backward(data, d_local, noise, diff_weight=0.0, want_boundaries=True, tape=_tape(rt, data, noise, tape_valid)))
    null = rt.encoder_cotangent_backward(data, d_local, None, None, noise, tape=_tape(rt, data, noise, tape_valid), want_boundaries=True)
    assert "diff_loss" not in null
    zeros = torch.zeros(A, 64, device=d_local.device)
    zero = rt.encoder_cotangent_backward(data, d_local, zeros, zeros.clone(), noise, tape=_tape(rt, data, noise, tape_valid), want_boundaries=True)
    one_side = rt.encoder_cotangent_backward(data, d_local, None, zeros, noise, tape=_tape(rt, data, noise, tape_valid), want_boundaries=True)
    torch.cuda.synchronize()
    assert float(want["aa_encoder.lin_q.weight"].abs().max()) > 0 and float(want["d_aa_out"].abs().max()) > 0
    for tag, res in (("null", null), ("zeros", zero), ("null | zeros", one_side)):
        got = _all(res)
        assert list(got) == list(want)
        assert [k for k in want if not torch.equal(got[k], want[k])] == [], tag


@pytest.mark.parametrize("tape_valid", [0, 1])
@pytest.mark.parametrize("w", [0.5, 1.0])
def test_the_torch_gradient_of_diffbce_reproduces_the_welded_call(w, tape_valid, case):
    from trajsde_amd import losses
    model, rt, data, noise, outs, d_local, N, A = case
    di, do = outs[1].detach().clone().requires_grad_(True), outs[2].detach().clone().requires_grad_(True)
    with torch.enable_grad():
        value = w * losses.DiffBCE()(None, {"diff_in": di, "diff_out": do, "label_in": outs[3], "label_out": outs[4]})
        d_in, d_out = torch.autograd.grad(value, [di, do])
    welded = rt.encoder_backward(data, d_local, noise, diff_weight=w, want_boundaries=True, tape=_tape(rt, data, noise, tape_valid))
    assert abs(float(value) - float(welded["diff_loss"])) <= 2e-5 * max(1.0, abs(float(value)))
    res = rt.encoder_cotangent_backward(data, d_local, d_in, d_out, noise, tape=_tape(rt, data, noise, tape_valid), want_boundaries=True)
    again = rt.encoder_cotangent_backward(data, d_local, d_in, d_out, noise, tape=_tape(rt, data, noise, tape_valid), want_boundaries=True)
    torch.cuda.synchronize()
    got, want = _all(res), _all(welded)
    assert [k for k in got if not torch.equal(got[k], _all(again)[k])] == []          # identical calls, identical words
    # the cotangent moved something: not the weight-zero result
    base = rt.encoder_cotangent_backward(data, d_local, None, None, noise, want_boundaries=True)
    assert not torch.equal(base["grads"]["lsde_func.g_nus.net.4.weight"], got["lsde_func.g_nus.net.4.weight"])
    bad = H.compare_grads(f"encoder cotangent vs welded DiffBCE, w={w} tape_valid={tape_valid}", got, want)
    assert not bad, bad


def test_a_cotangent_in_a_single_channel(case):
    """the diffusion output is one value repeated over 64 channels: only the channel sum of its cotangent matters, and the sum of one
    non-zero word and 63 zeros is that word exactly -- wherever it stands"""
    model, rt, data, noise, outs, d_local, N, A = case
    g = torch.Generator().manual_seed(6)
    v_in, v_out = torch.randn(A, generator=g), torch.randn(A, generator=g)

    def run(c_in, c_out):
        d_in, d_out = torch.zeros(A, 64), torch.zeros(A, 64)
        d_in[:, c_in], d_out[:, c_out] = v_in, v_out
        return _all(rt.encoder_cotangent_backward(data, d_local, d_in.to(d_local.device), d_out.to(d_local.device), noise, want_boundaries=True))
    a, b, c = run(0, 0), run(37, 63), run(63, 1)
    base = _all(rt.encoder_cotangent_backward(data, d_local, None, None, noise, want_boundaries=True))
    torch.cuda.synchronize()
    assert [k for k in a if not torch.equal(a[k], b[k]) or not torch.equal(a[k], c[k])] == []
    assert not torch.equal(a["lsde_func.g_argo.net.4.weight"], base["lsde_func.g_argo.net.4.weight"])
    # spread evenly over the channels instead (1/64 is a power of two: the same sum up to the tree's rounding)
    d_in, d_out = (v_in[:, None] / 64).expand(A, 64).contiguous(), (v_out[:, None] / 64).expand(A, 64).contiguous()
    spread = _all(rt.encoder_cotangent_backward(data, d_local, d_in.to(d_local.device), d_out.to(d_local.device), noise, want_boundaries=True))
    bad = H.compare_grads("single channel vs spread", spread, a, rel=2e-5)
    assert not bad, bad


def test_refusals(case):
    """what the header lists: a null required pointer, a graph without the fake-agent rows (A = 0), a wrong gradient count, a
    workspace below the query -- each an error status with a message, no launch"""
    from trajsde_amd import _lib, runtime
    model, rt, data, noise, outs, d_local, N, A = case
    m = model.encoder
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    dev = d_local.device
    tab = rt._enc_table()
    tab_dev = torch.from_numpy(tab).to(dev)
    grads = rt._grad_buffers(_lib.STAGE_ENCODER_BWD)
    arr, _keep = grads.pointer_array()
    cn = noise.c_noise(None, None)

    def call(gc, d_local_ptr, n_grads, ws_bytes=None):
        full = L.trajsde_encoder_backward_ws_bytes(C.byref(gc.batch), C.byref(gc.graph))
        ws = torch.empty(full, device=dev, dtype=torch.uint8)
        return L.trajsde_encoder_cotangent_backward(
            C.byref(gc.batch), C.byref(gc.graph), gc.rot.data_ptr(), rt.blob().data_ptr(), rt.blob(_lib.STAGE_ENCODER_BWD).data_ptr(),
            tab.ctypes.data_as(C.c_void_p), tab_dev.data_ptr(), C.byref(cn), d_local_ptr, None, None, ws.data_ptr(),
            full if ws_bytes is None else ws_bytes, arr, n_grads, None, None, None, 0, None, 0, st)

    gc = runtime.GraphContext.get(data, float(m.local_radius), int(m.historical_steps), noise)
    assert call(gc, None, len(grads)) != 0 and b"encoder_cotangent_backward: null pointer" in L.trajsde_last_error()
    assert call(gc, d_local.data_ptr(), len(grads) - 1) != 0 and b"gradient count" in L.trajsde_last_error()
    assert call(gc, d_local.data_ptr(), len(grads), ws_bytes=1024) != 0 and b"workspace too small" in L.trajsde_last_error()
    assert call(gc, d_local.data_ptr(), len(grads)) == 0                                  # the one-buffer form (scratch = null) runs
    bare = runtime.GraphContext.get(data, float(m.local_radius), int(m.historical_steps), noise, fake_agents=False)
    assert bare.batch.A == 0
    assert call(bare, d_local.data_ptr(), len(grads)) != 0 and b"fake-agent rows" in L.trajsde_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grads.flat).all()) and float(grads.flat.abs().max()) > 0
