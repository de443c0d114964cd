"""The trained-like weight profile (helpers.trained_like_parameters) on the oracle alone, no GPU: every parameter the kernels fold
into their weight images (csrc/pack.hip: LayerNorm gamma as a column scale, W beta + b as a constant, centred and prescaled biases)
visibly moves the outputs at that profile -- so that the GPU tests of tests/test_gpu_trained_weights.py, which compare the kernels
with the float64 oracle there, fail when one of those folds is wrong.  At the initial weights (biases 0, gamma 1) none of this is
tested: a dropped or misplaced constant is exactly zero there."""
import pytest
import torch

import helpers as H

TOL = 1e-4                      # the parity tolerance of the GPU suite
KEYS = ("loc", "pi", "diff_in", "diff_out")


def _case(strength):
    K, T, max_t, make = H.TRAINED_CASES["mixed_k6_t20"]
    model, cfg = H.build_model(K, T, max_t, init_seed=2)
    init = {k: v.clone() for k, v in model.state_dict().items()}
    H.trained_like_parameters(model, H.TRAINED_SEED, strength)
    return model, cfg, make(), init


def test_profile_is_deterministic_and_leaves_the_initial_point():
    a, _ = H.build_model(6, 20, 2.0, init_seed=2)
    b, _ = H.build_model(6, 20, 2.0, init_seed=2)
    init = {k: v.clone() for k, v in a.state_dict().items()}
    H.trained_like_parameters(a, 5, 1.0)
    H.trained_like_parameters(b, 5, 1.0)
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    folds = H.fold_tensors(a)
    assert len(folds) == 158                                    # 128 biases (LayerNorm betas among them) + 30 LayerNorm gammas
    for k in folds:
        assert not torch.equal(sa[k], init[k]), k
    gammas = [k for k in folds if not k.endswith(".bias")]
    assert len(gammas) == 30 and all(float(init[k].sub(1).abs().max()) == 0.0 for k in gammas)
    assert any(float(sa[k].min()) < 0 for k in gammas)          # some LayerNorm gammas flip sign
    for k in ("encoder.hidden", "decoder.hidden", "encoder.aa_encoder.bos_token"):
        assert not torch.equal(sa[k], init[k]), k
    for k in ("encoder.lsde_func.h_func.theta", "decoder.lsde_func.h_func.mu"):   # the frozen prior constants stay
        assert torch.equal(sa[k], init[k]), k
    for k, v in sa.items():                                     # matrices: scaled, never shrunk, never flipped
        if v.dim() == 2 and k.endswith(".weight"):
            assert bool((v.abs() >= init[k].abs()).all()) and bool((v * init[k] >= 0).all()), k


@pytest.mark.parametrize("strength", H.TRAINED_STRENGTHS)
def test_float64_oracle_is_the_fp32_oracle_to_well_inside_tol(strength):
    """the float64 oracle takes the same fp32 normals: it differs from the fp32 oracle (pinned to the reference by the golden
    fixtures) only by the fp32 rounding, far inside TOL, so it leaves the kernels their own error budget"""
    model, cfg, batch, _ = _case(strength)
    ref = H.oracle_forward64(model, cfg, batch, noise_seed=6, want_intermediates=False)
    r32 = H.oracle_forward(model, cfg, batch, noise_seed=6, want_intermediates=False)
    assert ref["loc"].dtype == torch.float64 and r32["loc"].dtype == torch.float32
    for k in KEYS:
        assert H.maxdiff(ref[k], r32[k]) <= TOL / 10, k


def test_every_folded_parameter_moves_the_oracle_at_the_profile():
    """resetting any one bias or LayerNorm tensor (bar the key biases, which the softmax cannot see) to its initial value moves an
    output by at least 10 x TOL at strength 1 on the first case batch"""
    model, cfg, batch, init = _case(1.0)
    ref = H.oracle_forward64(model, cfg, batch, noise_seed=6, want_intermediates=False)
    sd = model.state_dict()
    weak, moved = [], {}
    for name in H.fold_tensors(model):
        keep = sd[name].clone()
        with torch.no_grad():
            sd[name].copy_(init[name])
        try:
            o = H.oracle_forward64(model, cfg, batch, noise_seed=6, want_intermediates=False)
        finally:
            with torch.no_grad():
                sd[name].copy_(keep)
        moved[name] = max(H.maxdiff(o[k], ref[k]) for k in KEYS)
        if H.zero_by_softmax_symmetry(name):
            assert moved[name] <= 1e-9, (name, moved[name])     # ... and the symmetry holds: the kernels may drop them
        elif moved[name] < 10 * TOL:
            weak.append((name, moved[name]))
    assert sum(H.zero_by_softmax_symmetry(n) for n in moved) == 8
    assert not weak, weak
