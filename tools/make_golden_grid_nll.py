"""Generate tests/golden/train_grid_nll/*.npz: the REFERENCE's vanilla HiVT model (models/model_base_mix.py PredictionModel with
configs/nusargo/hivt_nuSArgo_trmenc_mlpdec.yml) trained under losses/laplace_nll_loss.py in place of losses/L2.py -- its loss value
and the digests of every parameter gradient its own torch.autograd produces, at perturbed weights, dropout off.

    python tools/make_golden_grid_nll.py            # only where the reference tree is present

The pieces are oracle/make_golden_train.py make_grid's (the batch, the weight perturbation, the torch 1.x TransformerEncoder, the
ReLU kink guard, the digest format that tests/helpers.py load_train_fixture reads); this script only swaps the regression loss,
whose module make_grid hard-codes, and writes its own output path.
"""
import os
import sys

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]

import make_golden_grid as G                                   # noqa: E402
import ref_loader as R                                         # noqa: E402
from make_golden_train import GRID_KINK_MARGIN, digest_signs  # noqa: E402
from trajsde_amd.models.model_base_mix import PredictionModel  # noqa: E402
from trajsde_amd.synth import synth                           # noqa: E402

OUT_DIR = os.path.join(ROOT, "tests", "golden", "train_grid_nll")
CASES = {
    # name: (synth kwargs, num_modes, future_steps, num_heads, temporal layers, init_seed): train_grid_k3_t12_h4's batch + weights
    "grid_nll_k3_t12_h4": (dict(S=3, n=9, L=6, F=12, box=70.0, seed=23, mixed_source=True, history_dropout=0.3), 3, 12, 4, 2, 43),
}
NLL_ARGS = {"eps": 1e-6, "reduction": "mean"}


def with_nll(cfg):
    """the config with the reference's Laplace NLL module as its only loss"""
    cfg["losses"], cfg["losses_module"], cfg["loss_weights"], cfg["loss_args"] = (
        ["losses/laplace_nll_loss.py"], ["LaplaceNLLLoss"], [1], [dict(NLL_ARGS)])
    return cfg


def make(name):
    skw, K, T, heads, layers, init_seed = CASES[name]
    batch = synth(**skw)
    with open(os.path.join(ROOT, "trajsde_amd/configs/mi355x_trmenc_mlpdec.yml")) as f:
        ours_cfg = G.edit(yaml.safe_load(f), K, T, heads, layers)
    ours = PredictionModel(**ours_cfg, init_seed=init_seed)
    g = torch.Generator().manual_seed(1000 + init_seed)
    with torch.no_grad():                                     # leave the initial point: zero biases hide bias-gradient bugs
        for p in ours.parameters():
            if p.requires_grad:
                p.add_(0.02 * torch.randn(p.shape, generator=g))
    sd = {k: v.detach().clone() for k, v in ours.state_dict().items()}
    with open(os.path.join(R.REFERENCE_ROOT, G.REF_CFG)) as f:
        ref_cfg = with_nll(G.edit(yaml.safe_load(f), K, T, heads, layers))
    ref = R.build_reference_model(ref_cfg)
    ref.load_state_dict(sd)
    assert ref.loss_names == ["LaplaceNLLLoss"], ref.loss_names
    ref.eval()                                                # dropout off
    data = R.to_reference_data(batch)
    # the ReLU kink guard of make_grid (module ReLUs, the scale head's among them: under this loss its gradient matters too)
    nearest = [float("inf")]
    hooks = [m.register_forward_pre_hook(lambda _m, a: nearest.__setitem__(0, min(nearest[0], float(a[0].detach().abs().min()))))
             for m in ref.modules() if isinstance(m, torch.nn.ReLU)]
    stock = torch.nn.TransformerEncoder.forward
    torch.nn.TransformerEncoder.forward = G.torch1_transformer_encoder_forward
    try:
        with R.reference_cwd(), torch.enable_grad():
            out = ref(data)
            parts = [fn(data, out) for fn in ref.losses]
            loss = sum(w * l for w, l in zip(ref.loss_weights, parts))
            loss.backward()
    finally:
        torch.nn.TransformerEncoder.forward = stock
        for h in hooks:
            h.remove()
    print(f"{name}: nearest ReLU input to zero {nearest[0]:.3e}")
    assert nearest[0] > GRID_KINK_MARGIN, f"{name}: a ReLU input at {nearest[0]:.2e} -- a kink, choose another init_seed"
    fx = {f"in.{k}": v.numpy() for k, v in batch.as_dict().items() if torch.is_tensor(v)}
    fx.update({"meta.num_modes": K, "meta.future_steps": T, "meta.num_heads": heads, "meta.num_temporal_layers": layers,
               "meta.init_seed": init_seed, "meta.perturb_seed": 1000 + init_seed, "meta.state_checksum": G.state_checksum(sd),
               "meta.nll_eps": NLL_ARGS["eps"]})
    for nm, w, l in zip(ref.loss_names, ref.loss_weights, parts):
        fx[f"loss.{nm}"] = np.float64(float(l))
        fx[f"weight.{nm}"] = np.float64(float(w))
    fx["loss.total"] = np.float64(float(loss))
    n_grad = 0
    for k, p in ref.named_parameters():
        if p.grad is None:
            continue
        gr = p.grad.detach().double().reshape(-1)
        n_grad += 1
        fx[f"digest.{k}"] = np.array([float(gr.norm()), float((gr * digest_signs(k, gr.numel())).sum())] + gr[:30].tolist(),
                                     dtype=np.float64)
    assert any(k.startswith("digest.decoder.scale.") for k in fx) and not any(k.startswith("digest.decoder.pi.") for k in fx)
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, **fx)
    print(f"{name}: N={batch.num_nodes} K={K} T={T} loss={float(loss):.6f} grads={n_grad} -> {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    if not R.reference_available():
        sys.exit("reference tree not found; golden vectors can only be generated where it is present")
    for name in (sys.argv[1:] or list(CASES)):
        make(name)
