"""Float64 yardstick of the vanilla variant under the Laplace NLL: whole-model autograd over oracle/restate_grid.py with
helpers.reference_laplace_nll (the Laplace NLL twin of helpers.oracle_grid_full_grads), the reference fixture of that training step
and the config that selects the loss.  Shared by tests/test_grid_nll_cpu.py, which pins the yardstick against the reference's own
training step, and tests/test_gpu_grid_nll.py."""
import os

import numpy as np
import torch

import helpers as H

FIXTURE = os.path.join(H.ROOT, "tests", "golden", "train_grid_nll", "grid_nll_k3_t12_h4.npz")


def oracle_grid_nll_grads(model, cfg, batch_cpu, eps=1e-6):
    """float64 autograd over oracle/restate_grid.py: the whole vanilla model (eval mode) under the Laplace NLL
    -> (loss, {name: grad or None})"""
    import restate
    import restate_grid
    c = restate_grid.flat_cfg(cfg)
    dt = torch.float64
    P = {k: (v.detach().cpu().to(dt) if v.is_floating_point() else v.detach().cpu().clone()) for k, v in model.state_dict().items()}
    names = [k for k in P if P[k].is_floating_point() and not k.endswith("attn_mask")]
    for k in names:
        P[k].requires_grad_(True)
    b = H.clone_batch(batch_cpu)
    for k in b.keys:
        if torch.is_tensor(b[k]) and b[k].is_floating_point():
            b[k] = b[k].to(dt)
    torch.set_default_dtype(dt)
    try:
        rot, y_rot = restate.rotate_inputs(b)
        with torch.enable_grad():
            local = restate_grid.local_encoder_grid(P, c, b, rot)
            glob = restate.global_interactor(P, c, b, rot, local, None)
            out = restate_grid.mlp_decoder(P, c, b, local, glob)
            loss, _ = H.reference_laplace_nll(y_rot, out["loc"], out["reg_mask"], eps)
            loss.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return float(loss.detach()), {k: P[k].grad for k in names}


def load_fixture():
    """the reference's vanilla training step under losses/laplace_nll_loss.py (tools/make_golden_grid_nll.py), in the format of
    helpers.load_train_fixture: (batch, meta, losses, weights, grads, digests)"""
    from trajsde_amd.data import TemporalData
    z = np.load(FIXTURE)
    batch = TemporalData(**{k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in.")})
    batch["num_nodes"] = batch["x"].shape[0]
    meta = {k[5:]: z[k].item() for k in z.files if k.startswith("meta.")}
    losses = {k[5:]: float(z[k]) for k in z.files if k.startswith("loss.")}
    weights = {k[7:]: float(z[k]) for k in z.files if k.startswith("weight.")}
    grads = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("grad.")}
    digests = {k[7:]: z[k] for k in z.files if k.startswith("digest.")}
    return batch, meta, losses, weights, grads, digests


def nll_cfg(K, T, heads, layers, dropout=0.0, eps=1e-6):
    """helpers.grid_cfg with trajsde_amd.losses.LaplaceNLLLoss as the only loss (how a user enables it in the shipped YAML)"""
    cfg = H.grid_cfg(K, T, heads, layers, dropout=dropout)
    cfg["losses_module"] = ["LaplaceNLLLoss"]
    cfg["loss_args"] = [{"eps": eps, "reduction": "mean"}]
    return cfg
