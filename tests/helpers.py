"""Shared helpers for the parity tests: golden fixture loading, model construction, oracle runs."""
import glob
import os

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))


# the irregular-mask fixtures other than the forward one (trajsde_amd/synth.py irregular_masks): name -> folder under tests/
FIXTURE_FOLDERS = {"ood_irregular_k3_t5": "golden/irregular_ood", "grid_irregular_k3_t12_h4": "golden/irregular_grid",
                   "train_irregular_k3_t12": "golden/irregular_train", "train_grid_irregular_k3_t12_h4": "golden/irregular_train"}


def fixture_arrays(name, folder):
    """{key: array} of tests/<folder>/<name>.npz, or of every part file of the folder tests/<folder>/<name>/ (a fixture too large
    for one file); `folder` None: FIXTURE_FOLDERS[name]"""
    base = os.path.join(ROOT, "tests", *(FIXTURE_FOLDERS[name] if folder is None else folder).split("/"), name)
    files = sorted(glob.glob(os.path.join(base, "*.npz"))) if os.path.isdir(base) else [base + ".npz"]
    assert files, base
    arrays = {}
    for f in files:
        z = np.load(f)
        assert not set(z.files) & set(arrays), f
        arrays.update({k: z[k] for k in z.files})
    return arrays


def our_cfg(num_modes, future_steps, max_fut_t, uncertain=True):
    with open(os.path.join(ROOT, "trajsde_amd/configs/mi355x_sde_encoder_decoder.yml")) as f:
        cfg = yaml.safe_load(f)
    cfg["model_specific"]["kwargs"].update(num_modes=num_modes, future_steps=future_steps)
    cfg["aggregator"]["kwargs"]["num_modes"] = num_modes
    cfg["decoder"]["kwargs"].update(num_modes=num_modes, future_steps=future_steps, max_fut_t=max_fut_t)
    if not uncertain:                                          # DEC:56: the decoder without its scale head
        cfg["decoder"]["kwargs"]["uncertain"] = False
    return cfg


def load_fixture(name):
    from trajsde_amd.data import TemporalData
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    batch = TemporalData(**{k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in.")})
    batch["num_nodes"] = batch["x"].shape[0]
    meta = {k[5:]: z[k].item() for k in z.files if k.startswith("meta.")}
    out = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("out.")}
    mid = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("mid.")}
    return batch, meta, out, mid


def build_model(meta_or_K, T=None, max_t=None, init_seed=0):
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    uncertain = True
    if isinstance(meta_or_K, dict):
        m = meta_or_K
        K, T, max_t, init_seed = int(m["num_modes"]), int(m["future_steps"]), float(m["max_fut_t"]), int(m["init_seed"])
        uncertain = bool(int(m.get("uncertain", 1)))
    else:
        K = meta_or_K
    cfg = our_cfg(K, T, max_t, uncertain)
    return PredictionModelSDENet(**cfg, init_seed=init_seed).eval(), cfg


def state_checksum(sd):
    return float(sum(v.double().abs().sum() for v in sd.values()))


def clone_batch(batch):
    from trajsde_amd.data import TemporalData
    return TemporalData(**{k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.as_dict().items()})


def oracle_forward(model, cfg, batch, noise_seed, want_intermediates=True):
    import restate
    P = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    return restate.forward(P, cfg, clone_batch(batch).to("cpu"), restate.PhiloxNoise(int(noise_seed)),
                           want_intermediates=want_intermediates)


def double_batch(batch):
    b = clone_batch(batch).to("cpu")
    for k in b.keys:
        if torch.is_tensor(b[k]) and b[k].is_floating_point():
            b[k] = b[k].double()
    return b


class Float64Noise:
    """a restate noise source whose float32 normals (the Philox stream the kernels draw, or injected ones) are handed on as float64:
    the same numbers, so that a float64 oracle run differs from the kernels only by their arithmetic"""

    def __init__(self, inner):
        self.inner = inner

    def fake_agent(self, shape):
        return self.inner.fake_agent(shape).detach().cpu().double()

    def encoder(self, idx, shape):
        return self.inner.encoder(idx, shape).detach().cpu().double()

    def decoder(self, k, shape):
        return self.inner.decoder(k, shape).detach().cpu().double()


def oracle_forward64(model, cfg, batch, noise_seed=None, noise=None, want_intermediates=True, ood=False, drop=None, device="cpu"):
    """oracle_forward in float64: the parameters and the batch's floating tensors cast to double, the fp32 normals of Philox seed
    `noise_seed` (or the restate noise source `noise`, e.g. restate.InjectedNoise) taken as they are.  Outputs are float64, on
    `device` (the host by default; a GPU for whole full-size batches)."""
    import restate
    P = {k: (v.detach().to(device, torch.float64) if v.is_floating_point() else v.detach().to(device).clone())
         for k, v in model.state_dict().items()}
    src = restate.PhiloxNoise(int(noise_seed)) if noise is None else noise
    return restate.forward(P, cfg, double_batch(batch).to(device), Float64Noise(src), want_intermediates=want_intermediates, ood=ood,
                           drop=drop)


def trained_like_parameters(model, seed, strength=1.0):
    """move every trainable parameter away from the initial point the way training does, so that the biases, LayerNorm affines,
    tokens and hidden vectors the kernels fold into their weight images (csrc/pack.hip) are no longer 0 / 1: with one normal
    draw z per entry, from one CPU generator in parameters() order,
      matrices           W <- W * (1 + 0.3 s |z|)
      biases (LN too)    b <- 0.3 s z
      LayerNorm gamma    g <- 1 + 0.4 s z        (some entries negative)
      tokens, hidden     t <- t + 0.3 s z
    with s = `strength`.  The frozen prior constants (h_func) are left alone.  Writes go through the parameters themselves (not
    `.data`), so their version counters move and the next forward re-packs."""
    g = torch.Generator().manual_seed(int(seed))
    s = float(strength)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if not p.requires_grad:
                continue
            z = torch.randn(p.shape, generator=g).to(p.device)
            if name.endswith("bias"):                                   # (nn.MultiheadAttention's in_proj_bias too)
                p.copy_(0.3 * s * z)
            elif name.endswith("weight") and p.dim() == 1:
                p.copy_(1.0 + 0.4 * s * z)
            elif name.endswith("weight") and p.dim() == 2:              # (in_proj_weight too)
                p.mul_(1.0 + 0.3 * s * z.abs())
            else:
                p.add_(0.3 * s * z)


def fold_tensors(model):
    """the state-dict entries a weight image folds away (see trained_like_parameters): every bias and every LayerNorm gamma"""
    return [k for k, v in model.state_dict().items() if k.endswith(".bias") or (k.endswith(".weight") and v.dim() == 1)]


def zero_by_softmax_symmetry(name):
    """key biases: a constant added to every logit of a softmax segment, so they cannot move any output"""
    return name.endswith("lin_k.bias") or name.endswith("lin_k_node.bias") or name.endswith("lin_k_edge.bias")


def maxdiff(a, b):
    return float((a.double() - b.double()).abs().max()) if a.numel() else 0.0


def load_reference_call(name):
    """tests/golden/reference_calls/<name>.npz (oracle/make_golden_reference_calls.py): what one of the reference's own
    functions returned on stored or seeded inputs, as {key: tensor}"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "reference_calls", name + ".npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def leave_only_agent_case():
    """the collated batch (3 scenes, ragged lanes) and forward output that reference_calls/leave_only_agent.npz holds the
    reference's `leave_only_agent` (MODEL:168-202) result for"""
    from trajsde_amd.data import collate
    from trajsde_amd.synth import synth
    batch = collate([synth(S=1, n=n, L=L, F=5, box=60.0, seed=s) for n, L, s in ((5, 3, 1), (7, 4, 2), (4, 2, 3))])
    N, K, T = batch["x"].shape[0], 2, 5
    g = torch.Generator().manual_seed(0)
    batch["rotate_mat"] = torch.randn(N, 2, 2, generator=g)
    batch["has_goal"] = torch.arange(N) % 2 == 0
    batch["goal_idcs"] = torch.arange(batch["lane_actor_index"].shape[1])
    out = {"loc": torch.randn(K, N, T, 4, generator=g), "pi": torch.randn(N, K, generator=g),
           "reg_mask": torch.rand(N, T, generator=g) > 0.3}
    return batch, out


LEAVE_ONLY_AGENT_KEYS = ("x", "y", "positions", "padding_mask", "bos_mask", "rotate_mat", "rotate_angles", "has_goal", "goal_idcs",
                         "lane_actor_vectors", "lane_actor_index", "agent_index", "av_index", "batch")


def reference_l2(y, loc, reg_mask):
    """losses/L2.py:10-27 spelled out on tensors (mean reduction)"""
    l2 = torch.norm(y.unsqueeze(0) - loc, p=2, dim=-1)
    ade = l2.clone()
    ade[:, ~reg_mask] = 0
    best = torch.argmin(ade.mean(-1), dim=0)
    minl2 = l2[best, torch.arange(l2.size(1), device=l2.device)]
    return minl2[reg_mask].mean(), best


def reference_laplace_nll(y, out_loc4, reg_mask, eps=1e-6):
    """losses/laplace_nll_loss.py:29-44 spelled out on tensors (mean reduction; the clamp is applied without a gradient)"""
    loc, scale = out_loc4.chunk(2, dim=-1)
    diff = torch.norm(y.unsqueeze(0) - loc, dim=-1)
    d_ = diff.clone()
    d_[:, ~reg_mask] = 0
    best = torch.argmin(d_.mean(-1), dim=0)
    ar = torch.arange(best.size(0), device=best.device)
    loc, scale = loc[best, ar], scale[best, ar]
    scale = scale.clone()
    with torch.no_grad():
        scale.clamp_(min=eps)
    nll = torch.log(2 * scale) + torch.abs(y - loc) / scale
    return nll[reg_mask].mean(), best


def oracle_full_grads(model, cfg, batch_cpu, seed, w_l2, w_diff, want_parts=False, drop=None, nll_eps=None, dt=torch.float64,
                      device="cpu"):
    """end-to-end autograd over the oracle (float64, or `dt`): encoder -> aggregator -> decoder -> w_l2 L2 (or, with `nll_eps`, the
    Laplace NLL) + w_diff DiffBCE;
    `drop`: a restate.PhiloxDropout for train-mode dropout (the masks the HIP kernels cut from their Philox stream); `device`: where
    the oracle and its tape live (the gradients are returned there)"""
    import restate
    import torch.nn.functional as F
    from trajsde_amd.schedule import decoder_schedule, encoder_schedule
    c = restate.flat_cfg(cfg)
    es = encoder_schedule(c["historical_steps"], c["max_past_t"], c["minimum_step"])
    ds = decoder_schedule(c["future_steps"], c["max_fut_t"], c["min_stepsize"])
    P = {k: (v.detach().to(device, dt) if v.is_floating_point() else v.detach().to(device).clone()) for k, v in model.state_dict().items()}
    names = [k for k in P if P[k].is_floating_point()]
    for k in names:
        P[k].requires_grad_(True)
    b = clone_batch(batch_cpu).to(device)
    for k in b.keys:
        if torch.is_tensor(b[k]) and b[k].is_floating_point():
            b[k] = b[k].to(dt)

    class Noise64(restate.PhiloxNoise):
        def fake_agent(self, shape):
            return super().fake_agent(shape).to(dt)

        def encoder(self, idx, shape):
            return super().encoder(idx, shape).to(dt)

        def decoder(self, k, shape):
            return super().decoder(k, shape).to(dt)

    torch.set_default_dtype(dt)
    try:
        rot, y_rot = restate.rotate_inputs(b)
        noise = Noise64(seed)
        with torch.enable_grad():
            local, diff_in, diff_out, _ = restate.local_encoder(P, c, b, rot, noise, es, False, drop)
            glob = restate.global_interactor(P, c, b, rot, local, None, drop)
            out = restate.sde_decoder(P, c, b, local, glob, noise, ds)
            if nll_eps is None:
                l2, _ = reference_l2(y_rot, out["loc"][..., :2], out["reg_mask"])
            else:                                                    # the regression loss is the Laplace NLL (both heads trained)
                l2, _ = reference_laplace_nll(y_rot, out["loc"], out["reg_mask"], nll_eps)
            bce = (F.binary_cross_entropy(diff_in, torch.zeros_like(diff_in)) +
                   F.binary_cross_entropy(diff_out, torch.ones_like(diff_out)))
            loss = w_l2 * l2 + w_diff * bce
            loss.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    if want_parts:
        return float(loss.detach()), {k: P[k].grad for k in names}, float(l2.detach()), float(bce.detach())
    return float(loss.detach()), {k: P[k].grad for k in names}


def perturb_parameters(model, seed):
    """leave the initial point the way oracle/make_golden_train.py does: every trainable parameter += 0.02 * N(0,1) drawn
    in parameters() order from one seeded CPU generator"""
    g = torch.Generator().manual_seed(int(seed))
    with torch.no_grad():
        for p in model.parameters():
            if p.requires_grad:
                p.add_(0.02 * torch.randn(p.shape, generator=g).to(p.device))


def fixture_dropout(meta):
    """the PhiloxDropout a train-mode fixture was made with (None for eval-mode fixtures)"""
    import restate
    if "dropout_p" not in meta or float(meta["dropout_p"]) <= 0:
        return None
    return restate.PhiloxDropout(int(meta["dropout_seed"]), float(meta["dropout_p"]))


def load_train_fixture(name, folder=None):
    """tests/golden_train/<name>.npz, or the fixture (a file, or a folder of part files) of that name under tests/<folder>"""
    from trajsde_amd.data import TemporalData
    z = fixture_arrays(name, FIXTURE_FOLDERS.get(name, "golden_train") if folder is None else folder)
    batch = TemporalData(**{k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("in.")})
    batch["num_nodes"] = batch["x"].shape[0]
    meta = {k[5:]: v.item() for k, v in z.items() if k.startswith("meta.")}
    losses = {k[5:]: float(v) for k, v in z.items() if k.startswith("loss.")}
    weights = {k[7:]: float(v) for k, v in z.items() if k.startswith("weight.")}
    grads = {k[5:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("grad.")}
    digests = {k[7:]: v for k, v in z.items() if k.startswith("digest.")}
    return batch, meta, losses, weights, grads, digests


def load_ood_fixture(name, folder=None):
    """(batch, meta, out) of an out-of-distribution forward fixture (oracle/make_golden.py make_ood)"""
    from trajsde_amd.data import TemporalData
    z = fixture_arrays(name, FIXTURE_FOLDERS.get(name, "golden_ood") if folder is None else folder)
    batch = TemporalData(**{k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("in.")})
    batch["num_nodes"] = batch["x"].shape[0]
    meta = {k[5:]: v.item() for k, v in z.items() if k.startswith("meta.")}
    out = {k[4:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("out.")}
    return batch, meta, out


def load_grid_arrays(name, folder=None):
    """{key: array} of a vanilla-HiVT forward fixture (oracle/make_golden_grid.py)"""
    return fixture_arrays(name, FIXTURE_FOLDERS.get(name, "golden_grid") if folder is None else folder)


def digest_signs(key, n):
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()))
    return (torch.randint(0, 2, (n,), generator=g) * 2 - 1).double()


def check_grads_against_train_fixture(got, grads, digests, rel):
    """`got`: {name: tensor or None}.  Full tensors: max-abs error <= rel * largest entry; digests: norm, a seeded +-1
    projection and the leading entries.  The edge-embedding matrices get 2 * rel (ill-conditioned, see test_gpu_backward)."""
    bad = []
    for k, w in grads.items():
        g = got.get(k)
        scale = float(w.abs().max())
        if g is None:
            if scale > 0:
                bad.append((k, "missing", scale))
            continue
        r = 2 * rel if "_embed.module_list" in k else rel
        zero_by_symmetry = k.endswith("lin_k.bias") or k.endswith("lin_k_node.bias") or k.endswith("lin_k_edge.bias")
        err = float((g.detach().cpu().double() - w.double()).abs().max())
        if (err > 5e-5 or scale > 5e-5) if zero_by_symmetry else (err > r * scale + 1e-7):
            bad.append((k, err, scale))
    for k, d in digests.items():
        g = got.get(k)
        norm, proj, lead = float(d[0]), float(d[1]), torch.from_numpy(d[2:])
        if g is None:
            if norm > 0:
                bad.append((k, "missing", norm))
            continue
        gd = g.detach().cpu().double().reshape(-1)
        n = gd.numel()
        r = 2 * rel if "_embed.module_list" in k else rel
        zero_by_symmetry = k.endswith("lin_k.bias") or k.endswith("lin_k_node.bias") or k.endswith("lin_k_edge.bias")
        if zero_by_symmetry:
            if norm > 5e-4 or float(gd.norm()) > 5e-4:
                bad.append((k, float(gd.norm()), norm))
            continue
        tol = r * norm * n ** 0.5 + 1e-7
        if abs(float(gd.norm()) - norm) > tol or abs(float((gd * digest_signs(k, n)).sum()) - proj) > tol:
            bad.append((k, "digest", float(gd.norm()), norm))
        m = min(n, lead.numel())
        if float((gd[:m] - lead[:m]).abs().max()) > r * max(float(lead[:m].abs().max()), norm) + 1e-7:
            bad.append((k, "lead", float((gd[:m] - lead[:m]).abs().max())))
    return bad


def grid_cfg(K, T, heads, layers, dropout=0.0, uncertain=True):
    with open(os.path.join(ROOT, "trajsde_amd/configs/mi355x_trmenc_mlpdec.yml")) as f:
        cfg = yaml.safe_load(f)
    if not uncertain:
        cfg["decoder"]["kwargs"]["uncertain"] = False
    cfg["encoder"]["kwargs"]["dropout"] = dropout
    cfg["aggregator"]["kwargs"]["dropout"] = dropout
    cfg["model_specific"]["kwargs"].update(num_modes=K, future_steps=T)
    cfg["encoder"]["kwargs"].update(num_heads=heads, num_temporal_layers=layers)
    cfg["aggregator"]["kwargs"].update(num_modes=K, num_heads=heads)
    cfg["decoder"]["kwargs"].update(num_modes=K, future_steps=T)
    return cfg


def oracle_grid_full_grads(model, cfg, batch_cpu, d_local=None, drop=None):
    """float64 autograd over oracle/restate_grid.py: whole model under L2, or the encoder alone under sum(local * d_local);
    `drop`: a restate.PhiloxDropout for train mode (the masks the HIP kernels cut from their Philox stream)"""
    import restate
    import restate_grid
    c = restate_grid.flat_cfg(cfg)
    dt = torch.float64
    P = {k: (v.detach().cpu().to(dt) if v.is_floating_point() else v.detach().cpu().clone()) for k, v in model.state_dict().items()}
    names = [k for k in P if P[k].is_floating_point() and not k.endswith("attn_mask")]
    for k in names:
        P[k].requires_grad_(True)
    b = clone_batch(batch_cpu)
    for k in b.keys:
        if torch.is_tensor(b[k]) and b[k].is_floating_point():
            b[k] = b[k].to(dt)
    torch.set_default_dtype(dt)
    try:
        rot, y_rot = restate.rotate_inputs(b)
        with torch.enable_grad():
            local = restate_grid.local_encoder_grid(P, c, b, rot, drop)
            if d_local is not None:
                loss = (local * d_local.cpu().to(dt)).sum()
            else:
                glob = restate.global_interactor(P, c, b, rot, local, None, drop)
                out = restate_grid.mlp_decoder(P, c, b, local, glob)
                loss, _ = reference_l2(y_rot, out["loc"][..., :2], out["reg_mask"])
            loss.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return float(loss.detach()), {k: P[k].grad for k in names}


def _isolated_batch(T):
    """a scene whose lanes all lie beyond the radius and an ordinary one, then two single-actor scenes (no agent-agent edge into
    them): targets of zero in-degree in the AA, AL and global attention next to targets with edges.  The single-actor scenes come
    last: the reference numbers its fake agents by torch.unique over the agents that HAVE in-edges (ENC:90), so an agent without
    any before an agent with some would hand that agent's in-edges to another fake agent"""
    from trajsde_amd.data import collate
    from trajsde_amd.synth import synth
    far = synth(S=1, n=6, L=3, F=T, box=40.0, seed=72)
    far["lane_actor_vectors"] = far["lane_actor_vectors"] + 1000.0
    return collate([far, synth(S=1, n=7, L=4, F=T, box=50.0, seed=73), synth(S=1, n=1, L=2, F=T, box=30.0, seed=61),
                    synth(S=1, n=1, L=2, F=T, box=30.0, seed=62)])


def _cache_edge_batch(T):
    """scenes of 32, 33, 256, 257 and 1 actors: the scene-cached global attention's chunk (32) and capacity (256) edges (the
    single-actor scene last, see _isolated_batch)"""
    from trajsde_amd.data import collate
    from trajsde_amd.synth import synth
    return collate([synth(S=1, n=n, L=6, F=T, box=box, seed=90 + i, mixed_source=i % 2 == 1)
                    for i, (n, box) in enumerate(((32, 90.0), (33, 90.0), (256, 300.0), (257, 300.0), (1, 30.0)))])


def _synth(**kw):
    from trajsde_amd.synth import synth
    return synth(**kw)


def _irregular(**kw):
    from trajsde_amd.synth import irregular
    return irregular(**kw)


def _irregular_tiles_batch(T):
    """scenes of 33, 70 and 1 actors under irregular masks (synth.irregular_masks deals its five row kinds round-robin, period 5,
    over the 104 rows): every kind boundary falls on every offset of a 16-row tile (the single-actor scene last, see _isolated_batch)"""
    from trajsde_amd.data import collate
    from trajsde_amd.synth import irregular_masks, synth
    return irregular_masks(collate([synth(S=1, n=n, L=5, F=T, box=box, seed=50 + i, source=i % 2)
                                    for i, (n, box) in enumerate(((33, 90.0), (70, 130.0), (1, 30.0)))]), 77, T)


# the irregular-mask batches among TRAINED_CASES (gaps, several bos, rows unobserved at step 20 or never, ragged and empty futures)
IRREGULAR_CASES = ("irregular_k6_t20", "irregular_tiles_k6_t20")


# the batches the weights of trained_like_parameters are tested on: name -> (K, T, max_fut_t, batch maker)
TRAINED_CASES = {
    "mixed_k6_t20": (6, 20, 2.0, lambda: _synth(S=3, n=20, L=8, F=20, box=90.0, seed=9, mixed_source=True)),
    "argo_dropout_k6_t30": (6, 30, 3.0, lambda: _synth(S=3, n=24, L=10, F=30, box=100.0, seed=21, source=1, history_dropout=0.4)),
    "shipped_k10_t60": (10, 60, 6.0, lambda: _synth(S=2, n=18, L=8, F=60, box=100.0, seed=33, mixed_source=True)),
    "isolated_k6_t20": (6, 20, 2.0, lambda: _isolated_batch(20)),
    "cache_edges_k6_t20": (6, 20, 2.0, lambda: _cache_edge_batch(20)),
    # N + A = 42: no multiple of 16
    "irregular_k6_t20": (6, 20, 2.0, lambda: _irregular(S=3, n=13, L=6, F=20, box=80.0, seed=41, mixed_source=True)),
    "irregular_tiles_k6_t20": (6, 20, 2.0, lambda: _irregular_tiles_batch(20)),
}
TRAINED_STRENGTHS = (1.0, 2.0)
TRAINED_SEED = 11

# ----------------------------------------------------------------------------- backward: per-stage oracles and the comparison rule
BACKWARD_REL = 2e-4             # the backward tests' bound: of each gradient tensor's largest entry
KEY_BIAS_ABS = 5e-5             # key biases: zero in exact arithmetic, an absolute bound on both sides


class NoiseAs:
    """a restate noise source whose float32 normals are handed on in `dt` (Float64Noise for any dtype)"""

    def __init__(self, inner, dt):
        self.inner, self.dt = inner, dt

    def fake_agent(self, shape):
        return self.inner.fake_agent(shape).detach().cpu().to(self.dt)

    def encoder(self, idx, shape):
        return self.inner.encoder(idx, shape).detach().cpu().to(self.dt)

    def decoder(self, k, shape):
        return self.inner.decoder(k, shape).detach().cpu().to(self.dt)


def params_as(model, dt, prefix, device="cpu"):
    """(P in `dt` on `device`, the names under `prefix` that require grad)"""
    P = {k: (v.detach().to(device, dt) if v.is_floating_point() else v.detach().to(device).clone()) for k, v in model.state_dict().items()}
    names = [k for k in P if k.startswith(prefix) and P[k].is_floating_point() and not k.endswith("attn_mask")]
    for k in names:
        P[k].requires_grad_(True)
    return P, names


def batch_as(batch_cpu, dt, device="cpu"):
    b = clone_batch(batch_cpu).to(device)
    for k in b.keys:
        if torch.is_tensor(b[k]) and b[k].is_floating_point():
            b[k] = b[k].to(dt)
    return b


def stage_grads(P, names, prefix):
    return {k[len(prefix):]: (P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])) for k in names}


def oracle_decoder_grads(model, cfg, batch_cpu, local, glob, y_rot, seed, nll_eps=None, dt=torch.float64, device="cpu"):
    """autograd over the oracle's SDE decoder in `dt` on `device` on the given (fp32) embeddings and the fp32 Philox normals of `seed`,
    under the L2 loss (or, with `nll_eps`, the Laplace NLL) -> (loss, best mode, {decoder param: grad}, d local_embed, d global_embed)"""
    import restate
    from trajsde_amd.schedule import decoder_schedule
    c = restate.flat_cfg(cfg)
    P, names = params_as(model, dt, "decoder.", device)
    lo = local.detach().to(device, dt).requires_grad_(True)
    gl = glob.detach().to(device, dt).requires_grad_(True)
    sched = decoder_schedule(c["future_steps"], c["max_fut_t"], c["min_stepsize"])
    torch.set_default_dtype(dt)
    try:
        with torch.enable_grad():
            out = restate.sde_decoder(P, c, batch_as(batch_cpu, dt, device), lo, gl, NoiseAs(restate.PhiloxNoise(seed), dt), sched)
            yr = y_rot.detach().to(device, dt)
            if nll_eps is None:
                loss, best = reference_l2(yr, out["loc"][..., :2], out["reg_mask"])
            else:
                loss, best = reference_laplace_nll(yr, out["loc"], out["reg_mask"], nll_eps)
            loss.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return float(loss.detach()), best, stage_grads(P, names, "decoder."), lo.grad, gl.grad


def oracle_aggregator_grads(model, cfg, batch_cpu, local, d_glob, heads=8, dt=torch.float64, device="cpu"):
    """autograd over the oracle's global interactor in `dt` on `device` under sum(global_embed * d_glob)
    -> ({aggregator param: grad}, d local)"""
    import restate
    c = dict(restate.flat_cfg(cfg), num_heads=heads)
    P, names = params_as(model, dt, "aggregator.", device)
    lo = local.detach().to(device, dt).requires_grad_(True)
    b = batch_as(batch_cpu, dt, device)
    torch.set_default_dtype(dt)
    try:
        rot, _ = restate.rotate_inputs(b)
        with torch.enable_grad():
            glob = restate.global_interactor(P, c, b, rot, lo)
            (glob * d_glob.detach().to(device, dt)).sum().backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return stage_grads(P, names, "aggregator."), lo.grad


def oracle_encoder_grads(model, cfg, batch_cpu, d_local, seed, diff_weight, dt=torch.float64, device="cpu"):
    """autograd over the oracle's SDE local encoder in `dt` on `device` under sum(local_embed * d_local) + diff_weight * DiffBCE
    -> ({encoder param: grad}, DiffBCE, d aa_out)"""
    import restate
    import torch.nn.functional as F
    from trajsde_amd.schedule import encoder_schedule
    c = restate.flat_cfg(cfg)
    sched = encoder_schedule(c["historical_steps"], c["max_past_t"], c["minimum_step"])
    P, names = params_as(model, dt, "encoder.", device)
    b = batch_as(batch_cpu, dt, device)
    torch.set_default_dtype(dt)
    try:
        rot, _ = restate.rotate_inputs(b)
        with torch.enable_grad():
            local, diff_in, diff_out, inter = restate.local_encoder(P, c, b, rot, NoiseAs(restate.PhiloxNoise(seed), dt), sched, True)
            inter["aa_out"].retain_grad()
            bce = (F.binary_cross_entropy(diff_in, torch.zeros_like(diff_in)) +
                   F.binary_cross_entropy(diff_out, torch.ones_like(diff_out)))
            ((local * d_local.detach().to(device, dt)).sum() + diff_weight * bce).backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return stage_grads(P, names, "encoder."), float(bce.detach()), inter["aa_out"].grad


def deviation(a, b):
    """{name: max|a - b|} over the names of `b` (a float32 oracle's own deviation from the float64 one)"""
    return {k: (maxdiff(a[k], w) if w is not None and a.get(k) is not None else 0.0) for k, w in b.items()}


def compare_grads(tag, got, want, noise32=None, rel=BACKWARD_REL):
    """the backward tests' per-tensor rule over `got` {name: tensor} against `want` {name: float64 tensor, or None for no gradient
    path (then zero is wanted)}: err = max|got - want| <= rel * max|want| + 1e-7; key biases (zero_by_softmax_symmetry) get
    KEY_BIAS_ABS on both err and max|want|.  `noise32` {name: the float32 oracle's deviation from float64} widens a tensor's bound to
    2 x that deviation where it is larger (the ill-conditioned encoder gradients, test_encoder_backward_matches_autograd) -- nothing
    else does.  Prints the worst error relative to its tensor's max ("[trained-backward] <tag>: ...") and returns the offenders."""
    bad, worst = [], (0.0, "-", 0.0)
    for k in sorted(got):
        g = got[k].detach().cpu().double()
        w = want.get(k)
        w = torch.zeros_like(g) if w is None else w.detach().cpu().double()
        if g.shape != w.shape or not bool(torch.isfinite(g).all()):
            bad.append((k, "shape or non-finite", tuple(g.shape), tuple(w.shape)))
            continue
        scale = float(w.abs().max()) if w.numel() else 0.0
        err = float((g - w).abs().max()) if w.numel() else 0.0
        if zero_by_softmax_symmetry(k):
            if err > KEY_BIAS_ABS or scale > KEY_BIAS_ABS:
                bad.append((k, err, scale))
            continue
        n32 = float(noise32.get(k, 0.0)) if noise32 is not None else 0.0
        if err > max(rel * scale, 2 * n32) + 1e-7:
            bad.append((k, err, scale, n32))
        r = err / max(scale, 1e-7 / rel)
        if r > worst[0]:
            worst = (r, k, err)
    print(f"[trained-backward] {tag}: worst {worst[1]} {worst[0]:.2e} of its max ({worst[2]:.1e}); {len(got)} tensors, {len(bad)} over")
    return bad


# the end-to-end training-step cases at trained-like weights (tests/test_gpu_trained_backward.py, tests/test_trained_grad_profile_cpu.py)
TRAINED_STEP_CASES = ("mixed_k6_t20", "shipped_k10_t60")
TRAINED_STEP_MODES = ("eval", "dropout", "nll")
TRAINED_STEP_SEED = 31


def trained_step_case(name, mode, strength):
    """(model in eval mode on the host, cfg, batch, oracle_full_grads keyword arguments) of one end-to-end case: TRAINED_CASES[name]
    at trained_like_parameters(strength), loss weights [1, 0.5]; `mode` "eval", "dropout" (train mode with the YAML's dropout 0.1,
    masks keyed by the noise seed TRAINED_STEP_SEED) or "nll" (losses_module: [LaplaceNLLLoss, DiffBCE], eps 1e-6)"""
    import restate
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    K, T, max_t, make = TRAINED_CASES[name]
    cfg = our_cfg(K, T, max_t)
    kw = {}
    if mode == "nll":
        cfg["losses_module"] = ["LaplaceNLLLoss", "DiffBCE"]
        cfg["loss_args"] = [{"eps": 1e-6, "reduction": "mean"}, {"reduction": "mean"}]
        kw["nll_eps"] = 1e-6
    elif mode == "dropout":
        assert cfg["encoder"]["kwargs"]["dropout"] == cfg["aggregator"]["kwargs"]["dropout"] == 0.1
        kw["drop"] = restate.PhiloxDropout(TRAINED_STEP_SEED, 0.1)
    model = PredictionModelSDENet(**cfg, init_seed=2).eval()
    model.loss_weights = [1.0, 0.5]
    trained_like_parameters(model, TRAINED_SEED, strength)
    return model, cfg, make(), kw
