"""Float64 restatement of the Milstein decoder for autograd -- the gradient oracle of the Milstein backward
(trajsde_decoder_l2_backward_milstein / _nll_backward_milstein, csrc/decoder_mil_bwd.hip).

tests/milstein_restate.py restates torchsde's MilsteinIto.step for the forward and takes the gdg vjp on a DETACHED y: it cannot be
differentiated.  The reference trains through it: for diagonal noise torchsde's g_prod_and_gdg_prod_diagonal (SDEINT:588-601) is

    y = y if y.requires_grad else y.detach().requires_grad_(True)
    g = sde.g(t, y)
    vjp(outputs=g, inputs=y, grad_outputs=g * v2, create_graph=requires_grad)

so the gradient goes through gdg, including its leading g (second derivatives of GFunc).  That is restated literally below; the rest
of the decoder (time bookkeeping, noise rows, output interpolation, heads, reg_mask) is oracle/restate.sde_decoder's.

`closed_form_step_vjp` restates the reverse sweep's closed form for the gdg term (decoder_mil_bwd.hip k_sde_bwd_mil) in float64, so
that the CPU suite checks it against autograd before any kernel runs.
"""
import contextlib

import torch
import torch.nn.functional as F

import restate

D = 64

# the stage cases of the Milstein backward's tests: test_gpu_trained_backward.py's DEC_SHAPES, at the initial weights (strength 0:
# trained_like_parameters not applied) and the trained-like strengths
DEC_SHAPES = [(3, 20, 4, 20, 2.0, dict(mixed_source=True, history_dropout=0.3)),
              (2, 13, 3, 30, 3.0, dict(source=1)),            # T=30: the solver's extra micro-step, outputs interpolated
              (2, 9, 1, 5, 0.5, dict(nus_sparsity=True))]     # a single mode, ragged masks
STRENGTHS = (0.0, 1.0, 2.0)


def gdg_graph(P, pre, y, sn, cs, v2):
    """(g, gdg) of torchsde's diagonal-noise step with the vjp kept in the graph: g = diffusion(y).repeat(1, 64) (DEC:194),
    gdg = vjp(g, y, g * v2) with create_graph"""
    with torch.enable_grad():
        y = y if y.requires_grad else y.detach().requires_grad_(True)
        g = restate.diffusion(P, pre, y, sn, cs).repeat(1, D)
        (gdg,) = torch.autograd.grad(outputs=g, inputs=y, grad_outputs=g * v2, create_graph=True)
    return g, gdg


def sde_decoder(P, cfg, batch, local_embed, global_embed, noise, dec_sched, pre="decoder.", method="milstein", gdg_detached=False):
    """milstein_restate.sde_decoder with y kept in the graph (method="euler": the Euler step of restate.sde_decoder); the output dict
    carries reg_mask when `batch` is given.  `gdg_detached`: the same forward values with the gdg term cut from the graph -- what a
    backward that ignored the second-order term computes (the discrimination checks)"""
    dt_ = next(v for v in P.values() if v.is_floating_point()).dtype
    K, T = cfg["num_modes"], cfg["future_steps"]
    N = local_embed.shape[0]
    loc_exp = local_embed.expand(K, N, D)
    y = F.relu(restate._ln(P, pre + "aggr_embed.1", restate._lin(P, pre + "aggr_embed.0", torch.cat((global_embed, loc_exp), -1))))
    y = y.reshape(K * N, D)
    lf = pre + "lsde_func"
    sol, o = [], 0
    for k in range(dec_sched.n_euler):
        s_t, c_t = float(dec_sched.sin_t0[k]), float(dec_sched.cos_t0[k])
        dt = float(dec_sched.dt[k])
        f = restate.drift(P, lf + ".f_func", y, s_t, c_t)
        I = noise.decoder(k, (K * N, D)).to(dt_) * float(dec_sched.sqrt_h[k])
        prev = y
        if method == "milstein":
            g, gdg = gdg_graph(P, lf + ".g_func", y, s_t, c_t, 0.5 * (I ** 2 - dt))     # MilsteinIto.v_term
            y = y + f * dt + g * I + (gdg.detach() if gdg_detached else gdg)
        else:
            y = y + f * dt + restate.diffusion(P, lf + ".g_func", y, s_t, c_t).repeat(1, D) * I
        while o < dec_sched.n_out and dec_sched.out_step[o] == k + 1:
            sol.append(float(dec_sched.out_w0[o]) * prev + float(dec_sched.out_w1[o]) * y)
            o += 1
    sol = torch.stack(sol).permute(1, 0, 2)                                     # [K*N, T, 64]
    pi = restate._lin(P, pre + "pi.3", F.relu(restate._ln(P, pre + "pi.1", restate._lin(P, pre + "pi.0", torch.cat((loc_exp, global_embed), -1)))))
    pi = pi.squeeze(-1).t()
    loc = restate._lin(P, pre + "decoder.3", F.relu(restate._ln(P, pre + "decoder.1", restate._lin(P, pre + "decoder.0", sol))))
    if pre + "scale.0.weight" in P:
        sc = restate._lin(P, pre + "scale.3", F.relu(restate._ln(P, pre + "scale.1", restate._lin(P, pre + "scale.0", sol))))
        sc = F.elu(sc, alpha=1.0) + 1.0 + cfg["min_scale"]
        loc = torch.cat((loc.view(K, N, T, 2), sc.view(K, N, T, 2)), -1)
    else:
        loc = loc.view(K, N, T, 2)
    out = {"loc": loc, "pi": pi}
    if batch is not None:
        out["reg_mask"] = ~batch["padding_mask"][:, -T:]
    return out


@contextlib.contextmanager
def decoder_as(**kw):
    """oracle/restate.sde_decoder replaced by the restatement above (keyword arguments: method, gdg_detached) while the block runs:
    the oracles of tests/helpers.py then differentiate the Milstein decoder"""
    orig = restate.sde_decoder

    def dec(P, cfg, batch, local_embed, global_embed, noise, dec_sched, want_intermediates=False):
        return sde_decoder(P, cfg, batch, local_embed, global_embed, noise, dec_sched, **kw)
    restate.sde_decoder = dec
    try:
        yield
    finally:
        restate.sde_decoder = orig


def oracle_decoder_grads(*args, method="milstein", gdg_detached=False, **kw):
    """helpers.oracle_decoder_grads over the Milstein decoder -> (loss, best mode, {decoder param: grad}, d local, d global)"""
    import helpers as H
    with decoder_as(method=method, gdg_detached=gdg_detached):
        return H.oracle_decoder_grads(*args, **kw)


def oracle_full_grads(*args, **kw):
    """helpers.oracle_full_grads (encoder -> aggregator -> Milstein decoder -> losses) -> (loss, {param: grad})"""
    import helpers as H
    with decoder_as(method="milstein"):
        return H.oracle_full_grads(*args, **kw)


def closed_form_step_vjp(P, pre, y, u, I, dt, sn, cs):
    """the gdg term's part of one step's vjp with the adjoint u, as the reverse sweep forms it: the gradient of
    Psi = c s (u . ds/dy) = c s^2 (1 - s) p' with c = sum_i 0.5 (I_i^2 - dt) per row and u held fixed ->
    {"y": dPsi/dy, "net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias"}, summed over rows"""
    W0, b0 = P[pre + ".net.0.weight"], P[pre + ".net.0.bias"]
    W2, b2 = P[pre + ".net.2.weight"], P[pre + ".net.2.bias"]
    w4, b4 = P[pre + ".net.4.weight"][0], P[pre + ".net.4.bias"]
    x = restate.sde_time_mlp_in(y, sn, cs)
    h1 = torch.tanh(x @ W0.t() + b0)
    h2 = torch.tanh(h1 @ W2.t() + b2)
    s = torch.sigmoid(h2 @ w4 + b4)                                       # [rows]
    c = 0.5 * (I ** 2 - dt).sum(1)
    W0y = W0[:, :D]
    a1 = u @ W0y.t()                                                      # the tangent pass along u
    h1t = (1 - h1 ** 2) * a1
    a2 = h1t @ W2.t()
    h2t = (1 - h2 ** 2) * a2
    pd = h2t @ w4
    alpha = c * s ** 2 * (1 - s)
    beta = c * pd * s * (1 - s) * (2 * s - 3 * s ** 2)
    g2b = alpha[:, None] * w4 * (1 - h2 ** 2)
    d2 = (beta[:, None] * w4 - 2 * alpha[:, None] * w4 * h2 * a2) * (1 - h2 ** 2)
    h1b = g2b @ W2
    d1 = (d2 @ W2 - 2 * h1b * h1 * a1) * (1 - h1 ** 2)
    g1b = h1b * (1 - h1 ** 2)
    dW0 = d1.t() @ x
    dW0[:, :D] += g1b.t() @ u
    return {"y": d1 @ W0y,
            "net.0.weight": dW0, "net.0.bias": d1.sum(0),
            "net.2.weight": d2.t() @ h1 + g2b.t() @ h1t, "net.2.bias": d2.sum(0),
            "net.4.weight": (beta[:, None] * h2 + alpha[:, None] * h2t).sum(0, keepdim=True), "net.4.bias": beta.sum(0, keepdim=True)}
