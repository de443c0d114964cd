"""The stages of the SDE model and of the vanilla HiVT variant as torch.autograd nodes (`autograd: true` among a stage's kwargs).

A stage's `forward` normally runs the inference kernels and returns tensors without a `grad_fn`; training then needs the model-level
`training_step` (models/model_base_mix_sde.py), one node over the three HIP backward entry points.  With the switch on, a stage whose
parameters or tensor inputs require grad (and while grad mode is enabled) goes through ONE node of its own instead:

    encoder      encoder_forward_train       / trajsde_encoder_cotangent_backward   (cotangents of local_embed, diff_in, diff_out)
    aggregator   aggregator_forward_train    / trajsde_aggregator_backward_heads    (cotangent of global_embed -> d local_embed)
    decoder      decoder_forward             / trajsde_decoder_cotangent_backward(_sel)  (cotangents of loc, pi -> d local / d global)

and, in the vanilla HiVT variant (LocalEncoder / GlobalInteractor / MLPDecoder; the aggregator's node is the one above, at 4 heads),

    encoder      encoder_grid_forward on the exact graph / trajsde_encoder_grid_backward_train   (cotangent of local_embed)
    decoder      mlp_decoder_forward         / trajsde_mlp_decoder_cotangent_backward    (cotangents of loc, pi -> d local / d global)

so a glue module other than ours -- the reference's own PredictionModelSDENet or PredictionModel with three `file_path` strings pointed
here -- trains under any torch loss on any of the outputs.  A node's inputs are the stage's tensor inputs and its parameters in named_parameters()
order; its backward returns one gradient per parameter, None where the stage's *_BWD table does not name it.  The noise (and the
dropout key in train mode) is resolved once in forward and replayed by backward; tapes live on the node and are released by backward.
Every other case -- the switch off, no_grad / inference_mode, nothing requiring grad -- takes the inference path untouched.

This module is imported the ordinary way and therefore once, unlike the stage files (models/glue_base.py resolve_class)."""
from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from trajsde_amd import _lib, runtime


def check_decoder(module) -> None:
    """what `autograd: true` asks of the decoder's configuration: the cotangent backward is built for the Euler-Maruyama solve and the
    four-channel output"""
    if not getattr(module, "autograd", False):
        return
    if getattr(module, "method", "euler") == "milstein":
        raise NotImplementedError("`autograd: true` with `method: milstein`: the stage's autograd node differentiates through the "
                                  "Euler-only cotangent route (trajsde_decoder_cotangent_backward); a Milstein decoder trains through the "
                                  "model-level training_step under L2 or LaplaceNLLLoss (+ DiffBCE)")
    if not getattr(module, "uncertain", True):
        raise NotImplementedError("`autograd: true` with `uncertain: False` is not built: the reference's own losses chunk loc | scale out "
                                  "of FOUR channels (losses/L2.py:12), so training needs the scale head; inference is supported")
    if getattr(module, "cotangent_support", "all") not in ("all", "winner"):
        raise ValueError(f"cotangent_support {module.cotangent_support!r}: 'all' or 'winner'")


def active(module, *tensors) -> bool:
    """True when this forward of `module` goes through the stage's autograd node"""
    if not getattr(module, "autograd", False) or not torch.is_grad_enabled():
        return False
    if any(t is not None and t.requires_grad for t in tensors):
        return True
    return any(p.requires_grad for p in module.parameters())


def _params(module):
    """(names, tensors) of the node's parameter inputs: named_parameters() order; refused where the kernels cannot run"""
    names, params = zip(*module.named_parameters())
    runtime._require_gpu(params[0], f"{module._rt.stage} parameters (autograd: true)")
    return list(names), list(params)


def _begin(ctx, module, data, noise, names, n_tensor_inputs: int) -> None:
    ctx.set_materialize_grads(False)
    ctx.module, ctx.data, ctx.noise, ctx.names = module, data, noise, names
    ctx.training = bool(module.training)
    ctx.n_front = 4 + n_tensor_inputs                   # module, data, noise, names, then the tensor inputs, then the parameters


def _replay_guard(ctx) -> None:
    if bool(ctx.module.training) != ctx.training:
        raise _lib.TrajsdeError(f"the {ctx.module._rt.stage} stage was switched between train() and eval() after its forward: the backward "
                                "replays the forward's dropout masks and cannot under the other mode")


def _param_grads(ctx, grads):
    """one gradient per parameter input; None: not in the stage's backward table, or the parameter does not require grad"""
    need = ctx.needs_input_grad[ctx.n_front:]
    return tuple(grads[n] if (w and n in grads) else None for n, w in zip(ctx.names, need))


class EncoderNode(torch.autograd.Function):
    """LocalEncoderSDESepPara2.forward -> (local_embed, diff_in, diff_out, label_in, label_out); the labels are constants"""

    @staticmethod
    def forward(ctx, module, data, noise, names, *params):
        _begin(ctx, module, data, noise, names, 0)
        outs, ctx.tape = module._rt.encoder_forward_train(data, noise)
        ctx.save_for_backward(*params)
        ctx.mark_non_differentiable(outs[3], outs[4])
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, d_local, d_diff_in, d_diff_out, _d_label_in, _d_label_out):
        ctx.saved_tensors                                # torch's version check: a parameter updated in place since the forward raises here
        _replay_guard(ctx)
        tape, ctx.tape = ctx.tape, None                  # a second backward over a retained graph recomputes the forward (tape=None)
        res = ctx.module._rt.encoder_cotangent_backward(ctx.data, d_local, d_diff_in, d_diff_out, ctx.noise, tape=tape)
        del tape
        return (None, None, None, None) + _param_grads(ctx, res["grads"])


class AggregatorNode(torch.autograd.Function):
    """GlobalInteractor.forward: local_embed [N,64] -> global_embed [K,N,64]"""

    @staticmethod
    def forward(ctx, module, data, noise, names, local_embed, *params):
        _begin(ctx, module, data, noise, names, 1)
        out, ctx.tape = module._rt.aggregator_forward_train(data, local_embed, noise)
        ctx.save_for_backward(local_embed, *params)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, d_global):
        local_embed = ctx.saved_tensors[0]
        _replay_guard(ctx)
        tape, ctx.tape = ctx.tape, None
        res = ctx.module._rt.aggregator_backward(ctx.data, local_embed, d_global, ctx.noise, tape=tape)
        del tape
        d_local = res["d_local_embed"] if ctx.needs_input_grad[4] else None
        return (None, None, None, None, d_local) + _param_grads(ctx, res["grads"])


class DecoderNode(torch.autograd.Function):
    """SDEDecoder.forward: (local_embed, global_embed) -> (loc [K,N,T,4], pi [N,K], reg_mask); Euler-Maruyama, all K modes or
    (`cotangent_support: winner`) each actor's one supported mode"""

    @staticmethod
    def forward(ctx, module, data, noise, names, local_embed, global_embed, *params):
        _begin(ctx, module, data, noise, names, 2)
        out = module._rt.decoder_forward(data, local_embed, global_embed, noise)
        ctx.save_for_backward(local_embed, global_embed, out["loc"], *params)
        ctx.mark_non_differentiable(out["reg_mask"])
        return out["loc"], out["pi"], out["reg_mask"]

    @staticmethod
    @once_differentiable
    def backward(ctx, d_loc, d_pi, _d_mask):
        local_embed, global_embed, loc = ctx.saved_tensors[:3]
        m = ctx.module
        res = m._rt.decoder_cotangent_backward(ctx.data, local_embed, global_embed, {"loc": loc}, ctx.noise, d_loc, d_pi,
                                               support=getattr(m, "cotangent_support", "all"))
        if "support_status" in res:
            m.last_support_status = res["support_status"]
        need = ctx.needs_input_grad
        return (None, None, None, None, res["d_local_embed"] if need[4] else None, res["d_global_embed"] if need[5] else None) \
            + _param_grads(ctx, res["grads"])


class GridEncoderNode(torch.autograd.Function):
    """the vanilla LocalEncoder.forward -> local_embed [N,64]; no tape: the backward entry point recomputes the forward under the
    node's dropout key"""

    @staticmethod
    def forward(ctx, module, data, noise, names, *params):
        _begin(ctx, module, data, noise, names, 0)
        local = module._rt.encoder_grid_forward(data, noise, exact=True)
        ctx.save_for_backward(*params)
        return local

    @staticmethod
    @once_differentiable
    def backward(ctx, d_local):
        ctx.saved_tensors                                # torch's version check (see EncoderNode)
        _replay_guard(ctx)
        res = ctx.module._rt.encoder_grid_backward(ctx.data, d_local, ctx.noise)
        return (None, None, None, None) + _param_grads(ctx, res["grads"])


class MLPDecoderNode(torch.autograd.Function):
    """MLPDecoder.forward: (local_embed, global_embed) -> (loc [K,N,T,4], pi [N,K], reg_mask); all K modes and the pi head"""

    @staticmethod
    def forward(ctx, module, data, noise, names, local_embed, global_embed, *params):
        _begin(ctx, module, data, noise, names, 2)
        out = module._rt.mlp_decoder_forward(data, local_embed, global_embed)
        ctx.save_for_backward(local_embed, global_embed, out["loc"], *params)
        ctx.mark_non_differentiable(out["reg_mask"])
        return out["loc"], out["pi"], out["reg_mask"]

    @staticmethod
    @once_differentiable
    def backward(ctx, d_loc, d_pi, _d_mask):
        local_embed, global_embed, loc = ctx.saved_tensors[:3]
        res = ctx.module._rt.mlp_decoder_cotangent_backward(ctx.data, local_embed, global_embed, {"loc": loc}, d_loc, d_pi)
        need = ctx.needs_input_grad
        return (None, None, None, None, res["d_local_embed"] if need[4] else None, res["d_global_embed"] if need[5] else None) \
            + _param_grads(ctx, res["grads"])


def _enter(module, noise: Optional["runtime.NoiseSpec"]):
    names, params = _params(module)
    return runtime.NoiseSpec.resolve(noise), names, params


def encoder(module, data, noise=None, preserve_side_effects: bool = False):
    noise, names, params = _enter(module, noise)
    outs = EncoderNode.apply(module, data, noise, names, *params)
    if preserve_side_effects:
        runtime.edge_snapshots(data, int(module.historical_steps))                          # ENC:107-110
    return outs


def aggregator(module, data, local_embed, noise=None, prepared=None):
    if prepared is not None:
        prepared.join()                                  # (the training forward embeds the relative poses itself: the prefetched rows are dropped)
    noise, names, params = _enter(module, noise)
    runtime._require_gpu(local_embed, "local_embed")
    return AggregatorNode.apply(module, data, noise, names, local_embed, *params)


def decoder(module, data, local_embed, global_embed, noise=None):
    check_decoder(module)
    noise, names, params = _enter(module, noise)
    runtime._require_gpu(local_embed, "local_embed")
    runtime._require_gpu(global_embed, "global_embed")
    loc, pi, reg_mask = DecoderNode.apply(module, data, noise, names, local_embed, global_embed, *params)
    return {"loc": loc, "pi": pi, "reg_mask": reg_mask}


def encoder_grid(module, data, noise=None):
    noise, names, params = _enter(module, noise)
    return GridEncoderNode.apply(module, data, noise, names, *params)


def decoder_mlp(module, data, local_embed, global_embed):
    """the dict of MLPDecoder.forward (dec_hivt_nusargo_grid.py:56-57: the embeddings ride along, here with their own history)"""
    check_decoder(module)
    names, params = _params(module)                                     # (the stage draws nothing: no key to resolve)
    runtime._require_gpu(local_embed, "local_embed")
    runtime._require_gpu(global_embed, "global_embed")
    loc, pi, reg_mask = MLPDecoderNode.apply(module, data, None, names, local_embed, global_embed, *params)
    return {"loc": loc, "pi": pi, "reg_mask": reg_mask, "local_embed": local_embed, "global_embed": global_embed}
