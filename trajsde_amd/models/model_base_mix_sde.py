"""PredictionModelSDENet -- the glue module of the hot path, MI355X build.

Mirrors the reference's `PredictionModelSDENet` (models/model_base_mix_sde.py:22-207) at the boundary:
built from the same YAML dict, stages resolved through the same {file_path, module_name, kwargs}
registry (MODEL:38-45), `forward(data) -> dict` with the same keys and the same in-place side effects
on `data` (MODEL:83-85), `validation_step/test_step` feeding the same metric formulas.  It is a
`pytorch_lightning.LightningModule` wherever that package is importable (what `pl.Trainer.fit / test` of train.py:54-66,
test.py:58 require of the model class) and a plain nn.Module in this image, where it is not and trajsde_amd.driver spells
the loops out (models/lightning_base.py); `test_epoch_end`, `only_agent` / `leave_only_agent` and the `self.log` calls
of the reference's steps are there under both.  What this model shares with the vanilla HiVT one (model_base_mix.py) -- the
constructor, the evaluation steps, the torch side of the cotangent route, `GradSet`, `resolve_class` -- is models/glue_base.py.
"""
from typing import Optional

import torch

from trajsde_amd import runtime
from trajsde_amd.models.glue_base import GlueBase, GradSet, resolve_class  # noqa: F401  (resolve_class: imported from here by the driver and tests)


class _PathLoss(torch.autograd.Function):
    """loss = sum_i w_i * loss_i over the configured {L2, DiffBCE} set as ONE autograd node whose inputs are the model
    parameters: forward runs the HIP forward and, right behind it, the three stage backward entry points of the
    C-ABI (decoder -> aggregator -> encoder); backward hands the gradients to autograd, so `loss.backward()`,
    optimizers, gradient accumulation and torch DDP hooks behave as with the reference's autograd graph."""

    @staticmethod
    def forward(ctx, model, data, noise, w_l2, w_diff, *params):
        """`w_l2`: the weight of the regression loss -- L2, or LaplaceNLLLoss when the model is configured with it"""
        with torch.no_grad():
            loss, gs = model._loss_and_gradients(data, noise, w_l2, w_diff)
            ctx.direct = model._direct_accumulation()
            ctx.sink = getattr(model, "_grad_sink", None) if ctx.direct else None
            ctx.n_inputs = len(params)
            ctx.model = model
            # the training loop's sink takes whole stage buffers: no per-parameter tensor is made for it
            ctx.gradset = gs if (isinstance(gs, GradSet) and ctx.sink is not None and hasattr(ctx.sink, "accumulate_bundles")) else None
            ctx.grads = None if ctx.gradset is not None else _PathLoss._spell_out(model, gs)
            return loss

    @staticmethod
    def _spell_out(model, gs):
        by_name = gs.by_name() if isinstance(gs, GradSet) else gs        # (a plain {name: gradient} dict is accepted too)
        return [by_name.get(n) for n in model._param_names]               # None: no path from these losses

    @staticmethod
    def backward(ctx, g):
        nothing = (None,) * (5 + ctx.n_inputs)
        if ctx.gradset is not None:
            if ctx.sink.accumulate_bundles(ctx.gradset.bundles, g):
                return nothing
            ctx.grads = _PathLoss._spell_out(ctx.model, ctx.gradset)       # (a layout the sink does not take whole)
        have = [x for x in ctx.grads if x is not None]
        if ctx.direct:
            # Leaf accumulation done here in two fused launches instead of one AccumulateGrad node (an add kernel and ~5 us of
            # host time) per parameter: `.grad += g * grad`, or `.grad = ...` where there is none yet -- what autograd's
            # accumulation would have left.  The parameters then receive no gradient THROUGH autograd, so per-parameter
            # hooks (torch DDP's reducer) do not fire: `model.direct_grad_accumulation = False` restores the plain route.
            params = [p for _, p in ctx.model.named_parameters()]
            sink = ctx.sink                                                  # driver.FlatGrads: all of it in six launches
            if sink is not None and sink.accumulate(params, ctx.grads, g):
                return nothing
            torch._foreach_mul_(have, g)                                     # our own buffers, fresh every step
            dst, src = [], []
            for p, x in zip(params, ctx.grads):
                if x is None or not p.requires_grad:
                    continue
                if p.grad is None:
                    p.grad = x
                else:
                    dst.append(p.grad)
                    src.append(x)
            if dst:
                torch._foreach_add_(dst, src)
            return nothing
        scaled = iter(torch._foreach_mul(have, g))                          # a handful of fused launches, not one per tensor
        return (None, None, None, None, None) + tuple(None if x is None else next(scaled) for x in ctx.grads)


class PredictionModelSDENet(GlueBase):
    # `cotangent_support` (model_specific.kwargs): what the cotangent route replays.  "all": every one of the K * N paths.  "winner": only
    # the one mode per actor in which dL/dloc is non-zero -- for loss sets whose losses on `loc` are winner-takes-all, e.g.
    # [L2, DiffBCE, SoftTargetCrossEntropyLoss]; check_cotangent_support() tells when a step broke that premise.  The welded sets ignore it.
    cotangent_support = "all"
    last_support_status = None

    def forward(self, data, noise: Optional["runtime.NoiseSpec"] = None, preserve_side_effects: Optional[bool] = None):
        """MODEL:74-102.  `noise` (optional, ours) selects the Philox seed or injected normals; the default
        draws a fresh Philox seed from torch's global generator, like the reference draws fresh noise.
        `preserve_side_effects=True` (or `preserve_side_effects: true` among the model / encoder kwargs of the YAML) makes
        the encoder also write `data['edge_index_{t}']`, `data['edge_attr_{t}']` (ENC:107-110); `rotate_mat` and the rotated
        `y` (MODEL:83-85) are always written."""
        if preserve_side_effects is None:
            preserve_side_effects = getattr(self, "preserve_side_effects", None)
        ood = bool(getattr(self, "ood", False))                              # test.py --ood injects this flag (test.py:45-46)
        noise = runtime.NoiseSpec.resolve(noise)
        if not self.rotate:
            raise NotImplementedError("rotate=False is not built (shipped config: rotate: true, CFG:18)")
        self._ensure_rotated(data)                                           # MODEL:76-85
        prepared = None
        if ood:
            local_embed, stds = self.encoder.forward_ood(data=data, noise=noise)            # MODEL:89-90
        else:
            # the aggregator's relative-pose embedding depends on the graph stage alone: on a side stream that the encoder call
            # forks where its recurrence starts, it shares the chip with that serial kernel (runtime.arm_rel_prefetch; eval mode only)
            rt = getattr(self.aggregator, "_rt", None)
            side = rt.arm_rel_prefetch(data, self.encoder) if (not self.training and rt is not None) else None
            local_embed, diff_in, diff_out, label_in, label_out = self.encoder(data=data, noise=noise,
                                                                               preserve_side_effects=preserve_side_effects)
            prepared = rt.launch_rel_prefetch(data, side) if side is not None else None
        global_embed = (self.aggregator(data=data, local_embed=local_embed, noise=noise, prepared=prepared) if prepared is not None
                        else self.aggregator(data=data, local_embed=local_embed, noise=noise))
        out = self.decoder(data=data, local_embed=local_embed, global_embed=global_embed, noise=noise)
        if ood:
            out["stds"] = stds                                                                 # MODEL:97-98
        else:
            out["diff_in"], out["diff_out"], out["label_in"], out["label_out"] = diff_in, diff_out, label_in, label_out
        return out

    @torch.no_grad()
    def predict_samples(self, data, n_samples: int, noise: Optional["runtime.NoiseSpec"] = None, return_samples: bool = False,
                        sample_stride: Optional[int] = None):
        """forward() with `n_samples` draws of the DECODER's noise for every (mode, actor) instead of one: graph stage, encoder and
        global interactor run once, the decoder solves all samples in one launch (SDEDecoder.sample) and reduces them on the device.
        Returns forward()'s dict -- `loc` is sample 0, bit for bit forward(data, noise)'s `loc`; `pi`, `reg_mask`, `diff_*` / `label_*`
        or `stds` as there -- plus `loc_mean` [K,N,T,4], `loc_cov` [K,N,T,3] (unbiased var_x, var_y, cov_xy) and, with `return_samples`,
        `samples` [R,K,N,T,4].  The encoder's noise is drawn once (forward_ood covers the latent side).  Eval mode only; no host
        synchronisation; `noise.seed_dev` is honoured.  `sample_stride`: runtime.StageRuntime.decoder_forward_mc."""
        from trajsde_amd import _lib
        if self.training:
            raise _lib.TrajsdeError("predict_samples is inference only: call model.eval() first")
        N = data["x"].shape[0]
        runtime.mc_check_arguments(n_samples, int(self.decoder.num_modes) * N, sample_stride)      # refused before any launch
        ood = bool(getattr(self, "ood", False))
        noise = runtime.NoiseSpec.resolve(noise)
        if not self.rotate:
            raise NotImplementedError("rotate=False is not built (shipped config: rotate: true, CFG:18)")
        runtime._require_gpu(data["x"], "the batch (predict_samples)")
        self._ensure_rotated(data)
        prepared = None
        if ood:
            local_embed, stds = self.encoder.forward_ood(data=data, noise=noise)
        else:
            rt = getattr(self.aggregator, "_rt", None)
            side = rt.arm_rel_prefetch(data, self.encoder) if rt is not None else None
            local_embed, diff_in, diff_out, label_in, label_out = self.encoder(data=data, noise=noise,
                                                                               preserve_side_effects=getattr(self, "preserve_side_effects", None))
            prepared = rt.launch_rel_prefetch(data, side) if side is not None else None
        global_embed = (self.aggregator(data=data, local_embed=local_embed, noise=noise, prepared=prepared) if prepared is not None
                        else self.aggregator(data=data, local_embed=local_embed, noise=noise))
        out = self.decoder.sample(data, local_embed, global_embed, n_samples, noise=noise, sample_stride=sample_stride,
                                  return_samples=return_samples)
        if ood:
            out["stds"] = stds
        else:
            out["diff_in"], out["diff_out"], out["label_in"], out["label_out"] = diff_in, diff_out, label_in, label_out
        return out

    @staticmethod
    def check_range() -> None:
        """raise if a launch since the last check left the fp16 range of the split-precision products (csrc/range.hpp);
        synchronises the current stream -- call it where the host waits anyway (epoch end, when a loss is read)"""
        from trajsde_amd import _lib
        _lib.check_range()

    def check_cotangent_support(self, status: Optional[torch.Tensor] = None) -> None:
        """`cotangent_support: winner` only: raise if the cotangent route's last step (or the step whose "support_status" tensor is
        handed in) met an actor whose dL/dloc was non-zero in more than one mode -- its gradients then covered the lowest such mode
        alone.  Reads two words off the device, so it synchronises: call it where the host waits anyway, like check_range()."""
        from trajsde_amd import _lib
        status = self.last_support_status if status is None else status
        if status is None:
            return
        many, some = (int(v) for v in status.tolist())
        if many:
            raise _lib.TrajsdeError(f"cotangent_support: winner -- dL/dloc of {many} actor(s) (of {some} with any) is non-zero in more "
                                    "than one mode: the loss set is not winner-takes-all on `loc`; train it with cotangent_support: all")

    def _cotangent_route(self) -> bool:
        """True when the configured loss set is not one the fused backward entry points differentiate ({L2 | LaplaceNLLLoss}
        (+ DiffBCE)): `training_step` then evaluates every loss except DiffBCE as the torch callable it is and hands dL/dloc, dL/dpi
        to trajsde_decoder_cotangent_backward.  A model without losses takes neither route."""
        if not self.loss_names:
            return False
        weights = dict(zip(self.loss_names, self.loss_weights))
        unknown = set(self.loss_names) - {"L2", "LaplaceNLLLoss", "DiffBCE"}
        return bool(unknown or self._regression_loss()[0] not in weights or ("L2" in weights and "LaplaceNLLLoss" in weights))

    def _backward_stage_ids(self):
        """under L2 / LaplaceNLLLoss the tables leave out the decoder's pi / scale heads and unused buffers-as-parameters; a loss set
        on the cotangent route reaches `decoder.scale.*` and `decoder.pi.*` too"""
        from trajsde_amd import _lib
        if self._cotangent_route():
            dec_stage = _lib.STAGE_DECODER_COT_BWD
        else:
            dec_stage = _lib.STAGE_DECODER_NLL_BWD if self._regression_loss()[0] == "LaplaceNLLLoss" else _lib.STAGE_DECODER_BWD
        return _lib.STAGE_ENCODER_BWD, _lib.STAGE_AGGREGATOR_BWD, dec_stage

    def _loss_and_gradients(self, data, noise, w_l2: float, w_diff: float):
        """the HIP forward and, right behind it, the three stage backward entry points of the C-ABI (decoder -> aggregator ->
        encoder): (weighted loss, {parameter name: gradient}).  Sets `last_output` / `last_losses` like the reference's step."""
        enc_rt, agg_rt, dec_rt = self.encoder._rt, self.aggregator._rt, self.decoder._rt
        for rt in (enc_rt, agg_rt, dec_rt):                   # no parameter changes inside this call: one stamp walk per stage
            rt.pin_stamp()
        try:
            if runtime.single_call_forms():
                self._step_pack_set().refresh()               # the six weight images of the step in one call (runtime.PackSet)
            return self._loss_and_gradients_pinned(data, noise, w_l2, w_diff)
        finally:
            for rt in (enc_rt, agg_rt, dec_rt):
                rt.unpin_stamp()

    def _step_pack_set(self) -> "runtime.PackSet":
        """forward and backward images of the three stages, as one packing call per optimizer step"""
        from trajsde_amd import _lib
        nll = self._regression_loss()[0] == "LaplaceNLLLoss"
        if getattr(self.decoder, "method", "euler") == "milstein":   # the Milstein images (the stage ids tell the two sets apart)
            dec_fwd = _lib.STAGE_DECODER_MILSTEIN
            dec_stage = _lib.STAGE_DECODER_MILSTEIN_NLL_BWD if nll else _lib.STAGE_DECODER_MILSTEIN_BWD
        else:
            dec_fwd = _lib.STAGE_DECODER
            dec_stage = _lib.STAGE_DECODER_NLL_BWD if nll else _lib.STAGE_DECODER_BWD
            if self._cotangent_route():
                dec_stage = _lib.STAGE_DECODER_COT_BWD
        ps = self.__dict__.get("_pack_set_obj")
        if ps is None or ps.entries[-1][1] != dec_stage:
            enc_rt, agg_rt, dec_rt = self.encoder._rt, self.aggregator._rt, self.decoder._rt
            ps = runtime.PackSet([(enc_rt, _lib.STAGE_ENCODER), (enc_rt, _lib.STAGE_ENCODER_BWD), (agg_rt, _lib.STAGE_AGGREGATOR),
                                  (agg_rt, _lib.STAGE_AGGREGATOR_BWD), (dec_rt, dec_fwd), (dec_rt, dec_stage)])
            self.__dict__["_pack_set_obj"] = ps
        return ps

    def _loss_and_gradients_pinned(self, data, noise, w_l2: float, w_diff: float):
        """one forward per step: the encoder and aggregator run their tape-keeping forward, the backward entry points then walk
        those tapes instead of recomputing the stage (runtime.*_forward_train).  The decoder step is the welded entry point of the
        configured regression loss, scaled by `w_l2` -- or, on the cotangent route, every configured loss except DiffBCE evaluated by
        torch on detached `loc` / `pi` leaves and dL/dloc, dL/dpi handed to the decoder's cotangent backward.  DiffBCE stays inside
        the encoder backward on both, through `diff_weight`."""
        enc_rt, agg_rt, dec_rt = self.encoder._rt, self.aggregator._rt, self.decoder._rt
        custom = self._cotangent_route()
        out, local, glob, enc_tape, agg_tape = self._forward_stages(data, noise, keep_tapes=True)
        if custom:
            values, total, d_loc, d_pi = self._torch_losses(data, out, skip=("DiffBCE",))
            dec = dec_rt.decoder_cotangent_backward(data, local, glob, out, noise, d_loc, d_pi, support=self.cotangent_support)
            self.last_support_status = dec.get("support_status")
            w_dec = 1.0                                       # (the loss weights are inside dL/dloc and dL/dpi)
        else:
            reg, eps = self._regression_loss()
            if reg == "LaplaceNLLLoss":
                dec = dec_rt.decoder_nll_backward(data, local, glob, out, noise, eps=eps)
            else:
                dec = dec_rt.decoder_l2_backward(data, local, glob, out, noise)
            w_dec = w_l2
        d_glob, d_local = dec["d_global_embed"], dec["d_local_embed"]
        if w_dec != 1.0:
            d_glob, d_local = d_glob * w_dec, d_local * w_dec
        agg = agg_rt.aggregator_backward(data, local, d_glob, noise, tape=agg_tape)
        del agg_tape
        gs = GradSet()
        gs.add("decoder.", dec["grads"], w_dec)
        gs.add("aggregator.", agg["grads"])
        self._early_reduce(gs)
        enc = enc_rt.encoder_backward(data, d_local + agg["d_local_embed"], noise, diff_weight=w_diff, tape=enc_tape)
        del enc_tape
        gs.add("encoder.", enc["grads"])
        self.last_output = out
        diff = enc["diff_loss"].detach() / w_diff if w_diff else None
        if custom:
            self.last_losses = dict(values)
            if "DiffBCE" in self.loss_names:
                self.last_losses["DiffBCE"] = diff
            value = enc["diff_loss"] if total is None else total.detach() + enc["diff_loss"]
        else:
            self.last_losses = {reg: dec["loss"].detach(), "DiffBCE": diff}
            value = w_l2 * dec["loss"] + enc["diff_loss"]
        return value.clone(), gs

    def _early_reduce(self, gs: GradSet) -> None:
        """multi-rank training loop (driver.train): the decoder's and aggregator's gradients are final -- their slice of the flat
        gradient buffer goes to the all-reduce now, on the collective stream, under the encoder backward (driver.FlatGrads)"""
        sink = getattr(self, "_grad_sink", None)
        if sink is not None and getattr(sink, "early_enabled", False) and self._direct_accumulation():
            if not (hasattr(sink, "early_reduce_bundles") and sink.early_reduce_bundles(gs.bundles)):
                early = gs.by_name()                                         # (a sink without the whole-buffer entry points)
                named = dict(self.named_parameters())
                sink.early_reduce([named[n] for n in early], [early[n] for n in early])

    def prefetch_graph(self, data, noise: "runtime.NoiseSpec", main_stream=None) -> None:
        """prepare `data` for the training_step that will follow with the same `noise`: rotation + graph stage on the side stream
        (runtime.prefetch_graph; driver.train calls it for batch i + 1 right after it has enqueued step i)"""
        enc = self.encoder
        runtime.prefetch_graph(data, float(enc.local_radius), int(enc.historical_steps), runtime.NoiseSpec.resolve(noise),
                               main_stream=main_stream)

    def _forward_stages(self, data, noise, keep_tapes: bool = False):
        """forward() that also hands back the two stage boundaries the backward entry points need; with `keep_tapes` the
        encoder and the aggregator run their tape-keeping forward and the tapes are returned too"""
        self._ensure_rotated(data)
        enc_tape = agg_tape = None
        if keep_tapes:
            (local_embed, diff_in, diff_out, label_in, label_out), enc_tape = self.encoder._rt.encoder_forward_train(data, noise)
            global_embed, agg_tape = self.aggregator._rt.aggregator_forward_train(data, local_embed, noise)
        else:
            local_embed, diff_in, diff_out, label_in, label_out = self.encoder(data=data, noise=noise)
            global_embed = self.aggregator(data=data, local_embed=local_embed, noise=noise)
        out = self.decoder(data=data, local_embed=local_embed, global_embed=global_embed, noise=noise)
        out["diff_in"], out["diff_out"], out["label_in"], out["label_out"] = diff_in, diff_out, label_in, label_out
        if keep_tapes:
            return out, local_embed, global_embed, enc_tape, agg_tape
        return out, local_embed, global_embed

    # -- Lightning-style hooks (MODEL:104-148) ------------------------------------------------------
    def training_step(self, data, batch_idx, noise: Optional["runtime.NoiseSpec"] = None):
        """MODEL:104-116: forward, the weighted sum of the configured losses, as a tensor whose `.backward()` fills
        `.grad` through the HIP backward kernels.  In train mode (`model.train()`) the stages' `dropout` is applied at the
        reference's sites (attention weights, out_proj output, the two FFN activations of every attention block) with masks
        cut from the Philox stream of `noise` (csrc/dropout.hpp); `model.eval()` switches it off, as in the reference.  The kernels fuse the
        shipped loss set (losses/L2.py + losses/diff_BCE.py, CFG:78-83) and losses/laplace_nll_loss.py in place of L2 into the decoder
        backward.  Any other loss set -- further `loss(data, output)` callables on `loc` / `pi`, or L2 together with LaplaceNLLLoss --
        takes the cotangent route: the losses (DiffBCE apart) are evaluated by torch on the forward's `loc` and `pi`, and their
        gradients dL/dloc, dL/dpi go through the HIP backward of all K modes (trajsde_decoder_cotangent_backward), which trains the
        `pi` and `scale` heads as well -- or, with `cotangent_support: winner`, of each actor's one supported mode (and `pi` over all K).  A decoder with `method: milstein` trains under the fused sets (its reverse sweep differentiates
        the gdg term: trajsde_decoder_*_backward_milstein), on the GPU only; the cotangent route is Euler-only."""
        custom = self._cotangent_route()
        if custom and self.cotangent_support not in ("all", "winner"):
            raise ValueError(f"cotangent_support {self.cotangent_support!r}: 'all' or 'winner'")
        if custom and getattr(self.decoder, "method", "euler") == "milstein":
            raise NotImplementedError("`method: milstein` trains under L2 or LaplaceNLLLoss (+ DiffBCE) only: the cotangent route that "
                                      f"differentiates {self.loss_names} is built for the Euler-Maruyama solve")
        runtime.refuse_milstein_training(self.decoder)
        if not self.rotate:
            raise NotImplementedError("rotate=False is not built (shipped config: rotate: true, CFG:18)")
        if not getattr(self.decoder, "uncertain", True):
            # losses/L2.py:12 and losses/laplace_nll_loss.py:28 take `loc, scale = output['loc'].chunk(2, dim=-1)`: on the
            # two-channel output of `uncertain: False` that makes `loc` the x coordinate alone, broadcast against BOTH target
            # coordinates -- the reference's losses are only meaningful with the scale head.  Inference is supported.
            raise NotImplementedError("training with `uncertain: False` is not built: the reference's own losses chunk loc | scale out of "
                                      "FOUR channels (losses/L2.py:12); on the two-channel output they regress x against both targets")
        weights = dict(zip(self.loss_names, self.loss_weights))
        reg_name = self._regression_loss()[0]
        if not self.loss_names:
            raise NotImplementedError("training_step needs a configured loss set (`losses` / `losses_module` / `loss_weights`)")
        if custom:                                           # (refused before the batch is touched where the kernels cannot run)
            runtime._require_gpu(next(self.parameters()), "model parameters (training_step)")
        if data.y is None:
            raise ValueError("training_step needs targets (data.y)")
        noise = runtime.NoiseSpec.resolve(noise)
        if not hasattr(self, "_param_names"):
            self._param_names = [n for n, _ in self.named_parameters()]
        direct = self._direct_accumulation()
        # (named_parameters() walks the ~270 modules of the tree: once per step on the autograd route, not at all on the direct one,
        #  whose single input is looked up once)
        one = self.__dict__.get("_one_param")               # (kept out of nn.Module's parameter registry: plain instance dict)
        if direct and one is not None and one.requires_grad:
            params = [one]
        else:
            params = [p for _, p in self.named_parameters()]
        if direct:
            # the gradients do not travel through autograd (`.grad` is written directly): ONE parameter as the node's input is
            # enough to make the loss differentiable, and 250 fewer inputs are 250 fewer edges for the engine to walk every step
            params = [p for p in params if p.requires_grad][:1]
            self.__dict__["_one_param"] = params[0] if params else None
        loss = _PathLoss.apply(self, data, noise, 1.0 if custom else float(weights[reg_name]), float(weights.get("DiffBCE", 0.0)), *params)
        self._log_training_step()
        return loss

    def _validation_trajectories(self, y_hat, y):
        if not self.is_gtabs:                                                 # MODEL:125-127: displacements -> positions
            y_hat, y = torch.cumsum(y_hat, dim=-2), torch.cumsum(y, dim=-2)
        return y_hat, y

    def configure_optimizers(self):
        """AdamW + per-epoch cosine annealing (MODEL:204-207)."""
        self.optimizer = torch.optim.AdamW(self.parameters(), lr=self.lr, weight_decay=self.weight_decay)
        self.scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(self.optimizer, T_max=self.T_max, eta_min=0.0)
        return [self.optimizer], [self.scheduler]
