"""What PredictionModelSDENet (model_base_mix_sde.py) and PredictionModel (model_base_mix.py) share above the C-ABI: the constructor
(the YAML's {file_path, module_name, kwargs} registry of stages, losses and metrics, MODEL:28-72), the evaluation steps, the rotation
of a batch that nobody rotated ahead of time, the torch-side half of the cotangent route, and the bookkeeping of a training step.

This module is imported the ordinary way and therefore exactly once, unlike the stage and model files, which `resolve_class` also
loads under their class name: `GradSet` is one class however the model file that fills it was loaded."""
import os
from copy import deepcopy
from importlib.machinery import SourceFileLoader
from typing import Optional

import torch

from trajsde_amd import runtime
from trajsde_amd.models.lightning_base import LightningHooks

_REPO_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def resolve_class(file_path: str, module_name: str):
    """The reference's registry: getattr(SourceFileLoader(name, path).load_module(name), name)."""
    path = file_path if os.path.isfile(file_path) else os.path.join(_REPO_ROOT, file_path)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"stage file '{file_path}' not found (cwd or {_REPO_ROOT})")
    return getattr(SourceFileLoader(module_name, path).load_module(module_name), module_name)


class GradSet:
    """the three stages' gradient buffers of one training step: (name prefix, runtime.GradBuffers, multiplier) each.  The training
    loop's sink takes them whole (driver.FlatGrads.accumulate_bundles); `by_name()` spells them out per parameter for everyone else."""

    def __init__(self) -> None:
        self.bundles = []

    def add(self, prefix: str, grads, mult: float = 1.0) -> None:
        self.bundles.append((prefix, grads, float(mult)))

    def by_name(self) -> dict:
        out = {}
        for prefix, grads, mult in self.bundles:
            for n, g in grads.items():
                out[prefix + n] = g if mult == 1.0 else g * mult
        return out


class GlueBase(LightningHooks):
    """base of the two glue modules; a subclass supplies forward, training_step, configure_optimizers and `_backward_stage_ids`"""

    def __init__(self, **kwargs) -> None:
        super().__init__()
        self._record_hparams(kwargs)                                      # MODEL:28 save_hyperparameters()
        init_seed: Optional[int] = kwargs.get("init_seed")
        for key, value in kwargs.items():
            if key == "training_specific":
                for k, v in value.items():
                    setattr(self, k, v)
            elif key == "model_specific":
                for k, v in value["kwargs"].items():
                    setattr(self, k, v)

        def build(section, offset):
            args = kwargs[section]
            kw = dict(args["kwargs"])
            if init_seed is not None:
                kw["init_seed"] = init_seed + offset
            return resolve_class(args["file_path"], args["module_name"])(**kw)

        self.encoder = build("encoder", 1)
        self.aggregator = build("aggregator", 2)
        self.decoder = build("decoder", 3)

        self.losses, self.loss_names = [], []
        for i, path in enumerate(kwargs.get("losses", [])):
            name = kwargs["losses_module"][i]
            self.losses.append(resolve_class(path, name)(**dict(kwargs["loss_args"][i])))
            self.loss_names.append(name)
        self.loss_weights = kwargs.get("loss_weights", [])
        self.metrics_tr, self.metrics_vl, self.metric_names = [], [], []
        for i, path in enumerate(kwargs.get("metrics", [])):
            name = kwargs["metrics_module"][i]
            metric = resolve_class(path, name)(**dict(kwargs["metric_args"][i]))
            self.metrics_tr.append(metric)
            self.metrics_vl.append(deepcopy(metric))
            self.metric_names.append(name)

    @property
    def device(self) -> torch.device:
        return next(self.parameters()).device

    def _ensure_rotated(self, data) -> None:
        """MODEL:76-85: `rotate_mat` and the rotated `y` written onto the batch, unless prefetch_graph did it ahead of time"""
        if not runtime.consume_rotation(data):
            rotate_mat, y_rot = runtime.rotate_inputs(data)
            if y_rot is not None:
                data.y = y_rot
            data["rotate_mat"] = rotate_mat

    # -- training ------------------------------------------------------------------------------------
    def _regression_loss(self):
        """(name, eps) of the configured regression loss: "L2" (losses/L2.py, the shipped one) or "LaplaceNLLLoss"
        (losses/laplace_nll_loss.py: the scale head is trained as well)"""
        for name, fn in zip(self.loss_names, self.losses):
            if name == "LaplaceNLLLoss":
                return name, float(getattr(fn, "eps", 1e-6))
        return "L2", None

    def _torch_losses(self, data, out, skip=()):
        """the torch side of the cotangent route: every configured loss not named in `skip`, evaluated as the `loss(data, output)`
        callable it is on detached `loc` / `pi` leaves -> ({name: value}, weighted sum, dL/dloc, dL/dpi).  The sum is None when
        nothing is left to evaluate; a gradient is None where the sum does not depend on that leaf."""
        loc = out["loc"].detach().requires_grad_(True)
        pi = out["pi"].detach().requires_grad_(True)
        view = dict(out)
        view["loc"], view["pi"] = loc, pi
        values, total = {}, None
        d_loc = d_pi = None
        with torch.enable_grad():
            for name, fn, w in zip(self.loss_names, self.losses, self.loss_weights):
                if name in skip:
                    continue
                v = fn(data, view)
                values[name] = v.detach()
                total = v * float(w) if total is None else total + v * float(w)
            if total is not None and total.requires_grad:
                d_loc, d_pi = torch.autograd.grad(total, [loc, pi], allow_unused=True)
        return values, total, d_loc, d_pi

    def _backward_stage_ids(self):
        """(encoder, aggregator, decoder) stage ids of the backward entry points the configured loss set takes"""
        raise NotImplementedError

    def params_with_gradient(self):
        """the parameters the configured losses reach: those of the three backward stages' parameter tables.  The reference's
        autograd leaves the others' `.grad` at None, so AdamW skips them."""
        reached = set()
        for stage, sid in zip(("encoder", "aggregator", "decoder"), self._backward_stage_ids()):
            reached |= {f"{stage}.{n}" for n in getattr(self, stage)._rt.param_names(sid)}
        return [p for n, p in self.named_parameters() if n in reached]

    def _log_training_step(self) -> None:
        """MODEL:112-113: one `train/<name>` entry per configured loss that the step evaluated, and the learning rate"""
        n_rows = int(self.last_output["loc"].size(1))
        for name in self.loss_names:
            if self.last_losses.get(name) is not None:
                self.log_value(f"train/{name}", self.last_losses[name], prog_bar=True, on_step=True, on_epoch=True, batch_size=n_rows)
        lr = self.current_lr()
        if lr is not None:                                                    # (once configure_optimizers has run)
            self.log_value("lr", lr, prog_bar=False, on_step=False, on_epoch=True, batch_size=1)

    # -- evaluation (MODEL:118-148) ------------------------------------------------------------------
    def _agent_eval_tensors(self, data, output):
        idx = data["agent_index"]
        return output["loc"][:, idx, :, :2], data.y[idx], output["reg_mask"][idx], data["source"]

    def _validation_trajectories(self, y_hat, y):
        """what validation_step's metrics compare; a model that predicts displacements overrides this"""
        return y_hat, y

    def validation_step(self, data, batch_idx):
        output = self(data)
        y_hat, y, mask, source = self._agent_eval_tensors(data, output)
        y_hat, y = self._validation_trajectories(y_hat, y)
        for metric in self.metrics_vl:
            metric.update(y_hat.detach(), y.detach(), mask.detach(), source.detach())
        return output

    def test_step(self, data, batch_idx):
        output = self(data)
        if getattr(self, "only_agent", False):                                # MODEL:136-137
            self.leave_only_agent(data, output)
        if data.y is not None:
            y_hat, y, mask, source = self._agent_eval_tensors(data, output)
            for metric in self.metrics_vl:
                metric.update(y_hat.detach(), y.detach(), mask.detach(), source.detach())
        return output

    def metric_results(self):
        return {n: float(m.compute()) for n, m in zip(self.metric_names, self.metrics_vl)}
