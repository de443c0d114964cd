"""The model-level boundary of the path: `train.py:49-66` / `test.py:48-58` build the model class named in the YAML and hand
it to `pl.Trainer.fit / test`, which accept LightningModules only.  pytorch_lightning is not in the image, so these tests
run a fresh interpreter with the build's stand-in package (oracle/shims/pytorch_lightning -- test infrastructure) importable:
the class resolved through the registry must then BE a LightningModule, log what the reference's training_step logs, write the
result file of `test_epoch_end` (MODEL:150-165) with the reference's keys, and `leave_only_agent` (MODEL:168-202) must cut a
batch exactly like the reference's own static method does (its result stored under tests/golden/reference_calls)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r'''
import json, os, sys, types
root, out_dir = sys.argv[1], sys.argv[2]
sys.path[:0] = [os.path.join(root, "oracle", "shims"), root, os.path.join(root, "tests")]
import pytorch_lightning as pl
import torch, yaml
from trajsde_amd.models import lightning_base
from trajsde_amd.models.model_base_mix_sde import resolve_class
res = {"have_lightning": lightning_base.HAVE_LIGHTNING}
for name, cfg_file in (("sde", "mi355x_sde_encoder_decoder.yml"), ("grid", "mi355x_trmenc_mlpdec.yml")):
    with open(os.path.join(root, "trajsde_amd", "configs", cfg_file)) as f:
        cfg = yaml.safe_load(f)
    ms = cfg["model_specific"]
    model = resolve_class(ms["file_path"], ms["module_name"])(**cfg, init_seed=0)          # test.py:48-49
    r = {"is_lightning_module": isinstance(model, pl.LightningModule), "class": type(model).__name__,
         "metric_names": list(model.metric_names)}
    # test_epoch_end under a Trainer stand-in (MODEL:152: self.trainer._ckpt_path)
    ck_dir = os.path.join(out_dir, name, "checkpoints")
    os.makedirs(ck_dir)
    ck = os.path.join(ck_dir, "epoch=3-step=40.ckpt")
    model.trainer = types.SimpleNamespace(_ckpt_path=ck)
    for m in model.metrics_vl:                                     # one update so that compute() is defined
        T = 60
        pred = torch.zeros(cfg["model_specific"]["kwargs"]["num_modes"], 2, T, 2)
        m.update(pred, torch.ones(2, T, 2), torch.ones(2, T, dtype=torch.bool), torch.tensor([0, 1]))
    model.test_epoch_end([])
    path = os.path.join(out_dir, name, "out", "result_epoch=3-step=40.json")
    r["result_file"] = os.path.isfile(path)
    r["result_keys"] = sorted(json.load(open(path)))
    # logging goes through LightningModule.log under a Trainer
    model.log_value("train/L2", torch.tensor(1.5), prog_bar=True)
    r["logged_via_lightning"] = float(model._logged["train/L2"]) if hasattr(model, "_logged") else None
    r["logged_mirror"] = float(model.logged["train/L2"])
    res[name] = r
print("RESULT " + json.dumps(res))
'''


def _run(tmp_path):
    r = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_model_classes_are_lightning_modules_where_lightning_exists(tmp_path):
    res = _run(tmp_path)
    assert res["have_lightning"] is True
    for name, cls in (("sde", "PredictionModelSDENet"), ("grid", "PredictionModel")):
        r = res[name]
        assert r["class"] == cls and r["is_lightning_module"] is True
        assert r["result_file"] is True
        assert r["result_keys"] == sorted(r["metric_names"]) == ["ADE_T", "FDE_T", "MR_T"]       # CFG:84-96 metrics_module
        assert r["logged_via_lightning"] == 1.5 and r["logged_mirror"] == 1.5


def test_without_lightning_the_classes_are_plain_modules_with_the_same_hooks(tmp_path):
    """this image: no pytorch_lightning -> nn.Module base, hooks present, test_epoch_end driven by `result_ckpt_path`"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers as H
    from trajsde_amd.models import lightning_base
    model, cfg = H.build_model(2, 5, 0.5, init_seed=1)
    if lightning_base.HAVE_LIGHTNING:
        pytest.skip("pytorch_lightning is importable here")
    assert isinstance(model, torch.nn.Module)
    for hook in ("training_step", "validation_step", "test_step", "test_epoch_end", "configure_optimizers", "leave_only_agent"):
        assert callable(getattr(model, hook))
    with pytest.raises(RuntimeError, match="no checkpoint path"):
        model.test_epoch_end([])
    ck = tmp_path / "run" / "checkpoints" / "last.ckpt"
    os.makedirs(ck.parent)
    model.result_ckpt_path = str(ck)
    for m in model.metrics_vl:
        m.update(torch.zeros(2, 2, 5, 2), torch.ones(2, 5, 2), torch.ones(2, 5, dtype=torch.bool), torch.tensor([0, 0]))
    model.test_epoch_end([])
    got = json.load(open(tmp_path / "run" / "out" / "result_last.json"))
    assert sorted(got) == sorted(model.metric_names)
    model.configure_optimizers()
    assert model.current_lr() == pytest.approx(float(model.lr))


def test_leave_only_agent_cuts_the_batch_like_the_reference(tmp_path):
    """MODEL:168-202 against what the reference's own static method left of the same collated batch (3 scenes, ragged lanes):
    tests/golden/reference_calls/leave_only_agent.npz, made by oracle/make_golden_reference_calls.py"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers as H
    from trajsde_amd.models.lightning_base import LightningHooks
    ref = H.load_reference_call("leave_only_agent")
    ours_d, ours_o = H.leave_only_agent_case()
    LightningHooks.leave_only_agent(ours_d, ours_o)
    for k in ("loc", "pi", "reg_mask"):
        assert torch.equal(ours_o[k], ref["out." + k]), k
    for k in H.LEAVE_ONLY_AGENT_KEYS:
        assert torch.equal(ours_d[k], ref["data." + k]), k
    assert ours_d.num_nodes == int(ref["num_nodes"])
