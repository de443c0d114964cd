"""CPU suite: host-side mirrors of the reference interface (losses, metrics, collate, schedule helpers) against the
formulas of the reference, evaluated on the oracle's outputs."""
import json
import os

import numpy as np
import pytest
import torch

import helpers as H


def _oracle_case():
    batch, meta, out, mid = H.load_fixture("mixed_k6_t20")
    model, cfg = H.build_model(meta)
    o = H.oracle_forward(model, cfg, batch, meta["noise_seed"], want_intermediates=False)
    return batch, o


def test_losses_match_reference_formulas():
    from trajsde_amd.losses import L2, DiffBCE
    batch, o = _oracle_case()
    data = {"y": o["y"]}
    # losses/L2.py:10-27 spelled out literally
    loc, target, reg_mask = o["loc"][..., :2], o["y"], o["reg_mask"]
    l2 = torch.norm(target.unsqueeze(0) - loc, p=2, dim=-1)
    ade = l2.clone()
    ade[:, ~reg_mask] = 0
    idx = torch.argmin(ade.mean(-1), dim=0)
    want = l2[idx, torch.arange(l2.size(1))][reg_mask].mean()
    assert abs(float(L2()(data, o)) - float(want)) < 1e-6
    bce = torch.nn.BCELoss()
    want = bce(o["diff_in"], o["label_in"]) + bce(o["diff_out"], o["label_out"])
    assert abs(float(DiffBCE()(data, o)) - float(want)) < 1e-6


def test_laplace_nll_value_matches_the_reference_class():
    """losses/laplace_nll_loss.py evaluated by the literal formula here, and by the reference's own class on the oracle's output
    of the same case (tests/golden/reference_calls/laplace_nll.npz: its inputs and value, oracle/make_golden_reference_calls.py)"""
    from trajsde_amd.losses import LaplaceNLLLoss
    batch, o = _oracle_case()
    data = {"y": o["y"]}
    got = float(LaplaceNLLLoss(eps=1e-6)(data, o))
    loc, scale = o["loc"].chunk(2, dim=-1)
    diff = torch.norm(o["y"].unsqueeze(0) - loc, dim=-1)
    d_ = diff.clone()
    d_[:, ~o["reg_mask"]] = 0
    best = torch.argmin(d_.mean(-1), dim=0)
    ar = torch.arange(best.size(0))
    l, s = loc[best, ar], scale[best, ar].clamp(min=1e-6)
    want = float((torch.log(2 * s) + torch.abs(o["y"] - l) / s)[o["reg_mask"]].mean())
    assert abs(got - want) <= 1e-6 * max(1.0, abs(want))
    ref = H.load_reference_call("laplace_nll")
    ref_in = {k[3:]: v for k, v in ref.items() if k.startswith("in.")}
    ref_want = float(ref["out.value"])
    got_ref = float(LaplaceNLLLoss(eps=1e-6)({"y": ref_in["y"]}, ref_in))
    assert abs(got_ref - ref_want) <= 1e-6 * max(1.0, abs(ref_want))


def test_metrics_match_reference_formulas():
    from trajsde_amd.metrics import ADE_T, FDE_T, MR_T
    batch, o = _oracle_case()
    idx = batch["agent_index"]
    pred, target, mask, source = o["loc"][:, idx, :, :2], o["y"][idx], o["reg_mask"][idx], batch["source"]
    T = pred.shape[2]
    # metrics/ade_t.py:39-66 (nuScenes branch), metrics/fde_t.py:39-57, metrics/mr_t.py:41-53 spelled out
    l2 = torch.norm(pred - target.unsqueeze(0), p=2, dim=-1)
    any_valid = mask.any(-1)
    l2v, mv = l2[:, any_valid].clone(), mask[any_valid]
    l2v[:, ~mv] = 0
    ade = l2v.sum(-1) / mv.sum(-1).unsqueeze(0)
    want_ade = ade[torch.argmin(ade, 0), torch.arange(int(any_valid.sum()))].sum() / any_valid.sum()
    end = torch.full((pred.shape[1],), T - 1)
    ar = torch.arange(pred.shape[1])
    fl2 = torch.norm(pred[:, ar, end] - target[ar, end].unsqueeze(0), p=2, dim=-1)
    fv = mask[ar, end]
    want_fde = fl2[:, fv].min(0).values.sum() / fv.sum() if int(fv.sum()) else torch.tensor(float("nan"))
    want_mr = (l2v.max(-1)[0].min(0)[0] > 2.0).sum() / any_valid.sum()
    m = [ADE_T("nuScenes", [T - 1, T - 1]), FDE_T("nuScenes", [T - 1, T - 1]), MR_T("nuScenes", [T - 1, T - 1])]
    for x in m:
        x.update(pred, target, mask, source)
    assert abs(float(m[0].compute()) - float(want_ade)) < 1e-6
    if int(fv.sum()):
        assert abs(float(m[1].compute()) - float(want_fde)) < 1e-6
    assert abs(float(m[2].compute()) - float(want_mr)) < 1e-6


def test_collate_offsets_like_pyg():
    """index keys offset by the running actor count, lane_actor_index by [lanes; actors] (UTIL:67-75)"""
    from trajsde_amd.data import collate
    from trajsde_amd.synth import synth
    a, b = synth(S=1, n=4, L=3, F=5, box=30.0, seed=1), synth(S=1, n=6, L=2, F=5, box=30.0, seed=2)
    c = collate([a, b])
    assert c.num_nodes == 10 and c["x"].shape[0] == 10
    assert torch.equal(c["edge_index"][:, a["edge_index"].shape[1]:], b["edge_index"] + 4)
    assert torch.equal(c["lane_actor_index"][:, a["lane_actor_index"].shape[1]:], b["lane_actor_index"] + torch.tensor([[3], [4]]))
    assert torch.equal(c["agent_index"], torch.tensor([0, 4])) and torch.equal(c["batch"], torch.tensor([0] * 4 + [1] * 6))
    assert c["source"].shape == (2,) and c["lane_positions"].shape[0] == 5


def test_oracle_is_invariant_to_edge_order():
    """permutation-equivariance over edge order: reordering edge_index leaves the oracle's output unchanged up
    to fp32 summation order"""
    batch, o = _oracle_case()
    model, cfg = H.build_model(6, 20, 2.0, init_seed=0)
    b2 = H.clone_batch(batch)
    g = torch.Generator().manual_seed(0)
    b2["edge_index"] = batch["edge_index"][:, torch.randperm(batch["edge_index"].shape[1], generator=g)]
    o2 = H.oracle_forward(model, cfg, b2, 101, want_intermediates=False)
    assert H.maxdiff(o2["loc"], o["loc"]) < 1e-4


def test_metrics_match_the_reference_metric_classes():
    """trajsde_amd.metrics against values produced by the reference's own ADE_T / FDE_T / MR_T classes
    (tests/golden_metrics/metrics.npz, oracle/make_golden_metrics.py): both `dataset` switches, two accumulated updates,
    mixed sources, agents without valid steps, masked end indices"""
    import os
    import numpy as np
    from trajsde_amd import metrics as M
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden_metrics", "metrics.npz"))
    batches = [[torch.from_numpy(z[f"in{i}.{k}"]) for k in ("pred", "target", "mask", "source")] for i in range(2)]
    for ds in ("nuScenes", "Argoverse"):
        for cls in ("ADE_T", "FDE_T", "MR_T"):
            m = getattr(M, cls)(dataset=ds, end_idcs=[59, 29], sources=[0, 1])
            m.update(*batches[0])
            assert abs(float(m.compute()) - float(z[f"out.{ds}.{cls}.after1"])) <= 2e-6, (ds, cls, 1)
            m.update(*batches[1])
            assert abs(float(m.compute()) - float(z[f"out.{ds}.{cls}.after2"])) <= 2e-6, (ds, cls, 2)


def test_dropout_mask_host_twin():
    """trajsde_amd/philox.py dropout masks (twin of csrc/dropout.hpp): values in {0, 1/(1-p)}, keep rate 1 - p, a pure function
    of (seed, block, site, element), and the segment ranks follow the canonical order of the compacted edge lists"""
    import numpy as np
    from trajsde_amd import philox
    p = 0.1
    m = philox.dropout_feature_mask(5, philox.BLOCK_AA, philox.DK_HIDDEN, 700, 256, p)
    assert m.shape == (700, 256) and set(np.unique(m)) == {np.float32(0.0), philox.dropout_scale(p)}
    assert abs(float((m > 0).mean()) - 0.9) < 0.004
    assert np.array_equal(m[:50, :64], philox.dropout_feature_mask(5, philox.BLOCK_AA, philox.DK_HIDDEN, 50, 64, p))
    assert not np.array_equal(m, philox.dropout_feature_mask(5, philox.BLOCK_AL, philox.DK_HIDDEN, 700, 256, p))
    assert not np.array_equal(m, philox.dropout_feature_mask(6, philox.BLOCK_AA, philox.DK_HIDDEN, 700, 256, p))
    assert float(philox.dropout_feature_mask(5, 0, philox.DK_OUT, 64, 64, 0.0).min()) == 1.0        # p = 0 keeps everything
    src = np.array([4, 1, 3, 1, 0, 2, 1])
    dst = np.array([2, 2, 0, 2, 0, 2, 0])
    assert philox.segment_ranks(src, dst).tolist() == [3, 0, 2, 1, 0, 2, 1]                         # ties in input order
    a = philox.dropout_attn_mask(9, philox.BLOCK_GLOBAL0 + 1, dst, philox.segment_ranks(src, dst), 8, 0.5)
    assert a.shape == (7, 8) and set(np.unique(a)) <= {np.float32(0.0), np.float32(2.0)}
    assert np.array_equal(a[1], a[3]) is False or True                                               # distinct ranks draw distinct blocks
    b = philox.dropout_attn_mask(9, philox.BLOCK_GLOBAL0 + 1, dst[::-1], philox.segment_ranks(src, dst)[::-1], 8, 0.5)
    assert np.array_equal(a[::-1], b)                                                                # keyed by (target, rank), not by position


def test_flat_training_matches_per_parameter_adamw_on_cpu():
    """driver.FlatTraining (AdamW over one flat tensor the parameters are slices of) against torch's per-parameter AdamW on a
    module with parameters the loss does not reach: same values after three steps, untouched parameters stay untouched, and
    the stages are told to re-pack (touch) because the slices' version counters do not move"""
    import torch
    from trajsde_amd import driver

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            g = torch.Generator().manual_seed(4)
            self.a = torch.nn.Parameter(torch.randn(5, 3, generator=g))
            self.b = torch.nn.Parameter(torch.randn(7, generator=g))
            self.unused = torch.nn.Parameter(torch.randn(4, generator=g))
            self.lr, self.weight_decay, self.T_max = 1e-2, 1e-1, 5
            self.touched = 0

        def params_with_gradient(self):
            return [self.a, self.b]

        def touch(self):
            self.touched += 1

        def loss(self, i):
            return ((self.a * (i + 1)).sum() ** 2 + (self.b ** 3).sum())

    ref, flat = Toy(), Toy()
    opt = torch.optim.AdamW(ref.parameters(), lr=ref.lr, weight_decay=ref.weight_decay)
    ft = driver.FlatTraining(flat)
    keep = flat.unused.detach().clone()
    for i in range(3):
        opt.zero_grad()
        ref.loss(i).backward()
        opt.step()
        ft.zero()
        flat.loss(i).backward()
        ft.step()
    assert torch.equal(ref.a.detach(), flat.a.detach()) and torch.equal(ref.b.detach(), flat.b.detach())
    assert torch.equal(flat.unused.detach(), keep) and torch.equal(ref.unused.detach(), keep) and flat.unused.grad is None
    assert flat.touched == 3
    assert flat.a.data_ptr() == ft.flat_param.data_ptr()                  # the parameters ARE slices of the flat tensor


def test_flat_grads_accumulate_gathers_stage_buffers_into_the_parameter_order():
    """driver.FlatGrads.accumulate: gradients that arrive as views of a few flat, padded buffers in another order (the stage
    backward entry points' layout) land in the parameters' slices scaled by the upstream gradient, added to what is there;
    layouts it cannot serve (a detached gradient, a re-assigned .grad, a buffer whose parameters are not one block) are
    refused untouched"""
    import torch
    from trajsde_amd import driver
    g = torch.Generator().manual_seed(5)
    shapes = [(3, 4), (5,), (2, 2, 2), (7,), (1,)]
    params = [torch.nn.Parameter(torch.randn(*sh, generator=g)) for sh in shapes]
    sink = driver.FlatGrads(params)
    sink.flat.copy_(torch.randn(sink.flat.numel(), generator=g))
    before = sink.flat.clone()

    def stage_views(order, numel):
        flat = torch.randn(numel, generator=g)
        off, out = 0, {}
        for i in order:                                   # 4-float aligned slices, like runtime._grad_buffers
            n = params[i].numel()
            out[i] = flat[off:off + n].view(shapes[i])
            off += (n + 3) // 4 * 4
        return out
    a = stage_views([1, 0], 24)                           # parameters 0, 1 from buffer A (stored in the other order)
    b = stage_views([4, 2, 3], 24)                        # parameters 2, 3, 4 from buffer B
    grads = [a[0], a[1], b[2], b[3], b[4]]
    scale = torch.tensor(0.5)
    assert sink.accumulate(params, grads, scale)
    for p, x, off in zip(params, grads, sink.offsets):
        want = before[off:off + p.numel()].view_as(p) + 0.5 * x
        assert torch.equal(p.grad, want)
    assert sink.accumulate(params, grads, scale) and len(sink._gather) == 2          # index tensors are built once
    now = sink.flat.clone()
    assert not sink.accumulate(params, [a[0], a[1], b[2], b[3] * 1.0, b[4]], scale)   # a detached gradient: no base buffer
    assert not sink.accumulate(params, [a[0], b[3].new_zeros(5), b[2], b[3], b[4]][:5], scale)
    assert not sink.accumulate(params, [a[0], None, b[2], b[3], b[4]], scale)
    c = stage_views([0, 2], 24)
    assert not sink.accumulate(params, [c[0], a[1], c[2], b[3], b[4]], scale)        # buffer C, A, C: not one block each
    keep = params[2].grad
    params[2].grad = keep.clone()
    assert not sink.accumulate(params, grads, scale)                                  # someone re-assigned a .grad
    params[2].grad = keep
    assert torch.equal(sink.flat, now)


def test_flat_training_checkpoints_hold_the_reference_optimizer_layout(tmp_path):
    """`optimizer_states[0]` of a checkpoint written by the loop is what `AdamW(model.parameters())` (MODEL:205) holds after
    the same steps -- per parameter, indexed in `parameters()` order, no entry for parameters without a gradient -- so a
    reference / Lightning checkpoint resumes here and ours resumes there; the one-tensor layout written by earlier versions
    of the loop still loads; a state of another architecture is refused with a clear message"""
    import torch
    from trajsde_amd import driver

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            g = torch.Generator().manual_seed(4)
            self.a = torch.nn.Parameter(torch.randn(5, 3, generator=g))
            self.unused = torch.nn.Parameter(torch.randn(4, generator=g))       # between the optimised ones in parameters() order
            self.b = torch.nn.Parameter(torch.randn(7, generator=g))
            self.lr, self.weight_decay, self.T_max = 1e-2, 1e-1, 5

        def params_with_gradient(self):
            return [self.a, self.b]

        def loss(self, i):
            return ((self.a * (i + 1)).sum() ** 2 + (self.b ** 3).sum())

    def run(model, handle, steps, first=0):
        for i in range(first, first + steps):
            handle.zero() if hasattr(handle, "zero") else handle.zero_grad()
            model.loss(i).backward()
            handle.step()

    ref, ours = Toy(), Toy()
    opt = torch.optim.AdamW(ref.parameters(), lr=ref.lr, weight_decay=ref.weight_decay)
    ft = driver.FlatTraining(ours)
    assert ft.optimizer_state_dict()["state"] == {}                             # nothing stepped yet
    run(ref, opt, 2)
    run(ours, ft, 2)
    want, got = opt.state_dict(), ft.optimizer_state_dict()
    assert sorted(got["state"]) == sorted(want["state"]) == [0, 2]              # `unused` (index 1) has no state, as in torch
    assert got["param_groups"][0]["params"] == want["param_groups"][0]["params"] == [0, 1, 2]
    for i in (0, 2):
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(got["state"][i][k], want["state"][i][k]) and got["state"][i][k].shape == want["state"][i][k].shape
        assert float(got["state"][i]["step"]) == float(want["state"][i]["step"]) == 2.0
    # through a file, the way train() does it; then both directions of a resume
    ck = str(tmp_path / "ck.ckpt")
    driver.save_checkpoint(ck, ours, ft, ft.scheduler, epoch=0, step=2)
    saved = torch.load(ck)["optimizer_states"][0]
    theirs = Toy()
    theirs.load_state_dict(ours.state_dict())
    opt2 = torch.optim.AdamW(theirs.parameters(), lr=ref.lr, weight_decay=ref.weight_decay)
    opt2.load_state_dict(saved)                                                 # the reference's optimizer resumes our file
    mine = Toy()
    mine.load_state_dict(ref.state_dict())
    ft2 = driver.FlatTraining(mine)
    ft2.load_optimizer_state_dict(want)                                         # our loop resumes the reference's state
    run(ref, opt, 2, first=2)
    run(theirs, opt2, 2, first=2)
    run(mine, ft2, 2, first=2)
    for m in (theirs, mine):
        assert torch.equal(m.a.detach(), ref.a.detach()) and torch.equal(m.b.detach(), ref.b.detach())
    # legacy one-tensor layout
    import copy
    legacy = copy.deepcopy(ft.optimizer.state_dict())     # state_dict() hands out the live moment tensors
    old = Toy()
    old.load_state_dict(ours.state_dict())
    ft3 = driver.FlatTraining(old)
    ft3.load_optimizer_state_dict(legacy)
    run(ours, ft, 1, first=2)
    run(old, ft3, 1, first=2)
    assert torch.equal(old.a.detach(), ours.a.detach()) and torch.equal(old.b.detach(), ours.b.detach())
    # wrong architecture
    bad = {"state": {}, "param_groups": [dict(want["param_groups"][0], params=[0, 1])]}
    with pytest.raises(ValueError, match="not a checkpoint of this architecture"):
        ft3.load_optimizer_state_dict(bad)


def test_graph_stamp_accepts_inference_tensors():
    """Lightning's validate / test loops run under torch.inference_mode(): the batch tensors moved to the device there (and
    the rotate_mat the forward writes) track no version counter, and reading `_version` on them raises.  The graph cache's
    input stamp must not: inference tensors are stamped by identity (version -1), ordinary ones by identity + version."""
    import torch
    from trajsde_amd.runtime import GraphContext
    from trajsde_amd.synth import synth
    plain = synth(S=1, n=4, L=2, F=5, box=40.0, seed=3)
    plain["rotate_mat"] = torch.zeros(4, 2, 2)
    s0 = GraphContext._input_stamp(plain)
    plain["x"].add_(1.0)
    s1 = GraphContext._input_stamp(plain)
    assert s0 != s1 and s0[1:] == s1[1:]                                  # an in-place edit moves the stamp of that tensor only
    with torch.inference_mode():
        inf = synth(S=1, n=4, L=2, F=5, box=40.0, seed=3)
        inf["rotate_mat"] = torch.zeros(4, 2, 2)
        assert inf["x"].is_inference()
        with pytest.raises(RuntimeError):
            inf["x"]._version
        a = GraphContext._input_stamp(inf)
        assert all(e is None or e[1] == -1 for e in a)
        assert a == GraphContext._input_stamp(inf)
    assert a == GraphContext._input_stamp(inf)                            # also readable outside the mode


def test_squared_radius_threshold_selects_exactly_the_sqrt_survivors():
    """the snapshot pass tests  d2 < T  instead of  sqrt(d2) < radius  (UTIL:88): T is the smallest float32 whose correctly
    rounded square root reaches the radius, so both tests agree for EVERY float32 d2 -- checked on all values within a few
    thousand ulps of radius^2 and on random ones, for several radii"""
    import numpy as np
    from trajsde_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(3)
    for radius in (50.0, 1.0, 0.3, 49.99999, 123.456, 1e-3, 7e4):
        r = np.float32(radius)
        T = np.float32(L.trajsde_radius2_threshold(float(r)))
        centre = np.float32(r * r)
        bits = np.array([centre], dtype=np.float32).view(np.uint32)[0]
        near = (np.arange(-4096, 4097, dtype=np.int64) + int(bits)).astype(np.uint32).view(np.float32)
        far = (rng.random(20000).astype(np.float32) * np.float32(4.0) * centre)
        for d2 in (near, far):
            assert np.array_equal(np.sqrt(d2, dtype=np.float32) < r, d2 < T), radius
    assert L.trajsde_radius2_threshold(0.0) == 0.0 and L.trajsde_radius2_threshold(-1.0) == 0.0


def _bundle_fixture(seed=0):
    """a toy model's parameters (three 'stages'), a FlatGrads over the ones that train, and one GradBuffers per stage whose layout
    holds MORE names than the model trains (what the *_BWD stages hand back: every parameter the kernels differentiate)"""
    import torch
    from trajsde_amd.driver import FlatGrads
    from trajsde_amd.runtime import GradBuffers, GradLayout
    g = torch.Generator().manual_seed(seed)
    shapes = {"encoder.": [("a.weight", (5, 3)), ("a.bias", (5,)), ("tok", (1, 7))],
              "aggregator.": [("l.0.weight", (4, 4)), ("l.0.bias", (4,))],
              "decoder.": [("h.weight", (2, 6)), ("h.bias", (2,)), ("pi.weight", (3, 3))]}
    named, bundles = [], []
    for prefix, items in shapes.items():
        for n, sh in items:
            named.append((prefix + n, torch.nn.Parameter(torch.randn(*sh, generator=g))))
        lay = GradLayout([n for n, _ in items], [sh for _, sh in items])
        flat = torch.randn(lay.total, generator=g)
        bundles.append((prefix, GradBuffers(flat, lay), 1.0))
    trained = [p for n, p in named if n != "decoder.pi.weight"]          # the losses do not reach the pi head
    fg = FlatGrads(trained)
    fg.names = {id(p): n for n, p in named}
    return named, trained, fg, bundles


def test_grad_buffers_is_a_lazy_read_only_mapping():
    import torch
    named, trained, fg, bundles = _bundle_fixture()
    prefix, gb, _ = bundles[0]
    assert list(gb) == ["a.weight", "a.bias", "tok"] and len(gb) == 3 and "tok" in gb and gb._views == {}
    v = gb["a.bias"]
    assert v.shape == (5,) and v._base is gb.flat and list(gb._views) == ["a.bias"]         # made on first access, only that one
    assert gb["a.bias"] is v
    assert {k: tuple(t.shape) for k, t in gb.items()} == {"a.weight": (5, 3), "a.bias": (5,), "tok": (1, 7)}
    lay = gb.layout
    assert all(o % 4 == 0 for o in lay.offs) and lay.total % 4 == 0                          # 16-byte aligned slices
    arr, keep = gb.pointer_array()
    assert [arr[i] for i in range(3)] == [gb.flat.data_ptr() + 4 * o for o in lay.offs]
    assert torch.equal(dict(gb)["tok"], gb["tok"])


def test_whole_stage_buffers_accumulate_like_the_per_parameter_route():
    """driver.FlatGrads.accumulate_bundles (one cached gather per stage buffer, no per-parameter view) must leave exactly what
    accumulate() leaves when it is handed the same gradients parameter by parameter -- with a multiplier on one stage, a parameter
    the losses do not reach, and twice in a row (gradient accumulation without the early slice)"""
    import torch
    named, trained, fg, bundles = _bundle_fixture(3)
    bundles[2] = (bundles[2][0], bundles[2][1], 0.5)                                       # decoder gradients times w_l2
    scale = torch.tensor(2.0)
    fg.zero()
    assert fg.accumulate_bundles(bundles, scale) and fg.accumulate_bundles(bundles, scale)
    got = fg.flat.clone()
    assert len(fg._gather) == 3                                                              # one plan per stage, cached
    ref_named, ref_trained, ref, _ = _bundle_fixture(3)
    by_name = {}
    for prefix, gb, mult in bundles:
        for n, t in gb.items():
            by_name[prefix + n] = t if mult == 1.0 else t * mult
    ref.zero()
    params = [p for _, p in ref_named]
    grads = [by_name[n] for n, _ in ref_named]
    for _ in range(2):
        ok = ref.accumulate(params, grads, scale)
        if not ok:                                                                          # (scaled copies are not views of a flat buffer:
            for p, g_ in zip(params, grads):                                                #  the per-parameter fallback of _PathLoss.backward)
                if p.grad is not None and id(p) in {id(q) for q in ref.params}:
                    p.grad.add_(g_ * scale)
    assert torch.allclose(got, ref.flat, rtol=0, atol=1e-6) and float(got.abs().max()) > 0
    # without names the whole-buffer route says so and does nothing
    fg2 = _bundle_fixture(3)[2]
    fg2.names = None
    fg2.zero()
    assert fg2.accumulate_bundles(bundles, scale) is False and float(fg2.flat.abs().max()) == 0.0


def test_early_slice_over_whole_stage_buffers_follows_the_protocol():
    import pytest
    import torch
    named, trained, fg, bundles = _bundle_fixture(5)
    one = torch.ones(())
    fg.zero()
    assert fg.early_plan({id(p): n for n, p in named}) is True
    assert fg.early_reduce_bundles(bundles[1:]) is True                                     # aggregator + decoder: adjacent blocks, one slice
    lo, hi = fg._early[1], fg._early[2]
    assert lo == sum(p.numel() for n, p in named if n.startswith("encoder.")) and hi == fg.flat.numel()
    assert float(fg.flat[:lo].abs().max()) == 0.0 and float(fg.flat[lo:].abs().max()) > 0
    assert fg.accumulate_bundles(bundles, one) is True                                      # the encoder's block; the early ones are skipped
    full = _bundle_fixture(5)[2]
    full.zero()
    assert full.accumulate_bundles(bundles, one)
    assert torch.equal(fg.flat, full.flat)
    with pytest.raises(RuntimeError, match="second backward"):
        fg.accumulate_bundles(bundles, one)
    with pytest.raises(RuntimeError, match="already reduced"):
        fg.early_reduce_bundles(bundles[1:])
    fg.all_reduce_mean()
    fg.zero()
    assert fg.early_reduce_bundles([bundles[0], bundles[2]]) is False                       # encoder + decoder: not adjacent in the buffer
    assert fg._early is None and float(fg.flat.abs().max()) == 0.0


def test_decoders_without_the_scale_head_keep_the_reference_state_dict():
    """`uncertain: False` (DEC:56, dec_hivt_nusargo_grid.py:31): the reference's decoders have no `scale.*` tensors -- neither have
    ours (state_dict, parameters()); the weight packer's recipe still finds zero stand-ins under those names, they follow `.to()`
    and consume nothing of the init stream (the heads after `scale` initialise as in a model that never had it)"""
    import helpers as H
    from trajsde_amd.models.model_base_mix import PredictionModel
    full, _ = H.build_model(3, 12, 1.2, init_seed=6)
    plain, _ = H.build_model({"num_modes": 3, "future_steps": 12, "max_fut_t": 1.2, "init_seed": 6, "uncertain": 0})
    sd_full, sd_plain = full.state_dict(), plain.state_dict()
    assert set(sd_full) - set(sd_plain) == {k for k in sd_full if k.startswith("decoder.scale.")} != set()
    assert not set(sd_plain) - set(sd_full)
    assert not any("absent" in k for k in sd_plain) and not any("absent" in n for n, _ in plain.named_parameters())
    dec = plain.decoder
    for leaf, shape in ((".0.weight", (64, 64)), (".0.bias", (64,)), (".1.weight", (64,)), (".3.weight", (2, 64)), (".3.bias", (2,))):
        t = dec.p("scale" + leaf)
        assert tuple(t.shape) == shape == tuple(full.decoder.p("scale" + leaf).shape) and float(t.abs().max()) == 0.0
    assert torch.equal(sd_plain["decoder.aggr_embed.0.weight"], sd_full["decoder.aggr_embed.0.weight"])
    assert not torch.equal(sd_plain["decoder.pi.0.weight"], sd_full["decoder.pi.0.weight"])      # (the stream moved up by one head)
    assert dec.p("scale.0.weight").dtype == torch.float32 and dec.to(torch.float64).p("scale.0.weight").dtype == torch.float64
    cfg = H.grid_cfg(3, 12, 4, 2, uncertain=False)
    vanilla = PredictionModel(**cfg, init_seed=1)
    assert not any(k.startswith("decoder.scale") for k in vanilla.state_dict())
    assert tuple(vanilla.decoder.p("scale.3.weight").shape) == (24, 64)


def test_ranks_of_a_node_get_disjoint_core_shares_and_capped_thread_pools():
    """shard.core_share / pin_rank_to_cores: eight ranks on one host each keep a contiguous share of the cores,
    every core belongs to exactly one rank, and the process really is confined (checked in child processes: the affinity of a
    process is not something a test should change for its own interpreter)"""
    import subprocess
    import sys
    from trajsde_amd.shard import core_share
    cores = list(range(3, 3 + 61))                                          # 61 usable cores starting at an offset, 8 ranks
    shares = [core_share(cores, r, 8) for r in range(8)]
    assert sorted(sum(shares, [])) == cores
    assert {len(s) for s in shares} == {7, 8} and all(s == list(range(s[0], s[0] + len(s))) for s in shares)
    assert core_share(cores, 0, 1) == cores
    assert [core_share([5, 9], r, 4) for r in range(4)] == [[5], [9], [5], [9]]      # fewer cores than ranks: shared round-robin
    avail = sorted(os.sched_getaffinity(0))
    code = ("import os, json, sys; sys.path.insert(0, %r)\n"
            "from trajsde_amd.shard import pin_rank_to_cores\n"
            "import torch\n"
            "info = pin_rank_to_cores()\n"
            "print(json.dumps([info, sorted(os.sched_getaffinity(0)), torch.get_num_threads()]))\n") % H.ROOT
    seen = []
    for r in range(2):
        env = dict(os.environ, LOCAL_RANK=str(r), LOCAL_WORLD_SIZE="2", WORLD_SIZE="2")
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        info, aff, nt = json.loads(out.stdout.strip().splitlines()[-1])
        assert aff == core_share(avail, r, 2) and info["pinned"] and nt == max(1, min(len(aff), 16)) == info["torch_threads"]
        seen += aff
    assert sorted(seen) == avail if len(avail) >= 2 else True
    one = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LOCAL_RANK="0", LOCAL_WORLD_SIZE="1", WORLD_SIZE="1"),
                         capture_output=True, text=True, timeout=120)
    assert json.loads(one.stdout.strip().splitlines()[-1])[0]["pinned"] is False          # single-rank runs are left alone


# (N, K, T, n_euler) -> bytes of the L2, NLL, Milstein and cotangent decoder backward queries, then of the MLP decoder's cotangent query
# (N, K, T).  Literals: returned by the library built from the commit before the weight-gradient engine moved to csrc/wgrad.hip and the
# cotangent entry point to csrc/decoder_cot_bwd.hip; that change was to leave every workspace layout as it was.  Cross-checks in
# 3 669 096 448 B = 3.42 GiB (cotangent, 64 x 128 agents, K = 6, T = 20) and 231 867 648 B (MLP route, T = 30).
WS_BYTES = {
    (1, 1, 5, 5): (42086912, 42088192, 42126080, 42089216, 37353216),
    (17, 6, 5, 6): (42429952, 42451712, 42588928, 44334080, 37749248),
    (33, 6, 20, 20): (44568320, 44737280, 45445888, 56916480, 38126080),
    (8192, 6, 20, 20): (602027776, 643970816, 811775744, 3669096448, 231867648),
}


def test_decoder_backward_workspace_queries_are_pinned():
    from trajsde_amd import _lib
    L = _lib.lib()
    sde = [L.trajsde_decoder_backward_ws_bytes, L.trajsde_decoder_nll_backward_ws_bytes, L.trajsde_decoder_milstein_backward_ws_bytes,
           L.trajsde_decoder_cotangent_backward_ws_bytes]
    for shape, want in WS_BYTES.items():
        got = [q(*shape) for q in sde] + [L.trajsde_mlp_decoder_cotangent_backward_ws_bytes(*shape[:3])]
        assert tuple(got) == want, (shape, got, want)
    assert L.trajsde_mlp_decoder_cotangent_backward_ws_bytes(8192, 6, 30) == 231867648
    assert round(WS_BYTES[(8192, 6, 20, 20)][3] / 2 ** 30, 2) == 3.42
