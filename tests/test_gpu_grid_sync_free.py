"""The forwards on a graph without fake agents (A = 0) in the sync-free form (-m gpu): the vanilla HiVT PredictionModel and the SDE model's
`forward_ood` run from a graph of trajsde_graph_prepare_async -- list lengths on the device, buffers and grids sized from bounds -- bit for
bit the forward on the exact graph; `forward_ood` captured whole by runtime.GraphedForward; and a training step on a batch whose graph a
sync-free forward left behind.

What runs here for the first time: the fused edge attention at 4 heads and on an A = 0 graph from device-side counts, the temporal kernels
and the OOD recurrences beside it, and the gathering global attention of a vanilla (4 heads) or OOD (8 heads, split rows) forward on such a
graph."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
K, T = 3, 6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    return torch.device("cuda:0")


def _check_range():
    from trajsde_amd import _lib
    torch.cuda.synchronize()
    _lib.check_range()


def _synth(**kw):
    from trajsde_amd.synth import synth
    return synth(**kw)


# name -> batch maker: no edge at all; one scene one below, at and above a 16-row tile; several scenes with padded history steps and both
# sources; irregular masks (gaps, rows without a bos, empty global segments)
SHAPES = {
    "n1": lambda: _synth(S=1, n=1, L=2, F=T, box=30.0, seed=60),
    "n15": lambda: _synth(S=1, n=15, L=4, F=T, box=60.0, seed=55),
    "n16": lambda: _synth(S=1, n=16, L=4, F=T, box=60.0, seed=56),
    "n17": lambda: _synth(S=1, n=17, L=4, F=T, box=60.0, seed=57),
    "3x13_padded_mixed": lambda: _synth(S=3, n=13, L=6, F=T, box=60.0, seed=5, mixed_source=True, history_dropout=0.3),
    "3x13_irregular": lambda: H._irregular(S=3, n=13, L=6, F=T, box=60.0, seed=5, mixed_source=True),
}


def _grid_model(heads, layers, dev, init_seed=9):
    from trajsde_amd.models.model_base_mix import PredictionModel
    model = PredictionModel(**H.grid_cfg(K, T, heads, layers), init_seed=init_seed).eval()
    H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
    return model.to(dev)


def _both_forms(model, batch, dev, keys, noise=None):
    """the forward under set_sync_free(True) and (False): {mode: (outputs, true counts)}; asserts the form of the graph each left"""
    from trajsde_amd import runtime
    assert runtime.sync_free()                                            # the default
    outs = {}
    for mode in (True, False):
        prev = runtime.set_sync_free(mode)
        try:
            data = batch.to(dev)
            with torch.no_grad():
                o = model(data, noise=noise() if noise is not None else None)
            gc = data["_trajsde_graph"]
            assert gc.batch.A == 0 and gc.graph.Nt == gc.batch.N
            assert bool(gc.graph.exact) == (not mode), ("graph form", mode)
            outs[mode] = ({k: o[k].clone() for k in keys}, gc.true_counts())
        finally:
            runtime.set_sync_free(prev)
    return outs


# ------------------------------------------------------------------ 1. vanilla
@pytest.mark.parametrize("heads,layers,name", [(4, 1, n) for n in SHAPES] + [(8, 2, "3x13_padded_mixed")])
def test_vanilla_sync_free_forward_is_bitwise_the_exact_forward(heads, layers, name, dev):
    """(on the parent commit the vanilla encoder asks for the exact graph under both settings: the `graph form` assertion fails)"""
    model = _grid_model(heads, layers, dev)
    keys = ("loc", "pi", "local_embed", "global_embed")
    outs = _both_forms(model, SHAPES[name](), dev, keys)
    assert outs[True][1] == outs[False][1]
    for k in keys:
        assert bool(torch.isfinite(outs[True][0][k]).all()), k
        assert torch.equal(outs[True][0][k], outs[False][0][k]), k
    _check_range()


# ------------------------------------------------------------------ 2. forward_ood
@pytest.mark.parametrize("n", [12, 17])
def test_ood_sync_free_forward_is_bitwise_the_exact_forward(n, dev):
    from trajsde_amd.runtime import NoiseSpec
    model, _ = H.build_model(K, T, 0.5, init_seed=3)
    H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
    model = model.to(dev).eval()
    model.ood = True
    batch = _synth(S=2, n=n, L=5, F=T, box=60.0, seed=40 + n, mixed_source=True, history_dropout=0.3)
    keys = ("loc", "pi", "stds")
    outs = _both_forms(model, batch, dev, keys, noise=lambda: NoiseSpec(seed=12))
    assert outs[True][1] == outs[False][1]
    assert float(outs[True][0]["stds"].abs().max()) > 0
    for k in keys:
        assert torch.equal(outs[True][0][k], outs[False][0][k]), k
    _check_range()


# ------------------------------------------------------------------ 3. capture
def _capture_batch():
    return _synth(S=4, n=40, L=12, F=T, box=80.0, seed=31, mixed_source=True)        # test_graph_replay_is_the_eager_forward's


def test_vanilla_capture_is_refused(dev):
    """runtime.GraphedForward takes the SDE model (plain or OOD); the vanilla model is refused with the reason"""
    from trajsde_amd import _lib, runtime
    model = _grid_model(4, 1, dev)
    with pytest.raises(_lib.TrajsdeError, match="does not capture the vanilla HiVT model"):
        runtime.GraphedForward(model, SHAPES["n17"]().to(dev))


def test_ood_graph_replay_is_the_eager_forward(dev):
    from trajsde_amd import runtime
    from trajsde_amd.runtime import NoiseSpec
    batch = _capture_batch()
    model, _ = H.build_model(K, T, 0.5, init_seed=6)
    model = model.to(dev).eval()
    model.ood = True
    gf = runtime.GraphedForward(model, batch.to(dev))
    keys = ("loc", "pi", "stds")
    stds = {}
    for seed in (5, 77):
        got = {k: gf(seed=seed)[k].clone() for k in keys}
        with torch.no_grad():
            want = model(batch.to(dev), noise=NoiseSpec(seed=seed))
        assert set(keys) <= set(want) and "diff_in" not in want
        for k in keys:
            assert torch.equal(got[k], want[k]), (seed, k)
        stds[seed] = got["stds"]
    assert not torch.equal(stds[5], stds[77])
    _check_range()


# ------------------------------------------------------------------ 4. training after a sync-free forward
def test_training_step_on_the_graph_a_sync_free_forward_left_behind(dev):
    """a batch that was rotated and given its graph ahead of the step (what runtime.prefetch_graph does, here by an inference forward):
    `training_step` finds the rotation marked done and the sync-free graph cached, and the backward entry points make that graph exact
    themselves.  Loss and gradients are those of the same step on a fresh copy of the batch, within 2e-5 relative: the bound-sized
    buffers change no arithmetic, only where the records lie"""
    from trajsde_amd import runtime
    from trajsde_amd.models.model_base_mix import PredictionModel
    from trajsde_amd.runtime import NoiseSpec
    batch = _synth(S=2, n=12, L=5, F=T, box=40.0, seed=8, history_dropout=0.3)
    model = PredictionModel(**H.grid_cfg(K, T, 4, 2, dropout=0.1), init_seed=4)
    H.perturb_parameters(model, 1234)
    model = model.to(dev)

    def step(data):
        for p in model.parameters():
            p.grad = None
        model.train()
        loss = model.training_step(data, 0, noise=NoiseSpec(seed=3, dropout_seed=7))
        loss.backward()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    data = batch.to(dev)
    model.eval()
    with torch.no_grad():
        model(data)                                                       # rotates data.y, leaves rotate_mat and the graph on the batch
    gc = data["_trajsde_graph"]
    assert not gc.graph.exact
    data[runtime.ROTATED_KEY] = True                                      # the rotation is done: the step must not apply it again
    loss, got = step(data)
    assert data["_trajsde_graph"] is gc and gc.graph.exact
    want_loss, want = step(batch.to(dev))
    _check_range()
    assert bool(torch.isfinite(loss)) and abs(float(loss) - float(want_loss)) <= 2e-5 * abs(float(want_loss))
    assert set(got) == set(want) and len(got) > 50
    bad = H.compare_grads("training step after a sync-free forward", got, want, rel=2e-5)
    assert not bad, bad
