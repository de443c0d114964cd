"""The actor CSR from the closed form of a dataset-order edge list (-m gpu; prep.hip k_direct2, DESIGN.md graph stage).

A batch is in dataset order when `batch` is non-decreasing and `edge_index` is, position for position, the concatenation over the
scenes of `for s in lo..hi-1: for d in lo..hi-1, d != s: (s, d)`.  The graph stage then writes the target-major CSR without sorting
("direct"); any other list goes through histogram, scatter and row sort ("general"), decided on the device.

The yardstick of every case is THE SAME BATCH WITH ITS EDGE LIST RANDOMLY PERMUTED: that run takes the general path (pinned by
test_edge_order_invariance and the oracle-list tests of test_gpu_parity.py).  Compared with torch.equal, in the exact form (with the
exported lists and intermediates of `capture_intermediates`) and in the sync-free form (outputs, and the lists after make_exact):
loc, pi, diff_in, diff_out, every list and segment pointer.

The batch vector is a required field of the C ABI for both models (the extended-node table reads source[batch[i]]), so there is no
"batch without a scene vector" to hand to the library: the vanilla model is run on the same batches and takes the same paths."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
K, T = 2, 5
KEYS = ("loc", "pi", "diff_in", "diff_out")
VANILLA_KEYS = ("loc", "pi", "local_embed", "global_embed")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sde(dev):
    model, _ = H.build_model(K, T, 0.5, init_seed=4)
    return model.to(dev).eval()


@pytest.fixture(scope="module")
def vanilla(dev):
    from trajsde_amd.models.model_base_mix import PredictionModel
    model = PredictionModel(**H.grid_cfg(K, T, 4, 1), init_seed=9).eval()
    H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
    return model.to(dev)


def _scenes(sizes, seed0=300):
    """one batch of scenes of the given sizes, collated the way the data loader does (node offsets, `batch` ascending)"""
    from trajsde_amd.data import collate
    from trajsde_amd.synth import synth
    return collate([synth(S=1, n=n, L=3, F=T, box=60.0, seed=seed0 + i, source=i % 2, history_dropout=0.3 if n > 2 else 0.0)
                    for i, n in enumerate(sizes)])


def _permuted(batch, seed=5):
    b = H.clone_batch(batch)
    E = b["edge_index"].shape[1]
    b["edge_index"] = b["edge_index"][:, torch.randperm(E, generator=torch.Generator().manual_seed(seed))]
    return b


def _run(model, batch, dev, sync_free, keys=KEYS):
    """one forward -> (path the graph stage took, {name: tensor or int} of everything compared)"""
    from trajsde_amd import runtime
    from trajsde_amd.runtime import GraphContext, NoiseSpec
    enc = model.encoder
    capture = not sync_free and keys is KEYS          # the SDE encoder exports its lists with their senders, aa_out and latent_ys
    prev = runtime.set_sync_free(sync_free)
    if capture:
        enc.capture_intermediates = True
    try:
        data = H.clone_batch(batch).to(dev)
        with torch.no_grad():
            o = model(data, noise=NoiseSpec(seed=12) if keys is KEYS else None)
        gc = data[GraphContext.KEY]
        assert bool(gc.graph.exact) == (not sync_free)
        path = gc.graph_path()
        out = {k: o[k].clone() for k in keys}
        out.update(gc.true_counts())
        more = enc.last_intermediates if capture else gc.edge_lists()
        out.update({k: (v.clone() if torch.is_tensor(v) else v) for k, v in more.items()})
    finally:
        runtime.set_sync_free(prev)
        if capture:
            enc.capture_intermediates = False
    return path, out


def _same(got, want, where):
    assert got.keys() == want.keys(), where
    for k in want:
        if torch.is_tensor(want[k]):
            assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), (where, k)
        else:
            assert got[k] == want[k], (where, k)


def _check(model, batch, dev, expect, keys=KEYS, where=""):
    """`batch` takes path `expect` and equals its randomly permuted self (general path), in both forms"""
    E = batch["edge_index"].shape[1]
    for sync_free in (False, True):
        path, got = _run(model, batch, dev, sync_free, keys)
        ypath, want = _run(model, _permuted(batch), dev, sync_free, keys)
        print(f"[graph-direct] {where} sync_free={sync_free}: E {E}, path {path}, yardstick {ypath}, E_aa {got['E_aa']}")
        assert path == expect, (where, sync_free, path)
        assert ypath == "general" or E <= 2, (where, "the yardstick did not take the general path")
        _same(got, want, (where, sync_free))


# ------------------------------------------------------------------ 1. direct path taken, bit-equal
# 64 | 65: either side of k_aa_count's 64-candidate chunk (in-degrees 63 and 64); 70: a partial second chunk; the singleton has no edge
@pytest.mark.parametrize("sizes", [(1, 2, 3, 64, 65, 70), (3, 65, 2, 1), (1, 70, 64, 3)],
                         ids=["1-2-3-64-65-70", "singleton_last", "singleton_first"])
def test_dataset_order_takes_the_direct_path_and_equals_the_sorted_csr(sizes, sde, dev):
    _check(sde, _scenes(sizes), dev, "direct", where=str(sizes))


def test_vanilla_model_on_dataset_order(vanilla, dev):
    """the vanilla model (A = 0 graph) hands the library the same batch fields, the scene vector included: same decision"""
    _check(vanilla, _scenes((1, 2, 3, 17, 66)), dev, "direct", keys=VANILLA_KEYS, where="vanilla")
    b = _scenes((4, 1, 6, 5))
    b["edge_index"] = b["edge_index"].flip(0).contiguous()
    _check(vanilla, b, dev, "general", keys=VANILLA_KEYS, where="vanilla target-major")


# ------------------------------------------------------------------ 2. near misses: one edit of a dataset-order list each
def _edit(name):
    b = _scenes((4, 1, 6, 5, 66))                      # nodes 0-3 | 4 | 5-10 | 11-15 | 16-81
    ei = b["edge_index"]
    E = ei.shape[1]
    j = 12 + 17                                         # an edge of the third scene (the first has 12): source 5 + 17 // 5 = 8
    assert int(ei[0, j]) == 8 and int(ei[1, j]) == 7
    if name == "dropped":
        ei = torch.cat([ei[:, :j], ei[:, j + 1:]], dim=1)
    elif name == "adjacent_swapped":
        ei = ei.clone()
        ei[:, [j, j + 1]] = ei[:, [j + 1, j]]
    elif name == "first_seventh_appended":
        ei = torch.cat([ei, ei[:, :E // 7]], dim=1)
    elif name == "target_in_another_scene":
        ei = ei.clone()
        ei[1, j] = 13
    elif name == "self_loop":
        ei = ei.clone()
        ei[1, j] = ei[0, j]
    elif name == "target_major":
        ei = ei.flip(0)
    elif name == "scene_ids_exchanged":
        bt = b["batch"].clone()
        bt[b["batch"] == 2], bt[b["batch"] == 3] = 3, 2
        b["batch"] = bt
    elif name == "no_edges":
        ei = ei[:, :0]
    else:
        raise KeyError(name)
    b["edge_index"] = ei.contiguous()
    return b


NEAR_MISSES = ("dropped", "adjacent_swapped", "first_seventh_appended", "target_in_another_scene", "self_loop", "target_major",
               "scene_ids_exchanged", "no_edges")


@pytest.mark.parametrize("name", NEAR_MISSES)
def test_near_miss_takes_the_general_path_and_is_still_right(name, sde, dev):
    _check(sde, _edit(name), dev, "general", where=name)


# ------------------------------------------------------------------ 3. alternation: the word and the optimistic writes leave nothing behind
def test_replays_alternate_between_the_paths(sde, dev):
    """one captured forward (one workspace, replayed): dataset order, then the list edited in place into a near miss, then back --
    each replay is bit for bit the stand-alone eager forward of what the batch held"""
    from trajsde_amd import runtime
    from trajsde_amd.runtime import GraphContext, NoiseSpec
    batch = _scenes((3, 65, 1, 9))
    j = 6 + 100
    miss = H.clone_batch(batch)
    miss["edge_index"][1, j] = 70                       # a target in the last scene (nodes 69-77), E unchanged
    assert int(batch["edge_index"][1, j]) < 68

    def eager(b):
        data = H.clone_batch(b).to(dev)
        with torch.no_grad():
            o = sde(data, noise=NoiseSpec(seed=21))
        return data[GraphContext.KEY].graph_path(), {k: o[k].clone() for k in KEYS}

    pa, want_a = eager(batch)
    pb, want_b = eager(miss)
    assert (pa, pb) == ("direct", "general")
    assert not torch.equal(want_a["loc"], want_b["loc"])
    data = H.clone_batch(batch).to(dev)
    gf = runtime.GraphedForward(sde, data)
    for step, (b, want) in enumerate(((batch, want_a), (miss, want_b), (batch, want_a), (batch, want_a), (miss, want_b))):
        data["edge_index"].copy_(b["edge_index"])
        out = gf(seed=21)
        for k in KEYS:
            assert torch.equal(out[k], want[k]), (step, k)
    # eager forwards of the three kinds in turn on the same model
    for b, (p, want) in ((batch, (pa, want_a)), (miss, (pb, want_b)), (batch, (pa, want_a))):
        got_p, got = eager(b)
        assert got_p == p
        _same(got, want, "eager alternation")
