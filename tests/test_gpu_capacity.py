"""The staging launch trajsde_batch_pad and runtime.CapacityBuffers (-m gpu): a batch of any shape into capacity-sized static tensors
with inert padding.

  1. the launch against its torch twin runtime.pad_batch_host, bit for bit, from poisoned static buffers: actors one below, at and
     one above a 16-row tile and over two tiles, the batch exactly at capacity, no edge, no lane, and large - small - large;
  2. the eager forward on the staged buffers under their row-id NoiseSpec against the eager forward of the UNPADDED batch under
     NoiseSpec(seed): real rows within 1e-5, the bound of test_scene_independence_and_sharding_invariance for a scene's rows in
     another batch -- four batches and the batch at capacity through ONE set of buffers, and the forward on the host twin moved to
     the device, bit for bit; two seeds; and `model.ood = True` (no fake rows, ten recurrences): stds, loc and pi, one batch;
  3. refusals."""
import pytest
import torch

import capacity_cases as CC
import helpers as H

pytestmark = pytest.mark.gpu
K, T = CC.K, CC.T
KEYS = ("loc", "pi", "diff_in", "diff_out")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    model, _ = H.build_model(K, T, 0.5, init_seed=6)
    H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
    return model.to(dev).eval()


@pytest.fixture(scope="module")
def buffers(model, dev):
    """ONE set of static buffers for the whole module"""
    from trajsde_amd import runtime
    return runtime.CapacityBuffers(CC.capacity(), K, dev, time_slots=21 + T, local_radius=float(model.encoder.local_radius))


FORWARD = {
    "4x13_mixed": lambda: CC._synth(S=4, n=13, L=4, F=T, box=60.0, seed=5, mixed_source=True),
    "1x40": lambda: CC._synth(S=1, n=40, L=5, F=T, box=80.0, seed=31),
    "3x13_irregular": lambda: H._irregular(S=3, n=13, L=5, F=T, box=60.0, seed=5),
    "single_actor_first": CC.single_actor_first,
    "at_capacity": CC.full_batch,
}


# ------------------------------------------------------------------------------------------------ 1. the staging launch
@pytest.mark.parametrize("name", list(CC.STAGING))
def test_staging_launch_is_the_host_twin(name, dev):
    from trajsde_amd import runtime
    batch = CC.STAGING[name]()
    cap = CC.capacity()
    sizes = runtime.BatchCapacity.sizes_of(batch)
    assert cap.fits(batch), cap.why_not(batch)
    assert {"n15": 15, "n16": 16, "n17": 17, "n33": 33, "at_capacity": 64}.get(name, sizes["actors"]) == sizes["actors"]
    if name == "at_capacity":
        assert sizes == dict(actors=cap.actors, scenes=cap.scenes, edges=cap.edges, lanes=cap.lanes, lane_edges=cap.lane_edges)
    if name == "no_edges":
        assert sizes["edges"] == 0
    if name == "no_lanes":
        assert sizes["lanes"] == 0 and sizes["lane_edges"] == 0
    static, ids = CC.poisoned_static(cap, dev)
    assert CC.stage(batch.to(dev), static, ids) == 0
    torch.cuda.synchronize()
    CC.assert_is_twin(static, ids, batch, cap, name)


def test_a_smaller_batch_after_a_larger_one_leaves_nothing_behind(dev):
    """large, small, large again from poisoned buffers: every call overwrites every element of every destination tensor and table"""
    cap = CC.capacity()
    static, ids = CC.poisoned_static(cap, dev)
    for name in ("at_capacity", "n15", "at_capacity", "no_edges", "n33"):
        batch = CC.STAGING[name]()
        assert CC.stage(batch.to(dev), static, ids) == 0
        torch.cuda.synchronize()
        CC.assert_is_twin(static, ids, batch, cap, name)


def test_capacity_buffers_stage_through_the_launch(buffers, dev):
    """the public route: CapacityBuffers.stage keeps every tensor's address and leaves the host twin's bytes"""
    before = {k: v.data_ptr() for k, v in buffers.batch.as_dict().items() if torch.is_tensor(v)}
    for name in ("n33", "n15"):
        batch = CC.STAGING[name]()
        buffers.stage(batch.to(dev))
        torch.cuda.synchronize()
        CC.assert_is_twin(buffers.batch, buffers.ids, batch, buffers.capacity, name)
        assert before == {k: v.data_ptr() for k, v in buffers.batch.as_dict().items() if torch.is_tensor(v)}


# ------------------------------------------------------------------------------------------------ 2. the forward on the staged buffers
@pytest.mark.parametrize("name", list(FORWARD))
def test_forward_on_the_staged_buffers_against_the_unpadded_forward(name, buffers, model, dev):
    from trajsde_amd import runtime
    from trajsde_amd.runtime import NoiseSpec
    batch = FORWARD[name]()
    assert buffers.fits(batch), buffers.why_not(batch)
    N, S = batch["x"].shape[0], batch["agent_index"].numel()
    if name == "at_capacity":
        assert (N, S) == (buffers.capacity.actors, buffers.capacity.scenes)      # it carries only the reserve
    for seed in (5, 77):
        _forward_case(name, batch, N, S, seed, buffers, model, dev)


def _forward_case(name, batch, N, S, seed, buffers, model, dev):
    from trajsde_amd import runtime
    from trajsde_amd.runtime import NoiseSpec
    ref = batch.to(dev)
    with torch.no_grad():
        want = model(ref, noise=NoiseSpec(seed=seed))
    buffers.stage(batch.to(dev))
    with torch.no_grad():
        got = model(buffers.batch, noise=buffers.noise(seed))
    real = {"loc": got["loc"][:, :N], "pi": got["pi"][:N], "diff_in": got["diff_in"][:S], "diff_out": got["diff_out"][:S]}
    diffs = {k: H.maxdiff(real[k], want[k]) for k in KEYS}
    print(name, seed, diffs, "graph path:", buffers.batch["_trajsde_graph"].graph_path())
    for k in KEYS:
        assert real[k].shape == want[k].shape, (name, k)
        assert diffs[k] < 1e-5, (name, k, diffs)
        assert bool(torch.isfinite(got[k]).all()), (name, k)                      # pad rows too
    assert torch.equal(got["reg_mask"][:N], want["reg_mask"]) and not bool(got["reg_mask"][N:].any())
    assert torch.equal(buffers.batch.y[:N], ref.y) and torch.equal(buffers.batch["rotate_mat"][:N], ref["rotate_mat"])
    # the launch's buffers and the host twin moved to the device are one input: the same words
    padded, ids = runtime.pad_batch_host(batch, buffers.capacity, K, buffers.radius)
    with torch.no_grad():
        twin = model(padded.to(dev), noise=NoiseSpec(seed=seed, **{k: v.to(dev) for k, v in ids.items()}))
    for k in KEYS:
        assert torch.equal(got[k], twin[k]), (name, k)
    from trajsde_amd import _lib
    torch.cuda.synchronize()
    _lib.check_range()


def test_ood_forward_on_the_staged_buffers_against_the_unpadded_ood_forward(buffers, dev):
    """`model.ood = True` (MODEL:89-98): a graph without fake rows, ten recurrences keyed through enc_row_ids, `stds` in the output"""
    from trajsde_amd.runtime import NoiseSpec
    model, _ = H.build_model(K, T, 0.5, init_seed=6)
    H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
    model = model.to(dev).eval()
    model.ood = True
    batch = FORWARD["3x13_irregular"]()
    N = batch["x"].shape[0]
    with torch.no_grad():
        want = model(batch.to(dev), noise=NoiseSpec(seed=9))
    buffers.stage(batch.to(dev))
    with torch.no_grad():
        got = model(buffers.batch, noise=buffers.noise(9))
    assert "stds" in got and "diff_in" not in got
    real = {"stds": got["stds"][:N], "loc": got["loc"][:, :N], "pi": got["pi"][:N]}
    diffs = {k: H.maxdiff(real[k], want[k]) for k in real}
    print("ood", diffs)
    for k, v in diffs.items():
        assert real[k].shape == want[k].shape and v < 1e-5, (k, diffs)
        assert bool(torch.isfinite(got[k]).all()), k


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals(buffers, dev):
    from trajsde_amd import _lib
    cap = CC.capacity()
    big = CC._synth(S=1, n=61, L=4, F=T, box=80.0, seed=3)             # 61 + 4 pad scenes > 64
    assert not buffers.fits(big)
    with pytest.raises(_lib.TrajsdeError, match="actors"):
        buffers.stage(big.to(dev))
    with pytest.raises(_lib.TrajsdeError, match="scenes"):
        buffers.stage(CC._synth(S=6, n=2, L=1, F=T, box=80.0, seed=3).to(dev))
    with pytest.raises(_lib.TrajsdeError, match="time slots"):
        buffers.stage(CC._synth(S=1, n=5, L=1, F=T + 1, box=80.0, seed=3).to(dev))
    with pytest.raises(_lib.TrajsdeError, match="must live on the GPU"):
        buffers.stage(CC._synth(S=1, n=5, L=1, F=T, box=80.0, seed=3))
    mixed = CC._synth(S=1, n=5, L=1, F=T, box=80.0, seed=3).to(dev)
    mixed["edge_index"] = mixed["edge_index"].cpu()                    # one host tensor among device tensors
    with pytest.raises(_lib.TrajsdeError, match="edge_index.*must live on the GPU"):
        buffers.stage(mixed)
    if torch.cuda.device_count() > 1:
        with pytest.raises(_lib.TrajsdeError, match="lives on cuda:1"):
            buffers.stage(CC._synth(S=1, n=5, L=1, F=T, box=80.0, seed=3).to("cuda:1"))
    assert CC.stage(big.to(dev), *CC.poisoned_static(cap, dev)) == -1   # the launch's own check, before any launch
    assert b"batch_pad: actors:" in _lib.lib().trajsde_last_error()
