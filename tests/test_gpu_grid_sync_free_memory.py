"""The vanilla HiVT forward and `forward_ood` inside the red-zone arenas of tests/guarded_memory.py (-m gpu), by the harness of
tests/test_gpu_memory_contract.py, in BOTH forms of the graph without fake agents: sync-free (trajsde_graph_prepare_async: list lengths
on the device, record slots and grids sized from bounds) and exact (`set_sync_free(False)`: the form the contract suite ran these two
forwards in before they became sync-free, and now runs only for the SDE forward).  Batch, graph workspaces, rotation, stage workspaces
and outputs in arenas; NaN / zero / random workspace fills: no guard byte touched, no input changed, finite and bit-identical outputs.

Shapes: the smallest of that suite -- `nt61_k10_t12` (58 actors in three scenes, partial tiles everywhere) and the `isolated` degenerate
batch (targets of zero in-degree in the AA, AL and global attention next to targets with edges)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
K, T = 6, 12


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    return torch.device("cuda:0")


def _batch(name):
    import test_gpu_memory_contract as MC
    return MC._case_batch(name) if name in MC.SHAPE_CASES else MC.degenerate_batch(name, T)


def _run(tag, model, name, sync_free, dev, keys):
    import test_gpu_memory_contract as MC
    from trajsde_amd import runtime
    from trajsde_amd.runtime import GraphContext
    seen = []

    def form(m, data, out):
        gc = data[GraphContext.KEY]
        assert gc.batch.A == 0 and bool(gc.graph.exact) == (not sync_free)
        seen.append(1)
        return {}
    prev = runtime.set_sync_free(sync_free)
    try:
        assert runtime.sync_free() == sync_free
        MC.forward_contract(f"{tag} {name} [{'sync-free' if sync_free else 'exact'} graph]", model, _batch(name), dev, K, keys=keys,
                            fake_agents=False, extra=form)
    finally:
        runtime.set_sync_free(prev)
    assert len(seen) == len(MC.FILL_RUNS)


@pytest.mark.parametrize("sync_free", [True, False])
@pytest.mark.parametrize("name", ["nt61_k10_t12", "isolated"])
def test_vanilla_forward_in_both_graph_forms(name, sync_free, dev):
    """trajsde_encoder_grid_forward_train, trajsde_aggregator_forward_heads at 4 heads, trajsde_mlp_decoder_forward"""
    import test_gpu_memory_contract as MC
    model = MC.grid_model(K, T).to(dev)
    _run("vanilla forward", model, name, sync_free, dev, ("loc", "pi", "local_embed", "global_embed"))


@pytest.mark.parametrize("sync_free", [True, False])
@pytest.mark.parametrize("name", ["nt61_k10_t12", "isolated"])
def test_ood_forward_in_both_graph_forms(name, sync_free, dev):
    """trajsde_encoder_forward_ood (ten recurrences), trajsde_aggregator_forward_heads at 8 heads on split rows, trajsde_decoder_forward"""
    import test_gpu_memory_contract as MC
    model = MC.sde_model(K, T).to(dev)
    model.ood = True
    _run("forward_ood", model, name, sync_free, dev, ("loc", "pi", "stds"))
