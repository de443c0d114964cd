"""trajsde_encoder_cotangent_backward inside the red-zone arenas of tests/guarded_memory.py (-m gpu), by the harness of
tests/test_gpu_memory_contract.py: the batch, d_local and both diffusion cotangents placed in arenas of their own, every output, the
gradient buffers, the tape and the scratch routed into arenas.  For Nt = N + A one below, at and one above a multiple of 16 (63, 64,
65), for three single-actor scenes (E = 0) and for one actor alone: every guard byte intact, the inputs -- both cotangents included --
unwritten, and the results bit-identical whether the workspaces started as NaN, as zeros or as random bits.

A batch with A = 0 cannot be made for this entry point: A is the number of scenes (one fake agent per `agent_index` entry), the only
graph without fake rows is forward_ood's, and the entry point refuses it like trajsde_encoder_backward does (the refusal is asserted in
tests/test_gpu_encoder_cotangent.py; k_diff_cot itself validates every slot against A)."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
SEED = 6
T = 12
# name -> agents per scene: Nt = N + A = 63 / 64 / 65
ROWS = {"nt63": (20, 20, 20), "nt64": (20, 20, 21), "nt65": (20, 21, 21)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    import test_gpu_memory_contract as MC
    return MC.sde_model(1, T, dropout=0.0).to(dev)


def test_every_entry_point_of_the_table_runs_in_these_arenas():
    from trajsde_amd import _lib
    assert set(_lib.ENC_COT_EXT_SIGNATURES) == {"trajsde_encoder_cotangent_backward"}


def _contract(tag, model, batch, dev, side=None):
    """forward_train + encoder_cotangent_backward under test_gpu_memory_contract.contract; `side`: "in" / "out" leaves the other
    cotangent null"""
    import test_gpu_memory_contract as MC
    from trajsde_amd import _lib
    from trajsde_amd.runtime import D, NoiseSpec, rotate_inputs
    rt = model.encoder._rt
    on_dev = batch.to(dev)
    N, A = on_dev["x"].shape[0], int(on_dev["agent_index"].numel())
    rt.blob()                                                             # the weight images are packed outside the arenas, once
    rt.blob(_lib.STAGE_ENCODER_BWD)
    torch.cuda.synchronize()
    held, calls = {}, []
    g = torch.Generator().manual_seed(5)
    host = dict(d_local=torch.randn(N, D, generator=g), d_diff_in=torch.randn(A, D, generator=g), d_diff_out=torch.randn(A, D, generator=g))

    def make(gm, fill):
        for k, v in host.items():
            held[k] = gm.placed(v.to(dev), fill, label=k)
        return MC.place_batch(gm, on_dev, fill)

    def call(data):
        noise = NoiseSpec(seed=SEED)
        real = _lib.lib().trajsde_encoder_cotangent_backward
        _lib.lib().trajsde_encoder_cotangent_backward = lambda *a: (calls.append(1), real(*a))[1]
        try:
            with torch.no_grad():
                data["rotate_mat"], _ = rotate_inputs(data)
                outs, tape = rt.encoder_forward_train(data, noise)
                res = rt.encoder_cotangent_backward(data, held["d_local"], None if side == "out" else held["d_diff_in"],
                                                    None if side == "in" else held["d_diff_out"], noise, tape=tape, want_boundaries=True)
                again = rt.encoder_cotangent_backward(data, held["d_local"], None if side == "out" else held["d_diff_in"],
                                                      None if side == "in" else held["d_diff_out"], noise, want_boundaries=True)   # tape_valid = 0
                torch.cuda.synchronize()
        finally:
            _lib.lib().trajsde_encoder_cotangent_backward = real
        assert torch.equal(res["grads"].flat, again["grads"].flat)
        return ({"local": outs[0], "grads": res["grads"].flat, "d_latent": res["d_latent"], "d_aa_out": res["d_aa_out"],
                 "grads_recomputed": again["grads"].flat},
                [outs[0], res["grads"].flat, res["d_latent"], res["d_aa_out"], tape[0], again["grads"].flat, again["d_aa_out"]])
    call.after = lambda gm, data: MC.assert_graph_pointers(gm, data)
    MC.contract(tag, make, call)
    assert len(calls) == 2 * len(MC.FILL_RUNS)
    return held


@pytest.mark.parametrize("name", list(ROWS))
def test_row_counts_around_a_multiple_of_16(name, model, dev):
    import test_gpu_memory_contract as MC
    batch = MC.shape_case(ROWS[name], 1, T)
    assert batch["x"].shape[0] + int(batch["agent_index"].numel()) == {"nt63": 63, "nt64": 64, "nt65": 65}[name]
    _contract(f"encoder cotangent backward {name}", model, batch, dev)


@pytest.mark.parametrize("side", ["in", "out"])
def test_one_null_cotangent(side, model, dev):
    import test_gpu_memory_contract as MC
    _contract(f"encoder cotangent backward, d_diff_{side} only", model, MC.shape_case(ROWS["nt65"], 1, T), dev, side=side)


@pytest.mark.parametrize("name", ["lonely", "single"])
def test_no_edges_and_one_agent(name, model, dev):
    """three single-actor scenes (E = 0) and one scene with one actor (Nt = 2)"""
    import test_gpu_memory_contract as MC
    batch = MC.degenerate_batch(name, T)
    assert batch["edge_index"].shape[1] == 0
    _contract(f"encoder cotangent backward {name}", model, batch, dev)
