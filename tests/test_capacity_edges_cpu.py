"""Staged batches at the padding's edges, the parts that need no GPU (tests/test_gpu_capacity_edges.py holds the kernels to the same
cases):

  1. concentrated padding -- a batch that fills the actor capacity, so that every pad edge (or pad lane-actor edge) lands on the two
     reserve actors of the permanent pad scene (capacity_cases.CONCENTRATED: rows of 462 and of 5290 copies of one sender, 266 pad
     lane-actor edges on one actor) -- is inert in the reference's semantics: `oracle/restate.forward` on the batch and on
     pad_batch_host's twin under the row-id noise, real rows within 1e-5, exactly as test_capacity_cpu.test_padding_is_inert_in_the_oracle;
  2. Monte-Carlo decoding on a padded batch: which Philox rows sample s of a real (mode, actor) draws under sample_stride = K * N_real
     (those of the unpadded batch under its default stride) and under the default K * N_padded (not those), and what they coincide
     with; `restate.sde_decoder` on the twin under the shifted ids against the unpadded batch under its shifted rows."""
import numpy as np
import pytest
import torch

import capacity_cases as CC
import helpers as H

K, T = CC.K, CC.T
SEED = 123
KEYS = ("loc", "pi", "diff_in", "diff_out")


@pytest.fixture(scope="module")
def trained_model():
    """test_capacity_cpu.trained_model at this module's future steps"""
    model, cfg = H.build_model(K, T, 0.5, init_seed=3)
    H.trained_like_parameters(model, 17, 1.0)
    return model, cfg


_RUNS = {}


def _oracle_runs(name, trained_model):
    """(cap, batch, twin, ids, oracle forward of the batch, oracle forward of the twin under the row-id noise), once per case"""
    if name not in _RUNS:
        import restate
        model, cfg = trained_model
        radius = float(cfg["encoder"]["kwargs"]["local_radius"])
        assert radius == CC.RADIUS
        cap, batch, twin, ids = CC.concentrated(name, radius)
        P = {k: v.detach().clone() for k, v in model.state_dict().items()}
        want = restate.forward(P, cfg, H.clone_batch(batch), restate.PhiloxNoise(SEED), want_intermediates=True)
        got = restate.forward(P, cfg, H.clone_batch(twin), restate.PhiloxNoise(SEED, enc_row_ids=ids["enc_row_ids"].numpy(),
                                                                               dec_row_ids=ids["dec_row_ids"].numpy(),
                                                                               fake_row_ids=ids["fake_row_ids"].numpy()),
                              want_intermediates=True)
        _RUNS[name] = (cap, batch, twin, ids, want, got, P)
    return _RUNS[name]


# ------------------------------------------------------------------------------------------------ 1. concentrated padding
@pytest.mark.parametrize("name", list(CC.CONCENTRATED))
def test_concentrated_padding_is_inert_in_the_oracle(name, trained_model):
    """observed (this test prints them): the largest of the four differences is 1.2e-7 for lds_rows (diff_out; loc and
    pi 0), 2.4e-6 for global_rows (loc; pi 1.2e-6) and 9.5e-7 for lane_rows (loc) -- fp32 summation order in BLAS at another row count"""
    cap, batch, twin, ids, want, got, _ = _oracle_runs(name, trained_model)
    N, S = batch["x"].shape[0], batch["agent_index"].numel()
    Np, Ap = cap.padded_sizes()[:2]
    diffs = {"loc": H.maxdiff(got["loc"][:, :N], want["loc"]), "pi": H.maxdiff(got["pi"][:N], want["pi"]),
             "diff_in": H.maxdiff(got["diff_in"][:S], want["diff_in"]), "diff_out": H.maxdiff(got["diff_out"][:S], want["diff_out"])}
    print("[capacity edges] oracle", name, diffs)
    assert want["loc"].shape[1] == N and got["loc"].shape[1] == Np and got["diff_in"].shape[0] == Ap
    for k, v in diffs.items():
        assert v < 1e-5, (name, k, v)
    assert torch.equal(got["reg_mask"][:N], want["reg_mask"]) and not bool(got["reg_mask"][N:].any())
    for k in KEYS:
        assert bool(torch.isfinite(got[k]).all()), (name, k)
    # what the graph stage has to make of the padding: no pad edge in any snapshot list or in the global list (neither end is ever
    # observed), no pad lane-actor edge (outside the radius) -- the oracle's lists of the twin name real actors and real lanes only
    Nt = Np + Ap
    aa = got["aa_edge_list"]
    assert bool(((aa[0] % Nt < N) | (aa[0] % Nt >= Np)).all()) and bool(((aa[1] % Nt < N) | (aa[1] % Nt >= Np)).all())
    assert got["g_edge_list"].numel() == 0 or int(got["g_edge_list"].max()) < N
    al = got["al_edge_list"]
    assert al.shape[1] == want["al_edge_list"].shape[1]
    assert al.numel() == 0 or (int(al[1].max()) < N and int(al[0].max()) < batch["lane_positions"].shape[0])


# ------------------------------------------------------------------------------------------------ 2. Monte-Carlo decoding
def _thin():
    return CC.capacity(), CC._synth(S=4, n=13, L=4, F=T, box=60.0, seed=5, mixed_source=True)


@pytest.mark.parametrize("R", (2, 17))
@pytest.mark.parametrize("name", ("4x13_mixed", "lds_rows"))
def test_sample_ids_of_the_real_rows_under_the_real_stride(name, R):
    """sample s of decoder row r draws Philox row dec_row_ids[r] + s D.  With D = K N_real the real rows of a padded batch draw, in
    every sample, what the unpadded batch draws under its default stride; no two real (row, sample) pairs share an id; the ids a
    real row of sample s >= 1 does share are pad rows' of EARLIER samples (pad ids start at K N_real: those of sample s - 1 are the
    first K (N_padded - N_real) real ids of sample s), whose draws nobody reads.  With the default D = K N_padded nothing is shared
    at all, and the real rows of every sample past the first draw other rows than the unpadded batch's."""
    from trajsde_amd import runtime
    cap, batch = _thin() if name == "4x13_mixed" else CC.concentrated(name)[:2]
    N = batch["x"].shape[0]
    Np = cap.padded_sizes()[0]
    tables = runtime.pad_batch_host(batch, cap, K, CC.RADIUS)[1]
    for k, v in CC.embedded_ids(N, batch["agent_index"].numel(), Np, cap.padded_sizes()[1]).items():
        assert torch.equal(tables[k], v), k                                          # (the rule, written down a second time)
    dec = tables["dec_row_ids"].long().view(K, Np)
    s = torch.arange(R)[:, None, None]
    unpadded = torch.arange(K * N).view(1, K, N) + s * (K * N)                       # the unpadded call, default stride
    D = K * N
    ids = dec[None] + s * D                                                          # [R, K, Np]
    real, pad = ids[:, :, :N], ids[:, :, N:]
    assert torch.equal(real, unpadded)
    assert int(ids.max()) < 2 ** 32 and real.unique().numel() == real.numel() and pad.unique().numel() == pad.numel()
    sample_of_pad = dict(zip(pad.reshape(-1).tolist(), s.expand_as(pad).reshape(-1).tolist()))
    shared = 0
    for smp in range(R):
        for i in real[smp].reshape(-1).tolist():
            if i in sample_of_pad:
                assert sample_of_pad[i] < smp, (i, smp)
                shared += 1
    assert shared > 0 and sample_of_pad[K * N] == 0                                  # the overlap is there: real ids of sample 1
    assert not bool(torch.isin(pad[0], real[0]).any())                               # ... and never inside one sample
    # the default stride of the padded tensor
    ids_default = dec[None] + s * (K * Np)
    assert ids_default.unique().numel() == ids_default.numel()
    assert torch.equal(ids_default[0, :, :N], unpadded[0])
    for smp in range(1, R):
        assert not bool((ids_default[smp, :, :N] == unpadded[smp]).any())
    runtime.mc_check_arguments(R, K * Np, D)                                         # the explicit stride is accepted


@pytest.mark.parametrize("s", (0, 1, 16))
def test_oracle_decoder_sample_on_the_padded_twin(s, trained_model):
    """restate.sde_decoder on lds_rows' twin (its own embeddings) under dec_row_ids + s K N_real against the unpadded batch under
    the rows arange(K N) + s K N (test_gpu_mc.ShiftedDecoderNoise's): the real rows of sample s agree within 1e-5"""
    import restate
    from trajsde_amd.schedule import decoder_schedule
    cap, batch, twin, ids, want0, got0, P = _oracle_runs("lds_rows", trained_model)
    c = restate.flat_cfg(trained_model[1])
    sched = decoder_schedule(c["future_steps"], c["max_fut_t"], c["min_stepsize"])
    N = batch["x"].shape[0]
    rows = K * N
    want = restate.sde_decoder(P, c, batch, want0["local_embed"], want0["global_embed"],
                               restate.PhiloxNoise(SEED, dec_row_ids=np.arange(rows) + s * rows), sched)
    got = restate.sde_decoder(P, c, twin, got0["local_embed"], got0["global_embed"],
                              restate.PhiloxNoise(SEED, dec_row_ids=ids["dec_row_ids"].numpy().astype(np.int64) + s * rows), sched)
    d = H.maxdiff(got["loc"][:, :N], want["loc"])
    print("[capacity edges] oracle decoder, sample", s, d)
    assert d < 1e-5, (s, d)
    assert bool(torch.isfinite(got["loc"]).all())
    if s == 0:
        assert torch.equal(want["loc"], want0["loc"]) and torch.equal(got["loc"], got0["loc"])
    else:
        assert H.maxdiff(want["loc"], want0["loc"]) > 1e-2                           # another draw
