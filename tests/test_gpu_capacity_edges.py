"""Staged batches (runtime.CapacityBuffers) at the padding's edges and through every consumer of a batch (-m gpu).
tests/test_gpu_capacity.py holds the eager SDE forward to the unpadded one at shapes where the padding is spread thin; here:

  A. concentrated padding (capacity_cases.CONCENTRATED, preconditions asserted on the host): a batch that fills the actor capacity
     leaves the permanent pad scene two actors, and all pad edges become two CSR rows of ONE duplicated sender -- 462 entries (the
     LDS bitonic network of sort_long_rows), 5290 (its global-memory network, no power of two) -- or 266 pad lane-actor edges on one
     actor.  The default forward builds the graph sync-free, so the lists are as long as the host's BOUND and the rows' tails beyond
     the true E go through the same sorts.  Forward against the unpadded forward (1e-5, two seeds, the host twin bit for bit), the
     compacted lists against the unpadded batch's as sets, the CSR invariants over pad rows too, then a thin batch through the same
     buffers;
  B. Monte-Carlo decoding: `predict_samples` on the buffers with `sample_stride = buffers.sample_stride` (K N_real) reproduces every
     sample of the unpadded call; with the default stride (K N_padded) only sample 0;
  C. the other consumers: `method: milstein`, bf16 state storage, the vanilla HiVT model, the metrics of driver.evaluate, and which
     way the graph stage built the CSR."""
import pytest
import torch

import capacity_cases as CC
import helpers as H

pytestmark = pytest.mark.gpu
K, T = CC.K, CC.T
KEYS = ("loc", "pi", "diff_in", "diff_out")
THIN = "4x13_mixed"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    """the trained-like weights of test_gpu_capacity.model"""
    model, _ = H.build_model(K, T, 0.5, init_seed=6)
    H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
    return model.to(dev).eval()


_BUFFERS = {}


def _buffers(cap, dev):
    """one set of static buffers per capacity for the whole module"""
    from trajsde_amd import runtime
    if cap not in _BUFFERS:
        _BUFFERS[cap] = runtime.CapacityBuffers(cap, K, dev, time_slots=21 + T, local_radius=CC.RADIUS)
    return _BUFFERS[cap]


def _case(name):
    """(capacity, batch) of the thin batch or of a concentrated case"""
    if name == "single_actor_first":
        return CC.capacity(), CC.single_actor_first()
    if name == THIN:
        return CC.capacity(), CC._synth(S=4, n=13, L=4, F=T, box=60.0, seed=5, mixed_source=True)
    return CC.concentrated(name)[:2]


def _real(out, N, S):
    return {"loc": out["loc"][:, :N], "pi": out["pi"][:N], "diff_in": out["diff_in"][:S], "diff_out": out["diff_out"][:S]}


def _sizes(batch):
    return batch["x"].shape[0], batch["agent_index"].numel()


# ------------------------------------------------------------------------------------------------ A. concentrated padding
def _lists(model, data, noise):
    """the compacted lists of the exact graph form (capture_intermediates), on the host"""
    model.encoder.capture_intermediates = True
    try:
        with torch.no_grad():
            model(data, noise=noise)
        return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in model.encoder.last_intermediates.items()}
    finally:
        model.encoder.capture_intermediates = False


def _check_lists(name, got, want, N, S, L, Np, Ap):
    """`got`: the lists of the staged batch, `want`: of the unpadded one.  Nodes of a snapshot: actors, then one fake row per scene."""
    from test_gpu_parity import _sorted_cols
    Nt, Ntp = N + S, Np + Ap

    def node(i):                                                         # a padded snapshot's node -> the unpadded one's, pad nodes -> -1
        i = i.to(torch.int64)
        return torch.where(i < N, i, torch.where((i >= Np) & (i < Np + S), i - Np + N, torch.full_like(i, -1)))

    lo = lambda v: int(v.min()) if v.numel() else 0
    hi = lambda v: int(v.max()) if v.numel() else -1
    t, i = torch.div(got["aa_dst"], Ntp, rounding_mode="floor").to(torch.int64), got["aa_dst"] % Ntp
    dst, src = node(i), node(got["aa_src"])
    # no pad edge survives: neither end of one is ever observed -- every entry of the snapshot lists and of the global list joins real nodes
    assert lo(dst) >= 0 and lo(src) >= 0, name
    assert got["E_aa"] == want["E_aa"] == want["aa_dst"].numel() and got["E_g"] == want["E_g"] and got["E_la"] == want["E_la"], name
    assert torch.equal(_sorted_cols(t * Nt + dst, src), _sorted_cols(want["aa_dst"], want["aa_src"])), name
    assert hi(got["g_src"]) < N and hi(got["g_dst"]) < N, name
    assert torch.equal(_sorted_cols(got["g_src"], got["g_dst"]), _sorted_cols(want["g_src"], want["g_dst"])), name
    # ... and no pad lane-actor edge: it lies outside the radius
    assert hi(got["la_lane"]) < L and hi(got["la_dst"]) < N, name
    assert torch.equal(_sorted_cols(got["la_lane"], got["la_dst"]), _sorted_cols(want["la_lane"], want["la_dst"])), name
    # over ALL rows, the pad rows included: target-major, senders ascending inside a row, segptr the bincount of the targets
    for d, s, segptr, rows in ((got["aa_dst"], got["aa_src"], got["aa_segptr"], 21 * Ntp), (got["g_dst"], got["g_src"], got["g_segptr"], Np),
                               (got["la_dst"], got["la_lane"], got["la_segptr"], Np)):
        assert segptr.numel() == rows + 1 and int(segptr[0]) == 0 and int(segptr[-1]) == d.numel(), name
        assert torch.equal(segptr[1:] - segptr[:-1], torch.bincount(d.to(torch.int64), minlength=rows).to(torch.int32)), name
        assert bool((d[1:] >= d[:-1]).all()), name
        same = d[1:] == d[:-1]
        assert bool((s[1:][same] >= s[:-1][same]).all()), name


@pytest.mark.parametrize("name", list(CC.CONCENTRATED))
def test_concentrated_padding_forward_lists_and_a_thin_batch_after_it(name, model, dev):
    import test_gpu_capacity as TGC
    from trajsde_amd import _lib
    from trajsde_amd.runtime import NoiseSpec
    cap, batch, twin, ids = CC.concentrated(name, float(model.encoder.local_radius))      # (its preconditions)
    buffers = _buffers(cap, dev)
    assert buffers.radius == float(model.encoder.local_radius)
    N, S = _sizes(batch)
    Np, Ap = cap.padded_sizes()[:2]
    for seed in (5, 77):                                                 # 1e-5 on the real rows, finite pad rows, the host twin bit for bit
        TGC._forward_case(name, batch, N, S, seed, buffers, model, dev)
    assert buffers.batch["_trajsde_graph"].graph_path() == "general"
    buffers.stage(batch.to(dev))
    got = _lists(model, buffers.batch, buffers.noise(5))
    want = _lists(model, batch.to(dev), NoiseSpec(seed=5))
    _check_lists(name, got, want, N, S, batch["lane_positions"].shape[0], Np, Ap)
    torch.cuda.synchronize()
    _lib.check_range()
    thin = CC.STAGING["n15"]()                                           # nothing of the long rows is left behind in a graph workspace
    assert buffers.fits(thin), buffers.why_not(thin)
    TGC._forward_case(name + ", then n15", thin, *_sizes(thin), 5, buffers, model, dev)


# ------------------------------------------------------------------------------------------------ B. Monte-Carlo decoding
@pytest.mark.parametrize("R", (3, 9, 17))
@pytest.mark.parametrize("name", (THIN, "lds_rows"))
def test_predict_samples_on_the_staged_buffers(name, R, model, dev):
    """R = 3: several paths per tile, 9: one path per tile, 17: two tiles with a one-sample tail"""
    import test_gpu_mc as MC
    from trajsde_amd.runtime import NoiseSpec
    cap, batch = _case(name)
    buffers = _buffers(cap, dev)
    N, S = _sizes(batch)
    with torch.no_grad():
        want = model.predict_samples(batch.to(dev), R, noise=NoiseSpec(seed=9), return_samples=True)
    ref = want["samples"]
    buffers.stage(batch.to(dev))
    assert buffers.sample_stride == K * N and buffers.batch["x"].shape[0] == cap.padded_sizes()[0] > N
    with torch.no_grad():
        got = model.predict_samples(buffers.batch, R, noise=buffers.noise(9), sample_stride=buffers.sample_stride, return_samples=True)
    assert tuple(got["samples"].shape) == (R, K, cap.padded_sizes()[0], T, 4)
    errs = [H.maxdiff(got["samples"][s][:, :N], ref[s]) for s in range(R)]
    print(f"[capacity edges] mc {name} R={R}:", " ".join(f"{e:.1e}" for e in errs))
    assert max(errs) < 1e-5, errs
    assert torch.equal(got["loc"], got["samples"][0])
    assert H.maxdiff(got["pi"][:N], want["pi"]) < 1e-5
    for k in ("samples", "loc_mean", "loc_cov"):
        assert bool(torch.isfinite(got[k]).all()), k                      # pad rows too
    MC._check_statistics({"loc_mean": got["loc_mean"][:, :N], "loc_cov": got["loc_cov"][:, :N]}, ref, R, 1e-5, f"staged {name}")
    # the default stride, K N_padded: sample 0 is still the forward's draw; the later samples are other draws -- finite, not the unpadded call's
    buffers.stage(batch.to(dev))
    with torch.no_grad():
        dflt = model.predict_samples(buffers.batch, R, noise=buffers.noise(9), return_samples=True)
    buffers.stage(batch.to(dev))
    with torch.no_grad():
        fwd = model(buffers.batch, noise=buffers.noise(9))
    assert torch.equal(dflt["samples"][0], fwd["loc"]) and torch.equal(dflt["loc"], fwd["loc"]) and torch.equal(got["loc"], fwd["loc"])
    assert bool(torch.isfinite(dflt["samples"][:, :, :N]).all())
    for s in range(1, R):
        assert H.maxdiff(dflt["samples"][s][:, :N], got["samples"][s][:, :N]) > 1e-3, s


# ------------------------------------------------------------------------------------------------ C. the other consumers
def _staged_against_unpadded(name, m, dev, seed=5, bound=1e-5):
    """the forward of `m` on the staged buffers against its forward on the unpadded batch -> (staged output, per-key differences)"""
    from trajsde_amd.runtime import NoiseSpec
    cap, batch = _case(name)
    buffers = _buffers(cap, dev)
    N, S = _sizes(batch)
    with torch.no_grad():
        want = m(batch.to(dev), noise=NoiseSpec(seed=seed))
    buffers.stage(batch.to(dev))
    with torch.no_grad():
        got = m(buffers.batch, noise=buffers.noise(seed))
    real = _real(got, N, S)
    diffs = {k: H.maxdiff(real[k], want[k]) for k in KEYS}
    for k in KEYS:
        assert real[k].shape == want[k].shape and bool(torch.isfinite(got[k]).all()), (name, k)
    assert torch.equal(got["reg_mask"][:N], want["reg_mask"]) and not bool(got["reg_mask"][N:].any())
    if bound is not None:
        for k in KEYS:
            assert diffs[k] < bound, (name, k, diffs)
    return got, want, diffs


@pytest.mark.parametrize("name", (THIN, "lds_rows"))
def test_milstein_forward_on_the_staged_buffers(name, dev):
    """configured as test_gpu_mc._variant_case: both stochastic stages under `method: milstein`"""
    from trajsde_amd import _lib
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    cfg = H.our_cfg(K, T, 0.5)
    cfg["decoder"]["kwargs"]["method"] = cfg["encoder"]["kwargs"]["method"] = "milstein"
    m = PredictionModelSDENet(**cfg, init_seed=7).eval().to(dev)
    assert m.decoder.method == "milstein"
    _, _, diffs = _staged_against_unpadded(name, m, dev)
    print("[capacity edges] milstein", name, diffs)
    torch.cuda.synchronize()
    _lib.check_range()


@pytest.mark.parametrize("name", ("single_actor_first", "lds_rows"))
def test_bf16_state_forward_on_the_staged_buffers(name, model, dev):
    """bf16 state storage rounds the recurrence's state, which may amplify a difference in summation order: the bound against the
    unpadded forward is twice what the SAME scenes show inside another REAL batch (the batch and one more scene of 7 actors behind
    it, the batch's rows keyed as in the unpadded call) -- the scene-independence comparison, under bf16, per output.
    Observed on one MI355X: 0 in every output for both batches, staged and embedded."""
    from trajsde_amd import runtime
    from trajsde_amd.data import collate
    from trajsde_amd.runtime import NoiseSpec
    cap, batch = _case(name)
    buffers = _buffers(cap, dev)
    N, S = _sizes(batch)
    assert runtime.set_state_storage("bf16") == "fp32"
    try:
        got, want, diffs = _staged_against_unpadded(name, model, dev, bound=None)
        scenes = CC.single_actor_first_scenes() if name == "single_actor_first" else CC.lds_rows_scenes()
        assert all(torch.equal(collate(scenes)[k], batch[k]) for k in ("x", "edge_index", "lane_actor_index"))
        other = collate(scenes + [CC._synth(S=1, n=7, L=3, F=T, box=60.0, seed=900)])
        N2, S2 = _sizes(other)
        assert (N2, S2) == (N + 7, S + 1) and torch.equal(other["x"][:N], batch["x"])
        with torch.no_grad():
            inside = model(other.to(dev), noise=NoiseSpec(seed=5, **{k: v.to(dev) for k, v in CC.embedded_ids(N, S, N2, S2).items()}))
        figure = {k: H.maxdiff(_real(inside, N, S)[k], want[k]) for k in KEYS}
        print("[capacity edges] bf16", name, "staged - unpadded:", diffs, "| inside another batch - unpadded:", figure)
        padded, ids = runtime.pad_batch_host(batch, cap, K, buffers.radius)
        with torch.no_grad():
            twin = model(padded.to(dev), noise=NoiseSpec(seed=5, **{k: v.to(dev) for k, v in ids.items()}))
        for k in KEYS:
            assert torch.equal(got[k], twin[k]), (name, k)                # the launch's buffers and the host twin: the same words
            assert diffs[k] <= 2.0 * figure[k], (name, k, diffs, figure)
    finally:
        runtime.set_state_storage("fp32")
    with torch.no_grad():
        fp32_loc = model(batch.to(dev), noise=NoiseSpec(seed=5))["loc"]
    assert H.maxdiff(fp32_loc, want["loc"]) > 1e-6                        # (the state really went through bf16)


@pytest.mark.parametrize("name", (THIN, "lds_rows"))
def test_vanilla_hivt_forward_on_the_staged_buffers(name, dev):
    """the deterministic variant takes the same batch (no fake rows, no noise): real rows of loc and pi within 1e-5, pad rows finite"""
    from trajsde_amd import _lib
    from trajsde_amd.models.model_base_mix import PredictionModel
    m = PredictionModel(**H.grid_cfg(K, T, 4, 2), init_seed=9).eval().to(dev)
    cap, batch = _case(name)
    buffers = _buffers(cap, dev)
    assert float(m.encoder.local_radius) == buffers.radius
    N, _ = _sizes(batch)
    with torch.no_grad():
        want = m(batch.to(dev))
    buffers.stage(batch.to(dev))
    with torch.no_grad():
        got = m(buffers.batch)
    diffs = {"loc": H.maxdiff(got["loc"][:, :N], want["loc"]), "pi": H.maxdiff(got["pi"][:N], want["pi"])}
    print("[capacity edges] vanilla", name, diffs)
    assert got["loc"].shape[1] == cap.padded_sizes()[0] and want["loc"].shape[1] == N
    for k, v in diffs.items():
        assert v < 1e-5, (name, k, diffs)
        assert bool(torch.isfinite(got[k]).all()), (name, k)
    assert float(want["loc"].abs().max()) > 1e-2
    torch.cuda.synchronize()
    _lib.check_range()


def test_driver_metrics_over_staged_batches(dev):
    """driver.evaluate seeds each batch with NoiseSpec(seed + i) and indexes the outputs with the batch's own agent_index: it has no
    way to take the row-id noise of staged buffers or to leave the pad scenes' agents out, so the metrics are updated here from the
    staged outputs sliced to the real agents and compared with driver.evaluate over the unpadded batches -- within 1e-4, the bound of
    test_gpu_parity.test_driver_metrics_match_oracle"""
    from trajsde_amd import driver
    cfg = H.our_cfg(K, T, 0.5)
    for m in cfg["metric_args"]:
        m["end_idcs"] = [T - 1, T - 1]
    model = driver.build_model(cfg, None, dev, init_seed=0)
    H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
    model.eval()
    cap = CC.capacity()
    buffers = _buffers(cap, dev)
    batches = [_case(THIN)[1], CC.single_actor_first(), _case("lds_rows")[1]]
    want = driver.evaluate(model, [b.to(dev) for b in batches], seed=40)
    for metric in model.metrics_vl:
        metric.reset()
    for i, b in enumerate(batches):
        S = b["agent_index"].numel()
        buffers.stage(b.to(dev))
        with torch.no_grad():
            out = model(buffers.batch, noise=buffers.noise(40 + i))
        idx = buffers.batch["agent_index"][:S]
        assert torch.equal(idx.cpu(), b["agent_index"])
        for metric in model.metrics_vl:
            metric.update(out["loc"][:, idx, :, :2], buffers.batch.y[idx], out["reg_mask"][idx], buffers.batch["source"][:S])
    got = model.metric_results()
    print("[capacity edges] metrics", got, want)
    assert set(want) == set(got) and {"ADE_T", "FDE_T", "MR_T"} <= set(want)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-4, (k, got, want)
    assert want["ADE_T"] > 1e-2


@pytest.mark.parametrize("name", (THIN, "at_capacity", "lds_rows"))
def test_staged_batches_take_the_general_graph_path(name, model, dev):
    """a padded edge list is not in dataset order -- also when the batch brings every edge the capacity holds: the pad scenes have
    actors and no edge -- so the closed-form CSR stands down on the device; the same batch unpadded takes it"""
    from trajsde_amd.runtime import NoiseSpec
    cap, batch = (CC.capacity(), CC.full_batch()) if name == "at_capacity" else _case(name)
    buffers = _buffers(cap, dev)
    ref = batch.to(dev)
    with torch.no_grad():
        model(ref, noise=NoiseSpec(seed=5))
    assert ref["_trajsde_graph"].graph_path() == "direct"
    buffers.stage(batch.to(dev))
    with torch.no_grad():
        model(buffers.batch, noise=buffers.noise(5))
    assert buffers.batch["_trajsde_graph"].graph_path() == "general"
