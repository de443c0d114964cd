"""GPU suite of Monte-Carlo decoding (-m gpu): trajsde_decoder_forward_mc (csrc/decoder_mc.hip) through
runtime.StageRuntime.decoder_forward_mc, SDEDecoder.sample and PredictionModelSDENet.predict_samples.

The contract: sample s of path r = k N + n is the plain decoder's solve with the Philox counter row rid(r) + s D.  So sample 0 is the
plain forward's draw, sample s is the plain decoder's draw under NoiseSpec(seed, dec_row_ids = ids + s D), and both references exist
without the new kernel: the float64 oracle (oracle/restate.py) driven by a noise source with the shifted rows, and the existing decoder
entry point.  The statistics are compared with runtime.mc_statistics_host (float64) of those references' samples.

Shapes: synth(S=2, n=7, L=4, F=5, box=60, seed=5) -> N = 14, K = 3: 42 paths (a partial last path tile in the plain kernels), T = 5,
R in {2, 16, 17, 33}: a partial sample tile, exactly one tile, two and three tiles with a one-sample tail -- and 3, 4, 8, 9: up to
R = 8 a tile holds several paths (groups of 2, 4 or 8 rows: 21, 11 and 6 tiles for the 42 paths, the last one partial each time), with
full and partial groups; 9 is the first R with one path per tile."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
K, T, MAX_T = 3, 5, 0.5
SEED = 77
RS = (2, 3, 4, 8, 9, 16, 17, 33)
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class ShiftedDecoderNoise:
    """restate noise source of sample s: the decoder's rows are arange(K N) + s K N of the Philox stream; fake agents and the encoder
    draw what restate.PhiloxNoise(seed) draws"""

    def __init__(self, seed, s, rows):
        import restate
        self.inner, self.seed, self.s, self.rows = restate.PhiloxNoise(seed), seed, s, rows

    def fake_agent(self, shape):
        return self.inner.fake_agent(shape)

    def encoder(self, idx, shape):
        return self.inner.encoder(idx, shape)

    def decoder(self, k, shape):
        from trajsde_amd import philox
        assert tuple(shape) == (self.rows, 64)
        return torch.from_numpy(philox.normals(self.seed, philox.STREAM_DECODER, k, np.arange(self.rows) + self.s * self.rows, 64))


def _batch():
    from trajsde_amd.synth import synth
    return synth(S=2, n=7, L=4, F=T, box=60.0, seed=5)


def _embeddings(model, data, seed=SEED):
    """(local_embed, global_embed) of the model's own encoder and interactor on the device"""
    from trajsde_amd.runtime import NoiseSpec, rotate_inputs
    data["rotate_mat"], _ = rotate_inputs(data)
    local = model.encoder(data=data, noise=NoiseSpec(seed=seed))[0]
    return local, model.aggregator(data=data, local_embed=local, noise=NoiseSpec(seed=seed))


def _decoder_samples(model, data, local, glob, R, seed=SEED, ids=None, stride=None):
    """[R,K,N,T,C] from R calls of the EXISTING decoder entry point under row ids shifted by s * stride"""
    from trajsde_amd.runtime import NoiseSpec
    rows = int(model.decoder.num_modes) * local.shape[0]
    ids = torch.arange(rows, dtype=torch.int64, device=local.device) if ids is None else ids.to(torch.int64)
    stride = rows if stride is None else stride
    outs = []
    for s in range(R):
        shifted = (ids + s * stride).to(torch.int32).contiguous()
        outs.append(model.decoder(data=data, local_embed=local, global_embed=glob, noise=NoiseSpec(seed=seed, dec_row_ids=shifted))["loc"])
    return torch.stack(outs)


@pytest.fixture(scope="module")
def case(dev):
    """the model, the batch on the device, its embeddings, and the existing decoder's samples for s < 33 -- computed once"""
    model, cfg = H.build_model(K, T, MAX_T, init_seed=7)
    batch = _batch()
    model = model.to(dev)
    data = H.clone_batch(batch).to(dev)
    local, glob = _embeddings(model, data)
    ref = _decoder_samples(model, data, local, glob, max(RS))
    torch.cuda.synchronize()
    return dict(model=model, cfg=cfg, batch=batch, data=data, local=local, glob=glob, ref=ref, N=batch.num_nodes)


@pytest.fixture(scope="module")
def oracle17(case):
    """[17,K,N,T,4] float64: restate.forward under ShiftedDecoderNoise(s) for s < 17.  Samples 0 and 16 are whole runs of
    H.oracle_forward64; the encoder and the interactor do not see the decoder's noise, so samples 1 .. 15 call the same
    restate.sde_decoder that restate.forward calls, on sample 0's own float64 embeddings -- asserted below to be bit for bit the whole
    run for s = 16 (seventeen whole runs are seventeen identical encoder recurrences, half a minute of host time).  For s = 0 the
    source's rows are arange(K N): restate.PhiloxNoise(seed) itself, the plain oracle forward."""
    import restate
    from trajsde_amd.schedule import decoder_schedule
    model, cfg, batch = case["model"], case["cfg"], case["batch"]
    rows = K * case["N"]
    first = H.oracle_forward64(model, cfg, batch, noise=ShiftedDecoderNoise(SEED, 0, rows))
    last = H.oracle_forward64(model, cfg, batch, noise=ShiftedDecoderNoise(SEED, 16, rows), want_intermediates=False)
    P = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone()) for k, v in model.state_dict().items()}
    c = restate.flat_cfg(cfg)
    sched = decoder_schedule(c["future_steps"], c["max_fut_t"], c["min_stepsize"])
    b64 = H.double_batch(batch)

    def solve(s):
        return restate.sde_decoder(P, c, b64, first["local_embed"], first["global_embed"], H.Float64Noise(ShiftedDecoderNoise(SEED, s, rows)),
                                   sched)["loc"]
    assert torch.equal(solve(16), last["loc"])
    return dict(samples=torch.stack([first["loc"]] + [solve(s) for s in range(1, 16)] + [last["loc"]]), first=first)


def _tolerances(ref, R, delta):
    """(mean tolerance, covariance tolerance, largest per-element std of the reference samples [R, ..., >= 2])"""
    x = ref.double()[..., :2]
    d = float((x - x.mean(0)).abs().max())
    return delta, 4.0 * delta * d * R / (R - 1) + 8.0 * R * EPS32 * d * d, float(x.std(0, unbiased=True).max())


def _check_statistics(out, ref, R, delta, what):
    from trajsde_amd.runtime import mc_statistics_host
    mean, cov = (t.cpu() for t in mc_statistics_host(ref))
    tol_m, tol_c, std = _tolerances(ref, R, delta)
    dm, dc = H.maxdiff(out["loc_mean"].cpu(), mean), H.maxdiff(out["loc_cov"].cpu(), cov)
    print(f"[mc] {what} R={R}: mean err {dm:.3e} (tol {tol_m:.1e}), cov err {dc:.3e} (tol {tol_c:.3e}), largest std {std:.3f}")
    assert std >= 100.0 * tol_c, (what, R, std, tol_c)          # a pass cannot be vacuous
    assert tuple(out["loc_mean"].shape) == tuple(mean.shape) and tuple(out["loc_cov"].shape) == tuple(cov.shape)
    assert dm <= tol_m, (what, R, dm)
    assert dc <= tol_c, (what, R, dc, tol_c)


# ----------------------------------------------------------------------------------------------------------------- 1. golden, sample 0
@pytest.mark.parametrize("name", H.GOLDEN)
def test_sample_zero_matches_golden(name, dev):
    """every golden fixture (the `uncertain: False` one included: two channels), the decoder fed the reference's own embeddings"""
    from trajsde_amd.runtime import NoiseSpec
    batch, meta, out, mid = H.load_fixture(name)
    model, cfg = H.build_model(meta)
    model = model.to(dev)
    data = batch.to(dev)
    got = model.decoder.sample(data, mid["local_embed"].to(dev), mid["global_embed"].to(dev), 2, noise=NoiseSpec(seed=int(meta["noise_seed"])),
                               return_samples=True)
    assert tuple(got["samples"].shape) == (2,) + tuple(out["loc"].shape) and tuple(got["loc_mean"].shape) == tuple(out["loc"].shape)
    assert tuple(got["loc_cov"].shape) == tuple(out["loc"].shape[:3]) + (3,)
    assert H.maxdiff(got["samples"][0].cpu(), out["loc"]) <= 1e-4
    assert H.maxdiff(got["loc"].cpu(), out["loc"]) <= 1e-4
    assert H.maxdiff(got["pi"].cpu(), out["pi"]) <= 1e-4
    if "reg_mask" in out:
        assert torch.equal(got["reg_mask"].cpu(), out["reg_mask"])


# ----------------------------------------------------------------------------------------------------------------- 2. oracle, every sample
def test_every_sample_matches_the_oracle(case, oracle17):
    from trajsde_amd.runtime import NoiseSpec
    got = case["model"].predict_samples(H.clone_batch(case["batch"]).to(case["data"]["x"].device), 17, noise=NoiseSpec(seed=SEED),
                                        return_samples=True)
    assert tuple(got["samples"].shape) == (17, K, case["N"], T, 4)
    errs = [H.maxdiff(got["samples"][s].cpu(), oracle17["samples"][s]) for s in range(17)]
    print("[mc] oracle, per sample:", " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= 1e-4, errs
    first = oracle17["first"]
    for k in ("pi", "diff_in", "diff_out"):
        assert H.maxdiff(got[k].cpu(), first[k]) <= 1e-4, k
    _check_statistics(got, oracle17["samples"], 17, 1e-4, "oracle")


# ----------------------------------------------------------------------------------------------------------------- 3. the existing decoder
@pytest.mark.parametrize("R", RS)
def test_samples_match_the_existing_decoder(R, case):
    """default ids and default stride: samples[s] is decoder_forward under NoiseSpec(seed, dec_row_ids = arange(K N) + s K N); the
    statistics against mc_statistics_host of those samples, and word for word the same without the samples buffer"""
    from trajsde_amd.runtime import NoiseSpec
    m = case["model"]
    got = m.decoder.sample(case["data"], case["local"], case["glob"], R, noise=NoiseSpec(seed=SEED), return_samples=True)
    ref = case["ref"][:R]
    errs = [H.maxdiff(got["samples"][s], ref[s]) for s in range(R)]
    print(f"[mc] decoder R={R}:", " ".join(f"{e:.1e}" for e in errs))
    assert max(errs) <= 1e-5, errs
    assert H.maxdiff(got["loc"], ref[0]) <= 1e-5 and torch.equal(got["loc"], got["samples"][0])
    _check_statistics(got, ref, R, 1e-5, "decoder")
    lean = m.decoder.sample(case["data"], case["local"], case["glob"], R, noise=NoiseSpec(seed=SEED))
    assert "samples" not in lean
    for k in ("loc", "pi", "loc_mean", "loc_cov"):
        assert torch.equal(lean[k], got[k]), k


@pytest.mark.parametrize("R", RS)
def test_caller_row_ids_and_explicit_stride(R, case):
    """caller ids = a non-identity permutation plus a base offset, D larger than K N"""
    from trajsde_amd.runtime import NoiseSpec
    m, rows = case["model"], K * case["N"]
    g = torch.Generator().manual_seed(3)
    perm = torch.randperm(rows, generator=g)
    assert not torch.equal(perm, torch.arange(rows))
    ids = (perm + 100000).to(case["local"].device)
    D = rows + 11
    got = m.decoder.sample(case["data"], case["local"], case["glob"], R, noise=NoiseSpec(seed=SEED, dec_row_ids=ids.to(torch.int32)),
                           sample_stride=D, return_samples=True)
    ref = _decoder_samples(m, case["data"], case["local"], case["glob"], R, ids=ids, stride=D)
    errs = [H.maxdiff(got["samples"][s], ref[s]) for s in range(R)]
    assert max(errs) <= 1e-5, errs
    assert H.maxdiff(ref[0], case["ref"][0]) > 1e-3             # the ids matter: not the default stream
    _check_statistics(got, ref, R, 1e-5, "decoder, caller ids")


# ----------------------------------------------------------------------------------------------------------------- 4. injected normals
@pytest.mark.parametrize("R", RS)
def test_injected_normals_give_the_in_kernel_samples(R, case):
    from trajsde_amd import philox
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.schedule import decoder_schedule
    m, rows = case["model"], K * case["N"]
    sched = decoder_schedule(T, MAX_T)
    z = torch.from_numpy(np.stack([philox.normals(SEED, philox.STREAM_DECODER, k, np.arange(R * rows), 64)
                                   for k in range(sched.n_euler)])).to(case["local"].device)
    assert tuple(z.shape) == (sched.n_euler, R * rows, 64)
    got = m.decoder.sample(case["data"], case["local"], case["glob"], R, noise=NoiseSpec(seed=0, z_dec=z), return_samples=True)
    assert H.maxdiff(got["samples"], case["ref"][:R]) <= 1e-5
    _check_statistics(got, case["ref"][:R], R, 1e-5, "injected")
    from trajsde_amd import _lib
    with pytest.raises(_lib.TrajsdeError, match="z_dec"):
        m.decoder.sample(case["data"], case["local"], case["glob"], R, noise=NoiseSpec(seed=0, z_dec=z[:, :rows].contiguous()))


# ----------------------------------------------------------------------------------------------------------------- 5. statistics, large offset
@pytest.mark.parametrize("R", RS)
def test_statistics_survive_a_large_common_offset(R, dev):
    """decoder.decoder.3.bias = (1000, -1000) at trained-like parameters: every sample of x sits near 1000, of y near -1000, spread
    ~0.3.  A variance formed as sum x^2 - (sum x)^2 / R errs by ~R 1e6 eps32 ~ 1 there; deviations from a mean do not (the last
    assertion forms that sum of squares in fp32 on the same samples and sees it miss the bound)."""
    from trajsde_amd.runtime import NoiseSpec
    model, cfg = H.build_model(K, T, MAX_T, init_seed=7)
    H.trained_like_parameters(model, 3)
    with torch.no_grad():
        dict(model.named_parameters())["decoder.decoder.3.bias"].copy_(torch.tensor([1000.0, -1000.0]))
    model = model.to(dev)
    data = _batch().to(dev)
    local, glob = _embeddings(model, data)
    ref = _decoder_samples(model, data, local, glob, R)
    assert float(ref[..., 0].min()) > 900.0 and float(ref[..., 1].max()) < -900.0
    got = model.decoder.sample(data, local, glob, R, noise=NoiseSpec(seed=SEED), return_samples=True)
    assert H.maxdiff(got["samples"], ref) <= 1e-4
    _check_statistics(got, ref, R, 1e-4, "offset 1000")
    # teeth: the sum-of-squares form in fp32 on the same samples misses the same bound
    x = ref[..., 0]
    naive = (x.pow(2).sum(0) - x.sum(0).pow(2) / R) / (R - 1)
    from trajsde_amd.runtime import mc_statistics_host
    assert H.maxdiff(naive.cpu(), mc_statistics_host(ref)[1][..., 0].cpu()) > _tolerances(ref, R, 1e-4)[1]


# ----------------------------------------------------------------------------------------------------------------- 6. reproducibility
@pytest.mark.parametrize("R", RS)
def test_identical_calls_are_bitwise_identical(R, case):
    from trajsde_amd.runtime import NoiseSpec
    m = case["model"]

    def run(noise):
        return m.decoder.sample(case["data"], case["local"], case["glob"], R, noise=noise, return_samples=True)
    a, b = run(NoiseSpec(seed=SEED)), run(NoiseSpec(seed=SEED))
    c = run(NoiseSpec(seed=0, seed_dev=torch.tensor([SEED], dtype=torch.int64, device=case["local"].device)))
    for k in ("loc", "pi", "loc_mean", "loc_cov", "samples"):
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k], c[k]), k                       # the key read on the device is the key
    other = run(NoiseSpec(seed=SEED + 1))
    assert not torch.equal(a["loc_mean"], other["loc_mean"]) and torch.equal(a["pi"], other["pi"])


# ----------------------------------------------------------------------------------------------------------------- 7. variants
def _variant_case(dev, S, n, Kv, Tv, max_t, method="euler", box=60.0, seed=5, uncertain=True, **kw):
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    from trajsde_amd.synth import synth
    cfg = H.our_cfg(Kv, Tv, max_t, uncertain)
    if method == "milstein":
        cfg["decoder"]["kwargs"]["method"] = cfg["encoder"]["kwargs"]["method"] = "milstein"
    model = PredictionModelSDENet(**cfg, init_seed=7).eval().to(dev)
    data = synth(S=S, n=n, L=4, F=Tv, box=box, seed=seed, **kw).to(dev)
    local, glob = _embeddings(model, data)
    return model, data, local, glob


def _compare_with_the_decoder(model, data, local, glob, R):
    from trajsde_amd.runtime import NoiseSpec
    got = model.decoder.sample(data, local, glob, R, noise=NoiseSpec(seed=SEED), return_samples=True)
    ref = _decoder_samples(model, data, local, glob, R)
    errs = [H.maxdiff(got["samples"][s], ref[s]) for s in range(R)]
    assert max(errs) <= 1e-5, errs
    assert float(ref.std(0).max()) > 1e-2                       # the samples differ
    _check_statistics(got, ref, R, 1e-5, "variant")
    return got, ref


def test_milstein(dev):
    model, data, local, glob = _variant_case(dev, 2, 7, K, 20, 2.0, method="milstein")
    assert model.decoder.method == "milstein"
    _compare_with_the_decoder(model, data, local, glob, 17)


def test_bf16_state(case):
    from trajsde_amd import runtime
    assert runtime.set_state_storage("bf16") == "fp32"
    try:
        got, ref = _compare_with_the_decoder(case["model"], case["data"], case["local"], case["glob"], 17)
        assert H.maxdiff(ref[0], case["ref"][0]) > 1e-6         # (y0 really went through bf16)
    finally:
        runtime.set_state_storage("fp32")


def test_uncertain_false_shapes(dev):
    model, data, local, glob = _variant_case(dev, 2, 7, K, T, MAX_T, uncertain=False)
    got, ref = _compare_with_the_decoder(model, data, local, glob, 17)
    N = local.shape[0]
    assert tuple(got["loc"].shape) == tuple(got["loc_mean"].shape) == (K, N, T, 2)
    assert tuple(got["samples"].shape) == (17, K, N, T, 2) and tuple(got["loc_cov"].shape) == (K, N, T, 3)
    assert tuple(got["_loc4"].shape) == (K, N, T, 4)


def test_k20_t50(dev):
    """the stress configuration's K = 20 modes and 51 Euler steps (test_forward_matches_oracle_on_synthetic's last case)"""
    model, data, local, glob = _variant_case(dev, 2, 11, 20, 50, 5.0, box=120.0, seed=111, mixed_source=True)
    _compare_with_the_decoder(model, data, local, glob, 17)


# ----------------------------------------------------------------------------------------------------------------- 8. range guard
def _range_flags(reset=1):
    from trajsde_amd import _lib
    L = _lib.lib()
    torch.cuda.synchronize()
    mask = C.c_uint32(0xFFFFFFFF)
    status = L.trajsde_range_status(int(reset), C.byref(mask), torch.cuda.current_stream().cuda_stream)
    return status, int(mask.value), (L.trajsde_last_error().decode() if status else "")


def test_range_guard_notes_the_state(dev):
    """a drift bias that carries state channel 5 to v over the solve (tests/test_gpu_range_guard.py `dec_state`): 7e4 sets site bit 0
    through the MC entry point, 6e4 leaves the flags clean"""
    import restate
    from trajsde_amd import _lib
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.schedule import decoder_schedule
    fp16x3 = _lib.lib().trajsde_split_products() == 3
    try:
        for v, want in ((7.0e4, 1), (6.0e4, 0)):
            model, cfg = H.build_model(K, T, MAX_T, init_seed=7)
            c = restate.flat_cfg(cfg)
            ds = decoder_schedule(c["future_steps"], c["max_fut_t"], c["min_stepsize"])
            with torch.no_grad():
                dict(model.named_parameters())["decoder.lsde_func.f_func.net.4.bias"][5] = v / float(np.sum(ds.dt.astype(np.float64)))
            model = model.to(dev)
            data = _batch().to(dev)
            local, glob = _embeddings(model, data)
            assert _range_flags(1)[0] in (0, -4)
            assert _range_flags(0)[:2] == (0, 0)
            model.decoder.sample(data, local, glob, 17, noise=NoiseSpec(seed=SEED))
            st, mask, msg = _range_flags(1)
            assert mask == (want if fp16x3 else 0), (v, mask, msg)
            assert st == (-4 if (want and fp16x3) else 0)
    finally:
        _range_flags(1)


# ----------------------------------------------------------------------------------------------------------------- 9. memory contract
@pytest.mark.parametrize("R,with_samples", [(17, True), (17, False), (2, True), (33, False)])
def test_memory_contract(R, with_samples, case):
    """every buffer of the call in a red-zone arena (tests/guarded_memory.py): inputs placed, outputs and the workspace routed, the
    workspace NaN-filled and filled with random bits: guards intact, inputs unchanged, outputs finite and equal across fills"""
    from guarded_memory import GuardedMemory
    from trajsde_amd.runtime import NoiseSpec
    m = case["model"]
    m.decoder._rt.blob()                                        # the weight image is packed outside the arenas
    torch.cuda.synchronize()
    outs = []
    for poison, fill in (("nan", "A"), (20240607, "B")):
        gm = GuardedMemory(poison=poison)
        local, glob = gm.placed(case["local"], fill, "local_embed"), gm.placed(case["glob"], fill, "global_embed")
        with gm:
            out = m.decoder._rt.decoder_forward_mc(case["data"], local, glob, R, noise=NoiseSpec(seed=SEED), return_samples=with_samples)
        torch.cuda.synchronize()
        rep = gm.check()
        assert rep.ok, str(rep)
        keys = ["loc", "pi", "loc_mean", "loc_cov"] + (["samples"] if with_samples else [])
        assert gm.routed >= len(keys) + 1                       # the outputs and the workspace came out of arenas
        for k in keys:
            assert gm.owns(out[k]) and bool(torch.isfinite(out[k]).all()), k
        outs.append({k: out[k].clone() for k in keys})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert H.maxdiff(outs[0]["loc"], case["ref"][0]) <= 1e-5


# ----------------------------------------------------------------------------------------------------------------- 10. model level
@pytest.mark.parametrize("ood", [False, True])
def test_predict_samples_keeps_the_forward(ood, case):
    from trajsde_amd.runtime import NoiseSpec
    m = case["model"]
    dev_ = case["local"].device
    m.ood = ood
    try:
        want = m(H.clone_batch(case["batch"]).to(dev_), noise=NoiseSpec(seed=SEED))
        got = m.predict_samples(H.clone_batch(case["batch"]).to(dev_), 16, noise=NoiseSpec(seed=SEED))
    finally:
        m.ood = False
    for k in ("loc", "pi") + (("stds",) if ood else ("diff_in", "diff_out")):
        assert H.maxdiff(got[k], want[k]) <= 1e-5, k
    assert torch.equal(got["reg_mask"], want["reg_mask"]) and set(want) <= set(got)
    assert "samples" not in got and tuple(got["loc_mean"].shape) == tuple(want["loc"].shape)
    assert bool(torch.isfinite(got["loc_mean"]).all()) and bool((got["loc_cov"][..., :2] > 0).all())


def test_evaluate_with_mc_samples(dev):
    from trajsde_amd import driver
    from trajsde_amd.synth import synth
    cfg = H.our_cfg(K, T, MAX_T)
    for m in cfg["metric_args"]:
        m["end_idcs"] = [T - 1, T - 1]
    model = driver.build_model(cfg, None, dev, init_seed=0)
    batches = [synth(S=2, n=7, L=4, F=T, box=60.0, seed=500 + i) for i in range(2)]
    mc = driver.evaluate(model, [H.clone_batch(b).to(dev) for b in batches], seed=40, mc_samples=4)
    one = driver.evaluate(model, [H.clone_batch(b).to(dev) for b in batches], seed=40)
    assert set(mc) == set(one) and all(np.isfinite(v) for v in mc.values()), mc
    assert any(abs(mc[k] - one[k]) > 1e-9 for k in mc)          # the sample mean was scored, not the single draw
    again = driver.evaluate(model, [H.clone_batch(b).to(dev) for b in batches], seed=40, mc_samples=4)
    assert again == mc
